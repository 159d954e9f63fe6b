"""Exit-only fine-tuning on the device: the reference's second training stage - ``only_train_head`` / ``no_backbone_grad=True``
(robot_flamingo/train/train_utils.py:487-543) with ``exit_optimizer = AdamW(get_grouped_params(only_head=True))``
(train_calvin_post_strategy.py:466-535) - which trains ``lm_head``, ``lm_exit_modules.*`` and ``extra_exit`` on a frozen trunk.  With the
trunk frozen the heads read nothing but the pooled (bs, W, NE, d) exit-layer features ``DeerEngine.window_exit_pooled`` leaves on the
GPU, so the loop closes here: features, per-exit loss, gradient, update, ``commit()``, then ``exit_losses_on_windows`` / thresholds /
rollouts on the same engine.

``HeadTrainer`` keeps its own f32 parameters, gradients and Adam moments per head as flat device buffers OUTSIDE the engine's weight
arena (laid out by the spine's table, ``deer_head_param_entry``); the engine computes what it computed before until ``commit()``.

Deviations from the reference's training step, on purpose and stated:
  * no dropout (the reference trains with ``policy_rnn_dropout_p`` and MLP dropout): the forward is the evaluation forward
  * no fp16 autocast / GradScaler: f32 arithmetic throughout
  * no LR scheduler: ``lr`` is a plain attribute the caller may change between steps
  * no DDP gradient all-reduce: one process trains
  * weight decay (``exit_decay=True``) reaches Linear / LSTM weights only - the reference's ``apply_decay`` tests the substrings "norm" and
    "bias", which the head's LayerNorm weights ("rnn.layers.1.weight", "actions.mlp.2.weight") do not carry, so it would decay those too
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import torch

from . import _abi as abi
from .ops import MAX_GRAD_ROWS, exit_head_count, exit_outputs_shapes, head_param_table, run_adamw_step, run_head_loss_grad


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Head:
    """flat buffers of one trained head"""

    def __init__(self, lib, handle, head: int, sd: Dict[str, torch.Tensor], dev):
        self.index = head
        self.table, self.total = head_param_table(lib, handle, head)
        self.params = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.shapes = {}
        for name, off, numel, _ in self.table:
            if name not in sd:
                raise KeyError(f"HeadTrainer: the state dict lacks {name}")
            t = sd[name]
            if t.numel() != numel:
                raise ValueError(f"HeadTrainer: {name} has {t.numel()} values, the head's table says {numel}")
            self.shapes[name] = tuple(t.shape)
            self.params[off:off + numel].copy_(t.detach().reshape(-1).to(device=dev, dtype=torch.float32))
        self.grad = torch.zeros_like(self.params)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        # segments of the AdamW launch: every tensor with its padding up to the next one
        ends = [off for _, off, _, _ in self.table[1:]] + [self.total]
        self.seg_end = torch.tensor(ends, dtype=torch.int32, device=dev)
        self.seg_decay = torch.tensor([1 if dec else 0 for _, _, _, dec in self.table], dtype=torch.int32, device=dev)


class HeadTrainer:
    """Trains exit heads of ``engine``'s model on pooled exit-layer features with the trunk frozen.

    heads: indices in the spine's numbering (0 = extra_exit, k >= 1 = per-layer head k: lm_exit_modules.(k-1), the last one lm_head);
    default every head of ``all_outputs`` - the per-layer heads of a layerwise_exit_eval model and extra_exit.  lr / weight_decay /
    betas / eps: torch.optim.AdamW's; weight_decay only acts with exit_decay=True (the reference's ``--exit_decay``)."""

    def __init__(self, engine, state_dict: Dict[str, torch.Tensor], heads: Optional[Sequence[int]] = None, lr: float = 1e-4,
                 weight_decay: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8, exit_decay: bool = False):
        cfg = engine.cfg
        if getattr(cfg, "use_state", False):
            raise NotImplementedError("HeadTrainer: a use_state head would need gradients for its state embeddings (embed_arm_state, "
                                      "embed_gripper_state, embed_state); they are not built")
        self.engine, self.cfg, self.lib, self.dev = engine, cfg, engine.lib, engine.dev
        self.n_layer_heads = exit_head_count(cfg) - 3                        # heads of the internal exits (layerwise_exit_eval)
        self.final_head = self.n_layer_heads + 1 if getattr(cfg, "layerwise_exit_eval", False) else 0
        every = list(range(1, self.final_head + 1)) + [0] if self.final_head else [0]
        heads = every if heads is None else [int(h) for h in heads]
        if not heads or len(set(heads)) != len(heads) or any(h not in every for h in heads):
            raise ValueError(f"HeadTrainer: heads {heads} for a model whose heads are {every}")
        self.heads: Dict[int, _Head] = {h: _Head(self.lib, engine._h, h, state_dict, self.dev) for h in heads}
        self.lr, self.weight_decay, self.betas, self.eps, self.exit_decay = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps), bool(exit_decay)
        self.steps = 0
        exits = [int(e) for e in cfg.exit_ids()]
        slots = [-1] * cfg.n_layers
        for k, layer in enumerate(exits):
            slots[layer] = k
        self._slots = (ctypes.c_int * cfg.n_layers)(*slots)

    # ------------------------------------------------------------------------------------------------------------------
    def _run(self, head: int, X: torch.Tensor, pose: torch.Tensor, grip: torch.Tensor, w_bin: float, weight: float) -> torch.Tensor:
        """one head on (bs, W, d) rows, chunked into whole windows of at most MAX_GRAD_ROWS rows: the gradient accumulates, the loss is
        the row-weighted mean of the chunks' losses (a device scalar)"""
        H = self.heads[head]
        bs, W = X.shape[:2]
        if W > MAX_GRAD_ROWS:
            raise ValueError(f"HeadTrainer: windows of {W} steps; one gradient call takes at most {MAX_GRAD_ROWS} rows")
        nc = max(1, MAX_GRAD_ROWS // W)
        total = None
        for b0 in range(0, bs, nc):
            b1 = min(bs, b0 + nc)
            share = (b1 - b0) / bs
            loss = run_head_loss_grad(self.lib, self.engine._h, self.cfg, head, H.params, X[b0:b1], pose[b0:b1], grip[b0:b1], w_bin, weight * share,
                                      H.grad, True)
            total = loss * share if total is None else total + loss * share
        return total.reshape(())

    def loss_and_grads(self, P: torch.Tensor, rand_layers, two_layers, pose, grip01, w_bin: float = 0.01,
                       weights: Optional[Sequence[float]] = None) -> torch.Tensor:
        """P (bs, W, NE, d) pooled exit-layer features (``window_exit_pooled``), rand_layers / two_layers (bs, W) the exit layer of every
        step under sampling strategy 1 / 2, pose (bs, W, 6 A), grip01 (bs, W, A): the gradients of sum_h weights[h] loss[h]
        (train_utils.py:541-543) are ADDED to the trainer's (``zero_grad`` clears them).  Per-layer head k runs on P[:, :, k]; extra_exit
        runs on the strategy-1 and the strategy-2 gather, its gradient is the sum.  Returns the (Hn,) unweighted losses in
        ``exit_outputs``' order on the device (NaN for a head this trainer does not hold); no host synchronisation."""
        rl, tl = torch.as_tensor(rand_layers), torch.as_tensor(two_layers)
        P = P.to(device=self.dev, dtype=torch.float32).contiguous()
        bs, W, NE, Hn, A = exit_outputs_shapes(self.cfg, P.shape, rl, tl)
        w = [1.0] * Hn if weights is None else [float(v) for v in weights]
        if len(w) != Hn:
            raise ValueError(f"{len(w)} exit weights for {Hn} heads")
        pose = torch.as_tensor(pose).to(device=self.dev, dtype=torch.float32).reshape(bs, W, 6 * A).contiguous()
        grip = torch.as_tensor(grip01).to(device=self.dev, dtype=torch.float32).reshape(bs, W, A).contiguous()
        losses: List[torch.Tensor] = []
        nan = torch.full((), float("nan"), device=self.dev)
        for k in range(self.n_layer_heads):
            losses.append(self._run(k + 1, P[:, :, k].contiguous(), pose, grip, w_bin, w[k]) if k + 1 in self.heads else nan)
        h = self.n_layer_heads
        losses.append(self._run(self.final_head, P[:, :, NE - 1].contiguous(), pose, grip, w_bin, w[h]) if self.final_head in self.heads else nan)
        if 0 in self.heads:
            sel = torch.stack([rl.to(device=self.dev, dtype=torch.int32), tl.to(device=self.dev, dtype=torch.int32)]).contiguous()
            XS = torch.empty(2, bs, W, self.cfg.d_model, dtype=torch.float32, device=self.dev)
            abi.check(self.lib.deer_window_gather_layers(abi.ptr(P), abi.ptr(sel), self._slots, self.cfg.n_layers, abi.ptr(XS), 2, bs, W, NE,
                                                         self.cfg.d_model, _stream()), "deer_window_gather_layers")
            for s in range(2):
                losses.append(self._run(0, XS[s], pose, grip, w_bin, w[h + 1 + s]))
        else:
            losses += [nan, nan]
        return torch.stack(losses)

    def zero_grad(self):
        for H in self.heads.values():
            H.grad.zero_()

    def step(self):
        """One AdamW update of every trained head (one launch per head)."""
        self.steps += 1
        wd = self.weight_decay if self.exit_decay else 0.0
        for H in self.heads.values():
            run_adamw_step(self.lib, H.params, H.grad, H.m, H.v, H.seg_end, H.seg_decay, self.lr, self.betas[0], self.betas[1], self.eps, wd, self.steps)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The trained tensors under the reference's names (f32 copies on the device)."""
        out = {}
        for H in self.heads.values():
            for name, off, numel, _ in H.table:
                out[name] = H.params[off:off + numel].view(H.shapes[name]).clone()
        return out

    def grads(self) -> Dict[str, torch.Tensor]:
        """The accumulated gradients under the reference's names (views of the flat buffers)."""
        return {name: H.grad[off:off + numel].view(H.shapes[name]) for H in self.heads.values() for name, off, numel, _ in H.table}

    def commit(self):
        """Re-ingests the trained tensors into the engine's weight arena (``deer_model_load_tensor``: rounded once to the engine's operand
        format).  Engines that share the arena (siblings, the owner) see them at their next step; captured graphs read the arena at
        replay, so nothing is recaptured."""
        self.engine.reload_tensors(self.state_dict())
