"""Host-side mirror of ``DeterministicDecoder`` (robot_flamingo/models/action_head.py:408-611) on top of the
engine's head kernels (csrc/head.hip).

Only the inference behaviour DeeR uses is mirrored: max/avg pooling over the text tokens (:519-520), the 4-layer
(LayerNorm-)LSTM evaluated one time step at a time with the ``update_hidden_state`` commit/stash protocol
(:548-558) and the two MLP heads (:604-605).  Window mode - a batch of feature sequences, (bs, L, T, d) or (bs * window_size, T, d)
(:509-518,588-597) - runs the whole sequences in one spine call (DeerEngine.head_sequence, csrc/head_seq.hip).  The weights live in the engine (``DeerEngine.head``); this object is the
stateful handle the reference's harness and ``ActionValueNet`` poke at: ``hidden_state``, ``history_memory``,
``window_size``, ``clear_hidden_state()``, ``update_hidden_state()``, ``__call__(feat, update_hidden_state=...)``.

The fast path never goes through this class (the exit gate runs on the device, see engine.enqueue_head); it exists
so that a FOREIGN exit controller written against the reference protocol keeps working (slow host loop).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _abi as abi


class DeterministicDecoder:
    def __init__(self, engine, window_size: int = 12):
        self.engine = engine
        self.window_size = window_size
        self.history_memory: list = []
        self.tmp_hidden_state = None
        self.last_action = False
        self.is_extra_exit = True

    # ---- state (kept on the device inside the engine) -------------------------------------------------------
    # A window call over bs sequences leaves h_n as the hidden state (action_head.py:592).  bs == n_envs: it becomes the engine's committed
    # LSTM state, so a following step call continues from it; otherwise it is held here (engine._window_hidden) and a step call raises
    # until clear_hidden_state() / engine.reset(), as the reference's LSTM fails on the batch mismatch.
    @property
    def hidden_state(self):
        e = self.engine
        if getattr(e, "_window_hidden", None) is not None:
            return e._window_hidden
        if not bool(e.h_state.any()) and not bool(e.c_state.any()):
            return None
        return (e.h_state.clone(), e.c_state.clone())           # (L, 1, H) like the reference (action_head.py:61-63)

    @hidden_state.setter
    def hidden_state(self, value):
        e = self.engine
        e._window_hidden = None
        if value is not None and value[0].numel() != e.h_state.numel():
            e._window_hidden = (value[0], value[1])
            return
        if value is None:
            e.h_state.zero_()
            e.c_state.zero_()
        else:
            e.h_state.copy_(value[0].reshape(e.h_state.shape))
            e.c_state.copy_(value[1].reshape(e.c_state.shape))
        e._head_state_changed()

    def clear_hidden_state(self) -> None:
        self.hidden_state = None

    def update_hidden_state(self):
        assert self.tmp_hidden_state is not None
        e = self.engine
        e.h_state.copy_(self.tmp_hidden_state[0])
        e.c_state.copy_(self.tmp_hidden_state[1])
        e._head_state_changed()
        self.tmp_hidden_state = None

    # ---- forward ---------------------------------------------------------------------------------------------
    def __call__(self, input_feature: torch.Tensor, h_0=None, state_tensor=None, return_feature=False,
                 return_aggregate_feature=False, with_gripper_logits=False, layer_indices=None,
                 update_hidden_state: bool = True):
        e = self.engine
        if input_feature.dim() != 3 or input_feature.shape[0] != 1:
            return self._window(input_feature, h_0, state_tensor, return_feature, return_aggregate_feature, with_gripper_logits)
        if getattr(e, "_window_hidden", None) is not None:
            raise RuntimeError(f"the hidden state holds {e._window_hidden[0].shape[1]} sequences from a window call, the step mode runs "
                               f"{e.B}: call clear_hidden_state() (or reset the engine) first")
        T = input_feature.shape[1]
        feats = input_feature.reshape(T, -1).to(device=e.dev, dtype=torch.float32).contiguous()
        self.history_memory.append(None)                      # the reference appends the pooled feature (unbounded leak)
        e.enqueue_head(0, T, abi.KIND_COMMIT, use_ctl=False, feats=feats, no_ctl_final=True)
        torch.cuda.current_stream().synchronize()
        a = e.action_dbg[0].clone()
        if update_hidden_state:
            e.h_state.copy_(e.h_tmp)
            e.c_state.copy_(e.c_tmp)
            e._head_state_changed()
        else:
            self.tmp_hidden_state = (e.h_tmp.clone(), e.c_tmp.clone())
        A = e.A                                              # multi_step_action: 6 A pose + A gripper outputs (action_head.py:472-473)
        pose = a[:6 * A].view(1, 1, 6 * A)
        grip = a[6 * A:7 * A].view(1, 1, A)
        if with_gripper_logits:
            return pose, (grip, a[7 * A:8 * A].view(1, 1, A))
        if return_feature:                                    # the pooled token feature (action_head.py:519-520: max or mean over the tokens)
            pooled = feats.amax(0, keepdim=True) if e.cfg.pooling == "max" else feats.mean(0, keepdim=True)
            return pose, grip, pooled
        return pose, grip

    def _window(self, input_feature, h_0, state_tensor, return_feature, return_aggregate_feature, with_gripper_logits):
        """Window mode (action_head.py:509-518 reshape rules, :588-597): the LSTM runs along each sequence from h_0 or zero."""
        e = self.engine
        x = input_feature
        if x.dim() == 4:                                     # (bs, L, T, d): the window size of this call
            cur_ws = int(x.shape[1])
            x = x.reshape(-1, *x.shape[2:])
        else:                                                # (bs * window_size, T, d)
            cur_ws = int(self.window_size)
        if x.dim() != 3:
            raise ValueError(f"DeterministicDecoder: input must be (1, T, d), (bs, L, T, d) or (bs * window_size, T, d), got {tuple(input_feature.shape)}")
        rows, T, d = (int(v) for v in x.shape)
        if cur_ws < 1 or rows % cur_ws:
            raise ValueError(f"DeterministicDecoder: {rows} feature rows are not whole windows of window_size {cur_ws}")
        N = rows // cur_ws
        if cur_ws == 1:                                      # one step per sequence: the reference's step mode (:548)
            if N == 1:
                return self(x, h_0, state_tensor, return_feature, return_aggregate_feature, with_gripper_logits)
            raise NotImplementedError(f"native head: step mode runs one sequence per call here ({N} given with window size 1)")
        h0 = c0 = None
        if h_0 is not None:                                  # nn.LSTM's (h_0, c_0)
            h0, c0 = h_0
        st = None
        if getattr(e.cfg, "use_state", False):
            if state_tensor is None:
                raise ValueError("a use_state head needs state_tensor (bs, L, 15) or (bs * L, 15) in window mode (action_head.py:524-536)")
            st = state_tensor
        from .ops import head_sequence_shapes
        head_sequence_shapes(e.cfg, (N, cur_ws, T, d), h0, c0, st, self.last_action)   # every shape checked before the device is touched
        feats = x.reshape(N, cur_ws, T, d)
        actions, h_n, c_n, org_feat, agg = e.head_sequence(feats, h0, c0, st, head=getattr(self, "head", 0), last_action=self.last_action,
                                                           features=True)
        self.hidden_state = (h_n, c_n)                       # :592 (the engine's committed state when bs == n_envs)
        A = e.A
        pose = actions[..., :6 * A]
        grip = actions[..., 6 * A:7 * A]
        gripper = (grip, actions[..., 7 * A:8 * A]) if with_gripper_logits else grip
        if return_aggregate_feature:
            return pose, gripper, agg
        if return_feature:
            if org_feat.shape[1] == 1:                       # :539-543
                org_feat = org_feat.view(cur_ws, org_feat.shape[-1])
            return pose, gripper, org_feat
        return pose, gripper
