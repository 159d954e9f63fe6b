"""Per-exit demonstration loss: how good every exit head of a checkpoint is on recorded demonstration windows, without a simulator or a
rollout - the forward half of the reference's multi-exit training step (robot_flamingo/train/train_utils.py:466-543) in ``eval()``: no
gradient, no optimizer, no dropout.

One batch is what the reference's CALVIN loader yields, by name:
  images, gripper   (bs, W, 3, S, S) camera frames of bs windows of W = model.window_size steps
  input_ids         (bs, T) one right-padded instruction per window (or (bs, W, T)); attention_mask the same shape, or absent
  labels            (bs, W, 7) relative actions = 6 pose values + the gripper command in {-1, 1}; (bs, W, A, 7) with multi_step_action = A
  state             (bs, W, 15) robot_obs rows (use_state models only)
The frames go through ``MPTFlamingo.all_exit_actions`` (one static full-depth pass + ``DeerEngine.exit_outputs``), the losses through
``DeerEngine.exit_losses``; the per-head sums stay on the device until the end.

``finetune_exit_heads`` is the other half of that step for a frozen trunk (``only_train_head``): the same features, then gradient and
AdamW on the device (``finetune.HeadTrainer``).

``on_policy_values`` is the other evaluation without labels: the exit values of a live rollout (shadow steps logged on the device), the
input of ``value_net.calibrate_on_policy``.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence

import torch

from .distributed import reduce_exit_losses


def split_labels(labels: torch.Tensor, multi_step_action: int = 1):
    """train_utils.py:485 (+ the multi_step_action reshape of :468,510-514): labels (bs, W, 7) or (bs, W, A, 7) / (bs, W, A * 7) ->
    (pose (bs, W, 6 A), grip01 (bs, W, A)): ``labels[..., :6]`` and the gripper command -1 / 1 as the BCE target ``(labels[..., 6:] + 1) // 2``."""
    A = max(1, int(multi_step_action))
    if labels.dim() < 3:
        raise ValueError(f"labels must be (bs, W, 7) or (bs, W, A, 7), got {tuple(labels.shape)}")
    bs, W = labels.shape[:2]
    if labels[0, 0].numel() != 7 * A:
        raise ValueError(f"labels {tuple(labels.shape)} do not hold 7 values for each of the {A} actions of a step")
    lab = labels.reshape(bs, W, A, 7)
    pose, grip = lab[..., :6], (lab[..., 6:] + 1) // 2
    return pose.reshape(bs, W, 6 * A), grip.reshape(bs, W, A)


def window_batch_inputs(batch: Dict[str, torch.Tensor], window_size: int):
    """The harness's reshaping of one loader batch (train_utils.py:470-478): batch and sequence dimension merged, one instruction row per
    frame -> the keywords of ``MPTFlamingo.all_exit_actions``."""
    images, gripper = batch["images"], batch["gripper"]
    bs, W = images.shape[:2]
    if W != window_size:
        raise ValueError(f"windows of {W} steps for a model with window_size {window_size}")
    ids = batch["input_ids"]
    mask = batch.get("attention_mask")

    def per_frame(t):
        if t is None:
            return None
        t = t.unsqueeze(1).repeat(1, W, 1) if t.dim() == 2 else t
        return t.flatten(0, 1)
    state = batch.get("state")
    return dict(vision_x=images.unsqueeze(2).unsqueeze(2).flatten(0, 1), vision_gripper=gripper.unsqueeze(2).unsqueeze(2).flatten(0, 1),
                lang_x=per_frame(ids), attention_mask=per_frame(mask),
                state_tensor=state.unsqueeze(2).unsqueeze(2).flatten(0, 1) if state is not None else None)


def exit_losses_on_windows(model, batches: Iterable[Dict[str, torch.Tensor]], w_bin: float = 0.01, generator: Optional[torch.Generator] = None,
                           weights: Optional[Sequence[float]] = None, device=None) -> Dict[str, object]:
    """Per-head means of num (Huber, delta = 1), bin (BCE with logits) and loss = num + w_bin bin (train_utils.py:519-540; w_bin 0.01, or
    0.05 for real data) over every (window, step) row of ``batches``, heads in the reference's ``all_outputs`` order (:503): per-layer
    heads, the last layer's head, extra_exit on sampling strategy 1, extra_exit on strategy 2.  ``total`` is the reference's weighted sum
    of the per-head losses (get_exit_weights, :179-181,541-543: all ones unless ``weights`` is given).  The layer tables of the two
    strategies are drawn per batch like the reference's (``generator`` seeds the torch draws).  With torch.distributed initialised the
    per-head (sum, count) pairs of all ranks are summed by one all-reduce."""
    e = model.engine
    A = e.A
    sums, count = None, 0
    for batch in batches:
        pose, grip01 = split_labels(batch["labels"], A)
        acts = model.all_exit_actions(generator=generator, **window_batch_inputs(batch, model.window_size))[0]     # (Hn, bs, W, 8 A)
        num, bin_, loss = e.exit_losses(acts, pose, grip01, w_bin)
        R = num.shape[1]
        s = torch.stack([num.sum(1, dtype=torch.float64), bin_.sum(1, dtype=torch.float64), loss.to(torch.float64) * R])    # stays on the device
        sums = s if sums is None else sums + s
        count += R
    if sums is None:
        raise ValueError("exit_losses_on_windows: no batches")
    sums, count = reduce_exit_losses(sums, count, device)
    means = sums / max(count, 1)
    Hn = means.shape[1]
    w = torch.ones(Hn, dtype=torch.float64) if weights is None else torch.as_tensor(list(weights), dtype=torch.float64)
    if w.numel() != Hn:
        raise ValueError(f"{w.numel()} exit weights for {Hn} heads")
    n_layer_heads = Hn - 3
    names = [f"exit{k}" for k in range(n_layer_heads)] + ["final", "extra", "extra2"]
    return {"heads": names, "num": means[0].tolist(), "bin": means[1].tolist(), "loss": means[2].tolist(),
            "total": float((means[2] * w).sum()), "rows": count, "w_bin": float(w_bin)}


def finetune_exit_heads(model, batches: Iterable[Dict[str, torch.Tensor]], steps: int, state_dict: Dict[str, torch.Tensor], lr: float = 1e-4,
                        w_bin: float = 0.01, generator: Optional[torch.Generator] = None, weights: Optional[Sequence[float]] = None,
                        commit: bool = True, **trainer_kw):
    """Exit-only fine-tuning on demonstration windows: the reference's second stage (train_utils.py:487-543 with only_train_head /
    no_backbone_grad, AdamW over the heads alone, train_calvin_post_strategy.py:466-535) with the trunk frozen.  The pooled exit-layer
    features of every batch are computed ONCE (``window_exit_pooled``; the trunk never changes), then ``steps`` optimizer steps cycle
    over the batches: layer tables drawn per step like ``exit_losses_on_windows`` draws them, ``HeadTrainer.loss_and_grads``, ``step``.
    ``state_dict`` holds the heads' current tensors (the checkpoint the model was built from); trainer_kw: ``finetune.HeadTrainer``'s
    (heads, weight_decay, betas, eps, exit_decay).  Returns (trainer, losses (steps, Hn) on the device); commit=True re-ingests the trained
    heads into the model's engine at the end."""
    e = model.engine
    A, Wn = e.A, model.window_size
    feats = []
    for batch in batches:
        pose, grip01 = split_labels(batch["labels"], A)
        kw = window_batch_inputs(batch, Wn)
        bs, rgb, grip_f, ids, mask, _ = model._window_inputs(kw["vision_x"], kw["lang_x"], kw["attention_mask"], kw["vision_gripper"], kw["state_tensor"])
        pooled = e.window_exit_pooled(rgb, grip_f, ids, mask)
        feats.append((pooled.view(bs, Wn, pooled.shape[1], pooled.shape[2]).clone(), pose.to(e.dev), grip01.to(e.dev)))
    if not feats:
        raise ValueError("finetune_exit_heads: no batches")
    trainer = e.head_trainer(state_dict, lr=lr, **trainer_kw)
    history = []
    for k in range(int(steps)):
        P, pose, grip01 = feats[k % len(feats)]
        rl, tl = model.draw_exit_layers(P.shape[0], Wn, generator)
        trainer.zero_grad()
        history.append(trainer.loss_and_grads(P, rl, tl, pose, grip01, w_bin=w_bin, weights=weights))
        trainer.step()
    if commit:
        trainer.commit()
    return trainer, (torch.stack(history) if history else torch.empty(0, device=e.dev))


def on_policy_values(wrapper, envs, eval_sequences, annotations, task_checker, controller, n_samples: int, ep_len: Optional[int] = None):
    """Exit values ON POLICY: the batched rollout loop (``rollout.evaluate_policy_batched``) on ``envs`` under ``controller``'s
    thresholds, every step a SHADOW step - all exits evaluated, every environment's LSTM history committed at the exit its criterion
    takes, as in a normal rollout - whose deltas and exit layers are appended to a value log on the device (``DeerEngine.log_values``,
    csrc/value_log.hip) until ``n_samples`` columns are there; the chains are run again from the start while the log is short.  The
    host reads three words per pass over the chains and the (n_samples,) exit layers at the end; the matrix never leaves the device.
    Returns (values (real_num_exit, n_samples) f32 on the device - what ``DeerEngine.solve_thresholds`` / ``solve_for_budget(engine=...)``
    take, taken (n_samples,) i32 exit layers on the device, (fractions, average exit layer) measured from taken -
    ``value_net.measured_exit_mix``).  This rank's chains only.  wrapper: a ``rollout.BatchedModelWrapper``; controller: a native
    ``ExitController`` with its thresholds set and ``steps_per_stage`` = 1 (a held step evaluates no exit: its deltas are NaN, which
    raises ValueError here like any other non-finite delta)."""
    from .rollout import EP_LEN, evaluate_policy_batched
    from .value_net import measured_exit_mix
    n_samples = int(n_samples)
    if n_samples < 1:
        raise ValueError(f"on_policy_values: n_samples must be positive, got {n_samples}")
    ctl = getattr(controller, "module", controller)
    m = wrapper.model.module
    e = m.engine
    m._sync_controller(ctl)                                  # the log is sized for this controller's reachable exits
    prev_ctl, wrapper.exit_controller = wrapper.exit_controller, ctl
    e.open_value_log(n_samples)
    try:
        count = 0
        while count < n_samples:
            evaluate_policy_batched(wrapper, envs, eval_sequences, annotations, task_checker, ep_len=EP_LEN if ep_len is None else ep_len,
                                    log_values=n_samples - count)
            values, taken, _, nonfinite = e.logged_values()
            if values.shape[1] == count:
                raise ValueError("on_policy_values: a pass over the evaluation chains logged no step")
            count = values.shape[1]
        if nonfinite:
            raise ValueError(f"on_policy_values: {nonfinite} non-finite deltas among the logged exit values")
    finally:
        e.close_value_log()
        wrapper.exit_controller = prev_ctl
    return values, taken, measured_exit_mix(taken, ctl.exit_id_list[: ctl.real_num_exit])
