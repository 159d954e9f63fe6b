"""PyTorch custom operators over the native spine (``torch.ops.deer.*``; BASELINE north_star: "host code stays Python calling HIP
through PyTorch-ROCm custom ops").  These are the three coarse operators SURVEY.md §8b specifies; each is one call into
``libdeer_hip.so`` (include/deer_model.h) on the CURRENT PyTorch HIP stream, so they compose with torch streams / graphs:

  deer::vit_l14_encode(Tensor images, int model) -> Tensor tokens              open_clip ``visual(x)[1]`` (flamingo_mpt.py:556-583)
  deer::perceiver_resample(Tensor tokens, int model) -> Tensor media           PerceiverResampler.forward (helpers.py:107-132)
  deer::llm_early_exit(Tensor ids, Tensor? key_mask, Tensor media, int model, int exit_id, bool shadow)
                                        -> (Tensor ctl, Tensor hidden)        mosaic_gpt_3b.py:274-449 + value_net.py:277-297
                                                                               + action_head.py:499-611 (exit gate on the device)
  deer::action_head_sequence(Tensor feats, Tensor? h0, Tensor? c0, int model, int head, bool last_action, Tensor? state=None)
                                        -> (Tensor actions, Tensor h_n, Tensor c_n) DeterministicDecoder.forward on sequences
                                                                               (action_head.py:499-611, window mode :588-595)
  deer::calibrate_values(Tensor feats, Tensor rand_layers, int model, str threshold_type) -> Tensor values
                                                                               ActionValueNet.forward(mode='generate')
                                                                               (value_net.py:134-160) on pooled exit-layer features
  deer::solve_thresholds(Tensor values, Tensor counts, bool leq) -> (Tensor thresholds, Tensor exit_counts, Tensor status)
                                                                               the solver of ExitController.set_threshold
                                                                               (value_net.py:242-262), k operating points per launch;
                                                                               model-free (no ``model`` argument)
  deer::value_log_append(Tensor ctl, int n_envs, int n_exit, int active_mask, Tensor(a!) values, int capacity, Tensor(b!) taken,
                         Tensor(c!) state) -> ()                               the deltas a shadow step left in the control blocks
                                                                               (value_net.py:120-133), one column per environment of
                                                                               active_mask, appended to a device value matrix; model-free

  deer::head_loss_grad(Tensor params, Tensor feats, Tensor pose, Tensor grip01, int model, int head, float w_bin, float scale,
                       Tensor(a!) grad, bool accumulate) -> Tensor loss        one head's loss and parameter gradients with a frozen
                                                                               trunk (train_utils.py:487-543, only_train_head) from a flat
                                                                               f32 parameter buffer; taped forward + backward on the device
  deer::adamw_step(Tensor(a!) param, Tensor grad, Tensor(b!) m, Tensor(c!) v, Tensor seg_end, Tensor seg_decay, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step) -> () torch.optim.AdamW over flat buffers
                                                                               (train_calvin_post_strategy.py:535); model-free

``model`` is the address of a ``deer_model`` (``NativeModel.handle``): weights, workspace, LSTM state and the exit controller
configuration live in that object, like they live in the reference's stateful ``MPTFlamingo`` module.
There is no CPU implementation: the ops raise without a HIP device / without the library.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _abi as abi

_MODELS: Dict[int, "NativeModel"] = {}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class NativeModel:
    """Owner of one ``deer_model``: creates it from a DeerConfig, allocates the weight arena + workspace as torch tensors and
    ingests a reference state dict.  No orchestration here - that is the spine's; ``DeerEngine`` adds graph scheduling on top."""

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], device="cuda", n_envs: int = 1, max_text_len: int = 32,
                 precision: Optional[str] = None):
        if not torch.cuda.is_available():
            raise abi.DeerHipError("deer_vla_amd needs a HIP device (no CPU fallback)")
        self.lib = abi.lib()
        self.cfg, self.B = cfg, n_envs
        self.dev = torch.device(device)
        precision = abi.resolve_precision(precision)        # "fp16" (default) / "bf16": product arithmetic on fp16 / bf16 operands; "fp32": parity arithmetic
        self.max_T = min(max_text_len, abi.max_trunk_rows(cfg, precision) // n_envs)   # the same row budget as DeerEngine (512 rows in the product arithmetic)
        self._h = ctypes.c_void_p()
        self.precision = precision
        # format of the camera frames / media tokens the operators hand around
        self.img_dtype = abi.torch_dtype16(precision)
        self.media_dtype = torch.float16 if precision == "fp16" else torch.bfloat16
        cc = abi.config_to_c(cfg, n_envs, self.max_T, precision=precision)
        abi.check(self.lib.deer_model_create(ctypes.byref(cc), ctypes.byref(self._h)), "deer_model_create")
        with torch.cuda.device(self.dev):
            self.arena = torch.zeros(self.lib.deer_model_arena_bytes(self._h), dtype=torch.uint8, device=self.dev)
            self.workspace = torch.zeros(self.lib.deer_model_workspace_bytes(self._h), dtype=torch.uint8, device=self.dev)
            abi.check(self.lib.deer_model_bind(self._h, abi.ptr(self.arena), abi.ptr(self.workspace)), "deer_model_bind")
            for name, t in state_dict.items():
                if not self.lib.deer_model_knows_tensor(self._h, name.encode()):
                    continue
                is_bf = t.dtype == torch.bfloat16
                src = t.detach().to(device=self.dev, dtype=torch.bfloat16 if is_bf else torch.float32).contiguous()
                abi.check(self.lib.deer_model_load_tensor(self._h, name.encode(), abi.ptr(src), 1 if is_bf else 0, src.numel(), _stream()),
                          f"deer_model_load_tensor({name})")
                torch.cuda.current_stream().synchronize()
        buf = ctypes.create_string_buffer(4096)
        n = self.lib.deer_model_missing_tensors(self._h, buf, len(buf))
        if n:
            raise abi.DeerHipError(f"{n} required parameters missing, e.g. {buf.value.decode().split()[:4]}")
        self.buffer("thresholds").view(torch.float32).fill_(1e8)
        self.exit_ids = list(cfg.exit_ids())                # the model's default exits until configure_exit
        _MODELS[self.handle] = self

    @property
    def handle(self) -> int:
        return int(self._h.value)

    def buffer(self, name: str) -> torch.Tensor:
        off, nbytes = ctypes.c_long(), ctypes.c_long()
        abi.check(self.lib.deer_model_buffer(self._h, 1, name.encode(), ctypes.byref(off), ctypes.byref(nbytes)), f"buffer {name}")
        return self.workspace[off.value: off.value + nbytes.value]

    def configure_exit(self, exit_ids: Sequence[int], max_layer: int, thresholds: Optional[Sequence[float]] = None,
                       threshold_type: str = "L2", leq: bool = True):
        ids = (ctypes.c_int * len(exit_ids))(*exit_ids)
        abi.check(self.lib.deer_model_configure_exit(self._h, ids, len(exit_ids), max_layer, abi.THR_TYPES[threshold_type], 1 if leq else 0),
                  "deer_model_configure_exit")
        self.exit_ids = list(exit_ids)
        if thresholds is not None:
            t = torch.full((16,), 1e8, dtype=torch.float32)
            t[: len(thresholds)] = torch.tensor([float(v) for v in thresholds])
            self.buffer("thresholds").view(torch.float32).copy_(t)

    def reset(self):
        for n in ("h_state", "c_state", "ctl"):
            self.buffer(n).zero_()

    def close(self):
        if self._h.value:
            _MODELS.pop(self.handle, None)
            torch.cuda.synchronize(self.dev)
            self.lib.deer_model_destroy(self._h)
            self._h = ctypes.c_void_p()


def _model(handle: int) -> NativeModel:
    m = _MODELS.get(int(handle))
    if m is None:
        raise abi.DeerHipError(f"deer op called with an unknown model handle {handle:#x}")
    return m


@torch.library.custom_op("deer::vit_l14_encode", mutates_args=(), device_types="cuda")
def vit_l14_encode(images: torch.Tensor, model: int) -> torch.Tensor:
    """images (N,3,S,S) CLIP-normalised (any float dtype; converted to the tower's format) -> patch tokens (N,256,W) f32 (x[:,1:], no ln_post)."""
    m = _model(model)
    cfg = m.cfg
    img = images.to(m.img_dtype).contiguous()
    out = torch.empty(img.shape[0], cfg.n_patches, cfg.vit_width, dtype=torch.float32, device=img.device)
    abi.check(m.lib.deer_vit_l14_encode(m._h, abi.ptr(img), img.shape[0], abi.ptr(out), _stream()), "deer_vit_l14_encode")
    return out


@vit_l14_encode.register_fake
def _(images, model):
    m = _model(model)
    return images.new_empty((images.shape[0], m.cfg.n_patches, m.cfg.vit_width), dtype=torch.float32)


@torch.library.custom_op("deer::perceiver_resample", mutates_args=(), device_types="cuda")
def perceiver_resample(tokens: torch.Tensor, model: int) -> torch.Tensor:
    """patch tokens (N,256,W) f32 -> media tokens (N*64, W) in the tower's 16-bit format (fp16 / bf16), frame order (rgb, gripper per environment);
    (N/2*64, W) with fusion_mode="pre" (one set of latents per environment)."""
    m = _model(model)
    cfg = m.cfg
    tok = tokens.to(torch.float32).contiguous()
    out = torch.empty(tok.shape[0] // 2 * cfg.n_media, cfg.vit_width, dtype=m.media_dtype, device=tok.device)
    abi.check(m.lib.deer_perceiver_resample(m._h, abi.ptr(tok), tok.shape[0], abi.ptr(out), None, _stream()), "deer_perceiver_resample")
    return out


@perceiver_resample.register_fake
def _(tokens, model):
    m = _model(model)
    return tokens.new_empty((tokens.shape[0] // 2 * m.cfg.n_media, m.cfg.vit_width), dtype=m.media_dtype)


@torch.library.custom_op("deer::llm_early_exit", mutates_args=(), device_types="cuda")
def llm_early_exit(ids: torch.Tensor, key_mask: Optional[torch.Tensor], media: torch.Tensor, model: int, exit_id: int,
                   shadow: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """ids (n_envs,T) int64, key_mask (n_envs,T) or None, media (n_envs*128, W) in the tower's 16-bit format; exit_id >= 0 static, < 0 dynamic (the
    model's configured controller).  Returns (ctl int32 [n_envs,64]: exit layer, action, deltas - include/deer_hip.h -,
    hidden f32 [n_layers, n_envs*T, d]); the LSTM state of the head is carried inside the model."""
    m = _model(model)
    cfg = m.cfg
    ids_c = ids.to(torch.int64).contiguous()
    T = ids_c.reshape(m.B, -1).shape[1]
    km = key_mask.to(torch.uint8).contiguous() if key_mask is not None else None
    # fp32-activation models keep their media tokens in f32 inside the model (the bf16 tensor handed around is only a view of them)
    med = None if m.precision == "fp32" else media.to(m.media_dtype).contiguous()
    abi.check(m.lib.deer_llm_early_exit(m._h, abi.ptr(ids_c), abi.ptr(km), T, abi.ptr(med), exit_id, 1 if shadow else 0, None, None, _stream()),
              "deer_llm_early_exit")
    rows = min(m.B * m.max_T, abi.max_trunk_rows(cfg, m.precision))
    ctl = m.buffer("ctl").view(torch.int32).view(m.B, abi.CTL_WORDS).clone()
    hidden = m.buffer("hidden").view(torch.float32).view(cfg.n_layers, rows, cfg.d_model)[:, : m.B * T].clone()
    return ctl, hidden


@llm_early_exit.register_fake
def _(ids, key_mask, media, model, exit_id, shadow):
    m = _model(model)
    T = ids.reshape(m.B, -1).shape[1]
    return (ids.new_empty((m.B, abi.CTL_WORDS), dtype=torch.int32),
            media.new_empty((m.cfg.n_layers, m.B * T, m.cfg.d_model), dtype=torch.float32))


def head_sequence_shapes(cfg, feats_shape, h0=None, c0=None, state=None, last_action: bool = False):
    """Host-side checks of a window-mode head call (no device touched): feats (N, L, T, d), h0 / c0 (L_lstm, N, H) or None, state
    (N, L, S) / (N * L, S) robot_obs rows (use_state models only).  Returns (N, L, T, shapes of actions, h_n / c_n)."""
    if len(feats_shape) != 4:
        raise ValueError(f"head sequence: feats must be (N, L, T, d), got {tuple(feats_shape)}")
    N, L, T, d = (int(v) for v in feats_shape)
    if min(N, L, T) < 1 or d != cfg.d_model:
        raise ValueError(f"head sequence: feats (N, L, T, d) = {tuple(feats_shape)} for d_model {cfg.d_model}")
    Lh, H, A = cfg.lstm_num_layers, cfg.head_hidden, max(1, int(getattr(cfg, "multi_step_action", 1)))
    if (h0 is None) != (c0 is None):
        raise ValueError("head sequence: h0 and c0 come together (nn.LSTM's (h_0, c_0)) or not at all")
    for t in (h0, c0):
        if t is not None and tuple(t.shape) != (Lh, N, H):
            raise ValueError(f"head sequence: initial state must be {(Lh, N, H)}, got {tuple(t.shape)}")
    if getattr(cfg, "use_state", False):
        if state is None:
            raise ValueError("head sequence: a use_state head needs the robot state of every step (state_tensor, action_head.py:524-536)")
        if state.numel() % (N * L) or state.numel() // (N * L) < 7:
            raise ValueError(f"head sequence: state {tuple(state.shape)} does not hold one robot_obs row per (sequence, step) of {N} x {L}")
    elif state is not None:
        raise ValueError("head sequence: state given to a head without use_state")
    return N, L, T, (N, 1 if last_action else L, 8 * A), (Lh, N, H)


def run_head_sequence(lib, handle, cfg, feats: torch.Tensor, h0=None, c0=None, state=None, head: int = 0, last_action: bool = False,
                      features: bool = False):
    """One ``deer_head_sequence_ex`` call on the current stream: (actions (N, L or 1, 8 A), h_n, c_n[, pooled (N, L, d), lstm_out (N, L or 1, H)])."""
    N, L, T, a_shape, s_shape = head_sequence_shapes(cfg, feats.shape, h0, c0, state, last_action)
    dev = feats.device
    f = feats.to(torch.float32).contiguous()
    h0c = h0.to(device=dev, dtype=torch.float32).contiguous() if h0 is not None else None
    c0c = c0.to(device=dev, dtype=torch.float32).contiguous() if c0 is not None else None
    st = None
    flags = abi.SEQ_LAST_ACTION if last_action else 0
    if state is not None:                       # (arm pose robot_obs[:6], gripper robot_obs[-1], pad) per row, like "state_in"
        s2 = state.reshape(N * L, -1).to(device=dev, dtype=torch.float32)
        st = torch.zeros(N * L, 8, dtype=torch.float32, device=dev)
        st[:, :6] = s2[:, :6]
        st[:, 6] = s2[:, -1]
        flags |= abi.SEQ_STATE
    actions = torch.empty(a_shape, dtype=torch.float32, device=dev)
    h_n = torch.empty(s_shape, dtype=torch.float32, device=dev)
    c_n = torch.empty(s_shape, dtype=torch.float32, device=dev)
    fo = torch.empty(N, L, cfg.d_model, dtype=torch.float32, device=dev) if features else None
    ao = torch.empty(N, a_shape[1], cfg.head_hidden, dtype=torch.float32, device=dev) if features else None
    abi.check(lib.deer_head_sequence_ex(handle, int(head), abi.ptr(f), N, L, T, abi.ptr(h0c), abi.ptr(c0c), abi.ptr(st), flags, abi.ptr(actions),
                                        abi.ptr(h_n), abi.ptr(c_n), abi.ptr(fo), abi.ptr(ao), _stream()), "deer_head_sequence")
    return (actions, h_n, c_n, fo, ao) if features else (actions, h_n, c_n)


@torch.library.custom_op("deer::action_head_sequence", mutates_args=(), device_types="cuda")
def action_head_sequence(feats: torch.Tensor, h0: Optional[torch.Tensor], c0: Optional[torch.Tensor], model: int, head: int, last_action: bool,
                         state: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """feats (N, L, T, d) f32 -> (actions (N, L or 1, 8 A) = [pose 6 A | gripper prob A | logit A], h_n, c_n (L_lstm, N, H)): the head's
    window mode (action_head.py:499-611) from (h0, c0) or from zero.  head 0 = extra_exit, k >= 1 = per-layer head k (layerwise_exit_eval);
    state: robot_obs rows (N, L, S) of a use_state model.  The model's own LSTM state is not touched."""
    m = _model(model)
    return run_head_sequence(m.lib, m._h, m.cfg, feats, h0, c0, state, head, last_action)


@action_head_sequence.register_fake
def _(feats, h0, c0, model, head, last_action, state=None):
    m = _model(model)
    _, _, _, a_shape, s_shape = head_sequence_shapes(m.cfg, feats.shape, h0, c0, state, last_action)
    return (feats.new_empty(a_shape, dtype=torch.float32), feats.new_empty(s_shape, dtype=torch.float32),
            feats.new_empty(s_shape, dtype=torch.float32))


def calib_layer_slots(exit_ids: Sequence[int], n_layers: int):
    """Layer -> slot table of the calibration pass: the candidate layers are [0] + exit_ids (value_net.py:139), slot k of the pooled
    features (.., NL, d) holds candidate layer k; every other layer has no slot (-1).  Layer 0 must not be an exit (value_net.py:135)."""
    ids = [int(e) for e in exit_ids]
    if not ids or any(e <= 0 or e >= n_layers for e in ids) or any(b <= a for a, b in zip(ids, ids[1:])):
        raise ValueError(f"calibration: the exits must be increasing layers in [1, {n_layers}) (layer 0 is the first candidate, not an exit), got {ids}")
    slots = [-1] * n_layers
    for k, layer in enumerate([0] + ids):
        slots[layer] = k
    return slots


def calibrate_shapes(cfg, exit_ids: Sequence[int], feats_shape, rand_layers, threshold_type: str = "L2"):
    """Host-side checks of a calibration call (no device touched): feats (bs, W, NL, d) pooled features of the candidate layers [0] + exit_ids,
    rand_layers (bs, W) the random EXIT layer of every step (checked here when it lives on the host; on the device a layer without a slot
    makes its window's values NaN).  Returns (bs, W, NL, S = W - W/2, A)."""
    if getattr(cfg, "use_state", False):
        raise NotImplementedError("calibration of a use_state head: the reference's dynamic exit cannot run with use_state (value_net.py:122-129 "
                                  "calls the head without the robot state), so its thresholds have no consumer")
    if threshold_type not in abi.THR_TYPES:
        raise NotImplementedError(threshold_type)
    slots = calib_layer_slots(exit_ids, cfg.n_layers)
    NL = len(exit_ids) + 1
    if len(feats_shape) != 4:
        raise ValueError(f"calibrate_values: feats must be (bs, W, NL, d), got {tuple(feats_shape)}")
    bs, W, nl, d = (int(v) for v in feats_shape)
    if bs < 1 or W < 2:
        raise ValueError(f"calibrate_values: needs bs >= 1 windows of W >= 2 steps, got bs = {bs}, W = {W}")
    if nl != NL or d != cfg.d_model:
        raise ValueError(f"calibrate_values: feats (bs, W, NL, d) = {tuple(feats_shape)} for the {NL} candidate layers {[0] + list(exit_ids)} "
                         f"and d_model {cfg.d_model}")
    if tuple(rand_layers.shape) != (bs, W):
        raise ValueError(f"calibrate_values: rand_layers must be (bs, W) = {(bs, W)}, got {tuple(rand_layers.shape)}")
    if rand_layers.device.type == "cpu":
        bad = [int(v) for v in rand_layers.reshape(-1).tolist() if not (0 <= int(v) < cfg.n_layers and slots[int(v)] > 0)]
        if bad:
            raise ValueError(f"calibrate_values: rand_layers holds {sorted(set(bad))}, not exit layers {list(exit_ids)}")
    return bs, W, NL, W - W // 2, max(1, int(getattr(cfg, "multi_step_action", 1)))


def run_calibrate_values(lib, handle, cfg, exit_ids, feats: torch.Tensor, rand_layers, threshold_type: str = "L2", return_actions: bool = False):
    """One ``deer_calibrate_values`` call on the current stream: values (n_exit, bs * (W - W/2)) on the device[, actions (NL, bs, W - W/2, 8 A)]."""
    rl = torch.as_tensor(rand_layers)
    bs, W, NL, S, A = calibrate_shapes(cfg, exit_ids, feats.shape, rl, threshold_type)
    dev = feats.device
    f = feats.to(torch.float32).contiguous()
    rl_d = rl.to(device=dev, dtype=torch.int32).contiguous()
    values = torch.empty(NL - 1, bs * S, dtype=torch.float32, device=dev)
    actions = torch.empty(NL, bs, S, 8 * A, dtype=torch.float32, device=dev) if return_actions else None
    abi.check(lib.deer_calibrate_values(handle, abi.ptr(f), abi.ptr(rl_d), bs, W, abi.THR_TYPES[threshold_type], abi.ptr(values), abi.ptr(actions),
                                        _stream()), "deer_calibrate_values")
    return (values, actions) if return_actions else values


def exit_head_count(cfg) -> int:
    """Heads of the all-exits forward in the reference's ``all_outputs`` order (train_utils.py:503): one per internal exit when the model
    carries per-layer heads (layerwise_exit_eval), the last layer's head, extra_exit on sampling strategy 1 and on strategy 2."""
    return (len(cfg.exit_ids()) - 1 if getattr(cfg, "layerwise_exit_eval", False) else 0) + 3


def exit_outputs_shapes(cfg, feats_shape, rand_layers, two_layers, state=None):
    """Host-side checks of an all-exits call (no device touched): feats (bs, W, NE, d) pooled features of the exit layers
    ``cfg.exit_ids()`` (flamingo_mpt.py:268-270), rand_layers / two_layers (bs, W) the exit LAYER of every step under sampling strategy
    1 / 2 (checked here when they live on the host; on the device a layer that is no exit makes its window's actions NaN), state
    (bs, W, S) / (bs * W, S) robot_obs rows (use_state models only).  Returns (bs, W, NE, Hn, A)."""
    exits = [int(e) for e in cfg.exit_ids()]
    NE = len(exits)
    if len(feats_shape) != 4:
        raise ValueError(f"exit_outputs: feats must be (bs, W, NE, d), got {tuple(feats_shape)}")
    bs, W, ne, d = (int(v) for v in feats_shape)
    if bs < 1 or W < 1:
        raise ValueError(f"exit_outputs: needs bs >= 1 windows of W >= 1 steps, got bs = {bs}, W = {W}")
    if ne != NE or d != cfg.d_model:
        raise ValueError(f"exit_outputs: feats (bs, W, NE, d) = {tuple(feats_shape)} for the {NE} exit layers {exits} and d_model {cfg.d_model}")
    for name, t in (("rand_layers", rand_layers), ("two_layers", two_layers)):
        if tuple(t.shape) != (bs, W):
            raise ValueError(f"exit_outputs: {name} must be (bs, W) = {(bs, W)}, got {tuple(t.shape)}")
        if t.device.type == "cpu":
            bad = [int(v) for v in t.reshape(-1).tolist() if int(v) not in exits]
            if bad:
                raise ValueError(f"exit_outputs: {name} holds {sorted(set(bad))}, not exit layers {exits}")
    if getattr(cfg, "use_state", False):
        if state is None:
            raise ValueError("exit_outputs: a use_state model needs the robot state of every step (state_tensor, action_head.py:524-536)")
        if state.numel() % (bs * W) or state.numel() // (bs * W) < 7:
            raise ValueError(f"exit_outputs: state {tuple(state.shape)} does not hold one robot_obs row per (window, step) of {bs} x {W}")
    elif state is not None:
        raise ValueError("exit_outputs: state given to a model without use_state")
    return bs, W, NE, exit_head_count(cfg), max(1, int(getattr(cfg, "multi_step_action", 1)))


def run_exit_outputs(lib, handle, cfg, feats: torch.Tensor, rand_layers, two_layers, state=None) -> torch.Tensor:
    """One ``deer_exit_outputs`` call on the current stream: actions (Hn, bs, W, 8 A) on the device."""
    rl, tl = torch.as_tensor(rand_layers), torch.as_tensor(two_layers)
    bs, W, NE, Hn, A = exit_outputs_shapes(cfg, feats.shape, rl, tl, state)
    dev = feats.device
    f = feats.to(torch.float32).contiguous()
    sel = torch.stack([rl.to(device=dev, dtype=torch.int32), tl.to(device=dev, dtype=torch.int32)]).contiguous()
    st = None
    if state is not None:                       # (arm pose robot_obs[:6], gripper robot_obs[-1], pad) per row, like "state_in"
        s2 = state.reshape(bs * W, -1).to(device=dev, dtype=torch.float32)
        st = torch.zeros(bs * W, 8, dtype=torch.float32, device=dev)
        st[:, :6] = s2[:, :6]
        st[:, 6] = s2[:, -1]
    assert lib.deer_exit_n_heads(handle) == Hn
    actions = torch.empty(Hn, bs, W, 8 * A, dtype=torch.float32, device=dev)
    abi.check(lib.deer_exit_outputs(handle, abi.ptr(f), 1, abi.ptr(sel), abi.ptr(st), bs, W, abi.ptr(actions), _stream()), "deer_exit_outputs")
    return actions


def exit_losses_shapes(cfg, actions_shape, pose_shape, grip_shape):
    """Host-side checks of a loss call: actions (Hn, ..., 8 A) with R rows per head, pose labels R x 6 A, gripper targets R x A (0 / 1).
    Returns (Hn, R, A)."""
    A = max(1, int(getattr(cfg, "multi_step_action", 1)))
    if len(actions_shape) < 2 or int(actions_shape[-1]) != 8 * A:
        raise ValueError(f"exit_losses: actions must be (Hn, ..., 8 A = {8 * A}), got {tuple(actions_shape)}")
    Hn = int(actions_shape[0])
    R = 1
    for v in actions_shape[1:-1]:
        R *= int(v)
    if Hn < 1 or R < 1:
        raise ValueError(f"exit_losses: no heads / rows in actions {tuple(actions_shape)}")
    n_pose, n_grip = 1, 1
    for v in pose_shape:
        n_pose *= int(v)
    for v in grip_shape:
        n_grip *= int(v)
    if n_pose != R * 6 * A or n_grip != R * A:
        raise ValueError(f"exit_losses: labels pose {tuple(pose_shape)} / gripper {tuple(grip_shape)} do not hold {6 * A} / {A} values for each of "
                         f"the {R} rows of actions {tuple(actions_shape)}")
    return Hn, R, A


def run_exit_losses(lib, cfg, actions: torch.Tensor, pose, grip01, w_bin: float = 0.01):
    """One ``deer_exit_losses`` call on the current stream: (num (Hn, R), bin (Hn, R), loss (Hn,)) on the device."""
    Hn, R, A = exit_losses_shapes(cfg, actions.shape, pose.shape, grip01.shape)
    dev = actions.device
    a = actions.to(torch.float32).contiguous()
    p = pose.to(device=dev, dtype=torch.float32).contiguous()
    g = grip01.to(device=dev, dtype=torch.float32).contiguous()
    num = torch.empty(Hn, R, dtype=torch.float32, device=dev)
    bin_ = torch.empty(Hn, R, dtype=torch.float32, device=dev)
    loss = torch.empty(Hn, dtype=torch.float32, device=dev)
    abi.check(lib.deer_exit_losses(abi.ptr(a), abi.ptr(p), abi.ptr(g), Hn, R, A, float(w_bin), abi.ptr(num), abi.ptr(bin_), abi.ptr(loss), _stream()),
              "deer_exit_losses")
    return num, bin_, loss


@torch.library.custom_op("deer::calibrate_values", mutates_args=(), device_types="cuda")
def calibrate_values(feats: torch.Tensor, rand_layers: torch.Tensor, model: int, threshold_type: str) -> torch.Tensor:
    """feats (bs, W, NL, d) pooled features of the candidate layers [0] + exits (deer_pool_exit_layers), rand_layers (bs, W) int -> the
    deltas between consecutive exits (n_exit, bs * (W - W/2)), window-major (value_net.py:134-160).  The model's LSTM state is not touched."""
    m = _model(model)
    return run_calibrate_values(m.lib, m._h, m.cfg, m.exit_ids, feats, rand_layers, threshold_type)


@calibrate_values.register_fake
def _(feats, rand_layers, model, threshold_type):
    m = _model(model)
    bs, W, NL, S, _ = calibrate_shapes(m.cfg, m.exit_ids, feats.shape, rand_layers, threshold_type)
    return feats.new_empty((NL - 1, bs * S), dtype=torch.float32)


def solve_thresholds_shapes(values, counts):
    """Host-side checks of a threshold solve (no device touched): values (n_stage, n_sample) float32 deltas of the calibration set,
    counts (k, n_exit) integers - ``value_net.exit_counts`` of every operating point; the solver reads rows 0 .. n_exit - 2 of values.
    Returns (n_stage, n_sample, k, n_exit)."""
    if values.dim() != 2 or values.dtype != torch.float32:
        raise ValueError(f"solve_thresholds: values must be (n_stage, n_sample) float32, got {tuple(values.shape)} {values.dtype}")
    n_stage, n_sample = (int(v) for v in values.shape)
    if counts.dim() != 2 or counts.dtype.is_floating_point or counts.dtype == torch.bool:
        raise ValueError(f"solve_thresholds: counts must be (k, n_exit) integers, got {tuple(counts.shape)} {counts.dtype}")
    k, n_exit = (int(v) for v in counts.shape)
    if k < 1 or n_exit < 1 or n_sample < 1:
        raise ValueError(f"solve_thresholds: needs k >= 1 points, n_exit >= 1 exits and n_sample >= 1 samples, got values {tuple(values.shape)}, "
                         f"counts {tuple(counts.shape)}")
    if n_exit > 16:
        raise ValueError(f"solve_thresholds: {n_exit} exits, a threshold row holds at most 16")
    if n_exit > n_stage:
        raise ValueError(f"solve_thresholds: counts for {n_exit} exits, values has {n_stage} rows")
    return n_stage, n_sample, k, n_exit


def run_solve_thresholds(lib, values: torch.Tensor, counts, leq: bool = True):
    """One ``deer_solve_thresholds`` launch on the current stream: (thresholds (k, n_exit) f32, exit_counts (k, n_exit) i32, status (k,)
    i32 - the NaNs met per point) on the device, nothing synchronised.  values stays where it is: a row stride above n_sample (a column
    slice of a wider matrix) is passed on as ``ld``."""
    counts = torch.as_tensor(counts)
    n_stage, n_sample, k, n_exit = solve_thresholds_shapes(values, counts)
    dev = values.device
    v = values.detach()
    if v.stride(1) != 1 or v.stride(0) < n_sample or v.stride(0) > 0x7fffffff:
        v = v.contiguous()
    c = counts.to(device=dev, dtype=torch.int32).contiguous()
    alive = torch.empty(k * n_sample, dtype=torch.uint8, device=dev)
    T = torch.empty(k, n_exit, dtype=torch.float32, device=dev)
    left = torch.empty(k, n_exit, dtype=torch.int32, device=dev)
    status = torch.empty(k, dtype=torch.int32, device=dev)
    abi.check(lib.deer_solve_thresholds(abi.ptr(v), n_stage, n_sample, v.stride(0), abi.ptr(c), k, n_exit, 1 if leq else 0, abi.ptr(alive), abi.ptr(T),
                                        abi.ptr(left), abi.ptr(status), _stream()), "deer_solve_thresholds")
    return T, left, status


@torch.library.custom_op("deer::solve_thresholds", mutates_args=(), device_types="cuda")
def solve_thresholds(values: torch.Tensor, counts: torch.Tensor, leq: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """values (n_stage, n_sample) f32, counts (k, n_exit) int -> (thresholds (k, n_exit) f32, exit_counts (k, n_exit) i32, status (k,) i32):
    the solver of ExitController.set_threshold (value_net.py:242-262) for k operating points in one launch (csrc/thresholds.hip)."""
    return run_solve_thresholds(abi.lib(), values, counts, leq)


@solve_thresholds.register_fake
def _(values, counts, leq):
    _, _, k, n_exit = solve_thresholds_shapes(values, counts)
    return (values.new_empty((k, n_exit), dtype=torch.float32), values.new_empty((k, n_exit), dtype=torch.int32),
            values.new_empty((k,), dtype=torch.int32))


def value_log_shapes(ctl, n_envs: int, n_exit: int, active_mask: int, values, capacity: int, taken, state):
    """Host-side checks of one append to a value log (no device touched): ctl int32 control blocks of n_envs environments, values
    (n_exit or more rows, capacity or more columns) float32 with unit column stride, taken (capacity,) int32, state (3,) int32 =
    {count, dropped, nonfinite}.  Returns the row stride of values."""
    if ctl.dtype != torch.int32 or ctl.numel() < n_envs * abi.CTL_WORDS or not ctl.is_contiguous():
        raise ValueError(f"value_log_append: ctl must hold {n_envs} contiguous int32 control blocks, got {tuple(ctl.shape)} {ctl.dtype}")
    if not 1 <= n_envs <= abi.MAX_ENVS or not 1 <= n_exit <= 16:
        raise ValueError(f"value_log_append: n_envs = {n_envs} (1..{abi.MAX_ENVS}), n_exit = {n_exit} (1..16)")
    if active_mask < 0 or active_mask >> n_envs:
        raise ValueError(f"value_log_append: active_mask {active_mask:#x} names environments beyond the {n_envs} of the batch")
    if values.dim() != 2 or values.dtype != torch.float32 or values.shape[0] < n_exit or values.shape[1] < capacity or capacity < 1 \
            or values.stride(1) != 1 or not capacity <= values.stride(0) <= 0x7fffffff:
        raise ValueError(f"value_log_append: values must be ({n_exit}+, {capacity}+) float32 rows, got {tuple(values.shape)} {values.dtype} "
                         f"strides {tuple(values.stride())}")
    if taken.dtype != torch.int32 or taken.dim() != 1 or taken.numel() < capacity or not taken.is_contiguous():
        raise ValueError(f"value_log_append: taken must be ({capacity},) int32, got {tuple(taken.shape)} {taken.dtype}")
    if state.dtype != torch.int32 or state.numel() != 3 or not state.is_contiguous():
        raise ValueError(f"value_log_append: state must be 3 int32 words, got {tuple(state.shape)} {state.dtype}")
    return int(values.stride(0))


def run_value_log_append(lib, ctl: torch.Tensor, n_envs: int, n_exit: int, active_mask: int, values: torch.Tensor, capacity: int,
                         taken: torch.Tensor, state: torch.Tensor):
    """One ``deer_value_log_append`` launch on the current stream (csrc/value_log.hip); nothing is synchronised or allocated."""
    ld = value_log_shapes(ctl, n_envs, n_exit, active_mask, values, capacity, taken, state)
    abi.check(lib.deer_value_log_append(abi.ptr(ctl), n_envs, n_exit, active_mask, abi.ptr(values), ld, capacity, abi.ptr(taken), abi.ptr(state),
                                        _stream()), "deer_value_log_append")


@torch.library.custom_op("deer::value_log_append", mutates_args=("values", "taken", "state"), device_types="cuda")
def value_log_append(ctl: torch.Tensor, n_envs: int, n_exit: int, active_mask: int, values: torch.Tensor, capacity: int, taken: torch.Tensor,
                     state: torch.Tensor) -> None:
    """Appends the deltas (ctl[b][CTL_DELTAS + e], e < n_exit) and the exit layer of every environment of active_mask to the value log
    (values, taken, state = {count, dropped, nonfinite}) after a shadow step: on-policy exit values (value_net.py:120-133)."""
    run_value_log_append(abi.lib(), ctl, n_envs, n_exit, active_mask, values, capacity, taken, state)


@value_log_append.register_fake
def _(ctl, n_envs, n_exit, active_mask, values, capacity, taken, state):
    value_log_shapes(ctl, n_envs, n_exit, active_mask, values, capacity, taken, state)


MAX_GRAD_ROWS = 2048       # rows (N * L) of one deer_head_loss_grad call (csrc/model.hip kSeqRows); longer batches are chunked by the caller


def head_param_table(lib, handle, head: int):
    """The spine's table of one head's trainable tensors (``deer_head_param_entry``, host only): ([(name, offset, numel, decays)] in the
    reference's state-dict order, floats of the flat buffer).  head 0 = extra_exit, k >= 1 = per-layer head k."""
    n = lib.deer_head_param_count(handle, int(head))
    if n < 0:
        raise ValueError(f"head {head}: the model has no such head")
    name = ctypes.create_string_buffer(256)
    off, numel, dec = ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
    out = []
    for i in range(n):
        abi.check(lib.deer_head_param_entry(handle, int(head), i, name, len(name), ctypes.byref(off), ctypes.byref(numel), ctypes.byref(dec)),
                  "deer_head_param_entry")
        out.append((name.value.decode(), off.value, numel.value, bool(dec.value)))
    abi.check(lib.deer_head_param_entry(handle, int(head), -1, None, 0, ctypes.byref(off), ctypes.byref(numel), None), "deer_head_param_entry")
    return out, numel.value


def head_loss_grad_shapes(cfg, total: int, params, feats_shape, pose_shape, grip_shape, grad):
    """Host-side checks of one loss-gradient call (no device touched): params / grad flat float32 buffers of ``total`` values, feats
    (N, L, d) pooled rows, pose N L x 6 A, grip01 N L x A.  Returns (N, L, A)."""
    if getattr(cfg, "use_state", False):
        raise NotImplementedError("head_loss_grad: a use_state head would need gradients for its state embeddings (embed_arm_state, "
                                  "embed_gripper_state, embed_state); they are not built")
    A = max(1, int(getattr(cfg, "multi_step_action", 1)))
    if len(feats_shape) != 3 or int(feats_shape[2]) != cfg.d_model:
        raise ValueError(f"head_loss_grad: feats must be (N, L, d = {cfg.d_model}) pooled rows, got {tuple(feats_shape)}")
    N, L = int(feats_shape[0]), int(feats_shape[1])
    if N < 1 or L < 1 or N * L > MAX_GRAD_ROWS:
        raise ValueError(f"head_loss_grad: {N} x {L} rows; one call takes 1..{MAX_GRAD_ROWS} (chunk whole sequences with accumulate=True)")
    for name, t in (("params", params), ("grad", grad)):
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != total or not t.is_contiguous():
            raise ValueError(f"head_loss_grad: {name} must be a contiguous float32 buffer of {total} values, got {tuple(t.shape)} {t.dtype}")
    n_pose, n_grip = 1, 1
    for v in pose_shape:
        n_pose *= int(v)
    for v in grip_shape:
        n_grip *= int(v)
    if n_pose != N * L * 6 * A or n_grip != N * L * A:
        raise ValueError(f"head_loss_grad: labels pose {tuple(pose_shape)} / gripper {tuple(grip_shape)} do not hold {6 * A} / {A} values for each "
                         f"of the {N * L} rows")
    return N, L, A


def run_head_loss_grad(lib, handle, cfg, head: int, params: torch.Tensor, feats: torch.Tensor, pose, grip01, w_bin: float, scale: float,
                       grad: torch.Tensor, accumulate: bool, loss_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``deer_head_loss_grad`` call on the current stream: grad (+)= scale d loss / d params, returns the (1,) loss of the call's rows
    on the device (written into ``loss_out`` when given); nothing is synchronised."""
    _, total = head_param_table(lib, handle, head)
    N, L, A = head_loss_grad_shapes(cfg, total, params, feats.shape, pose.shape, grip01.shape, grad)
    dev = params.device
    f = feats.to(device=dev, dtype=torch.float32).contiguous()
    p = pose.to(device=dev, dtype=torch.float32).contiguous()
    g = grip01.to(device=dev, dtype=torch.float32).contiguous()
    loss = loss_out if loss_out is not None else torch.empty(1, dtype=torch.float32, device=dev)
    abi.check(lib.deer_head_loss_grad(handle, int(head), abi.ptr(params), abi.ptr(f), N, L, abi.ptr(p), abi.ptr(g), float(w_bin), float(scale),
                                      abi.ptr(grad), 1 if accumulate else 0, abi.ptr(loss), _stream()), "deer_head_loss_grad")
    return loss


@torch.library.custom_op("deer::head_loss_grad", mutates_args=("grad",), device_types="cuda")
def head_loss_grad(params: torch.Tensor, feats: torch.Tensor, pose: torch.Tensor, grip01: torch.Tensor, model: int, head: int, w_bin: float,
                   scale: float, grad: torch.Tensor, accumulate: bool) -> torch.Tensor:
    """params / grad: flat f32 buffers laid out by ``head_param_table``; feats (N, L, d) pooled rows of N windows; pose (N, L, 6 A), grip01
    (N, L, A) labels -> the (1,) loss mean_rows(Huber + w_bin BCE) (train_utils.py:519-540); grad (+)= scale d loss / d params."""
    m = _model(model)
    return run_head_loss_grad(m.lib, m._h, m.cfg, head, params, feats, pose, grip01, w_bin, scale, grad, accumulate)


@head_loss_grad.register_fake
def _(params, feats, pose, grip01, model, head, w_bin, scale, grad, accumulate):
    return params.new_empty((1,), dtype=torch.float32)


def adamw_shapes(param, grad, m, v, seg_end, seg_decay, step: int):
    """Host-side checks of one AdamW launch (no device touched).  Returns (numel, n_seg)."""
    n = param.numel()
    for name, t in (("param", param), ("grad", grad), ("m", m), ("v", v)):
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"adamw_step: {name} must be a contiguous float32 buffer of {n} values, got {tuple(t.shape)} {t.dtype}")
    if n < 1:
        raise ValueError("adamw_step: empty buffers")
    if seg_end.dtype != torch.int32 or seg_decay.dtype != torch.int32 or seg_end.shape != seg_decay.shape or seg_end.dim() != 1:
        raise ValueError(f"adamw_step: seg_end / seg_decay must be int32 vectors of one length, got {tuple(seg_end.shape)} {seg_end.dtype} / "
                         f"{tuple(seg_decay.shape)} {seg_decay.dtype}")
    if step < 1:
        raise ValueError(f"adamw_step: step counts from 1, got {step}")
    return n, int(seg_end.numel())


def run_adamw_step(lib, param, grad, m, v, seg_end, seg_decay, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int):
    """One ``deer_adamw_step`` launch on the current stream (csrc/head_grad.hip); nothing is synchronised or allocated."""
    n, n_seg = adamw_shapes(param, grad, m, v, seg_end, seg_decay, step)
    hyper = (ctypes.c_double * 5)(float(lr), float(beta1), float(beta2), float(eps), float(weight_decay))     # read on the host during the call
    abi.check(lib.deer_adamw_step(abi.ptr(param), abi.ptr(grad), abi.ptr(m), abi.ptr(v), n, abi.ptr(seg_end) if n_seg else None,
                                  abi.ptr(seg_decay) if n_seg else None, n_seg, hyper, int(step), _stream()), "deer_adamw_step")


@torch.library.custom_op("deer::adamw_step", mutates_args=("param", "m", "v"), device_types="cuda")
def adamw_step(param: torch.Tensor, grad: torch.Tensor, m: torch.Tensor, v: torch.Tensor, seg_end: torch.Tensor, seg_decay: torch.Tensor,
               lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int) -> None:
    """torch.optim.AdamW's update of flat f32 buffers in one launch; seg_end / seg_decay (int32, device): ascending exclusive segment ends and
    their decay flags (biases and norms 0) - empty: every element decays."""
    run_adamw_step(abi.lib(), param, grad, m, v, seg_end, seg_decay, lr, beta1, beta2, eps, weight_decay, step)


@adamw_step.register_fake
def _(param, grad, m, v, seg_end, seg_decay, lr, beta1, beta2, eps, weight_decay, step):
    adamw_shapes(param, grad, m, v, seg_end, seg_decay, step)


def decode_ctl(ctl: torch.Tensor):
    """control blocks -> list of dict(exit_layer, pose (6,), gripper, gripper_logit, deltas) per environment"""
    c = ctl.cpu()
    f = c.view(torch.float32)
    out = []
    for b in range(c.shape[0]):
        a = f[b, abi.CTL_OUT_ACTION: abi.CTL_OUT_ACTION + 8]
        out.append(dict(exit_layer=int(c[b, abi.CTL_EXIT_LAYER]), pose=a[:6].clone(), gripper=float(a[6]), gripper_logit=float(a[7]),
                        deltas=f[b, abi.CTL_DELTAS: abi.CTL_DELTAS + 16].clone()))
    return out
