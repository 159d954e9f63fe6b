"""Threshold calibration as one device pass (``deer_pool_exit_layers`` / ``deer_calibrate_values``, csrc/calib.hip) through the C ABI:
against the oracle's generate mode, the reference's recorded deltas, the existing per-step loop (``DeerEngine.generate_values``) on the
same device hidden states, its own chunking, and at full size.  Every figure is printed before it is asserted."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load, full_size_state, s2str  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_3b, deer_9b, deer_tiny  # noqa: E402
from deer_vla_amd.engine import DeerEngine  # noqa: E402
from deer_vla_amd.value_net import ActionValueNet, generate_action_values, solve_thresholds  # noqa: E402
from oracle import deer_oracle as orc  # noqa: E402

GATE16, GATE32 = 5e-3, 2e-4          # values: the project's gate for this quantity (16-bit operands); twice the 1e-4 per-action gate (fp32)
TYPES = ["L2", "mean", "max", "cosine"]


def _gate(precision):
    return GATE32 if precision == "fp32" else GATE16


def _small_towers(cfg, **kw):
    """tower dims the engine can be built with around a head (and trunk depth) configuration; every tensor is seeded by its name"""
    return dataclasses.replace(cfg, vit_width=128, vit_heads=2, vit_layers=1, vit_mlp=256, image_size=28, perc_heads=2, perc_dim_head=64,
                               perc_latents=8, perc_depth=1, xattn_heads=2, xattn_dim_head=64, **kw)


def _pool(hid, layers, pooling):
    """hid (..., L, T, d) -> (..., NL, d): the head's pooling (action_head.py:519-520) of the candidate layers, on the host"""
    h = hid[..., layers, :, :]
    return h.amax(-2) if pooling == "max" else h.mean(-2)


def _delta64(a, ttype):
    """get_delta (value_net.py:105-117) of consecutive candidate layers in float64: a (NL, bs, S, 6 A) -> (n_exit, bs * S)"""
    a = a.double()
    return orc.get_delta(a[:-1], a[1:], ttype).flatten(1, 2)


class _ZeroStartHead(orc.OracleHead):
    """OracleHead with every evaluation started from the zero LSTM state - what generate mode is for every W > 2, where each call is a
    window-mode sequence.  At W = 2 the sequences have ONE step, and a one-step call takes the head's step mode, which continues from whatever
    state the previous call left behind (the previous candidate layer, or an earlier window batch): that carry-over is call history, not
    part of generate mode, and ``DeerEngine.generate_values`` starts W = 2 from zero as well.  W = 3 has one such call too: its first seq_id
    is W/2 - 1 = 0, an empty history + the candidate's own step, so that call is a one-step sequence as at W = 2 (its seq_id = 1 calls have
    two steps and are window mode).  For W > 3 this class changes nothing."""

    def __call__(self, *a, **k):
        self.clear_hidden_state()
        return super().__call__(*a, **k)


def _oracle_values(head, exit_ids, hid, rl, ttype):
    """OracleValueNet(mode='generate') (value_net.py:134-160): hid (bs, W, L, T, d), rl (bs, W) -> values (n_exit, bs * S)"""
    bs, W, L, T, d = hid.shape
    head.window_size = W
    vn = orc.OracleValueNet(exit_ids, head, 0, W, ttype)
    feats = tuple(hid[:, :, l].reshape(bs * W, T, d) for l in range(L))
    rand = torch.stack([hid[b, t, int(rl[b, t])] for b in range(bs) for t in range(W)])
    return vn(feats, mode="generate", rand_layer_feat=rand)


def _oracle_actions(head, exit_ids, hid, rl):
    """the candidates' actions behind those values (the loop of value_net.py:139-153 with the actions kept): (NL, bs, S, 6 A)"""
    bs, W, L, T, d = hid.shape
    head.window_size = W
    rand = torch.stack([hid[b, t, int(rl[b, t])] for b in range(bs) for t in range(W)])
    acts = []
    for seq_id in range(W // 2 - 1, W - 1):
        prev = rand.reshape(bs, W, T, d)[:, :seq_id]
        row = []
        for i in [0] + list(exit_ids):
            head.last_action = True
            a = head(torch.cat([prev, hid[:, seq_id:seq_id + 1, i]], dim=1))
            head.last_action = False
            row.append(a[0].squeeze(1))
        acts.append(torch.stack(row))
    return torch.stack(acts).permute(1, 2, 0, 3)


def _oracle_generate(head, exit_ids, hid, rl, ttype):
    """(values (n_exit, bs * S), actions (NL, bs, S, 6 A))"""
    return _oracle_values(head, exit_ids, hid, rl, ttype), _oracle_actions(head, exit_ids, hid, rl)


COS_MIN_NORM, COS_MAX_LEFT_OUT = 0.1, 0.10


def _cosine_comparable(a_ref):
    """Where the cosine value of a pair of consecutive candidate layers is compared with the oracle's: both fp64 norms of the oracle's actions
    are >= 0.1.  An action error e turns a unit vector by at most e / |a|, so there the value moves by at most ~ 2 e / 0.1 and the project's
    gate on values holds for action errors of a twentieth of it; with both actions near zero the direction is rounding noise.  a_ref
    (NL, bs, S, 6 A) -> bool (n_exit, bs * S)"""
    n = a_ref.double().norm(dim=-1).flatten(1, 2)
    return (n[:-1] >= COS_MIN_NORM) & (n[1:] >= COS_MIN_NORM)


BS_TINY, W_TINY = (1, 3, 20), (2, 3, 4, 5, 7, 8, 11, 12)


def _tiny_case(pool, exit_ids, bs, W):
    """the committed inputs of test_values_and_actions_vs_oracle_tiny: (hid (bs, W, L, T, d), rand_layers (bs, W))"""
    idx = torch.tensor([[(7 * b + t) % pool.shape[0] for t in range(W)] for b in range(bs)])
    return pool[idx], _rand_layers(exit_ids, bs, W, 100 * bs + W)


def _rand_layers(exit_ids, bs, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.tensor([exit_ids[int(i)] for i in torch.randint(0, len(exit_ids), (W,), generator=g)]) for _ in range(bs)])


# ---- 1. against the oracle on the tiny config -----------------------------------------------------------------------------------------
_TINY_HID = {}


def _tiny_oracle_hidden(n_frames=24):
    """the oracle's own hidden states of every layer for a pool of frames: (n_frames, L, T, d).  The head variants below share the trunk
    (tensors are seeded by name), so one pool serves them all."""
    if "h" not in _TINY_HID:
        cfg = deer_tiny()
        sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
        model = orc.OracleDeer(sd, cfg)
        hid = []
        for f in range(n_frames):
            rgb, grip, ids, mask = syn.synthetic_step_inputs(cfg, 50 + f, text_len=9)
            h, _ = orc.llm_forward(sd, cfg, ids, mask, model.encode_vision(rgb, grip), exit_id=cfg.n_layers - 1)
            hid.append(torch.stack([x[0] for x in h]))
        _TINY_HID["h"] = torch.stack(hid)
    return _TINY_HID["h"]


_ORACLE_MEMO = {}
VARIANTS = {"ln_max": {}, "plain": dict(lstm_layernorm=False, mlp_layernorm=False), "avg": dict(pooling="avg"), "ms2": dict(multi_step_action=2)}


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_values_and_actions_vs_oracle_tiny(variant, precision):
    pool = _tiny_oracle_hidden()
    cfg = deer_tiny(**VARIANTS[variant])
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)        # 8-bit significands: the weights every precision of the engine holds exactly
    ecfg = _small_towers(cfg)
    eng = DeerEngine(ecfg, syn.make_synthetic_state(ecfg, 3, bf16_round=True), precision=precision)
    head = _ZeroStartHead(sd, cfg, "extra_exit.")
    exit_ids = cfg.exit_ids()
    layers = [0] + exit_ids
    A = max(1, cfg.multi_step_action)
    gate, worst = _gate(precision), {}
    pairs = left_out = 0
    memo = _ORACLE_MEMO.setdefault(variant, {})                   # the oracle does not depend on the engine's precision: once per variant
    for bs in BS_TINY:                                            # 20 windows: more than one sibling engine holds in the per-step loop
        for W in W_TINY:                                          # odd W: W/2 - 1 + s and S = W - W/2 round differently; W = 3 starts at seq_id 0
            hid, rl = _tiny_case(pool, exit_ids, bs, W)           # (bs, W, L, T, d)
            P = _pool(hid, layers, cfg.pooling).cuda()
            if (bs, W) not in memo:
                memo[bs, W] = (_oracle_actions(head, exit_ids, hid, rl), {t: _oracle_values(head, exit_ids, hid, rl, t) for t in TYPES})
            a_ref, v_refs = memo[bs, W]
            cos_ok = _cosine_comparable(a_ref)
            pairs, left_out = pairs + cos_ok.numel(), left_out + int((~cos_ok).sum())
            for ttype in TYPES:
                v_ref = v_refs[ttype]
                v, a = eng.calibrate_values(P, rl, ttype, return_actions=True)
                assert v.is_cuda and tuple(v.shape) == tuple(v_ref.shape) == (len(exit_ids), bs * (W - W // 2))
                assert tuple(a.shape) == (len(layers), bs, W - W // 2, 8 * A)
                v, a = v.cpu(), a.cpu()[..., :6 * A]
                ea = float((a - a_ref).abs().max())
                e64 = float((v.double() - _delta64(a, ttype)).abs().max())
                ev = float((v - v_ref).abs().max())
                print(f"{variant} {precision} bs={bs} W={W} {ttype}: |actions-oracle|={ea:.3e} |values-oracle|={ev:.3e} |values-fp64(own actions)|={e64:.3e}")
                assert ea < gate, (bs, W, ttype, ea)
                assert e64 < 1e-5, (bs, W, ttype, e64)            # the delta kernel is f32
                if ttype == "cosine":                             # compared wherever both oracle actions have a norm >= 0.1 (_cosine_comparable)
                    ev = float((v - v_ref).abs()[cos_ok].max()) if bool(cos_ok.any()) else 0.0
                    print(f"{variant} {precision} bs={bs} W={W} cosine: {int((~cos_ok).sum())} of {cos_ok.numel()} pairs left out, |values-oracle|={ev:.3e} on the rest")
                worst[ttype] = max(worst.get(ttype, 0.0), ev)
                assert ev < gate, (bs, W, ttype, ev)
    print(f"{variant} {precision}: worst |values-oracle| {worst}; cosine pairs left out {left_out} of {pairs}")
    assert left_out <= COS_MAX_LEFT_OUT * pairs, (left_out, pairs)   # the same count on the CPU: test_calibrate_cpu.py


# ---- 2. against the reference's recorded output --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_values_vs_reference_recording(precision):
    cfg0, seed, g = load("valuenet_generate.npz")
    ecfg = _small_towers(cfg0)
    eng = DeerEngine(ecfg, syn.make_synthetic_state(ecfg, seed), precision=precision)
    exit_ids, W, bs = cfg0.exit_ids(), cfg0.window_size, int(g["bs"])
    feats = g["feats"]                                            # (L, bs * W, T, d), recorded from the reference's ActionValueNet
    hid = feats.view(feats.shape[0], bs, W, *feats.shape[2:]).permute(1, 2, 0, 3, 4)
    P = _pool(hid, [0] + exit_ids, cfg0.pooling).cuda()
    v = eng.calibrate_values(P, g["rand_layers"].view(bs, W), s2str(g["threshold_type"])).cpu()
    err = float((v - g["delta"]).abs().max())
    print(f"valuenet_generate.npz {precision}: |values-recorded delta|={err:.3e}")
    assert v.shape == g["delta"].shape
    assert err < _gate(precision)


# ---- 3. against the existing loop on identical device hidden states -----------------------------------------------------------------
def _window_batch(cfg, bs, W, seed0=0):
    frames = [[syn.synthetic_step_inputs(cfg, seed0 + 10 * b + t, text_len=9) for t in range(W)] for b in range(bs)]
    S = cfg.image_size
    images = torch.stack([torch.stack([f[0].reshape(3, S, S) for f in fr]) for fr in frames])
    gripper = torch.stack([torch.stack([f[1].reshape(3, S, S) for f in fr]) for fr in frames])
    ids = torch.cat([fr[0][2] for fr in frames])
    return (images, (ids, torch.ones_like(ids)), None, gripper)


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("pooling", ["max", "avg"])
def test_fused_vs_per_step_loop_on_device_hidden_states(pooling, precision, monkeypatch):
    cfg = deer_tiny(pooling=pooling)
    eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, 3, bf16_round=True), precision=precision)
    exit_ids = cfg.exit_ids()
    eng.configure_exit(exit_ids, 12, 1)
    bs, W = 3, 8
    images, (ids, _), _, gripper = _window_batch(cfg, bs, W)
    S, T = cfg.image_size, ids.shape[-1]
    rgb = images.reshape(bs * W, 3, S, S).cuda().to(eng.img_dtype)
    grip = gripper.reshape(bs * W, 3, S, S).cuda().to(eng.img_dtype)
    ids_f = ids.cuda().unsqueeze(1).expand(bs, W, T).reshape(bs * W, T)
    hid = eng.window_hidden_states(rgb, grip, ids_f)                                  # (F, L, T, d)
    feats = eng.window_exit_features(rgb, grip, ids_f)                                # (F, NL, d)
    torch.cuda.synchronize()
    layers = [0] + exit_ids
    assert tuple(feats.shape) == (bs * W, len(layers), cfg.d_model)
    h = hid[:, layers]
    if pooling == "max":
        assert torch.equal(feats, h.amax(2))                                          # max is exact
    else:
        acc = h[:, :, 0].clone()
        for t in range(1, T):                                                         # the kernel's order: rows 0 .. T - 1, then / T
            acc = acc + h[:, :, t]
        want = acc / T
        ulps = float(((feats - want).abs() / (want.abs() * 2.0 ** -23).clamp_min(1e-38)).max())
        print(f"mean pooling {precision}: worst difference {ulps:.2f} ulp (gate {T})")
        assert ulps <= T
    # the per-step loop on the same hidden states, its candidates' actions captured
    cap = {}
    orig = DeerEngine._values_from_actions

    def spy(a, ttype):
        cap["a"] = a.clone()
        return orig(a, ttype)
    monkeypatch.setattr(DeerEngine, "_values_from_actions", staticmethod(spy))
    rl = _rand_layers(exit_ids, bs, W, 4)
    hid_b = hid.view(bs, W, *hid.shape[1:])
    for ttype in ("L2", "mean", "max"):
        v_loop = eng.generate_values(hid_b, rl, ttype)
        v, a = eng.calibrate_values(feats.view(bs, W, *feats.shape[1:]), rl, ttype, return_actions=True)
        ea = float((a.cpu()[..., :6 * eng.A] - cap["a"]).abs().max())
        ev = float((v.cpu() - v_loop).abs().max())
        print(f"{pooling} {precision} {ttype}: |actions-loop|={ea:.3e} |values-loop|={ev:.3e}")
        assert ea < 1e-4 and ev < 2e-4, (ttype, ea, ev)


# ---- 4. chunking and determinism ------------------------------------------------------------------------------------------------------
def _chunking(bs, W, ttype):
    cfg = _small_towers(deer_tiny())
    eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, 3, bf16_round=True))
    exit_ids = cfg.exit_ids()
    NL = len(exit_ids) + 1
    assert bs * (W - 1) > 2048 and (bs // 2) * (W - 1) <= 2048                        # the full call runs in two chunks, each half in one
    P = torch.randn(bs, W, NL, cfg.d_model, generator=torch.Generator().manual_seed(1)).cuda()
    rl = _rand_layers(exit_ids, bs, W, 2)
    eng.h_state.normal_()
    eng.c_state.normal_()
    eng.ctl.fill_(7)
    snap = [t.clone() for t in (eng.h_state, eng.c_state, eng.ctl)]
    v, a = eng.calibrate_values(P, rl, ttype, return_actions=True)
    v2, a2 = eng.calibrate_values(P, rl, ttype, return_actions=True)
    hb = bs // 2
    va, aa = eng.calibrate_values(P[:hb], rl[:hb], ttype, return_actions=True)
    vb, ab = eng.calibrate_values(P[hb:], rl[hb:], ttype, return_actions=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0
    assert torch.equal(v, v2) and torch.equal(a, a2)                                  # identical calls, identical bits
    assert torch.equal(v, torch.cat([va, vb], dim=1)) and torch.equal(a, torch.cat([aa, ab], dim=1))
    for now, before in zip((eng.h_state, eng.c_state, eng.ctl), snap):
        assert torch.equal(now, before)
    S = W - W // 2
    for b in (5, bs - 1):                                                             # one window (W, NL, d) == its columns of the batch
        assert torch.equal(eng.calibrate_values(P[b], rl[b], ttype), v[:, b * S:(b + 1) * S])


def test_chunking_determinism_and_untouched_state():
    _chunking(190, 12, "L2")                                                          # chunks of 186 + 4 windows


def test_chunking_odd_window_ragged_last_chunk():
    """W = 11 (S = 6 of 10 history steps per window): chunks of 204 + 46 windows, the `max` criterion"""
    _chunking(250, 11, "max")


# ---- 5. full size -----------------------------------------------------------------------------------------------------------------------
def _window_reference(cfg, sd, frames, W):
    """oracle hidden states of every layer for every frame of every window: (bs, W, L, T, d)"""
    model = orc.OracleDeer(sd, cfg)
    model.set_all_exit_window_size(1)                       # the head call behind the static exit is a single step (its output is not used)
    out = []
    for fr in frames:
        hid = []
        for t in range(W):
            rgb, grip, ids_t, mask = fr[t]
            h = model.forward(rgb, ids_t, mask, grip, exit_id=cfg.n_layers - 1)["hidden_states"]   # memoised per input (conftest.py)
            hid.append(torch.stack([x[0] for x in h]))
        model.clear_all_exit_memory()
        out.append(torch.stack(hid))
    return torch.stack(out)


def test_full_size_3b_window_vs_oracle():
    """the construction of test_engine_parity._window_full_size_vs_oracle (max_layer = 12), through the pooled features"""
    cfg = deer_3b(max_layer=12)
    sd = full_size_state(cfg, 0, std="0.02", bf16_round=True)
    eng = DeerEngine(cfg, sd)
    W = 12
    exit_ids = cfg.exit_ids()
    frames = [[syn.synthetic_step_inputs(cfg, 100 + t) for t in range(W)]]
    S = cfg.image_size
    images = torch.stack([f[0].reshape(3, S, S) for f in frames[0]]).cuda().to(eng.img_dtype)
    gripper = torch.stack([f[1].reshape(3, S, S) for f in frames[0]]).cuda().to(eng.img_dtype)
    ids = frames[0][0][2].cuda()
    eng.configure_exit(exit_ids, 12, 1)
    feats = eng.window_exit_features(images, gripper, ids, None)                 # (W, NL, d): two groups of 8 / 4 frames
    ref = _window_reference(cfg, sd, frames, W)                                  # (1, W, L, T, d)
    g = torch.Generator().manual_seed(4)
    rl = torch.tensor([[exit_ids[int(i)] for i in torch.randint(0, len(exit_ids), (W,), generator=g)]])
    vals = eng.calibrate_values(feats, rl[0], "L2").cpu()
    head = _ZeroStartHead(sd, cfg, "extra_exit.")
    vref, _ = _oracle_generate(head, exit_ids, ref, rl, "L2")
    err = float((vals - vref).abs().max())
    print(f"3B, one 12-step window: |values-oracle|={err:.3e}")
    assert vals.shape == vref.shape == (len(exit_ids), W - W // 2)
    assert err < GATE16


def test_full_size_9b_head_width_vs_oracle():
    """the head of the default 9B model (d = 4096, 13 layers, seven exits) on one 12-step window of random hidden states"""
    c9 = deer_9b()
    cfg = _small_towers(deer_tiny(), d_model=c9.d_model, n_heads=c9.d_model // 128, mlp_ratio=1, head_hidden=c9.head_hidden,
                        lstm_num_layers=c9.lstm_num_layers, mlp_num_hidden_layers=c9.mlp_num_hidden_layers, n_layers_total=c9.n_layers,
                        early_exit_layer=c9.early_exit_layer, exit_interval=c9.exit_interval, vocab_size=100, media_token_id=98, eoc_token_id=97)
    exit_ids = cfg.exit_ids()
    assert exit_ids == c9.exit_ids() and len(exit_ids) == 7
    sd = syn.make_synthetic_state(cfg, 7, bf16_round=True)
    eng = DeerEngine(cfg, sd)
    W, T = 12, 4
    hid = torch.randn(1, W, cfg.n_layers, T, cfg.d_model, generator=torch.Generator().manual_seed(9))
    rl = _rand_layers(exit_ids, 1, W, 9)
    vals = eng.calibrate_values(_pool(hid, [0] + exit_ids, cfg.pooling).cuda(), rl, "L2").cpu()
    vref, _ = _oracle_generate(_ZeroStartHead(sd, cfg, "extra_exit."), exit_ids, hid, rl, "L2")
    err = float((vals - vref).abs().max())
    print(f"9B head width, one 12-step window: |values-oracle|={err:.3e}")
    assert vals.shape == vref.shape == (7, W - W // 2)
    assert err < GATE16


def test_generate_action_values_fused_end_to_end():
    cfg = deer_tiny()
    eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, 3, bf16_round=True))
    exit_ids, W = cfg.exit_ids(), 8
    eng.configure_exit(exit_ids, 12, 1)

    class _M:                                                           # the bits of MPTFlamingo generate_action_values touches
        def __init__(self, e):
            self.module, self.engine = self, e
    loader = [_window_batch(cfg, 2, W, 0), _window_batch(cfg, 3, W, 40)]
    vn = ActionValueNet(exit_ids, None, cfg.exit_interval, W, "L2")
    v0, _ = generate_action_values(None, _M(eng), vn, loader, generator=torch.Generator().manual_seed(4))
    v1, _ = generate_action_values(None, _M(eng), vn, loader, generator=torch.Generator().manual_seed(4), fused=True)
    assert v1.is_cuda and v0.shape == v1.shape == (len(exit_ids), 5 * (W - W // 2))
    err = float((v1.cpu() - v0).abs().max())
    print(f"fused vs unfused values: {err:.3e}")
    assert err < 2e-4
    for ratio in (0.6, 1.0):
        t0 = solve_thresholds(v0, len(exit_ids), ratio)
        t1 = solve_thresholds(v1, len(exit_ids), ratio)
        rel = float(((t1 - t0).abs() / t0.abs()).max())
        print(f"exit_ratio {ratio}: thresholds {t0.tolist()} vs {t1.tolist()} (relative {rel:.3e})")
        assert rel < 1e-3
