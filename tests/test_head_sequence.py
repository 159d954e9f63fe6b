"""Window mode of the action head on the device (DeterministicDecoder.forward on feature sequences, action_head.py:499-611): the
spine call ``deer_head_sequence`` (csrc/head_seq.hip) through the reference-shaped handle, the engine and the torch op, against the
reference's recorded outputs, the oracle head and the engine's per-step head evaluation."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load, s2str  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.engine import DeerEngine  # noqa: E402
from deer_vla_amd.action_head import DeterministicDecoder  # noqa: E402
from oracle import deer_oracle as orc  # noqa: E402


def _head_only_cfg(cfg, **kw):
    """tower dims the engine can be built with around a head configuration (the head's tensors are seeded by name)"""
    return dataclasses.replace(cfg, vit_width=128, vit_heads=2, vit_layers=1, vit_mlp=256, image_size=28, perc_heads=2, perc_dim_head=64,
                               perc_latents=8, perc_depth=1, xattn_heads=2, xattn_dim_head=64, n_layers_total=4, early_exit_layer=1, **kw)


def _rounded(cfg, sd, precision):
    if precision == "fp32":
        return sd
    return syn.round_state_to_bf16(cfg, sd) if precision == "bf16" else syn.round_state_to_fp16(cfg, sd)


def _oracle_window(o, feats, h0=None):
    """OracleHead's window mode with the LSTM output kept: feats (N, L, T, d) -> (pooled (N, L, d), x (N, L, H), (h_n, c_n))"""
    cfg = o.cfg
    p = feats.amax(2) if cfg.pooling == "max" else feats.mean(2)
    state, outs = h0, []
    for t in range(p.shape[1]):
        y, state = orc.head_rnn_step(o.sd, cfg, o.prefix, p[:, t], state)
        outs.append(y)
    return p, torch.stack(outs, 1), state


# ---- 1. the reference's own window outputs (tests/golden/head_*.npz) -----------------------------------------------------------------
@pytest.mark.parametrize("precision,tol", [("fp32", 2e-5), ("fp16", 2e-3), ("bf16", 2e-3)])
@pytest.mark.parametrize("name", ["head_ln.npz", "head_plain.npz", "head_avg3.npz"])
def test_window_mode_matches_reference_decoder(name, precision, tol):
    cfg0, seed, g = load(name)
    sd = syn.make_synthetic_state(_head_only_cfg(cfg0), seed)
    W = cfg0.window_size
    exp = {k: g[k] for k in ("wpose", "wgrip", "wpose_last", "wgrip_last", "wgrip_logits")}
    if precision != "fp32":                  # the weights the engine holds, through the oracle head (pinned by test_oracle_golden.py)
        o = orc.OracleHead(_rounded(cfg0, syn.make_synthetic_state(cfg0, seed), precision), cfg0)
        o.window_size = W
        exp["wpose"], exp["wgrip"] = o(g["wfeat"])
        o.last_action = True
        exp["wpose_last"], (exp["wgrip_last"], exp["wgrip_logits"]) = o(g["wfeat"], with_gripper_logits=True)
    eng = DeerEngine(_head_only_cfg(cfg0), sd, precision=precision)
    head = DeterministicDecoder(eng, window_size=W)
    pose, grip = head(g["wfeat"].cuda())                                    # (bs * window_size, T, d)
    assert pose.shape == exp["wpose"].shape and grip.shape == exp["wgrip"].shape
    assert float((pose.cpu() - exp["wpose"]).abs().max()) < tol
    assert float((grip.cpu() - exp["wgrip"]).abs().max()) < tol
    head.last_action = True
    pose, (grip, logit) = head(g["wfeat"].view(2, W, *g["wfeat"].shape[1:]).cuda(), with_gripper_logits=True)   # (bs, L, T, d)
    assert pose.shape == exp["wpose_last"].shape == (2, 1, 6)
    assert float((pose.cpu() - exp["wpose_last"]).abs().max()) < tol
    assert float((grip.cpu() - exp["wgrip_last"]).abs().max()) < tol
    assert float((logit.cpu() - exp["wgrip_logits"]).abs().max()) < 4 * tol


# ---- 2. the reference's ActionValueNet(mode='generate') with the native handle as its exit head ------------------------------------
@pytest.mark.parametrize("precision,tol", [("fp16", 5e-3), ("fp32", 1e-4)])
def test_value_net_generate_with_native_exit_head(precision, tol):
    cfg0, seed, g = load("valuenet_generate.npz")
    eng = DeerEngine(_head_only_cfg(cfg0), syn.make_synthetic_state(_head_only_cfg(cfg0), seed), precision=precision)
    head = DeterministicDecoder(eng, window_size=cfg0.window_size)
    vn = orc.OracleValueNet(cfg0.exit_ids(), head, cfg0.exit_interval, cfg0.window_size, s2str(g["threshold_type"]))
    feats, rl = g["feats"].cuda(), g["rand_layers"]
    rand_feat = torch.stack([feats[int(rl[j]), j] for j in range(feats.shape[1])])
    delta = vn(tuple(feats[l] for l in range(feats.shape[0])), mode="generate", rand_layer_feat=rand_feat)
    assert delta.shape == g["delta"].shape
    assert float((delta.cpu() - g["delta"]).abs().max()) < tol


# ---- 3. agreement with the per-step head evaluation at full size ----------------------------------------------------------------------
def _full_cfg(d):
    base = _head_only_cfg(load("head_ln.npz")[0])
    return dataclasses.replace(base, d_model=d, n_heads=d // 128, mlp_ratio=1, head_hidden=1024, lstm_num_layers=4, lstm_layernorm=True,
                               mlp_layernorm=True, mlp_num_hidden_layers=3, vocab_size=100, media_token_id=98, eoc_token_id=97)


_ENGINES = {}


def _full_engine(d, precision):
    key = (d, precision)
    if key not in _ENGINES:
        _ENGINES.clear()
        cfg = _full_cfg(d)
        _ENGINES[key] = DeerEngine(cfg, syn.make_synthetic_state(cfg, 7), precision=precision)
    return _ENGINES[key]


def _step_loop(eng, feats, h0, c0):
    """the per-step path: DeerEngine._head_eval on siblings of <= 16 sequences, one call per time step, the state committed"""
    N, L = feats.shape[:2]
    acts, hs, cs = [], [], []
    for n0 in range(0, N, 16):
        n = min(16, N - n0)
        w = eng.sibling(n)
        w.h_state.copy_(h0[:, n0:n0 + n])
        w.c_state.copy_(c0[:, n0:n0 + n])
        w._head_state_changed()
        rows = [w._head_eval(feats[n0:n0 + n, t].reshape(-1, feats.shape[-1]).contiguous(), commit=True) for t in range(L)]
        acts.append(torch.stack(rows, 1))
        hs.append(w.h_state.clone())
        cs.append(w.c_state.clone())
    return torch.cat(acts, 0), torch.cat(hs, 1), torch.cat(cs, 1)


def _feats(N, L, T, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, L, T, d, generator=g).cuda()


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_sequence_matches_step_path_3b(precision):
    eng = _full_engine(2048, precision)
    cfg = eng.cfg
    Lh, H = cfg.lstm_num_layers, cfg.head_hidden
    worst = 0.0
    for N in (1, 16, 64, 200):
        for L in (1, 12):
            for nz in (False, True):
                g = torch.Generator().manual_seed(N * 100 + L)
                h0 = (0.5 * torch.randn(Lh, N, H, generator=g)).cuda() if nz else torch.zeros(Lh, N, H, device="cuda")
                c0 = (0.5 * torch.randn(Lh, N, H, generator=g)).cuda() if nz else torch.zeros(Lh, N, H, device="cuda")
                f = _feats(N, L, 5, cfg.d_model, N + L)
                a, h_n, c_n = eng.head_sequence(f, h0 if nz else None, c0 if nz else None)
                ra, rh, rc = _step_loop(eng, f, h0, c0)
                err = max(float((a - ra).abs().max()), float((h_n - rh).abs().max()), float((c_n - rc).abs().max()))
                worst = max(worst, err)
                assert err < 1e-4, (N, L, nz, err)
    print(f"max |sequence - step loop| at 3B width ({precision}): {worst:.2e}")


def test_sequence_matches_oracle_fp32_3b():
    eng = _full_engine(2048, "fp32")
    cfg = eng.cfg
    sd = syn.make_synthetic_state(cfg, 7)
    o = orc.OracleHead(sd, cfg)
    f = _feats(16, 12, 5, cfg.d_model, 3)
    a, h_n, c_n = eng.head_sequence(f)
    _, x, (rh, rc) = _oracle_window(o, f.cpu())
    pose = orc.head_mlp(sd, cfg, "extra_exit.actions.", x, "tanh")
    grip, logit = orc.head_mlp(sd, cfg, "extra_exit.gripper.", x, "sigmoid", True)
    assert float((a[..., :6].cpu() - pose).abs().max()) < 1e-4
    assert float((a[..., 6:7].cpu() - grip).abs().max()) < 1e-4
    assert float((a[..., 7:8].cpu() - logit).abs().max()) < 1e-3
    assert float((h_n.cpu() - rh).abs().max()) < 1e-4 and float((c_n.cpu() - rc).abs().max()) < 1e-4


def test_sequence_matches_step_path_9b_width():
    eng = _full_engine(4096, "fp16")
    cfg = eng.cfg
    f = _feats(16, 12, 5, cfg.d_model, 9)
    z = torch.zeros(cfg.lstm_num_layers, 16, cfg.head_hidden, device="cuda")
    a, h_n, c_n = eng.head_sequence(f)
    ra, rh, rc = _step_loop(eng, f, z, z)
    err = max(float((a - ra).abs().max()), float((h_n - rh).abs().max()), float((c_n - rc).abs().max()))
    assert err < 1e-4, err


# ---- 4. variants against the oracle head (fp32 arithmetic) -------------------------------------------------------------------------------
VARIANTS = [("head_avg3.npz", {}), ("head_plain.npz", {}), ("head_ln.npz", {}), ("head_ln.npz", dict(multi_step_action=3)),
            ("head_ln.npz", dict(use_state=True))]


@pytest.mark.parametrize("name,kw", VARIANTS)
def test_sequence_variants_match_oracle(name, kw):
    cfg0, seed, _ = load(name)
    cfg = _head_only_cfg(cfg0, **kw)
    sd = syn.make_synthetic_state(cfg, seed)
    eng = DeerEngine(cfg, sd, precision="fp32")
    N, L, T = 3, 5, 4
    f = _feats(N, L, T, cfg.d_model, 11)
    state = None
    if cfg.use_state:
        g = torch.Generator().manual_seed(5)
        state = torch.randn(N, L, 15, generator=g)
        state[..., -1] = torch.where(torch.rand(N, L, generator=g) > 0.5, 1.0, -1.0)
    o = orc.OracleHead(sd, cfg)
    o.window_size = L
    head = DeterministicDecoder(eng, window_size=L)
    A = max(1, cfg.multi_step_action)
    pose, grip, org = head(f, state_tensor=state, return_feature=True)
    rp, rg = o(f.cpu(), state_tensor=state)
    assert pose.shape == rp.shape == (N, L, 6 * A) and grip.shape == rg.shape == (N, L, A)
    assert float((pose.cpu() - rp).abs().max()) < 1e-4 and float((grip.cpu() - rg).abs().max()) < 1e-4
    assert org.shape == (N, L, cfg.d_model)
    if not cfg.use_state:
        p, x, _ = _oracle_window(o, f.cpu())
        assert float((org.cpu() - p).abs().max()) < 1e-6
        _, _, agg = head(f, return_aggregate_feature=True)
        assert agg.shape == (N, L, cfg.head_hidden) and float((agg.cpu() - x).abs().max()) < 1e-4
        head.last_action = True
        _, _, agg = head(f, return_aggregate_feature=True)
        assert agg.shape == (N, 1, cfg.head_hidden) and float((agg.cpu() - x[:, -1:]).abs().max()) < 1e-4
    # state rows as (bs * L, 15) give the same result
    if cfg.use_state:
        pose2, _ = head(f, state_tensor=state.reshape(N * L, 15))
        assert torch.equal(pose2, pose)


def test_sequence_layerwise_head_matches_oracle():
    cfg0, seed, _ = load("head_ln.npz")
    cfg = _head_only_cfg(cfg0, layerwise_exit_eval=True)
    sd = syn.make_synthetic_state(cfg, seed)
    eng = DeerEngine(cfg, sd, precision="fp32")
    f = _feats(2, 6, 3, cfg.d_model, 12)
    for k, (prefix, layer) in enumerate(cfg.layerwise_heads(), start=1):
        assert eng.lib.deer_model_layerwise_head(eng._h, layer) == k
        a, h_n, _ = eng.head_sequence(f, head=k)
        o = orc.OracleHead(sd, cfg, prefix=prefix)
        o.window_size = 6
        rp, rg = o(f.cpu())
        assert float((a[..., :6].cpu() - rp).abs().max()) < 1e-4 and float((a[..., 6:7].cpu() - rg).abs().max()) < 1e-4
        assert float((h_n.cpu() - o.hidden_state[0]).abs().max()) < 1e-4
    from deer_vla_amd import _abi as abi
    with pytest.raises(abi.DeerHipError):                                   # a head the model lacks
        eng.head_sequence(f, head=len(cfg.layerwise_heads()) + 1)


# ---- 5. hard inputs: outlier channels past the fp16 range -----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_sequence_outlier_features_stay_finite(precision):
    cfg0, seed, _ = load("head_ln.npz")
    cfg = _head_only_cfg(cfg0)
    eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, seed), precision=precision)
    f = _feats(4, 6, 5, cfg.d_model, 13)
    f[:, :, :, 3] = 1.0e5
    f[:, :, 2, 7] = -7.0e4
    f[:, 1, :, 11] = 3.0e5
    a, h_n, c_n = eng.head_sequence(f)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(h_n).all()) and bool(torch.isfinite(c_n).all())
    z = torch.zeros(cfg.lstm_num_layers, 4, cfg.head_hidden, device="cuda")
    ra, rh, _ = _step_loop(eng, f, z, z)
    assert float((a - ra).abs().max()) < 1e-3 and float((h_n - rh).abs().max()) < 1e-3


# ---- 6. state semantics --------------------------------------------------------------------------------------------------------------
def test_window_call_state_semantics():
    cfg0, seed, g = load("head_ln.npz")
    cfg = _head_only_cfg(cfg0)
    sd = syn.make_synthetic_state(cfg, seed)
    eng = DeerEngine(cfg, sd, precision="fp32")
    head = DeterministicDecoder(eng, window_size=12)
    head(g["wfeat"].cuda())                                                  # 2 sequences, the engine runs 1
    o = orc.OracleHead(syn.make_synthetic_state(cfg0, seed), cfg0)
    o.window_size = 12
    o(g["wfeat"])
    hs = head.hidden_state
    assert hs[0].shape == (cfg.lstm_num_layers, 2, cfg.head_hidden)
    assert float((hs[0].cpu() - o.hidden_state[0]).abs().max()) < 2e-5 and float((hs[1].cpu() - o.hidden_state[1]).abs().max()) < 2e-5
    with pytest.raises(RuntimeError):
        head(g["feats"][0].cuda())
    head.clear_hidden_state()
    for t in range(g["feats"].shape[0]):                                     # the step results of the fixture, unchanged
        a, gr = head(g["feats"][t].cuda(), update_hidden_state=bool(g["upd"][t]))
        assert float((a.cpu() - g["pose"][t]).abs().max()) < 2e-5 and float((gr.cpu() - g["grip"][t]).abs().max()) < 2e-5
    # one sequence: h_n becomes the engine's committed state and the next step continues from it (as the reference's)
    head.clear_hidden_state()
    w1 = g["wfeat"][:12].view(1, 12, *g["wfeat"].shape[1:])
    head(w1.cuda())
    o.hidden_state = None
    o(w1)
    assert float((eng.h_state.cpu() - o.hidden_state[0]).abs().max()) < 2e-5
    a, _ = head(g["feats"][0].cuda())
    o.window_size = 1
    ra, _ = o(g["feats"][0])
    assert float((a.cpu() - ra).abs().max()) < 2e-5
    # engine reset drops a held window state too
    head(g["wfeat"].cuda())
    eng.reset()
    assert head.hidden_state is None
    head(g["feats"][0].cuda())


# ---- 7. determinism + the torch op ---------------------------------------------------------------------------------------------------
def test_sequence_deterministic_and_torch_op():
    from deer_vla_amd import ops
    eng = _full_engine(2048, "fp16")
    cfg = eng.cfg
    f = _feats(64, 12, 5, cfg.d_model, 21)
    h0 = torch.randn(cfg.lstm_num_layers, 64, cfg.head_hidden, device="cuda")
    a1 = eng.head_sequence(f, h0, h0)
    a2 = eng.head_sequence(f, h0, h0)
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)
    sd = syn.make_synthetic_state(cfg, 7)
    nm = ops.NativeModel(cfg, sd, precision="fp16")
    try:
        out = torch.ops.deer.action_head_sequence(f, h0, h0, nm.handle, 0, True)
        assert out[0].shape == (64, 1, 8) and out[1].shape == h0.shape
        assert torch.equal(out[0], a1[0][:, -1:]) and torch.equal(out[1], a1[1]) and torch.equal(out[2], a1[2])
    finally:
        nm.close()
