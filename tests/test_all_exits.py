"""The all-exits window forward (flamingo_mpt.py:463-517) and the per-exit demonstration loss on the GPU, against the reference's own
forward with ``multi_exit=True`` (tests/golden/all_exits*.npz, made by tests/golden/make_all_exits_golden.py).

Gates.  Head-only inputs (the golden's pooled exit-layer features through ``DeerEngine.exit_outputs``): the tolerances of
test_head_sequence.py::test_window_mode_matches_reference_decoder for the same arithmetics - 2e-5 (fp32) / 2e-3 (fp16, bf16) on pose and
gripper probability, four times that on the logit.  End to end (frames through ``MPTFlamingo.forward``): the gates of the padded-window
parity test of tests/test_variant_parity.py (ACTION_TOL, 1e-3 in fp32) on pose and gripper probability.  Losses: Huber(delta = 1) and
BCE-with-logits are 1-Lipschitz in the prediction, so a head's per-row num / bin differ from the golden's by at most the pose / logit
error measured in the same run (plus the f32 rounding of the loss kernel itself, bounded in tests/test_exit_eval_kernels.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load  # noqa: E402
from test_variant_parity import ACTION_TOL  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_tiny  # noqa: E402
from deer_vla_amd.engine import DeerEngine  # noqa: E402
from deer_vla_amd.flamingo_mpt import MPTFlamingo  # noqa: E402

HEAD_TOL = {"fp32": 2e-5, "fp16": 2e-3, "bf16": 2e-3}
LOSS_ROUNDING = 64 * 2.0 ** -24                    # the loss kernel's own f32 error on O(1) terms (test_exit_eval_kernels.py: < (6 A + 3) u)
STEP_VS_SEQUENCE = 1e-4                            # test_head_sequence.py::test_sequence_matches_step_path_3b

_models = {}


def _model(name, precision):
    """one model per (golden, precision) for the module; READ-ONLY use"""
    key = (name, precision)
    if key not in _models:
        cfg, seed, g = load(name)
        sd = syn.make_synthetic_state(cfg, seed, bf16_round=True)
        _models[key] = (cfg, g, MPTFlamingo(cfg, sd, window_size=cfg.window_size, precision=precision))
    return _models[key]


def _window_kwargs(cfg, g):
    W, S = cfg.window_size, cfg.image_size
    bs, T = g["ids"].shape
    kw = dict(vision_x=g["rgb"].reshape(bs * W, 1, 1, 3, S, S), vision_gripper=g["grip"].reshape(bs * W, 1, 1, 3, S, S),
              lang_x=g["ids"].long().unsqueeze(1).repeat(1, W, 1).flatten(0, 1),
              attention_mask=g["mask"].bool().unsqueeze(1).repeat(1, W, 1).flatten(0, 1))
    if cfg.use_state:
        kw["state_tensor"] = g["state"].unsqueeze(2).unsqueeze(2).flatten(0, 1)               # (bs W, 1, 1, 15), train_utils.py:470-475
    return kw


def _golden_heads(cfg, g):
    """the golden's heads this repository's model of `cfg` carries: all of them, or (use_state: no per-layer heads are built with it, and
    the reference's lm_head has weights of its own) extra_exit on the two strategies"""
    Hn = g["pose"].shape[0]
    return list(range(Hn)) if cfg.layerwise_exit_eval else [Hn - 2, Hn - 1]


def _errors(acts, cfg, g, heads, engine_heads):
    A = max(1, cfg.multi_step_action)
    a = acts.cpu()[engine_heads]
    e_pose = float((a[..., :6 * A] - g["pose"][heads]).abs().max())
    e_prob = float((a[..., 6 * A:7 * A] - g["gprob"][heads]).abs().max())
    e_logit = float((a[..., 7 * A:] - g["glogit"][heads]).abs().max())
    return e_pose, e_prob, e_logit


def _engine_heads(cfg, acts):
    return list(range(acts.shape[0])) if cfg.layerwise_exit_eval else [acts.shape[0] - 2, acts.shape[0] - 1]


def _check_losses(eng, acts, cfg, g, heads, engine_heads, e_pose, e_logit):
    """(b): per-row num / bin and per-head loss against torch.nn.functional on the reference's outputs, gated on the measured errors"""
    num, bin_, loss = eng.exit_losses(acts, g["label_pose"], g["label_grip01"], float(g["w_bin"]))
    bs, W = g["rand_layers"].shape
    num, bin_, loss = num.cpu().view(-1, bs, W)[engine_heads], bin_.cpu().view(-1, bs, W)[engine_heads], loss.cpu()[engine_heads]
    d_num, d_bin = float((num - g["num"][heads]).abs().max()), float((bin_ - g["bin"][heads]).abs().max())
    d_loss = float((loss - g["loss"][heads]).abs().max())
    print(f"  losses: |d num| {d_num:.2e} (pose err {e_pose:.2e}), |d bin| {d_bin:.2e} (logit err {e_logit:.2e}), |d loss| {d_loss:.2e}")
    assert d_num <= e_pose + LOSS_ROUNDING and d_bin <= e_logit + LOSS_ROUNDING * 8
    assert d_loss <= e_pose + float(g["w_bin"]) * e_logit + LOSS_ROUNDING


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["all_exits.npz", "all_exits_ms2.npz", "all_exits_state.npz"])
def test_heads_on_golden_features_match_reference(name, precision):
    """(a) head-only, (b), (e): every head on the reference's pooled features with the reference's layer tables"""
    cfg, g, model = _model(name, precision)
    eng = model.engine
    bs, W = g["rand_layers"].shape
    feats = g["pooled"].view(bs, W, *g["pooled"].shape[1:]).cuda()
    acts = eng.exit_outputs(feats, g["rand_layers"], g["two_layers"], state=g["state"] if cfg.use_state else None)
    A = max(1, cfg.multi_step_action)
    heads, eh = _golden_heads(cfg, g), _engine_heads(cfg, acts)
    assert acts.shape == ((g["pose"].shape[0] if cfg.layerwise_exit_eval else 3), bs, W, 8 * A)
    e_pose, e_prob, e_logit = _errors(acts, cfg, g, heads, eh)
    print(f"{name} {precision} head-only: pose {e_pose:.2e} prob {e_prob:.2e} logit {e_logit:.2e}")
    tol = HEAD_TOL[precision]
    assert e_pose < tol and e_prob < tol and e_logit < 4 * tol
    _check_losses(eng, acts, cfg, g, heads, eh, e_pose, e_logit)
    acts2 = eng.exit_outputs(feats, g["rand_layers"], g["two_layers"], state=g["state"] if cfg.use_state else None)
    assert torch.equal(acts, acts2)


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("name", ["all_exits.npz", "all_exits_ms2.npz", "all_exits_state.npz"])
def test_forward_all_exits_matches_reference_end_to_end(name, precision):
    """(a) end to end, (b), (e): the four-tuple of MPTFlamingo.forward in the reference's layout, frames in, with the reference's tables"""
    cfg, g, model = _model(name, precision)
    bs, W = g["rand_layers"].shape
    A = max(1, cfg.multi_step_action)
    kw = _window_kwargs(cfg, g)
    out, exit_outputs, extra, extra2 = model._forward_all_exits(kw["vision_x"], kw["lang_x"], kw["attention_mask"], kw["vision_gripper"],
                                                                kw.get("state_tensor"), with_gripper_logits=True,
                                                                rand_layers=g["rand_layers"], two_layers=g["two_layers"])
    n_exit = len(cfg.exit_ids()) - 1 if cfg.layerwise_exit_eval else 0
    assert len(exit_outputs) == n_exit and len(out.hidden_states) == cfg.n_layers and out.exit_layer == cfg.n_layers - 1
    allo = exit_outputs + [out.logits, extra, extra2]
    for pose, (prob, logit) in allo:
        assert pose.shape == (bs, W, 6 * A) and prob.shape == logit.shape == (bs, W, A)
    acts = torch.stack([torch.cat([p, pr, lg], dim=-1) for p, (pr, lg) in allo])
    heads, eh = _golden_heads(cfg, g), _engine_heads(cfg, acts)
    e_pose, e_prob, e_logit = _errors(acts, cfg, g, heads, eh)
    print(f"{name} {precision} end to end: pose {e_pose:.2e} prob {e_prob:.2e} logit {e_logit:.2e}")
    tol = ACTION_TOL if precision != "fp32" else 1e-3
    assert e_pose < tol and e_prob < tol
    _check_losses(model.engine, acts, cfg, g, heads, eh, e_pose, e_logit)


def test_public_forward_returns_the_reference_tuples_and_draws_like_the_reference():
    """the four- and five-tuple of ``forward`` itself; (d): with the generators seeded like the golden's call, the host draws the
    reference's tables (strategy 2 constant in each of its two segments) - so the public call equals the explicit-table call bit for bit"""
    import random
    cfg, g, model = _model("all_exits.npz", "fp16")
    kw = _window_kwargs(cfg, g)
    ref = model._forward_all_exits(kw["vision_x"], kw["lang_x"], kw["attention_mask"], kw["vision_gripper"], None, with_gripper_logits=True,
                                   rand_layers=g["rand_layers"], two_layers=g["two_layers"])
    torch.manual_seed(int(g["torch_seed"]))
    random.seed(int(g["py_seed"]))
    out, exit_outputs, extra, extra2 = model(with_gripper_logits=True, **kw)
    assert torch.equal(extra[0], ref[2][0]) and torch.equal(extra2[0], ref[3][0]) and torch.equal(extra2[1][1], ref[3][1][1])
    assert torch.equal(out.logits[0], ref[0].logits[0]) and all(torch.equal(a[0], b[0]) for a, b in zip(exit_outputs, ref[1]))
    torch.manual_seed(int(g["torch_seed"]))
    random.seed(int(g["py_seed"]))
    rl, tl = model.draw_exit_layers(*g["rand_layers"].shape)
    assert torch.equal(rl, g["rand_layers"]) and torch.equal(tl, g["two_layers"])
    p = int(g["prev_len"])
    assert bool((tl[:, :p] == tl[:, :1]).all()) and bool((tl[:, p:] == tl[:, p:p + 1]).all())
    torch.manual_seed(int(g["torch_seed"]))
    random.seed(int(g["py_seed"]))
    out5 = model(return_in_feat=True, **kw)                                                   # (pose, gripper) without logits
    assert len(out5) == 5 and out5[3].shape == (kw["vision_x"].shape[0], g["ids"].shape[1], cfg.d_model)
    assert torch.equal(out5[4].cpu(), g["rand_layers"]) and torch.equal(out5[2][0], ref[2][0]) and out5[2][1].shape == ref[2][1][0].shape
    hid = torch.stack(out5[0].hidden_states)                                                  # rand_layer_feat is the hidden state of the drawn layer
    F = hid.shape[1]
    assert torch.equal(out5[3], hid[g["rand_layers"].reshape(-1).cuda(), torch.arange(F, device=hid.device)])


@pytest.mark.parametrize("cfg", [deer_tiny(), deer_tiny(llm_name="mpt_9b", attn_qk_ln=False, cross_attn_every_n_layers=4, n_layers_total=12, early_exit_layer=9)], ids=["3b-tiny", "9b-tiny"])
def test_model_without_per_layer_heads_runs_the_three_remaining_heads(cfg):
    """3B- and 9B-shaped tiny configs without per-layer heads: no exit_outputs; the last layer's head is extra_exit on the last layer"""
    import dataclasses
    cfg = dataclasses.replace(cfg, window_size=3)
    model = MPTFlamingo(cfg, syn.make_synthetic_state(cfg, 5, bf16_round=True), window_size=3)
    bs, W, S = 2, 3, cfg.image_size
    g = torch.Generator().manual_seed(0)
    ids = syn.synthetic_step_inputs(cfg, 0, text_len=7)[2].reshape(1, -1).repeat(bs * W, 1)
    vx, vg = torch.randn(bs * W, 1, 1, 3, S, S, generator=g), torch.randn(bs * W, 1, 1, 3, S, S, generator=g)
    out, exit_outputs, extra, extra2 = model(vision_x=vx, lang_x=ids, attention_mask=torch.ones_like(ids, dtype=torch.bool), vision_gripper=vg)
    assert exit_outputs == [] and len(out.hidden_states) == cfg.n_layers
    for pose, grip in (out.logits, extra, extra2):
        assert pose.shape == (bs, W, 6) and grip.shape == (bs, W, 1) and bool(torch.isfinite(pose).all())
    last = out.hidden_states[-1].view(bs, W, -1, cfg.d_model)
    a = model.engine.head_sequence(last)[0]
    assert torch.equal(a[..., :6], out.logits[0])
    assert len(model(vision_x=vx, lang_x=ids, attention_mask=None, vision_gripper=vg, return_in_feat=True)) == 5


def test_per_layer_heads_equal_head_sequence_on_their_layer():
    """(c): exit_outputs[k] (and the last layer's head) is head_sequence(head = k + 1) on that layer's unpooled features, bit for bit"""
    cfg, g, model = _model("all_exits.npz", "fp16")
    kw = _window_kwargs(cfg, g)
    acts, rl, tl, hid = model.all_exit_actions(kw["vision_x"], kw["lang_x"], kw["attention_mask"], kw["vision_gripper"],
                                               rand_layers=g["rand_layers"], two_layers=g["two_layers"], hidden=True)
    bs, W = g["rand_layers"].shape
    T = hid.shape[2]
    for k, layer in enumerate(cfg.exit_ids()):
        a = model.engine.head_sequence(hid[:, layer].reshape(bs, W, T, cfg.d_model).contiguous(), head=k + 1)[0]
        assert torch.equal(a, acts[k]), (k, layer)
    F = hid.shape[0]
    for s, tab in ((0, rl), (1, tl)):                                                         # and extra_exit on the mixed layers
        mixed = hid[torch.arange(F, device=hid.device), tab.reshape(-1).to(hid.device)]
        a = model.engine.head_sequence(mixed.reshape(bs, W, T, cfg.d_model).contiguous())[0]
        assert torch.equal(a, acts[len(cfg.exit_ids()) + s]), s


def test_use_state_window_calls_run():
    """(e): the old refusal is gone - the calibration call and the all-exits call of a use_state model run in window mode, and the state
    reaches the head (another state, other actions)"""
    cfg, g, model = _model("all_exits_state.npz", "fp16")
    kw = _window_kwargs(cfg, g)
    o5 = model(return_in_feat=True, only_extra_exit=True, with_gripper_logits=True, **kw)
    assert len(o5) == 5 and o5[1] == [] and o5[2][0].shape == (2, cfg.window_size, 6)
    a = model._forward_window(kw["vision_x"], kw["lang_x"], kw["attention_mask"], kw["vision_gripper"], with_gripper_logits=True,
                              rand_layers=g["rand_layers"], state_tensor=kw["state_tensor"])[2]
    Hn = g["pose"].shape[0]
    assert float((a[0].cpu() - g["pose"][Hn - 2]).abs().max()) < ACTION_TOL                  # strategy 1 = the reference's extra_exit_output
    b = model._forward_window(kw["vision_x"], kw["lang_x"], kw["attention_mask"], kw["vision_gripper"], with_gripper_logits=True,
                              rand_layers=g["rand_layers"], state_tensor=-kw["state_tensor"])[2]
    assert float((a[0] - b[0]).abs().max()) > 1e-4
    with pytest.raises(ValueError, match="state_tensor"):
        model(vision_x=kw["vision_x"], lang_x=kw["lang_x"], attention_mask=kw["attention_mask"], vision_gripper=kw["vision_gripper"])


def test_forward_window_equals_the_per_step_head_loop():
    """(f): _forward_window's single head_sequence call against the per-time-step ``_head_eval`` loop it replaced (groups of <= 8 windows
    as the environments of a sibling engine), for a fixed rand_layers"""
    cfg, g, model = _model("all_exits.npz", "fp16")
    e = model.engine
    kw = _window_kwargs(cfg, g)
    out, _, extra, rand_feat, rand_idx = model._forward_window(kw["vision_x"], kw["lang_x"], kw["attention_mask"], kw["vision_gripper"],
                                                               with_gripper_logits=True, rand_layers=g["rand_layers"])
    bs, Wn = g["rand_layers"].shape
    T = rand_feat.shape[1]
    G = max(1, min(8, e.MAX_ROWS // T, bs))
    w = e.sibling(G)
    rows = []
    rf = rand_feat.view(bs, Wn, T, cfg.d_model)
    for b0 in range(0, bs, G):
        gidx = [min(b0 + i, bs - 1) for i in range(G)]
        w.h_state.zero_()
        w.c_state.zero_()
        acts = [w._head_eval(rf[gidx, t].reshape(G * T, cfg.d_model).contiguous(), commit=True) for t in range(Wn)]
        rows.append(torch.stack(acts, dim=1)[: min(G, bs - b0)])
    a = torch.cat(rows, dim=0)                                                                # (bs, W, 8)
    got = torch.cat([extra[0], extra[1][0], extra[1][1]], dim=-1)
    err = float((got - a[..., :8]).abs().max())
    print(f"_forward_window vs the per-step loop: {err:.2e}")
    assert err < STEP_VS_SEQUENCE


def test_more_than_one_chunk_equals_two_calls():
    """(g): bs W > 2048 rows (the spine chunks by whole windows) on pooled features: the same rows as two calls, bit for bit"""
    cfg = deer_tiny(layerwise_exit_eval=True)
    eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, 2, bf16_round=True))
    bs, W = 700, 3
    exits = torch.tensor(cfg.exit_ids())
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(bs, W, len(exits), cfg.d_model, generator=g).cuda()
    rl, tl = exits[torch.randint(0, len(exits), (bs, W), generator=g)], exits[torch.randint(0, len(exits), (bs, W), generator=g)]
    whole = eng.exit_outputs(feats, rl, tl)
    assert whole.shape == (len(exits) + 2, bs, W, 8) and bool(torch.isfinite(whole).all())
    h = 350
    parts = torch.cat([eng.exit_outputs(feats[:h], rl[:h], tl[:h]), eng.exit_outputs(feats[h:], rl[h:], tl[h:])], dim=1)
    assert torch.equal(whole, parts)
    lo = eng.exit_losses(whole, torch.zeros(bs, W, 6), torch.ones(bs, W, 1))
    assert lo[0].shape == (len(exits) + 2, bs * W) and bool(torch.isfinite(lo[2]).all())
