"""End-to-end parity of the HIP engine (through libdeer_hip.so's C ABI) against
  (a) golden vectors produced by the REFERENCE's own MPTFlamingo.forward (tests/golden/deer_forward.npz), and
  (b) the CPU oracle on the same seeded inputs (tiny config: every step of an episode; full MPT-1B/ViT-L
      config: a few steps).
Tolerances (BASELINE.json north_star): action outputs within 1e-2 for the bf16 path, exit-layer indices EXACT.
The oracle / golden weights are the bf16-representable weights the engine holds, so the two arms differ only by
bf16 rounding of activations and summation order."""
import numpy as np

import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load, full_size_state  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_tiny, deer_3b  # noqa: E402
from deer_vla_amd.engine import DeerEngine  # noqa: E402
from deer_vla_amd import _abi as abi  # noqa: E402
from oracle import deer_oracle as orc  # noqa: E402

ACTION_TOL = 1e-2


def gap_threshold(vals, lo=0.2, hi=0.8):
    v = np.sort(np.asarray(vals, dtype=np.float64))
    a = int(len(v) * lo)
    b = min(max(int(len(v) * hi), a + 2), len(v))
    gaps = v[a + 1:b] - v[a:b - 1]
    i = int(np.argmax(gaps)) + a
    return float(0.5 * (v[i] + v[i + 1])), float(gaps.max())


class RecVN(orc.OracleValueNet):
    def __call__(self, feats, i=None, mode="infer", rand_layer_feat=None):
        v = super().__call__(feats, i, mode, rand_layer_feat)
        if not hasattr(self, "rec"):
            self.rec = []
        self.rec.append((i, float(v)))
        return v


def oracle_episode(cfg, sd, inputs, thresholds, max_layer, steps_per_stage=1):
    model = orc.OracleDeer(sd, cfg)
    model.set_all_exit_window_size(1)
    vn = RecVN(cfg.exit_ids(), model.extra_exit, cfg.exit_interval, 1, "L2")
    ctl = orc.OracleExitController(vn, cfg.exit_ids(), steps_per_stage=steps_per_stage, max_layer=max_layer)
    ctl._set_threshold_value(thresholds)
    outs = []
    for s, (rgb, grip, ids, mask) in enumerate(inputs):
        ctl.set_timestep(s)
        o = model.forward(rgb, ids, mask, grip, dynamic_early_exit=True, exit_controller=ctl)
        outs.append((o["exit_layer"], o["logits"][0].reshape(-1), float(o["logits"][1])))
    return outs, vn.rec, ctl


def min_margin(rec, thr_by_exit):
    m = [abs(v - thr_by_exit[i]) / thr_by_exit[i] for (i, v) in rec if thr_by_exit[i] < 1e4]
    return min(m) if m else 1.0


def probe_thresholds(cfg, sd, inputs, max_layer, sps=1, iters=5):
    """Thresholds with a wide safety margin: start in the widest gap of the oracle's never-exit deltas, then re-pick
    each threshold in the widest gap of the deltas the oracle's OWN policy visits (on-policy, a few rounds) and keep
    the set with the largest minimum relative margin.  Exit decisions are then far from knife-edge, which is what
    makes "exit-layer indices match exactly" a meaningful requirement for a bf16 device path."""
    exit_ids = cfg.exit_ids()
    ctl0 = orc.OracleExitController(None, exit_ids, max_layer=max_layer)
    real = ctl0.real_num_exit
    _, rec, _ = oracle_episode(cfg, sd, inputs, [-1.0] * real, max_layer)
    thr = [gap_threshold([v for (i, v) in rec if i == e])[0] for e in exit_ids[:real]]
    thr[-1] = 1e5
    best, best_m = list(thr), -1.0
    for _ in range(iters):
        _, rec, _ = oracle_episode(cfg, sd, inputs, thr, max_layer, sps)
        m = min_margin(rec, dict(zip(exit_ids, thr)))
        if m > best_m:
            best, best_m = list(thr), m
        if m > 0.08:
            break
        new = list(thr)
        for k, e in enumerate(exit_ids[:real - 1]):
            vals = [v for (i, v) in rec if i == e]
            if len(vals) >= 4:
                new[k] = gap_threshold(vals, 0.15, 0.85)[0]
        if new == thr:
            break
        thr = new
    return best, best_m


def make_inputs(cfg, n_steps, text_len=14):
    return [syn.synthetic_step_inputs(cfg, s, text_len=text_len) for s in range(n_steps)]


# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_engine_matches_reference_golden_forward(precision):
    """HIP engine vs the reference's own MPTFlamingo.forward outputs (static exit ids = BASELINE config[0],
    and the dynamic-exit step protocol with LSTM carry), in the product arithmetic on fp16 operands (default: the reference's amp
    arithmetic) and on bf16 operands (a --precision bf16 run)."""
    cfg, seed, g = load("deer_forward.npz")
    sd = syn.make_synthetic_state(cfg, seed, bf16_round=True)
    eng = DeerEngine(cfg, sd, precision=precision)
    assert eng.precision == precision and eng.img.dtype == (torch.float16 if precision == "fp16" else torch.bfloat16)
    ids, mask = g["ids"].long(), g["mask"].bool()
    rgb, grip = g["rgb"], g["grip"]
    for eid in (3, 4, -1):
        eng.reset()
        r = eng.step(rgb[0], grip[0], ids, mask, exit_id=eid, use_graph=False)
        tag = f"static{eid}"
        assert r["exit_layer"] == int(g[tag + "_exit"])
        torch.cuda.synchronize()
        if eid == 3:
            vis = eng.vis_x_f32.cpu().view(1, 1, cfg.n_media, cfg.vit_width)
            assert float((vis - g["vis_x"]).abs().max()) < 5e-2
        hid = eng.hidden[: r["exit_layer"] + 1, : ids.shape[1]].cpu()
        ref_h = g[tag + "_hidden"][:, 0]
        assert float((hid - ref_h).abs().max() / ref_h.abs().max()) < 2e-2
        assert float((r["pose"] - g[tag + "_pose"].reshape(-1)).abs().max()) < ACTION_TOL
        assert abs(r["gripper"] - float(g[tag + "_grip"])) < ACTION_TOL
    for tag in ("dyn", "dynS"):
        eng.reset()
        eng.configure_exit(cfg.exit_ids(), int(g[tag + "_max_layer"]), 1)
        eng.set_thresholds([float(t) for t in g[tag + "_thr"]])
        for s in range(rgb.shape[0]):
            r = eng.step(rgb[s], grip[s], ids, mask, use_graph=(s > 1))
            assert r["exit_layer"] == int(g[tag + "_exit"][s]), (tag, s, r["exit_layer"], g[tag + "_exit"])
            assert float((r["pose"] - g[tag + "_pose"][s].reshape(-1)).abs().max()) < ACTION_TOL, (tag, s)
            assert abs(r["gripper"] - float(g[tag + "_grip"][s])) < ACTION_TOL


@pytest.fixture(scope="module")
def tiny():
    cfg = deer_tiny()
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
    eng = DeerEngine(cfg, sd)
    return cfg, sd, eng


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_tiny_vision_and_hidden_states_vs_oracle(tiny, precision):
    cfg, sd, eng = tiny
    if precision == "bf16":
        eng = DeerEngine(cfg, sd, precision="bf16")
    rgb, grip, ids, mask = syn.synthetic_step_inputs(cfg, 0)
    model = orc.OracleDeer(sd, cfg)
    model.set_all_exit_window_size(1)
    o = model.forward(rgb, ids, mask, grip, exit_id=cfg.n_layers - 1)
    eng.reset()
    r = eng.step(rgb, grip, ids, mask, exit_id=cfg.n_layers - 1, use_graph=False)
    vis = eng.vis_x_f32.cpu()
    ref_vis = o["vis_x"].reshape(cfg.n_media, cfg.vit_width)
    assert float((vis - ref_vis).abs().max()) < 6e-2 and float((vis - ref_vis).norm() / ref_vis.norm()) < (1e-2 if precision == "bf16" else 1.5e-3)
    T = ids.shape[1]
    for i in range(cfg.n_layers):
        a, b = eng.hidden[i, :T].cpu(), o["hidden_states"][i][0]
        assert float((a - b).norm() / b.norm()) < 1e-2, i
    assert r["exit_layer"] == cfg.n_layers - 1
    assert float((r["pose"] - o["logits"][0].reshape(-1)).abs().max()) < ACTION_TOL
    assert abs(r["gripper"] - float(o["logits"][1])) < ACTION_TOL


@pytest.mark.parametrize("max_layer,sps", [(12, 1), (4, 1), (12, 3)])
def test_tiny_dynamic_exit_episode_vs_oracle(tiny, max_layer, sps):
    """A 24-step episode with LSTM carry: exit layers identical, actions within 1e-2, per-exit deltas close."""
    cfg, sd, eng = tiny
    inputs = make_inputs(cfg, 24, text_len=11)
    thr, margin = probe_thresholds(cfg, sd, inputs, max_layer, sps)
    assert margin > 0.01, margin
    ref, rec, ctl = oracle_episode(cfg, sd, inputs, thr, max_layer, sps)
    eng.configure_exit(cfg.exit_ids(), max_layer, sps)
    eng.set_thresholds(thr)
    eng.reset()
    exits = []
    for s, (rgb, grip, ids, mask) in enumerate(inputs):
        r = eng.step(rgb, grip, ids, mask, use_graph=(s >= 2))
        exits.append(r["exit_layer"])
        assert r["exit_layer"] == ref[s][0], (s, exits, [x[0] for x in ref], r["deltas"][:6].tolist(), thr, margin)
        assert float((r["pose"] - ref[s][1]).abs().max()) < ACTION_TOL, s
        assert abs(r["gripper"] - ref[s][2]) < ACTION_TOL
    assert len(set(exits)) > 1, exits                     # the schedule really is dynamic
    assert exits == [x[0] for x in ref]


def test_mpt7b_shaped_variant_dynamic_episode_vs_oracle():
    """OpenFlamingo-9B / MPT-7B structure (BASELINE configs[4]) at reduced width: no q/k LayerNorm, ``norm_1/norm_2`` and
    ``ffn.up_proj/down_proj`` parameter names, gated x-attn only in front of every 4th decoder layer, exits every 2 layers."""
    cfg = deer_tiny(llm_name="mpt_9b", attn_qk_ln=False, cross_attn_every_n_layers=4, n_layers_total=12, early_exit_layer=9)
    assert [i for i in range(cfg.n_layers) if cfg.has_xattn(i)] not in ([], list(range(cfg.n_layers)))
    sd = syn.make_synthetic_state(cfg, 7, bf16_round=True)
    assert any(".norm_1." in k for k in sd) and any("ffn.up_proj" in k for k in sd) and not any("q_ln" in k for k in sd)
    eng = DeerEngine(cfg, sd)
    inputs = make_inputs(cfg, 16, text_len=9)
    thr, margin = probe_thresholds(cfg, sd, inputs, 12, 1)
    assert margin > 0.01, margin
    ref, _, _ = oracle_episode(cfg, sd, inputs, thr, 12, 1)
    eng.configure_exit(cfg.exit_ids(), 12, 1)
    eng.set_thresholds(thr)
    eng.reset()
    exits = []
    for s, (rgb, grip, ids, mask) in enumerate(inputs):
        r = eng.step(rgb, grip, ids, mask, use_graph=(s >= 2))
        exits.append(r["exit_layer"])
        assert r["exit_layer"] == ref[s][0], (s, exits, [x[0] for x in ref])
        assert float((r["pose"] - ref[s][1]).abs().max()) < ACTION_TOL, s
        assert abs(r["gripper"] - ref[s][2]) < ACTION_TOL


def test_shadow_calibration_mode_records_every_exit_on_policy(tiny):
    """Shadow mode (bench.py calibration): all exits are evaluated every step, the state is committed at the first
    exit that fires.  Reference semantics restated with the oracle head/controller pieces."""
    cfg, sd, eng = tiny
    inputs = make_inputs(cfg, 10, text_len=9)
    thr, margin = probe_thresholds(cfg, sd, inputs, 12)
    exit_ids = cfg.exit_ids()
    model = orc.OracleDeer(sd, cfg)
    model.set_all_exit_window_size(1)
    head = model.extra_exit
    eng.configure_exit(exit_ids, 12, 1)
    eng.set_thresholds(thr)
    eng.reset()
    for s, (rgb, grip, ids, mask) in enumerate(inputs):
        hidden, _ = orc.llm_forward(sd, cfg, ids, mask, model.encode_vision(rgb, grip), exit_id=exit_ids[-1])
        prev = head(hidden[0], update_hidden_state=False)
        deltas, first = [], None
        for k, e in enumerate(exit_ids):
            act = head(hidden[e], update_hidden_state=False)
            d = float(orc.get_delta(act[0], prev[0], "L2"))
            deltas.append(d)
            prev = act
            if first is None and (d <= thr[k] or e >= exit_ids[-1]):
                first = e
        ref_act = head(hidden[first], update_hidden_state=True)
        r = eng.step(rgb, grip, ids, mask, use_graph=(s >= 2), shadow=True)
        assert r["exit_layer"] == first, (s, r["exit_layer"], first)
        got = r["deltas"][: len(exit_ids)]
        assert float((got - torch.tensor(deltas)).abs().max()) < 5e-3, (s, got, deltas)
        assert float((r["pose"] - ref_act[0].reshape(-1)).abs().max()) < ACTION_TOL
    # leaving shadow mode restores normal early termination
    r = eng.step(*inputs[0][:3], inputs[0][3], use_graph=False)
    assert r["n_evals"] <= len(exit_ids) + 1


def test_window_mode_calibration_values_vs_oracle(tiny):
    """``generate_action_values`` / ``ExitController.set_threshold`` (value_net.py:185-264,301-397): window-mode deltas of a
    calibration batch on the engine == the oracle's generate mode (pinned against the reference: valuenet_generate.npz)."""
    from deer_vla_amd.value_net import ActionValueNet, ExitController, generate_action_values
    cfg, sd, eng = tiny
    W, bs = 8, 2
    exit_ids = cfg.exit_ids()
    gen = torch.Generator().manual_seed(4)
    frames = [[syn.synthetic_step_inputs(cfg, 10 * b + t, text_len=9) for t in range(W)] for b in range(bs)]
    images = torch.stack([torch.stack([f[0].reshape(3, cfg.image_size, cfg.image_size) for f in fr]) for fr in frames])
    gripper = torch.stack([torch.stack([f[1].reshape(3, cfg.image_size, cfg.image_size) for f in fr]) for fr in frames])
    ids = torch.cat([fr[0][2] for fr in frames])                       # (bs, T)
    batch = (images, (ids, torch.ones_like(ids)), None, gripper)
    # --- oracle: hidden states of every layer for every frame, same random history layers ---
    model = orc.OracleDeer(sd, cfg)
    head = model.extra_exit
    head.window_size = W
    vn_o = orc.OracleValueNet(exit_ids, head, cfg.exit_interval, W, "L2")
    g2 = torch.Generator().manual_seed(4)
    ref = []
    for b in range(bs):
        idx = torch.randint(0, len(exit_ids), (W,), generator=g2)
        rl = [exit_ids[int(i)] for i in idx]
        hid = []
        for t in range(W):
            rgb, grip, ids_t, mask = frames[b][t]
            h, _ = orc.llm_forward(sd, cfg, ids_t, mask, model.encode_vision(rgb, grip), exit_id=cfg.n_layers - 1)
            hid.append(torch.stack([x[0] for x in h]))                  # (L, T, d)
        hid = torch.stack(hid)                                          # (W, L, T, d)
        feats = tuple(hid[:, l] for l in range(cfg.n_layers))           # per layer: (bs*W = W, T, d)
        rand_feat = torch.stack([hid[t, rl[t]] for t in range(W)])
        ref.append(vn_o(feats, mode="generate", rand_layer_feat=rand_feat))
    ref = torch.cat(ref, dim=1)

    class _M:                                                           # the bits of MPTFlamingo generate_action_values touches
        def __init__(self, e):
            self.module, self.engine = self, e
    eng.configure_exit(exit_ids, 12, 1)
    vn = ActionValueNet(exit_ids, None, cfg.exit_interval, W, "L2")
    vals, _ = generate_action_values(None, _M(eng), vn, [batch], generator=gen)
    assert vals.shape == ref.shape == (len(exit_ids), bs * (W - W // 2))
    assert float((vals - ref).abs().max()) < 5e-3, (vals, ref)
    # and the controller solves thresholds from them exactly like from reference values
    ctl = ExitController(vn, exit_ids, max_layer=12)
    ctl.set_threshold(None, _M(eng), [batch], 0.8, cfg.llm_name, values=None)
    ctl_ref = orc.OracleExitController(None, exit_ids, max_layer=12)
    assert len(ctl.threshold_list()) == ctl_ref.real_num_exit and ctl.threshold_list()[-1] >= 1e7


def test_graph_replay_is_bit_identical_to_eager(tiny):
    """Three schedules of the same dynamic step - eager launches, ONE graph with device-side skipping, and the pipelined
    pieces (two-chain vision, head evaluations on a side stream, host stops feeding at the published verdict) - give
    bit-identical actions, exit layers and deltas."""
    cfg, sd, eng = tiny
    inputs = make_inputs(cfg, 24, text_len=11)
    thr, _ = probe_thresholds(cfg, sd, inputs, 12, 1)              # thresholds that make the episode exit at several layers
    eng.configure_exit(cfg.exit_ids(), 12, 1)
    eng.set_thresholds(thr)
    res = []
    try:
        for use_graph, pieces in ((False, False), (True, False), (True, True)):
            eng.segmented = pieces
            eng.reset()
            out = []
            for s, (rgb, grip, ids, mask) in enumerate(inputs):
                r = eng.step(rgb, grip, ids, mask, use_graph=use_graph)
                out.append((r["exit_layer"], r["pose"].clone(), r["gripper"], r["deltas"].clone(), r["n_evals"]))
            res.append(out)
    finally:
        eng.segmented = True
    assert len({o[0] for o in res[0]}) > 1                      # exits at different layers within the episode
    for a, b, c in zip(*res):
        for x in (b, c):
            assert a[0] == x[0] and torch.equal(a[1], x[1]) and a[2] == x[2] and a[4] == x[4]
            assert torch.equal(torch.nan_to_num(a[3], nan=-1.0), torch.nan_to_num(x[3], nan=-1.0))


def test_pipelined_step_publishes_verdicts_to_the_host_mirror(tiny):
    """The pinned mirror carries, for the last step: done == sequence number, progress == seq*64 + checks evaluated, and the
    exiting environment's control block (csrc/head.hip::check_done)."""
    cfg, sd, eng = tiny
    inputs = make_inputs(cfg, 4)
    eng.configure_exit(cfg.exit_ids(), 12, 1)
    eng.set_thresholds([-1.0] * (eng.real_num_exit - 1) + [1e5])     # never below threshold: forced exit at the last check
    eng.reset()
    for rgb, grip, ids, mask in inputs:
        r = eng.step(rgb, grip, ids, mask)
    torch.cuda.synchronize()
    hm = eng.host_mirror
    assert int(hm[abi.HOSTM_DONE]) == eng._seq
    assert int(hm[abi.HOSTM_PROGRESS]) == eng._seq * 64 + eng.real_num_exit
    blk = hm[abi.CTL_WORDS: 2 * abi.CTL_WORDS]
    assert int(blk[abi.CTL_EXIT_LAYER]) == r["exit_layer"] == eng.ctl_max_layer
    assert int(blk[abi.CTL_EXIT_FLAG]) == 1


def test_padding_mask_and_text_lengths(tiny):
    cfg, sd, eng = tiny
    for T, pad in ((5, 0), (16, 3), (17, 0), (32, 5)):
        rgb, grip, ids, mask = syn.synthetic_step_inputs(cfg, 1, text_len=T)
        if pad:
            mask[0, T - pad:] = False
        o = orc.OracleDeer(sd, cfg)
        o.set_all_exit_window_size(1)
        ref = o.forward(rgb, ids, mask, grip, exit_id=2)
        eng.reset()
        r = eng.step(rgb, grip, ids, mask, exit_id=2, use_graph=False)
        a, b = eng.hidden[2, :T].cpu(), ref["hidden_states"][2][0]
        assert float((a - b).norm() / b.norm()) < 1e-2, (T, pad)
        assert float((r["pose"] - ref["logits"][0].reshape(-1)).abs().max()) < ACTION_TOL


def oracle_episode_margins(cfg, sd, inputs, thresholds, max_layer, steps_per_stage=1, restart=None):
    """oracle_episode + the relative margin |delta - thr| / thr of the tightest exit check the oracle evaluated at each step.
    restart: step at which this environment begins a NEW sub-task (eval_utils.py:252-277 reset, its step index counts from 0 again)"""
    model = orc.OracleDeer(sd, cfg)
    model.set_all_exit_window_size(1)
    vn = RecVN(cfg.exit_ids(), model.extra_exit, cfg.exit_interval, 1, "L2")
    vn.rec = []
    ctl = orc.OracleExitController(vn, cfg.exit_ids(), steps_per_stage=steps_per_stage, max_layer=max_layer)
    ctl._set_threshold_value(thresholds)
    thr_by_exit = dict(zip(cfg.exit_ids(), thresholds))
    outs = []
    for s, (rgb, grip, ids, mask) in enumerate(inputs):
        if restart is not None and s == restart:
            model.clear_all_exit_memory()
            vn.reset_actions()
        ctl.set_timestep(s if restart is None or s < restart else s - restart)
        n0 = len(vn.rec)
        o = model.forward(rgb, ids, mask, grip, dynamic_early_exit=True, exit_controller=ctl)
        m = [abs(v - thr_by_exit[i]) / thr_by_exit[i] for (i, v) in vn.rec[n0:] if thr_by_exit[i] < 1e4]
        outs.append((o["exit_layer"], o["logits"][0].reshape(-1), float(o["logits"][1]), min(m) if m else float("inf")))
    return outs


BAND = 1e-2


def run_env_batch_against_independent_oracles(cfg, sd, eng, env_inputs, thr, sps, n_steps, B, restarts=None):
    """Every environment of the batch must behave exactly like an independent single-environment oracle run.  Rule (the same
    as tests/test_episode_parity.py): exit layers are compared at every step whose oracle decision is not knife-edge (margin >
    1e-2); an environment whose knife-edge decision flips is reported and left out FROM THAT STEP ON (its LSTM history
    diverged; a batch cannot be re-aligned per environment).  Returns (#compared env-steps, flips, seen exit layers)."""
    refs = [oracle_episode_margins(cfg, sd, env_inputs[e], thr, 12, sps, None if restarts is None else restarts[e]) for e in range(B)]
    eng.configure_exit(cfg.exit_ids(), 12, sps)
    eng.set_thresholds(thr)
    eng.reset()
    seen, flips, compared = set(), [], 0
    alive = [True] * B
    for s in range(n_steps):
        rgb = torch.stack([env_inputs[e][s][0] for e in range(B)])
        grip = torch.stack([env_inputs[e][s][1] for e in range(B)])
        T = max(env_inputs[e][s][2].shape[1] for e in range(B))
        ids = torch.zeros(B, T, dtype=torch.long)
        mask = torch.zeros(B, T, dtype=torch.bool)
        for e in range(B):                                         # right-pad to the longest instruction of the batch
            te = env_inputs[e][s][2].shape[1]
            ids[e, :te], mask[e, :te] = env_inputs[e][s][2][0], True
        env_steps = None
        if restarts is not None:                                   # every environment's step index inside ITS sub-task
            for e in range(B):
                if restarts[e] is not None and s == restarts[e]:
                    eng.reset_env(e)
            env_steps = [s if restarts[e] is None or s < restarts[e] else s - restarts[e] for e in range(B)]
        out = eng.step(rgb, grip, ids, mask, use_graph=(s >= 2), env_steps=env_steps)
        out = out if isinstance(out, list) else [out]
        assert len(out) == B
        for e in range(B):
            if not alive[e]:
                continue
            ex, pose, g, margin = refs[e][s]
            if out[e]["exit_layer"] != ex:
                assert margin <= BAND, ("exit mismatch outside the knife-edge band", e, s, out[e]["exit_layer"], ex, margin)
                flips.append((e, s, margin))
                alive[e] = False
                continue
            assert float((out[e]["pose"] - pose).abs().max()) < ACTION_TOL, (e, s)
            assert abs(out[e]["gripper"] - g) < ACTION_TOL
            compared += 1
            seen.add(ex)
    print(f"\n[env batch B={B}] compared {compared}/{B * n_steps} env-steps, knife-edge flips {flips}")
    return compared, flips, seen


@pytest.mark.parametrize("B,sps", [(2, 1), (4, 1), (3, 2), (8, 1), (16, 2)])   # 12 / 13 environments: the compaction and batch-parity tests
def test_batched_environments_match_independent_oracle_runs(B, sps):
    """n_envs environments per step (one env batch per rank): every environment must behave exactly like an
    independent single-environment run - its own exit layer (exact), action (1e-2), LSTM carry - while sharing the
    weight stream.  B=2 -> 22 LLM rows (2 MFMA row tiles), B=4 -> 44 rows, B=8 -> 88 rows (6 row tiles)."""
    cfg = deer_tiny()
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
    eng = DeerEngine(cfg, sd, n_envs=B)
    n_steps, T = 12, 11
    env_inputs = [[syn.synthetic_step_inputs(cfg, s, rank=e, text_len=T, text_seed=7 + e) for s in range(n_steps)] for e in range(B)]
    thr, _ = probe_thresholds(cfg, sd, env_inputs[0], 12, sps)
    compared, flips, seen = run_env_batch_against_independent_oracles(cfg, sd, eng, env_inputs, thr, sps, n_steps, B)
    assert compared >= 0.8 * B * n_steps, (compared, flips)
    assert len(seen) > 1


@pytest.mark.parametrize("B,sps,restarts", [(4, 3, [None, 4, 5, 7]), (3, 2, [None, 3, 6])])
def test_env_batch_with_steps_per_stage_and_staggered_sub_tasks(B, sps, restarts):
    """``steps_per_stage`` > 1 (value_net.py:285-286, eval_calvin.py:340) for ENV BATCHES: the slots of a batch are at different steps of
    their sub-tasks (eval_utils.py:662-663 hands every rollout's own step to ``set_timestep``), so the stage hold is per environment on
    the device (CTL_HOLD of every control block, bit b of the step info).  Here the environments restart their sub-tasks at different
    batch steps - their hold phases drift apart - and each must still match an independent single-environment oracle run that sees the
    same resets and step indices."""
    cfg = deer_tiny()
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
    eng = DeerEngine(cfg, sd, n_envs=B)
    n_steps, T = 14, 11
    env_inputs = [[syn.synthetic_step_inputs(cfg, s, rank=e, text_len=T, text_seed=7 + e) for s in range(n_steps)] for e in range(B)]
    thr, _ = probe_thresholds(cfg, sd, env_inputs[0], 12, sps)
    compared, flips, seen = run_env_batch_against_independent_oracles(cfg, sd, eng, env_inputs, thr, sps, n_steps, B, restarts)
    assert compared >= 0.8 * B * n_steps, (compared, flips)
    assert len(seen) > 1


def test_batched_environments_with_different_instruction_lengths():
    """Instructions of an env batch are right-padded to the longest one; an environment with a shorter instruction must still
    match its own UNPADDED single-environment oracle run: padded key rows are masked in the attention and stay out of the
    head's token pool (head_pool_kernel pooled over pad rows)."""
    cfg = deer_tiny()
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
    B, n_steps = 3, 8
    lens = [14, 9, 11]
    eng = DeerEngine(cfg, sd, n_envs=B)
    env_inputs = [[syn.synthetic_step_inputs(cfg, s, rank=e, text_len=lens[e], text_seed=7 + e) for s in range(n_steps)] for e in range(B)]
    thr, _ = probe_thresholds(cfg, sd, env_inputs[0], 12, 1)
    compared, flips, seen = run_env_batch_against_independent_oracles(cfg, sd, eng, env_inputs, thr, 1, n_steps, B)
    assert compared >= 0.8 * B * n_steps, (compared, flips)


def test_eight_environments_with_instructions_up_to_32_tokens():
    """the reference pads an instruction batch to its longest member with max_length = 32 (data.py:905-919); 8
    environments x 32 tokens = 256 trunk rows (two row blocks of the hi/lo-plane GEMM, two MFMA row tiles per environment in the x-attn
    and MPT attention kernels).  Mixed lengths 9..32: every environment against its own UNPADDED single-environment oracle run."""
    cfg = deer_tiny()
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
    B, n_steps = 8, 6
    lens = [32, 14, 20, 9, 27, 16, 31, 11]
    eng = DeerEngine(cfg, sd, n_envs=B)
    assert eng.max_T == 32 and eng.max_rows == 256
    env_inputs = [[syn.synthetic_step_inputs(cfg, s, rank=e, text_len=lens[e], text_seed=7 + e) for s in range(n_steps)] for e in range(B)]
    thr, _ = probe_thresholds(cfg, sd, env_inputs[0], 12, 1)
    compared, flips, seen = run_env_batch_against_independent_oracles(cfg, sd, eng, env_inputs, thr, 1, n_steps, B)
    assert compared >= 0.8 * B * n_steps, (compared, flips)


def _mpt7b_tiny():
    return deer_tiny(llm_name="mpt_9b", attn_qk_ln=False, cross_attn_every_n_layers=4, n_layers_total=12, early_exit_layer=9)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("B,sps", [(2, 1), (4, 1), (8, 1), (16, 2)])
def test_mpt7b_shaped_env_batch_matches_independent_oracle_runs(B, sps, precision):
    """The env batch on the MPT-7B / OpenFlamingo-9B trunk shape (no q/k LayerNorm, bias-free LayerNorms, x-attn in front of every 4th
    layer): every environment against its own independent single-environment oracle run, in both 16-bit arithmetics."""
    cfg = _mpt7b_tiny()
    sd = syn.make_synthetic_state(cfg, 7, bf16_round=True)
    eng = DeerEngine(cfg, sd, n_envs=B, precision=precision)
    n_steps, T = 12, 9
    env_inputs = [[syn.synthetic_step_inputs(cfg, s, rank=e, text_len=T, text_seed=7 + e) for s in range(n_steps)] for e in range(B)]
    thr, _ = probe_thresholds(cfg, sd, env_inputs[0], 12, sps)
    compared, flips, seen = run_env_batch_against_independent_oracles(cfg, sd, eng, env_inputs, thr, sps, n_steps, B)
    assert compared >= 0.8 * B * n_steps, (compared, flips)
    assert len(seen) > 1


def test_mpt7b_shaped_env_batch_with_instructions_up_to_32_tokens():
    """8 environments x up to 32 tokens (256 trunk rows: deer_gemm_skinny_hl_rows) on the MPT-7B trunk shape, mixed lengths, each
    environment against its own UNPADDED oracle run"""
    cfg = _mpt7b_tiny()
    sd = syn.make_synthetic_state(cfg, 7, bf16_round=True)
    B, n_steps = 8, 6
    lens = [32, 14, 20, 9, 27, 16, 31, 11]
    eng = DeerEngine(cfg, sd, n_envs=B)
    assert eng.max_rows == 256
    env_inputs = [[syn.synthetic_step_inputs(cfg, s, rank=e, text_len=lens[e], text_seed=7 + e) for s in range(n_steps)] for e in range(B)]
    thr, _ = probe_thresholds(cfg, sd, env_inputs[0], 12, 1)
    compared, flips, seen = run_env_batch_against_independent_oracles(cfg, sd, eng, env_inputs, thr, 1, n_steps, B)
    assert compared >= 0.8 * B * n_steps, (compared, flips)


def test_mpt7b_shaped_env_batch_with_staggered_sub_tasks():
    """steps_per_stage = 3 with sub-tasks restarting at different batch steps (per-environment stage hold) on the MPT-7B trunk shape"""
    cfg = _mpt7b_tiny()
    sd = syn.make_synthetic_state(cfg, 7, bf16_round=True)
    B, sps, restarts = 4, 3, [None, 4, 5, 7]
    eng = DeerEngine(cfg, sd, n_envs=B)
    n_steps, T = 14, 9
    env_inputs = [[syn.synthetic_step_inputs(cfg, s, rank=e, text_len=T, text_seed=7 + e) for s in range(n_steps)] for e in range(B)]
    thr, _ = probe_thresholds(cfg, sd, env_inputs[0], 12, sps)
    compared, flips, seen = run_env_batch_against_independent_oracles(cfg, sd, eng, env_inputs, thr, sps, n_steps, B, restarts)
    assert compared >= 0.8 * B * n_steps, (compared, flips)
    assert len(seen) > 1


def test_full_size_mpt1b_vitl14_steps_vs_oracle():
    """BASELINE config sizes (ViT-L/14 x2, Perceiver, MPT-1B d=2048 x12 layers, 4x1024 LSTM head): static exit
    and a short dynamic episode against the fp32 CPU oracle."""
    cfg = deer_3b(max_layer=12)
    sd = full_size_state(cfg, 0, std="0.02", bf16_round=True)
    eng = DeerEngine(cfg, sd)
    inputs = make_inputs(cfg, 3)
    model = orc.OracleDeer(sd, cfg)
    model.set_all_exit_window_size(1)
    rgb, grip, ids, mask = inputs[0]
    o = model.forward(rgb, ids, mask, grip, exit_id=11)
    eng.reset()
    r = eng.step(rgb, grip, ids, mask, exit_id=11, use_graph=False)
    vis, ref_vis = eng.vis_x_f32.cpu(), o["vis_x"].reshape(cfg.n_media, cfg.vit_width)
    assert float((vis - ref_vis).norm() / ref_vis.norm()) < 2e-2
    for i in (0, 5, 11):
        a, b = eng.hidden[i, :14].cpu(), o["hidden_states"][i][0]
        assert float((a - b).norm() / b.norm()) < 2e-2, i
    assert float((r["pose"] - o["logits"][0].reshape(-1)).abs().max()) < ACTION_TOL
    assert abs(r["gripper"] - float(o["logits"][1])) < ACTION_TOL
    # dynamic: thresholds in the widest gaps of the oracle's deltas
    thr, margin = probe_thresholds(cfg, sd, inputs, 12, iters=1)
    ref, rec, _ = oracle_episode(cfg, sd, inputs, thr, 12)
    eng.configure_exit(cfg.exit_ids(), 12, 1)
    eng.set_thresholds(thr)
    eng.reset()
    for s, (rgb, grip, ids, mask) in enumerate(inputs):
        rr = eng.step(rgb, grip, ids, mask, use_graph=False)
        assert rr["exit_layer"] == ref[s][0], (s, rr["exit_layer"], ref[s][0], rr["deltas"][:6], thr)
        assert float((rr["pose"] - ref[s][1]).abs().max()) < ACTION_TOL


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_full_size_pre_fusion_vs_oracle(precision):
    """``fusion_mode='pre'`` (flamingo_mpt.py:585-607) at FULL size: the 2 x 256 patch tokens of the two frames are one 512-token media
    sequence for the 64 latents (the two-segment attention at kv1 = 512), 64 media tokens for the x-attn - same weights as the post-fusion
    model (the variant shares every parameter): media tokens, hidden states and the action of static steps (graph replay included)."""
    import dataclasses
    cfg0 = deer_3b(max_layer=12)
    cfg = dataclasses.replace(cfg0, fusion_mode="pre")
    sd = full_size_state(cfg0, 0, std="0.02", bf16_round=True)
    eng = DeerEngine(cfg, sd, precision=precision)
    model = orc.OracleDeer(sd, cfg)
    model.set_all_exit_window_size(1)
    eng.reset()
    rel, tol = (2e-2, ACTION_TOL) if precision != "fp32" else (2e-4, 1e-3)
    for s, eid in enumerate((11, 5, 11)):
        rgb, grip, ids, mask = syn.synthetic_step_inputs(cfg, s)
        o = model.forward(rgb, ids, mask, grip, exit_id=eid)
        r = eng.step(rgb, grip, ids, mask, exit_id=eid, use_graph=(s == 2))
        vis, ref_vis = eng.vis_x_f32.cpu(), o["vis_x"].reshape(cfg.n_media, cfg.vit_width)
        assert vis.shape == (cfg.perc_latents, cfg.vit_width) and float((vis - ref_vis).norm() / ref_vis.norm()) < rel, s
        a, b = eng.hidden[eid, :14].cpu(), o["hidden_states"][eid][0]
        assert float((a - b).norm() / b.norm()) < rel, s
        assert float((r["pose"] - o["logits"][0].reshape(-1)).abs().max()) < tol, s
        assert abs(r["gripper"] - float(o["logits"][1])) < tol, s


def test_full_size_mpt7b_openflamingo9b_steps_vs_oracle():
    """BASELINE configs[4] at FULL size (MPT-7B trunk: d=4096, 32 heads x 128, FF 16384, gated x-attn in front of every 4th
    layer, no q/k LayerNorm; 13 layers for max_layer=12): hidden states, static exits and a dynamic episode (pipelined
    schedule included) against the fp32 CPU oracle."""
    _full_size_9b_vs_oracle("fp16")


def test_full_size_mpt7b_openflamingo9b_steps_vs_oracle_bf16():
    """the same in the bf16 arithmetic (BASELINE config 5); the oracle's trunk memo makes this arm cost engine time only"""
    _full_size_9b_vs_oracle("bf16")


def _full_size_9b_vs_oracle(precision):
    from deer_vla_amd.config import deer_9b
    cfg = deer_9b(max_layer=12)
    sd = syn.make_synthetic_state(cfg, 0, std="0.02", bf16_round=True)
    eng = DeerEngine(cfg, sd, precision=precision)
    inputs = make_inputs(cfg, 4)
    model = orc.OracleDeer(sd, cfg)
    model.set_all_exit_window_size(1)
    rgb, grip, ids, mask = inputs[0]
    last = cfg.n_layers - 1
    o = model.forward(rgb, ids, mask, grip, exit_id=last)
    eng.reset()
    r = eng.step(rgb, grip, ids, mask, exit_id=last, use_graph=False)
    for i in (0, 3, 7, last):                                  # 3, 7: layers with a gated x-attn block in front
        a, b = eng.hidden[i, :ids.shape[1]].cpu(), o["hidden_states"][i][0]
        assert float((a - b).norm() / b.norm()) < 2e-2, i
    assert float((r["pose"] - o["logits"][0].reshape(-1)).abs().max()) < ACTION_TOL
    assert abs(r["gripper"] - float(o["logits"][1])) < ACTION_TOL
    thr, margin = probe_thresholds(cfg, sd, inputs, 12, iters=1)
    ref, _, _ = oracle_episode(cfg, sd, inputs, thr, 12)
    eng.configure_exit(cfg.exit_ids(), 12, 1)
    eng.set_thresholds(thr)
    for use_graph in (False, True, True):                      # eager, graph capture, pipelined replay
        eng.reset()
        for s, (rgb, grip, ids, mask) in enumerate(inputs):
            rr = eng.step(rgb, grip, ids, mask, use_graph=use_graph)
            assert rr["exit_layer"] == ref[s][0], (use_graph, s, rr["exit_layer"], ref[s][0], rr["deltas"][:7], thr)
            assert float((rr["pose"] - ref[s][1]).abs().max()) < ACTION_TOL


def test_full_size_mpt7b_openflamingo9b_env_batch_vs_oracle_and_compaction():
    """The MPT-7B / OpenFlamingo-9B trunk at FULL size (d = 4096, 32 heads) with FOUR environments in one engine: static exits at the last
    layer and at an exit layer (LSTM carried from the first), every environment against its own fp32 oracle (hidden states of layers 0, 3,
    7 and the last, actions); then a short dynamic episode with compaction on, bit-identical to a compaction-off sibling engine."""
    from deer_vla_amd.config import deer_9b
    cfg = deer_9b(max_layer=12)
    sd = syn.make_synthetic_state(cfg, 0, std="0.02", bf16_round=True)
    B, T, n_steps = 4, 14, 3
    eng = DeerEngine(cfg, sd, n_envs=B)
    env_inputs = [[syn.synthetic_step_inputs(cfg, s, rank=e, text_len=T, text_seed=7 + e) for s in range(n_steps)] for e in range(B)]
    rgb = torch.stack([env_inputs[e][0][0] for e in range(B)])
    grip = torch.stack([env_inputs[e][0][1] for e in range(B)])
    ids = torch.cat([env_inputs[e][0][2] for e in range(B)])
    last = cfg.n_layers - 1
    mid = 7 if 7 in cfg.exit_ids() else cfg.exit_ids()[len(cfg.exit_ids()) // 2]
    models = [orc.OracleDeer(sd, cfg) for _ in range(B)]
    for m in models:
        m.set_all_exit_window_size(1)
    eng.reset()
    for k, exit_id in enumerate((last, mid)):                   # the same frame twice: the second step carries the first one's LSTM state
        out = eng.step(rgb, grip, ids, None, exit_id=exit_id, use_graph=False)
        assert len(out) == B
        for e in range(B):
            r_e, g_e, i_e, m_e = env_inputs[e][0]
            o = models[e].forward(r_e, i_e, m_e, g_e, exit_id=exit_id)
            assert out[e]["exit_layer"] == exit_id
            if k == 0:
                for i in (0, 3, 7, last):                      # 3, 7: layers with a gated x-attn block in front
                    a, b = eng.hidden[i, e * T:(e + 1) * T].cpu(), o["hidden_states"][i][0]
                    assert float((a - b).norm() / b.norm()) < 2e-2, (e, i)
            assert float((out[e]["pose"] - o["logits"][0].reshape(-1)).abs().max()) < ACTION_TOL, (e, exit_id)
            assert abs(out[e]["gripper"] - float(o["logits"][1])) < ACTION_TOL, (e, exit_id)
    # dynamic episode: compaction on vs off (thresholds = per-exit median of a shadow step's deltas: the environments leave at different layers)
    eng_off = DeerEngine(cfg, None, n_envs=B, weights_from=eng)
    eng_off.set_compaction(False)
    exit_ids = cfg.exit_ids()
    eng_off.configure_exit(exit_ids, 12, 1)
    real = eng_off.real_num_exit                                  # exits up to max_layer = 12
    eng_off.set_thresholds([1e-9] * (real - 1) + [1e5])
    eng_off.reset()
    rec = [[] for _ in range(real)]
    for s in range(n_steps):
        rgb = torch.stack([env_inputs[e][s][0] for e in range(B)]).cuda().to(eng.img_dtype)
        grip = torch.stack([env_inputs[e][s][1] for e in range(B)]).cuda().to(eng.img_dtype)
        for r in eng_off.step(rgb, grip, ids, None, use_graph=False, shadow=True):
            for k in range(real):
                rec[k].append(float(r["deltas"][k]))
    thr = [float(np.median(v)) for v in rec[:-1]] + [1e5]
    for en in (eng, eng_off):
        en.configure_exit(exit_ids, 12, 1)
        en.set_thresholds(thr)
        en.reset()
    seen = set()
    for s in range(n_steps):
        rgb = torch.stack([env_inputs[e][s][0] for e in range(B)]).cuda().to(eng.img_dtype)
        grip = torch.stack([env_inputs[e][s][1] for e in range(B)]).cuda().to(eng.img_dtype)
        ra = eng.step(rgb, grip, ids, None, use_graph=(s >= 1))
        rb = eng_off.step(rgb, grip, ids, None, use_graph=(s >= 1))
        for e in range(B):
            assert ra[e]["exit_layer"] == rb[e]["exit_layer"], (s, e)
            assert torch.equal(ra[e]["pose"], rb[e]["pose"]) and ra[e]["gripper"] == rb[e]["gripper"], (s, e)
            assert torch.equal(torch.nan_to_num(ra[e]["deltas"], nan=-1.0), torch.nan_to_num(rb[e]["deltas"], nan=-1.0)), (s, e)
            seen.add(ra[e]["exit_layer"])
        torch.cuda.synchronize()
        assert torch.equal(eng.h_state, eng_off.h_state) and torch.equal(eng.c_state, eng_off.c_state), s
    assert len(seen) > 1, seen                                    # environments left at different layers: rows were compacted


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


def test_window_mode_forward_frames_as_batch_rows_vs_oracle(tiny):
    """MPTFlamingo.forward in window mode (flamingo_mpt.py:463-517 as value_net.py:375-385 calls it): bs*W frames as batch rows,
    hidden states of every layer, extra_exit over the random-layer history as sequences from a zero state (action_head.py:588-595)."""
    from deer_vla_amd.flamingo_mpt import MPTFlamingo
    cfg, sd, _ = tiny
    W, bs = 4, 3
    model = MPTFlamingo(cfg, sd, window_size=W)
    frames = [[syn.synthetic_step_inputs(cfg, 7 * b + t, text_len=9, text_seed=7 + b) for t in range(W)] for b in range(bs)]
    S = cfg.image_size
    vx = torch.stack([f[0].reshape(1, 1, 3, S, S) for fr in frames for f in fr])
    vg = torch.stack([f[1].reshape(1, 1, 3, S, S) for fr in frames for f in fr])
    ids = torch.cat([f[2] for fr in frames for f in fr])
    mask = torch.ones_like(ids)
    out, exit_outputs, extra, rand_feat, rand_idx = model._forward_window(vx, ids, mask, vg, with_gripper_logits=True,
                                                                         generator=torch.Generator().manual_seed(5))
    ref = _window_reference(cfg, sd, frames, W)                                  # (bs, W, L, T, d)
    got = torch.stack(out.hidden_states, dim=1).cpu().view(bs, W, cfg.n_layers, -1, cfg.d_model)
    assert len(out.hidden_states) == cfg.n_layers and exit_outputs == []
    assert float((got - ref).norm() / ref.norm()) < 1e-2
    # the head over the windows: oracle DeterministicDecoder in window mode on the SAME random layers
    rl = rand_idx.cpu()
    head = orc.OracleHead(sd, cfg, "extra_exit.")
    head.window_size = W
    rf = torch.stack([ref[b, t, int(rl[b, t])] for b in range(bs) for t in range(W)])            # (bs*W, T, d)
    a_ref, g_ref = head(rf)
    assert float((extra[0].cpu() - a_ref).abs().max()) < ACTION_TOL and float((extra[1][0].cpu() - g_ref).abs().max()) < ACTION_TOL
    assert tuple(extra[0].shape) == (bs, W, 6) and tuple(rand_feat.shape) == (bs * W, ids.shape[1], cfg.d_model)
    # and through the public forward signature (the call of value_net.py:375-385)
    o2 = model(vision_x=vx.cuda(), lang_x=ids.cuda(), attention_mask=mask.cuda(), vision_gripper=vg.cuda(), with_gripper_logits=True,
               return_in_feat=True, only_extra_exit=True)
    assert len(o2) == 5 and len(o2[0].hidden_states) == cfg.n_layers and torch.equal(torch.stack(o2[0].hidden_states), torch.stack(out.hidden_states))


_WINDOW_REF = {}


@pytest.mark.parametrize("max_layer", [12, 4])
def test_window_mode_calibration_full_size_batched_vs_oracle(max_layer):
    """the 12-frame history window as batch rows at FULL size (ViT at M = 8*514 rows, trunk at 112 rows):
    calibration deltas (value_net.py:134-160) of one 12-step window against the fp32 oracle.  max_layer = 4 is BASELINE configs[1]
    (DeeR-S, "12-step history": 5 layers built, exit ids {1, 3, 4})."""
    _window_full_size_vs_oracle(max_layer, None)


def test_window_mode_calibration_full_size_batched_vs_oracle_bf16():
    """DeeR-S (max_layer = 4) of the test above in the bf16 arithmetic (same weights, same oracle reference)"""
    _window_full_size_vs_oracle(4, "bf16")


def _window_full_size_vs_oracle(max_layer, precision):
    cfg = deer_3b(max_layer=max_layer)
    # one weight set for both cases: every tensor is seeded by its NAME (synthetic.make_synthetic_state), so the five-layer DeeR-S model
    # is the first five layers of the twelve-layer one - and so are the oracle's hidden states, computed once for both
    cfg12 = deer_3b(max_layer=12)
    sd12 = full_size_state(cfg12, 0, std="0.02", bf16_round=True)
    sd = {k: sd12[k] for k in syn.param_shapes(cfg)}
    eng = DeerEngine(cfg, sd, precision=precision)
    W = 12
    exit_ids = cfg.exit_ids()
    frames = [[syn.synthetic_step_inputs(cfg, 100 + t) for t in range(W)]]
    S = cfg.image_size
    images = torch.stack([f[0].reshape(3, S, S) for f in frames[0]]).cuda().to(eng.img_dtype)
    gripper = torch.stack([f[1].reshape(3, S, S) for f in frames[0]]).cuda().to(eng.img_dtype)
    ids = frames[0][0][2].cuda()
    hid = eng.window_hidden_states(images, gripper, ids, None)                   # (W, L, T, d): two groups of 8 / 4 frames
    if "ref12" not in _WINDOW_REF:
        _WINDOW_REF["ref12"] = _window_reference(cfg12, sd12, frames, W)[0]
    ref = _WINDOW_REF["ref12"][:, :cfg.n_layers]
    for l in sorted({0, cfg.n_layers // 2, cfg.n_layers - 1}):
        assert float((hid[:, l].cpu() - ref[:, l]).norm() / ref[:, l].norm()) < 2e-2, l
    g = torch.Generator().manual_seed(4)
    rl = [exit_ids[int(i)] for i in torch.randint(0, len(exit_ids), (W,), generator=g)]
    eng.configure_exit(exit_ids, max_layer, 1)
    vals = eng.generate_values(hid, rl, "L2")
    head = orc.OracleHead(sd, cfg, "extra_exit.")
    head.window_size = W
    vn = orc.OracleValueNet(exit_ids, head, cfg.exit_interval, W, "L2")
    feats = tuple(ref[:, l] for l in range(cfg.n_layers))
    vref = vn(feats, mode="generate", rand_layer_feat=torch.stack([ref[t, rl[t]] for t in range(W)]))
    assert vals.shape == vref.shape == (len(exit_ids), W - W // 2)
    assert float((vals - vref).abs().max()) < 5e-3, (vals, vref)


@pytest.mark.parametrize("B,lens,use_graph,exits", [(8, None, True, None), (8, None, False, None), (3, [14, 9, 11], True, None),
                                                   (8, [32, 14, 20, 9, 27, 16, 31, 11], True, None), (2, None, True, None),
                                                   (8, None, True, [1, 2, 3, 4, 5]), (8, None, False, [1, 2, 3, 4, 5]), (4, [14, 9, 11, 20], True, [1, 2, 3, 4, 5]),
                                                   (16, None, True, None), (16, [32, 14, 20, 9, 27, 16, 31, 11, 12, 30, 10, 25, 13, 18, 22, 15], True, None),
                                                   (13, None, False, [1, 2, 3, 4, 5])])
def test_compaction_of_exited_environments_is_bit_identical_to_the_uncompacted_batch(B, lens, use_graph, exits):
    """SURVEY 8(f).4 / VERDICT r3 item 3a: in an env batch the rows of an environment that has exited leave the trunk two layers after its
    exit check (gathering first row operation + row map, csrc/model.hip).  No arithmetic depends on a row's position, so every
    environment's exit layer, action, deltas and LSTM state must be BIT-identical to the same engine with compaction switched off -
    over an episode in which the environments leave at different layers (thresholds spread so that every exit is used), with mixed
    instruction lengths (padding masks follow the environment, not the slot), 256 trunk rows (two row blocks), graph pieces and eager
    single-stream enqueueing.  ``exits``: CONSECUTIVE exit layers - every layer from 2 on is then a compaction layer and
    the exit check of layer i - 1 is still running on the side stream while layer i gathers: the gather may only drop environments whose
    verdict the stream has ordered (exit layer <= i - 2, csrc/norm_embed.hip), else workgroups could disagree about the packing."""
    cfg = deer_tiny()
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
    _compaction_vs_uncompacted(cfg, sd, B, lens, use_graph, exits)


def _compaction_vs_uncompacted(cfg, sd, B, lens, use_graph, exits):
    """the body of the compaction test above; returns the exit layers of every step (one list of B per step)"""
    n_steps = 10 if exits is None else 16
    lens = lens or [11] * B
    eng_on = DeerEngine(cfg, sd, n_envs=B)
    eng_off = DeerEngine(cfg, None, n_envs=B, weights_from=eng_on)
    eng_off.set_compaction(False)
    env_inputs = [[syn.synthetic_step_inputs(cfg, s, rank=e, text_len=lens[e], text_seed=7 + e) for s in range(n_steps)] for e in range(B)]
    thr, _ = probe_thresholds(cfg, sd, env_inputs[0], 12, 1)
    exit_ids = cfg.exit_ids() if exits is None else exits
    T = max(lens)
    ids = torch.full((B, T), 1, dtype=torch.long)
    mask = torch.zeros(B, T, dtype=torch.bool)
    for e in range(B):
        ids[e, :lens[e]] = env_inputs[e][0][2].reshape(-1)
        mask[e, :lens[e]] = True
    ids, mask = ids.cuda(), mask.cuda()
    seen, steps = set(), []
    if exits is not None:
        # thresholds of the denser exit list: the per-exit median of the deltas of a shadow episode (every exit evaluated, none taken) -
        # about half of the environments that reach an exit leave there, so ADJACENT layers both see exits
        eng_off.configure_exit(exit_ids, 12, 1)
        eng_off.set_thresholds([1e-9] * (len(exit_ids) - 1) + [1e5])
        eng_off.reset()
        rec = [[] for _ in exit_ids]
        for s in range(6):
            rgb = torch.stack([env_inputs[e][s][0] for e in range(B)]).cuda().to(eng_on.img_dtype)
            grip = torch.stack([env_inputs[e][s][1] for e in range(B)]).cuda().to(eng_on.img_dtype)
            for r in eng_off.step(rgb, grip, ids, mask if len(set(lens)) > 1 else None, use_graph=False, shadow=True):
                for k in range(len(exit_ids)):
                    rec[k].append(float(r["deltas"][k]))
        thr = [float(np.median(v)) for v in rec[:-1]] + [1e5]
    for eng in (eng_on, eng_off):
        eng.configure_exit(exit_ids, 12, 1)
        eng.set_thresholds(thr)
        eng.reset()
    for s in range(n_steps):
        rgb = torch.stack([env_inputs[e][s][0] for e in range(B)]).cuda().to(eng_on.img_dtype)
        grip = torch.stack([env_inputs[e][s][1] for e in range(B)]).cuda().to(eng_on.img_dtype)
        ra = eng_on.step(rgb, grip, ids, mask if len(set(lens)) > 1 else None, use_graph=use_graph)
        rb = eng_off.step(rgb, grip, ids, mask if len(set(lens)) > 1 else None, use_graph=use_graph)
        steps.append([ra[e]["exit_layer"] for e in range(B)])
        for e in range(B):
            assert ra[e]["exit_layer"] == rb[e]["exit_layer"], (s, e)
            assert torch.equal(ra[e]["pose"], rb[e]["pose"]) and ra[e]["gripper"] == rb[e]["gripper"], (s, e)
            da, db = ra[e]["deltas"], rb[e]["deltas"]
            assert torch.equal(torch.nan_to_num(da, nan=-1.0), torch.nan_to_num(db, nan=-1.0)), (s, e)
            seen.add(ra[e]["exit_layer"])
        torch.cuda.synchronize()
        assert torch.equal(eng_on.h_state, eng_off.h_state) and torch.equal(eng_on.c_state, eng_off.c_state), s
    assert len(seen) > 1, seen                                    # environments really left at different layers
    if exits is not None:                                         # ... and at ADJACENT layers (the case the gather's rule exists for)
        assert any(l + 1 in seen for l in seen), seen
    return steps


@pytest.mark.parametrize("use_graph", [True, False])
def test_compaction_in_the_mpt7b_shaped_trunk_is_bit_identical_to_the_uncompacted_batch(use_graph):
    """The compaction test above on the MPT-7B / OpenFlamingo-9B trunk shape (no q/k LayerNorm, bias-free LayerNorms, gated x-attn only in
    front of every 4th layer) with consecutive exits 1..7 (the last one always fires): every layer 3 .. 7 is a compaction layer; the
    gathering row operation is the x-attn block's LayerNorm on layers 3 and 7 and the decoder's ln_1 (beta = NULL) on the others
    (csrc/model.hip).  `gathers` = the layers on which a gather must have dropped rows (worked out from the exit layers of each step: an
    environment that exited at l leaves at layer l + 2 if another one still runs it) - it must hold both kinds of layer."""
    cfg = deer_tiny(llm_name="mpt_9b", attn_qk_ln=False, cross_attn_every_n_layers=4, n_layers_total=12, early_exit_layer=9)
    sd = syn.make_synthetic_state(cfg, 7, bf16_round=True)
    steps = _compaction_vs_uncompacted(cfg, sd, 8, None, use_graph, [1, 2, 3, 4, 5, 6, 7])
    # a gather at layer i drops the environments that exited at layer i - 2 while another one still runs layer i
    gathers = {l + 2 for ex in steps for l in ex if l + 2 <= max(ex)}
    assert any(cfg.has_xattn(i) for i in gathers) and any(not cfg.has_xattn(i) for i in gathers), (gathers, steps)
