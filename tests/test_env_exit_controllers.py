"""Per-environment exit operating points (DeerEngine.set_env_exit, per-slot ExitController lists, evaluate_policy_batched(operating_points=)):
one env batch carries several threshold rows / layer caps side by side, and every environment computes exactly what a uniform run with its
own operating point computes.  Environments of a batch do not influence each other's arithmetic (compaction moves rows, it does not change
them: test_batch_parity.py::test_full_size_compaction_is_bit_identical_to_the_uncompacted_batch), so the gates here are BIT-identity."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deer_vla_amd import _abi as abi  # noqa: E402
from deer_vla_amd import rollout as ro  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import DeerConfig, deer_tiny  # noqa: E402
from deer_vla_amd.engine import DeerEngine  # noqa: E402
from golden_util import full_size_state  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "episode_batch8.npz")
N_STEPS = 24


@pytest.fixture(scope="module")
def full():
    """the full-size 3B env batch of test_batch_parity.py (episode_batch8.npz config, 8 environments)"""
    z = np.load(GOLD)
    cfg = DeerConfig(**json.loads(bytes(z["cfg_json"]).decode()))
    sd = full_size_state(cfg, int(z["seed"]), std="0.02", bf16_round=True)
    eng = DeerEngine(cfg, sd, n_envs=int(z["n_envs"]))
    return z, cfg, eng


def batch_inputs(cfg, B, s, dev):
    per_env = [syn.synthetic_step_inputs(cfg, s, rank=e % 8, text_seed=7 + e % 8) for e in range(B)]
    rgb = torch.stack([p[0] for p in per_env]).to(dev, torch.bfloat16)
    grip = torch.stack([p[1] for p in per_env]).to(dev, torch.bfloat16)
    ids = torch.cat([p[2] for p in per_env]).to(dev)
    return rgb, grip, ids


def episode(eng, cfg, n, schedule=None):
    """n dynamic steps from a reset; schedule: {step: callable(eng)} applied before that step.  -> [step][env] result dicts"""
    eng.reset()
    out, ids_keep = [], None
    for s in range(n):
        if schedule and s in schedule:
            schedule[s](eng)
        rgb, grip, ids = batch_inputs(cfg, eng.B, s, eng.dev)
        ids_keep = ids if ids_keep is None else ids_keep
        out.append(eng.step(rgb, grip, ids_keep, None))
    return out


def same(a, b):
    return (a["exit_layer"] == b["exit_layer"] and torch.equal(a["pose"], b["pose"]) and a["gripper"] == b["gripper"]
            and torch.equal(a["ens_pose"], b["ens_pose"]) and a["ens_gripper"] == b["ens_gripper"] and a["ens_count"] == b["ens_count"])


def uniform(eng, cfg, max_layer, row):
    eng.clear_env_exit()
    eng.configure_exit(cfg.exit_ids(), max_layer, 1)
    eng.set_thresholds(row)


@pytest.mark.parametrize("compact", [True, False])
def test_four_threshold_rows_in_one_batch_equal_four_uniform_runs_bit_for_bit(full, compact):
    """Four operating points, two environments each (rows scaled from the committed exit_ratio row: from 'exits early' to 'exits late'),
    on a weights_from= sibling; per point a uniform run of the same inputs on the base engine is the reference."""
    z, cfg, eng = full
    B, ML = eng.B, int(z["max_layer"])
    thr = [float(t) for t in z["thr"]]
    rows = [[t * f for t in thr[:-1]] + thr[-1:] for f in (2.0, 1.0, 0.6, 0.3)]
    point = [e // 2 for e in range(B)]
    mixed = DeerEngine(cfg, None, n_envs=B, weights_from=eng)
    for e_ in (eng, mixed):
        e_.set_compaction(compact)
    try:
        mixed.configure_exit(cfg.exit_ids(), ML, 1)
        mixed.set_env_exit([rows[point[e]] for e in range(B)], [mixed.ctl_max_layer] * B)
        got = episode(mixed, cfg, N_STEPS)
        layers = set()
        for p, row in enumerate(rows):
            uniform(eng, cfg, ML, row)
            ref = episode(eng, cfg, N_STEPS)
            for s in range(N_STEPS):
                for e in range(B):
                    if point[e] == p:
                        assert same(got[s][e], ref[s][e]), (p, s, e, got[s][e]["exit_layer"], ref[s][e]["exit_layer"])
                        layers.add(got[s][e]["exit_layer"])
        assert len(layers) > 2, layers                               # the points really exit at different layers
    finally:
        eng.set_compaction(True)


def test_per_environment_caps_and_graphs_survive_a_change_of_one_slot(full):
    """DeeR-S-like cap 3 and DeeR-B cap 11 in one batch, thresholds that never fire: every environment exits exactly at its own cap,
    bit-identical to a uniform run with that cap.  Then one slot's cap and another slot's row change between steps: the captured graph
    pieces stay the same objects, and the results equal a fresh sibling that recaptures after the change."""
    z, cfg, eng = full
    B = eng.B
    never = [-1.0] * 6                                             # leq: delta <= -1 never holds
    caps = [3 if e % 2 == 0 else 11 for e in range(B)]
    mixed = DeerEngine(cfg, None, n_envs=B, weights_from=eng)
    mixed.configure_exit(cfg.exit_ids(), 12, 1)
    mixed.set_env_exit([never] * B, caps)
    assert mixed.ctl_max_layer == 11
    n = 8
    got = episode(mixed, cfg, n)
    for cap in (3, 11):
        uniform(eng, cfg, cap + 1, [-1.0] * len([x for x in cfg.exit_ids() if x <= cap]))
        ref = episode(eng, cfg, n)
        for s in range(n):
            for e in range(B):
                if caps[e] == cap:
                    assert got[s][e]["exit_layer"] == cap and same(got[s][e], ref[s][e]), (cap, s, e)

    # a change of one slot between two steps: graphs are kept and read the new table
    caps2 = list(caps)
    caps2[0] = 11
    rows2 = [never] * B
    rows2[1] = [1e8] * 6                                            # fires at the first check (layer 1)

    def switch(e_):
        e_.set_env_exit(rows2, caps2)

    graphs = {}

    def switch_and_watch(e_):
        graphs.update(e_._graphs)
        switch(e_)

    a = episode(mixed, cfg, n, {4: switch_and_watch})
    assert graphs and all(mixed._graphs.get(k) is g for k, g in graphs.items()) and set(mixed._graphs) == set(graphs)
    fresh = DeerEngine(cfg, None, n_envs=B, weights_from=eng)
    fresh.configure_exit(cfg.exit_ids(), 12, 1)
    fresh.set_env_exit([never] * B, caps)

    def switch_recapture(e_):
        switch(e_)
        torch.cuda.synchronize()
        e_._drop_graphs()

    b = episode(fresh, cfg, n, {4: switch_recapture})
    for s in range(n):
        for e in range(B):
            assert same(a[s][e], b[s][e]), (s, e)
            want = (caps if s < 4 else caps2)[e] if not (s >= 4 and e == 1) else 1
            assert a[s][e]["exit_layer"] == want, (s, e, a[s][e]["exit_layer"], want)


def test_table_equal_to_the_engine_row_is_bit_identical_to_the_shared_path(full):
    z, cfg, eng = full
    B, ML = eng.B, int(z["max_layer"])
    thr = [float(t) for t in z["thr"]]
    uniform(eng, cfg, ML, thr)
    ref = episode(eng, cfg, 10)
    table = DeerEngine(cfg, None, n_envs=B, weights_from=eng)
    table.configure_exit(cfg.exit_ids(), ML, 1)
    table.set_thresholds(thr)
    table.set_env_exit([thr] * B, [table.ctl_max_layer] * B)
    got = episode(table, cfg, 10)
    layers = set()
    for s in range(10):
        for e in range(B):
            assert same(got[s][e], ref[s][e]), (s, e)
            layers.add(got[s][e]["exit_layer"])
    assert len(layers) > 2, layers
    # the device-row form: the same table from a (B, 16) CUDA tensor
    dev_rows = torch.full((B, 16), 1e8, dtype=torch.float32, device=table.dev)
    dev_rows[:, :len(thr)] = torch.tensor(thr)
    table.set_env_exit(dev_rows, [table.ctl_max_layer] * B)
    got2 = episode(table, cfg, 10)
    assert all(same(got2[s][e], ref[s][e]) for s in range(10) for e in range(B))


def test_refusals():
    from deer_vla_amd.flamingo_mpt import MPTFlamingo
    from deer_vla_amd.value_net import ActionValueNet, ExitController
    cfg = deer_tiny()
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
    model = MPTFlamingo(cfg, sd, n_envs=2)
    e = model.engine
    ids = model.get_all_exit_idx()

    def ctl(exit_ids=ids, leq=True, max_layer=cfg.early_exit_layer + 1):
        c = ExitController(ActionValueNet(ids, None, cfg.exit_interval, 12, "L2"), exit_ids, leq=leq, max_layer=max_layer)
        c._set_threshold_value([0.02] * (c.real_num_exit - 1) + [1e5])
        return c

    rgb, grip, tid, mask = syn.synthetic_step_inputs(cfg, 0)
    rgb2, grip2, tid2 = torch.cat([rgb, rgb]).cuda(), torch.cat([grip, grip]).cuda(), torch.cat([tid, tid]).cuda()
    with pytest.raises(ValueError, match="exit_id_list"):
        model.step_env_batch(rgb2, tid2, None, grip2, exit_controller=[ctl(), ctl(exit_ids=ids[:-1])])
    with pytest.raises(ValueError, match="leq"):
        model.step_env_batch(rgb2, tid2, None, grip2, exit_controller=[ctl(), ctl(leq=False)])
    # a mixed DeeR-S / DeeR-B list works, and a single controller afterwards runs the shared path again
    pose, g, exits = model.step_env_batch(rgb2, tid2, None, grip2, exit_controller=[ctl(max_layer=2), ctl()])
    assert exits[0] == 1 and e.env_caps == [1, cfg.early_exit_layer]
    model.step_env_batch(rgb2, tid2, None, grip2, exit_controller=ctl())
    assert e.env_caps is None
    # a cap that is not an exit (no forced check -> no verdict): DEER_ERR_SHAPE
    with pytest.raises(abi.DeerHipError, match="code 1"):
        e.set_env_exit([[0.02] * 3] * 2, [2, 5])
    with pytest.raises(abi.DeerHipError, match="code 1"):
        e.set_env_exit([[0.02] * 3] * 2, [0, 5])
    assert e.env_caps is None
    e.set_env_exit([[0.02] * 3] * 2, [3, 9])                        # beyond the last exit = the last exit (value_net.py:173)
    assert e.ctl_max_layer == 5
    e.clear_env_exit()
    # layerwise_exit_eval and one-environment engines keep one operating point
    cfg_lw = deer_tiny(layerwise_exit_eval=True)
    lw = MPTFlamingo(cfg_lw, syn.make_synthetic_state(cfg_lw, 3, bf16_round=True), n_envs=2)
    with pytest.raises(NotImplementedError):
        lw.step_env_batch(rgb2, tid2, None, grip2, exit_controller=[ctl(), ctl()])
    one = MPTFlamingo(cfg, sd, n_envs=1)
    with pytest.raises(NotImplementedError):
        one.step_env_batch(rgb.cuda(), tid.cuda(), None, grip.cuda(), exit_controller=[ctl()])
    with pytest.raises(NotImplementedError):
        one.engine.set_env_exit([[0.02] * 3], [5])


class CountingDebugEnv(ro.DebugEnv):
    """the harness's constant-frame debug environment, with the step count as ``info`` (for steps_task_checker): every slot sees the same
    frames whatever chain or point it serves, so a chain's exits depend on its instruction and its operating point only"""

    def __init__(self):
        self.t = 0

    def step(self, action):
        self.t += 1
        return self.get_random_obs(), 0.0, False, self.t

    def reset(self, **kwargs):
        self.t = 0

    def get_info(self):
        return self.t


def _report(fn):
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn()
    return out, buf.getvalue()


@pytest.mark.parametrize("with_groups", [False, True])
def test_sweep_equals_separate_runs(with_groups):
    from deer_vla_amd.factory import create_model_and_transforms
    from deer_vla_amd.value_net import ActionValueNet, ExitController
    cfg = deer_tiny()
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
    B = 3
    model, proc, tok = create_model_and_transforms("ViT-L-14", "openai", "", "", window_size=12, use_gripper=True, fusion_mode="post",
                                                   llm_name="mpt_dolly_3b", state_dict=sd, cfg=cfg, n_envs=B)
    ids = model.get_all_exit_idx()
    vn = ActionValueNet(ids, None, cfg.exit_interval, 12, "L2")

    def point(thr, max_layer):
        c = ExitController(vn, ids, max_layer=max_layer)
        c._set_threshold_value(thr)
        return c

    points = [point([0.004, 0.004, 1e5], 6), point([0.05, 0.05, 1e5], 6), point([0.02, 1e5], 4)]
    ann = {"a": ["open"], "b": ["push"], "c": ["turn"], "d": ["lift"]}      # one word each, like the idle slots' "idle": one T for every batch
    seqs = [(None, ["a", "b", "c"]), (None, ["b", "a"]), (None, ["c"]), (None, ["a", "c", "b"]), (None, ["d", "b"])]
    ok = ro.steps_task_checker(3)
    second = model.sibling() if with_groups else None

    def run(controller, sweep=None):
        w = ro.BatchedModelWrapper(model, tok, proc, torch.float32, exit_controller=controller)
        groups = [(ro.BatchedModelWrapper(second, tok, proc, torch.float32, exit_controller=controller), [CountingDebugEnv() for _ in range(B)])] \
            if with_groups else ()
        return _report(lambda: ro.evaluate_policy_batched(w, [CountingDebugEnv() for _ in range(B)], seqs, ann, ok, ep_len=5, report=True,
                                                          groups=groups, operating_points=sweep))

    sweep, text = run(None, points)
    blocks = text.split("Operating point ")[1:]
    assert len(sweep) == len(blocks) == 3
    volatile = ("wall_s_mean", "steps_per_s")
    hists = []
    for p, c in enumerate(points):
        one, one_text = run(c)
        assert {k: v for k, v in sweep[p].items() if k not in volatile} == {k: v for k, v in one.items() if k not in volatile}, p
        assert blocks[p].split("\n", 1)[1] == one_text, p
        hists.append(tuple(one["exit_hist"]))
    assert len(set(hists)) >= 2, hists                                     # the operating points really differ
    assert all(h[i] == 0 for h in hists[2:] for i in range(4, cfg.n_layers))   # the DeeR-S point never passes its cap
