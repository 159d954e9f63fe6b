"""On-policy exit values on a tiny model: what ``DeerEngine.log_values`` appends after a shadow step is that step's ``read_result()``
bit for bit, ties to the criterion the device applied (exact: the exit taken is the first whose logged delta passes its threshold), feeds
the device threshold solver where it lies, and leaves a run that never logs untouched; ``value_net.calibrate_on_policy`` on the synthetic
environments re-solves the budget every round exactly like the host solver on a copy of that round's matrix."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from deer_vla_amd import rollout as ro  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd import value_net as vn  # noqa: E402
from deer_vla_amd.config import deer_tiny  # noqa: E402
from deer_vla_amd.evaluate import on_policy_values  # noqa: E402
from deer_vla_amd.flamingo_mpt import MPTFlamingo  # noqa: E402

N_STEPS = 12
RESET_AT, SUBSET_AT = 5, 8                              # reset_env before step 5; at step 8 only a subset of the batch is logged


def _inputs(cfg, eng, B, s):
    per_env = [syn.synthetic_step_inputs(cfg, s, rank=e) for e in range(B)]
    return (torch.cat([p[0] for p in per_env]).cuda().to(eng.img_dtype), torch.cat([p[1] for p in per_env]).cuda().to(eng.img_dtype),
            torch.cat([p[2] for p in per_env]).cuda())


def _as_list(r):
    return r if isinstance(r, list) else [r]


@pytest.fixture(scope="module", params=[1, 4])
def logged(request):
    """12 shadow steps with log_values on an engine of B environments, under thresholds at the medians of a first look at the deltas"""
    B = request.param
    cfg = deer_tiny()
    model = MPTFlamingo(cfg, syn.make_synthetic_state(cfg, 3, bf16_round=True), n_envs=B)
    eng = model.engine
    n_exit = eng.real_num_exit
    eng.set_thresholds([-1.0] * (n_exit - 1) + [1e5])                   # no delta passes: every step runs to the cap
    rec = [[] for _ in range(n_exit)]
    for s in range(4):
        for r in _as_list(eng.step(*_inputs(cfg, eng, B, s), None, shadow=True)):
            for k in range(n_exit):
                rec[k].append(float(r["deltas"][k]))
    thr = [float(np.median(v)) for v in rec[:-1]] + [1e5]
    eng.set_thresholds(thr)
    eng.reset()
    eng.open_value_log(64)
    want_cols, want_taken = [], []
    for s in range(N_STEPS):
        if s == RESET_AT:
            eng.reset_env(B - 1)
        res = _as_list(eng.step(*_inputs(cfg, eng, B, s), None, shadow=True))
        active = list(range(B)) if s != SUBSET_AT else list(range(0, B, 2))
        if s == SUBSET_AT + 1:
            eng.log_values((1 << B) - 1)                                 # a mask
        elif s == SUBSET_AT:
            eng.log_values(active)                                       # environment indices
        else:
            eng.log_values()
        for b in active:
            want_cols.append(res[b]["deltas"][:n_exit].numpy().view(np.uint32).copy())
            want_taken.append(res[b]["exit_layer"])
    values, taken, dropped, nonfinite = eng.logged_values()
    return dict(B=B, cfg=cfg, model=model, eng=eng, thr=thr, n_exit=n_exit, values=values, taken=taken, dropped=dropped, nonfinite=nonfinite,
                want_cols=np.stack(want_cols, axis=1), want_taken=np.array(want_taken, dtype=np.int32))


def test_log_equals_read_result_bit_for_bit(logged):
    L = logged
    assert L["values"].is_cuda and L["taken"].is_cuda and L["values"].dtype == torch.float32 and L["taken"].dtype == torch.int32
    assert tuple(L["values"].shape) == (L["n_exit"], L["want_cols"].shape[1]) and L["want_cols"].shape[1] == len(L["want_taken"])
    assert (L["dropped"], L["nonfinite"]) == (0, 0)
    assert np.array_equal(L["values"].cpu().numpy().view(np.uint32), L["want_cols"])
    assert np.array_equal(L["taken"].cpu().numpy(), L["want_taken"])


def test_taken_is_the_first_exit_whose_logged_delta_passes_its_threshold(logged):
    L = logged
    v, taken, ids = L["values"].cpu(), L["taken"].cpu().tolist(), L["eng"].exit_ids
    T = torch.tensor(L["thr"], dtype=torch.float32)                       # what set_thresholds stored
    for n in range(v.shape[1]):
        first = next((e for e in range(L["n_exit"] - 1) if bool(v[e, n] <= T[e])), L["n_exit"] - 1)
        assert taken[n] == ids[first], (n, taken[n], ids[first], v[:, n].tolist())
    print(f"B={L['B']}: exit layers taken {sorted(set(taken))}, measured mix {vn.measured_exit_mix(taken, ids[: L['n_exit']])}")


def test_device_solver_on_the_logged_matrix_equals_the_host_solver(logged):
    L = logged
    n = L["values"].shape[1]
    counts = [vn.exit_counts(n, L["n_exit"], r) for r in (0.6, 1.0, 1.7)]
    T, left, status = L["eng"].solve_thresholds(L["values"], torch.tensor(counts, dtype=torch.int32), return_status=True)
    assert int(status.sum()) == 0
    host = L["values"].cpu()
    for p, c in enumerate(counts):
        hT, hleft = vn.solve_from_counts(host, c)
        assert torch.equal(T[p].cpu(), hT) and left[p].tolist() == hleft, p


def test_log_values_refusals(logged):
    L = logged
    cfg, eng, B = L["cfg"], L["eng"], L["B"]
    eng.step(*_inputs(cfg, eng, B, 0), None)                              # a normal step: it stops at its exit
    with pytest.raises(RuntimeError, match="shadow"):
        eng.log_values()
    with pytest.raises(RuntimeError, match="already open"):
        eng.open_value_log(8)
    with pytest.raises(RuntimeError, match="value log"):
        eng.configure_exit(eng.exit_ids, eng.exit_ids[1] + 1)            # fewer reachable exits than the open log has rows
    assert eng.real_num_exit == L["n_exit"]
    eng.step(*_inputs(cfg, eng, B, 1), None, shadow=True)
    with pytest.raises(ValueError):
        eng.log_values([B])
    with pytest.raises(ValueError):
        eng.log_values(1 << B)
    before = int(eng.logged_values()[0].shape[1])
    eng.log_values()
    assert int(eng.logged_values()[0].shape[1]) == before + B
    eng.close_value_log()
    with pytest.raises(RuntimeError, match="no value log"):
        eng.log_values()
    with pytest.raises(RuntimeError, match="no value log"):
        eng.logged_values()
    eng.open_value_log(64)                                                # the other tests of this module may still run on the fixture
    eng.reset()
    with pytest.raises(RuntimeError, match="shadow"):                     # a reset cleared the control blocks
        eng.log_values()


def test_run_without_a_log_is_bit_identical_to_an_engine_that_never_had_one(logged):
    L = logged
    cfg, B = L["cfg"], L["B"]
    fresh = MPTFlamingo(cfg, syn.make_synthetic_state(cfg, 3, bf16_round=True), n_envs=B).engine
    fresh.set_thresholds(L["thr"])

    def episode(eng):
        eng.reset()
        out = []
        for s in range(5):
            for r in _as_list(eng.step(*_inputs(cfg, eng, B, s), None)):
                out.append((r["exit_layer"], r["pose"].clone(), r["gripper"], r["deltas"].numpy().view(np.uint32).copy()))
        return out

    for (la, pa, ga, da), (lb, pb, gb, db) in zip(episode(L["eng"]), episode(fresh)):
        assert la == lb and torch.equal(pa, pb) and ga == gb and np.array_equal(da, db)


TASKS = ["open", "push", "turn", "lift"]                # one word each, like the idle slots' "idle": one T for every batch


def test_calibrate_on_policy_rounds_equal_the_host_solver():
    from deer_vla_amd.factory import create_model_and_transforms
    cfg = deer_tiny()
    B, n_samples, budget = 4, 40, 4.0
    model, proc, tok = create_model_and_transforms("ViT-L-14", "openai", "", "", window_size=12, use_gripper=True, fusion_mode="post",
                                                   llm_name="mpt_dolly_3b", state_dict=syn.make_synthetic_state(cfg, 3, bf16_round=True), cfg=cfg,
                                                   n_envs=B)
    ids = model.get_all_exit_idx()
    net = vn.ActionValueNet(ids, None, cfg.exit_interval, 12, "L2")
    start = vn.ExitController(net, ids, max_layer=ids[-1] + 1)
    start._set_threshold_value([0.15, 0.3, 1e8])                         # in the range of this model's deltas on these frames: a mixed start
    seqs = [(None, [TASKS[(i + j) % 4] for j in range(3)]) for i in range(6)]
    ann = {t: [t] for t in TASKS}
    w = ro.BatchedModelWrapper(model, tok, proc, torch.float32, exit_controller=start)
    args = (w, [ro.SyntheticEnv(seed=b) for b in range(B)], seqs, ann, ro.steps_task_checker(3))
    eng = model.engine
    calls = []
    solve = eng.solve_thresholds
    eng.solve_thresholds = lambda *a, **k: (calls.append(a[0].is_cuda), solve(*a, **k))[1]
    try:
        ctl, records = vn.calibrate_on_policy(*args, start, n_samples, budget, rounds=2, engine=eng, ep_len=5, grid=16)
    finally:
        del eng.solve_thresholds
    assert len(records) == 2 and calls and all(calls)                     # every solve ran on the device matrix
    assert w.exit_controller is start and getattr(eng, "_vlog", None) is None
    under = [start.threshold_list()] + [r["thresholds"] for r in records]  # the thresholds every collection ran under, in order
    for k, (v, taken) in enumerate([(r["values"], r["taken"]) for r in records]):
        v, taken, T = v.cpu(), taken.cpu().tolist(), torch.tensor(under[k], dtype=torch.float32)
        for n in range(n_samples):                                        # the rollout really ran under that round's thresholds
            first = next((e for e in range(len(ids) - 1) if bool(v[e, n] <= T[e])), len(ids) - 1)
            assert taken[n] == ids[first], (k, n, taken[n], v[:, n].tolist(), under[k])
    for r, nxt in zip(records, records[1:] + [None]):
        assert r["values"].is_cuda and tuple(r["values"].shape) == (len(ids), n_samples) and tuple(r["taken"].shape) == (n_samples,)
        h_ctl, h_ratio, h_mix = vn.solve_for_budget(r["values"].cpu(), ids, budget, engine=None, grid=16, value_net=net)
        assert r["thresholds"] == h_ctl.threshold_list() and r["exit_ratio"] == h_ratio and r["predicted"] == h_mix
        bc = torch.bincount(r["taken"].cpu().long(), minlength=ids[-1] + 1)
        assert r["collected"] == vn.predicted_exit_mix([int(bc[e]) for e in ids], ids)
        bc = torch.bincount(r["measured_taken"].cpu().long(), minlength=ids[-1] + 1)
        assert r["measured"] == vn.predicted_exit_mix([int(bc[e]) for e in ids], ids)
        if nxt is not None:
            assert r["measured"] == nxt["collected"] and r["measured_taken"] is nxt["taken"]
        print(f"round {r['round']}: budget {budget}, collected under the previous thresholds {r['collected'][1]:.3f}, predicted "
              f"{r['predicted'][1]:.3f}, measured in the next rollout {r['measured'][1]:.3f}; thresholds {r['thresholds']}")
    assert ctl.threshold_list() == records[-1]["thresholds"]
    # the last record's measured mix comes from one more collection under the final thresholds: the same call reproduces it
    _, taken, mix = on_policy_values(*args, ctl, n_samples, ep_len=5)
    bc = torch.bincount(taken.cpu().long(), minlength=ids[-1] + 1)
    assert mix == vn.predicted_exit_mix([int(bc[e]) for e in ids], ids)
