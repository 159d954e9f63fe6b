"""Host side of the device threshold solver (deer_solve_thresholds, csrc/thresholds.hip): the counts every solver starts from
(``value_net.exit_counts``, pinned as the integers ``solve_thresholds`` used before it called that function), the unchanged host solver on
the committed controller goldens, the budget search on the host solver (``solve_for_budget(engine=None)``, the yardstick of the device
form), ``predicted_exit_mix`` against a direct count, and the refusals of ``torch.ops.deer.solve_thresholds`` before the device is touched
(through its fake kernel on meta tensors).  No GPU needed."""
import pytest
import torch

from golden_util import load
from deer_vla_amd import ops
from deer_vla_amd import value_net as vn

EXITS = [1, 3, 5, 7, 9, 11]

# (n_sample, real_num_exit, exit_ratio, exit_dist, model_name) -> floor(n_sample * probs[k]) for every exit but the last, recorded from
# solve_thresholds' own loop before exit_counts existed
PINNED = [
    ((1000, 5, 0.8, "exp", "mpt_dolly_3b"), [297, 237, 190, 152]),
    ((1000, 5, 2.0, "gauss", "mpt_dolly_3b"), [54, 244, 402, 244]),
    ((1000, 5, 2.0, "gamma", "mpt_dolly_3b"), [204, 248, 225, 182]),
    ((1000, 5, 0.8, "exp", "mpt_9b"), [0, 338, 271, 216]),
    ((4099, 6, 1.2, "exp", "mpt_dolly_3b"), [412, 495, 594, 713, 855]),
    ((257, 16, 0.9, "exp", "mpt_dolly_3b"), [31, 28, 25, 22, 20, 18, 16, 15, 13, 12, 10, 9, 8, 8, 7]),
    ((63, 2, 0.5, "gauss", "mpt_9b"), [0]),
    ((1, 3, 1.0, "exp", "mpt_dolly_3b"), [0, 0]),
    ((50, 6, 1.0, "exp", "mpt_dolly_3b"), [8, 8, 8, 8, 8]),
    ((640, 6, 3.5, "gamma", "mpt_9b"), [0, 70, 117, 146, 155]),
]


@pytest.mark.parametrize("args,want", PINNED, ids=[f"{a[3]}-{a[2]}-n{a[0]}-{a[4]}" for a, _ in PINNED])
def test_exit_counts_are_the_integers_the_solver_used(args, want):
    got = vn.exit_counts(*args)
    assert len(got) == args[1] and all(type(c) is int for c in got)
    assert got[:-1] == want and got[-1] == 0                               # the last exit takes whoever is left
    assert vn.exit_counts(args[0], 1, args[2], args[3], args[4]) == [0]    # one exit: no count is computed (mpt_9b: probs would be 0 / 0)
    with pytest.raises(ValueError, match="Unsupported exit distribution"):
        vn.exit_counts(args[0], args[1], args[2], "poisson", args[4])


def test_solve_thresholds_still_returns_the_recorded_goldens():
    cfg, seed, g = load("thresholds.npz")
    values = g["values"]
    keys = [k for k in g if k.startswith("T_") or k.startswith("D_")]
    assert len(keys) >= 4
    for key in keys:
        if key.startswith("T_"):
            model_name, ratio, max_layer = key[2:].rsplit("_", 2)
            dist, leq = "exp", True
        else:
            _, dist, leq, ratio, max_layer = key.split("_")
            model_name, leq = "mpt_dolly_3b", bool(int(leq))
        ctl = vn.ExitController(None, cfg.exit_ids(), max_layer=int(max_layer), exit_dist=dist, leq=leq)
        n = ctl.real_num_exit
        T = vn.solve_thresholds(values[:n].clone(), n, float(ratio), dist, leq, model_name)
        assert torch.equal(T, g[key].float()), key
        # the two halves solve_thresholds is now made of, and the mix they report
        counts = vn.exit_counts(values.shape[1], n, float(ratio), dist, model_name)
        T2, left = vn.solve_from_counts(values[:n], counts, leq)
        assert torch.equal(T2, T) and left == _mix_by_loop(values, T.tolist(), leq), key


def _mix_by_loop(values, thresholds, leq):
    """how many samples leave at every exit: each sample walks the exits in order and leaves at the first whose criterion holds"""
    left = [0] * len(thresholds)
    for s in range(values.shape[1]):
        for e, t in enumerate(thresholds):
            v = float(values[e, s])
            if (v <= t if leq else v >= t) or e == len(thresholds) - 1:
                left[e] += 1
                break
    return left


@pytest.mark.parametrize("leq", [True, False])
def test_predicted_exit_mix_matches_a_direct_count(leq):
    g = torch.Generator().manual_seed(5)
    values = (torch.rand(6, 301, generator=g) * 8).floor() / 64            # eight levels: heavy ties
    for ratio, cap in [(0.7, 12), (1.3, 12), (1.0, 6)]:
        ctl = vn.ExitController(None, EXITS, max_layer=cap, leq=leq)
        ctl.set_threshold_from_values(values, ratio)
        thr = ctl.threshold_list()
        left = _mix_by_loop(values, thr, leq)
        _, solved = vn.solve_from_counts(values[: len(thr)], vn.exit_counts(301, len(thr), ratio), leq)
        assert solved == left and sum(left) == 301
        frac, avg = vn.predicted_exit_mix(solved, EXITS)
        assert frac == [c / 301 for c in left]
        assert avg == sum(c * (e + 1) for c, e in zip(left, EXITS)) / 301
        assert EXITS[0] + 1 <= avg <= ctl.max_layer + 1
    with pytest.raises(ValueError):
        vn.predicted_exit_mix([1] * 7, EXITS)
    with pytest.raises(ValueError):
        vn.predicted_exit_mix([0, 0], EXITS)


def _seeded_matrix(n=400):
    g = torch.Generator().manual_seed(11)
    return torch.rand(6, n, generator=g) * torch.tensor([0.08, 0.06, 0.05, 0.04, 0.03, 0.02]).unsqueeze(1)


@pytest.mark.parametrize("dist,leq,cap", [("exp", True, None), ("gauss", True, None), ("gamma", True, None), ("exp", False, None), ("exp", True, 6)])
def test_solve_for_budget_on_the_host_solver(dist, leq, cap):
    values = _seeded_matrix()
    n_exit = 6 if cap is None else 3
    budgets = (3.0, 4.5, 7.25, 11.0) if cap is None else (3.0, 4.5)
    if dist == "gamma":
        budgets = budgets[1:]                # its most front-loaded member still sends a third of the samples past the first exit
    for budget in budgets:
        trace = []
        ctl, ratio, (frac, avg) = vn.solve_for_budget(values, EXITS, budget, max_layer=cap, exit_dist=dist, leq=leq, grid=24, trace=trace)
        assert len(trace) == 2 and len(trace[0][0]) == len(trace[1][0]) == 24
        assert ctl.real_num_exit == n_exit and ctl.exit_dist == dist and ctl.leq is leq
        # the controller carries the thresholds of the chosen ratio, and the mix is theirs
        ref = vn.ExitController(None, EXITS, max_layer=cap if cap is not None else 12, exit_dist=dist, leq=leq)
        ref.set_threshold_from_values(values, ratio)
        assert ctl.threshold_list() == ref.threshold_list()
        left = _mix_by_loop(values, ctl.threshold_list(), leq)
        assert (frac, avg) == vn.predicted_exit_mix(left, EXITS)
        # at most the budget, and every grid point that predicts more lies above the budget: the next one up would exceed it
        assert avg <= budget
        every = [(a, r) for ratios, avgs in trace for r, a in zip(ratios, avgs)]
        assert (avg, ratio) in every
        above = [a for a, _ in every if a > avg]
        if above:
            assert min(above) > budget, (budget, avg, min(above))
        # the second round refines between the neighbours of the first round's choice, and never loses it
        r0, a0 = trace[0]
        i0 = max((i for i in range(24) if a0[i] <= budget), key=lambda i: (a0[i], -r0[i]))
        assert avg >= a0[i0]
        assert trace[1][0][0] == r0[max(i0 - 1, 0)] and trace[1][0][-1] == pytest.approx(r0[min(i0 + 1, 23)])
        assert all(trace[1][0][j] < trace[1][0][j + 1] for j in range(23))


def test_solve_for_budget_refuses_an_unreachable_budget():
    values = _seeded_matrix()
    with pytest.raises(ValueError, match=r"not reachable.*average exit layers 2\.\d+ \.\. "):
        vn.solve_for_budget(values, EXITS, 1.5)                            # below the first exit (layer 1: two layers run)
    with pytest.raises(ValueError, match="not reachable"):
        vn.solve_for_budget(values, EXITS, 2.0, exit_dist="gamma", grid=16)
    # a budget above everything the grid predicts is met by the latest-exiting point
    ctl, ratio, (_, avg) = vn.solve_for_budget(values, EXITS, 100.0, grid=16)
    assert avg <= 12.0 and avg > 10.0


def test_budget_grids():
    e = vn.budget_ratio_grid("exp", 6, 5)
    assert e[0] == 1 / 64 and e[-1] == pytest.approx(64.0) and e[2] == pytest.approx(1.0)
    assert vn.budget_ratio_grid("gauss", 6, 3) == [-3.0, 2.5, 8.0]
    assert vn.budget_ratio_grid("gamma", 4, 2) == [0.05, 6.0]
    assert vn.budget_ratio_grid("exp", 6, 3, 0.5, 2.0) == pytest.approx([0.5, 1.0, 2.0])
    with pytest.raises(ValueError):
        vn.budget_ratio_grid("poisson", 6, 4)


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_op_shapes_through_the_fake_kernel():
    for n_stage, n_sample, k, n_exit in [(6, 100, 1, 6), (6, 1, 65, 1), (16, 4099, 3, 16), (7, 33, 2, 3)]:
        T, left, status = torch.ops.deer.solve_thresholds(_meta(n_stage, n_sample), _meta(k, n_exit, dtype=torch.int32), True)
        assert tuple(T.shape) == (k, n_exit) and T.dtype == torch.float32
        assert tuple(left.shape) == (k, n_exit) and left.dtype == torch.int32
        assert tuple(status.shape) == (k,) and status.dtype == torch.int32
        assert ops.solve_thresholds_shapes(torch.zeros(n_stage, n_sample), torch.zeros(k, n_exit, dtype=torch.int64)) == (n_stage, n_sample, k, n_exit)


def test_op_refuses_bad_arguments():
    c = _meta(3, 6, dtype=torch.int32)
    for bad in (_meta(6 * 100), _meta(2, 6, 100), _meta(6, 100, dtype=torch.float64), _meta(6, 100, dtype=torch.float16)):
        with pytest.raises(ValueError, match=r"values must be \(n_stage, n_sample\) float32"):
            torch.ops.deer.solve_thresholds(bad, c, True)
    for bad in (_meta(18, dtype=torch.int32), _meta(3, 6, 1, dtype=torch.int32), _meta(3, 6), _meta(3, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match=r"counts must be \(k, n_exit\) integers"):
            torch.ops.deer.solve_thresholds(_meta(6, 100), bad, True)
    with pytest.raises(ValueError, match="at most 16"):
        torch.ops.deer.solve_thresholds(_meta(20, 100), _meta(3, 17, dtype=torch.int32), True)
    with pytest.raises(ValueError, match="values has 5 rows"):
        torch.ops.deer.solve_thresholds(_meta(5, 100), c, True)
    for v, cc in ((_meta(6, 0), c), (_meta(6, 100), _meta(0, 6, dtype=torch.int32)), (_meta(6, 100), _meta(3, 0, dtype=torch.int32))):
        with pytest.raises(ValueError, match="needs k >= 1"):
            torch.ops.deer.solve_thresholds(v, cc, True)
    # the helper itself, on host tensors: nothing is launched, no device is needed
    with pytest.raises(ValueError, match="float32"):
        ops.solve_thresholds_shapes(torch.zeros(6, 10, dtype=torch.float64), torch.zeros(1, 6, dtype=torch.int32))


def test_c_entry_refuses_bad_shapes_without_launching():
    """DEER_ERR_SHAPE comes back before anything is enqueued, so the refusals can be exercised without a device (the pointers are never
    dereferenced on the host)."""
    import ctypes
    from deer_vla_amd import _abi as abi
    lib = abi.lib()
    p = ctypes.c_void_p(4096)

    def call(n_stage=6, n_sample=100, ld=100, n_points=3, n_exit=6, values=p, out_n=p, alive=p, T=p, left=p, status=p):
        return lib.deer_solve_thresholds(values, n_stage, n_sample, ld, out_n, n_points, n_exit, 1, alive, T, left, status, None)

    for kw in (dict(n_exit=0), dict(n_exit=17, n_stage=20), dict(n_exit=6, n_stage=5), dict(n_sample=0, ld=0), dict(ld=99), dict(n_points=0),
               dict(values=None), dict(out_n=None), dict(alive=None), dict(T=None), dict(left=None), dict(status=None)):
        assert call(**kw) == 1, kw
