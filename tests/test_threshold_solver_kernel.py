"""deer_solve_thresholds (csrc/thresholds.hip) through ``torch.ops.deer.solve_thresholds`` against the host solver.

The yardstick is ``value_net.solve_thresholds`` on the CPU (for explicit counts: ``value_net.solve_from_counts``, the loop it is made of),
never the kernel itself.  Selection and counting are exact, so there is no tolerance: thresholds are compared with ``==`` (-0.0 equals
0.0: the kernel orders keys, where the two zeros differ, the host sorts floats, where they tie), exit counts with a host loop over the
exits that applies the HOST's thresholds.

Shapes: n_sample in {1, 63, 64, 65, 257, 4099} (below / at / above one wave, above one workgroup pass, a vector body with a scalar tail, many
passes), n_exit in {1, 2, 6, 16}, k in {1, 3, 65}, both criteria, the three distributions, seven value families - a thinned crossing of that
grid in which every value of every parameter occurs (asserted below)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from deer_vla_amd import ops  # noqa: E402,F401  (registers torch.ops.deer.*)
from deer_vla_amd import value_net as vn  # noqa: E402

N_SAMPLE = [1, 63, 64, 65, 257, 4099]
N_EXIT = [1, 2, 6, 16]
K = [1, 3, 65]
DISTS = ["exp", "gauss", "gamma"]
FAMILIES = ["uniform", "quant8", "equal", "signs", "subnormal", "sentinel", "inf"]


def make_values(family, n_stage, n_sample, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n_stage, n_sample, generator=g)
    pick = torch.randint(0, 8, (n_stage, n_sample), generator=g)
    if family == "uniform":
        return u
    if family == "quant8":                              # eight levels: ties everywhere
        return (u * 8).floor() / 8
    if family == "equal":
        return torch.full((n_stage, n_sample), 0.25)
    if family == "signs":                               # both signs, and both zeros
        v = u - 0.5
        v[pick == 0] = 0.0
        v[pick == 1] = -0.0
        return v
    if family == "subnormal":                           # |v| < 2^-126, either sign, some zeros
        bits = torch.randint(0, 1 << 23, (n_stage, n_sample), generator=g, dtype=torch.int32)
        bits = torch.where(pick < 4, bits, bits | torch.tensor(-(1 << 31), dtype=torch.int32))
        return bits.view(torch.float32)
    if family == "sentinel":                            # at and beyond the sentinels -1e8 / +1e8
        table = torch.tensor([-3e8, -1e8, -5e7, 1e8, 3e8, 5e7, 0.0, 0.0])
        return torch.where(pick < 6, table[pick], u)
    if family == "inf":
        v = u.clone()
        v[pick == 0] = float("inf")
        v[pick == 1] = float("-inf")
        return v
    raise KeyError(family)


def ratios_of(dist, n_exit, k):
    return vn.budget_ratio_grid(dist, n_exit, k) if k > 1 else [{"exp": 0.8, "gauss": 2.0, "gamma": 2.0}[dist]]


def mix_by_loop(values, T, leq):
    """the samples that leave at every exit under thresholds T: exits in order, whoever is alive and meets the criterion leaves"""
    alive = torch.ones(values.shape[1], dtype=torch.bool)
    left = []
    for e in range(len(T) - 1):
        out = alive & ((values[e] <= T[e]) if leq else (values[e] >= T[e]))
        left.append(int(out.sum()))
        alive &= ~out
    return left + [int(alive.sum())]


def device_solve(values, counts, leq):
    T, left, status = torch.ops.deer.solve_thresholds(values.cuda() if not values.is_cuda else values, torch.as_tensor(counts), leq)
    return T.cpu(), left.cpu(), status.cpu()


def check_against_host(values, counts, leq, host_T=None):
    """every point of ``counts`` against the host loop; host_T: thresholds already solved by value_net.solve_thresholds"""
    T, left, status = device_solve(values, counts, leq)
    assert T.dtype == torch.float32 and left.dtype == torch.int32 and status.tolist() == [0] * len(counts)
    for p, c in enumerate(counts):
        want = host_T[p] if host_T is not None else vn.solve_from_counts(values[: len(c)], list(c), leq)[0]
        assert bool((T[p] == want).all()), (p, list(c), T[p].tolist(), want.tolist())
        assert left[p].tolist() == mix_by_loop(values, want, leq), (p, list(c))
        assert int(left[p].sum()) == values.shape[1]
    return T, left


def _thinned():
    cases, i = [], 0
    for n_sample in N_SAMPLE:
        for n_exit in N_EXIT:
            cases.append((n_sample, n_exit, K[(i + i // 3) % 3], i % 2 == 0, DISTS[(i + i // 4) % 3], FAMILIES[i % 7]))
            i += 1
    return cases


CASES = _thinned()


def test_the_thinned_crossing_hits_every_value():
    for col, full in enumerate([N_SAMPLE, N_EXIT, K, [True, False], DISTS, FAMILIES]):
        assert {c[col] for c in CASES} == set(full), col
    for fam in FAMILIES:                                # every family meets both criteria and more than one point per call
        assert {c[3] for c in CASES if c[5] == fam} == {True, False} and max(c[2] for c in CASES if c[5] == fam) > 1, fam


@pytest.mark.parametrize("n_sample,n_exit,k,leq,dist,family", CASES, ids=["-".join(str(v) for v in c) for c in CASES])
def test_points_equal_the_host_solver(n_sample, n_exit, k, leq, dist, family):
    n_stage = n_exit + (1 if n_exit % 2 else 0)         # sometimes more rows than exits
    values = make_values(family, n_stage, n_sample, 1000 + n_sample + n_exit)
    ratios = ratios_of(dist, n_exit, k)
    counts = [vn.exit_counts(n_sample, n_exit, r, dist) for r in ratios]
    host_T = [vn.solve_thresholds(values[:n_exit], n_exit, r, dist, leq) for r in ratios]
    check_against_host(values, counts, leq, host_T)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("leq", [True, False])
def test_every_family_at_a_size_with_vector_body_and_tail(family, leq):
    """each family with each criterion at one size (257 = 64 vectors + 1), six exits, the mpt_9b rule (a zero first count) among the points"""
    values = make_values(family, 6, 257, 7)
    counts = [vn.exit_counts(257, 6, r, "exp") for r in (0.5, 0.8, 1.0, 1.25)] + [vn.exit_counts(257, 6, 0.8, "exp", "mpt_9b")]
    host_T = [vn.solve_thresholds(values, 6, r, "exp", leq) for r in (0.5, 0.8, 1.0, 1.25)] + [vn.solve_thresholds(values, 6, 0.8, "exp", leq, "mpt_9b")]
    check_against_host(values, counts, leq, host_T)


@pytest.mark.parametrize("leq", [True, False])
def test_count_edge_cases(leq):
    n = 65
    values = make_values("uniform", 4, n, 3)
    sentinel, last = (-1e8, 1e8) if leq else (1e8, -1e8)
    counts = [[0, 0, 0, 0],               # c = 0: nobody is asked for, nobody leaves
              [n, 5, 5, 0],               # c = n_sample: the first exit removes everyone
              [40, 30, 1, 0],             # c larger than the alive count (25) at the second exit; the third still selects
              [1, n - 1, 1, 0],           # exactly everyone who is left, then nobody left to select from
              [n + 1, -3, 1 << 30, 0],    # out of range either way: sentinel
              [10, 20, 30, 0]]
    T, left = check_against_host(values, counts, leq)
    assert T[0].tolist() == [sentinel] * 3 + [last] and left[0].tolist() == [0, 0, 0, n]
    assert T[1][1:].tolist() == [sentinel, sentinel, last] and left[1].tolist() == [n, 0, 0, 0]
    assert float(T[1][0]) == float(values[0].max() if leq else values[0].min())
    assert left[2].tolist()[0] == 40 and float(T[2][1]) == sentinel and left[2].tolist()[1:3] == [0, 1]
    assert left[3].tolist() == [1, n - 1, 0, 0] and float(T[3][2]) == sentinel
    assert T[4].tolist() == [sentinel] * 3 + [last] and left[4].tolist() == [0, 0, 0, n]
    assert left[5].tolist() == [10, 20, 30, 5]
    # values at or beyond the sentinel leave even where nothing was selected (value_net.py:259-261 applies the criterion regardless)
    v2 = values.clone()
    v2[0, :7] = -2e8 if leq else 2e8
    v2[1, 7:9] = sentinel
    _, left2 = check_against_host(v2, [[0, 0, 0, 0]], leq)
    assert left2[0].tolist() == [7, 2, 0, n - 9]


def test_row_stride_above_n_sample():
    n = 257
    wide = make_values("quant8", 6, n + 11, 9).cuda()
    counts = [vn.exit_counts(n, 6, r, "exp") for r in (0.7, 1.1)]
    for off in (4, 3):                                  # 16-byte aligned rows (268 columns: the vector body) and unaligned ones
        view = wide[:, off:off + n]
        assert view.stride(0) == n + 11 and not view.is_contiguous()
        a = torch.ops.deer.solve_thresholds(view, torch.tensor(counts), True)
        b = torch.ops.deer.solve_thresholds(view.contiguous(), torch.tensor(counts), True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        check_against_host(view.cpu(), counts, True)
    odd = make_values("uniform", 6, n + 2, 9).cuda()[:, 1:1 + n]    # ld % 4 != 0
    check_against_host(odd.cpu(), counts, True)
    a = torch.ops.deer.solve_thresholds(odd, torch.tensor(counts), True)
    b = torch.ops.deer.solve_thresholds(odd.contiguous(), torch.tensor(counts), True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_two_calls_are_bit_identical():
    values = make_values("quant8", 16, 4099, 21).cuda()
    counts = torch.tensor([vn.exit_counts(4099, 16, r, "exp") for r in vn.budget_ratio_grid("exp", 16, 65)])
    a = torch.ops.deer.solve_thresholds(values, counts, True)
    b = torch.ops.deer.solve_thresholds(values, counts, True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_nan_is_reported_and_raises_in_the_callers():
    from deer_vla_amd import synthetic as syn
    from deer_vla_amd.config import deer_tiny
    from deer_vla_amd.engine import DeerEngine
    exits = [1, 3, 5]
    values = make_values("uniform", 4, 130, 5)
    counts = [vn.exit_counts(130, 3, r, "exp") for r in (0.6, 1.0, 1.4)]
    planted = values.clone()
    planted[1, 77] = float("nan")                       # row 1 is read by a three-exit solve
    _, _, status = device_solve(planted, counts, True)
    assert all(s > 0 for s in status.tolist())
    _, _, status = device_solve(planted, [c[:2] for c in counts], True)
    assert status.tolist() == [0, 0, 0]                 # two exits read row 0 only
    unused = values.clone()
    unused[2:, 5] = float("nan")                        # the last exit's row and a row beyond the exits (n_stage > n_exit): never read
    _, _, status = device_solve(unused, counts, True)
    assert status.tolist() == [0, 0, 0]
    check_against_host(unused, counts, True, [vn.solve_thresholds(values[:3], 3, r) for r in (0.6, 1.0, 1.4)])

    cfg = deer_tiny()
    eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, 3, bf16_round=True))
    T, left = eng.solve_thresholds(unused.cuda(), counts)
    assert T.is_cuda and left.is_cuda and len(eng.solve_thresholds(unused.cuda(), counts, return_status=True)) == 3
    ok = vn.controllers_from_values(None, exits, unused.cuda(), [0.6, 1.0, 1.4], engine=eng)
    assert [c.thresholds for c in ok] == [c.thresholds for c in vn.controllers_from_values(None, exits, unused, [0.6, 1.0, 1.4])]
    with pytest.raises(ValueError, match="NaN in calibration values"):
        vn.controllers_from_values(None, exits, planted.cuda(), [0.6, 1.0, 1.4], engine=eng)
    with pytest.raises(ValueError, match="NaN in calibration values"):
        vn.ExitController(None, exits, max_layer=6).set_threshold_from_values(planted.cuda(), 0.8, engine=eng)
    with pytest.raises(ValueError, match="NaN in calibration values"):
        vn.solve_for_budget(planted.cuda(), exits, 4.0, engine=eng, grid=8)
