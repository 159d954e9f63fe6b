"""The device threshold solver at the public surface, on a tiny model: a value matrix that ``generate_action_values(fused=True)`` left
on the device goes through ``controllers_from_values(engine=...)`` / ``solve_for_budget(engine=...)`` without the matrix ever coming to
the host, and yields what the host solver yields on a copy of it - the same ``thresholds`` dicts (``==``: selection is exact), hence the
same exits in an env batch that carries all the operating points side by side."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_calibrate_values import _window_batch  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd import value_net as vn  # noqa: E402
from deer_vla_amd.config import deer_tiny  # noqa: E402
from deer_vla_amd.flamingo_mpt import MPTFlamingo  # noqa: E402

RATIOS, CAPS = [0.6, 1.0, 1.5], [6, 4]                 # three exit ratios x (every exit | the DeeR-S style cap: exits 1 and 3 only)
B = len(RATIOS) * len(CAPS)
W = 8


class _M:                                              # the bits of a model generate_action_values touches
    def __init__(self, e):
        self.module, self.engine = self, e


@pytest.fixture(scope="module")
def calibrated():
    cfg = deer_tiny()
    model = MPTFlamingo(cfg, syn.make_synthetic_state(cfg, 3, bf16_round=True), n_envs=B)
    exits = model.get_all_exit_idx()
    net = vn.ActionValueNet(exits, None, cfg.exit_interval, W, "L2")
    loader = [_window_batch(cfg, 3, W, 0), _window_batch(cfg, 2, W, 40)]
    values, _ = vn.generate_action_values(None, _M(model.engine), net, loader, generator=torch.Generator().manual_seed(4), fused=True)
    assert values.is_cuda and tuple(values.shape) == (len(exits), 5 * (W - W // 2))
    return cfg, model, exits, net, values, values.cpu()


def _points(exits, net, values, engine):
    pairs = [(r, m) for m in CAPS for r in RATIOS]
    return vn.controllers_from_values(net, exits, values, [r for r, _ in pairs], [m for _, m in pairs], engine=engine)


def test_controllers_equal_the_host_path_and_drive_the_same_exits(calibrated):
    cfg, model, exits, net, values, host_values = calibrated
    eng = model.engine
    calls = []
    solve = eng.solve_thresholds
    eng.solve_thresholds = lambda *a, **k: (calls.append(a[1].shape), solve(*a, **k))[1]
    try:
        dev_ctls = _points(exits, net, values, eng)
    finally:
        del eng.solve_thresholds
    host_ctls = _points(exits, net, host_values, None)
    assert [tuple(s) for s in calls] == [(3, 2), (3, 3)]                   # one call per group of points with the same number of exits
    for d, h in zip(dev_ctls, host_ctls):
        assert d.thresholds == h.thresholds and d.max_layer == h.max_layer and d.real_num_exit == h.real_num_exit
    assert len({tuple(c.threshold_list()) for c in dev_ctls}) == B         # six different operating points
    one = vn.ExitController(net, exits, max_layer=6)
    one.set_threshold_from_values(values, 1.0, engine=eng)
    assert one.thresholds == host_ctls[1].thresholds

    def episode(ctls):
        eng.reset()
        out = []
        for s in range(5):
            per_env = [syn.synthetic_step_inputs(cfg, s, rank=e) for e in range(B)]
            rgb, grip = torch.cat([p[0] for p in per_env]).cuda(), torch.cat([p[1] for p in per_env]).cuda()
            ids = torch.cat([p[2] for p in per_env]).cuda()
            pose, g, ex = model.step_env_batch(rgb, ids, None, grip, exit_controller=ctls)
            out.append((pose.clone(), ex))
        return out

    got, want = episode(dev_ctls), episode(host_ctls)
    for (pa, ea), (pb, eb) in zip(got, want):
        assert ea == eb and torch.equal(pa, pb)
        assert all(x <= c.max_layer for x, c in zip(ea, dev_ctls))


@pytest.mark.parametrize("dist", ["exp", "gauss"])
def test_budget_solve_equals_the_host_search_in_two_device_calls(calibrated, dist):
    cfg, model, exits, net, values, host_values = calibrated
    eng = model.engine
    top = vn.solve_for_budget(host_values, exits, 100.0, exit_dist=dist, grid=16)[2][1]      # the latest-exiting point of the grid
    for budget in (3.0, 4.0, top):
        calls = []
        solve = eng.solve_thresholds
        eng.solve_thresholds = lambda *a, **k: (calls.append(a[1].shape), solve(*a, **k))[1]
        try:
            d_ctl, d_ratio, d_mix = vn.solve_for_budget(values, exits, budget, exit_dist=dist, engine=eng, grid=16)
        finally:
            del eng.solve_thresholds
        h_ctl, h_ratio, h_mix = vn.solve_for_budget(host_values, exits, budget, exit_dist=dist, grid=16)
        assert len(calls) == 2 and all(tuple(s) == (16, len(exits)) for s in calls)
        assert d_ratio == h_ratio and d_ctl.thresholds == h_ctl.thresholds and d_mix == h_mix
        assert d_mix[1] <= budget
    with pytest.raises(ValueError, match="not reachable"):
        vn.solve_for_budget(values, exits, 1.0, exit_dist=dist, engine=eng, grid=16)
