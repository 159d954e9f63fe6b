"""Host side of the one-pass threshold calibration (deer_calibrate_values, csrc/calib.hip): argument validation of
``torch.ops.deer.calibrate_values`` (through its fake kernel on meta tensors - no device touched), the layer -> slot table, and
``generate_action_values(fused=True)`` drawing the same random layers as the per-step path.  No GPU needed."""
import dataclasses

import pytest
import torch

from deer_vla_amd import ops
from deer_vla_amd.config import deer_tiny
from deer_vla_amd.value_net import ActionValueNet, ExitController, generate_action_values


class _StubModel:
    """what ops._model() hands to the op's host-side checks"""
    def __init__(self, cfg, exit_ids=None):
        self.cfg, self.exit_ids = cfg, list(exit_ids if exit_ids is not None else cfg.exit_ids())


@pytest.fixture
def handle():
    cfg = deer_tiny()
    h = 0x7E57
    ops._MODELS[h] = _StubModel(cfg)
    yield h, cfg
    ops._MODELS.pop(h, None)


def _meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_op_shapes_through_the_fake_kernel(handle):
    h, cfg = handle
    NL, d = len(cfg.exit_ids()) + 1, cfg.d_model
    for bs, W in [(1, 2), (3, 4), (20, 12), (2, 5)]:
        out = torch.ops.deer.calibrate_values(_meta(bs, W, NL, d), _meta(bs, W, dtype=torch.int32), h, "L2")
        assert tuple(out.shape) == (NL - 1, bs * (W - W // 2)) and out.dtype == torch.float32


def test_op_refuses_bad_arguments(handle):
    h, cfg = handle
    NL, d = len(cfg.exit_ids()) + 1, cfg.d_model
    rl = _meta(2, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"\(bs, W, NL, d\)"):
        torch.ops.deer.calibrate_values(_meta(2 * 8, NL, d), rl, h, "L2")                      # wrong rank
    with pytest.raises(ValueError, match="W >= 2"):
        torch.ops.deer.calibrate_values(_meta(2, 1, NL, d), _meta(2, 1, dtype=torch.int32), h, "L2")
    with pytest.raises(ValueError, match="candidate layers"):
        torch.ops.deer.calibrate_values(_meta(2, 8, NL + 1, d), rl, h, "L2")                   # NL does not match the exit list
    with pytest.raises(ValueError, match="candidate layers"):
        torch.ops.deer.calibrate_values(_meta(2, 8, NL, d + 8), rl, h, "L2")
    with pytest.raises(ValueError, match="rand_layers must be"):
        torch.ops.deer.calibrate_values(_meta(2, 8, NL, d), _meta(2, 7, dtype=torch.int32), h, "L2")
    with pytest.raises(NotImplementedError):
        torch.ops.deer.calibrate_values(_meta(2, 8, NL, d), rl, h, "chebyshev")
    with pytest.raises(Exception, match="unknown model handle"):
        torch.ops.deer.calibrate_values(_meta(2, 8, NL, d), rl, h + 1, "L2")


def test_rand_layers_must_be_exit_layers():
    cfg = deer_tiny()
    exits = cfg.exit_ids()
    NL, d = len(exits) + 1, cfg.d_model
    ok = torch.tensor([[exits[i % len(exits)] for i in range(4)]] * 2)
    assert ops.calibrate_shapes(cfg, exits, (2, 4, NL, d), ok) == (2, 4, NL, 2, 1)
    for bad_layer in (0, 2, -1, cfg.n_layers):                                                 # layer 0 is a candidate, never a history layer
        bad = ok.clone()
        bad[1, 2] = bad_layer
        with pytest.raises(ValueError, match="not exit layers"):
            ops.calibrate_shapes(cfg, exits, (2, 4, NL, d), bad)


def test_use_state_is_refused():
    cfg = dataclasses.replace(deer_tiny(), use_state=True)
    exits = cfg.exit_ids()
    with pytest.raises(NotImplementedError, match="use_state"):
        ops.calibrate_shapes(cfg, exits, (1, 4, len(exits) + 1, cfg.d_model), torch.full((1, 4), exits[0]))
    h = 0x7E58
    ops._MODELS[h] = _StubModel(cfg)
    try:
        with pytest.raises(NotImplementedError, match="use_state"):
            torch.ops.deer.calibrate_values(_meta(1, 4, len(exits) + 1, cfg.d_model), _meta(1, 4, dtype=torch.int32), h, "L2")
    finally:
        ops._MODELS.pop(h, None)


def test_layer_slot_table():
    assert ops.calib_layer_slots([1, 3, 5], 6) == [0, 1, -1, 2, -1, 3]
    assert ops.calib_layer_slots([1, 3, 5, 7, 9, 11, 12], 13) == [0, 1, -1, 2, -1, 3, -1, 4, -1, 5, -1, 6, 7]
    assert ops.calib_layer_slots([4], 5) == [0, -1, -1, -1, 1]
    for bad in ([], [0, 2], [3, 1], [2, 2], [1, 6]):                                           # layer 0 among the exits: value_net.py:135
        with pytest.raises(ValueError):
            ops.calib_layer_slots(bad, 6)


class _StubEngine:
    """records the random layers each calibration path is handed (the bits of DeerEngine generate_action_values touches)"""
    dev, img_dtype = torch.device("cpu"), torch.float32

    def __init__(self, n_exit, d=8):
        self.n_exit, self.d, self.rand, self.calls = n_exit, d, [], []

    def window_hidden_states(self, rgb, grip, ids, mask=None, group=8):
        self.calls.append("hidden")
        return torch.zeros(rgb.shape[0], 4, ids.shape[-1], self.d)

    def generate_values(self, hidden, rand_layers, threshold_type="L2", group=8):
        self.calls.append("loop")
        self.rand.append(torch.as_tensor(rand_layers).clone())
        bs, W = hidden.shape[:2]
        return torch.zeros(self.n_exit, bs * (W - W // 2))

    def window_exit_features(self, rgb, grip, ids, mask=None, group=8):
        self.calls.append("pooled")
        return torch.zeros(rgb.shape[0], self.n_exit + 1, self.d)

    def calibrate_values(self, feats, rand_layers, threshold_type="L2", return_actions=False):
        self.calls.append("fused")
        assert feats.dim() == 4 and feats.shape[2] == self.n_exit + 1
        self.rand.append(torch.as_tensor(rand_layers).clone())
        bs, W = feats.shape[:2]
        return torch.zeros(self.n_exit, bs * (W - W // 2))


class _M:
    def __init__(self, e):
        self.module, self.engine = self, e


def _loader(W, sizes, S=4, T=5):
    for bs in sizes:
        ids = torch.ones(bs, T, dtype=torch.long)
        yield (torch.zeros(bs, W, 3, S, S), (ids, torch.ones_like(ids)), None, torch.zeros(bs, W, 3, S, S))


@pytest.mark.parametrize("W", [2, 8, 12])
def test_fused_draws_the_same_random_layers(W):
    exits = [1, 3, 5, 7, 9, 11]
    vn = ActionValueNet(exits, None, 2, W, "L2")
    runs = {}
    for fused in (False, True):
        e = _StubEngine(len(exits))
        vals, _ = generate_action_values(None, _M(e), vn, _loader(W, [3, 2]), generator=torch.Generator().manual_seed(11), fused=fused)
        assert tuple(vals.shape) == (len(exits), 5 * (W - W // 2))
        runs[fused] = e
    assert runs[False].calls == ["hidden", "loop"] * 2 and runs[True].calls == ["pooled", "fused"] * 2
    assert len(runs[True].rand) == 2
    for a, b in zip(runs[False].rand, runs[True].rand):
        assert a.shape == b.shape and torch.equal(a, b) and set(a.reshape(-1).tolist()) <= set(exits)
    # the generator ends in the same state: what is drawn after the calibration is the same too
    g1, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    generate_action_values(None, _M(_StubEngine(len(exits))), vn, _loader(W, [3]), generator=g1, fused=False)
    generate_action_values(None, _M(_StubEngine(len(exits))), vn, _loader(W, [3]), generator=g2, fused=True)
    assert torch.equal(g1.get_state(), g2.get_state())


def test_set_threshold_routes_fused(monkeypatch):
    exits = [1, 3, 5]
    vn = ActionValueNet(exits, None, 2, 4, "L2")
    e = _StubEngine(len(exits))
    ctl = ExitController(vn, exits, max_layer=6)
    monkeypatch.setattr("deer_vla_amd.distributed.all_gather_values", lambda v: v)
    ctl.set_threshold(None, _M(e), _loader(4, [2]), 0.8, "mpt_dolly_3b", fused=True)
    assert e.calls == ["pooled", "fused"] and len(ctl.threshold_list()) == 3


@pytest.mark.parametrize("variant", ["ln_max", "plain", "avg", "ms2"])
def test_cosine_condition_of_the_committed_oracle_inputs(variant):
    """tests/test_calibrate_values.py compares cosine values with the oracle wherever both oracle actions of a pair have a norm >= 0.1, on
    condition that at most 10 % of the pairs of a parametrisation are left out.  The oracle alone decides that, so it is checked here, on the
    very inputs of that test (the engine's precision plays no part)."""
    import test_calibrate_values as tcv
    assert list(tcv.VARIANTS) == ["ln_max", "plain", "avg", "ms2"]
    pool = tcv._tiny_oracle_hidden()
    cfg = deer_tiny(**tcv.VARIANTS[variant])
    head = tcv._ZeroStartHead(tcv.syn.make_synthetic_state(cfg, 3, bf16_round=True), cfg, "extra_exit.")
    exit_ids = cfg.exit_ids()
    pairs = left_out = 0
    for bs in tcv.BS_TINY:
        for W in tcv.W_TINY:
            ok = tcv._cosine_comparable(tcv._oracle_actions(head, exit_ids, *tcv._tiny_case(pool, exit_ids, bs, W)))
            pairs, left_out = pairs + ok.numel(), left_out + int((~ok).sum())
    print(f"{variant}: {left_out} of {pairs} cosine pairs have an oracle action of norm < {tcv.COS_MIN_NORM}")
    assert pairs > 0 and left_out <= tcv.COS_MAX_LEFT_OUT * pairs
