"""deer_value_log_append (csrc/value_log.hip) against a numpy restatement, bit for bit: control blocks of random 32-bit words are
planted, appended through ``torch.ops.deer.value_log_append`` and the WHOLE buffers - value rows with their padding columns (ld >
capacity), a guard region behind them, the exit layers taken and the three state words - are compared as integers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from deer_vla_amd import _abi as abi  # noqa: E402
from deer_vla_amd import ops  # noqa: E402,F401  (registers torch.ops.deer.*)

W, DELTAS, LAYER = abi.CTL_WORDS, abi.CTL_DELTAS, abi.CTL_EXIT_LAYER
GUARD = 64
FILL_V, FILL_T = 0xDEADBEEF, -77


def _ctl(rng, n_envs):
    """n_envs control blocks of random words: every word the kernel must NOT read is noise too"""
    return rng.integers(0, 1 << 32, size=(n_envs, W), dtype=np.uint64).astype(np.uint32)


def _nonfinite(u):
    return (u & 0x7F800000) == 0x7F800000


class Log:
    """the device buffers of one log and their numpy model"""

    def __init__(self, n_exit, capacity, ld, count=0):
        self.n_exit, self.capacity, self.ld = n_exit, capacity, ld
        self.v = np.full(n_exit * ld + GUARD, FILL_V, dtype=np.uint32)
        self.t = np.full(capacity + GUARD, FILL_T, dtype=np.int32)
        self.s = np.array([count, 0, 0], dtype=np.int32)
        self.dv = torch.from_numpy(self.v.view(np.int32).copy()).cuda()
        self.dt = torch.from_numpy(self.t.copy()).cuda()
        self.ds = torch.from_numpy(self.s.copy()).cuda()

    def append(self, ctl, mask):
        n_envs = ctl.shape[0]
        # the numpy restatement
        rows = self.v[: self.n_exit * self.ld].reshape(self.n_exit, self.ld)
        count, written, active = int(self.s[0]), 0, 0
        for b in range(n_envs):
            if not (mask >> b) & 1:
                continue
            slot = count + active
            active += 1
            if slot >= self.capacity:
                continue
            rows[:, slot] = ctl[b, DELTAS: DELTAS + self.n_exit]
            self.t[slot] = ctl[b].view(np.int32)[LAYER]
            self.s[2] += int(_nonfinite(ctl[b, DELTAS: DELTAS + self.n_exit]).sum())
            written += 1
        self.s[0] += written
        self.s[1] += active - written
        # the device
        d_ctl = torch.from_numpy(ctl.view(np.int32).reshape(-1).copy()).cuda()
        values = self.dv[: self.n_exit * self.ld].view(torch.float32).view(self.n_exit, self.ld)
        torch.ops.deer.value_log_append(d_ctl, n_envs, self.n_exit, mask, values, self.capacity, self.dt[: self.capacity], self.ds)

    def check(self, what):
        torch.cuda.synchronize()
        assert np.array_equal(self.ds.cpu().numpy(), self.s), (what, self.ds.cpu().numpy(), self.s)
        assert np.array_equal(self.dt.cpu().numpy(), self.t), what
        assert np.array_equal(self.dv.cpu().numpy().view(np.uint32), self.v), what
        return self.dv.cpu().numpy().copy(), self.dt.cpu().numpy().copy(), self.ds.cpu().numpy().copy()


def _masks(n_envs):
    full = (1 << n_envs) - 1
    return {"all": full, "none": 0, "alternating": 0x5555 & full, "last": 1 << (n_envs - 1)}


@pytest.mark.parametrize("n_envs", [1, 3, 16])
@pytest.mark.parametrize("n_exit", [1, 2, 6, 16])
def test_appends_accumulate_bit_for_bit(n_envs, n_exit):
    for name, mask in _masks(n_envs).items():
        runs = []
        for _ in range(2):                                                # two runs identical
            rng = np.random.default_rng(100 * n_envs + n_exit)
            log = Log(n_exit, capacity=3 * n_envs + 2, ld=3 * n_envs + 7)   # ld > capacity (and no multiple of 4); room for three appends
            log.append(_ctl(rng, n_envs), mask)
            log.check((name, 1))
            log.append(_ctl(rng, n_envs), mask)
            log.check((name, 2))
            log.append(_ctl(rng, n_envs), _masks(n_envs)["all"])          # a third append behind the two, every environment
            runs.append(log.check((name, 3)))
            assert log.s[0] == 2 * bin(mask).count("1") + n_envs and log.s[1] == 0
        assert all(np.array_equal(a, b) for a, b in zip(*runs)), name


def test_full_log_drops_columns_and_writes_nothing_past_capacity():
    rng = np.random.default_rng(5)
    for n_exit, capacity, ld in ((6, 9, 9), (3, 9, 13), (16, 1, 4)):
        log = Log(n_exit, capacity, ld, count=capacity - 1)
        before = log.v.copy()
        ctl = _ctl(rng, 5)
        log.append(ctl, 0b10110)                                           # three active environments, room for one column
        v, t, s = log.check((n_exit, capacity, ld))
        assert list(s[:2]) == [capacity, 2]
        rows = v.view(np.uint32)[: n_exit * ld].reshape(n_exit, ld)
        assert np.array_equal(rows[:, capacity - 1], ctl[1, DELTAS: DELTAS + n_exit])          # environment 1, the lowest set bit
        changed = np.flatnonzero(v.view(np.uint32) != before)
        assert set(changed) <= {e * ld + capacity - 1 for e in range(n_exit)}
        assert (v.view(np.uint32)[n_exit * ld:] == FILL_V).all() and (t[capacity:] == FILL_T).all()   # the guard regions
        log.append(_ctl(rng, 5), 0b11111)                                  # a full log: everything dropped, nothing written
        _, _, s = log.check("full")
        assert list(s[:2]) == [capacity, 7]


def test_special_values_are_copied_bitwise_and_counted():
    specials = np.array([0x00000000, 0x80000000,                           # +0, -0
                         0x00000001, 0x807FFFFF, 0x00400000,               # subnormals
                         0x7F800000, 0xFF800000,                           # +inf, -inf
                         0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFBFFFFF, 0x7FFFFFFF,   # quiet and signalling NaNs with payloads
                         0x7F7FFFFF, 0x00800000, 0x3F800000, 0xBF800000], dtype=np.uint32)
    n_nonfinite = int(_nonfinite(specials).sum())
    assert n_nonfinite == 7
    rng = np.random.default_rng(9)
    ctl = _ctl(rng, 4)
    for b in range(4):
        ctl[b, DELTAS: DELTAS + 16] = np.roll(specials, 5 * b)
    log = Log(16, capacity=8, ld=10)
    log.append(ctl, 0b1111)
    v, _, s = log.check("specials")
    assert list(s) == [4, 0, 4 * n_nonfinite]
    rows = v.view(np.uint32)[: 16 * 10].reshape(16, 10)
    for b in range(4):
        assert np.array_equal(rows[:, b], np.roll(specials, 5 * b))
    log6 = Log(6, capacity=8, ld=10)                                       # only the first n_exit deltas count
    log6.append(ctl, 0b0101)
    _, _, s = log6.check("specials, 6 exits")
    assert list(s) == [2, 0, int(_nonfinite(specials[:6]).sum()) + int(_nonfinite(np.roll(specials, 10)[:6]).sum())]
