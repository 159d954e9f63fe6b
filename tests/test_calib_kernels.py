"""The calibration kernels (csrc/calib.hip) one entry point at a time, through the C ABI, against float64 references built from the
committed oracle's pieces (oracle/deer_oracle.py: lstm_cell, get_delta, _lin, _ln) or plain torch on the weights exactly as the device holds
them (bf16 / f32 / fp16 rows, w_kind 0 / 1 / 2); then the launch sequence of ``deer_calibrate_values`` (csrc/model.hip) re-chained on the host
from those entry points and compared with the composed call bit for bit.  Every output buffer starts as NaN: every in-range element must be
written, nothing past an edge may be.

Gates (none is measured; each is a project constant or an operation count).
  copies        deer_calib_gather (rows and index words), max pooling, T = 1 pooling of either kind, the orchestration: bit for bit.
  mean pooling  the gate of test_head_kernels._check_pool: a sequential f32 sum of T values, then one division:
                |err| <= mean|x| (T + 1) 2^-24 + |mean| 2^-24.
  LSTM step     test_head_kernels.test_head_seq_lstm_step's: SEQ_TOL[w_kind] (the 16-bit plane split of the f32 activation: bf16 4 x 2^-17,
                fp16 8 x 2^-22, f32 weights 4e-6 summation order) + 2^-22 (the f32 transcendentals of the cell), relative to the largest
                |pre| + |h| |W_hh|^T + |b_hh| of the unit's four gate rows; 2 x for c (|dc| <= |df| |c| / 4 + |di| / 4 + |dg|), 3 x for h
                (+ |do| / 4).  The reference of a step takes the DEVICE's previous state as its input, so steps do not compound.
  deltas        L2 / mean / max: every term is non-negative, so the f32 result is a rounding chain of at most NP + 4 operations (subtract,
                square, NP adds, divide, square root) on the fp64 value: (NP + 4) 2^-23 RELATIVE.  cosine: the normalised terms are <= 1
                and 1 - ab cancels, so the same chain (two more divisions and the norm's root per term) is ABSOLUTE: (NP + 8) 2^-23, on
                inputs whose norms are >= 0.1 (asserted), where the eps clamp is far away.
Row independence of the LSTM step (a row alone == the row in a 70-row launch; an index of -1 == an index to a row of real zeros) is
``torch.equal``."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_calibrate_values import VARIANTS, _rand_layers, _small_towers  # noqa: E402
from deer_vla_amd import _abi as abi  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_tiny  # noqa: E402
from deer_vla_amd.engine import DeerEngine  # noqa: E402
from oracle import deer_oracle as orc  # noqa: E402

SEQ_TOL = {0: 4 * 2.0 ** -17, 1: 4e-6, 2: 8 * 2.0 ** -22}    # tests/test_head_kernels.py
WKINDS = [0, 1, 2]
_WDT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float16}
NAN = float("nan")
HUGE = 1e30
MAX_NL = 17                                                  # DEER_CALIB_MAX_NL
THR = ["L2", "mean", "max", "cosine"]                        # thr_type 0 .. 3 (abi.THR_TYPES)
EPI_NONE, EPI_RELU, EPI_TANH, EPI_SIGMOID_LOGIT = 0, 1, 2, 3  # DEER_SEQ_EPI_*


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def cu(t):
    return t.to("cuda").contiguous()


def nanbuf(*shape):
    return torch.full(shape, NAN, device="cuda")


def wq(w, wk):
    """(device rows in weight kind wk, float64 copy of exactly those values)"""
    q = w.to(_WDT[wk])
    return cu(q), q.double()


def gate(out, ref, scale, tol, what):
    """|out - ref| <= tol * scale elementwise; every element written (no NaN)"""
    out = out.detach().double().cpu()
    assert torch.isfinite(out).all(), f"{what}: unwritten / non-finite outputs"
    r = float(((out - ref).abs() / scale).max())
    assert r <= tol, f"{what}: max |err| / scale = {r:.3g} > {tol:.3g}"
    return r


def sync():
    torch.cuda.synchronize()


def same(a, b):
    """bit-for-bit up to the payload of a NaN: the same NaN positions, equal values everywhere else"""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.fixture(scope="module")
def lib():
    l = abi.lib()
    assert l.deer_hip_arch() == b"gfx950"
    return l


def test_thr_type_numbers():
    assert [abi.THR_TYPES[n] for n in THR] == [0, 1, 2, 3]


# ================================================================================================ 1. deer_calib_pool_layers
def _layers(NL):
    """NL non-contiguous layers of NL + 2 with 0 and the last one: 1 and the last but one are left out"""
    n_layers = NL + 2
    lay = [l for l in range(n_layers) if l not in (1, n_layers - 2)]
    assert len(lay) == NL and lay[0] == 0 and lay[-1] == n_layers - 1
    return n_layers, lay


@pytest.mark.parametrize("d", [1000, 2048, 4096])
@pytest.mark.parametrize("T", [1, 5, 33])
@pytest.mark.parametrize("n_frames,NL", [(1, 2), (1, MAX_NL), (3, 7), (16, 2), (16, MAX_NL)])
def test_calib_pool_layers(lib, n_frames, NL, T, d):
    """P[frame][k] = max / mean over the T rows of frame `frame` of hidden[layers[k]], with the engine's layout: the layer stride is
    larger than n_frames T d (rows_cap > n_frames T).  A layer that is not asked for and the rows after the last frame hold 1e30: neither
    may reach P.  d = 1000 leaves a partial 1024-column block, d = 4096 runs blockIdx.z > 0."""
    n_layers, lay = _layers(NL)
    rows, rows_cap = n_frames * T, n_frames * T + 5
    hidden = rnd(n_layers, rows_cap, d, seed=1000 * n_frames + 10 * T + NL)
    hidden[:, rows:] = HUGE
    hidden[1] = HUGE
    hidden[n_layers - 2] = -HUGE
    hd = cu(hidden)
    feats = hidden[lay][:, :rows].reshape(NL, n_frames, T, d).permute(1, 0, 2, 3).reshape(n_frames * NL, T, d).double()
    for avg in (0, 1):
        P = nanbuf(n_frames * NL + 1, d)                     # + one row that must stay NaN
        abi.check(lib.deer_calib_pool_layers(abi.ptr(hd), rows_cap * d, (ctypes.c_int * NL)(*lay), NL, abi.ptr(P), n_frames, T, d, avg, st()), "pool_layers")
        sync()
        assert bool(torch.isnan(P[-1]).all()), "stores past the last (frame, layer) row"
        out = P[:-1].cpu()
        if not avg or T == 1:                                # max, and one row of either kind (x / 1.0f): exact
            assert torch.equal(out, (feats.mean(1) if avg else feats.amax(1)).float()), f"avg={avg}"
            continue
        ref, mag = feats.mean(1), feats.abs().mean(1)
        gate(out, ref, mag * (T + 1) * 2.0 ** -24 + ref.abs() * 2.0 ** -24 + 1e-30, 1.0, "mean pooling")   # sequential f32 sum of T values, then / T


# ================================================================================================ 2. deer_calib_gather
def _gather_ref(P, rl, slot_of, W):
    """the comment above calib_gather_kernel on the host: history rows (b, t < W - 1) = P[b][t][slot(rand_layers[b][t])] (no slot: NaN),
    then candidate rows (k, b, s) = P[b][W/2 - 1 + s][k] with idx = history row (b, W/2 - 2 + s), or -1 before step 0"""
    bc, _, NL, d = P.shape
    S, t0 = W - W // 2, W // 2 - 1
    slot = lambda l: slot_of[l] if 0 <= l < len(slot_of) else -1                                        # noqa: E731
    hist = [P[b, t, slot(int(rl[b, t]))] if slot(int(rl[b, t])) >= 0 else torch.full((d,), NAN) for b in range(bc) for t in range(W - 1)]
    cand = [P[b, t0 + s, k] for k in range(NL) for b in range(bc) for s in range(S)]
    idx = [b * (W - 1) + t0 + s - 1 if t0 + s > 0 else -1 for _ in range(NL) for b in range(bc) for s in range(S)]
    return torch.stack(hist + cand), torch.tensor(idx, dtype=torch.int32)


def _gather(lib, P, rl, slot_of, W):
    bc, _, NL, d = P.shape
    Rc = NL * bc * (W - W // 2)
    R = bc * (W - 1) + Rc
    X = nanbuf(R + 1, d)
    idx = torch.full((Rc + 3,), -7777, dtype=torch.int32, device="cuda")
    Pd, rld = cu(P), cu(rl.to(torch.int32))
    abi.check(lib.deer_calib_gather(abi.ptr(Pd), abi.ptr(rld), (ctypes.c_int * len(slot_of))(*slot_of), len(slot_of), abi.ptr(X), abi.ptr(idx), bc, W, NL,
                                    d, st()), "gather")
    sync()
    assert bool(torch.isnan(X[R]).all()) and idx[Rc:].tolist() == [-7777] * 3, "stores past the last row"
    return X[:R].cpu(), idx[:Rc].cpu()


def _slots(NL):
    """layer -> slot over 2 NL + 1 layers: even layers hold the slots (in a scrambled order), odd layers have none"""
    n_layers = 2 * NL + 1
    slot_of = [-1] * n_layers
    for k in range(NL):
        slot_of[2 * ((3 * k + 1) % NL) if NL % 3 else 2 * k] = k
    assert sorted(s for s in slot_of if s >= 0) == list(range(NL))
    return slot_of


@pytest.mark.parametrize("NL,d", [(2, 1000), (2, 2048), (7, 1000), (7, 2048)])
@pytest.mark.parametrize("bc", [1, 3, 20])
@pytest.mark.parametrize("W", [2, 3, 4, 5, 7, 12])
def test_calib_gather(lib, W, bc, NL, d):
    """every X row of both regions and every index word, bit for bit; rand_layers[b][W - 1] is never read (an out-of-range value there leaves
    no NaN); the zero-state index -1 appears exactly where W/2 - 1 + s == 0, i.e. in the s = 0 rows of W = 2 and W = 3"""
    slot_of = _slots(NL)
    have = [l for l, s in enumerate(slot_of) if s >= 0]
    P = rnd(bc, W, NL, d, seed=100 * W + bc)
    g = torch.Generator().manual_seed(W + 7 * bc)
    rl = torch.tensor(have)[torch.randint(0, NL, (bc, W), generator=g)]
    rl[:, W - 1] = 9999
    X, idx = _gather(lib, P, rl, slot_of, W)
    X_ref, idx_ref = _gather_ref(P, rl, slot_of, W)
    assert not bool(torch.isnan(X).any())
    assert torch.equal(X, X_ref)
    assert torch.equal(idx, idx_ref)
    S = W - W // 2
    minus = (idx.view(NL, bc, S) == -1)
    assert bool(minus[:, :, 0].all()) == (W in (2, 3)) and not bool(minus[:, :, 1:].any())


@pytest.mark.parametrize("W", [2, 5, 12])
def test_calib_gather_layer_without_slot(lib, W):
    """a random layer without a slot, a negative one and one >= n_layers give all-NaN rows in exactly those history rows; the candidate rows
    and the index words do not change"""
    bc, NL, d = 3, 7, 1000
    slot_of = _slots(NL)
    n_layers = len(slot_of)
    have = [l for l, s in enumerate(slot_of) if s >= 0]
    P = rnd(bc, W, NL, d, seed=W)
    rl = torch.tensor([[have[(b + 2 * t) % NL] for t in range(W)] for b in range(bc)])
    bad = [(0, 0, 1), (1, (W - 2) // 2, -3), (2, W - 2, n_layers), (2, 0, n_layers + 50), (1, W - 2, -1)]   # (window, step < W - 1, layer)
    for b, t, lay in bad:
        rl[b, t] = lay
    rl[:, W - 1] = -5                                        # never read
    X, idx = _gather(lib, P, rl, slot_of, W)
    X_ref, idx_ref = _gather_ref(P, rl, slot_of, W)
    nan_rows = sorted({b * (W - 1) + t for b, t, _ in bad})
    assert torch.isnan(X).all(1).nonzero().flatten().tolist() == nan_rows
    assert torch.isnan(X).any(1).nonzero().flatten().tolist() == nan_rows
    assert same(X, X_ref) and torch.equal(idx, idx_ref)


# ================================================================================================ 3. deer_calib_lstm_step
_EYE = {}


def _cell_ref(pre64, h64, c64, whh64, b64):
    """oracle lstm_cell in fp64 with the identity as W_ih (its input half is `pre` itself), and per hidden unit the largest
    |pre| + |h| |W_hh|^T + |b_hh| of its four gate rows"""
    H = h64.shape[1]
    eye = _EYE.setdefault(H, torch.eye(4 * H, dtype=torch.float64))
    h2, c2 = orc.lstm_cell(pre64, h64, c64, eye, whh64, None, b64)
    mag = pre64.abs() + h64.abs() @ whh64.abs().t() + b64.abs()
    return h2, c2, torch.stack([mag[:, q * H:(q + 1) * H] for q in range(4)]).amax(0)


def _lstm(lib, pre, ld_pre, h_prev, ld_h, c_prev, ld_c, idx, zero_row, whh, wk, bhh, c_out, ld_co, h_out, ld_out, N, H):
    abi.check(lib.deer_calib_lstm_step(pre, ld_pre, h_prev, ld_h, c_prev, ld_c, idx, zero_row, abi.ptr(whh), wk, abi.ptr(bhh), c_out, ld_co, h_out,
                                       ld_out, N, H, st()), "calib_lstm_step")
    sync()


def _cand_idx(N, n_prev):
    """candidate row -> previous-state row: not monotone, with repeats and several -1 (every fifth row, and the last one)"""
    idx = [(7 * m + 3) % n_prev for m in range(N)]
    for m in range(N):
        if m % 4 == 3:
            idx[m] = idx[m - 1]
        if m % 5 == 2 or (N > 1 and m == N - 1):
            idx[m] = -1
    return idx


@pytest.mark.parametrize("wk", WKINDS)
@pytest.mark.parametrize("H", [16, 48, 1024])
@pytest.mark.parametrize("N", [1, 31, 33, 70])
def test_calib_lstm_step(lib, wk, N, H):
    """The two launch forms of deer_calibrate_values.  History: idx NULL, (h, c) of step t written into column block t of [N][L][H] buffers
    next to the block t - 1 it reads (row strides L 4H / L H); step 0 has h_prev = c_prev = NULL.  Only block t may change.  Candidates:
    an index into previous-state buffers of another row count, a zero row, c dropped (c_out NULL); and the same with h_prev NULL (every
    row from zero).  H = 16 / 48 leave k-slices of a wave past H; N = 1 / 31 / 33 / 70 are ragged 32-row tiles.

    seq_frag_mac_wide, the fp16 outlier path of the GEMM, is not reachable here: the recurrence calls seq_frag_mac (the recurrent input is
    an LSTM output, |h| < 1), so there is no |h_prev| > 65504 case."""
    whh, whh64 = wq(rnd(4 * H, H, seed=4, scale=H ** -0.5), wk)
    bhh = rnd(4 * H, seed=5, scale=0.1)
    bhh_d, b64 = cu(bhh), bhh.double()
    tol = SEQ_TOL[wk] + 2.0 ** -22
    # ---- history form
    L = 3
    pre = rnd(N, L, 4 * H, seed=N + H)
    pre_d = cu(pre)
    Y, CS = nanbuf(N, L, H), nanbuf(N, L, H)
    for t in range(L):
        y0, c0 = Y.clone(), CS.clone()
        hp = abi.ptr(Y, (t - 1) * H * 4) if t > 0 else None
        cp = abi.ptr(CS, (t - 1) * H * 4) if t > 0 else None
        _lstm(lib, abi.ptr(pre_d, t * 4 * H * 4), L * 4 * H, hp, L * H, cp, L * H, None, None, whh, wk, bhh_d, abi.ptr(CS, t * H * 4), L * H,
              abi.ptr(Y, t * H * 4), L * H, N, H)
        keep = [u for u in range(L) if u != t]
        assert same(Y[:, keep], y0[:, keep]) and same(CS[:, keep], c0[:, keep]), f"step {t} wrote outside its column block"
        zero = torch.zeros(N, H, dtype=torch.float64)
        h64, c64 = (y0[:, t - 1].double().cpu(), c0[:, t - 1].double().cpu()) if t > 0 else (zero, zero)
        h_ref, c_ref, S = _cell_ref(pre[:, t].double(), h64, c64, whh64, b64)
        gate(CS[:, t], c_ref, S, 2 * tol, f"history c, step {t}")
        gate(Y[:, t], h_ref, S, 3 * tol, f"history h, step {t}")
    # ---- candidate form: different row strides for every operand, so that one taken for another shows
    n_prev = N + 5
    ld_pre, ld_h, ld_c, ld_out = 4 * H + 8, H + 8, H + 4, H + 4
    pre = rnd(N, ld_pre, seed=N + H + 1)
    hp = torch.tanh(rnd(n_prev, ld_h, seed=2))
    cp = rnd(n_prev, ld_c, seed=3, scale=0.5)
    idx = _cand_idx(N, n_prev)
    pre_d, hp_d, cp_d, idx_d, zero_d = cu(pre), cu(hp), cu(cp), cu(torch.tensor(idx, dtype=torch.int32)), torch.zeros(H, device="cuda")
    sel = torch.tensor([max(i, 0) for i in idx])
    live = torch.tensor([float(i >= 0) for i in idx], dtype=torch.float64)[:, None]
    for use_h in (True, False):
        h_out = nanbuf(N + 1, ld_out)
        _lstm(lib, abi.ptr(pre_d), ld_pre, abi.ptr(hp_d) if use_h else None, ld_h, abi.ptr(cp_d) if use_h else None, ld_c, abi.ptr(idx_d),
              abi.ptr(zero_d) if use_h else None, whh, wk, bhh_d, None, 0, abi.ptr(h_out), ld_out, N, H)
        m = live if use_h else torch.zeros_like(live)
        h_ref, _, S = _cell_ref(pre[:, :4 * H].double(), hp[sel, :H].double() * m, cp[sel, :H].double() * m, whh64, b64)
        gate(h_out[:N, :H], h_ref, S, 3 * tol, f"candidate h (h_prev {'given' if use_h else 'NULL'})")
        assert bool(torch.isnan(h_out[:N, H:]).all()) and bool(torch.isnan(h_out[N]).all()), "stores past an edge"
    # c_out given in this form too: the cell state of the indexed rows
    h_out, c_out = nanbuf(N, ld_out), nanbuf(N + 1, H + 12)
    _lstm(lib, abi.ptr(pre_d), ld_pre, abi.ptr(hp_d), ld_h, abi.ptr(cp_d), ld_c, abi.ptr(idx_d), abi.ptr(zero_d), whh, wk, bhh_d, abi.ptr(c_out), H + 12,
          abi.ptr(h_out), ld_out, N, H)
    h_ref, c_ref, S = _cell_ref(pre[:, :4 * H].double(), hp[sel, :H].double() * live, cp[sel, :H].double() * live, whh64, b64)
    gate(c_out[:N, :H], c_ref, S, 2 * tol, "candidate c")
    gate(h_out[:, :H], h_ref, S, 3 * tol, "candidate h (c kept)")
    assert bool(torch.isnan(c_out[:N, H:]).all()) and bool(torch.isnan(c_out[N]).all())


@pytest.mark.parametrize("wk", WKINDS)
@pytest.mark.parametrize("H", [48, 1024])
def test_calib_lstm_step_row_independence(lib, wk, H):
    """a row of a 70-row candidate launch equals the same row launched alone; a row with idx = -1 equals the same row indexed to a row of
    real zeros in h_prev / c_prev: bit for bit (what lets deer_calibrate_values chunk its windows freely)"""
    N, n_prev = 70, 40
    whh, _ = wq(rnd(4 * H, H, seed=14, scale=H ** -0.5), wk)
    bhh_d = cu(rnd(4 * H, seed=15, scale=0.1))
    pre_d = cu(rnd(N, 4 * H, seed=16))
    hp, cp = torch.tanh(rnd(n_prev, H, seed=17)), rnd(n_prev, H, seed=18, scale=0.5)
    hp[n_prev - 1] = 0
    cp[n_prev - 1] = 0
    hp_d, cp_d, zero_d = cu(hp), cu(cp), torch.zeros(H, device="cuda")
    idx = _cand_idx(N, n_prev - 1)                            # never the zero row itself
    idx_d = cu(torch.tensor(idx, dtype=torch.int32))
    idx0_d = cu(torch.tensor([i if i >= 0 else n_prev - 1 for i in idx], dtype=torch.int32))

    def run(ix, row0, n):
        h, c = nanbuf(n, H), nanbuf(n, H)
        _lstm(lib, abi.ptr(pre_d, row0 * 4 * H * 4), 4 * H, abi.ptr(hp_d), H, abi.ptr(cp_d), H, abi.ptr(ix, row0 * 4), abi.ptr(zero_d), whh, wk, bhh_d,
              abi.ptr(c), H, abi.ptr(h), H, n, H)
        assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(c).all())
        return h, c

    h, c = run(idx_d, 0, N)
    h0, c0 = run(idx0_d, 0, N)
    assert idx.count(-1) >= 10 and torch.equal(h, h0) and torch.equal(c, c0)
    for r in (0, 2, 15, 16, 31, 32, 63, 64, 69):              # tile edges, rows with idx -1 (2, 32, 69), repeats (15, 63)
        h1, c1 = run(idx_d, r, 1)
        assert torch.equal(h1[0], h[r]) and torch.equal(c1[0], c[r]), r


# ================================================================================================ 4. deer_calib_delta
def _delta(lib, act, NP, thr_type, pad=3):
    """act (NL, rows, ld_act) on the host -> values (NL - 1, rows) from a launch with ld_val = rows + pad; the padding must stay NaN"""
    NL, rows, ld_act = act.shape
    a = cu(act)
    v = nanbuf(NL - 1, rows + pad)
    abi.check(lib.deer_calib_delta(abi.ptr(a), ld_act, NL, rows, NP, thr_type, abi.ptr(v), rows + pad, st()), "delta")
    sync()
    assert bool(torch.isnan(v[:, rows:]).all()), "stores past the end of a row of values"
    return v[:, :rows].cpu()


def _actions(NL, rows, NP, seed):
    """tanh outputs of a random head in the 6 A pose columns of rows of 8 A; the gripper columns are NaN (never read)"""
    act = torch.full((NL, rows, NP // 6 * 8), NAN)
    act[..., :NP] = torch.tanh(rnd(NL, rows, NP, seed=seed))
    return act


def _delta_gate(v, ref, NP, thr_type, what):
    if thr_type == 3:
        gate(v, ref, torch.ones_like(ref), (NP + 8) * 2.0 ** -23, what)          # absolute: terms <= 1, 1 - ab cancels
    else:
        assert bool((ref > 0).all())
        gate(v, ref, ref, (NP + 4) * 2.0 ** -23, what)                           # relative: a chain of <= NP + 4 roundings of non-negative terms


@pytest.mark.parametrize("thr_type", [0, 1, 2, 3])
@pytest.mark.parametrize("NP", [6, 12, 48])
@pytest.mark.parametrize("NL", [2, 7, MAX_NL])
@pytest.mark.parametrize("rows", [1, 255, 257, 2048])
def test_calib_delta(lib, rows, NL, NP, thr_type):
    """values[e][r] = get_delta(actions[e][r], actions[e + 1][r]) over the NP pose values of rows of 8 A (ld_act > NP, ld_val > rows)"""
    act = _actions(NL, rows, NP, seed=rows + NL + NP)
    a64 = act[..., :NP].double()
    if thr_type == 3:
        assert float(a64.norm(dim=-1).min()) >= 0.1
    v = _delta(lib, act, NP, thr_type)
    _delta_gate(v, orc.get_delta(a64[:-1], a64[1:], THR[thr_type]), NP, thr_type, THR[thr_type])


@pytest.mark.parametrize("NP", [6, 12, 48])
def test_calib_delta_exact_and_nan(lib, NP):
    """equal actions: exactly 0 (cosine: within its gate); cosine of two zero vectors: exactly 1; of a vector of norm < 1e-5 with itself:
    1 - (|a| / 1e-5)^2; a NaN pose value (first, middle, last) gives NaN for every type, a NaN gripper column (every row here) none"""
    NL, rows = 3, 9
    act = _actions(NL, rows, NP, seed=NP)
    act[1] = act[0]                                           # pair 0: identical; pair 1: ordinary
    tiny = rnd(NP, seed=1) * 1e-6 / NP ** 0.5
    assert 0 < float(tiny.double().norm()) < 1e-5
    act[:2, 7, :NP] = 0
    act[:2, 8, :NP] = tiny
    cos_tol = (NP + 8) * 2.0 ** -23
    for thr_type in range(4):
        v = _delta(lib, act, NP, thr_type)
        assert bool(torch.isfinite(v).all())
        if thr_type != 3:
            assert bool((v[0] == 0.0).all()) and bool((v[1] > 0).all())
        else:
            assert float(v[0, :7].abs().max()) <= cos_tol
            assert float(v[0, 7]) == 1.0
            assert abs(float(v[0, 8]) - (1.0 - float((tiny.double().norm() / 1e-5) ** 2))) <= cos_tol
    for pos in (0, NP // 2, NP - 1):
        bad = _actions(NL, rows, NP, seed=NP + 1)
        bad[1, 4, pos] = NAN                                  # layer 1 sits in both pairs of row 4
        for thr_type in range(4):
            v = _delta(lib, bad, NP, thr_type)
            assert torch.isnan(v).nonzero().tolist() == [[0, 4], [1, 4]], (THR[thr_type], pos)


# ================================================================================================ 5. the orchestration, bit for bit
def _head_weights(sd, cfg, wk):
    """the tensors of extra_exit as the engine holds them: matrices in weight kind wk, biases and LayerNorms f32 (csrc/model.hip add_head)"""
    p = "extra_exit."
    mat = lambda k: cu(sd[k].to(_WDT[wk]))                                       # noqa: E731
    vec = lambda k: cu(sd[k].float())                                            # noqa: E731
    w = {"lstm": [], "fc": [[], []], "out": []}
    for l in range(cfg.lstm_num_layers):
        r, sfx = (f"{p}rnn.layers.{3 * l}.", "_l0") if cfg.lstm_layernorm else (f"{p}rnn.", f"_l{l}")
        lw = dict(wih=mat(r + "weight_ih" + sfx), whh=mat(r + "weight_hh" + sfx), bih=vec(r + "bias_ih" + sfx), bhh=vec(r + "bias_hh" + sfx))
        if cfg.lstm_layernorm:
            lw.update(lnw=vec(f"{p}rnn.layers.{3 * l + 1}.weight"), lnb=vec(f"{p}rnn.layers.{3 * l + 1}.bias"))
        w["lstm"].append(lw)
    dims = cfg.mlp_hidden_dims
    for g, name in enumerate(("actions", "gripper")):
        for i, dim in enumerate(dims):
            fw = dict(w=mat(f"{p}{name}.mlp.{1 + 4 * i}.weight"), b=vec(f"{p}{name}.mlp.{1 + 4 * i}.bias"), dim=dim)
            if cfg.mlp_layernorm:
                fw.update(lnw=vec(f"{p}{name}.mlp.{2 + 4 * i}.weight"), lnb=vec(f"{p}{name}.mlp.{2 + 4 * i}.bias"))
            assert fw["w"].shape[0] == dim
            w["fc"][g].append(fw)
        w["out"].append(dict(w=mat(f"{p}{name}.mlp.{1 + 4 * len(dims)}.weight"), b=vec(f"{p}{name}.mlp.{1 + 4 * len(dims)}.bias")))
    w.update(wk=wk, H=cfg.head_hidden, A=max(1, cfg.multi_step_action), lstm_ln=cfg.lstm_layernorm, mlp_ln=cfg.mlp_layernorm,
             n_layers=cfg.n_layers, layers=[0] + list(cfg.exit_ids()))
    return w


def _host_chain(lib, weights, P, rl, W, thr_type):
    """The launches of deer_calibrate_values (csrc/model.hip) for ONE chunk holding all bs windows, from the entry points checked above +
    deer_head_seq_gemm / deer_head_seq_ln: gather; per LSTM layer [LayerNorm of the layer below,] W_ih for history and candidate rows at
    once, W - 1 history steps, one candidate step; [LayerNorm,] the two MLP heads; deltas.  P (bs, W, NL, d) f32 and rl (bs, W) int32 on the
    device -> (values (NL - 1, bs S), actions (NL, bs, S, 8 A))."""
    w = weights
    wk, H, A, layers = w["wk"], w["H"], w["A"], w["layers"]
    bs, _, NL, d = P.shape
    assert NL == len(layers)
    S, L = W - W // 2, W - 1
    rh, rc = bs * L, NL * bs * S
    rows = rh + rc
    F4 = 4                                                    # bytes per float
    slot_of = [-1] * w["n_layers"]
    for k, l in enumerate(layers):
        slot_of[l] = k
    X = nanbuf(rows * max(d, H))
    PRE, Y, CS = nanbuf(rows, 4 * H), nanbuf(rows, H), nanbuf(rh, H)
    HZ = torch.zeros(H, device="cuda")
    IDX = torch.full((rc,), -7777, dtype=torch.int32, device="cuda")
    ACT = nanbuf(rc, 8 * A)
    s = st()

    def gemm(x, ldx, m, out, ldo, M, N, K, epi):
        abi.check(lib.deer_head_seq_gemm(x, ldx, abi.ptr(m["w"]), wk, abi.ptr(m["b"]), out, ldo, M, N, K, epi, s), "seq_gemm")

    def ln(x, ldx, dst, ldd, lnw, lnb, M, n, relu):
        abi.check(lib.deer_head_seq_ln(x, ldx, dst, ldd, abi.ptr(lnw), abi.ptr(lnb), M, n, 1e-5, relu, s), "seq_ln")

    abi.check(lib.deer_calib_gather(abi.ptr(P), abi.ptr(rl), (ctypes.c_int * len(slot_of))(*slot_of), len(slot_of), abi.ptr(X), abi.ptr(IDX), bs, W, NL, d,
                                    s), "gather")
    for l, lw in enumerate(w["lstm"]):
        xin, in_dim = abi.ptr(X), d
        if l > 0:
            in_dim = H
            if w["lstm_ln"]:
                ln(abi.ptr(Y), H, abi.ptr(X), H, w["lstm"][l - 1]["lnw"], w["lstm"][l - 1]["lnb"], rows, H, 0)
            else:
                xin = abi.ptr(Y)
        gemm(xin, in_dim, dict(w=lw["wih"], b=lw["bih"]), abi.ptr(PRE), 4 * H, rows, 4 * H, in_dim, EPI_NONE)
        for t in range(L):
            abi.check(lib.deer_calib_lstm_step(abi.ptr(PRE, t * 4 * H * F4), L * 4 * H, abi.ptr(Y, (t - 1) * H * F4) if t > 0 else None, L * H,
                                               abi.ptr(CS, (t - 1) * H * F4) if t > 0 else None, L * H, None, None, abi.ptr(lw["whh"]), wk,
                                               abi.ptr(lw["bhh"]), abi.ptr(CS, t * H * F4), L * H, abi.ptr(Y, t * H * F4), L * H, bs, H, s), "history step")
        abi.check(lib.deer_calib_lstm_step(abi.ptr(PRE, rh * 4 * H * F4), 4 * H, abi.ptr(Y), H, abi.ptr(CS), H, abi.ptr(IDX), abi.ptr(HZ), abi.ptr(lw["whh"]),
                                           wk, abi.ptr(lw["bhh"]), None, 0, abi.ptr(Y, rh * H * F4), H, rc, H, s), "candidate step")
    xo = abi.ptr(Y, rh * H * F4)
    if w["lstm_ln"]:
        ln(xo, H, abi.ptr(X), H, w["lstm"][-1]["lnw"], w["lstm"][-1]["lnb"], rc, H, 0)
        xo = abi.ptr(X)
    zs = []                                                   # kept alive until the synchronize below
    for g in range(2):
        src, lds, kin = xo, H, H
        for fw in w["fc"][g]:
            z = nanbuf(rc, fw["dim"])
            zs.append(z)
            gemm(src, lds, fw, abi.ptr(z), fw["dim"], rc, fw["dim"], kin, EPI_NONE if w["mlp_ln"] else EPI_RELU)
            if w["mlp_ln"]:
                ln(abi.ptr(z), fw["dim"], abi.ptr(z), fw["dim"], fw["lnw"], fw["lnb"], rc, fw["dim"], 1)
            src, lds, kin = abi.ptr(z), fw["dim"], fw["dim"]
        if g == 0:
            gemm(src, lds, w["out"][0], abi.ptr(ACT), 8 * A, rc, 6 * A, kin, EPI_TANH)
        else:
            gemm(src, lds, w["out"][1], abi.ptr(ACT, 6 * A * F4), 8 * A, rc, A, kin, EPI_SIGMOID_LOGIT)
    values = nanbuf(NL - 1, bs * S)
    abi.check(lib.deer_calib_delta(abi.ptr(ACT), 8 * A, NL, bs * S, 6 * A, thr_type, abi.ptr(values), bs * S, s), "delta")
    sync()
    return values, ACT.view(NL, bs, S, 8 * A)


_PRECISION_WK = {"bf16": 0, "fp32": 1, "fp16": 2}


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_calibrate_values_equals_host_chain(lib, variant, precision):
    """eng.calibrate_values == _host_chain, torch.equal, values and actions: pins the row layout, the strides, the chunk offsets and the 2-D
    copy of `actions` in csrc/model.hip.  The engine runs chunks of 2048 // (W - 1) windows, the chain ONE chunk of all of them: equality
    there rests on the row independence calib.hip and head_seq.hip state (a row's result does not depend on the rows sharing its launch).
    W = 11, bs = 250 runs the engine in chunks of 204 + 46 windows."""
    cfg = _small_towers(deer_tiny(**VARIANTS[variant]))
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)    # 8-bit significands: exact in every weight kind
    eng = DeerEngine(cfg, sd, precision=precision)
    weights = _head_weights(sd, cfg, _PRECISION_WK[precision])
    exit_ids = cfg.exit_ids()
    NL = len(exit_ids) + 1
    cases = [(bs, W) for bs in (1, 3, 20) for W in (2, 3, 5, 8, 11, 12)] + [(250, 11)]
    assert 250 * 10 > 2048 and 250 % (2048 // 10) not in (0, 2048 // 10)
    for bs, W in cases:
        P = cu(rnd(bs, W, NL, cfg.d_model, seed=10 * bs + W))
        rl = _rand_layers(exit_ids, bs, W, bs + W)
        rl_d = cu(rl.to(torch.int32))
        for ti, ttype in enumerate(THR):
            v, a = eng.calibrate_values(P, rl, ttype, return_actions=True)
            v_ref, a_ref = _host_chain(lib, weights, P, rl_d, W, ti)
            sync()
            assert bool(torch.isfinite(v_ref).all()) and bool(torch.isfinite(a_ref).all())
            assert torch.equal(a, a_ref), (bs, W, ttype, float((a - a_ref).abs().max()))
            assert torch.equal(v, v_ref), (bs, W, ttype, float((v - v_ref).abs().max()))
