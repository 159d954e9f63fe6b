"""The action-head and exit-gate kernels (csrc/head.hip, csrc/head_seq.hip) one entry point at a time, through the C ABI, against the
committed oracle (oracle/deer_oracle.py: lstm_cell, head_mlp, get_delta, the controller rule) evaluated in float64 on the weights exactly as
the device holds them (bf16 / f32 / fp16 rows, w_kind 0 / 1 / 2).

Gates.  A dot-product result is gated relative to sum |w x| (+ |bias|) of its own row, not pointwise: its error is a rounding of that sum.
  STEP_TOL  the step head (head.hip): f32 activations x 16-bit or f32 weights, f32 accumulation.  The error is summation order only: a lane
            sums in_dim / 64 products (each rounded once, 2^-24) before a 6-level wave reduction, ~1e-6 of sum |w x| at in_dim 4096.
            Gate 4e-6.
  SEQ_TOL   the window-mode GEMM / recurrence (head_seq.hip): a 16-bit weight meets the f32 activation as two 16-bit planes hi + lo (the
            16-bit plane split), so the activation keeps ~16 (bf16: error 2^-17) or ~22 (fp16: 2^-22) significand bits; f32 weights run
            the exact-f32 MFMA (summation order only, ~1e-6).  Gates 4 x those (fp16: 8 x, the f32 accumulation over K = 1024 is of the
            same size as the plane split).
Max-pooling, copies, the control-block words and the LSTM-state commit are checked bit for bit.  The control-block protocol is checked against
a host model written from value_net.py:92-123,277-297 and the word layout of csrc/common.h (class Proto)."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from deer_vla_amd import _abi as abi  # noqa: E402
from oracle import deer_oracle as orc  # noqa: E402

STEP_TOL = 4e-6
SEQ_TOL = {0: 4 * 2.0 ** -17, 1: 4e-6, 2: 8 * 2.0 ** -22}
WKINDS = [0, 1, 2]
_WDT = {0: torch.bfloat16, 1: torch.float32, 2: torch.float16}
NAN = float("nan")
SHAPE = 1                                   # DEER_ERR_SHAPE


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
    """|out - ref| <= tol * scale elementwise (scale: sum |w x| + |b| of each output's row); every element written (no NaN)"""
    out = out.detach().double().cpu()
    assert torch.isfinite(out).all(), f"{what}: unwritten / non-finite outputs"
    r = float(((out - ref).abs() / scale).max())
    assert r <= tol, f"{what}: max |err| / sum|w x| = {r:.3g} > {tol:.3g}"
    return r


def sync():
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def lib():
    l = abi.lib()
    assert l.deer_hip_arch() == b"gfx950"
    return l


# ================================================================================================ 1. pooling
def _pool_ref(feats, avg, km=None):
    """fp64 max / mean over the valid tokens, and mean |x| of them (the scale of an f32 sum)"""
    f = feats.double()
    if km is None:
        km = torch.ones(f.shape[:2], dtype=torch.uint8)
    rows = [f[b][km[b].bool()] for b in range(f.shape[0])]
    ref = torch.stack([r.mean(0) if avg else r.amax(0) for r in rows])
    return ref, torch.stack([r.abs().mean(0) for r in rows])


def _check_pool(out, feats, avg, km=None, add=None):
    ref, mag = _pool_ref(feats, avg, km)
    if not avg:                                            # max: exact; + emb: one f32 add on both sides
        exp = ref.float() if add is None else ref.float() + add
        assert torch.equal(out.cpu(), exp)
        return
    T = feats.shape[1]
    scale = mag * (T + 1) * 2.0 ** -24 + ref.abs() * 2.0 ** -24 + 1e-30   # sequential f32 sum of <= T values, then / n
    if add is not None:
        ref = ref + add.double()
        scale = scale + ref.abs() * 2.0 ** -24
    gate(out, ref, scale, 1.0, "avg pool")


@pytest.mark.parametrize("d", [1000, 2048, 4096])
@pytest.mark.parametrize("T", [1, 5, 33])
@pytest.mark.parametrize("B", [1, 3, 8, 16])
def test_head_pool(lib, B, T, d):
    feats = rnd(B, T, d, seed=B * 100 + T)
    fd = cu(feats)
    for avg in (0, 1):
        out = nanbuf(B, d)
        abi.check(lib.deer_head_pool(abi.ptr(fd), abi.ptr(out), T, d, avg, B, None, None, 0, 0, st()), "pool")
        sync()
        _check_pool(out, feats, avg)


@pytest.mark.parametrize("T", [5, 33])
def test_head_pool_key_mask(lib, T):
    """right-padded instructions of an env batch: padded tokens are left out; a single valid token comes out exactly (max and avg)"""
    B, d = 4, 1000
    feats = rnd(B, T, d, seed=7)
    feats[:, -1] = 1e3                                      # a padded row that would win every max
    one = torch.zeros(B, T, dtype=torch.uint8)
    some = torch.zeros(B, T, dtype=torch.uint8)
    for b in range(B):
        one[b, (3 * b + 1) % (T - 1)] = 1
        some[b, :1 + (7 * b) % (T - 1)] = 1
    fd = cu(feats)
    for km, single in ((one, True), (some, False)):
        for avg in (0, 1):
            out = nanbuf(B, d)
            kmd = cu(km)
            abi.check(lib.deer_head_pool(abi.ptr(fd), abi.ptr(out), T, d, avg, B, abi.ptr(kmd), None, 0, 0, st()), "pool")
            sync()
            if single:
                assert torch.equal(out.cpu(), torch.stack([feats[b, int(km[b].nonzero()[0])] for b in range(B)]))
            else:
                _check_pool(out, feats, avg, km)


def test_head_pool_active_row_map(lib):
    """compaction: environment e's rows live at its slot of the row map; a dropped environment (slot -1) pools to zeros"""
    B, T, d = 5, 5, 1000
    slot_of = [2, -1, 0, 3, 1]                               # env 1 dropped, the others permuted over 4 slots
    feats = rnd(4, T, d, seed=3)
    cmap = torch.full((abi.CTL_WORDS,), -1, dtype=torch.int32)
    cmap[0] = 4
    for e, s in enumerate(slot_of):
        cmap[17 + e] = s
        if s >= 0:
            cmap[1 + s] = e
    fd, cmd = cu(feats), cu(cmap)
    for avg in (0, 1):
        out = nanbuf(B, d)
        abi.check(lib.deer_head_pool_active(abi.ptr(fd), abi.ptr(out), T, d, avg, B, None, None, 0, 0, abi.ptr(cmd), st()), "pool_active")
        sync()
        for e, s in enumerate(slot_of):
            if s < 0:
                assert torch.equal(out[e].cpu(), torch.zeros(d))
            else:
                _check_pool(out[e:e + 1], feats[s:s + 1], avg)


def test_head_pool_state_and_all_exited(lib):
    B, T, d = 3, 5, 1000
    feats, emb = rnd(B, T, d, seed=4), rnd(B, d, seed=5)
    fd, ed = cu(feats), cu(emb)
    for avg in (0, 1):
        out = nanbuf(B, d)
        abi.check(lib.deer_head_pool_state(abi.ptr(fd), abi.ptr(out), T, d, avg, B, None, abi.ptr(ed), None, 0, 0, st()), "pool_state")
        sync()
        _check_pool(out, feats, avg, add=emb)
    ctl = torch.zeros(B, abi.CTL_WORDS, dtype=torch.int32, device="cuda")
    ctl[0, abi.CTL_ALL_EXITED] = 1                           # every environment exited: the launches return at entry
    out = torch.full((B, d), 7.0, device="cuda")
    abi.check(lib.deer_head_pool(abi.ptr(fd), abi.ptr(out), T, d, 0, B, None, abi.ptr(ctl), 1, 3, st()), "pool")
    abi.check(lib.deer_head_pool_state(abi.ptr(fd), abi.ptr(out), T, d, 0, B, None, abi.ptr(ed), abi.ptr(ctl), 1, 3, st()), "pool_state")
    sync()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0


# ================================================================================================ 2. robot-state embedding
_GRIPS = [-1.0, 1.0, 0.0, 0.999, -0.999, 0.5]


def _state_inputs(B, d, seed):
    state = torch.zeros(B, 8)
    state[:, :6] = rnd(B, 6, seed=seed)
    for b in range(B):
        state[b, 6] = _GRIPS[b % len(_GRIPS)]
    return state, rnd(d, 6, seed=seed + 1, scale=0.5), rnd(d, seed=seed + 2, scale=0.1), rnd(2, d, seed=seed + 3)


def _state_u_ref(state, w_arm, b_arm, e_grip):
    """u = [relu(embed_arm_state) ; relu(embed_gripper_state)] of OracleHead.__call__'s use_state branch (oracle/deer_oracle.py:312-319,
    action_head.py:524-532) in fp64, and the scale of each element"""
    s = state.double()
    arm = torch.relu(orc._lin(s[:, :6], w_arm.double()) + b_arm.double())
    gidx = ((s[:, 6] + 1.0) / 2).long()                     # .long() truncates: 0.999 -> 0, 1 -> 1
    grp = torch.relu(e_grip.double()[gidx])
    mag = b_arm.double().abs() + s[:, :6].abs() @ w_arm.double().abs().t()
    return torch.cat((arm, grp), 1), torch.cat((mag, grp), 1)


@pytest.mark.parametrize("wk", WKINDS)
@pytest.mark.parametrize("d", [256, 1000])
def test_head_state_embed(lib, wk, d):
    B = len(_GRIPS)
    state, w_arm, b_arm, e_grip = _state_inputs(B, d, 11)
    ws, ws64 = wq(rnd(d, 2 * d, seed=15, scale=(2 * d) ** -0.5), wk)
    bs = rnd(d, seed=16, scale=0.1)
    out = nanbuf(B, d)
    dv = [cu(t) for t in (state, w_arm, b_arm, e_grip, bs)]                  # bound: a temporary's block is reused by the next allocation
    abi.check(lib.deer_head_state_embed(*[abi.ptr(t) for t in dv[:4]], abi.ptr(ws), abi.ptr(dv[4]), abi.ptr(out), d, B, wk, st()), "state_embed")
    sync()
    u, umag = _state_u_ref(state, w_arm, b_arm, e_grip)
    gate(out, orc._lin(u, ws64, bs.double()), umag @ ws64.abs().t() + bs.double().abs(), STEP_TOL, "state embed")


def test_head_seq_state_u(lib):
    M, d = len(_GRIPS), 1000
    state, w_arm, b_arm, e_grip = _state_inputs(M, d, 21)
    u = nanbuf(M, 2 * d)
    dv = [cu(t) for t in (state, w_arm, b_arm, e_grip)]
    abi.check(lib.deer_head_seq_state_u(*[abi.ptr(t) for t in dv], abi.ptr(u), M, d, st()), "state_u")
    sync()
    ref, mag = _state_u_ref(state, w_arm, b_arm, e_grip)
    assert torch.equal(u[:, d:].cpu(), ref[:, d:].float())                         # the gripper half: a row copy (+ relu)
    gate(u[:, :d], ref[:, :d], mag[:, :d] + 1e-30, 8 * 2.0 ** -24, "arm embedding")   # 7 f32 roundings of bias + a 6-term sum


# ================================================================================================ 3. LSTM layer (step head)
def _lstm_ref(x64, h, c, wih64, whh64, bih, bhh):
    """oracle lstm_cell in fp64, and per hidden unit the largest sum |w x| + |b| of its four gate rows"""
    h64, c64 = h.double(), c.double()
    h2, c2 = orc.lstm_cell(x64, h64, c64, wih64, whh64, bih.double(), bhh.double())
    mag = x64.abs() @ wih64.abs().t() + bih.double().abs() + h64.abs() @ whh64.abs().t() + bhh.double().abs()
    H = h.shape[1]
    return h2, c2, torch.stack([mag[:, q * H:(q + 1) * H] for q in range(4)]).amax(0)


@pytest.mark.parametrize("wk", WKINDS)
@pytest.mark.parametrize("B,in_dim,mode,T", [(1, 2048, abi.X_RAW, 1), (3, 1024, abi.X_LN, 1), (8, 2048, abi.X_POOL_MAX, 5),
                                             (5, 1000, abi.X_POOL_AVG, 33), (12, 2048, abi.X_RAW, 1), (16, 4096, abi.X_POOL_MAX, 3),
                                             (9, 1024, abi.X_LN, 1), (4, 4096, abi.X_RAW, 1)])
def test_head_lstm_layer(lib, wk, B, in_dim, mode, T):
    """one LSTM step for B environments (action_head.py:548-558) in every weight kind and input mode; B > 8 and batches whose B x (in_dim + H)
    f32 exceed the LDS go through the launcher's chunks; 4 x (4096 + 1024) f32 = 80 KB of LDS in one launch (also in fp16).  The recurrent
    half once per step (deer_head_lstm_hh) + the layer on W_ih only (deer_head_lstm_layer_pre) meet the same reference."""
    H = 1024
    x = rnd(B, T, in_dim, seed=1)
    h0, c0 = rnd(B, H, seed=2, scale=0.5), rnd(B, H, seed=3, scale=0.5)
    wih, wih64 = wq(rnd(4 * H, in_dim, seed=4, scale=in_dim ** -0.5), wk)
    whh, whh64 = wq(rnd(4 * H, H, seed=5, scale=H ** -0.5), wk)
    bih, bhh = rnd(4 * H, seed=6, scale=0.1), rnd(4 * H, seed=7, scale=0.1)
    lw, lb = 1.0 + rnd(in_dim, seed=8, scale=0.1), rnd(in_dim, seed=9, scale=0.1)
    ln = mode == abi.X_LN
    xd, bihd, bhhd, h0d, c0d, lwd, lbd = cu(x), cu(bih), cu(bhh), cu(h0), cu(c0), cu(lw), cu(lb)
    h1, c1 = nanbuf(B, H), nanbuf(B, H)
    abi.check(lib.deer_head_lstm_layer(abi.ptr(xd), T * in_dim, mode, T, in_dim, abi.ptr(lwd) if ln else None, abi.ptr(lbd) if ln else None,
                                       abi.ptr(wih), abi.ptr(whh), abi.ptr(bihd), abi.ptr(bhhd), abi.ptr(h0d), abi.ptr(c0d), abi.ptr(h1), abi.ptr(c1),
                                       H, B, 1e-5, None, 2, 0, wk, st()), "lstm")
    sync()
    x64 = x.double()
    x64 = x64.amax(1) if mode == abi.X_POOL_MAX else x64.mean(1)
    if ln:
        x64 = orc._ln(x64, lw.double(), lb.double())
    h_ref, c_ref, S = _lstm_ref(x64, h0, c0, wih64, whh64, bih, bhh)
    gate(c1, c_ref, S, 2 * STEP_TOL, "c")            # c' = s(f) c + s(i) tanh(g): |dc| <= |df| |c| / 4 + |di| / 4 + |dg|
    gate(h1, h_ref, S, 3 * STEP_TOL, "h")            # h' = s(o) tanh(c'): + |do| / 4
    if mode == abi.X_RAW and B <= 8:
        ghh = nanbuf(1, B, 4 * H)
        wp, bp = (ctypes.c_void_p * 1)(whh.data_ptr()), (ctypes.c_void_p * 1)(bhhd.data_ptr())
        abi.check(lib.deer_head_lstm_hh(wp, bp, 1, abi.ptr(h0d), abi.ptr(ghh), H, B, wk, st()), "lstm_hh")
        h2, c2 = nanbuf(B, H), nanbuf(B, H)
        abi.check(lib.deer_head_lstm_layer_pre(abi.ptr(xd), in_dim, mode, T, in_dim, None, None, abi.ptr(wih), abi.ptr(bihd), abi.ptr(ghh),
                                               abi.ptr(c0d), abi.ptr(h2), abi.ptr(c2), H, B, 1e-5, None, 2, 0, wk, st()), "lstm_pre")
        sync()
        gate(c2, c_ref, S, 2 * STEP_TOL, "c (recurrent half once per step)")
        gate(h2, h_ref, S, 3 * STEP_TOL, "h (recurrent half once per step)")


# ================================================================================================ 4. hidden Linear of both MLP heads
def _pro_ref(src, in_dim, pro, lns):
    """pro(src) of both groups in fp64: PRO_RAW x, PRO_LN LN(x) (shared), PRO_GROUP_LN_RELU relu(LN_g(x_g)), PRO_GROUP_RELU relu(x_g)"""
    s = src.double()
    if pro == abi.PRO_RAW:
        return [s[:, :in_dim]] * 2
    if pro == abi.PRO_LN:
        return [orc._ln(s[:, :in_dim], lns[0].double(), lns[1].double())] * 2
    xs = [s[:, g * in_dim:(g + 1) * in_dim] for g in range(2)]
    if pro == abi.PRO_GROUP_LN_RELU:
        xs = [orc._ln(xs[g], lns[2 * g].double(), lns[2 * g + 1].double()) for g in range(2)]
    return [torch.relu(x) for x in xs]


def _lns(in_dim, seed):
    return [1.0 + rnd(in_dim, seed=seed, scale=0.1), rnd(in_dim, seed=seed + 1, scale=0.1),
            1.0 + rnd(in_dim, seed=seed + 2, scale=0.1), rnd(in_dim, seed=seed + 3, scale=0.1)]


_FC_CASES = [(pro, in_dim) for pro in (abi.PRO_RAW, abi.PRO_LN, abi.PRO_GROUP_LN_RELU, abi.PRO_GROUP_RELU) for in_dim in (256, 1024, 2048)]
_FC_CASES.append((abi.PRO_RAW, 4096))                    # the LayerNorm prologues take <= 2048 values (test_head_fc_refusals)


@pytest.mark.parametrize("wk", WKINDS)
@pytest.mark.parametrize("B", [1, 8, 9, 16])
@pytest.mark.parametrize("pro,in_dim", _FC_CASES)
def test_head_fc(lib, wk, B, pro, in_dim):
    """dst[b][g out + n] = W_g[n] . pro(src_b)_g + b_g[n] for every prologue; batches above 8 run in chunks of 8; a chunk whose activations
    exceed 64 KB of LDS (8 x 2048 f32 and up) is refused with DEER_ERR_SHAPE and nothing is written"""
    out_dim = 37 if B in (1, 9) else 256                     # odd: the last wave has a single row
    grouped = pro in (abi.PRO_GROUP_LN_RELU, abi.PRO_GROUP_RELU)
    stride = 2 * in_dim if grouped else (in_dim if B in (1, 9) else in_dim + 8)
    src = rnd(B, stride, seed=in_dim + B)
    lns = _lns(in_dim, 30)
    W = [wq(rnd(out_dim, in_dim, seed=40 + g, scale=in_dim ** -0.5), wk) for g in range(2)]
    bias = [rnd(out_dim, seed=50 + g, scale=0.1) for g in range(2)]
    lnd, bd = [cu(t) for t in lns], [cu(t) for t in bias]
    dst = nanbuf(B, 2 * out_dim)
    srcd = cu(src)
    rc = lib.deer_head_fc(abi.ptr(srcd), stride, in_dim, pro, *[abi.ptr(t) for t in lnd], abi.ptr(W[0][0]), abi.ptr(bd[0]),
                          abi.ptr(W[1][0]), abi.ptr(bd[1]), out_dim, abi.ptr(dst), B, 1e-5, None, 2, 0, wk, st())
    sync()
    if (min(B, 8) * in_dim + 16) * 4 > 64 * 1024:
        assert rc == SHAPE and bool(torch.isnan(dst).all())
        return
    abi.check(rc, "fc")
    xs = _pro_ref(src, in_dim, pro, lns)
    for g in range(2):
        ref = orc._lin(xs[g], W[g][1], bias[g].double())
        scale = xs[g].abs() @ W[g][1].abs().t() + bias[g].double().abs()
        gate(dst[:, g * out_dim:(g + 1) * out_dim], ref, scale, STEP_TOL, f"fc group {g}")


def test_head_fc_refusals(lib):
    x = torch.zeros(8, 4096, device="cuda")
    w = torch.zeros(8, 4096, dtype=torch.bfloat16, device="cuda")
    p = torch.zeros(8192, device="cuda")
    dst = nanbuf(8, 16)
    for pro, B, in_dim in ((abi.PRO_LN, 1, 4096), (abi.PRO_GROUP_LN_RELU, 1, 2056), (abi.PRO_RAW, 8, 2048), (abi.PRO_RAW, 4, 4096)):
        assert lib.deer_head_fc(abi.ptr(x), in_dim, in_dim, pro, abi.ptr(p), abi.ptr(p), abi.ptr(p), abi.ptr(p), abi.ptr(w), abi.ptr(p), abi.ptr(w),
                                abi.ptr(p), 8, abi.ptr(dst), B, 1e-5, None, 2, 0, 0, st()) == SHAPE, (pro, B, in_dim)
    sync()
    assert bool(torch.isnan(dst).all())


# ================================================================================================ 5./6. output Linear + exit gate
class Final:
    """weights of the output Linears (Wa [6 A, in_dim], Wg [A, in_dim]) + the LayerNorms of the last hidden layer, one weight kind"""

    def __init__(self, in_dim=256, A=1, wk=2, seed=0):
        self.in_dim, self.A, self.wk = in_dim, A, wk
        self.Wa, self.Wa64 = wq(rnd(6 * A, in_dim, seed=seed + 1, scale=1.5 * in_dim ** -0.5), wk)
        self.Wg, self.Wg64 = wq(rnd(A, in_dim, seed=seed + 2, scale=1.5 * in_dim ** -0.5), wk)
        self.ba, self.bg = rnd(6 * A, seed=seed + 3, scale=0.1), rnd(A, seed=seed + 4, scale=0.1)
        self.lns = _lns(in_dim, seed + 10)
        self.dev = [cu(t) for t in (self.ba, self.bg, *self.lns)]

    def call(self, lib, src, B, pro=abi.PRO_GROUP_LN_RELU, ctl=None, kind=abi.KIND_CHECK, layer=0, slot=0, thr=None, force=0, thr_type=0, leq=1,
             state=None, L=1, H=8, env_exit=None, act_ext=None):
        """one launch: deer_head_final_env with a table, deer_head_final_multi for A > 1, else deer_head_final; returns action_dbg (CPU)"""
        ba, bg, lw0, lb0, lw1, lb1 = self.dev
        dbg = nanbuf(B, 64)
        h_tmp, c_tmp, h_st, c_st = state if state is not None else (None,) * 4
        head = (abi.ptr(src), src.shape[1], self.in_dim, pro, abi.ptr(lw0), abi.ptr(lb0), abi.ptr(lw1), abi.ptr(lb1), abi.ptr(self.Wa), abi.ptr(ba),
                abi.ptr(self.Wg), abi.ptr(bg), abi.ptr(ctl), kind, layer, slot)
        tail = (force, thr_type, leq, abi.ptr(h_tmp), abi.ptr(c_tmp), abi.ptr(h_st), abi.ptr(c_st), L, H, B, abi.ptr(dbg), 1e-5, self.wk)
        if env_exit is not None:
            rc = lib.deer_head_final_env(*head, abi.ptr(env_exit), *tail, self.A, abi.ptr(act_ext), st())
        elif self.A > 1:
            rc = lib.deer_head_final_multi(*head, abi.ptr(thr), *tail, self.A, abi.ptr(act_ext), st())
        else:
            rc = lib.deer_head_final(*head, abi.ptr(thr), *tail, st())
        abi.check(rc, "head_final")
        sync()
        return dbg.cpu()

    def reference(self, src, pro):
        """fp64 (pose 6 A | gripper A | logit A) through oracle head_mlp with no hidden layer, and the row scales sum |w x| + |b|"""
        xa, xg = _pro_ref(src, self.in_dim, pro, self.lns)
        cfg = types.SimpleNamespace(mlp_num_hidden_layers=0, mlp_layernorm=False)
        pose = orc.head_mlp({"a.mlp.1.weight": self.Wa64, "a.mlp.1.bias": self.ba.double()}, cfg, "a.", xa, "tanh")
        grip, logit = orc.head_mlp({"g.mlp.1.weight": self.Wg64, "g.mlp.1.bias": self.bg.double()}, cfg, "g.", xg, "sigmoid", with_logits=True)
        sa = xa.abs() @ self.Wa64.abs().t() + self.ba.double().abs()
        sg = xg.abs() @ self.Wg64.abs().t() + self.bg.double().abs()
        return torch.cat((pose, grip, logit), 1), torch.cat((sa, sg, sg), 1)


@pytest.mark.parametrize("wk", WKINDS)
@pytest.mark.parametrize("A", [1, 2, 3, 8])
@pytest.mark.parametrize("in_dim", [256, 2048, 2560])
def test_head_final_outputs(lib, wk, A, in_dim):
    """action_dbg (pose tanh | gripper sigmoid | logit) with ctl = NULL for every prologue; in_dim <= 2048 takes the one-wave LayerNorm, above
    it the block LayerNorm; A = multi_step_action output rows"""
    B = 3
    fin = Final(in_dim, A, wk, seed=A * 10 + wk)
    for pro in (abi.PRO_RAW, abi.PRO_LN, abi.PRO_GROUP_LN_RELU, abi.PRO_GROUP_RELU):
        src = rnd(B, 2 * in_dim, seed=pro)
        dbg = fin.call(lib, cu(src), B, pro=pro, kind=abi.KIND_COMMIT)
        ref, scale = fin.reference(src, pro)
        gate(dbg[:, :8 * A], ref, scale, STEP_TOL, f"action_dbg pro={pro}")
        assert bool(torch.isnan(dbg[:, 8 * A:]).all())


# ---- the control-block protocol ------------------------------------------------------------------------------------------------------------
_FLOAT_WORDS = np.zeros(abi.CTL_WORDS, bool)
_FLOAT_WORDS[abi.CTL_PREV_ACTION:abi.CTL_DELTAS + 16] = True
_FLOAT_WORDS[abi.CTL_ENS_ACTION:abi.CTL_ENS_ACTION + 8] = True
_THR_NAMES = {v: k for k, v in abi.THR_TYPES.items()}
f32 = np.float32


def _i32(v):
    """an unsigned 32-bit word as the int32 the control block stores"""
    v &= 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


class Proto:
    """Host model of the exit gate's control blocks (csrc/common.h CTL_*): ExitController.__call__ (value_net.py:277-297, the oracle's
    OracleExitController) and ActionValueNet's action_list / get_ensemble_action (value_net.py:92-123) per environment.  A = 1 keeps the
    previous and the ensemble action in the block; A > 1 keeps 7 A values of each in act_ext [B][4][64] (previous | committed | ensemble) and
    only the ensemble's count in the block."""

    def __init__(self, B, A):
        self.B, self.A = B, A
        self.ctl = np.zeros((B, abi.CTL_WORDS), np.int32)
        self.ext = np.zeros((B, 256), np.float32)

    def load(self, ctl, ext=None):
        self.ctl = ctl.cpu().numpy().copy()
        if ext is not None:
            self.ext = ext.cpu().numpy().reshape(self.B, 256).copy()

    def begin_step(self, info):
        for b in range(self.B):
            c = self.ctl[b]
            c[abi.CTL_EXIT_FLAG], c[abi.CTL_EXIT_LAYER], c[abi.CTL_N_EVALS], c[abi.CTL_COMMITTED], c[abi.CTL_PREV_REAL] = 0, -1, 0, 0, 0
            c[abi.CTL_ENS_ACTION + 7] = 0                     # reset_actions(): no ensemble action yet
            c[abi.CTL_HOLD] = (info[0] >> b) & 1 if info is not None else 0
            c[abi.CTL_DELTAS:abi.CTL_DELTAS + 16] = 0x7fc00000   # NaN: not evaluated
        c0 = self.ctl[0]
        c0[abi.CTL_SEQ], c0[abi.CTL_HOST_PTR], c0[abi.CTL_HOST_PTR + 1] = (info[1], info[2], info[3]) if info is not None else (0, 0, 0)
        c0[abi.CTL_ALL_EXITED] = c0[abi.CTL_N_EXITED] = c0[abi.CTL_EVALS_DONE] = 0

    def step(self, dbg, dev_ctl, kind, layer, slot, thr, force, thr_type, leq):
        """one launch.  dbg: its action_dbg; dev_ctl: the device blocks after it (the kernel's delta is taken from there once checked against
        fp64 get_delta).  thr / force: per environment.  Returns (evaluated, committed) per environment."""
        A, NP, NA = self.A, 6 * self.A, 7 * self.A
        ev, cm = [False] * self.B, [False] * self.B
        if self.ctl[0, abi.CTL_ALL_EXITED] != 0:
            return ev, cm
        shadow = self.ctl[0, abi.CTL_SHADOW] != 0
        for b in range(self.B):
            c, fl = self.ctl[b], self.ctl[b].view(np.float32)
            hold = c[abi.CTL_HOLD] != 0
            if c[abi.CTL_EXIT_FLAG] != 0 or (hold and (kind == abi.KIND_PSEUDO or (kind == abi.KIND_CHECK and layer < c[abi.CTL_CUR_EXIT_ID]))):
                continue
            ev[b] = True
            cur = dbg[b].numpy().astype(np.float32)
            prev = fl[abi.CTL_PREV_ACTION:abi.CTL_PREV_ACTION + 8].copy() if A == 1 else self.ext[b, :NA].copy()
            commit = False
            if kind == abi.KIND_PSEUDO:                      # not a member of action_list
                if A == 1:
                    fl[abi.CTL_PREV_ACTION:abi.CTL_PREV_ACTION + 8] = cur[:8]
                else:
                    self.ext[b, :NA] = cur[:NA]
                c[abi.CTL_PREV_REAL] = 0
            elif kind == abi.KIND_CHECK and not hold:
                delta = dev_ctl[b].view(np.float32)[abi.CTL_DELTAS + slot]
                ref = float(orc.get_delta(torch.from_numpy(cur[:NP]).double(), torch.from_numpy(prev[:NP]).double(), _THR_NAMES[thr_type]))
                if math.isnan(ref):
                    assert math.isnan(delta), (b, _THR_NAMES[thr_type], float(delta))
                else:                                        # 6 A-term f32 sums: a few ulp of the result (cosine: of 1 - a.b)
                    tol = 1e-6 if thr_type == abi.THR_TYPES["cosine"] else 1e-6 * abs(ref)
                    assert abs(float(delta) - ref) <= tol, (b, _THR_NAMES[thr_type], float(delta), ref)
                fl[abi.CTL_DELTAS + slot] = delta
                two = c[abi.CTL_PREV_REAL] != 0              # get_ensemble_action(): mean of action_list[-2:]
                ens = (f32(0.5) * (prev[:NA] + cur[:NA])).astype(np.float32) if two else cur[:NA]
                if A == 1:
                    fl[abi.CTL_ENS_ACTION:abi.CTL_ENS_ACTION + 7] = ens
                    fl[abi.CTL_PREV_ACTION:abi.CTL_PREV_ACTION + 8] = cur[:8]
                else:
                    self.ext[b, 128:128 + NA] = ens
                    self.ext[b, :NA] = cur[:NA]
                fl[abi.CTL_ENS_ACTION + 7] = 2.0 if two else 1.0
                c[abi.CTL_PREV_REAL] = 1
                # `i >= max_layer or bool(value <= thr) is leq` (a NaN delta compares False); forced at the deepest layer / the layer cap
                if (bool(f32(delta) <= f32(thr[b])) == bool(leq)) or force[b]:
                    c[abi.CTL_CUR_EXIT_ID] = layer
                    commit = True
            else:                                            # COMMIT, or a CHECK at / above cur_exit_id while holding the stage
                commit = True
            c[abi.CTL_N_EVALS] += 1
            if commit and shadow:
                if c[abi.CTL_COMMITTED] != 0:
                    commit = False
                else:
                    c[abi.CTL_COMMITTED] = 1
            if commit:
                fl[abi.CTL_OUT_ACTION:abi.CTL_OUT_ACTION + 6] = cur[:6]
                fl[abi.CTL_OUT_ACTION + 6] = cur[NP]
                fl[abi.CTL_OUT_ACTION + 7] = cur[NA]
                if A > 1:
                    self.ext[b, 64:64 + 8 * A] = cur[:8 * A]
                c[abi.CTL_EXIT_LAYER] = layer
                if not shadow:
                    c[abi.CTL_EXIT_FLAG] = 1
                    if self.B == 1:
                        self.ctl[0, abi.CTL_ALL_EXITED] = 1
                    else:
                        self.ctl[0, abi.CTL_N_EXITED] += 1
                        if self.ctl[0, abi.CTL_N_EXITED] == self.B:
                            self.ctl[0, abi.CTL_ALL_EXITED] = 1
            cm[b] = commit
        return ev, cm

    def compare(self, ctl, ext=None, what=""):
        got = ctl.cpu().numpy()
        for b in range(self.B):
            gi, mi = got[b], self.ctl[b]
            assert np.array_equal(gi[~_FLOAT_WORDS], mi[~_FLOAT_WORDS]), (what, b, np.nonzero(gi != mi)[0])
            gf, mf = gi.view(np.float32)[_FLOAT_WORDS], mi.view(np.float32)[_FLOAT_WORDS]
            assert np.array_equal(gf, mf, equal_nan=True), (what, b, gf, mf)
        if ext is not None:
            assert np.array_equal(ext.cpu().numpy().reshape(self.B, 256)[:, :192], self.ext[:, :192], equal_nan=True), what


class Rig:
    """one env batch on the device (control blocks, act_ext, LSTM state [L][B][H]) + its Proto model; every launch is followed by a full
    comparison of the blocks and the act_ext fields, of action_dbg of the environments that were skipped, and of the committed LSTM state"""

    def __init__(self, lib, B, A, H=8, L=2, in_dim=256, wk=2, seed=0):
        self.lib, self.B, self.A, self.H, self.L = lib, B, A, H, L
        self.fin = Final(in_dim, A, wk, seed=seed)
        self.ctl = torch.full((B, abi.CTL_WORDS), 12345, dtype=torch.int32, device="cuda")   # every word begin_step resets starts as garbage
        self.ctl[:, abi.CTL_SHADOW] = 0
        self.ext = torch.zeros(B, 4, 64, device="cuda") if A > 1 else None
        self.h_st, self.c_st = cu(rnd(L, B, H, seed=seed + 90)), cu(rnd(L, B, H, seed=seed + 91))
        self.model = Proto(B, A)
        self.model.load(self.ctl, self.ext)
        self.n = 0

    def begin(self, info=None):
        info_d = cu(torch.tensor(info, dtype=torch.int32)) if info is not None else None
        abi.check(self.lib.deer_ctl_begin_step(abi.ptr(self.ctl), abi.ptr(info_d), self.B, st()), "begin_step")
        sync()
        self.model.begin_step(info)
        self.model.compare(self.ctl, self.ext, "begin_step")

    def poke(self, words):
        """set control-block words on the device and in the model: {(env, word): int32 value}"""
        blk = self.ctl.cpu()
        for (b, w), v in words.items():
            blk[b, w] = v
        self.ctl.copy_(blk)
        self.model.load(self.ctl, self.ext)

    def snapshot(self):
        return (self.ctl.clone(), None if self.ext is None else self.ext.clone(), self.h_st.clone(), self.c_st.clone(),
                self.model.ctl.copy(), self.model.ext.copy())

    def restore(self, s):
        self.ctl.copy_(s[0])
        if self.ext is not None:
            self.ext.copy_(s[1])
        self.h_st.copy_(s[2])
        self.c_st.copy_(s[3])
        self.model.ctl, self.model.ext = s[4].copy(), s[5].copy()

    def src(self, seed):
        return cu(rnd(self.B, 2 * self.fin.in_dim, seed=seed))

    def run(self, kind, layer, slot=0, thr=None, force=0, thr_type=0, leq=1, env_rows=None, caps=None, rows_on_device=False, src=None):
        """one head_final launch; thr: the shared threshold row's value, or env_rows / caps: per-environment operating points written by
        deer_env_exit_write and read by deer_head_final_env"""
        B = self.B
        self.n += 1
        src = self.src(1000 + self.n) if src is None else src
        h_tmp, c_tmp = cu(rnd(self.L, B, self.H, seed=2000 + self.n)), cu(rnd(self.L, B, self.H, seed=3000 + self.n))
        h0, c0 = self.h_st.clone(), self.c_st.clone()
        env_exit = thr_d = None
        if env_rows is not None:
            env_exit = torch.full((abi.ENV_EXIT_WORDS,), NAN, device="cuda")
            rows = torch.tensor(env_rows, dtype=torch.float32).reshape(-1).contiguous()
            rows_d = cu(rows)
            capv = (ctypes.c_int * B)(*caps)
            rows_arg = abi.ptr(rows_d) if rows_on_device else ctypes.c_void_p(rows.data_ptr())
            abi.check(self.lib.deer_env_exit_write(abi.ptr(env_exit), rows_arg, 1 if rows_on_device else 0, capv, B, st()), "env_exit_write")
            thr_b = [env_rows[b][slot] for b in range(B)]
            force_b = [bool(force) or layer >= caps[b] for b in range(B)]
        else:
            thr_d = cu(torch.full((16,), thr, dtype=torch.float32)) if thr is not None else None
            thr_b = [thr if thr is not None else 0.0] * B
            force_b = [bool(force)] * B
        dbg = self.fin.call(self.lib, src, B, ctl=self.ctl, kind=kind, layer=layer, slot=slot, thr=thr_d, force=force, thr_type=thr_type, leq=leq,
                            state=(h_tmp, c_tmp, self.h_st, self.c_st), L=self.L, H=self.H, env_exit=env_exit, act_ext=self.ext)
        ev, cm = self.model.step(dbg, self.ctl.cpu().numpy(), kind, layer, slot, thr_b, force_b, thr_type, leq)
        self.model.compare(self.ctl, self.ext, f"launch {self.n}: kind {kind} layer {layer}")
        for b in range(B):
            if not ev[b]:
                assert bool(torch.isnan(dbg[b]).all()), f"env {b} was skipped but its action_dbg was written"
            hs, cs = (h_tmp, c_tmp) if cm[b] else (h0, c0)
            assert torch.equal(self.h_st[:, b], hs[:, b]) and torch.equal(self.c_st[:, b], cs[:, b]), f"LSTM state of env {b} (commit={cm[b]})"
        return dbg, ev, cm

    def delta(self, b, slot):
        return self.ctl[b].cpu().numpy().view(np.float32)[abi.CTL_DELTAS + slot]

    def word(self, b, w):
        return int(self.ctl[b, w].item())


@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("thr_type", [0, 1, 2, 3])
@pytest.mark.parametrize("leq", [1, 0])
def test_exit_decision_at_the_threshold(lib, A, thr_type, leq):
    """every criterion x leq: the kernel's own delta (CTL_DELTAS, checked against fp64 get_delta on action_dbg) replayed with the threshold at
    that delta and one ulp above / below it; the decision must be exactly (delta <= thr) == leq"""
    rig = Rig(lib, 2, A, seed=thr_type)
    rig.begin()
    rig.run(abi.KIND_PSEUDO, 0)
    snap = rig.snapshot()
    src = rig.src(77)
    rig.run(abi.KIND_CHECK, 3, slot=2, thr=-1e30 if leq else 1e30, thr_type=thr_type, leq=leq, src=src)   # fires for nobody
    assert rig.ctl[:, abi.CTL_EXIT_FLAG].tolist() == [0, 0]
    for b in range(2):
        d = rig.delta(b, 2)
        assert np.isfinite(d) and d > 0
        for thr in (d, np.nextafter(d, f32(np.inf)), np.nextafter(d, f32(-np.inf))):
            rig.restore(snap)
            rig.run(abi.KIND_CHECK, 3, slot=2, thr=float(thr), thr_type=thr_type, leq=leq, src=src)
            assert rig.delta(b, 2).tobytes() == d.tobytes()                       # same inputs, same bits
            assert (rig.word(b, abi.CTL_EXIT_FLAG) == 1) == ((d <= thr) == bool(leq)), (b, d, thr)


@pytest.mark.parametrize("A", [1, 2])
def test_exit_decision_rare_inputs(lib, A):
    """a NaN delta (exits only when leq is False, like `bool(nan <= thr) is leq`), the cosine against an all-zero and against a tiny (norm below
    the 1e-5 clamp) previous action, identical actions (delta 0), `force`"""
    rig = Rig(lib, 2, A, seed=5)
    NA = 7 * A
    for thr_type in (0, 1, 2, 3):
        for prev in ("nan", "zero", "tiny"):
            if prev != "nan" and thr_type != abi.THR_TYPES["cosine"]:
                continue
            for leq in (1, 0):
                rig.begin()
                rig.run(abi.KIND_PSEUDO, 0)
                vals = {"nan": torch.full((NA,), NAN), "zero": torch.zeros(NA), "tiny": rnd(NA, seed=3) * 1e-7}[prev]
                if A > 1:
                    rig.ext[:, 0, :NA] = vals.cuda()
                words = {(b, abi.CTL_PREV_REAL): 1 for b in range(2)}          # an exit-check action of this step: the ensemble averages it
                if A == 1:
                    words.update({(b, abi.CTL_PREV_ACTION + i): int(vals[i:i + 1].view(torch.int32)) for b in range(2) for i in range(7)})
                rig.poke(words)
                rig.run(abi.KIND_CHECK, 2, slot=0, thr=0.5, thr_type=thr_type, leq=leq)
                if prev == "nan":
                    assert np.isnan(rig.delta(0, 0)) and rig.word(0, abi.CTL_EXIT_FLAG) == (0 if leq else 1)
                elif prev == "zero":
                    assert rig.delta(0, 0) == 1.0
    # identical actions: the same features twice -> delta exactly 0 (cosine: 1 - a.b of two equal unit vectors, a few ulp)
    for thr_type in (0, 1, 2, 3):
        rig.begin()
        src = rig.src(8)
        rig.run(abi.KIND_PSEUDO, 0, src=src)
        rig.run(abi.KIND_CHECK, 1, slot=0, thr=1e-6 if thr_type == abi.THR_TYPES["cosine"] else 0.0, thr_type=thr_type, leq=1, src=src)
        assert rig.ctl[:, abi.CTL_EXIT_FLAG].tolist() == [1, 1]
        if thr_type != abi.THR_TYPES["cosine"]:
            assert rig.delta(0, 0) == 0.0 and rig.delta(1, 0) == 0.0
    # force: a threshold that never fires
    rig.begin()
    rig.run(abi.KIND_PSEUDO, 0)
    rig.run(abi.KIND_CHECK, 5, slot=1, thr=-1.0, force=1, leq=1)
    assert rig.ctl[:, abi.CTL_EXIT_FLAG].tolist() == [1, 1]


@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("B", [1, 5])
def test_exit_protocol_full_step(lib, A, B):
    """begin_step -> PSEUDO -> CHECK(slot 0) -> CHECK(slot 1) -> COMMIT with some environments exiting at each check, for two steps in a
    row, with the pinned host mirror of the verdicts; H = 1024 (the float4 path of the LSTM-state commit)"""
    rig = Rig(lib, B, A, H=1024, L=2, seed=B + A)
    mirror = torch.zeros((1 + 16) * abi.CTL_WORDS + 16 * 128, dtype=torch.int32).pin_memory()
    mp = mirror.data_ptr()
    for seq in (1, 2):
        rig.begin([0, seq, _i32(mp), _i32(mp >> 32)])
        rig.run(abi.KIND_PSEUDO, 0)
        for slot, layer in ((0, 3), (1, 7)):
            snap, src = rig.snapshot(), rig.src(100 * seq + slot)
            rig.run(abi.KIND_CHECK, layer, slot=slot, thr=-1e30, leq=1, src=src)          # dry run: read the deltas
            ds = sorted(float(rig.delta(b, slot)) for b in range(B) if snap[0][b, abi.CTL_EXIT_FLAG].item() == 0)
            rig.restore(snap)
            if B == 1:
                thr = ds[0] * (0.5 if slot == 0 else 1.0)                              # the one environment exits at the second check
            else:
                thr = 0.5 * (ds[len(ds) // 2 - 1] + ds[len(ds) // 2])                 # 2 of 5, then 1 of 3 exit
            rig.run(abi.KIND_CHECK, layer, slot=slot, thr=thr, leq=1, src=src)
            assert mirror[0].item() == seq * 64 + slot + 1                              # progress: check `slot` of step `seq` complete
        rig.run(abi.KIND_COMMIT, 11)
        c = rig.ctl.cpu()
        assert c[0, abi.CTL_ALL_EXITED].item() == 1 and (c[:, abi.CTL_EXIT_FLAG] == 1).all()
        assert c[0, abi.CTL_N_EXITED].item() == (B if B > 1 else 0)
        layers = c[:, abi.CTL_EXIT_LAYER].tolist()
        assert sorted(layers) == ([7] if B == 1 else [3, 3, 7, 11, 11]), layers
        # a later check of the step returns at entry: nothing changes, nothing is written, the host learns that the step is over
        _, ev, _ = rig.run(abi.KIND_CHECK, 13, slot=2, thr=1e30, leq=1)
        assert not any(ev)
        assert mirror[1].item() == seq                                                 # done
        m = mirror[abi.CTL_WORDS:(1 + B) * abi.CTL_WORDS].view(B, abi.CTL_WORDS)
        keep = list(range(0, 7)) + list(range(8, 40)) + list(range(45, 56))         # the per-environment words
        hx = mirror[(1 + B) * abi.CTL_WORDS:(1 + B) * abi.CTL_WORDS + B * 128].view(torch.float32).view(B, 128)
        for b in range(B):
            if layers[b] != 11:                                                        # exited at a check: the mirror holds its block
                assert torch.equal(m[b, keep], c[b, keep]), b
                if A > 1:                                                              # ... and its committed | ensemble action
                    assert torch.equal(hx[b, :64], rig.ext[b, 1].cpu()) and torch.equal(hx[b, 64:], rig.ext[b, 2].cpu())


@pytest.mark.parametrize("A", [1, 2])
def test_exit_protocol_hold_and_shadow(lib, A):
    """stage hold (step_info bit b): a check below CUR_EXIT_ID changes nothing for that environment, one at / above it commits without a
    delta; shadow (calibration): every exit evaluated, only the first that fires commits, EXIT_FLAG stays 0.  H = 6: the scalar path of the
    LSTM-state commit"""
    B = 4
    rig = Rig(lib, B, A, H=6, L=3, seed=9)
    rig.begin()
    rig.poke({(b, abi.CTL_CUR_EXIT_ID): v for b, v in enumerate([7, 3, 7, 7])})
    rig.begin([0b0101, 3, 0, 0])                              # envs 0 and 2 hold their stage at cur_exit_id 7
    rig.run(abi.KIND_PSEUDO, 0)
    rig.run(abi.KIND_CHECK, 3, slot=0, thr=-1.0, leq=1)       # nobody exits by the criterion; 0 and 2 are below their exit
    rig.run(abi.KIND_CHECK, 7, slot=1, thr=-1.0, leq=1)       # 0 and 2 commit without a delta
    c = rig.ctl.cpu()
    assert c[[0, 2], abi.CTL_EXIT_FLAG].tolist() == [1, 1] and c[[0, 2], abi.CTL_EXIT_LAYER].tolist() == [7, 7]
    assert c[[1, 3], abi.CTL_EXIT_FLAG].tolist() == [0, 0]
    assert torch.isnan(c[[0, 2], abi.CTL_DELTAS:abi.CTL_DELTAS + 16].view(torch.float32)).all()
    rig.run(abi.KIND_COMMIT, 11)
    rig.begin([0b1111, 4, 0, 0])                              # everybody holds, the check is below every exit: the launch is skipped
    rig.run(abi.KIND_PSEUDO, 0)
    _, ev, _ = rig.run(abi.KIND_CHECK, 1, slot=0, thr=1e30, leq=1)
    assert not any(ev)
    rig.begin()
    rig.poke({(0, abi.CTL_SHADOW): 1})
    rig.run(abi.KIND_PSEUDO, 0)
    rig.run(abi.KIND_CHECK, 3, slot=0, thr=1e30, leq=1)       # fires for everybody: the first commit
    rig.run(abi.KIND_CHECK, 7, slot=1, thr=1e30, leq=1)       # fires again: evaluated, not committed
    rig.run(abi.KIND_COMMIT, 11)
    c = rig.ctl.cpu()
    assert (c[:, abi.CTL_EXIT_FLAG] == 0).all() and (c[:, abi.CTL_EXIT_LAYER] == 3).all() and (c[:, abi.CTL_N_EVALS] == 4).all()
    assert c[0, abi.CTL_ALL_EXITED].item() == 0


@pytest.mark.parametrize("A", [1, 2])
@pytest.mark.parametrize("rows_on_device", [0, 1])
def test_exit_protocol_per_environment_operating_points(lib, A, rows_on_device):
    """deer_env_exit_write + deer_head_final_env: each environment compares with its own threshold row and is forced at layer >= its cap
    (at the cap itself, not only above it)"""
    B = 4
    rig = Rig(lib, B, A, H=1024, L=1, seed=13)
    rig.begin()
    rig.run(abi.KIND_PSEUDO, 0)
    rows = [[1e30] * 16, [-1e30] * 16, [-1e30] * 16, [-1e30] * 16]   # env 0 always fires
    rows[3][1] = 1e30                                                # env 3 fires at slot 1 only
    caps = [99, 5, 99, 99]                                           # env 1 is forced from layer 5 on
    for slot, layer in ((0, 3), (1, 5), (2, 7)):
        rig.run(abi.KIND_CHECK, layer, slot=slot, env_rows=rows, caps=caps, rows_on_device=rows_on_device, leq=1)
    assert rig.ctl[:, abi.CTL_EXIT_LAYER].tolist() == [3, 5, -1, 5]
    rig.run(abi.KIND_COMMIT, 9)
    assert rig.ctl[:, abi.CTL_EXIT_LAYER].tolist() == [3, 5, 9, 5]


# ================================================================================================ 7. head_seq kernels
def _seq_gemm(lib, X, ldx, W, wk, bias, M, N, K, epi, row0=0):
    ldo = 2 * N + 3
    out = nanbuf(M, ldo)
    abi.check(lib.deer_head_seq_gemm(abi.ptr(X, row0 * ldx * 4), ldx, abi.ptr(W), wk, abi.ptr(bias), abi.ptr(out), ldo, M, N, K, epi, st()), "seq_gemm")
    sync()
    return out.cpu()


@pytest.mark.parametrize("wk", WKINDS)
@pytest.mark.parametrize("K", [8, 40, 1024])
@pytest.mark.parametrize("N", [7, 64, 100])
@pytest.mark.parametrize("M", [1, 63, 65, 200])
def test_head_seq_gemm(lib, wk, M, N, K):
    """out[m][n] = epi(X[m] . W[n] + b[n]) at ragged M / N edges and K % 32 != 0, all four epilogues (SIGMOID_LOGIT also stores the logit
    at column N + n); nothing is stored past the edges"""
    ldx = K + 8
    Xc = rnd(M, ldx, seed=M + K)
    W, W64 = wq(rnd(N, K, seed=N, scale=K ** -0.5), wk)
    bias = rnd(N, seed=5, scale=0.1)
    X, bd = cu(Xc), cu(bias)
    x64 = Xc[:, :K].double()
    ref = orc._lin(x64, W64, bias.double())
    scale = x64.abs() @ W64.abs().t() + bias.double().abs()
    tol = SEQ_TOL[wk]
    for epi, fn in ((0, None), (1, torch.relu), (2, torch.tanh), (3, torch.sigmoid)):
        out = _seq_gemm(lib, X, ldx, W, wk, bd, M, N, K, epi)
        gate(out[:, :N], fn(ref) if fn is not None else ref, scale, tol, f"seq_gemm epi {epi}")      # relu / tanh / sigmoid: slope <= 1
        if epi == 3:
            gate(out[:, N:2 * N], ref, scale, tol, "seq_gemm logit")
        assert bool(torch.isnan(out[:, 2 * N if epi == 3 else N:]).all()), f"epi {epi}: stores past the edge"


@pytest.mark.parametrize("wk", WKINDS)
def test_head_seq_gemm_fp16_outliers_and_row_independence(lib, wk):
    """activations beyond the fp16 range in some rows and some k-steps only (the wave-uniform outlier path), values exactly at 65504 and
    just above it; every row of a 200-row call equals the same row computed alone, bit for bit"""
    M, N, K = 200, 100, 1024
    Xc = rnd(M, K, seed=31)
    Xc[5, 100] = 1e6                        # one outlier in one k-step of one row
    Xc[70, 10:18] = -3e5                    # a whole lane slice
    Xc[71, 500] = 65504.0                   # the largest fp16: the ordinary path
    Xc[72, 501] = 65505.0                   # just above it
    Xc[72, 700] = -65519.0                  # rounds to -65504 in fp16, but lies beyond it
    Xc[199, 1023] = 2e9
    X = cu(Xc)
    W, W64 = wq(rnd(N, K, seed=32, scale=K ** -0.5), wk)
    bias = rnd(N, seed=33, scale=0.1)
    bd = cu(bias)
    out = _seq_gemm(lib, X, K, W, wk, bd, M, N, K, 0)
    x64 = Xc.double()
    gate(out[:, :N], orc._lin(x64, W64, bias.double()), x64.abs() @ W64.abs().t() + bias.double().abs(), SEQ_TOL[wk], "seq_gemm outliers")
    for r in (0, 5, 63, 64, 70, 71, 72, 199):
        assert torch.equal(_seq_gemm(lib, X, K, W, wk, bd, 1, N, K, 0, row0=r)[0, :N], out[r, :N]), r


@pytest.mark.parametrize("wk", WKINDS)
@pytest.mark.parametrize("H", [16, 48, 1024])
@pytest.mark.parametrize("N", [1, 31, 33])
def test_head_seq_lstm_step(lib, wk, N, H):
    """one recurrence step over N rows: gates = pre + h_prev W_hh^T + b_hh (h_prev NULL = zero state), c in place, h at row stride ld_out,
    (h_n, c_n) when given; H = 16 / 48 leave k-slices of a wave past H"""
    ld_pre, ld_h, ld_out = 4 * H + 8, H + 8, H + 4
    pre = rnd(N, ld_pre, seed=1)
    hp = rnd(N, ld_h, seed=2, scale=0.5)
    c0 = rnd(N, H, seed=3, scale=0.5)
    whh, whh64 = wq(rnd(4 * H, H, seed=4, scale=H ** -0.5), wk)
    bhh = rnd(4 * H, seed=5, scale=0.1)
    pre_d, hp_d, bhh_d = cu(pre), cu(hp), cu(bhh)
    for use_h, store_n in ((True, True), (False, False), (True, False)):
        c = cu(c0)
        h_out = nanbuf(N, ld_out)
        hn, cn = (nanbuf(N, H), nanbuf(N, H)) if store_n else (None, None)
        abi.check(lib.deer_head_seq_lstm_step(abi.ptr(pre_d), ld_pre, abi.ptr(hp_d) if use_h else None, ld_h, abi.ptr(whh), wk, abi.ptr(bhh_d),
                                              abi.ptr(c), abi.ptr(h_out), ld_out, abi.ptr(hn), abi.ptr(cn), N, H, st()), "seq_lstm_step")
        sync()
        p64, b64 = pre[:, :4 * H].double(), bhh.double()
        h64 = hp[:, :H].double() if use_h else torch.zeros(N, H, dtype=torch.float64)
        # the oracle cell with the identity as W_ih: its input half is `pre` itself
        h_ref, c_ref = orc.lstm_cell(p64, h64, c0.double(), torch.eye(4 * H, dtype=torch.float64), whh64, None, b64)
        mag = p64.abs() + h64.abs() @ whh64.abs().t() + b64.abs()
        S = torch.stack([mag[:, q * H:(q + 1) * H] for q in range(4)]).amax(0)
        tol = SEQ_TOL[wk] + 2.0 ** -22                       # + the f32 transcendentals of the cell (a few ulp of values <= 1)
        gate(c, c_ref, S, 2 * tol, "seq c")
        gate(h_out[:, :H], h_ref, S, 3 * tol, "seq h")
        assert bool(torch.isnan(h_out[:, H:]).all())
        if store_n:
            assert torch.equal(hn, h_out[:, :H]) and torch.equal(cn, c)


@pytest.mark.parametrize("n", [100, 1000, 1024])
def test_head_seq_ln(lib, n):
    """LayerNorm (+ ReLU) of rows of n values (n % 64 != 0 too), out of place with row strides and in place"""
    M = 7
    x = rnd(M, n + 4, seed=n) * 3 + 1
    w, b = 1.0 + rnd(n, seed=1, scale=0.1), rnd(n, seed=2, scale=0.1)
    wd, bd = cu(w), cu(b)
    ref = orc._ln(x[:, :n].double(), w.double(), b.double())
    scale = (orc._ln(x[:, :n].double(), None, None) * w.double()).abs() + b.double().abs() + 1e-30
    for relu in (0, 1):
        dst, xd = nanbuf(M, n + 8), cu(x)
        abi.check(lib.deer_head_seq_ln(abi.ptr(xd), n + 4, abi.ptr(dst), n + 8, abi.ptr(wd), abi.ptr(bd), M, n, 1e-5, relu, st()), "seq_ln")
        inp = cu(x)
        abi.check(lib.deer_head_seq_ln(abi.ptr(inp), n + 4, abi.ptr(inp), n + 4, abi.ptr(wd), abi.ptr(bd), M, n, 1e-5, relu, st()), "seq_ln in place")
        sync()
        gate(dst[:, :n], torch.relu(ref) if relu else ref, scale, 4e-6, "seq_ln")   # f32 statistics over <= 1024 values, rsqrtf: a few ulp per output
        assert bool(torch.isnan(dst[:, n:]).all())
        assert torch.equal(inp[:, :n], dst[:, :n]) and torch.equal(inp[:, n:].cpu(), x[:, n:])


def test_head_seq_pool(lib):
    M, d = 6, 1000
    emb = rnd(M, d, seed=9)
    for T in (1, 5):
        feats = rnd(M, T, d, seed=T)
        for avg in (0, 1):
            for e in (None, emb):
                X, fd, ed = nanbuf(M, d), cu(feats), cu(e) if e is not None else None
                abi.check(lib.deer_head_seq_pool(abi.ptr(fd), abi.ptr(ed), abi.ptr(X), M, T, d, avg, st()), "seq_pool")
                sync()
                if T == 1:                                   # one row: a copy (+ one f32 add)
                    assert torch.equal(X.cpu(), feats[:, 0] if e is None else feats[:, 0] + e)
                else:
                    _check_pool(X, feats, avg, add=e)


# ================================================================================================ 8. one step / one loss kernel, three doors
@pytest.mark.parametrize("wk", WKINDS)
@pytest.mark.parametrize("H", [16, 48, 160])
@pytest.mark.parametrize("N", [1, 33])
def test_lstm_step_entry_points_same_bits(lib, wk, N, H):
    """deer_head_seq_lstm_step (c in place, h_n / c_n), deer_calib_lstm_step (idx NULL with its own c_out; an identity idx) and, on f32
    rows, deer_head_grad_lstm_step launch one kernel: equal h and c bit for bit, from a given state and from the zero state (NULL h_prev /
    c_prev; the in-place form has no NULL for c and gets zeros).  N = 1 a lone row, 33 a ragged second 32-row tile; H = 16 / 48 leave
    k-slices of a wave past H, 160 gives wave 0 a second k-iteration.  The taped gates reproduce c = gf c_prev + gi gg: two products and a
    sum, each rounded once (2^-24 of its own magnitude) or fused, so |c - c64| <= 4 x 2^-24 (|gf c_prev| + |gi gg|) - relative to the
    terms, as every gate of this module is, since the sum itself may cancel - and h = go tanh(c).  Every output is pitched and starts as NaN:
    padding stays NaN."""
    ld_pre, ld_h, ld_c, ld_out = 4 * H + 8, H + 8, H + 4, H + 12
    pre = rnd(N, 4 * H, seed=11)
    whh, _ = wq(rnd(4 * H, H, seed=14, scale=H ** -0.5), wk)
    bhh_d = cu(rnd(4 * H, seed=15, scale=0.1))
    pre_d = nanbuf(N, ld_pre)
    pre_d[:, :4 * H] = cu(pre)
    idx = torch.arange(N, dtype=torch.int32, device="cuda")
    zero_row = torch.zeros(H, device="cuda")
    for given in (True, False):
        hp = nanbuf(N, ld_h)
        hp[:, :H] = cu(rnd(N, H, seed=12, scale=0.5))
        cp = nanbuf(N, ld_c)
        cp[:, :H] = cu(rnd(N, H, seed=13, scale=0.5))
        hp_p, cp_p = (abi.ptr(hp), abi.ptr(cp)) if given else (None, None)
        # the sequence head's form
        c_seq = cp[:, :H].clone() if given else torch.zeros(N, H, device="cuda")
        h_seq, hn, cn = nanbuf(N, ld_out), nanbuf(N, H), nanbuf(N, H)
        abi.check(lib.deer_head_seq_lstm_step(abi.ptr(pre_d), ld_pre, hp_p, ld_h, abi.ptr(whh), wk, abi.ptr(bhh_d), abi.ptr(c_seq), abi.ptr(h_seq),
                                              ld_out, abi.ptr(hn), abi.ptr(cn), N, H, st()), "seq_lstm_step")
        outs = []
        # calibration's form: idx NULL, then the identity index
        for ix in (None, idx):
            c_o, h_o = nanbuf(N, ld_c), nanbuf(N, ld_out)
            abi.check(lib.deer_calib_lstm_step(abi.ptr(pre_d), ld_pre, hp_p, ld_h, cp_p, ld_c, abi.ptr(ix), abi.ptr(zero_row), abi.ptr(whh), wk,
                                               abi.ptr(bhh_d), abi.ptr(c_o), ld_c, abi.ptr(h_o), ld_out, N, H, st()), "calib_lstm_step")
            outs.append(("calib idx " + ("NULL" if ix is None else "identity"), h_o, c_o))
        gates = None
        if wk == 1:                                          # the tape's form: f32 rows only
            gates, c_o, h_o = pre_d.clone(), nanbuf(N, ld_c), nanbuf(N, ld_out)
            abi.check(lib.deer_head_grad_lstm_step(abi.ptr(gates), ld_pre, hp_p, ld_h, abi.ptr(whh), abi.ptr(bhh_d), cp_p, abi.ptr(c_o), ld_c,
                                                   abi.ptr(h_o), ld_out, N, H, st()), "head_grad_lstm_step")
            outs.append(("tape", h_o, c_o))
        sync()
        assert bool(torch.isfinite(h_seq[:, :H]).all()) and bool(torch.isfinite(c_seq).all())
        assert bool(torch.isnan(h_seq[:, H:]).all())
        assert torch.equal(hn, h_seq[:, :H]) and torch.equal(cn, c_seq)
        for what, h_o, c_o in outs:
            assert torch.equal(h_o[:, :H], h_seq[:, :H]), f"{what}: h (state given: {given})"
            assert torch.equal(c_o[:, :H], c_seq), f"{what}: c (state given: {given})"
            assert bool(torch.isnan(h_o[:, H:]).all()) and bool(torch.isnan(c_o[:, H:]).all()), f"{what}: padding written"
        if gates is not None:
            assert bool(torch.isnan(gates[:, 4 * H:]).all())
            gi, gf, gg, go = (gates[:, q * H:(q + 1) * H].double() for q in range(4))
            c_prev = cp[:, :H].double() if given else torch.zeros(N, H, dtype=torch.float64, device="cuda")
            t1, t2 = gf * c_prev, gi * gg
            r = float(((c_seq.double() - (t1 + t2)).abs() / (t1.abs() + t2.abs())).max())
            assert r <= 4 * 2.0 ** -24, f"taped gates vs c: {r:.3g}"
            # the fourth slot: h = go tanh(c), one f32 tanh of a value <= 1 (2^-22, as in test_head_seq_lstm_step) and one product
            rh = float(((h_seq[:, :H].double() - go * torch.tanh(c_seq.double())).abs() / go).max())
            assert rh <= 2.0 ** -22 + 2.0 ** -24, f"taped gates vs h: {rh:.3g}"


@pytest.mark.parametrize("R", [1, 257, 600])
@pytest.mark.parametrize("A", [1, 2])
def test_head_grad_loss_equals_exit_losses(lib, A, R):
    """deer_head_grad_loss and deer_exit_losses with one head launch the same two kernels: num, bin and loss bit for bit.  R = 257 / 600: the
    reduce's strided row loop (256 threads) with a ragged tail.  Pose errors a - label are exact in f32 and lie on both sides of the Huber
    knee |e| = 1 (1 -+ 2^-20), at it and well away from it.  dz starts as NaN: all of it is written, its last A slots per row are zero, and
    the rest is scale / R times [Huber'(e) (1 - a^2) / 6A | w_bin (prob - target) / A] in float64 within 8 x 2^-24 of each value: the f32
    factor (two roundings), 1 - a^2 or prob - target (at most two; a^2 is exact for these a) and two products."""
    errs = torch.tensor([0.25, -0.75, 1.0, -1.0, 1 + 2.0 ** -20, 1 - 2.0 ** -20, -(1 + 2.0 ** -20), -(1 - 2.0 ** -20), 1.5, -2.0, 0.0],
                        dtype=torch.float64)
    g = torch.Generator().manual_seed(100 * A + R)
    act = torch.randn(R, 8 * A, generator=g, dtype=torch.float64)
    act[:, :6 * A] = torch.randint(-8, 8, (R, 6 * A), generator=g).double() / 8        # multiples of 1/8: a - e and a - (a - e) are exact
    e = errs[torch.randint(0, len(errs), (R, 6 * A), generator=g)]
    e[0, 0] = 1.0
    pose = (act[:, :6 * A] - e).float()
    act = act.float()
    assert torch.equal((act[:, :6 * A].double() - pose.double()), e)
    grip = torch.randint(0, 2, (R, A), generator=g).float()
    act_d, pose_d, grip_d = cu(act), cu(pose), cu(grip)
    w_bin, scale = 0.01, 0.5
    num_e, bin_e, loss_e = nanbuf(R), nanbuf(R), nanbuf(1)
    abi.check(lib.deer_exit_losses(abi.ptr(act_d), abi.ptr(pose_d), abi.ptr(grip_d), 1, R, A, w_bin, abi.ptr(num_e), abi.ptr(bin_e), abi.ptr(loss_e),
                                   st()), "exit_losses")
    dz, num_g, bin_g, loss_g = nanbuf(R, 8 * A), nanbuf(R), nanbuf(R), nanbuf(1)
    abi.check(lib.deer_head_grad_loss(abi.ptr(act_d), abi.ptr(pose_d), abi.ptr(grip_d), R, A, w_bin, scale, abi.ptr(dz), abi.ptr(num_g),
                                      abi.ptr(bin_g), abi.ptr(loss_g), st()), "head_grad_loss")
    sync()
    assert bool(torch.isfinite(loss_e).all())
    assert torch.equal(num_g, num_e) and torch.equal(bin_g, bin_e) and torch.equal(loss_g, loss_e)
    assert bool(torch.isfinite(dz[:, :7 * A]).all()) and bool((dz[:, 7 * A:] == 0).all())
    a64, wb = act.double(), float(np.float32(w_bin))
    ref = torch.cat([scale / (R * 6 * A) * torch.where(e.abs() < 1, e, torch.sign(e)) * (1 - a64[:, :6 * A] ** 2),
                     scale * wb / (R * A) * (a64[:, 6 * A:7 * A] - grip.double())], 1)
    err = (dz[:, :7 * A].double().cpu() - ref).abs()
    assert bool((err <= 8 * 2.0 ** -24 * ref.abs()).all()), float((err / ref.abs().clamp_min(1e-300)).max())
