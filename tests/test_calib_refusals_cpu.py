"""Argument rules of the four calibration entry points (csrc/calib.hip, include/deer_hip.h): every call below differs from a valid call in
ONE argument and is refused with DEER_ERR_SHAPE on the host, before anything is enqueued, so these run without a GPU.  The calling pattern
is tests/test_head_refusals_cpu.py's: without a GPU the device pointers are a dummy address that is never dereferenced; on a machine with a
GPU they point into a zeroed device buffer large enough for every read and write the valid call names, and that valid call is made once and
must return DEER_OK - which shows that each refusal is owed to the one argument it changes.  `layers` and `slot_of_layer` are HOST arrays
(the entry points read them) and are real in both cases."""
import ctypes

import pytest
import torch

from deer_vla_amd import _abi as abi

OK, SHAPE = 0, 1
MAX_NL, MAX_LAYERS = 17, 64                                  # DEER_CALIB_MAX_NL, DEER_CALIB_MAX_LAYERS (include/deer_hip.h)


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


@pytest.fixture(scope="module")
def env():
    abi.build()
    lib = abi.lib()
    if torch.cuda.is_available():
        buf = torch.zeros(1 << 21, device="cuda")                          # 8 MB of zeros: floats 0.0, int32 words 0
        yield lib, (lambda k: ctypes.c_void_p(buf.data_ptr() + (k << 20))), True    # eight disjoint regions of 1 MB
        torch.cuda.synchronize()
    else:
        yield lib, (lambda k: ctypes.c_void_p((1 + k) << 20)), False       # never dereferenced: the calls are refused on the host


def _variations(call, base, cases, gpu):
    if gpu:
        assert call(**base) == OK, "the valid call every refusal is a variation of"
    for what, change in cases:
        assert call(**{**base, **change}) == SHAPE, what


def test_calib_pool_layers_refusals(env):
    lib, at, gpu = env

    def call(hidden, stride, layers, NL, P, n_frames, T, d):
        return lib.deer_calib_pool_layers(hidden, stride, layers, NL, P, n_frames, T, d, 0, None)

    base = dict(hidden=at(0), stride=2 * 3 * 8 + 8, layers=ints(0, 2), NL=2, P=at(1), n_frames=2, T=3, d=8)
    _variations(call, base, [
        ("hidden NULL", dict(hidden=None)), ("layers NULL", dict(layers=None)), ("P NULL", dict(P=None)),
        ("NL 0", dict(NL=0)), ("NL above DEER_CALIB_MAX_NL", dict(NL=MAX_NL + 1, layers=ints(*range(MAX_NL + 1)))),
        ("n_frames 0", dict(n_frames=0)), ("T 0", dict(T=0)), ("d 0", dict(d=0)),
        ("d % 4", dict(d=6, stride=64)),
        ("layer_stride below n_frames T d", dict(stride=2 * 3 * 8 - 1)),
        ("a negative layer", dict(layers=ints(0, -1))),
    ], gpu)


def test_calib_gather_refusals(env):
    lib, at, gpu = env

    def call(P, rl, slots, n_layers, X, idx, bc, W, NL, d):
        return lib.deer_calib_gather(P, rl, slots, n_layers, X, idx, bc, W, NL, d, None)

    base = dict(P=at(0), rl=at(1), slots=ints(0, -1, 1), n_layers=3, X=at(2), idx=at(3), bc=2, W=4, NL=2, d=8)
    _variations(call, base, [
        ("P NULL", dict(P=None)), ("rand_layers NULL", dict(rl=None)), ("slot_of_layer NULL", dict(slots=None)), ("X NULL", dict(X=None)),
        ("idx NULL", dict(idx=None)),
        ("n_layers 0", dict(n_layers=0)), ("n_layers above DEER_CALIB_MAX_LAYERS", dict(n_layers=MAX_LAYERS + 1, slots=ints(*([0] * (MAX_LAYERS + 1))))),
        ("bc 0", dict(bc=0)), ("W 1", dict(W=1)), ("W 0", dict(W=0)),
        ("NL 1", dict(NL=1, slots=ints(0, -1, 0))), ("NL 0", dict(NL=0, slots=ints(-1, -1, -1))),
        ("NL above DEER_CALIB_MAX_NL", dict(NL=MAX_NL + 1)),
        ("d 0", dict(d=0)), ("d % 4", dict(d=6)),
        ("slot_of_layer[l] == NL", dict(slots=ints(0, -1, 2))), ("slot_of_layer[l] > NL", dict(slots=ints(7, -1, 1))),
    ], gpu)


def test_calib_lstm_step_refusals(env):
    lib, at, gpu = env

    def call(pre, ld_pre, h_prev, ld_h, c_prev, ld_c, idx, zero_row, w_hh, wk, b_hh, c_out, ld_co, h_out, ld_out, N, H):
        return lib.deer_calib_lstm_step(pre, ld_pre, h_prev, ld_h, c_prev, ld_c, idx, zero_row, w_hh, wk, b_hh, c_out, ld_co, h_out, ld_out, N, H, None)

    H = 32
    base = dict(pre=at(0), ld_pre=4 * H, h_prev=at(1), ld_h=H, c_prev=at(2), ld_c=H, idx=at(3), zero_row=at(4), w_hh=at(5), wk=1, b_hh=at(4),
                c_out=at(6), ld_co=H, h_out=at(7), ld_out=H, N=4, H=H)
    _variations(call, base, [
        ("pre NULL", dict(pre=None)), ("w_hh NULL", dict(w_hh=None)), ("b_hh NULL", dict(b_hh=None)), ("h_out NULL", dict(h_out=None)),
        ("N 0", dict(N=0)), ("H 0", dict(H=0)),
        ("H % 16", dict(H=24, ld_pre=128, ld_h=32)),
        ("ld_h % 8", dict(ld_h=H + 4)), ("ld_h < H", dict(ld_h=H - 8)),
        ("c_prev without h_prev", dict(h_prev=None)), ("ld_c < H", dict(ld_c=H - 1)),
        ("idx with h_prev but no zero_row", dict(zero_row=None)),
        ("ld_pre < 4 H", dict(ld_pre=4 * H - 1)), ("ld_out < H", dict(ld_out=H - 1)), ("c_out with ld_co < H", dict(ld_co=H - 1)),
        ("w_kind 3", dict(wk=3)), ("w_kind -1", dict(wk=-1)),
    ], gpu)
    # what the rules leave open stays open: no previous state at all, and an index without a zero row when there is no h_prev to index
    if gpu:
        assert call(**{**base, "h_prev": None, "c_prev": None, "zero_row": None}) == OK
        assert call(**{**base, "c_out": None, "ld_co": 0}) == OK


def test_calib_delta_refusals(env):
    lib, at, gpu = env

    def call(act, ld_act, NL, rows, NP, thr, values, ld_val):
        return lib.deer_calib_delta(act, ld_act, NL, rows, NP, thr, values, ld_val, None)

    base = dict(act=at(0), ld_act=8, NL=3, rows=5, NP=6, thr=0, values=at(1), ld_val=5)
    _variations(call, base, [
        ("actions NULL", dict(act=None)), ("values NULL", dict(values=None)),
        ("NL 1", dict(NL=1)), ("rows 0", dict(rows=0)), ("NP 0", dict(NP=0)),
        ("ld_act < NP", dict(ld_act=5)), ("ld_val < rows", dict(ld_val=4)),
        ("thr_type 4", dict(thr=4)), ("thr_type -1", dict(thr=-1)),
    ], gpu)
