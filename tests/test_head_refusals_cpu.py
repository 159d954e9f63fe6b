"""Argument rules of the action-head entry points (include/deer_hip.h): each call below is refused with DEER_ERR_SHAPE on the host, before
anything is enqueued, so these run without a GPU.  On a machine with a GPU the pointers are zeroed device buffers large enough for every read
the call names and the control block says ALL_EXITED, so that a call which slipped past its rule would return at entry instead of faulting."""
import ctypes

import pytest
import torch

from deer_vla_amd import _abi as abi

SHAPE = 1
SEQ_EPI_SIGMOID_LOGIT = 3


@pytest.fixture(scope="module")
def env():
    abi.build()
    lib = abi.lib()
    if torch.cuda.is_available():
        buf = torch.zeros(1 << 22, device="cuda")                           # 16 MB
        ctl = torch.zeros(16 * abi.CTL_WORDS, dtype=torch.int32, device="cuda")
        ctl[abi.CTL_ALL_EXITED] = 1
        yield lib, abi.ptr(buf), abi.ptr(ctl)
        torch.cuda.synchronize()
    else:
        fake = ctypes.c_void_p(1 << 20)                                     # never dereferenced: the calls are refused on the host
        yield lib, fake, fake


def _final(lib, p, c, fn="deer_head_final", in_dim=256, kind=abi.KIND_COMMIT, slot=0, thr=True, ctl=True, A=None, act_ext=None):
    args = [p, 2 * in_dim, in_dim, abi.PRO_GROUP_LN_RELU, p, p, p, p, p, p, p, p, c if ctl else None, kind, 3, slot, p if thr else None,
            0, 0, 1, None, None, None, None, 1, 8, 1, p, 1e-5, 2]
    if fn != "deer_head_final":
        args += [A, act_ext]
    return getattr(lib, fn)(*args, None)


def test_head_final_refusals(env):
    lib, p, c = env
    assert _final(lib, p, c, in_dim=1004) == SHAPE                                   # in_dim % 8
    for A in (0, 9):                                                                # multi_step_action outside 1..8
        assert _final(lib, p, c, fn="deer_head_final_multi", A=A, act_ext=p) == SHAPE
    assert _final(lib, p, c, fn="deer_head_final_multi", A=2, act_ext=None) == SHAPE    # A > 1 with a control block needs act_ext
    assert _final(lib, p, c, kind=abi.KIND_CHECK, thr=False) == SHAPE                # an exit check needs thresholds ...
    assert _final(lib, p, c, kind=abi.KIND_CHECK, ctl=False) == SHAPE                # ... and a control block
    assert _final(lib, p, c, fn="deer_head_final_env", kind=abi.KIND_CHECK, slot=16, A=1, act_ext=None) == SHAPE   # rows of 16 exit slots


def test_head_fc_and_lstm_refusals(env):
    lib, p, c = env

    def fc(in_dim, pro, B):
        return lib.deer_head_fc(p, in_dim, in_dim, pro, p, p, p, p, p, p, p, p, 8, p, B, 1e-5, c, 1, 3, 0, None)

    def lstm(in_dim, H):
        return lib.deer_head_lstm_layer(p, in_dim, abi.X_RAW, 1, in_dim, None, None, p, p, p, p, p, p, p, p, H, 1, 1e-5, c, 1, 3, 0, None)

    assert fc(1004, abi.PRO_RAW, 1) == SHAPE                                          # in_dim % 8
    assert fc(2056, abi.PRO_LN, 1) == SHAPE                                           # a LayerNorm over more than 2048 values
    assert fc(2048, abi.PRO_RAW, 8) == SHAPE                                          # 8 x 2048 f32 (+ 16): past 64 KB of LDS
    assert lstm(1004, 1024) == SHAPE and lstm(1024, 1020) == SHAPE                    # in_dim % 8, H % 8


def test_head_seq_refusals(env):
    lib, p, _ = env

    def step(H, ld_h):
        return lib.deer_head_seq_lstm_step(p, 4 * H, p, ld_h, p, 2, p, p, p, H, None, None, 4, H, None)

    def gemm(ldx, K, ldo, epi):
        return lib.deer_head_seq_gemm(p, ldx, p, 2, p, p, ldo, 4, 16, K, epi, None)

    assert step(24, 24) == SHAPE                                                      # H % 16
    assert step(32, 36) == SHAPE                                                      # h_prev row stride % 8
    assert gemm(16, 12, 16, 0) == SHAPE                                               # K % 8
    assert gemm(12, 8, 16, 0) == SHAPE                                                # ldx % 8
    assert gemm(16, 16, 20, SEQ_EPI_SIGMOID_LOGIT) == SHAPE                           # the logit epilogue stores 2 N columns per row
