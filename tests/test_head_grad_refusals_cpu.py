"""Argument rules of the exit-only fine-tuning entry points (csrc/head_grad.hip, deer_head_loss_grad of csrc/model.hip): every refusal is
DEER_ERR_SHAPE on the host, before any launch, attribute call or allocation - so they can be checked on a machine without a GPU (the
pointers below are never dereferenced)."""
import ctypes

import pytest

from deer_vla_amd import _abi as abi
from deer_vla_amd.config import deer_tiny
from deer_vla_amd.engine import config_to_c

ERR = 1
FAKE = ctypes.c_void_p(0x10000)          # a non-NULL, 16-byte aligned address that is never read


@pytest.fixture(scope="module")
def lib():
    abi.build()
    return abi.lib()


def _model(lib, **kw):
    h = ctypes.c_void_p()
    cc = config_to_c(deer_tiny(**kw), 1, 32)
    assert lib.deer_model_create(ctypes.byref(cc), ctypes.byref(h)) == 0
    return h


def _loss_grad(lib, h, head=0, params=FAKE, X=FAKE, N=2, L=3, pose=FAKE, grip=FAKE, grad=FAKE, loss=FAKE):
    return lib.deer_head_loss_grad(h, head, params, X, N, L, pose, grip, 0.01, 1.0, grad, 0, loss, None)


def test_loss_grad_refuses_null_pointers_and_row_counts(lib):
    h = _model(lib)
    try:
        for k in ("params", "X", "pose", "grip", "grad"):
            assert _loss_grad(lib, h, **{k: None}) == ERR, k
        assert lib.deer_head_loss_grad(None, 0, FAKE, FAKE, 2, 3, FAKE, FAKE, 0.01, 1.0, FAKE, 0, FAKE, None) == ERR
        for N, L in ((0, 3), (2, 0), (-1, 3), (2, -3), (2049, 1), (1, 2049), (64, 33), (1 << 20, 1 << 20)):
            assert _loss_grad(lib, h, N=N, L=L) == ERR, (N, L)
    finally:
        lib.deer_model_destroy(h)


def test_loss_grad_refuses_a_head_the_model_lacks(lib):
    h = _model(lib)
    hl = _model(lib, layerwise_exit_eval=True)
    try:
        for head in (-1, 1, 7):
            assert _loss_grad(lib, h, head=head) == ERR
        n = len(deer_tiny(layerwise_exit_eval=True).exit_ids())
        assert _loss_grad(lib, hl, head=n + 1) == ERR and _loss_grad(lib, hl, head=-1) == ERR
        assert lib.deer_head_param_count(hl, n) > 0 and lib.deer_head_param_count(hl, n + 1) == -1
        off, numel, dec = ctypes.c_long(), ctypes.c_long(), ctypes.c_int()
        assert lib.deer_head_param_entry(h, 1, 0, None, 0, ctypes.byref(off), ctypes.byref(numel), ctypes.byref(dec)) == ERR
        assert lib.deer_head_param_entry(h, 0, 10 ** 6, None, 0, ctypes.byref(off), ctypes.byref(numel), ctypes.byref(dec)) == ERR
    finally:
        lib.deer_model_destroy(h)
        lib.deer_model_destroy(hl)


def test_loss_grad_refuses_a_use_state_model_and_says_why(lib, capfd):
    h = _model(lib, use_state=True)
    try:
        capfd.readouterr()
        assert _loss_grad(lib, h) == ERR
        err = capfd.readouterr().err
        assert "use_state" in err and "state embeddings" in err and "not built" in err, err
    finally:
        lib.deer_model_destroy(h)


def test_multi_step_action_outside_1_to_8_has_no_model(lib):
    """A outside 1..8: such a model cannot be created, so no gradient call can reach it (0 means one action)"""
    for A in (9, -1):
        h = ctypes.c_void_p()
        cc = config_to_c(deer_tiny(), 1, 32)
        cc.multi_step_action = A
        assert lib.deer_model_create(ctypes.byref(cc), ctypes.byref(h)) == ERR
    assert lib.deer_head_grad_loss(FAKE, FAKE, FAKE, 4, 0, 0.01, 1.0, FAKE, FAKE, FAKE, FAKE, None) == ERR
    assert lib.deer_head_grad_loss(FAKE, FAKE, FAKE, 4, 9, 0.01, 1.0, FAKE, FAKE, FAKE, FAKE, None) == ERR
    assert lib.deer_head_grad_loss(FAKE, FAKE, FAKE, 0, 1, 0.01, 1.0, FAKE, FAKE, FAKE, FAKE, None) == ERR


def test_piece_kernels_refuse_bad_arguments(lib):
    F = FAKE
    assert lib.deer_head_grad_ln(None, 8, F, 8, F, F, F, 4, 8, 1e-5, 0, None) == ERR
    assert lib.deer_head_grad_ln(F, 8, F, 8, F, F, None, 4, 8, 1e-5, 0, None) == ERR
    assert lib.deer_head_grad_ln(F, 4, F, 8, F, F, F, 4, 8, 1e-5, 0, None) == ERR                    # pitch below the row
    assert lib.deer_head_grad_lstm_step(F, 64, None, 0, F, F, None, F, 16, F, 16, 2, 24, None) == ERR   # H % 16
    assert lib.deer_head_grad_lstm_step(F, 32, None, 0, F, F, None, F, 16, F, 16, 2, 16, None) == ERR   # pitch below 4H
    assert lib.deer_head_grad_lstm_step(F, 64, F, 16, F, F, None, F, 16, F, 16, 2, 16, None) == ERR     # h_prev without c_prev
    assert lib.deer_head_grad_lstm_step(F, 64, None, 0, F, F, None, F, 16, F, 16, 0, 16, None) == ERR
    assert lib.deer_head_grad_gemm(None, 8, 0, F, 8, 0, F, 8, 4, 4, 8, 0, None) == ERR
    assert lib.deer_head_grad_gemm(F, 8, 0, F, 8, 0, F, 8, 0, 4, 8, 0, None) == ERR
    assert lib.deer_head_grad_gemm(F, 4, 0, F, 8, 0, F, 8, 4, 4, 8, 0, None) == ERR                  # lda below K
    assert lib.deer_head_grad_gemm(F, 8, 1, F, 8, 0, F, 8, 16, 4, 8, 0, None) == ERR                 # k-major A: lda below M
    assert lib.deer_head_grad_gemm(F, 8, 0, F, 8, 0, F, 2, 4, 4, 8, 0, None) == ERR                  # ldc below N
    assert lib.deer_head_grad_colsum(F, 8, None, 0, None, None, None, None, 4, 8, 0, None) == ERR    # no output
    assert lib.deer_head_grad_colsum(F, 8, None, 0, None, F, None, F, 4, 8, 0, None) == ERR          # d gamma without x / stats
    assert lib.deer_head_grad_colsum(F, 4, None, 0, None, F, None, None, 4, 8, 0, None) == ERR
    assert lib.deer_head_grad_relu_mask(F, F, 6, None) == ERR                                        # n % 4
    assert lib.deer_head_grad_relu_mask(F, None, 8, None) == ERR
    assert lib.deer_head_grad_ln_bwd(F, 8, F, 8, None, F, F, 8, 4, 8, None) == ERR
    assert lib.deer_head_grad_ln_bwd(F, 8, F, 8, F, F, F, 4, 4, 8, None) == ERR
    assert lib.deer_head_grad_lstm_bwd_step(F, 16, None, F, F, 64, F, F, None, 16, None, 2, 16, None) == ERR   # no dc
    assert lib.deer_head_grad_lstm_bwd_step(F, 16, None, F, F, 64, F, F, None, 16, F, 2, 20, None) == ERR      # H % 16
    assert lib.deer_head_grad_lstm_bwd_step(F, 8, None, F, F, 64, F, F, None, 16, F, 2, 16, None) == ERR       # pitch below H


def test_adamw_refuses_bad_arguments(lib):
    F = FAKE

    def call(p=F, g=F, m=F, v=F, n=8, se=None, sd=None, ns=0, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=1):
        hyper = (ctypes.c_double * 5)(lr, b1, b2, eps, wd)
        return lib.deer_adamw_step(p, g, m, v, n, se, sd, ns, hyper, step, None)
    for k in ("p", "g", "m", "v"):
        assert call(**{k: None}) == ERR, k
    assert call(n=0) == ERR and call(n=-4) == ERR and call(n=1 << 31) == ERR
    assert call(ns=2) == ERR and call(ns=-1) == ERR and call(ns=2, se=F) == ERR          # a segment table needs both arrays
    assert call(step=0) == ERR and call(lr=-1.0) == ERR and call(b1=1.0) == ERR and call(b2=-0.1) == ERR and call(eps=-1.0) == ERR
    assert call(wd=-0.1) == ERR and call(lr=float("nan")) == ERR
    assert lib.deer_adamw_step(F, F, F, F, 8, None, None, 0, None, 1, None) == ERR          # no hyper-parameters
