"""Argument rules of deer_value_log_append (csrc/value_log.hip): each call below is wrong in exactly ONE argument and is refused with
DEER_ERR_SHAPE on the host, before anything is enqueued, so these run without a GPU (tests/test_fp32_refusals_cpu.py).  On a machine with
a GPU the pointers are zeroed device buffers large enough for every access the call names."""
import ctypes

import pytest
import torch

from deer_vla_amd import _abi as abi

SHAPE = 1


@pytest.fixture(scope="module")
def env():
    abi.build()
    lib = abi.lib()
    if torch.cuda.is_available():
        buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
        yield lib, abi.ptr(buf)
        torch.cuda.synchronize()
    else:
        yield lib, ctypes.c_void_p(1 << 20)                                 # never dereferenced: the calls are refused on the host


def test_value_log_append_refusals(env):
    lib, p = env

    def append(ctl="p", n_envs=4, n_exit=6, active_mask=0b1011, values="p", ld=40, capacity=32, taken="p", state="p"):
        g = lambda a: p if a == "p" else a
        return lib.deer_value_log_append(g(ctl), n_envs, n_exit, active_mask, g(values), ld, capacity, g(taken), g(state), None)

    for bad in (dict(n_envs=0), dict(n_envs=-1), dict(n_envs=17, active_mask=0),
                dict(n_exit=0), dict(n_exit=-2), dict(n_exit=17),
                dict(capacity=0), dict(capacity=-5),
                dict(ld=31), dict(ld=0),
                dict(active_mask=0b10000), dict(active_mask=0b11011), dict(active_mask=-1), dict(active_mask=1 << 16), dict(n_envs=3),
                dict(ctl=None), dict(values=None), dict(taken=None), dict(state=None)):
        assert append(**bad) == SHAPE, bad                                  # (the call without `bad` is valid: tests/test_value_log_kernel.py)
