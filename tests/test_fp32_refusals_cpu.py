"""Argument rules of the fp32 arithmetic's entry points (csrc/precise.hip: deer_gemm_f32_nt, deer_attn_f32, deer_xattn_f32) and of
deer_gemm_skinny's operand modes: each call below is wrong in exactly ONE argument and is refused with DEER_ERR_SHAPE on the host, before
anything is enqueued, so these run without a GPU (tests/test_head_refusals_cpu.py).  On a machine with a GPU the pointers are zeroed device
buffers large enough for every read the call names and the control block says ALL_EXITED."""
import ctypes

import pytest
import torch

from deer_vla_amd import _abi as abi

SHAPE = 1
A_BF16, A_SLABS_GELU, A_SLABS, A_F32 = 0, 1, 2, 3


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


def test_gemm_f32_nt_refusals(env):
    lib, p, _ = env

    def gemm(A="p", W="p", C="p", lda=32, ldw=32, ldc=64, M=8, N=64, K=32, epi=0):
        g = lambda a: p if a == "p" else a
        return lib.deer_gemm_f32_nt(g(A), lda, g(W), ldw, p, g(C), ldc, M, N, K, epi, None)

    for bad in (dict(K=30, lda=32), dict(N=62), dict(lda=34), dict(ldw=34), dict(ldc=66), dict(epi=4), dict(epi=-1), dict(M=0), dict(N=0), dict(K=0),
                dict(A=None), dict(W=None), dict(C=None)):
        assert gemm(**bad) == SHAPE, bad


def _attn(lib, p, Q="p", K1="p", V1="p", K2="p", V2="p", O="p", batch=2, heads=2, q_len=5, kv1=40, kv2=24, ldq=128, ld1=128, ld2=128, ldo=128,
          qb=5 * 128, b1=40 * 128, b2=24 * 128, ob=5 * 128):
    g = lambda a: p if a == "p" else a
    return lib.deer_attn_f32(g(Q), g(K1), g(V1), g(K2), g(V2), g(O), batch, heads, q_len, kv1, kv2, ldq, ld1, ld2, ldo, qb, b1, b2, ob, 0.125, None)


def test_attn_f32_refusals(env):
    lib, p, _ = env
    new = (dict(ldo=124), dict(ldo=127), dict(ldq=64), dict(ld1=64), dict(ld2=64), dict(qb=5 * 128 + 2), dict(b1=40 * 128 + 1), dict(b2=24 * 128 + 3))
    old = (dict(kv1=600, kv2=65, b1=600 * 128, b2=65 * 128),         # 665 keys: past the chunked kernel's 156 KB of LDS (664 is its last)
           dict(kv1=1000, kv2=25, b1=1000 * 128, b2=25 * 128),       # past PAL_MAXKV
           dict(K2=None), dict(V2=None),                             # a second segment without its pointers
           dict(ldq=130), dict(ld1=130), dict(ld2=130), dict(Q=None), dict(K1=None), dict(V1=None), dict(O=None), dict(batch=0), dict(heads=0),
           dict(q_len=0), dict(kv1=0), dict(kv2=-1))
    for bad in new + old:
        assert _attn(lib, p, **bad) == SHAPE, bad
    assert _attn(lib, p, kv1=665, kv2=0, b1=665 * 128, K2=None, V2=None) == SHAPE            # 665 keys in one segment


def _xattn(lib, p, c, qslab="p", kv="p", tt="p", out="p", s_in=2, stride=32 * 512, ldqs=512, ldkv=3 * 2 * 512, inner=512, npm=64, ldo=512, T=5, n_kv=64,
           heads=8, batch=2):
    g = lambda a: p if a == "p" else a
    return lib.deer_xattn_f32(g(qslab), s_in, stride, ldqs, g(kv), ldkv, inner, g(tt), npm, g(out), ldo, T, n_kv, heads, batch, 0.125, c, None)


def test_xattn_f32_refusals(env):
    lib, p, c = env
    new = (dict(qslab=None), dict(kv=None), dict(tt=None), dict(out=None), dict(heads=0), dict(heads=-1), dict(inner=448), dict(inner=514),
           dict(ldo=508), dict(ldqs=508), dict(ldkv=1020), dict(stride=32 * 512 + 2))
    old = (dict(T=33), dict(T=0), dict(n_kv=129), dict(n_kv=0), dict(s_in=0), dict(npm=0), dict(batch=0), dict(ldkv=3 * 2 * 512 + 2), dict(ldqs=514))
    for bad in new + old:
        assert _xattn(lib, p, c, **bad) == SHAPE, bad


@pytest.mark.parametrize("name", ["deer_gemm_skinny", "deer_gemm_skinny_f16"])
def test_gemm_skinny_mode_refusals(env, name):
    lib, p, c = env
    f = getattr(lib, name)

    def sk(A="p", lda=64, slab="p", s_in=2, mode=A_F32, M=5, N=32, K=64, splitk=1):
        g = lambda a: p if a == "p" else a
        return f(g(A), lda, g(slab), s_in, 16 * 64, mode, p, p, M, N, K, splitk, c, None)

    for bad in (dict(mode=A_BF16, A=None), dict(mode=A_BF16, lda=68),          # bf16 rows: a pointer, 16-byte rows
                dict(mode=A_F32, A=None), dict(mode=A_F32, lda=66),            # f32 rows: a pointer, 16-byte rows
                dict(mode=A_SLABS, slab=None), dict(mode=A_SLABS, s_in=0),
                dict(mode=A_SLABS_GELU, slab=None), dict(mode=A_SLABS_GELU, s_in=0),
                dict(mode=4), dict(mode=-1),
                dict(M=0), dict(M=129), dict(N=40), dict(K=48), dict(splitk=0), dict(splitk=3)):
        assert sk(**bad) == SHAPE, bad
