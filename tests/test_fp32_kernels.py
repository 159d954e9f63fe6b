"""The kernels only the fp32 arithmetic (deer_config.precision = 1) reaches in a default build, one at a time through the C ABI, against
float64 references gated ELEMENT BY ELEMENT (tests/test_hip_ops.py gates them with one norm ratio per tensor on contiguous N(0, 1) buffers):
csrc/precise.hip - deer_gemm_f32_nt, deer_attn_f32 (keys resident in LDS / chunked), deer_xattn_f32 - and the non-plane trunk form of
csrc/model.hip::llm_layer: deer_gemm_skinny (and its `_f16` twin) launched once per weight plane as model.hip::skinny does, deer_mpt_attn_small
with f32 output, deer_resadd_ln with out_f32.

Conventions of tests/test_trunk_kernels.py (helpers copied, not imported): operands drawn on the device from fixed seeds; every operand is
a strided VIEW of a NaN-filled buffer (padding columns, gap rows, the other projections' columns), every output a view of a NaN-filled
buffer that must still be NaN everywhere else; check() works per element in float64 and names the worst element; the largest error /
bound per family is printed at the end of the module.  Slab operands lie on a 2^-10 grid, so that their f32 sum is exact and the reference
sees the value the kernel reads.
  ACC    f32 accumulation: |err| <= ACC * S, S = sum_k |a_k w_k|.  4e-6, the class gate of the other per-kernel suites
  PAIR   the residue of a hi + lo pair: 2^-16 (bf16), 2^-22 (fp16); U / TINY half an ulp / half the subnormal step of the 16-bit format
  SM     what a softmax row adds beside the score error: expf of the numerators and of the denominator's terms (2 + 2 ulp), the sum (<= 11
         terms per lane and 6 butterfly levels), the reciprocal and the product: 25 roundings as worst cases, 2^-19 = 32 * 2^-24
The launches go through the k_* functions, so that the same cases can be run with torch float32 in their place (how the references and
bounds were checked before the first GPU run; ratios in the commit message)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from deer_vla_amd import _abi as abi  # noqa: E402

DEV = "cuda"
ACC = 4e-6
SM = 2.0 ** -19
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TINY = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25}
PAIR = {"bf16": 2.0 ** -16, "f16": 2.0 ** -22}
F16_MAX = 65504.0
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
NAN = float("nan")
FLOOR = 2.0 ** -149
A_BF16, A_SLABS_GELU, A_SLABS, A_F32 = 0, 1, 2, 3
PE_F32, PE_QGELU, PE_GELU, PE_RESADD = 0, 1, 2, 3
RATIOS = {}                                  # family -> largest measured error / bound


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if DEV == "cuda" else None


def sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


def randn(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


def on_grid(x, step=2.0 ** -10):
    """values on a grid coarse enough that sums of a few of them are exact in f32"""
    return torch.round(x / step) * step


def ctl_block(all_exited):
    c = torch.zeros(abi.CTL_WORDS, dtype=torch.int32, device=DEV)
    c[abi.CTL_ALL_EXITED] = 1 if all_exited else 0
    return c


@pytest.fixture(scope="module")
def lib():
    l = abi.lib()
    assert l.deer_hip_arch() == b"gfx950"
    yield l
    print("\nlargest error / bound per family: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RATIOS.items())))


def check(out, ref, bound, what, key=None):
    """|out - ref| <= bound element by element (float64 on the device); a NaN / inf output where the reference is finite fails"""
    out = out.double()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=out.device).expand(out.shape)
    ref = ref.expand(out.shape)
    r = torch.nan_to_num((out - ref).abs() / bound, nan=math.inf, posinf=math.inf)
    worst = int(r.argmax())
    rmax = float(r.reshape(-1)[worst])
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(r.shape)))
    assert rmax <= 1.0, (f"{what}: worst element {idx}: out {float(out.reshape(-1)[worst])!r} ref {float(ref.reshape(-1)[worst])!r} "
                         f"bound {float(bound.reshape(-1)[worst]):.3g} (error / bound {rmax:.3g})")
    if key is not None:
        RATIOS[key] = max(RATIOS.get(key, 0.0), rmax)
    return rmax


def half_ulp32(v):
    """1/2 ulp of the f32 nearest to every element of a float64 tensor"""
    a = v.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a)))).clamp(min=-126)
    e = torch.where(a > 0, e, torch.full_like(e, -126))
    return torch.exp2(e - 24)


def untouched(buf, *views):
    """every element of `buf` outside the given views (slices of it) is still NaN"""
    seen = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    for v in views:
        off = (v.data_ptr() - buf.data_ptr()) // buf.element_size()
        torch.as_strided(seen, v.shape, v.stride(), off).fill_(True)
    return all_nan(buf[~seen])


# ================================================================================================ 1. deer_gemm_f32_nt
def k_gemm(lib, A, W, bias, C, epi):
    """A [M, K], W [N, K], C [M, N]: views whose row stride is the leading dimension"""
    (M, K), N = A.shape, W.shape[0]
    abi.check(lib.deer_gemm_f32_nt(abi.ptr(A), A.stride(0), abi.ptr(W), W.stride(0), abi.ptr(bias), abi.ptr(C), C.stride(0), M, N, K, epi, st()), "gemm_f32_nt")
    sync()


def quick_gelu64(x):
    return x * torch.sigmoid(1.702 * x)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 2.0 ** -0.5))


def gemm_ref(A, W, bias, epi, C0):
    """fp64 of the epilogue and its bound: ACC S with S = sum |a w| + |bias| on the pre-activation; through an activation its largest slope
    (QuickGELU x sigmoid(1.702 x): 1.0998 at 1.702 x = 2.4; erf-GELU: 1.129) and half an f32 ulp of the result; the residual epilogue half an
    ulp of the new C"""
    A64, W64 = A.double(), W.double()
    x, S = A64 @ W64.t(), A64.abs() @ W64.abs().t()
    if bias is not None:
        x, S = x + bias.double(), S + bias.double().abs()
    e = ACC * S
    if epi == PE_QGELU:
        y = quick_gelu64(x)
        return y, 1.1 * e + half_ulp32(y) + FLOOR, S
    if epi == PE_GELU:
        y = gelu64(x)
        return y, 1.13 * e + half_ulp32(y) + FLOOR, S
    if epi == PE_RESADD:
        y = C0.double() + x
        return y, e + half_ulp32(y) + FLOOR, S
    return x, e + FLOOR, S


def gemm_operands(M, N, K, seed, hard):
    """hard: activation channel K / 2 at 1000 x, the output columns of one group of four at 1e-3, and the last row of A made orthogonal to
    W[0] in fp64 up to 1e-6 of sum |a w|: C[M - 1, 0] is what is left of a cancellation"""
    A, W, bias = randn(M, K, seed=seed), randn(N, K, seed=seed + 1, scale=K ** -0.5), randn(N, seed=seed + 2, scale=0.5)
    if hard:
        A[:, K // 2] *= 1000.0
        g0 = 4 * ((N // 4) // 2)
        W[g0:g0 + 4] *= 1e-3
        a, w = A[M - 1].double(), W[0].double()
        a = a - (a @ w) / (w @ w) * w
        a = a + 1e-6 * float(a.abs() @ w.abs()) / (w @ w) * w
        A[M - 1] = a.float()
        assert abs(float(A[M - 1].double() @ w)) <= 3e-6 * float(A[M - 1].double().abs() @ w.abs())
    return A, W, bias


GEMM_M, GEMM_N, GEMM_K = [1, 63, 64, 65, 130], [4, 60, 64, 68, 132], [4, 28, 32, 36, 68, 100]
GEMM_EPI = [PE_F32, PE_QGELU, PE_GELU, PE_RESADD]


def run_gemm(lib, M, N, K, epi, has_bias, pad, hard, seed):
    A, W, bias = gemm_operands(M, N, K, seed, hard)
    if not has_bias:
        bias = None
    Ab, Wb, Cb = nans(M + 1, K + pad), nans(N + 1, K + 16 - pad), nans(M + 2, N + pad)
    Av, Wv, Cv = Ab[:M, :K], Wb[:N, :K], Cb[:M, :N]
    Av.copy_(A)
    Wv.copy_(W)
    C0 = randn(M, N, seed=seed + 3) if epi == PE_RESADD else None
    if C0 is not None:
        Cv.copy_(C0)
    k_gemm(lib, Av, Wv, bias, Cv, epi)
    assert untouched(Cb, Cv), f"M {M} N {N} K {K} epi {epi}: stored past row M / column N"
    ref, bound, S = gemm_ref(A, W, bias, epi, C0)
    return Cv, ref, bound, S


@pytest.mark.parametrize("epi", GEMM_EPI)
def test_gemm_f32_nt(lib, epi):
    """half of the M x N x K product per epilogue (the other half under the next one): one row, rows and columns one short of / at / one
    past the 64-wide tile, three tiles; K of one float4, tails inside the 32-column tile (4, 28, 36 = 32 + 4, 68, 100) and whole tiles, one
    to four tiles (odd and even counts of the double buffer); leading dimensions 4 and 12 past K / N; bias by case; N(0, 1) and hard operands"""
    n = 0
    for im, M in enumerate(GEMM_M):
        for i_n, N in enumerate(GEMM_N):
            for ik, K in enumerate(GEMM_K):
                if (im + i_n + ik + epi) % 2:
                    continue
                n += 1
                has_bias, pad, hard = (n % 2 == 0), (4 if n % 3 else 12), (n % 4 in (1, 2))
                C, ref, bound, _ = run_gemm(lib, M, N, K, epi, has_bias, pad, hard, seed=1000 * epi + 10 * n)
                check(C, ref, bound, f"M {M} N {N} K {K} epi {epi} bias {has_bias} hard {hard}", key=f"gemm_f32{'_hard' if hard else ''}/epi{epi}")
    assert n == 75


# ================================================================================================ 2. deer_attn_f32
def k_attn(lib, q, k1, v1, k2, v2, o, scale):
    """q / o [batch, q_len, heads * 64], k_s / v_s [batch, kv_s, heads * 64]: views; strides 1 and 0 are the leading dimension and the batch stride"""
    batch, q_len, C = q.shape
    kv1, kv2 = k1.shape[1], (k2.shape[1] if k2 is not None else 0)
    ld2, b2 = (k2.stride(1), k2.stride(0)) if k2 is not None else (0, 0)
    abi.check(lib.deer_attn_f32(abi.ptr(q), abi.ptr(k1), abi.ptr(v1), abi.ptr(k2), abi.ptr(v2), abi.ptr(o), batch, C // 64, q_len, kv1, kv2, q.stride(1),
                                k1.stride(1), ld2, o.stride(1), q.stride(0), k1.stride(0), b2, o.stride(0), scale, st()), "attn_f32")
    sync()


def softmax_ref(s, es, vis, v, n_sum):
    """fp64 softmax(s) v over the visible keys and the bound of the f32 kernels (csrc/precise.hip), from fp64 quantities alone:
    scores: every score within es of fp64, E = the row's largest es: |p~_j - p_j| <= p_j (1 - p_j) (e^2E - 1) (tests/test_trunk_kernels.py::
            xattn_ref: a one-hot row moves by nothing, a flat row by 2 E);
    expf(s_j - max): the rounded difference is off by 2^-24 (max - s_j) relative on p_j (2^-23 with the two operands' own rounding);
    the rest of the row (SM, top of the module);
    P V: `n_sum` sequential multiply-adds in f32: ACC sum_j p_j |v_j|; probabilities that underflow f32: 2^-120 sum_j |v_j|"""
    sm = s.masked_fill(~vis, -math.inf)
    m = sm.amax(-1, keepdim=True)
    p = torch.exp(sm - m)
    p = p / p.sum(-1, keepdim=True)
    E = es.masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    rp = torch.expm1(2 * E) * (1 - p) + 2.0 ** -23 * (m - sm).masked_fill(~vis, 0.0) + SM
    av = v.abs()
    o = p @ v
    eo = (p * rp) @ av + ACC * (p @ av) + 2.0 ** -120 * av.sum(-2, keepdim=True) + FLOOR
    return o, eo, (sm, m)


def attn_ref(q, k, v, scale):
    """q [batch, q_len, C], k / v [batch, kv, C] (both segments): fp64 attention per head of 64 and its bound.  Scores: q * scale rounded once,
    then 64 sequential multiply-adds: es = ACC scale sum_d |q_d k_d|"""
    batch, q_len, C = q.shape
    hs = lambda t: t.double().reshape(batch, t.shape[1], C // 64, 64).transpose(1, 2)
    q, k, v = hs(q), hs(k), hs(v)
    s = scale * (q @ k.transpose(-1, -2))
    es = ACC * scale * (q.abs() @ k.abs().transpose(-1, -2))
    o, eo, extra = softmax_ref(s, es, torch.ones_like(s, dtype=torch.bool), v, k.shape[2])
    back = lambda t: t.transpose(1, 2).reshape(batch, q_len, C)
    return back(o), back(eo), extra


def attn_operands(batch, heads, q_len, kv, seed, scale):
    """N(0, 1) q / k / v; with more than one key, per (batch, head): the LAST key is 82 / (scale |q_0|^2) q_0, so that it leads query 0 by
    ~82 (every other key sits near -80 after the max) and, with more than one query, the last query is 0 (all scores equal, uniform row)"""
    C = heads * 64
    q, k, v = randn(batch, q_len, C, seed=seed), randn(batch, kv, C, seed=seed + 1), randn(batch, kv, C, seed=seed + 2)
    if kv > 1:
        q0 = q[:, 0].reshape(batch, heads, 64)
        k[:, kv - 1] = (q0 * (82.0 / (scale * (q0 * q0).sum(-1, keepdim=True)))).reshape(batch, C)
        if q_len > 1:
            q[:, q_len - 1] = 0.0
    return q, k, v


ATTN_QLEN = [1, 31, 32, 33, 70]
ATTN_KV1 = [1, 63, 64, 65, 352, 353, 512, 513, 664]
ATTN_KV2 = [(1, 63), (63, 2), (255, 2), (300, 271), (352, 1), (600, 64)]
ATTN_HB = [(1, 2), (3, 1), (3, 2), (1, 1)]


def run_attn(lib, batch, heads, q_len, kv1, kv2, seed, scale=0.125):
    """q | k | v as column slices of one [batch][rows + 1][3 C + 4] buffer (one NaN gap row per batch, four NaN columns); the second segment
    as k | v in its own [batch][kv2 + 1][2 C + 8] buffer; out [batch][q_len + 1][C + 4]"""
    C, kv = heads * 64, kv1 + kv2
    q, k, v = attn_operands(batch, heads, q_len, kv, seed, scale)
    rows = max(q_len, kv1)
    buf = nans(batch, rows + 1, 3 * C + 4)
    qv, k1v, v1v = buf[:, :q_len, :C], buf[:, :kv1, C:2 * C], buf[:, :kv1, 2 * C:3 * C]
    qv.copy_(q)
    k1v.copy_(k[:, :kv1])
    v1v.copy_(v[:, :kv1])
    k2v = v2v = None
    if kv2:
        buf2 = nans(batch, kv2 + 1, 2 * C + 8)
        k2v, v2v = buf2[:, :kv2, :C], buf2[:, :kv2, C:2 * C]
        k2v.copy_(k[:, kv1:])
        v2v.copy_(v[:, kv1:])
    ob = nans(batch, q_len + 1, C + 4)
    ov = ob[:, :q_len, :C]
    k_attn(lib, qv, k1v, v1v, k2v, v2v, ov, scale)
    what = f"batch {batch} heads {heads} q_len {q_len} kv {kv1} + {kv2}"
    assert untouched(ob, ov), f"{what}: stored outside the result"
    ref, bound, (sm, m) = attn_ref(q, k, v, scale)
    if kv > 1:
        gap = (m - sm)[:, :, 0, :kv - 1]
        assert float(gap.min()) > 70.0 and float(gap.max()) < 95.0, f"{what}: the leading key of query 0 leads by {float(gap.min()):.1f} .. {float(gap.max()):.1f}"
        if q_len > 1:
            assert float((m - sm)[:, :, q_len - 1].abs().max()) == 0.0
    return ov, ref, bound, what


@pytest.mark.parametrize("q_len", ATTN_QLEN)
def test_attn_f32(lib, q_len):
    """one query, one short of / at / one past the 32 queries of a workgroup, three workgroups; keys: one, around the 64-key group, the last
    resident count 352 and the first chunked one 353, two chunks exactly, one key past them, 664 = the last the 156 KB of LDS admit; two
    segments split inside a group, at the chunk edge, across it, at the resident kernel's limit, at 664; heads 1 / 3 and batch 1 / 2"""
    iq = ATTN_QLEN.index(q_len)
    for i, kv1 in enumerate(ATTN_KV1):
        heads, batch = ATTN_HB[(i + iq) % 4]
        o, ref, bound, what = run_attn(lib, batch, heads, q_len, kv1, 0, seed=100 * q_len + i)
        check(o, ref, bound, what, key="attn_f32_long" if kv1 > 352 else "attn_f32")
    for i, (kv1, kv2) in enumerate(ATTN_KV2):
        heads, batch = ATTN_HB[(i + iq + 1) % 4]
        o, ref, bound, what = run_attn(lib, batch, heads, q_len, kv1, kv2, seed=100 * q_len + 50 + i)
        check(o, ref, bound, what, key="attn_f32_long" if kv1 + kv2 > 352 else "attn_f32")


# ================================================================================================ 3. deer_xattn_f32
def k_xattn(lib, slab, stride, k, v, tt, npm, out, T, heads, scale, ctl):
    """slab [s_in, batch * T, inner], k / v [batch * n_kv, inner] (column slices of one buffer), out [batch * T, inner]: views"""
    s_in, rows, _ = slab.shape
    batch = rows // T
    n_kv = k.shape[0] // batch
    inner = (v.data_ptr() - k.data_ptr()) // 4
    abi.check(lib.deer_xattn_f32(abi.ptr(slab), s_in, stride, slab.stride(1), abi.ptr(k), k.stride(0), inner, abi.ptr(tt), npm, abi.ptr(out), out.stride(0), T,
                                 n_kv, heads, batch, scale, abi.ptr(ctl), st()), "xattn_f32")
    sync()


def xattn_ref(slab, k, v, tt, npm, T, heads, scale):
    """fp64 gated cross attention (media-time mask; a row past the last media sees every key at -FLT_MAX: uniform; text_time 0: exactly 0).
    q = the exact slab sum (grid operands) * scale, rounded once; 64 sequential multiply-adds: es = ACC scale sum |q k|"""
    rows = slab.shape[1]
    batch = rows // T
    n_kv = k.shape[0] // batch
    hs = lambda t, n: t.double().reshape(batch, n, heads, 64).transpose(1, 2)
    q, kk, vv = hs(slab.double().sum(0), T), hs(k, n_kv), hs(v, n_kv)
    s = scale * (q @ kk.transpose(-1, -2))
    es = ACC * scale * (q.abs() @ kk.abs().transpose(-1, -2))
    j = torch.arange(n_kv, device=slab.device).view(1, 1, 1, n_kv)
    t = tt.view(batch, 1, T, 1).long()
    vis = (t == j // npm + 1).expand(batch, heads, T, n_kv)
    none = ~vis.any(-1, keepdim=True)
    s, es, vis = s.masked_fill(none, 0.0), es.masked_fill(none, 0.0), vis | none
    o, eo, _ = softmax_ref(s, es, vis, vv, n_kv)
    zero = (tt == 0).view(batch, 1, T, 1)
    o, eo = o.masked_fill(zero, 0.0), eo.masked_fill(zero, FLOOR)
    back = lambda x: x.transpose(1, 2).reshape(rows, heads * 64)
    uniform = vv.mean(-2, keepdim=True).expand(batch, heads, T, 64)
    return back(o), back(eo), back(uniform)


XATTN_T, XATTN_KV = [1, 5, 32], [1, 64, 65, 128]
XATTN_HBS = [(1, 1, 1), (8, 3, 3), (8, 1, 3), (1, 3, 1), (8, 3, 1), (1, 1, 3), (8, 1, 1), (1, 3, 3)]          # heads, batch, s_in


def xattn_text_time(batch, T, n_media, shift):
    """per row, cycling: a valid media, 0 (before the first media), the last media, one past the last, two past it"""
    pat = [1, 0, n_media, n_media + 1, min(2, n_media), n_media + 2, 1]
    return torch.tensor([pat[(r + shift) % len(pat)] for r in range(batch * T)], dtype=torch.int32, device=DEV)


def run_xattn(lib, T, n_kv, npm, heads, batch, s_in, seed, ctl=None, scale=0.125):
    """q slabs [s_in][batch T + 1][inner + 4] (a NaN row between the slabs, four NaN columns); K / V of layer 1 of 3 inside a
    [batch n_kv + 1][3 * 2 * inner] buffer; out [batch T + 1][inner + 4]"""
    inner, rows = heads * 64, batch * T
    sb = nans(s_in, rows + 1, inner + 4)
    slab = sb[:, :rows, :inner]
    slab.copy_(on_grid(randn(s_in, rows, inner, seed=seed, scale=s_in ** -0.5)))
    kvb = nans(batch * n_kv + 1, 6 * inner)
    k, v = kvb[:batch * n_kv, 2 * inner:3 * inner], kvb[:batch * n_kv, 3 * inner:4 * inner]
    k.copy_(randn(batch * n_kv, inner, seed=seed + 1))
    v.copy_(randn(batch * n_kv, inner, seed=seed + 2))
    n_media = (n_kv + npm - 1) // npm
    tt = xattn_text_time(batch, T, n_media, seed)
    ob = nans(rows + 1, inner + 4)
    out = ob[:rows, :inner]
    k_xattn(lib, slab, (rows + 1) * (inner + 4), k, v, tt, npm, out, T, heads, scale, ctl)
    return ob, out, slab, k, v, tt


@pytest.mark.parametrize("T", XATTN_T)
def test_xattn_f32(lib, T):
    """key counts 1, one media of 64, 65 (a second media of one key), 128; one key per media, 64, one media over all keys; heads 1 / 8,
    batch 1 / 3, one and three q slabs; every launch holds rows before the first media (exactly 0.0), on a valid media, and past the last
    media (the uniform average of V)"""
    n, past_rows = 0, 0
    for n_kv in XATTN_KV:
        for npm in sorted({1, 64, n_kv}):
            heads, batch, s_in = XATTN_HBS[(n + XATTN_T.index(T)) % 8]
            n += 1
            what = f"T {T} n_kv {n_kv} n_per_media {npm} heads {heads} batch {batch} s_in {s_in}"
            ob, out, slab, k, v, tt = run_xattn(lib, T, n_kv, npm, heads, batch, s_in, seed=1000 * T + 10 * n)
            assert untouched(ob, out), f"{what}: stored outside the result"
            ref, bound, uniform = xattn_ref(slab, k, v, tt, npm, T, heads, 0.125)
            check(out, ref, bound, what, key="xattn_f32")
            assert bool((out[tt == 0] == 0).all()), f"{what}: a text_time 0 row is not exactly 0"
            past = tt > (n_kv + npm - 1) // npm
            past_rows += int(past.sum())
            if bool(past.any()):
                check(out[past], uniform[past], bound[past], f"{what}: rows past the last media against the mean of V")
    assert T == 1 or past_rows > 0


def test_xattn_f32_exit_flag(lib):
    ob, out, *_ = run_xattn(lib, 5, 65, 64, 8, 3, 3, seed=7, ctl=ctl_block(True))
    assert all_nan(ob), "ALL_EXITED: something was written"
    ob, out, *_ = run_xattn(lib, 5, 65, 64, 8, 3, 3, seed=7, ctl=ctl_block(False))
    assert untouched(ob, out) and bool(torch.isfinite(out).all())


# ================================================================================================ 4. deer_gemm_skinny, one launch per weight plane
_PACKED = {}


def pack(lib, W):
    """deer_pack_weight_mfma16 of a 16-bit [N, K] plane (kept per tensor: the same planes serve every M)"""
    key = (W.data_ptr(), tuple(W.shape))
    if key not in _PACKED:
        Wp = torch.empty_like(W)
        abi.check(lib.deer_pack_weight_mfma16(abi.ptr(W), abi.ptr(Wp), W.shape[0], W.shape[1], st()), "pack")
        _PACKED[key] = (Wp, W)                                    # (W itself kept alive: the key is its address)
    return _PACKED[key][0]


def k_skinny(lib, fmt, mode, A, slab, stride, planes, part, M, N, K, S, ctl):
    """model.hip::skinny: one launch per weight plane, plane p into slabs p S .. p S + S - 1 of `part` [len(planes) S + 1][mpad][N].
    A: [M, K] view (row stride = lda) or None; slab: [s_in, M, K] view with row stride K, or None"""
    f = lib.deer_gemm_skinny_f16 if fmt == "f16" else lib.deer_gemm_skinny
    mpad = abi.skinny_mpad(M)
    for p, W in enumerate(planes):
        abi.check(f(abi.ptr(A), A.stride(0) if A is not None else 0, abi.ptr(slab), slab.shape[0] if slab is not None else 0, stride, mode, abi.ptr(pack(lib, W)),
                    abi.ptr(part, p * S * mpad * N * 4), M, N, K, S, abi.ptr(ctl), st()), "gemm_skinny")
    sync()


def gelu_bound(x, y, e32):
    """0.5 x (1 + erff(x / sqrt 2)) in f32 of a value carrying error e32 (tests/test_trunk_kernels.py::gelu_bound): slope <= 1.13; erff ~2 ulp
    of a value <= 1, i.e. absolute 2^-22 before the product with x / 2; the products ~1 ulp each (2^-21 |y|)"""
    return 1.13 * e32 + x.abs() * 2.0 ** -22 + y.abs() * 2.0 ** -21


def weight_planes(N, K, seed):
    """W f32 and the planes the loader makes of it (csrc/model.hip::ingest_pack_kernel): hi = bf16(w), lo = bf16(w - hi); and fp16(w)"""
    key = ("W", N, K, seed, DEV)
    if key not in _PACKED:
        W = randn(N, K, seed=seed, scale=K ** -0.5)
        hi = W.bfloat16()
        _PACKED[key] = (W, hi, (W - hi.float()).bfloat16(), W.half())
    return _PACKED[key]


def skinny_activation(mode, fmt, M, K, s_in, seed):
    """the operand as the kernel reads it and the fp64 value a of the product with its error ea (0 unless a GELU stands before the product):
    A_F32: [M, K] inside [M + 1][K + 8]; A_BF16: the same in 16 bits; A_SLABS(_GELU): [s_in][M + 1][K] with row stride K, one NaN row
    between the slabs, grid values (exact f32 sum)"""
    if mode in (A_F32, A_BF16):
        buf = nans(M + 1, K + 8, dtype=torch.float32 if mode == A_F32 else TDT[fmt])
        A = buf[:M, :K]
        A.copy_(randn(M, K, seed=seed))
        return A, None, 0, A.double(), None
    buf = nans(s_in, M + 1, K)
    slab = buf[:, :M]
    slab.copy_(on_grid(randn(s_in, M, K, seed=seed, scale=s_in ** -0.5)))
    a = slab.double().sum(0)
    if mode == A_SLABS_GELU:
        y = gelu64(a)
        return None, slab, (M + 1) * K, y, gelu_bound(a, y, 0.0)
    return None, slab, (M + 1) * K, a, None


def run_skinny(lib, fmt, mode, M, N, K, S, planes, W_ref, per_unit, seed, s_in=1, ctl=None):
    """the slab sum against a W_ref^T in fp64 with per_unit * S (+ the GELU's error through |W|); padded rows zero, the slab behind the last NaN"""
    A, slab, stride, a, ea = skinny_activation(mode, fmt, M, K, s_in, seed)
    mpad, P = abi.skinny_mpad(M), len(planes)
    part = nans(P * S + 1, mpad, N)
    k_skinny(lib, fmt, mode, A, slab, stride, planes, part, M, N, K, S, ctl)
    W64 = W_ref.double()
    ref, Sm = a @ W64.t(), a.abs() @ W64.abs().t()
    bound = per_unit * Sm + FLOOR
    if fmt == "f16" and mode != A_BF16:
        bound = bound + TINY[fmt] * W64.abs().sum(-1)             # the subnormal floor of the activation's fp16 lo plane
    if ea is not None:
        bound = bound + ea @ W64.abs().t()
    return part, ref, bound


SK_M = [1, 16, 17, 33, 49, 65, 81, 97, 113, 128]
SK_N, SK_K = [16, 48, 80, 272], [32, 96, 160, 288, 512]
SK_FORCED = {96: 3, 160: 5, 288: 3, 512: 1}          # K / splitk = 32, 32, 96 (under one chunk), 512 (two chunks of 256 / four of 128)
SK_MODES = [(A_SLABS, 1), (A_SLABS_GELU, 1), (A_BF16, 1), (A_SLABS_GELU, 3), (A_SLABS, 3)]


def check_skinny(part, ref, bound, M, S, P, what, key):
    assert all_nan(part[P * S]), f"{what}: stored past the last slab"
    assert bool((part[:P * S, M:] == 0).all()), f"{what}: padded rows are not zero"
    check(part[:P * S, :M].double().sum(0), ref, bound, what, key=key)


@pytest.mark.parametrize("M", SK_M)
def test_gemm_skinny_two_planes(lib, M):
    """every row-tile count 1 .. 8 (M = 16 MT and one past it), 4-wave (M <= 16) and 16-wave workgroups against N of one tile, less than a
    workgroup, 272 = 256 + 16; K of one fragment, under one chunk (256 columns up to 64 rows, 128 above), 288 = whole chunks + 32, 512; the
    split-K of deer_skinny_splitk and a forced one.  Per (N, K): DEER_A_F32 on the hi and lo planes against fp64 on the f32 W with
    (ACC + 2 PAIR) S; one more mode by turns (slabs, slabs through GELU with one and three slabs, bf16 rows on the hi plane alone with
    ACC S); and deer_gemm_skinny_f16 on the one fp16 plane of W with (ACC + PAIR) S"""
    im, n = SK_M.index(M), 0
    two = ACC + 2 * PAIR["bf16"]
    for i_n, N in enumerate(SK_N):
        for ik, K in enumerate(SK_K):
            n += 1
            W, hi, lo, W16 = weight_planes(N, K, seed=7 * N + K)
            for S in sorted({lib_splitk(lib, M, N, K), SK_FORCED.get(K, 1)}):
                what = f"M {M} N {N} K {K} splitk {S}"
                part, ref, bound = run_skinny(lib, "bf16", A_F32, M, N, K, S, [hi, lo], W, two, seed=100 * M + n)
                check_skinny(part, ref, bound, M, S, 2, f"{what} A_F32, hi + lo planes", "skinny_2plane_f32")
                mode, s_in = SK_MODES[(im + i_n + ik + S) % len(SK_MODES)]
                if mode == A_BF16:
                    part, ref, bound = run_skinny(lib, "bf16", mode, M, N, K, S, [hi], hi, ACC, seed=100 * M + n + 50)
                    check_skinny(part, ref, bound, M, S, 1, f"{what} A_BF16, hi plane", "skinny_bf16_rows")
                else:
                    part, ref, bound = run_skinny(lib, "bf16", mode, M, N, K, S, [hi, lo], W, two, seed=100 * M + n + 50, s_in=s_in)
                    check_skinny(part, ref, bound, M, S, 2, f"{what} mode {mode} s_in {s_in}, hi + lo planes", "skinny_2plane_gelu" if mode == A_SLABS_GELU else "skinny_2plane_slabs")
                mode16 = [A_F32, A_SLABS_GELU, A_BF16, A_SLABS][(im + i_n + ik) % 4]
                per = ACC if mode16 == A_BF16 else ACC + PAIR["f16"]
                part, ref, bound = run_skinny(lib, "f16", mode16, M, N, K, S, [W16], W16, per, seed=100 * M + n + 70, s_in=3)
                check_skinny(part, ref, bound, M, S, 1, f"{what} fp16 plane, mode {mode16}", "skinny_f16")


def lib_splitk(lib, M, N, K):
    return abi.lib().deer_skinny_splitk(M, N, K)          # a host function (no launch)


def test_gemm_skinny_exit_flag(lib):
    W, hi, lo, _ = weight_planes(48, 96, seed=7 * 48 + 96)
    A, _, _, _, _ = skinny_activation(A_F32, "bf16", 17, 96, 1, seed=3)
    part = nans(3, 32, 48)
    k_skinny(lib, "bf16", A_F32, A, None, 0, [hi, lo], part, 17, 48, 96, 1, ctl_block(True))
    assert all_nan(part), "ALL_EXITED: something was written"


# ================================================================================================ 5. deer_mpt_attn_small, f32 output
def k_mpt(lib, slab, stride, d, H, gq, gk, mask, bias_max, out, T, ctl):
    """slab [s_in, batch * T, 3 d] (rows contiguous), out [batch * T, d] view (row stride = ldo), mask [batch, T] uint8 or None"""
    s_in, rows, _ = slab.shape
    ws = nans(rows, 3 * d)
    abi.check(lib.deer_mpt_attn_small(abi.ptr(slab), s_in, stride, d, H, abi.ptr(gq), abi.ptr(gk), 1e-5, abi.ptr(mask), bias_max, abi.ptr(ws), abi.ptr(out), 1,
                                      out.stride(0), T, rows // T, abi.ptr(ctl), st()), "mpt_attn_small")
    sync()


def k_mpt_hl(lib, slab, stride, d, H, gq, gk, mask, bias_max, hi, lo, T):
    s_in, rows, _ = slab.shape
    ws = nans(rows, 3 * d)
    abi.check(lib.deer_mpt_attn_small_hl(abi.ptr(slab), s_in, stride, d, H, abi.ptr(gq), abi.ptr(gk), 1e-5, abi.ptr(mask), bias_max, abi.ptr(ws), abi.ptr(hi),
                                         abi.ptr(lo), hi.stride(0), T, rows // T, None, st()), "mpt_attn_small_hl")
    sync()


def ln_ref(x, gamma, beta, eps=1e-5):
    """fp64 LayerNorm of the rows of x and the bound of the kernels' f32 two-pass arithmetic (tests/test_trunk_kernels.py::ln_ref):
    mean: |dmu| <= 32 2^-24 mean|x|, which enters every output as gamma dmu rstd; rstd: the centred squares, their sum and rsqrtf: relative
    2^-18, plus (dmu rstd)^2; the two products with rstd and gamma and the beta add: 2^-23 (|y| + |beta|)"""
    x = x.double()
    g = gamma.double()
    b = beta.double() if beta is not None else torch.zeros_like(g)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * rstd
    y = xh * g + b
    dmu = 32 * 2.0 ** -24 * x.abs().mean(-1, keepdim=True) * rstd
    bound = g.abs() * (dmu + xh.abs() * (2.0 ** -18 + dmu ** 2)) + 2.0 ** -23 * (y.abs() + b.abs()) + 2.0 ** -140
    return y, bound


def mpt_ref(qkv, d, H, gq, gk, mask, bias_max, T):
    """tests/test_env_batch_ops.py::_mpt_attn_ref in fp64 with its bound (tests/test_trunk_kernels.py::mpt_ref): MPT attention of ONE
    environment on q|k|v [T, 3d] (the exact slab sum): q / k LayerNorm over the full row, score = q k / sqrt(hd) - (T - 1 - j) 2^(-bias_max
    (h + 1) / H), causal, key mask (key 0 visible: every row sees a key).
    q^, k^: the LayerNorm bound per element (eq, ek);
    score:  es = sc (eq |k^| + |q^| ek + eq ek summed over the head) + ACC sc sum|q^ k^| (hd sequential multiply-adds) + 2^-23 |s| (rsqrtf of
            hd, the scale) + 2^-21 alibi (exp2f of the slope, its product, the subtraction);
    softmax and P V as softmax_ref (<= 32 keys), the sum (T + 2) 2^-24 sum_j p_j |v_j| inside its ACC"""
    hd = d // H
    q, k, v = qkv.double().chunk(3, -1)
    eq = ek = torch.zeros_like(q)
    if gq is not None:
        q, eq = ln_ref(q, gq, None)
        k, ek = ln_ref(k, gk, None)
    hs = lambda t: t.reshape(T, H, hd).transpose(0, 1)
    q, k, v, eq, ek = hs(q), hs(k), hs(v), hs(eq), hs(ek)
    sc = hd ** -0.5
    kt, akt = k.transpose(-1, -2), k.abs().transpose(-1, -2)
    slopes = 2.0 ** (-bias_max * torch.arange(1, H + 1, device=qkv.device, dtype=torch.float64) / H)
    alibi = (T - 1 - torch.arange(T, device=qkv.device, dtype=torch.float64)).view(1, 1, T) * slopes.view(H, 1, 1)
    s = (q @ kt) * sc - alibi
    es = sc * (eq @ akt + q.abs() @ ek.transpose(-1, -2) + eq @ ek.transpose(-1, -2)) + ACC * sc * (q.abs() @ akt) + 2.0 ** -23 * s.abs() + 2.0 ** -21 * alibi
    vis = torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril()
    if mask is not None:
        vis = vis & mask.bool().view(1, T)
    assert bool(vis.any(-1).all())
    o, eo, _ = softmax_ref(s, es, vis.expand(H, T, T), v, T)
    back = lambda t: t.transpose(0, 1).reshape(T, d)
    return back(o), back(eo)


MPT_T = [1, 2, 16, 17, 32]
MPT_CFG = [(64, 2), (256, 2), (96, 8), (2048, 16)]         # head widths 32, 128, 12, 128


def mpt_masks(batch, T, kind):
    """[batch, T] uint8, every environment its own: right padding of (b + 1) keys, or holes (every (b + 2)-th key from key 1 + b % 2 on); key 0 stays"""
    if kind == "none":
        return None
    m = torch.ones(batch, T, dtype=torch.uint8, device=DEV)
    for b in range(batch):
        if kind == "pad":
            m[b, max(1, T - 1 - b):] = 0
        else:
            m[b, 1 + b % 2::b + 2] = 0
    m[:, 0] = 1
    return m


def run_mpt(lib, T, d, H, qk_ln, kind, batch, s_in, seed, ctl=None, bias_max=8.0):
    """slabs [s_in][batch T + 1][3 d] (a NaN row between the slabs), out [batch T + 1][d + 4]"""
    rows = batch * T
    sb = nans(s_in, rows + 1, 3 * d)
    slab = sb[:, :rows]
    slab.copy_(on_grid(randn(s_in, rows, 3 * d, seed=seed, scale=1.5 * s_in ** -0.5) + 0.3 / s_in))
    gq, gk = (1.0 + randn(d, seed=seed + 1, scale=0.1), 1.0 + randn(d, seed=seed + 2, scale=0.1)) if qk_ln else (None, None)
    mask = mpt_masks(batch, T, kind)
    ob = nans(rows + 1, d + 4)
    out = ob[:rows, :d]
    k_mpt(lib, slab, (rows + 1) * 3 * d, d, H, gq, gk, mask, bias_max, out, T, ctl)
    return ob, out, slab, gq, gk, mask


def mpt_reference(slab, d, H, gq, gk, mask, bias_max, T):
    qkv = slab.double().sum(0)
    batch = qkv.shape[0] // T
    res = [mpt_ref(qkv[b * T:(b + 1) * T], d, H, gq, gk, None if mask is None else mask[b], bias_max, T) for b in range(batch)]
    return torch.cat([r[0] for r in res]), torch.cat([r[1] for r in res])


@pytest.mark.parametrize("qk_ln", [True, False], ids=["qkln", "noln"])
@pytest.mark.parametrize("d,H", MPT_CFG, ids=[f"d{d}-H{H}" for d, H in MPT_CFG])
def test_mpt_attn_small_f32(lib, d, H, qk_ln):
    """T of one row, two, 16, 17 and the kernel's limit 32; no mask, right padding and holes, every environment its own; batch 1 / 3; one and
    three slabs; alibi_bias_max 8 and 16"""
    n = 0
    for T in MPT_T:
        for kind in ("none", "pad", "holes"):
            if T == 1 and kind != "none":
                continue
            n += 1
            batch, s_in, bias_max = (1, 3)[n % 2], (3, 1)[(n // 2) % 2], (8.0, 16.0)[(n // 3) % 2]
            what = f"d {d} H {H} T {T} {kind} batch {batch} s_in {s_in} bias_max {bias_max}"
            ob, out, slab, gq, gk, mask = run_mpt(lib, T, d, H, qk_ln, kind, batch, s_in, seed=1000 * T + d + n, bias_max=bias_max)
            assert untouched(ob, out), f"{what}: stored outside the result"
            ref, bound = mpt_reference(slab, d, H, gq, gk, mask, bias_max, T)
            check(out, ref, bound, what, key=f"mpt_attn_small/{'qkln' if qk_ln else 'noln'}")


def test_mpt_attn_small_exit_flag_and_planes(lib):
    """ALL_EXITED: nothing written.  deer_mpt_attn_small_hl on the same operands: hi + lo is the f32 output up to the pair residue"""
    T, d, H = 17, 256, 2
    ob, out, *_ = run_mpt(lib, T, d, H, True, "pad", 3, 3, seed=5, ctl=ctl_block(True))
    assert all_nan(ob), "ALL_EXITED: something was written"
    ob, out, slab, gq, gk, mask = run_mpt(lib, T, d, H, True, "pad", 3, 3, seed=5)
    hb, lb = nans(3 * T + 1, d + 8, dtype=torch.bfloat16), nans(3 * T + 1, d + 8, dtype=torch.bfloat16)
    hi, lo = hb[:3 * T, :d], lb[:3 * T, :d]
    k_mpt_hl(lib, slab, (3 * T + 1) * 3 * d, d, H, gq, gk, mask, 8.0, hi, lo, T)
    assert untouched(hb, hi) and untouched(lb, lo)
    check(hi.double() + lo.double(), out.double(), PAIR["bf16"] * out.double().abs() + TINY["bf16"], "hi + lo planes against the f32 output", key="mpt_attn_small/planes")


# ================================================================================================ 6. deer_resadd_ln with out_f32
def k_resadd(lib, x, slab, stride, gate, gamma, beta, y32, xc, ctl):
    """x [T, d] contiguous, updated in place; slab [s_in, T, d] view or None; y32 / xc [T, d] contiguous or None"""
    T, d = x.shape
    abi.check(lib.deer_resadd_ln(abi.ptr(x), abi.ptr(slab), slab.shape[0] if slab is not None else 0, stride, abi.ptr(gate), None, abi.ptr(gamma), abi.ptr(beta),
                                 None, abi.ptr(y32), abi.ptr(xc), T, d, 1e-5, abi.ptr(ctl), st()), "resadd_ln")
    sync()


# what model.hip::llm_layer's non-plane form asks of it: (slabs, gate, LayerNorm, beta, x_copy)
RESADD_USES = [("first layer: LayerNorm of x alone", 0, False, True, True, False),
               ("pending down-projection + hidden-state copy", 4, False, True, False, True),
               ("x-attn slabs under tanh(attn_gate)", 2, True, True, True, False),
               ("ff slabs under tanh(ff_gate), no beta", 8, True, True, False, False),
               ("out-projection slabs", 2, False, True, True, False),
               ("finalize: slabs + copy, no LayerNorm", 16, False, False, False, True)]


@pytest.mark.parametrize("d", [96, 256, 2048])
def test_resadd_ln_out_f32(lib, d):
    """T = 1, 14, 33 rows: the residual per element against fp64, the f32 LayerNorm of the kernel's own new x per element, x_copy its bits;
    the row behind the last untouched (tests/test_frame_kernels.py gates out_f32 at one row with a bias; the trunk's calls pass a gate, an
    x_copy and up to 16 slabs)"""
    gate = torch.tensor([0.3], device=DEV)
    gamma, beta = 1.0 + randn(d, seed=10, scale=0.1), randn(d, seed=11, scale=0.1)
    for T in (1, 14, 33):
        for i, (name, s_in, gated, ln, has_beta, copy) in enumerate(RESADD_USES):
            what = f"d {d} T {T} {name}"
            x0 = randn(T, d, seed=100 * T + i)
            xb, yb, cb = nans(T + 1, d), nans(T + 1, d), nans(T + 1, d)
            xb[:T] = x0
            slab, stride = None, 0
            if s_in:
                sbuf = nans(s_in, T + 1, d)
                slab, stride = sbuf[:, :T], (T + 1) * d
                slab.copy_(randn(s_in, T, d, seed=100 * T + i + 1, scale=0.2))
            k_resadd(lib, xb[:T], slab, stride, gate if gated else None, gamma if ln else None, beta if (ln and has_beta) else None, yb[:T] if ln else None,
                     cb[:T] if copy else None, None)
            assert all_nan(xb[T:]) and all_nan(yb[T:] if ln else yb) and all_nan(cb[T:] if copy else cb), f"{what}: stored past row T / into an absent output"
            if s_in:
                # x += tanh(gate) sum_s slab[s]: s_in - 1 f32 adds (each <= 2^-24 of sum |slab|), the product, the add; tanhf a few ulp
                t = math.tanh(0.3) if gated else 1.0
                sl = slab.double()
                mag = x0.double().abs() + t * sl.abs().sum(0)
                check(xb[:T], x0.double() + t * sl.sum(0), (s_in + 4) * 2.0 ** -24 * mag + 2.0 ** -21 * t * sl.abs().sum(0) + 1e-30, f"{what}: residual", key="resadd_x")
            else:
                assert torch.equal(xb[:T], x0)
            if copy:
                assert torch.equal(cb[:T], xb[:T]), f"{what}: x_copy"
            if ln:
                y, e = ln_ref(xb[:T], gamma, beta if has_beta else None)
                check(yb[:T], y, e, f"{what}: LayerNorm f32", key="resadd_ln_f32")


# ================================================================================================ 7. the gates bite
def _shifted(out, bound, idx):
    bad = out.double().clone()
    bad[idx] += 2 * bound[idx]
    return bad


def test_gates_reject_perturbed_results(lib):
    """negative controls, one per family: the kernel's own result with ONE element moved by twice its bound must fail check(); the two-plane
    product against the reference of a product that dropped the lo plane (fp64 on bf16(W)) must fail"""
    C, ref, bound, _ = run_gemm(lib, 65, 68, 100, PE_QGELU, True, 4, True, seed=1)
    check(C, ref, bound, "unperturbed GEMM")
    with pytest.raises(AssertionError):
        check(_shifted(C, bound, (64, 67)), ref, bound, "GEMM element moved by 2 bounds")
    o, ref, bound, _ = run_attn(lib, 2, 3, 33, 300, 271, seed=2)
    check(o, ref, bound, "unperturbed attention")
    with pytest.raises(AssertionError):
        check(_shifted(o, bound, (1, 32, 191)), ref, bound, "attention element moved by 2 bounds")
    ob, out, slab, k, v, tt = run_xattn(lib, 5, 65, 64, 8, 3, 3, seed=3)
    ref, bound, _ = xattn_ref(slab, k, v, tt, 64, 5, 8, 0.125)
    check(out, ref, bound, "unperturbed x-attn")
    with pytest.raises(AssertionError):
        check(_shifted(out, bound, (14, 511)), ref, bound, "x-attn element moved by 2 bounds")
    with pytest.raises(AssertionError):
        check(out, xattn_ref(slab, k, v, torch.where(tt == 1, 2, tt).int(), 64, 5, 8, 0.125)[0], bound, "media 1 rows read media 2")
    M, N, K = 33, 80, 160
    W, hi, lo, _ = weight_planes(N, K, seed=7 * N + K)
    part, ref, bound = run_skinny(lib, "bf16", A_F32, M, N, K, 1, [hi, lo], W, ACC + 2 * PAIR["bf16"], seed=4)
    y = part[:2, :M].double().sum(0)
    check(y, ref, bound, "unperturbed two-plane product")
    with pytest.raises(AssertionError):
        check(_shifted(y, bound, (32, 79)), ref, bound, "product element moved by 2 bounds")
    A = skinny_activation(A_F32, "bf16", M, K, 1, seed=4)[3]
    with pytest.raises(AssertionError):
        check(y, A @ hi.double().t(), bound, "reference with the lo plane dropped")
    with pytest.raises(AssertionError):
        check(part[:1, :M].double().sum(0), ref, bound, "the lo plane's slab missing")
    ob, out, slab, gq, gk, mask = run_mpt(lib, 17, 256, 2, True, "holes", 3, 3, seed=5)
    ref, bound = mpt_reference(slab, 256, 2, gq, gk, mask, 8.0, 17)
    check(out, ref, bound, "unperturbed MPT attention")
    with pytest.raises(AssertionError):
        check(_shifted(out, bound, (50, 255)), ref, bound, "MPT attention element moved by 2 bounds")
    with pytest.raises(AssertionError):
        check(out, mpt_reference(slab, 256, 2, gq, gk, mask, 8.0 / 2, 17)[0], bound, "wrong ALiBi slopes")
    x = randn(14, 256, seed=6)
    gamma = 1.0 + randn(256, seed=7, scale=0.1)
    y32 = nans(14, 256)
    k_resadd(lib, x, None, 0, None, gamma, None, y32, None, None)
    y, e = ln_ref(x, gamma, None)
    check(y32, y, e, "unperturbed LayerNorm")
    with pytest.raises(AssertionError):
        check(_shifted(y32, e, (13, 0)), y, e, "LayerNorm element moved by 2 bounds")
