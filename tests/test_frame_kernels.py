"""The frame path - ViT-L/14 tower, Perceiver resampler, media K/V projection - one kernel at a time through the C ABI, against float64
references computed on the device and gated ELEMENT BY ELEMENT (tests/test_hip_ops.py gates the same kernels with one norm ratio per tensor).

Inputs are drawn on the device from fixed seeds and rounded to the operand format, so the fp64 reference sees exactly the kernel's operands.
Every gate is relative to the magnitude that bounds the error of its element, not to |out|:
  ACC     f32 accumulation (MFMA chains, split-K slabs, the P V product): |err| <= ACC * S, S = sum_k |a_k w_k| (+ |bias|).  ACC = 4e-6: the
          class gate of tests/test_head_kernels.py; an f32 MFMA chain measures 1e-7 .. 3.5e-7 S on gfx950 for K <= 4096.
  16-bit  one round to nearest even of an f32 value carrying error e32: |out - ref| <= U |ref| + (1 + U) e32 + TINY, U = half an ulp (2^-8
          bf16, 2^-11 fp16), TINY = half the subnormal step (fp16 2^-25).  +-inf only where |ref| + e32 reaches the overflow threshold
          (fp16 65520), never NaN.  Where the same tile also has an f32 form with the same K order, the 16-bit result must be the RNE of that
          f32 result bit for bit (EXACT16).
  attention, LayerNorm, activations: the bounds are derived next to their reference functions below.
On failure the worst element is reported: index, value, reference, bound."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from deer_vla_amd import _abi as abi  # noqa: E402

ACC = 4e-6
# the f32 gate of test_frame_gemm_hard_operands: on fp16 operands with a 1000x channel in A and fp16-subnormal weights (columns scaled to
# 1e-3) v_mfma_f32_16x16x32_f16 measures up to 8.7e-6 S on gfx950 (1.6e-7 S on N(0, 1) operands, 1e-6 S on the same data in bf16)
ACC_HARD = {"bf16": ACC, "f16": 4 * ACC}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TINY = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25}
OVF = {"bf16": 2.0 ** 128 * (1 - 2.0 ** -9), "f16": 65520.0}     # the smallest magnitude that rounds to inf
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
ATTN = {"bf16": "mfma", "f16": "f16"}
FMTS = ["bf16", "f16"]
NAN = float("nan")
RATIOS = {}                                  # family / format -> largest measured error / bound


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    torch.cuda.synchronize()


def randn(*shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda") * scale


def uniform(n, seed):
    return torch.rand(n, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda")


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device="cuda", dtype=dtype)


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


@pytest.fixture(scope="module")
def lib():
    l = abi.lib()
    assert l.deer_hip_arch() == b"gfx950"
    yield l
    print("\nlargest error / bound per family: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(RATIOS.items())))


def check(out, ref, bound, what, key=None):
    """|out - ref| <= bound element by element (float64 on the device); a NaN / inf output where the reference is finite fails"""
    out = out.double()
    r = torch.nan_to_num((out - ref).abs() / bound, nan=math.inf, posinf=math.inf)
    worst = int(r.argmax())
    rmax = float(r.reshape(-1)[worst])
    idx = tuple(int(i) for i in np.unravel_index(worst, tuple(r.shape)))
    assert rmax <= 1.0, (f"{what}: worst element {idx}: out {float(out.reshape(-1)[worst])!r} ref {float(ref.reshape(-1)[worst])!r} "
                         f"bound {float(bound.reshape(-1)[worst]):.3g} (error / bound {rmax:.3g})")
    if key is not None:
        RATIOS[key] = max(RATIOS.get(key, 0.0), rmax)
    return rmax


def check16(out, ref, e32, fmt, what, key=None):
    """a 16-bit result of an f32 value with error <= e32 against the fp64 value: half an ulp + e32; +-inf only where ref may overflow"""
    o = out.double()
    may_ovf = (ref.abs() + e32 >= OVF[fmt]) & torch.isinf(o) & (torch.sign(o) == torch.sign(ref))
    o = torch.where(may_ovf, ref, o)                       # an allowed overflow counts as error 0
    return check(o, ref, U[fmt] * ref.abs() + (1 + U[fmt]) * e32 + TINY[fmt], what, key)


# ================================================================================================ 1. tower / Perceiver / media K/V GEMMs
def pick_split(M, N, K, target=320, max_split=8):
    """csrc/model.hip::pick_split (split-K factor of out_proj / c_proj / to_out / ff.3)"""
    blocks = -(-M // 64) * -(-N // 64)
    S = 1
    while S * 2 <= max_split and blocks * S * 2 <= target and K % (S * 2 * 64) == 0 and K // (S * 2) >= 128:
        S *= 2
    if S == 1 and M >= 2048 and K >= 4096 and K % 128 == 0:
        S = 2
    return S


def select_tile(M, N, K, batch, epi):
    """the tile gemm_dispatch picks for tile 0 (csrc/gemm_tiled.hip, default environment); every call below runs tile 0 AND this tile
    explicitly and requires identical bits, so the mirror is checked on the machine"""
    nblk = lambda bm, bn: -(-M // bm) * -(-N // bn) * batch
    if K % 64:
        return 2 if nblk(64, 128) >= 256 else 1
    if nblk(128, 128) >= 256:
        frames = M // 257 if M % 257 == 0 else 0

        def one_round(bn):
            if frames <= 0 or N % bn:
                return False
            w = frames * (N // bn) * batch
            return 192 <= w <= 256 or w == 512
        e16 = epi in (abi.EPI_BF16, abi.EPI_QGELU_BF16, abi.EPI_GELU_BF16, abi.EPI_BF16OUT)
        if K % 32 == 0 and e16 and one_round(192):
            return 64
        if K % 32 == 0 and e16 and one_round(256):
            return 63
        if K % 32 == 0 and epi == abi.EPI_F32 and one_round(128):
            return 67
        if N % 256 == 0 and K % 32 == 0 and 192 <= nblk(256, 256) <= 256:
            return 61
        if N <= 1024 and batch == 1:
            return 17
        cost = lambda bm, bn, rel: ((nblk(bm, bn) + 255) // 256) * rel
        tile, best = 17, cost(128, 128, 1.0)
        if cost(192, 128, 1.35) < best:
            tile, best = 39, cost(192, 128, 1.35)
        if cost(128, 192, 1.35) < best:
            tile = 45
        return tile
    if nblk(64, 64) > 512:
        return 8
    if nblk(64, 64) > 256:
        return 16
    return 4


SPLIT = -1                                   # the projection runs split-K into f32 slabs, closed by deer_resadd_ln
FRAMES = [1, 2, 8, 12, 16, 24, 32]
# (op, frames / environments, M, N, K, epilogue, weight batch, bias): the calls of csrc/model.hip vit_blocks / patch_embed / perceiver /
# media_kv at ViT-L/14 (width 1024, MLP 4096, 257 tokens), Perceiver (8 x 64 heads, 64 latents, ff x4, 6 layers), MPT-1B x-attn K|V of 12 layers
GEMM_CASES = []
for _n in FRAMES:
    _R, _L = 257 * _n, 64 * _n
    GEMM_CASES += [("vit_in_proj", _n, _R, 3072, 1024, abi.EPI_BF16, 1, True), ("vit_out_proj", _n, _R, 1024, 1024, SPLIT, 1, True),
                   ("vit_c_fc", _n, _R, 4096, 1024, abi.EPI_QGELU_BF16, 1, True), ("vit_c_proj", _n, _R, 1024, 4096, SPLIT, 1, True),
                   ("patch_embed", _n, 256 * _n, 1024, 640, abi.EPI_F32, 1, False),
                   ("perc_to_qkv", _n, _L, 1536, 1024, abi.EPI_BF16, 1, False), ("perc_to_kv", _n, 256 * _n, 1024, 1024, abi.EPI_BF16, 6, False),
                   ("perc_to_out", _n, _L, 1024, 512, SPLIT, 1, False), ("perc_ff1", _n, _L, 4096, 1024, abi.EPI_GELU_BF16, 1, False),
                   ("perc_ff2", _n, _L, 1024, 4096, SPLIT, 1, False)]
GEMM_CASES += [("media_kv", _b, 128 * _b, 12288, 1024, abi.EPI_BF16, 1, False) for _b in (1, 4, 16)]
GEMM_CASES += [("media_kv_bf16out", 16, 2048, 12288, 1024, abi.EPI_BF16OUT, 1, False)]
# tiles whose 16-bit epilogue is the RNE of their own f32 epilogue, bit for bit (same K order per output element in both forms)
EXACT16 = {4, 8, 16, 17, 39, 45, 61, 63, 64, 67}


def _tile_of(M, N, K, epi, batch):
    if epi == SPLIT:
        S = pick_split(M, N, K)
        return select_tile(M, N, K // S, S, abi.EPI_F32)
    return select_tile(M, N, K, batch, epi)


def test_selector_mirror_reaches_every_frame_tile():
    """the sweep below runs every tile the selector returns for the frame-path shapes"""
    tiles = {_tile_of(M, N, K, epi, b) for _, _, M, N, K, epi, b, _ in GEMM_CASES}
    assert tiles >= {4, 8, 16, 17, 39, 45, 61, 63, 64, 67}, sorted(tiles)


def _operands(fmt, batch, M, N, K, seed):
    A = randn(batch, M, K, seed=seed).to(TDT[fmt])
    W = (randn(batch, N, K, seed=seed + 1) * K ** -0.5).to(TDT[fmt])
    return A, W


def _ref(A, W, bias):
    """fp64 A W^T + b and S = |A| |W|^T + |b| of every output"""
    A64, W64 = A.double(), W.double()
    ref = A64 @ W64.transpose(-1, -2)
    S = A64.abs() @ W64.abs().transpose(-1, -2)
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    return ref, S


def _gemm(lib, fmt, A, W, bias, C, M, N, K, epi, tile, batch=1, ldc=None, gate=None, strideC=0):
    """one deer_gemm_{bf16,f16}_nt (batch 1) / _wbatch call; C [batch][rows][ldc]"""
    ldc = ldc or N
    if batch == 1:
        return getattr(lib, f"deer_gemm_{fmt}_nt")(abi.ptr(A), K, 0, abi.ptr(W), K, abi.ptr(bias), abi.ptr(C), ldc, 0, M, N, K, 1, epi,
                                                   abi.ptr(gate), tile, None, st())
    return getattr(lib, f"deer_gemm_{fmt}_nt_wbatch")(abi.ptr(A), K, M * K, abi.ptr(W), K, N * K, abi.ptr(bias), abi.ptr(C), ldc, strideC,
                                                       M, N, K, batch, epi, tile, None, st())


def qgelu_bound(x, y, e32, fmt):
    """x sigma(1.702 x) as quick_gelu_bf computes it (csrc/common.h: x * v_rcp(1 + v_exp(-2.4554669596 x))): the input error e32 times the
    slope (<= 1.1); v_exp / v_rcp / the product ~1 ulp each (2^-21 |y|); the rounding of the exp2 argument, relative 2^-24 of 2.455 |x|
    (1.2 |x| 2^-24 |y| after ln 2); should v_rcp flush results below 2^-126, a bf16 result may be 0 where |y| < |x| 2^-126 (2^-119 covers
    |x| < 128; beyond it the reference itself is below 2^-300)"""
    return 1.1 * e32 + y.abs() * (2.0 ** -21 + 1.2 * x.abs() * 2.0 ** -24) + (2.0 ** -119 if fmt == "bf16" else 0.0)


def gelu_bound(x, y, e32):
    """0.5 x (1 + erff(x / sqrt 2)) in f32: slope <= 1.13; erff is ~2 ulp of a value <= 1, i.e. absolute 2^-22 before the product with
    x / 2 (for x << 0 that is the whole result: 1 + erf cancels); the products ~1 ulp each (2^-21 |y|)"""
    return 1.13 * e32 + x.abs() * 2.0 ** -22 + y.abs() * 2.0 ** -21


def ln_ref(x, gamma, beta, eps=1e-5):
    """fp64 LayerNorm of the rows of x (the f32 values the kernel reads) and the bound of the kernels' f32 two-pass arithmetic:
    mean: a tree of <= 24 roundings over the row (4 values per thread, 6 wave levels, <= 16 waves, then / C) -> |dmu| <= 32 2^-24 mean|x|,
          which enters every output as gamma dmu rstd: the error that grows with |mu| / sigma;
    rstd: the centred squares, their sum and rsqrtf: relative 2^-18, plus (dmu rstd)^2 (the variance about the f32 mean);
    the two products with rstd and gamma and the beta add: 2^-23 (|y| + |beta|)"""
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


def _resadd(lib, fmt, x, slab, S, slab_stride, bias, gamma, beta, out16, out_f32, T, d):
    fn = lib.deer_resadd_ln_f16 if fmt == "f16" else lib.deer_resadd_ln
    abi.check(fn(abi.ptr(x), abi.ptr(slab), S, slab_stride, None, abi.ptr(bias), abi.ptr(gamma), abi.ptr(beta), abi.ptr(out16),
                 abi.ptr(out_f32), None, T, d, 1e-5, None, st()), "resadd_ln")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("op,n,M,N,K,epi,batch,has_bias", GEMM_CASES, ids=[f"{c[0]}-{c[1]}" for c in GEMM_CASES])
def test_frame_gemm(lib, fmt, op, n, M, N, K, epi, batch, has_bias):
    """every frame-path GEMM at 1 .. 32 frames (or 1 .. 16 environments): tile 0 and the tile it selects give the same bits; each output
    element within its f32 / 16-bit bound; nothing stored past row M or column N (C is NaN-filled with ldc = N + 16 and two extra rows);
    split-K slabs one by one, then deer_resadd_ln(_f16) closes them (slab sum + bias + residual, LayerNorm -> 16 bits) as the tower does"""
    tile = _tile_of(M, N, K, epi, batch)
    A, W = _operands(fmt, batch, M, N, K, seed=1000 * n + N + K)
    bias = randn(N, seed=7, scale=0.1) if has_bias else None
    if epi == SPLIT:
        S = pick_split(M, N, K)
        ks = K // S
        outs = []
        for t in (0, tile):
            slab = nans(S * M * N + 64)
            abi.check(getattr(lib, f"deer_gemm_{fmt}_nt_splitk")(abi.ptr(A), K, abi.ptr(W), K, abi.ptr(slab), M, N, K, S, t, None, st()), "splitk")
            sync()
            assert all_nan(slab[S * M * N:]), "stored past the last slab"
            outs.append(slab[:S * M * N].view(S, M, N))
        assert torch.equal(outs[0], outs[1]), f"tile 0 != tile {tile}"
        slabs = outs[0]
        ref_t = torch.zeros(M, N, dtype=torch.float64, device="cuda")
        S_t = torch.zeros(M, N, dtype=torch.float64, device="cuda")
        for s in range(S):
            r, Sm = _ref(A[0, :, s * ks:(s + 1) * ks], W[0, :, s * ks:(s + 1) * ks], None)
            check(slabs[s], r, ACC * Sm + 1e-30, f"{op} slab {s}/{S} tile {tile}", key=f"gemm_f32/{fmt}")
            ref_t += r
            S_t += Sm
        # the consumer: x += sum_s slab[s] + bias, then LayerNorm -> 16 bits (as the tower runs it: no f32 LayerNorm output, so from 2048
        # rows on the multi-row kernel)
        x0 = randn(M, N, seed=8)
        bias2 = bias if bias is not None else randn(N, seed=9, scale=0.1)
        gamma, beta = 1.0 + randn(N, seed=10, scale=0.1), randn(N, seed=11, scale=0.1)
        x = x0.clone()
        out16 = nans(M + 2, N, dtype=TDT[fmt])
        _resadd(lib, fmt, x, slabs, S, M * N, bias2, gamma, beta, out16, None, M, N)
        sync()
        b64 = bias2.double()
        mag = x0.double().abs() + S_t + b64.abs()
        check(x, x0.double() + ref_t + b64, ACC * (S_t + b64.abs()) + (S + 2) * 2.0 ** -24 * mag, f"{op} residual", key=f"resadd_x/{fmt}")
        y, yb = ln_ref(x, gamma, beta)
        check16(out16[:M], y, yb, fmt, f"{op} LayerNorm", key=f"layernorm_16/{fmt}")
        assert all_nan(out16[M:])
        return
    odt = torch.float32 if epi == abi.EPI_F32 else (torch.bfloat16 if epi == abi.EPI_BF16OUT else TDT[fmt])
    ofmt = "bf16" if epi == abi.EPI_BF16OUT else fmt
    ldc, rows = N + 16, M + 2
    outs = []
    for t in (0, tile):
        C = nans(batch, rows, ldc, dtype=odt)
        abi.check(_gemm(lib, fmt, A, W, bias, C, M, N, K, epi, t, batch, ldc, strideC=rows * ldc), f"gemm tile {t}")
        sync()
        assert all_nan(C[:, M:]) and all_nan(C[:, :, N:]), f"tile {t} stored past row M / column N"
        outs.append(C[:, :M, :N])
    assert torch.equal(outs[0], outs[1]), f"tile 0 != tile {tile}"
    out = outs[0]
    ref, Sm = _ref(A, W, bias)
    e32 = ACC * Sm + 1e-30
    if epi == abi.EPI_F32:
        check(out, ref, e32, f"{op} f32 tile {tile}", key=f"gemm_f32/{fmt}")
    elif epi == abi.EPI_QGELU_BF16:
        y = ref * torch.sigmoid(1.702 * ref)
        check16(out, y, qgelu_bound(ref, y, e32, fmt), fmt, f"{op} QuickGELU tile {tile}", key=f"gemm_qgelu/{fmt}")
    elif epi == abi.EPI_GELU_BF16:
        y = F.gelu(ref)
        check16(out, y, gelu_bound(ref, y, e32), fmt, f"{op} GELU tile {tile}", key=f"gemm_gelu/{fmt}")
    else:
        check16(out, ref, e32, ofmt, f"{op} 16-bit tile {tile}", key=f"gemm_16/{ofmt}")
        C32 = nans(batch, rows, ldc)
        rc = _gemm(lib, fmt, A, W, bias, C32, M, N, K, abi.EPI_F32, tile, batch, ldc, strideC=rows * ldc)
        sync()
        if rc == 0:
            check(C32[:, :M, :N], ref, e32, f"{op} f32 form of tile {tile}", key=f"gemm_f32/{fmt}")
        exact = rc == 0 and torch.equal(C32[:, :M, :N].to(odt), out)
        assert exact == (tile in EXACT16), f"tile {tile}: the 16-bit result {'is' if exact else 'is not'} the RNE of its f32 form (rc {rc})"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M", [514, 4112])
def test_frame_gemm_hard_operands(lib, fmt, M):
    """massive activations (two channels at 100x / 1000x), a bias 4x larger than the product, outputs spread over 1e-3 .. 1e5 in both signs
    (fp16 results past 65504: +-inf exactly where the fp64 value may round to it, never NaN; QuickGELU of |x| up to ~1e5), every epilogue:
    f32, 16-bit, bf16-out, QuickGELU, and the residual update with / without the gate"""
    N, K = 3072, 1024
    A = randn(M, K, seed=21)
    A[:, 5] *= 100.0
    A[:, 77] *= 1000.0
    A = A.to(TDT[fmt])
    W0 = randn(N, K, seed=22, scale=K ** -0.5)
    rms = (A.float() @ W0.t()).pow(2).mean(0).sqrt()
    spread = torch.logspace(-3, 5, N, device="cuda")[torch.randperm(N, generator=torch.Generator().manual_seed(3)).cuda()]
    W = (W0 * (spread / rms)[:, None]).to(TDT[fmt])
    bias = 4 * spread * randn(N, seed=23)
    ref, Sm = _ref(A, W, bias)
    e32 = ACC_HARD[fmt] * Sm + 1e-30
    ldc = N + 16

    def run(epi, C, gate=None):
        abi.check(_gemm(lib, fmt, A, W, bias, C, M, N, K, epi, 0, 1, ldc, gate=gate), f"gemm epi {epi}")
        sync()
        assert all_nan(C[M:]) and all_nan(C[:, N:]), f"epi {epi}: stored past row M / column N"
        return C[:M, :N]

    assert bool((ref.abs() > 65520).any()) and bool((ref.abs() < 1e-2).any())
    c32 = run(abi.EPI_F32, nans(M + 2, ldc))
    check(c32, ref, e32, "hard f32", key=f"gemm_f32/{fmt}")
    c16 = run(abi.EPI_BF16, nans(M + 2, ldc, dtype=TDT[fmt]))
    check16(c16, ref, e32, fmt, "hard 16-bit", key=f"gemm_16/{fmt}")
    assert torch.equal(c16, c32.to(TDT[fmt]))                 # round to nearest even of the same accumulators, +-inf past 65520
    cb = run(abi.EPI_BF16OUT, nans(M + 2, ldc, dtype=torch.bfloat16))
    check16(cb, ref, e32, "bf16", "hard bf16-out", key="gemm_16/bf16")
    assert torch.equal(cb, c32.to(torch.bfloat16))
    cq = run(abi.EPI_QGELU_BF16, nans(M + 2, ldc, dtype=TDT[fmt]))
    y = ref * torch.sigmoid(1.702 * ref)
    check16(cq, y, qgelu_bound(ref, y, e32, fmt), fmt, "hard QuickGELU", key=f"gemm_qgelu/{fmt}")
    # C += tanh(gate) (A W^T + b): tanhf and the product ~1 ulp each, then one f32 add
    R0 = randn(M, N, seed=24) * spread
    for gate in (torch.tensor([0.5], device="cuda"), None):
        t = math.tanh(0.5) if gate is not None else 1.0
        R = nans(M + 2, ldc)
        R[:M, :N] = R0
        r = run(abi.EPI_RESADD_F32, R, gate)
        refr = R0.double() + t * ref
        check(r, refr, t * e32 + 2.0 ** -22 * t * ref.abs() + 2.0 ** -24 * refr.abs() + 1e-30, "hard resadd", key=f"gemm_resadd/{fmt}")


# ================================================================================================ 2. attention
ATTN_CASES = [  # name, batch, heads, q_len, kv1, kv2 (0: one segment) -> the branch of attention.hip launch_attn_mfma
    ("vit_8wave", 2, 16, 257, 257, 0),               # attn_vit_kernel, 8 waves, one query tile per wave (B H < 128)
    ("vit_8wave_ragged", 3, 16, 200, 270, 0),        # the same, ragged query / key counts (14 keys in the last tile)
    ("vit_16wave_loop", 8, 16, 257, 257, 0),         # B H >= 128: one 16-wave workgroup walks all 17 query tiles
    ("general_4wave", 2, 8, 64, 200, 0),             # attn_mfma_kernel, 4 waves (q_len <= 64)
    ("general_8wave", 2, 4, 100, 150, 0),            # 8 waves, no loop
    ("general_8wave_loop", 16, 8, 100, 100, 0),      # 8 waves, query-tile loop (B H >= 128)
    ("general_4wave_2seg", 2, 8, 64, 100, 30),       # two segments through the general kernel (<= 19 key tiles)
    ("perceiver_2seg", 2, 8, 64, 256, 64),           # attn_vit_kernel SEG2: 305 .. 320 keys, q_len <= 64
    ("perceiver_2seg_ragged", 2, 8, 64, 250, 60),    # kv1 not a multiple of 16
    ("long_36tile", 2, 8, 64, 512, 64),              # attn_mfma_kernel with 36 key tiles (321 .. 576 keys)
    ("long_36tile_ragged", 1, 2, 37, 300, 41)]
FAMILIES = ["plain", "peaked", "max_last", "max_first", "offset60", "equal", "max_seg2"]
SCALE = 0.125
ACC_S = 2.0 ** -21      # a 64-term score: two chained 32-term MFMAs (f32 MFMA chains measure 1e-7 .. 3.5e-7 of sum |q k|)
PAD = 3                 # NaN rows behind every q / k / v / o block of a batch entry


def attn_inputs(fam, B, H, Q, KV, kv1, fmt, seed):
    """q [B, H, Q, 64], k / v [B, H, KV, 64] in the operand format (device)"""
    q, k, v = randn(B, H, Q, 64, seed=seed), randn(B, H, KV, 64, seed=seed + 1), randn(B, H, KV, 64, seed=seed + 2)
    if fam == "peaked":                                    # scores ~ N(0, 10^2): softmax rows of a few keys, spanning about +-40
        q, k = q * 3.2, k * 3.2
    elif fam.startswith("max_"):                           # one key ~24 above every other score, for every query
        u = torch.sign(randn(B, H, 1, 64, seed=seed + 3))
        q = u + 0.3 * q
        k = 0.5 * k
        j = {"max_last": KV - 1, "max_first": 0, "max_seg2": kv1 + 3}[fam]
        k[:, :, j] = 3.0 * u[:, :, 0]
    elif fam == "offset60":                                # a common +60 on every score (softmax-invariant)
        c = math.sqrt(60.0 / SCALE)
        q[..., 0], k[..., 0] = c, c
    elif fam == "equal":                                   # every key the same: exactly equal scores, O = mean of V
        k = k[:, :, :1].expand(B, H, KV, 64).contiguous()
    return q.to(TDT[fmt]), k.to(TDT[fmt]), v.to(TDT[fmt])


def attn_ref(q, k, v, fmt):
    """fp64 softmax(scale q k^T) v and the bound of the kernels' arithmetic (attention.hip:135-205, 300-363):
    scores: f32 MFMA sums of 64 exact products, error <= ACC_S scale sum_d |q k| -> p_j = exp(s_j - max) in f32 carries relative
            Es = 2 ACC_S max_j scale sum|q k_j| + 2^-22 (1 + span of the row) (scaled score, subtraction / fused exp2 argument, v_exp);
    P V:    P rounded to 16 bits (U, and absolute TINY_P per key: fp16 P below 2^-14 is subnormal) under an f32 MFMA chain (ACC):
            numerator error <= M1 (Es + U + ACC) + TINY_P sum|v| / D, M1 = sum_j p_j |v_j| / D;
    divisor: the sum of the unrounded f32 P (Es + kv 2^-24 relative) and 1 / sum, the product (2^-21): |o| (Es + kv 2^-24 + 2^-21);
    then the 16-bit output rounding (check16)."""
    q64, k64, v64 = q.double(), k.double(), v.double()
    s = (q64 @ k64.transpose(-1, -2)) * SCALE
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    D = p.sum(-1, keepdim=True)
    o = (p @ v64) / D
    M1 = (p @ v64.abs()) / D
    smag = ((q64.abs() @ k64.abs().transpose(-1, -2)) * SCALE).amax(-1, keepdim=True)
    Es = 2 * ACC_S * smag + 2.0 ** -22 * (1 + m - s.amin(-1, keepdim=True))
    kv = k.shape[-2]
    tiny_p = 2.0 ** -25 if fmt == "f16" else 2.0 ** -120
    e32 = M1 * (Es + U[fmt] + ACC) + tiny_p * v64.abs().sum(-2, keepdim=True) / D + o.abs() * (Es + kv * 2.0 ** -24 + 2.0 ** -21)
    return o, e32


def _blk(x, rows, ld, fmt):
    """[B, H, L, 64] -> a NaN-filled [B, rows + PAD, ld] buffer holding x in its first L rows / H * 64 columns"""
    B, H, L, _ = x.shape
    t = nans(B, rows + PAD, ld, dtype=TDT[fmt])
    t[:, :L, :H * 64] = x.transpose(1, 2).reshape(B, L, H * 64)
    return t


def run_attn(lib, fmt, q, k, v, kv1, kv2):
    """the kernel's O [B, H, Q, 64]; the K / V rows past each segment's keys, the Q rows past q_len and the columns past H * 64 are NaN; the
    O rows / columns past the output must stay NaN"""
    B, H, Q, _ = q.shape
    ld = H * 64 + 8
    Qb, Ob = _blk(q, Q, ld, fmt), nans(B, Q + PAD, ld, dtype=TDT[fmt])
    if kv2 == 0:
        Kb, Vb = _blk(k, kv1, ld, fmt), _blk(v, kv1, ld, fmt)
        rc = getattr(lib, f"deer_attn_{ATTN[fmt]}_hd64")(abi.ptr(Qb), abi.ptr(Kb), abi.ptr(Vb), abi.ptr(Ob), B, H, Q, kv1, ld, ld, ld, ld,
                                                         (Q + PAD) * ld, (kv1 + PAD) * ld, (kv1 + PAD) * ld, (Q + PAD) * ld, SCALE, st())
    else:
        K1, V1 = _blk(k[:, :, :kv1], kv1, ld, fmt), _blk(v[:, :, :kv1], kv1, ld, fmt)
        K2, V2 = _blk(k[:, :, kv1:], kv2, ld, fmt), _blk(v[:, :, kv1:], kv2, ld, fmt)
        rc = getattr(lib, f"deer_attn_{ATTN[fmt]}_hd64_2seg")(abi.ptr(Qb), abi.ptr(K1), abi.ptr(V1), abi.ptr(K2), abi.ptr(V2), abi.ptr(Ob), B, H, Q,
                                                              kv1, kv2, ld, ld, ld, ld, (Q + PAD) * ld, (kv1 + PAD) * ld, (kv2 + PAD) * ld,
                                                              (Q + PAD) * ld, SCALE, st())
    abi.check(rc, "attention")
    sync()
    assert all_nan(Ob[:, Q:]) and all_nan(Ob[:, :, H * 64:]), "stored past q_len / the heads' columns"
    return Ob[:, :Q, :H * 64].reshape(B, Q, H, 64).transpose(1, 2)


_ATTN_PARAMS = [(c, f) for c in ATTN_CASES for f in FAMILIES if f != "max_seg2" or c[5] > 0]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case,fam", _ATTN_PARAMS, ids=[f"{c[0]}-{f}" for c, f in _ATTN_PARAMS])
def test_frame_attention(lib, fmt, case, fam):
    name, B, H, Q, kv1, kv2 = case
    q, k, v = attn_inputs(fam, B, H, Q, kv1 + kv2, kv1, fmt, seed=len(name) * 100 + FAMILIES.index(fam))
    o = run_attn(lib, fmt, q, k, v, kv1, kv2)
    ref, e32 = attn_ref(q, k, v, fmt)
    check16(o, ref, e32, fmt, f"{name} {fam}", key=f"attention/{fmt}")


# ================================================================================================ 3. LayerNorm row ops
ROWS = ["plain", "offset1e2", "offset1e3", "offset3e3", "channel1000", "constant3", "gamma_spread", "gamma_overflow"]


def ln_rows(C, seed):
    """one row per kind (x, gamma, beta): x ~ N(0.5, 2^2), or unit rows offset by 1e2 / 1e3 / 3e3, one channel at 1000, the constant 3;
    gamma 1 + N(0, 0.1^2), spread over two decades, or 3000 on a row with one channel at 100 (|y| past 65504 for fp16)"""
    n = len(ROWS)
    x = randn(n, C, seed=seed) * 2 + 0.5
    for i, kind in enumerate(ROWS):
        if kind.startswith("offset"):
            x[i] = randn(C, seed=seed + i) + float(kind[6:])
        elif kind == "channel1000":
            x[i] = randn(C, seed=seed + i)
            x[i, 7] = 1000.0
        elif kind == "constant3":
            x[i] = 3.0                                   # sum exact: mean 3, variance 0 -> y == beta bit for bit
        elif kind == "gamma_overflow":
            x[i, 7] = 100.0                              # normalised ~sqrt(C) on channel 7: 1e5 .. 2e5 after gamma = 3000
    gamma = 1.0 + randn(n, C, seed=seed + 50, scale=0.1)
    gamma[ROWS.index("gamma_spread")] = 10.0 ** (2 * uniform(C, seed) - 1)
    gamma[ROWS.index("gamma_overflow")] = 3000.0
    beta = randn(n, C, seed=seed + 60, scale=0.1)
    return x, gamma, beta


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("C", [1024, 4096])
def test_layernorm_rows_hard_rows(lib, fmt, C):
    """deer_layernorm_rows(_f16) with both outputs: f32 per element against fp64, the 16-bit output the RNE of the f32 one bit for bit (+-inf
    past 65520 in fp16), the constant row gives beta exactly; _multi(_f16) gives the same 16 bits for each of its (gamma, beta) sets"""
    x, gamma, beta = ln_rows(C, seed=C)
    sfx = "_f16" if fmt == "f16" else ""
    ldi, ldo = C + 8, C + 4
    xin = nans(len(ROWS), ldi)
    xin[:, :C] = x
    for i, kind in enumerate(ROWS):                        # one launch per row: every row has its own gamma / beta
        o16, o32 = nans(2, ldo, dtype=TDT[fmt]), nans(2, ldo)
        abi.check(getattr(lib, f"deer_layernorm_rows{sfx}")(abi.ptr(xin[i]), ldi, 0, 1, 1, abi.ptr(gamma[i]), abi.ptr(beta[i]), abi.ptr(o16),
                                                            abi.ptr(o32), ldo, 0, C, 1e-5, st()), "layernorm_rows")
        sync()
        assert all_nan(o16[0, C:]) and all_nan(o16[1]) and all_nan(o32[0, C:]) and all_nan(o32[1])
        y, yb = ln_ref(x[i:i + 1], gamma[i], beta[i])
        check(o32[:1, :C], y, yb, f"LayerNorm f32 row {kind}", key="layernorm_f32")
        assert torch.equal(o16[0, :C], o32[0, :C].to(TDT[fmt])), f"16-bit output is not the RNE of the f32 output (row {kind})"
        if kind == "constant3":
            assert torch.equal(o32[0, :C], beta[i])
        if kind == "gamma_overflow" and fmt == "f16":
            assert bool(torch.isinf(o16[0, :C]).any())
        # Perceiver norm_media: one pass of statistics, 3 (gamma, beta) sets; set 1 is this row's
        gs, bs = torch.stack([gamma[0], gamma[i], gamma[1]]), torch.stack([beta[0], beta[i], beta[1]])
        om = nans(3, 2, ldo, dtype=TDT[fmt])
        abi.check(getattr(lib, f"deer_layernorm_rows_multi{sfx}")(abi.ptr(xin[i]), ldi, 0, 1, 1, abi.ptr(gs), abi.ptr(bs), 3, C, abi.ptr(om),
                                                                  2 * ldo, ldo, 0, C, 1e-5, st()), "layernorm_rows_multi")
        sync()
        assert torch.equal(om[1, 0, :C], o16[0, :C]) and all_nan(om[:, 1]) and all_nan(om[:, 0, C:])


@pytest.mark.parametrize("fmt", FMTS)
def test_resadd_ln_hard_rows(lib, fmt):
    """deer_resadd_ln(_f16): x += slab0 + slab1 + bias (f32 in slab order: equal to the same sums in torch f32), LayerNorm of the new x with
    both outputs (f32 gated, 16 bits = RNE of f32); 2048 copies of the row go through the multi-row kernel (no f32 output; and
    deer_resadd_ln_multirow at R = 2 / 4) and must give the same 16 bits - fp16 results past 65504 are +-inf on every path, as .half()"""
    C = 1024
    x, gamma, beta = ln_rows(C, seed=5)
    s = randn(2, len(ROWS), C, seed=6, scale=0.01)
    bias = randn(C, seed=7, scale=0.01)
    xs = x - ((s[0] + s[1]) + bias)                          # x0 such that x0 + (s0 + s1 + b) lands near the hard row
    exp_x = xs + ((s[0] + s[1]) + bias)
    T = 2048
    for i, kind in enumerate(ROWS):
        xr = xs[i:i + 1].clone()
        si = s[:, i].contiguous()
        o16, o32 = nans(2, C, dtype=TDT[fmt]), nans(2, C)
        _resadd(lib, fmt, xr, si, 2, C, bias, gamma[i], beta[i], o16, o32, 1, C)
        sync()
        assert torch.equal(xr[0], exp_x[i])
        y, yb = ln_ref(xr, gamma[i], beta[i])
        check(o32[:1], y, yb, f"resadd LayerNorm f32 row {kind}", key="layernorm_f32")
        assert torch.equal(o16[0], o32[0].to(TDT[fmt])), f"16-bit output is not the RNE of the f32 output (row {kind})"
        assert all_nan(o16[1]) and all_nan(o32[1])
        if kind == "gamma_overflow" and fmt == "f16":
            assert bool(torch.isinf(o16[0]).any())
        big = xs[i:i + 1].expand(T, C).contiguous()
        sb = si[:, None].expand(2, T, C).contiguous()
        ob = nans(T + 1, C, dtype=TDT[fmt])
        _resadd(lib, fmt, big, sb, 2, T * C, bias, gamma[i], beta[i], ob, None, T, C)
        sync()
        assert torch.equal(ob[:T], o16[0].expand(T, C)) and all_nan(ob[T:]), f"multi-row kernel != one-row kernel (row {kind})"
        if fmt == "bf16":
            for R in (2, 4):
                big = xs[i:i + 1].expand(T - 1, C).contiguous()
                ob = nans(T, C, dtype=torch.bfloat16)
                abi.check(lib.deer_resadd_ln_multirow(abi.ptr(big), abi.ptr(sb), 2, T * C, None, abi.ptr(bias), abi.ptr(gamma[i]), abi.ptr(beta[i]),
                                                      abi.ptr(ob), T - 1, C, 1e-5, R, st()), "resadd_ln_multirow")
                sync()
                assert torch.equal(ob[:T - 1], o16[0].expand(T - 1, C)) and all_nan(ob[T - 1:]), (R, kind)


def test_vit_embed_lnpre(lib):
    """x[n][t] = ln_pre([cls ; patches[n]][t] + pos[t]): the f32 sum as torch computes it, then the LayerNorm gated against fp64; gamma over
    two decades; positional rows offset by 1e2 / 1e3 / 3e3 and one channel at 1000; cls + pos[0] = 3.0 exactly gives beta bit for bit"""
    N, P, W = 3, 256, 1024
    patch = randn(N * P, W, seed=31)
    cls = torch.full((W,), 1.5, device="cuda")
    pos = randn(P + 1, W, seed=32, scale=0.5)
    pos[0] = 1.5
    for t, off in ((1, 1e2), (2, 1e3), (3, 3e3)):
        pos[t] += off
    pos[4, 9] = 1000.0
    g, b = 10.0 ** (2 * uniform(W, 33) - 1), randn(W, seed=34, scale=0.1)
    x = nans(N * (P + 1) + 1, W)
    abi.check(lib.deer_vit_embed_lnpre(abi.ptr(patch), abi.ptr(cls), abi.ptr(pos), abi.ptr(g), abi.ptr(b), abi.ptr(x), N, P, W, 1e-5, st()), "embed_lnpre")
    sync()
    assert all_nan(x[N * (P + 1):])
    src = torch.cat([torch.cat([cls[None], patch[n * P:(n + 1) * P]]) + pos for n in range(N)])
    y, yb = ln_ref(src, g, b)
    check(x[:N * (P + 1)], y, yb, "vit_embed_lnpre", key="layernorm_f32")
    for n in range(N):
        assert torch.equal(x[n * (P + 1)], b)


# ================================================================================================ 4. untested entry points (exact)
def test_vit_im2col_f32(lib):
    """im2col of f32 frames = F.unfold(14 x 14, stride 14) row for row, pad columns 588 .. Kpad zero, nothing past the last row"""
    N, S, p, Kpad = 2, 224, 14, 640
    img = randn(N, 3, S, S, seed=41)
    P = (S // p) ** 2
    out = nans(N * P + 1, Kpad)
    abi.check(lib.deer_vit_im2col_f32(abi.ptr(img), N, S, p, abi.ptr(out), Kpad, st()), "im2col_f32")
    sync()
    ref = F.unfold(img, p, stride=p).transpose(1, 2).reshape(N * P, 3 * p * p)
    assert torch.equal(out[:N * P, :3 * p * p], ref)
    assert torch.equal(out[:N * P, 3 * p * p:], torch.zeros(N * P, Kpad - 3 * p * p, device="cuda"))
    assert all_nan(out[N * P:])


@pytest.mark.parametrize("table", ["f16", "f32"])
def test_embed_tokens(lib, table):
    """x = wte[ids] bit for bit (ids -1 and vocab clamp to 0 / vocab - 1, norm_embed.hip:451-452), text_time = the running count of the media
    token per environment (B = 3 environments with 0 / 1 / 3 media tokens); nothing written past the B T rows"""
    B, T, d, vocab, media = 3, 9, 1000, 50, 7
    wte = randn(vocab, d, seed=51).to(torch.float16 if table == "f16" else torch.float32)
    ids = torch.tensor([[1, 2, 3, -1, 4, 5, vocab, 6, 8],
                        [media, 2, 3, 4, 5, 6, 8, 9, 10],
                        [media, 11, media, 12, 13, media, vocab, -1, 14]], dtype=torch.int64, device="cuda")
    x = nans(B * T + 1, d)
    tt = torch.full((B * T + 1,), -5, dtype=torch.int32, device="cuda")
    fn = lib.deer_embed_tokens_f16 if table == "f16" else lib.deer_embed_tokens_f32
    abi.check(fn(abi.ptr(ids), abi.ptr(wte), abi.ptr(x), abi.ptr(tt), T, B, d, vocab, media, st()), "embed_tokens")
    sync()
    assert torch.equal(x[:B * T], wte[ids.clamp(0, vocab - 1)].float().reshape(B * T, d)) and all_nan(x[B * T:])
    assert torch.equal(tt[:B * T], torch.cumsum((ids == media).int(), 1).int().reshape(-1)) and int(tt[B * T]) == -5


# ================================================================================================ 5. the gates bite
@pytest.mark.parametrize("fmt", FMTS)
def test_gates_reject_perturbed_results(lib, fmt):
    """negative controls: the kernel's own results, perturbed on the host, must fail the same checkers - 16-bit results truncated toward zero;
    the 257th row of a frame (the row the frame tiles deal out over the waves) scaled by 1 + 4 U; the attention reference without the
    dominant last key; a LayerNorm with the one-pass variance E[x^2] - E[x]^2 in f32 on rows offset by 1e3 sigma"""
    M, N, K = 514, 3072, 1024
    tile = select_tile(M, N, K, 1, abi.EPI_BF16)
    A, W = _operands(fmt, 1, M, N, K, seed=61)
    bias = randn(N, seed=62, scale=0.1)
    ref, Sm = _ref(A[0], W[0], bias)
    e32 = ACC * Sm + 1e-30
    c16, c32 = nans(M, N, dtype=TDT[fmt]), nans(M, N)
    abi.check(_gemm(lib, fmt, A, W, bias, c16, M, N, K, abi.EPI_BF16, tile), "gemm")
    abi.check(_gemm(lib, fmt, A, W, bias, c32, M, N, K, abi.EPI_F32, tile), "gemm")
    sync()
    check16(c16, ref, e32, fmt, "unperturbed")
    rtz = c32.to(TDT[fmt])                                 # round to nearest even, then one ulp back wherever that went away from zero
    away = rtz.float().abs() > c32.abs()
    bits = rtz.view(torch.int16)
    rtz = torch.where(away, bits - 1, bits).view(TDT[fmt])
    with pytest.raises(AssertionError):
        check16(rtz, ref, e32, fmt, "round toward zero")
    bad = c16.clone()
    bad[256] = (c16[256].double() * (1 + 4 * U[fmt])).to(TDT[fmt])
    with pytest.raises(AssertionError):
        check16(bad, ref, e32, fmt, "257th row x (1 + 4 U)")
    B, H, Q, KV = 2, 16, 257, 257
    q, k, v = attn_inputs("max_last", B, H, Q, KV, KV, fmt, seed=63)
    o = run_attn(lib, fmt, q, k, v, KV, 0)
    r, e = attn_ref(q, k, v, fmt)
    check16(o, r, e, fmt, "unperturbed attention")
    r, e = attn_ref(q, k[:, :, :-1], v[:, :, :-1], fmt)
    with pytest.raises(AssertionError):
        check16(o, r, e, fmt, "reference without the last key")
    C = 1024
    x = randn(4, C, seed=64) + 1e3
    y, yb = ln_ref(x, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"))
    mu = x.mean(-1, keepdim=True)
    one_pass = (x - mu) * torch.rsqrt((x * x).mean(-1, keepdim=True) - mu * mu + 1e-5)
    with pytest.raises(AssertionError):
        check(one_pass, y, yb, "one-pass variance")
