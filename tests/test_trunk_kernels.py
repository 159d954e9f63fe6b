"""The one-environment trunk layer (csrc/model.hip::llm_layer_r16: <= 16 text rows, one MFMA row tile) one kernel at a time through the C ABI,
against float64 references computed on the device and gated ELEMENT BY ELEMENT (tests/test_hip_ops.py gates the same kernels with one norm
ratio per tensor): deer_resadd_ln_packed, deer_trunk_wide_gemm (epilogues 0 / 1 / 2), deer_trunk_mpt_attn alone and behind the GEMM that
writes its q|k|v and LayerNorm moments, deer_xattn_fused_packed / deer_xattn_fused at one environment, deer_gemm_skinny_hl at one row tile -
each with its `_f16` twin (the default arithmetic).

Conventions of tests/test_frame_kernels.py (helpers copied, not imported): operands drawn on the device from fixed seeds and rounded to the
operand format, so the fp64 reference sees the kernel's operands; NaN sentinels in and around every buffer; the worst element (index, value,
reference, bound) in the assertion message; the largest error / bound per family printed at the end of the module.
  ACC     f32 accumulation: |err| <= ACC * S, S = sum_k |a_k w_k|.  4e-6: the class gate of tests/test_frame_kernels.py / test_head_kernels.py
  U       half an ulp of the 16-bit format (2^-8 bf16, 2^-11 fp16), TINY half its subnormal step, OVF the smallest magnitude that rounds to inf
          (tests/test_frame_kernels.py)
  PAIR    the residue of a hi + lo pair (csrc/common.h::split2): hi = fmt(v) leaves |v - hi| <= U |v|, lo = fmt(v - hi) leaves U of that:
          |v - hi - lo| <= U^2 |v| (+ TINY where lo is subnormal) = 2^-16 (bf16) / 2^-22 (fp16) - inside the pair gates SEQ_TOL of
          tests/test_head_kernels.py (4 * 2^-17, 8 * 2^-22).  fp16: hi saturates at +-65504 and lo = fp16(v - hi) carries the rest up to
          |v| < 65504 + 65520; beyond, lo = +-inf and hi + lo = +-inf (as .half() gives), never NaN.
Every other bound (LayerNorm, erf-GELU, moments, the two attentions) is derived next to its reference function from fp64 quantities of the
reference.  No element is skipped: the only elements without a finite bound are those the reference puts past the overflow threshold, and
rows the reference itself cannot define (asserted where they occur)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from deer_vla_amd import _abi as abi  # noqa: E402

ACC = 4e-6
# the f32 gate of test_trunk_wide_gemm_hard_operands (a 1000x activation channel, fp16-subnormal weights in the columns scaled to 1e-3):
# deer_trunk_wide_gemm_f16 measures 7.8e-6 S there (error / bound 0.49 under 4 ACC; 1.0e-6 S in bf16, 0.26 under ACC), above the class gate
# ACC = 4e-6 that holds on N(0, 1) operands (measured 6e-8 S).  tests/test_frame_kernels.py::ACC_HARD widens by the same factor for the same
# reason (v_mfma_f32_16x16x32_f16 on such operands: 8.7e-6 S in the frame GEMMs).  The wider gate still fails a wrong kernel: with the lo MFMA
# of one k-tile dropped, or with 7 of the 8 wave partials summed, test_trunk_wide_gemm_hard_operands fails (mutation table of the commit)
ACC_HARD = {"bf16": ACC, "f16": 4 * ACC}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TINY = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25}
OVF = {"bf16": 2.0 ** 128 * (1 - 2.0 ** -9), "f16": 65520.0}
PAIR = {"bf16": 2.0 ** -16, "f16": 2.0 ** -22}
F16_MAX = 65504.0
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
FMTS = ["bf16", "f16"]
NAN = float("nan")
SHAPE = 1                                    # DEER_ERR_SHAPE
ALL_T = list(range(1, 17))
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


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def fn(lib, fmt, name):
    return getattr(lib, name + ("_f16" if fmt == "f16" else ""))


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


def half_ulp(hi):
    """1/2 ulp of every element of a 16-bit tensor in fp64 (tests/test_env_batch_ops.py::_half_ulp)"""
    p, emin = (10, -14) if hi.dtype == torch.float16 else (7, -126)
    h = hi.double().abs()
    e = torch.floor(torch.log2(torch.where(h > 0, h, torch.ones_like(h)))).clamp(min=emin)
    e = torch.where(h > 0, e, torch.full_like(e, emin))
    return torch.exp2(e - p - 1)


def split_hl(a, fmt):
    """csrc/common.h::split2 on f32 values: hi = fmt(v) (fp16: saturated at +-65504), lo = fmt(v - hi), the difference in f32"""
    hi = (a.clamp(-F16_MAX, F16_MAX) if fmt == "f16" else a).to(TDT[fmt])
    return hi, (a - hi.float()).to(TDT[fmt])


def check_pair(hi, lo, ref, e32, fmt, what, key=None):
    """hi / lo planes of an f32 value v with |v - ref| <= e32: hi + lo (exact in fp64) within e32 + the pair residue PAIR |ref| + TINY
    (fp16 past 65504: + U (|ref| - 65504), lo carries the excess; +-inf allowed only where |ref| + e32 reaches 65504 + 65520, never NaN);
    and the pair is a split: |lo| <= ulp(hi) / 2 and hi = fmt(hi + lo) unless hi + lo is a rounding tie (below the saturation zone);
    hi = +-65504 exactly where |ref| - e32 >= 65520.
    The residue U^2 |v| is attainable (v half an ulp of hi away from hi, v - hi half an ulp of lo away from lo), so on large fp16 tensors the
    measured error / bound is expected to sit just below 1 (0.997 in the attention tests): that is the bound being sharp, not a near miss"""
    h, l = hi.double(), lo.double()
    s = h + l
    ra = ref.abs()
    resid = PAIR[fmt] * ra + TINY[fmt]
    if fmt == "f16":
        resid = resid + U[fmt] * (ra - F16_MAX).clamp(min=0)
        may_inf = (ra + e32 >= F16_MAX + OVF["f16"]) & torch.isinf(s) & (torch.sign(s) == torch.sign(ref))
        s = torch.where(may_inf, ref, s)
        safe = ra + e32 < F16_MAX
        must = ra - e32 >= OVF["f16"]
        assert bool((h.abs()[must] == F16_MAX).all()), f"{what}: hi is not +-65504 where the value is past 65520"
    else:
        safe = torch.ones_like(ra, dtype=torch.bool)
    rmax = check(s, ref, e32 + resid, what, key)
    hu = half_ulp(hi)
    bad = safe & (l.abs() > hu)
    assert not bool(bad.any()), f"{what}: |lo| > ulp(hi) / 2 at {tuple(int(i) for i in bad.nonzero()[0])}"
    r = s.float().to(TDT[fmt]).double()
    bad = safe & (r != h) & ((s - h).abs() != (s - r).abs())
    assert not bool(bad.any()), f"{what}: hi != fmt(hi + lo) at {tuple(int(i) for i in bad.nonzero()[0])}"
    return rmax


def poison(rows, cols, fmt):
    """what an earlier, longer instruction may have left above row T: NaN, +-inf, +-65504 patterns"""
    vals = torch.tensor([NAN, math.inf, -math.inf, 65504.0, -65504.0, NAN, 65504.0], device="cuda")
    idx = (torch.arange(rows * cols, device="cuda") * 3 + torch.arange(rows * cols, device="cuda") // cols) % 7
    return vals[idx].view(rows, cols).to(TDT[fmt])


def pack_frag(p, T, fmt, fill):
    """16-bit [T, K] -> MFMA-fragment order [K/32][16 * (k % 32 / 8) + row][8] (csrc/norm_embed.hip: resadd_ln_body); rows >= T: zeros, `poison` or NaN"""
    K = p.shape[1]
    full = {"zero": lambda: torch.zeros(16, K, dtype=TDT[fmt], device="cuda"), "poison": lambda: poison(16, K, fmt),
            "nan": lambda: nans(16, K, dtype=TDT[fmt])}[fill]()
    full[:T] = p[:T]
    return full.view(16, K // 32, 4, 8).permute(1, 2, 0, 3).contiguous().view(-1)


def pack(lib, W):
    Wp = torch.empty_like(W)
    abi.check(lib.deer_pack_weight_mfma16(abi.ptr(W), abi.ptr(Wp), W.shape[0], W.shape[1], st()), "pack")
    return Wp


def ctl_block(all_exited):
    c = torch.zeros(abi.CTL_WORDS, dtype=torch.int32, device="cuda")
    c[abi.CTL_ALL_EXITED] = 1 if all_exited else 0
    return c


def gemm_ref(A, W):
    """fp64 A W^T and S = |A| |W|^T"""
    A64, W64 = A.double(), W.double()
    return A64 @ W64.t(), A64.abs() @ W64.abs().t()


def pair_operand_err(W, S, fmt, acc=ACC):
    """error of an f32-accumulated product whose activation entered as a hi + lo pair of the TRUE f32 value (the reference is on the true
    value, so a dropped lo MFMA fails): ACC S + PAIR S, and in fp16 the subnormal floor of lo, TINY sum_k |w_k|"""
    e = (acc + PAIR[fmt]) * S + 1e-30
    if fmt == "f16":
        e = e + TINY[fmt] * W.double().abs().sum(-1)
    return e


def gelu_bound(x, y, e32):
    """0.5 x (1 + erff(x / sqrt 2)) in f32 of a value carrying error e32 (tests/test_frame_kernels.py::gelu_bound): slope <= 1.13; erff ~2 ulp
    of a value <= 1, i.e. absolute 2^-22 before the product with x / 2 (for x << 0 that is the whole result: 1 + erf cancels, the kernel gives
    -0.0 where fp64 gives -1e-80); the products ~1 ulp each (2^-21 |y|)"""
    return 1.13 * e32 + x.abs() * 2.0 ** -22 + y.abs() * 2.0 ** -21


def ln_ref(x, gamma, beta, eps=1e-5):
    """fp64 LayerNorm of the rows of x (the f32 values the kernel reads) and the bound of the kernels' f32 two-pass arithmetic
    (tests/test_frame_kernels.py::ln_ref; the packed kernel reduces over 8 waves, the q/k LayerNorm of deer_trunk_mpt_attn over <= 128 group
    means - both inside the 32 roundings of the mean):
    mean: |dmu| <= 32 2^-24 mean|x|, which enters every output as gamma dmu rstd: the error that grows with |mu| / sigma;
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


# ================================================================================================ 1. deer_resadd_ln_packed
def _resadd_packed(lib, fmt, x, slab, s_in, stride, gate, gamma, beta, hi, lo, y32, xc, T, d, ctl=None, bias=None):
    return fn(lib, fmt, "deer_resadd_ln_packed")(abi.ptr(x), abi.ptr(slab), s_in, stride, abi.ptr(gate), abi.ptr(bias), abi.ptr(gamma), abi.ptr(beta),
                                               abi.ptr(hi), abi.ptr(lo), abi.ptr(y32), abi.ptr(xc), T, d, 1e-5, abi.ptr(ctl), st())


def _frag_expected(p, T, fmt, d):
    """the whole plane buffer a packed kernel must leave: p's rows < T at their fragment address, NaN sentinels everywhere else"""
    return torch.cat([pack_frag(p, T, fmt, "nan"), nans(64, dtype=TDT[fmt])])


def _run_packed(lib, fmt, x0, slab, s_in, gate, gamma, beta, T, d, want_f32, want_copy):
    x = nans(T + 1, d)
    x[:T] = x0
    hi, lo = nans(16 * d + 64, dtype=TDT[fmt]), nans(16 * d + 64, dtype=TDT[fmt])
    y32 = nans(T + 1, d) if want_f32 else None
    xc = nans(T + 1, d) if want_copy else None
    abi.check(_resadd_packed(lib, fmt, x, slab, s_in, 16 * d, gate, gamma, beta, hi, lo, y32, xc, T, d), "resadd_ln_packed")
    sync()
    assert all_nan(x[T:]) and (y32 is None or all_nan(y32[T:])) and (xc is None or all_nan(xc[T:])), "stored past row T"
    return x, hi, lo, y32, xc


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", [256, 2048, 4096])
def test_resadd_ln_packed(lib, fmt, d):
    """every T; no slab / the 8 x-attn head slabs under tanh(gate) / the split-K slab counts of the out- and down-projection without a gate;
    beta, x_copy by T.  Residual stream and x_copy bit for bit deer_resadd_ln's and per element against fp64; the f32 LayerNorm per element
    against fp64; the planes exactly split2 of that f32 value AT THE FRAGMENT ADDRESS, the same bits with and without out_f32, rows >= T
    and the tail keep their sentinel bits"""
    gamma, beta_t = 1.0 + randn(d, seed=10, scale=0.1), randn(d, seed=11, scale=0.1)
    gate = torch.tensor([0.3], device="cuda")
    cfgs = [("none", 0, None), ("xattn8", 8, gate), ("splitk_d", lib.deer_skinny_hl_splitk(16, d, d), None),
            ("splitk_4d", lib.deer_skinny_hl_splitk(16, d, 4 * d), None)]
    assert {c[1] for c in cfgs} >= {0, 8} and cfgs[3][1] in (4, 8, 16)
    for T in ALL_T:
        beta = beta_t if T % 2 == 0 else None
        want_copy = (T // 2) % 2 == 0
        for name, s_in, g in cfgs:
            what = f"d {d} T {T} {name}"
            x0 = randn(T, d, seed=100 * T + s_in)
            slab = None
            if s_in:
                slab = nans(s_in, 16, d)
                slab[:, :T] = randn(s_in, T, d, seed=100 * T + s_in + 1, scale=0.2)
            x, hi, lo, y32, xc = _run_packed(lib, fmt, x0, slab, s_in, g, gamma, beta, T, d, True, want_copy)
            # the row-major kernel on the same inputs
            xr, yr, xcr = nans(T + 1, d), nans(T + 1, d), nans(T + 1, d)
            xr[:T] = x0
            abi.check(fn(lib, fmt, "deer_resadd_ln")(abi.ptr(xr), abi.ptr(slab), s_in, 16 * d, abi.ptr(g), None, abi.ptr(gamma), abi.ptr(beta), None,
                                                     abi.ptr(yr), abi.ptr(xcr), T, d, 1e-5, None, st()), "resadd_ln")
            sync()
            assert same_bits(x, xr), f"{what}: residual stream differs from deer_resadd_ln"
            if want_copy:
                assert same_bits(xc, xcr) and same_bits(xc, x), f"{what}: x_copy"
            if s_in:
                # x += tanh(gate) sum_s slab[s]: s_in - 1 f32 adds (each <= 2^-24 of sum |slab|), the product, the add; tanhf a few ulp
                t = math.tanh(0.3) if g is not None else 1.0
                sl = slab[:, :T].double()
                mag = x0.double().abs() + t * sl.abs().sum(0)
                check(x[:T], x0.double() + t * sl.sum(0), (s_in + 4) * 2.0 ** -24 * mag + 2.0 ** -21 * t * sl.abs().sum(0) + 1e-30,
                      f"{what}: residual", key=f"resadd_x/{fmt}")
            else:
                assert same_bits(x[:T], x0)
            y, yb = ln_ref(x[:T], gamma, beta)
            check(y32[:T], y, yb, f"{what}: LayerNorm f32", key=f"resadd_ln/{fmt}")
            eh, el = split_hl(y32[:T], fmt)
            assert same_bits(hi, _frag_expected(eh, T, fmt, d)), f"{what}: hi plane is not fmt(y) in fragment order / rows >= T written"
            assert same_bits(lo, _frag_expected(el, T, fmt, d)), f"{what}: lo plane is not fmt(y - hi) in fragment order / rows >= T written"
            _, hi2, lo2, _, _ = _run_packed(lib, fmt, x0, slab, s_in, g, gamma, beta, T, d, False, False)
            assert same_bits(hi2, hi) and same_bits(lo2, lo), f"{what}: planes differ without out_f32"


LN_ROWS = ["plain", "offset1e3", "channel1000", "constant3", "gamma_wide", "overflow"]


def ln_hard(d, kind, seed):
    """16 rows of one kind and their gamma / beta: unit rows offset by 1e3; one channel 1000x the rest; the constant 3 (variance 0);
    gamma over two decades; `overflow`: channels 7 / 9 at +-100 with gamma chosen (from the fp64 normalised value of row 0) so that
    |y| ~ 1e5 on channel 7 (past 65504, inside what hi + lo holds) and ~2e5 on channel 9 (past 65504 + 65520: lo = +-inf in fp16)"""
    x = randn(16, d, seed=seed)
    gamma, beta = 1.0 + randn(d, seed=seed + 1, scale=0.1), randn(d, seed=seed + 2, scale=0.1)
    if kind == "offset1e3":
        x += 1e3
    elif kind == "channel1000":
        x[:, 7] *= 1000.0
    elif kind == "constant3":
        x[:] = 3.0
    elif kind == "gamma_wide":
        gamma = 10.0 ** (2 * uniform(d, seed) - 1)
    elif kind == "overflow":
        x[:, 7], x[:, 9] = 100.0, -100.0
        z, _ = ln_ref(x[:1], torch.ones(d, device="cuda"), None)
        gamma[7], gamma[9] = 1e5 / float(z[0, 7].abs()), 2e5 / float(z[0, 9].abs())
    return x, gamma, beta


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", [256, 2048, 4096])
def test_resadd_ln_packed_hard_rows(lib, fmt, d):
    """the hard LayerNorm rows through the packed kernel: f32 value per element, planes exactly split2 of it; a constant row gives beta bit
    for bit; fp16 outputs past 65504 have hi = +-65504 and a finite lo, past 65504 + 65520 lo = +-inf - never NaN, at exactly the
    elements the fp64 reference puts there"""
    for i, kind in enumerate(LN_ROWS):
        x0, gamma, beta = ln_hard(d, kind, seed=1000 + 10 * i + d)
        x, hi, lo, y32, _ = _run_packed(lib, fmt, x0, None, 0, None, gamma, beta, 16, d, True, False)
        y, yb = ln_ref(x0, gamma, beta)
        check(y32[:16], y, yb, f"d {d} {kind}: LayerNorm f32", key=f"resadd_ln/{fmt}")
        eh, el = split_hl(y32[:16], fmt)
        assert same_bits(hi, _frag_expected(eh, 16, fmt, d)) and same_bits(lo, _frag_expected(el, 16, fmt, d)), f"d {d} {kind}: planes"
        assert not bool(torch.isnan(hi[:16 * d].float()).any() | torch.isnan(lo[:16 * d].float()).any()), f"d {d} {kind}: NaN in a plane"
        if kind == "constant3":
            assert same_bits(y32[:16], beta.expand(16, d))
        if kind == "overflow":
            past, far = y.abs() >= OVF["f16"], y.abs() >= F16_MAX + OVF["f16"]
            assert int(past.sum()) == 32 and int(far.sum()) == 16 and bool(past[:, 7].all()) and bool(far[:, 9].all())
            if fmt == "f16":
                s = eh.double() + el.double()
                assert bool((eh.double().abs()[past] == F16_MAX).all()) and bool(torch.isfinite(eh).all())
                assert torch.equal(torch.isinf(s), far) and bool((torch.sign(s[far]) == torch.sign(y[far])).all())
                check_pair(eh, el, y, yb, fmt, f"d {d} overflow: hi + lo", key=f"resadd_pair/{fmt}")
        else:
            check_pair(eh, el, y, yb, fmt, f"d {d} {kind}: hi + lo", key=f"resadd_pair/{fmt}")


def test_resadd_ln_packed_exit_flag_and_refusals(lib):
    d, T = 256, 5
    for fmt in FMTS:
        x0, gamma = randn(T, d, seed=1), torch.ones(d, device="cuda")
        slab = randn(2, 16, d, seed=2)
        x, hi, lo, y32 = x0.clone(), nans(16 * d, dtype=TDT[fmt]), nans(16 * d, dtype=TDT[fmt]), nans(T, d)
        abi.check(_resadd_packed(lib, fmt, x, slab, 2, 16 * d, None, gamma, None, hi, lo, y32, None, T, d, ctl=ctl_block(True)), "resadd_ln_packed")
        sync()
        assert same_bits(x, x0) and all_nan(hi) and all_nan(lo) and all_nan(y32), "ALL_EXITED: something was written"
        ok = lambda **kw: _resadd_packed(lib, fmt, x, kw.get("slab", slab), kw.get("s_in", 2), 16 * d, None, kw.get("gamma", gamma), None,
                                         kw.get("hi", hi), kw.get("lo", lo), y32, None, kw.get("T", T), kw.get("d", d), ctl=ctl_block(True))
        assert ok() == 0
        for bad in (dict(T=0), dict(T=17), dict(d=48), dict(d=4128), dict(s_in=0), dict(gamma=None), dict(hi=None), dict(lo=None)):
            assert ok(**bad) == SHAPE, bad


# ================================================================================================ 2. deer_trunk_wide_gemm
WIDE_SHAPES = [(256, 768), (256, 1024), (2048, 6144), (2048, 8192), (4096, 12288), (4096, 16384), (256, 32), (2048, 32), (4096, 32)]


def _weights(lib, fmt, N, K, seed, kind="plain"):
    """[N, K] in the operand format and its packed form.  `shared`: the 32 columns of a moment group share a component 300x their own part,
    so a row's mean over the group is >= 100x its spread (what an uncentred second moment cannot survive)"""
    W = randn(N, K, seed=seed, scale=K ** -0.5)
    if kind == "shared":
        W = 0.003 * W + randn(N // 32, 1, K, seed=seed + 1, scale=K ** -0.5).expand(N // 32, 32, K).reshape(N, K)
    W = W.to(TDT[fmt])
    return W, pack(lib, W)


def _wide(lib, fmt, ph, pl, Wp, N, K, epi, T, ldo=None, ctl=None, rows=18):
    """one launch into NaN-filled buffers with two extra rows, 32 extra columns and one extra moment group"""
    ldo = ldo or N + 32
    out = nans(rows, ldo)
    oh, ol = nans(rows, ldo, dtype=TDT[fmt]), nans(rows, ldo, dtype=TDT[fmt])
    stats = nans(N // 32 + 1, 16, 2)
    rc = fn(lib, fmt, "deer_trunk_wide_gemm")(abi.ptr(ph), abi.ptr(pl), abi.ptr(Wp), N, K, epi, abi.ptr(out), abi.ptr(oh), abi.ptr(ol), ldo,
                                              abi.ptr(stats), T, abi.ptr(ctl), st())
    sync()
    return rc, out, oh, ol, stats


def _untouched(out, oh, ol, stats, N, T, epi):
    """rows >= T, columns >= N and the moment group past the last keep their sentinels; so does every buffer the epilogue does not own"""
    f32, planes = (out,) if epi != 1 else (), (oh, ol) if epi == 1 else ()
    for b in f32 + planes:
        assert all_nan(b[T:]) and all_nan(b[:, N:]), f"epi {epi}: stored past row T / column N"
    for b in (set((out, oh, ol)) - set(f32 + planes)):
        assert all_nan(b), f"epi {epi}: wrote a buffer of another epilogue"
    assert all_nan(stats[N // 32:]) and (epi == 2 or all_nan(stats))


def moments_ref(v):
    """fp64 mean and centred sum of squares of f32 values over groups of 32 (last axis) and the bound of the kernel's f32 arithmetic
    (csrc/trunk_r16.hip:95-103): the sum is a 5-level butterfly (5 roundings, each <= 2^-24 sum|v|) and an exact / 32:
    |dmu| <= 6 2^-24 mean|v|; the centred squares about the f32 mean give M2 + 32 dmu^2 (the cross term vanishes), each term with a rounded
    subtraction and square, summed over 5 levels: relative 10 2^-24"""
    v = v.double()
    mu = v.mean(-1)
    m2 = ((v - mu.unsqueeze(-1)) ** 2).sum(-1)
    bmu = 6 * 2.0 ** -24 * v.abs().mean(-1) + 1e-45
    return mu, m2, bmu, 10 * 2.0 ** -24 * m2 + 32 * bmu ** 2 + 1e-37


def check_moments(stats, out, T, N, what, fmt):
    """the moments of deer_trunk_wide_gemm(epi 2) against the fp64 moments of the kernel's own out_f32, per (group, row < T).  (The kernel
    writes moments for all 16 rows - csrc/trunk_r16.hip:103 - from accumulators of plane rows it does not own: rows >= T are not gated.)"""
    mu, m2, bmu, bm2 = moments_ref(out[:T, :N].reshape(T, N // 32, 32))
    check(stats[:N // 32, :T, 0].t(), mu, bmu, f"{what}: group mean", key=f"wide_moments/{fmt}")
    check(stats[:N // 32, :T, 1].t(), m2, bm2, f"{what}: centred sum of squares", key=f"wide_moments/{fmt}")
    return mu, m2


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K,N", WIDE_SHAPES)
def test_trunk_wide_gemm(lib, fmt, K, N):
    """every T, the three epilogues, operand planes once with zero rows above T and once with NaN / inf / 65504 there: rows < T bit-identical
    between the two, everything past T / N untouched.  epi 0 per element against fp64 ON THE TRUE f32 ACTIVATION (a dropped lo MFMA fails);
    epi 1 hi + lo against gelu(fp64) with the erf-GELU bound of the epi-0 error and a valid split; epi 2 the same f32 bits as epi 0 and the
    moments of those values.  Then planes with INDEPENDENT hi and lo (every MFMA of every k-tile carries weight at any K)"""
    A = randn(16, K, seed=K + N)
    W, Wp = _weights(lib, fmt, N, K, seed=K + N + 1)
    hi, lo = split_hl(A, fmt)
    ref, S = gemm_ref(A, W)
    e0 = pair_operand_err(W, S, fmt)
    g = F.gelu(ref)
    epis = (0, 1, 2) if K != 4096 else (0, 1)
    for T in ALL_T:
        res = {}
        for fill in ("zero", "poison"):
            ph, pl = pack_frag(hi, T, fmt, fill), pack_frag(lo, T, fmt, fill)
            for epi in epis:
                rc, out, oh, ol, stats = _wide(lib, fmt, ph, pl, Wp, N, K, epi, T)
                abi.check(rc, "trunk_wide_gemm")
                _untouched(out, oh, ol, stats, N, T, epi)
                res[fill, epi] = (out[:T, :N], oh[:T, :N], ol[:T, :N], stats[:N // 32, :T])
        for epi in epis:
            for a, b in zip(res["zero", epi], res["poison", epi]):
                assert same_bits(a, b), f"K {K} N {N} T {T} epi {epi}: rows >= T of the operand planes reached rows < T"
        what = f"K {K} N {N} T {T}"
        check(res["poison", 0][0], ref[:T], e0[:T], f"{what} epi 0", key=f"wide_f32/{fmt}")
        check_pair(res["poison", 1][1], res["poison", 1][2], g[:T], gelu_bound(ref[:T], g[:T], e0[:T]), fmt, f"{what} epi 1", key=f"wide_gelu/{fmt}")
        if 2 in epis:
            assert same_bits(res["poison", 2][0], res["poison", 0][0]), f"{what}: epi 2 and epi 0 give different f32 bits"
            check_moments(res["poison", 2][3].contiguous(), res["poison", 2][0], T, N, what, fmt)
    if K == 4096:
        ph, pl = pack_frag(hi, 16, fmt, "zero"), pack_frag(lo, 16, fmt, "zero")
        assert _wide(lib, fmt, ph, pl, Wp, N, K, 2, 16)[0] == SHAPE, "epi 2 at K = 4096 must be refused"
    h2, l2 = randn(16, K, seed=K + N + 2).to(TDT[fmt]), randn(16, K, seed=K + N + 3).to(TDT[fmt])
    r2, S2 = gemm_ref(h2.double() + l2.double(), W)
    S2 = (h2.double().abs() + l2.double().abs()) @ W.double().abs().t()
    for T in (5, 16):
        rc, out, oh, ol, stats = _wide(lib, fmt, pack_frag(h2, T, fmt, "poison"), pack_frag(l2, T, fmt, "poison"), Wp, N, K, 0, T)
        abi.check(rc, "trunk_wide_gemm")
        check(out[:T, :N], r2[:T], ACC * S2[:T] + 1e-30, f"K {K} N {N} T {T} independent planes", key=f"wide_f32/{fmt}")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", [256, 2048])
def test_trunk_wide_gemm_moments_of_offset_groups(lib, fmt, K):
    """weights whose 32-column groups share a component: a row's group mean is >= 100x its spread over the group in most groups; the centred
    sum of squares must still hold its relative bound (an uncentred E[v^2] - mean^2 in f32 is off by ~2^-24 32 mean^2 >> the bound)"""
    N = 3 * K
    A = randn(16, K, seed=77)
    W, Wp = _weights(lib, fmt, N, K, seed=78, kind="shared")
    hi, lo = split_hl(A, fmt)
    ref, S = gemm_ref(A, W)
    for T in (1, 9, 16):
        rc, out, oh, ol, stats = _wide(lib, fmt, pack_frag(hi, T, fmt, "poison"), pack_frag(lo, T, fmt, "poison"), Wp, N, K, 2, T)
        abi.check(rc, "trunk_wide_gemm")
        _untouched(out, oh, ol, stats, N, T, 2)
        check(out[:T, :N], ref[:T], pair_operand_err(W, S, fmt)[:T], f"K {K} T {T} shared-component weights", key=f"wide_f32/{fmt}")
        mu, m2 = check_moments(stats, out, T, N, f"K {K} T {T} offset groups", fmt)
        far = mu.abs() >= 100 * torch.sqrt(m2 / 32)
        assert float(far.double().mean()) > 0.25, "the case lost its offset groups"


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", [256, 2048, 4096])
def test_trunk_wide_gemm_hard_operands(lib, fmt, K):
    """one activation channel 1000x the rest, weight columns scaled so that the outputs span 1e-3 .. 3e5 in both signs: epi 0 per element
    (ACC_HARD), epi 1 with fp16 GELU results past 65504 (hi = +-65504, lo the rest, never NaN) on the 32-column (K <= 2048) and the
    16-column (K = 4096) form, and large negative pre-activations (GELU -> -0.0 / 0).  The counts come from the fp64 reference"""
    N = 1024
    A = randn(16, K, seed=31)
    A[:, 5] *= 1000.0
    W0 = randn(N, K, seed=32, scale=K ** -0.5)
    rms = (A @ W0.t()).pow(2).mean(0).sqrt()
    spread = torch.logspace(-3, 5.5, N, device="cuda")[torch.randperm(N, generator=torch.Generator().manual_seed(3)).cuda()]
    W = (W0 * (spread / rms)[:, None]).to(TDT[fmt])
    Wp = pack(lib, W)
    hi, lo = split_hl(A, fmt)
    ref, S = gemm_ref(A, W)
    e0 = pair_operand_err(W, S, fmt, ACC_HARD[fmt])
    g = F.gelu(ref)
    assert int((g >= OVF["f16"]).sum()) > 20 and int((ref < -10).sum()) > 1000 and int((ref.abs() < 1e-2).sum()) > 100
    for T in (7, 16):
        ph, pl = pack_frag(hi, T, fmt, "poison"), pack_frag(lo, T, fmt, "poison")
        rc, out, oh, ol, stats = _wide(lib, fmt, ph, pl, Wp, N, K, 0, T)
        abi.check(rc, "trunk_wide_gemm")
        check(out[:T, :N], ref[:T], e0[:T], f"K {K} T {T} hard epi 0", key=f"wide_f32_hard/{fmt}")
        rc, out, oh, ol, stats = _wide(lib, fmt, ph, pl, Wp, N, K, 1, T)
        abi.check(rc, "trunk_wide_gemm")
        _untouched(out, oh, ol, stats, N, T, 1)
        eg = gelu_bound(ref[:T], g[:T], e0[:T])
        check_pair(oh[:T, :N], ol[:T, :N], g[:T], eg, fmt, f"K {K} T {T} hard epi 1", key=f"wide_gelu_hard/{fmt}")
        neg = ref[:T] + e0[:T] < -10
        assert bool(((oh[:T, :N].double() + ol[:T, :N].double())[neg].abs() <= 1e-20).all()), "GELU of x < -10 is not 0"
        if fmt == "f16":
            # which elements saturate / overflow, from the reference alone: hi = 65504 from 65488 (the midpoint below 65504) upwards, lo = inf
            # from 65504 + 65520; only elements whose reference lies within its own bound of such an edge may fall on either side
            gT = g[:T]
            sat, inf = oh[:T, :N].double().abs() == F16_MAX, torch.isinf(ol[:T, :N].double())
            for got, edge, name in ((sat, 65488.0, "hi = 65504"), (inf, F16_MAX + OVF["f16"], "lo = inf")):
                clear = (gT - edge).abs() > eg
                assert int((gT >= edge).sum()) > 0, name
                assert torch.equal(got[clear], (gT >= edge)[clear]), f"K {K} T {T}: {name} at {int(got[clear].sum())} elements, reference {int((gT >= edge)[clear].sum())}"


def test_trunk_wide_gemm_exit_flag_and_refusals(lib):
    """ALL_EXITED: nothing written.  Refusals, every other operand valid in each case (tests/test_hip_ops.py::test_abi_rejects_bad_shapes)"""
    for fmt in FMTS:
        K, N = 256, 64
        A = randn(16, K, seed=41)
        W, Wp = _weights(lib, fmt, N, K, seed=42)
        hi, lo = split_hl(A, fmt)
        ph, pl = pack_frag(hi, 16, fmt, "zero"), pack_frag(lo, 16, fmt, "zero")
        for epi in (0, 1, 2):
            rc, out, oh, ol, stats = _wide(lib, fmt, ph, pl, Wp, N, K, epi, 16, ctl=ctl_block(True))
            assert rc == 0 and all_nan(out) and all_nan(oh) and all_nan(ol) and all_nan(stats), f"ALL_EXITED epi {epi}: something was written"
            rc, out, oh, ol, stats = _wide(lib, fmt, ph, pl, Wp, N, K, epi, 16, ctl=ctl_block(False))
            assert rc == 0 and not all_nan(oh if epi == 1 else out)
        f = fn(lib, fmt, "deer_trunk_wide_gemm")
        out, oh, ol, stats = nans(16, N), nans(16, N, dtype=TDT[fmt]), nans(16, N, dtype=TDT[fmt]), nans(N // 32, 16, 2)
        big = pack_frag(randn(16, 4096, seed=43).to(TDT[fmt]), 16, fmt, "zero")        # planes wide enough for every K tried below
        Wbig = torch.zeros(64 * 4096, dtype=TDT[fmt], device="cuda")

        def call(a_hi=big, a_lo=big, w=Wbig, N=N, K=K, epi=0, o=out, h=oh, l=ol, ldo=N, s=stats, T=16):
            return f(abi.ptr(a_hi), abi.ptr(a_lo), abi.ptr(w), N, K, epi, abi.ptr(o), abi.ptr(h), abi.ptr(l), ldo, abi.ptr(s), T, abi.ptr(ctl_block(True)), st())
        assert call() == 0 and call(epi=1) == 0 and call(epi=2) == 0 and call(K=2048) == 0 and call(K=4096) == 0
        for bad in (dict(T=0), dict(T=17), dict(N=48), dict(N=0), dict(K=512), dict(K=1024), dict(K=8192), dict(epi=3), dict(epi=-1),
                    dict(epi=1, ldo=N + 1), dict(a_hi=None), dict(a_lo=None), dict(w=None), dict(o=None), dict(epi=1, h=None), dict(epi=1, l=None),
                    dict(epi=2, s=None), dict(epi=2, o=None), dict(epi=2, K=4096)):
            assert call(**bad) == SHAPE, bad
        sync()


# ================================================================================================ 3. deer_trunk_mpt_attn
def mpt_ref(qkv, d, H, gq, gk, mask, bias_max, T):
    """fp64 MPT attention of one environment on f32 q|k|v [T, 3d]: q/k LayerNorm over the full row, score = q k / sqrt(hd) - (T - 1 - j)
    2^(-bias_max (h + 1) / H), causal, key mask; and the bound of the kernel's f32 arithmetic (csrc/trunk_r16.hip:183-346):
    q^, k^: the LayerNorm bound of ln_ref per element (eq, ek; the statistics come from 32-column moments combined by Chan's formula);
    score:  es = sc (eq |k^| + |q^| ek + eq ek summed over the head) + (hd / 4 + 4) 2^-24 sc sum|q^ k^| (hd / 4 products per lane, two
            shuffles, the scale) + 2^-23 |s| + 2^-21 alibi (exp2f of the slope, its product, the subtraction);
    softmax: with E = the largest es of the row's visible keys every normalised p_j is within exp(+-2 E) of fp64; expf of numerator and
            denominator, the 4-level sum and the division: 2^-20; the rounding of s_j - max: 2^-23 (max - s_j) relative on p_j;
    P V:    <= 16 sequential multiply-adds: (T + 2) 2^-24 sum_j p_j |v_j|; products that underflow f32: 2^-120 sum_j |v_j|.
    Returns o [T, d], its bound, and the rows that see no unmasked key (NaN in this reference's softmax)"""
    hd = d // H
    q, k, v = qkv[:T].double().chunk(3, -1)
    eq = ek = torch.zeros_like(q)
    if gq is not None:
        q, eq = ln_ref(q, gq, None)
        k, ek = ln_ref(k, gk, None)
    hs = lambda t: t.reshape(T, H, hd).transpose(0, 1)
    q, k, v, eq, ek = hs(q), hs(k), hs(v), hs(eq), hs(ek)
    sc = hd ** -0.5
    kt, akt = k.transpose(-1, -2), k.abs().transpose(-1, -2)
    slopes = 2.0 ** (-bias_max * torch.arange(1, H + 1, device="cuda", dtype=torch.float64) / H)
    alibi = (T - 1 - torch.arange(T, device="cuda", dtype=torch.float64)).view(1, 1, T) * slopes.view(H, 1, 1)
    s = (q @ kt) * sc - alibi
    es = sc * (eq @ akt + q.abs() @ ek.transpose(-1, -2) + eq @ ek.transpose(-1, -2)) + (hd / 4 + 4) * 2.0 ** -24 * sc * (q.abs() @ akt) \
        + 2.0 ** -23 * s.abs() + 2.0 ** -21 * alibi
    vis = torch.ones(T, T, dtype=torch.bool, device="cuda").tril()
    if mask is not None:
        vis = vis & mask.bool().view(1, T)
    blind = ~vis.any(-1)
    vis = vis | blind.view(T, 1)                              # (keeps the arithmetic finite; these rows are asserted NaN by the caller)
    sm = s.masked_fill(~vis, -math.inf)
    m = sm.amax(-1, keepdim=True)
    p = torch.exp(sm - m)
    p = p / p.sum(-1, keepdim=True)
    E = es.masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    rp = torch.expm1(2 * E) + 2.0 ** -20 + 2.0 ** -23 * (m - sm).masked_fill(~vis, 0.0)
    av = v.abs()
    o = p @ v
    eo = (p * rp) @ av + (T + 2) * 2.0 ** -24 * (p @ av) + 2.0 ** -120 * av.sum(-2, keepdim=True)
    back = lambda t: t.transpose(0, 1).reshape(T, d)
    return back(o), back(eo), blind, (sm, m)


ATTN_CFG = [(256, 64), (256, 32), (768, 32), (2048, 32), (256, 4), (2048, 16), (4096, 32), (256, 2)]     # head widths 4, 8, 24, 64, 64, 128, 128, 128
ATTN_FAMS = ["plain", "peaked", "equal", "alibi", "offset30"]


def attn_inputs(fam, T, d, H, qk_ln, seed):
    """q|k|v [T, 3d] f32 and the q / k LayerNorm weights.  peaked: q = a u, k_0 = a u, every other key = -a u + noise (u a sign pattern): key 0
    wins every row by > 80 with or without the LayerNorm (whose weights are then scaled so that g_q g_k sqrt(hd) = 100); equal: every key
    row the same, scores differ by ALiBi alone; alibi: q (or its LayerNorm weight) x 0.01, the bias decides; offset30: q, k rows of unit
    spread around 30 (under the LayerNorm only: the moments' cancellation case)"""
    hd = d // H
    qkv = randn(T, 3 * d, seed=seed) * 1.5 + 0.3
    gq, gk = 1.0 + randn(d, seed=seed + 1, scale=0.1), 1.0 + randn(d, seed=seed + 2, scale=0.1)
    if fam == "peaked":
        u = torch.sign(randn(d, seed=seed + 3))
        a = 1.0 if qk_ln else (100.0 / math.sqrt(hd)) ** 0.5
        qkv[:, :d] = a * (u + 0.05 * randn(T, d, seed=seed + 4))
        qkv[:, d:2 * d] = a * (-u + 0.05 * randn(T, d, seed=seed + 5))
        qkv[0, d:2 * d] = a * u
        gq, gk = gq * (100.0 / math.sqrt(hd)) ** 0.5, gk * (100.0 / math.sqrt(hd)) ** 0.5
    elif fam == "equal":
        qkv[:, d:2 * d] = qkv[:1, d:2 * d]
    elif fam == "alibi":
        qkv[:, :d] *= 0.01
        gq = gq * 0.01
    elif fam == "offset30":
        qkv[:, :2 * d] = 30.0 + randn(T, 2 * d, seed=seed + 6)
    return qkv, (gq if qk_ln else None), (gk if qk_ln else None)


def stats_of(qkv, T, d):
    """the moments deer_trunk_wide_gemm(epi 2) would write for q|k|v, computed in fp64 and rounded to f32 (rows >= T: NaN)"""
    g = qkv[:T].double().view(T, 3 * d // 32, 32)
    mu = g.mean(-1)
    stats = nans(3 * d // 32, 16, 2)
    stats[:, :T, 0] = mu.t().float()
    stats[:, :T, 1] = ((g - mu.unsqueeze(-1)) ** 2).sum(-1).t().float()
    return stats


def run_mpt(lib, fmt, qkv, stats, d, H, gq, gk, mask, bias_max, T, ctl=None, ldo=None):
    """hi / lo planes [18, ldo], NaN-filled"""
    ldo = ldo or d + 8
    hi, lo = nans(18, ldo, dtype=TDT[fmt]), nans(18, ldo, dtype=TDT[fmt])
    rc = fn(lib, fmt, "deer_trunk_mpt_attn")(abi.ptr(qkv), abi.ptr(stats), d, H, abi.ptr(gq), abi.ptr(gk), 1e-5, abi.ptr(mask), bias_max, abi.ptr(hi),
                                             abi.ptr(lo), ldo, T, abi.ptr(ctl), st())
    sync()
    return rc, hi, lo


def check_mpt(hi, lo, qkv, d, H, gq, gk, mask, bias_max, T, fmt, what, key):
    """the planes against mpt_ref.  A row that sees no unmasked key: MPT fills masked scores with the finite minimum (oracle/deer_oracle.py::
    mpt_attn_bias / mpt_block), so its softmax is uniform over ALL T keys, future ones included; the kernel fills with -inf and gives NaN.
    The engine cannot produce such a row (instructions are right-padded, key 0 is always valid - DESIGN.md section 2), so the kernel is
    kept and its NaN row asserted"""
    assert all_nan(hi[T:]) and all_nan(lo[T:]) and all_nan(hi[:, d:]) and all_nan(lo[:, d:]), f"{what}: stored past row T / column d"
    o, eo, blind, sm = mpt_ref(qkv, d, H, gq, gk, mask, bias_max, T)
    h, l = hi[:T, :d].clone(), lo[:T, :d].clone()
    if bool(blind.any()):
        assert all_nan(h[blind]) and all_nan(l[blind]), f"{what}: a row without a visible key is expected to be NaN"
        h[blind], l[blind], o[blind] = 0, 0, 0
    check_pair(h, l, o, eo, fmt, what, key=key)
    return int(blind.sum()), sm


def _masks(T):
    """(name, key mask or None): none; right padding of 1 .. T - 1 keys; a hole in the middle; key 0 masked"""
    out = [("none", None)]
    for pad in range(1, T):
        m = torch.ones(T, dtype=torch.uint8, device="cuda")
        m[T - pad:] = 0
        out.append((f"pad{pad}", m))
    if T >= 3:
        m = torch.ones(T, dtype=torch.uint8, device="cuda")
        m[T // 2] = 0
        out.append(("hole", m))
    if T >= 2:
        m = torch.ones(T, dtype=torch.uint8, device="cuda")
        m[0] = 0
        out.append(("key0", m))
    return out


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("qk_ln", [True, False], ids=["qkln", "noln"])
@pytest.mark.parametrize("d,H", ATTN_CFG, ids=[f"d{d}-hd{d // H}" for d, H in ATTN_CFG])
def test_trunk_mpt_attn(lib, fmt, d, H, qk_ln):
    """every T; the scalar (hd 4, 8, 24), float4 (64) and unrolled (128) dot products, 2 * lane >= hd for narrow heads, > 8 moment groups per
    thread at d = 4096; N(0, 1) scores with every mask, the other score shapes without a mask and with two padded keys; alibi_bias_max 8 / 16"""
    blind_rows = 0
    for T in ALL_T:
        for fam in ATTN_FAMS:
            if fam == "offset30" and not qk_ln:
                continue
            qkv, gq, gk = attn_inputs(fam, T, d, H, qk_ln, seed=1000 * T + 7 * ATTN_FAMS.index(fam) + d)
            buf = nans(18, 3 * d)
            buf[:T] = qkv
            stats = stats_of(qkv, T, d) if qk_ln else None
            bias_max = 16.0 if (T % 2 and fam in ("alibi", "plain")) else 8.0
            masks = _masks(T) if fam == "plain" else [mk for mk in _masks(T) if mk[0] in ("none", "pad2")]
            for mname, mask in masks:
                what = f"d {d} H {H} T {T} {fam} {mname}"
                rc, hi, lo = run_mpt(lib, fmt, buf, stats, d, H, gq, gk, mask, bias_max, T)
                abi.check(rc, "trunk_mpt_attn")
                nb, (sm, m) = check_mpt(hi, lo, buf, d, H, gq, gk, mask, bias_max, T, fmt, what, f"mpt_attn_{fam}/{fmt}")
                assert nb == (1 if mname == "key0" else 0), f"{what}: {nb} rows without a visible key"
                blind_rows += nb
                if fam == "peaked" and mname == "none" and T > 1:
                    gap = (m - sm)[:, 1:, 1:]                                 # rows >= 1: every visible key but key 0
                    assert float(gap[torch.isfinite(gap)].min()) > 80.0, f"{what}: the winning key leads by less than 80"
    assert blind_rows == 15


def test_trunk_mpt_attn_exit_flag_and_refusals(lib):
    for fmt in FMTS:
        T, d, H = 7, 256, 4
        qkv, gq, gk = attn_inputs("plain", T, d, H, True, seed=5)
        stats = stats_of(qkv, T, d)
        rc, hi, lo = run_mpt(lib, fmt, qkv, stats, d, H, gq, gk, None, 8.0, T, ctl=ctl_block(True))
        assert rc == 0 and all_nan(hi) and all_nan(lo), "ALL_EXITED: something was written"
        big = randn(16, 3 * 4096, seed=6)                         # q|k|v wide enough for every d tried below
        bstats = torch.zeros(3 * 4096 // 32, 16, 2, device="cuda")
        g = torch.ones(4096, device="cuda")
        f = fn(lib, fmt, "deer_trunk_mpt_attn")
        oh, ol = nans(16, 4096, dtype=TDT[fmt]), nans(16, 4096, dtype=TDT[fmt])

        def call(q=big, s=bstats, d=256, H=4, gq=g, gk=g, h=oh, l=ol, T=7):
            return f(abi.ptr(q), abi.ptr(s), d, H, abi.ptr(gq), abi.ptr(gk), 1e-5, None, 8.0, abi.ptr(h), abi.ptr(l), d, T, abi.ptr(ctl_block(True)), st())
        assert call() == 0 and call(gq=None, gk=None, s=None) == 0 and call(d=4096, H=32) == 0
        for bad in (dict(T=0), dict(T=17), dict(d=512, H=2), dict(d=256, H=128), dict(d=768, H=128), dict(d=384, H=6), dict(d=128, H=2),
                    dict(d=256, H=3), dict(gq=None), dict(gk=None), dict(s=None), dict(q=None), dict(h=None), dict(l=None)):
            assert call(**bad) == SHAPE, bad
        sync()


PAIR_CFG = [(256, 2), (256, 64), (2048, 16)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("kind", ["plain", "shared"])
@pytest.mark.parametrize("d,H", PAIR_CFG, ids=[f"d{d}-hd{d // H}" for d, H in PAIR_CFG])
def test_wide_gemm_feeds_mpt_attn(lib, fmt, d, H, kind):
    """THE PAIR the model runs: deer_trunk_wide_gemm(epi 2) writes q|k|v and the 32-column moments, deer_trunk_mpt_attn rebuilds the q/k
    LayerNorm from them (Chan's combination).  Reference: fp64 attention on the kernel's own f32 q|k|v, same bound as the kernel alone.
    Operand-plane rows >= T are poisoned, so q|k|v rows >= T stay NaN and the moments of those rows are NaN.  `shared`: weights whose moment
    groups sit far from the row mean (the between-group term 32 sum (mean_g - mean)^2 carries most of the variance)"""
    K, N = d, 3 * d
    A = randn(16, K, seed=91)
    W, Wp = _weights(lib, fmt, N, K, seed=92, kind=kind)
    hi, lo = split_hl(A, fmt)
    gq, gk = 1.0 + randn(d, seed=93, scale=0.1), 1.0 + randn(d, seed=94, scale=0.1)
    for T in ALL_T:
        rc, out, oh, ol, stats = _wide(lib, fmt, pack_frag(hi, T, fmt, "poison"), pack_frag(lo, T, fmt, "poison"), Wp, N, K, 2, T, ldo=N)
        abi.check(rc, "trunk_wide_gemm")
        assert all_nan(out[T:])
        masks = [mk for mk in _masks(T) if mk[0] in ("none", "pad1", "hole")]
        for mname, mask in masks:
            rc, ah, al = run_mpt(lib, fmt, out, stats, d, H, gq, gk, mask, 8.0, T)
            abi.check(rc, "trunk_mpt_attn")
            check_mpt(ah, al, out, d, H, gq, gk, mask, 8.0, T, fmt, f"pair d {d} H {H} T {T} {kind} {mname}", f"pair_gemm_attn/{fmt}")


# ================================================================================================ 4. deer_xattn_fused_packed / deer_xattn_fused
ACC_S = 2.0 ** -21      # a 64-term score: two chained 32-term MFMAs (tests/test_frame_kernels.py)
HEADS, INNER = 8, 512   # 8 heads of 64 (config.py: every configuration, the tiny test one included)
XSCALE = 0.125


def xattn_ref(xn, Wq, Wo, kk, vv, tt, npm, n_kv, fmt, T, tied=False):
    """fp64 gated cross attention per HEAD SLAB: y_h = softmax_media(q_h k_h^T) v_h Wo[:, h]^T [H, T, d], and the bound of the kernel's
    arithmetic (csrc/xattn_fused.hip):
    q:      f32 MFMA sums of xn as a hi + lo pair: (ACC + PAIR) sum|x w|; times the scale, rounded ONCE to the format: U |q| + TINY;
    scores: f32 MFMA of exact products: es = eq |k| summed over the head + ACC_S sum|q k|; keys outside the row's media get -FLT_MAX (a row
            past the last media sees every key: uniform), keys >= n_kv do not exist;
    P:      with every score within E (the row's largest es) the normalised p~_j = p_j e^dj / sum_l p_l e^dl, so p~_j - p_j = p_j sum_{l != j}
            p_l (e^dj - e^dl) / Z with Z >= e^-E: |p~_j - p_j| <= p_j (1 - p_j) (e^2E - 1) - the q rounding moves a one-hot row by nothing and
            a flat row by 2 E; v_exp and the rounded s - max: 2^-20 + 2^-23 (max - s); P rounded to the format: U relative - except the row's
            largest key, whose P is exp(0) = 1 exactly (taken as exact only where it leads the runner-up by more than 2 E, so that the
            kernel's largest key is the reference's) - and, fp16, 2^-25 absolute per probability (times |v| over the divisor >= 1); f32 MFMA
            of P V: ACC; divisor: the unrounded f32 sum and the reciprocal: |o| (n_kv 2^-24 + 2^-21);
            `tied` (every key row the same bits): the MFMA gives every key of a row the SAME score bits whatever q's error is, so every
            visible P is exactly 1: E = 0 and no P rounding - what is left is the o pair and the out-projection at PAIR / ACC level;
    o:      a hi + lo pair: PAIR |o| + TINY (fp16 past 65504: U of the excess);  out-projection: eo |Wo| + ACC sum|o Wo|.
    text_time 0: the row is exactly 0.  Returns y, its bound, the (head, row) whose scaled q reaches the format's overflow threshold, and
    o / the per-head Wo / the lead of each row's largest key over its runner-up (inf for a uniform or one-key row)"""
    d = xn.shape[1]
    x = xn[:T].double()
    Wq64, Wo64 = Wq.double(), Wo.double()
    q = x @ Wq64.t()
    eq = (ACC + PAIR[fmt]) * (x.abs() @ Wq64.abs().t()) + (TINY[fmt] * Wq64.abs().sum(-1) if fmt == "f16" else 0.0)
    qs = q * XSCALE
    eqs = XSCALE * eq + U[fmt] * qs.abs() + TINY[fmt]
    qovf = ((qs.abs() + eqs) >= OVF[fmt]).reshape(T, HEADS, 64).any(-1).t()          # [H, T]
    hs = lambda t, n: t.reshape(n, HEADS, 64).transpose(0, 1)
    qs, eqs, k, v = hs(qs, T), hs(eqs, T), hs(kk[:n_kv].double(), n_kv), hs(vv[:n_kv].double(), n_kv)
    s = qs @ k.transpose(-1, -2)
    es = eqs @ k.abs().transpose(-1, -2) + ACC_S * (qs.abs() @ k.abs().transpose(-1, -2))
    j = torch.arange(n_kv, device="cuda").view(1, n_kv)
    t = tt[:T].view(T, 1).long()
    vis = (j >= (t - 1) * npm) & (j < t * npm)
    none = ~vis.any(-1, keepdim=True)                            # every key at -FLT_MAX: exactly equal scores, a uniform row
    s, es, vis = s.masked_fill(none, 0.0), es.masked_fill(none, 0.0), vis | none
    sm = s.masked_fill(~vis, -math.inf)
    m = sm.amax(-1, keepdim=True)
    p = torch.exp(sm - m)
    D = p.sum(-1, keepdim=True)
    p = p / D
    E = es.masked_fill(~vis, 0.0).amax(-1, keepdim=True)
    top = sm.topk(min(2, n_kv), -1).values
    gap = (top[..., 0] - top[..., 1] if n_kv > 1 else torch.full_like(top[..., 0], math.inf)).masked_fill(none.view(1, T), math.inf)
    if tied:
        E, round_p = torch.zeros_like(E), 0.0
    else:
        exact1 = (sm == m) & (gap.unsqueeze(-1) > 2 * E + 1e-6)
        round_p = U[fmt] * (~exact1).double()
    rp = torch.expm1(2 * E) * (1 - p) + 2.0 ** -20 + 2.0 ** -23 * (m - sm).masked_fill(~vis, 0.0) + round_p + ACC
    av = v.abs()
    o = p @ v
    tiny_p = 2.0 ** -25 if fmt == "f16" else 2.0 ** -120
    eo = (p * rp) @ av + tiny_p * (vis.double() @ av) / D + o.abs() * (n_kv * 2.0 ** -24 + 2.0 ** -21)
    eo = eo + PAIR[fmt] * o.abs() + TINY[fmt] + (U[fmt] * (o.abs() - F16_MAX).clamp(min=0) if fmt == "f16" else 0.0)
    zero = (tt[:T] == 0).view(1, T, 1)
    o, eo = o.masked_fill(zero, 0.0), eo.masked_fill(zero, 0.0)
    Wo_h = Wo64.view(d, HEADS, 64).permute(1, 2, 0)              # [H, 64, d]
    y = o @ Wo_h
    ey = eo @ Wo_h.abs() + ACC * (o.abs() @ Wo_h.abs()) + 1e-30
    return y, ey, qovf, dict(o=o, Wo_h=Wo_h, gap=gap)


def xattn_operands(lib, fmt, d, n_kv, fam, seed):
    """Wq / Wo in the format (and packed), K / V of layer 1 of 3 inside a [130, 3 * 2 * inner] buffer whose other columns and rows >= n_kv are
    NaN.  tied: every key row the same (equal scores, o = mean of v).  peaked: key 3 of each media (keys 3 and 67) is, head by head, 120 x
    the unit vector of the scaled fp64 q of a base row; the test's rows are that base row + 10 % noise, so this key leads every other key of
    its media by ~100 (asserted > 80 from the reference's scores): P is 1 for it and underflows for the rest, o is one row of v"""
    Wq = randn(INNER, d, seed=seed, scale=d ** -0.5).to(TDT[fmt])
    Wo = randn(d, INNER, seed=seed + 1, scale=INNER ** -0.5).to(TDT[fmt])
    k, v = randn(n_kv, INNER, seed=seed + 2), randn(n_kv, INNER, seed=seed + 3)
    if fam == "peaked":
        qb = ((xattn_base(d).double() @ Wq.double().t()) * XSCALE).view(HEADS, 64)
        kstar = (120.0 * qb / qb.norm(dim=-1, keepdim=True)).reshape(INNER).float()
        for j in (3, 67):
            if j < n_kv:
                k[j] = kstar
    elif fam == "tied":
        k = k[:1].expand(n_kv, INNER).contiguous()
    ldkv = 3 * 2 * INNER
    kv = nans(130, ldkv, dtype=TDT[fmt])
    kv[:n_kv, 2 * INNER:3 * INNER] = k.to(TDT[fmt])
    kv[:n_kv, 3 * INNER:4 * INNER] = v.to(TDT[fmt])
    return Wq, Wo, pack(lib, Wq), pack(lib, Wo), kv, ldkv


def xattn_base(d):
    """the base row of the peaked family"""
    return randn(d, seed=4242 + d)


def xattn_rows(fam, T, d, seed):
    """LN(x) rows [T, d]: N(0, 1); peaked: the base row + 10 % noise"""
    x = randn(T, d, seed=seed)
    return xattn_base(d) + 0.1 * x if fam == "peaked" else x


def _kv_views(kv, n_kv):
    return kv[:n_kv, 2 * INNER:3 * INNER], kv[:n_kv, 3 * INNER:4 * INNER]


def _tt(T, shift):
    """text_time per row: before the first media (0: zero row), media 1, 2, and past the last media (5: every key masked -> uniform)"""
    pat = [1, 0, 2, 5, 1, 2, 1, 0, 2, 1, 5, 1, 2, 2, 1, 1, 0, 1, 2, 5]
    return torch.tensor([pat[(r + shift) % len(pat)] for r in range(T)], dtype=torch.int32, device="cuda")


def run_xattn(lib, fmt, packed, xn, planes, d, Wqp, Wop, kv, ldkv, tt, npm, n_kv, T, ctl=None):
    """head slabs [H][mpad + 1][d], NaN-filled (slab stride (mpad + 1) d: one sentinel row past the padded tile)"""
    mpad = abi.skinny_mpad(T)
    out = nans(HEADS, mpad + 1, d)
    kvp = abi.ptr(kv, 2 * INNER * 2)                            # layer 1's K|V columns
    if packed:
        rc = fn(lib, fmt, "deer_xattn_fused_packed")(abi.ptr(planes[0]), abi.ptr(planes[1]), d, abi.ptr(Wqp), kvp, ldkv, INNER, abi.ptr(tt), npm, n_kv,
                                                     abi.ptr(Wop), abi.ptr(out), (mpad + 1) * d, T, HEADS, XSCALE, abi.ptr(ctl), st())
    else:
        rc = fn(lib, fmt, "deer_xattn_fused")(abi.ptr(xn), d, abi.ptr(Wqp), kvp, ldkv, INNER, abi.ptr(tt), npm, n_kv, abi.ptr(Wop), abi.ptr(out),
                                              (mpad + 1) * d, T, HEADS, 1, XSCALE, abi.ptr(ctl), st())
    sync()
    return rc, out


def check_xattn(out, xn, Wq, Wo, kv, tt, npm, n_kv, fmt, T, what, key, expect_qovf=0, tied=False):
    assert all_nan(out[:, T:]), f"{what}: stored past row T"
    k, v = _kv_views(kv, n_kv)
    y, ey, qovf, extra = xattn_ref(xn, Wq, Wo, k, v, tt, npm, n_kv, fmt, T, tied=tied)
    assert int(qovf.sum()) == expect_qovf, f"{what}: {int(qovf.sum())} (head, row) with q past the overflow threshold"
    o = out[:, :T].clone()
    if expect_qovf:
        assert not bool(torch.isfinite(o[qovf]).all()), f"{what}: q * scale past 65504 is expected to overflow"
        o[qovf], y[qovf], ey[qovf] = 0, 0, 1.0                 # (the reference's own bound is inf - inf there)
    zero = tt[:T] == 0
    assert bool((o[:, zero] == 0).all()), f"{what}: a text_time 0 row is not exactly 0"
    for h in range(HEADS):
        check(o[h], y[h], ey[h], f"{what} head {h}", key=key)
    check(o.double().sum(0), y.sum(0), ey.sum(0), f"{what} sum of the head slabs", key=key)
    return y, ey, extra


XKV = [(64, 64), (128, 64), (1, 64), (50, 64), (127, 64)]        # (n_kv, n_per_media): the engine's call, two media, ragged counts


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", [256, 2048, 4096])
def test_xattn_fused_packed(lib, fmt, d):
    """every T, the engine's n_kv = n_per_media = 64, two media, ragged key counts; text_time 0 / 1 / 2 / past the last media in every
    launch; N(0, 1), peaked (one key of the row's media leads by > 80: a one-hot softmax) and tied scores (bounded at the level of the o
    pair: a dropped lo plane of o fails).  Each head slab per element against fp64, then their sum; and the packed form (plane rows
    >= T poisoned) bit for bit the f32-operand form"""
    one_hot_rows = 0
    for fi, fam in enumerate(["plain", "peaked", "tied"]):
        for n_kv, npm in XKV:
            Wq, Wo, Wqp, Wop, kv, ldkv = xattn_operands(lib, fmt, d, n_kv, fam, seed=10 * n_kv + fi + d)
            for T in ALL_T:
                what = f"d {d} n_kv {n_kv} T {T} {fam}"
                xn = nans(17, d)
                xn[:T] = xattn_rows(fam, T, d, seed=T + 100 * fi)
                hi, lo = split_hl(xn[:T], fmt)
                planes = (pack_frag(hi, T, fmt, "poison"), pack_frag(lo, T, fmt, "poison"))
                tt = _tt(T, T + n_kv)
                rc, out = run_xattn(lib, fmt, True, None, planes, d, Wqp, Wop, kv, ldkv, tt, npm, n_kv, T)
                abi.check(rc, "xattn_fused_packed")
                _, _, extra = check_xattn(out, xn, Wq, Wo, kv, tt, npm, n_kv, fmt, T, what, f"xattn_{fam}/{fmt}", tied=fam == "tied")
                if fam == "peaked":                                  # rows whose media holds the leading key (and another key beside it)
                    led = ((tt == 1) & (n_kv > 3)) | ((tt == 2) & (n_kv > 67))
                    if bool(led.any()):
                        assert float(extra["gap"][:, led].min()) > 80.0, f"{what}: the leading key leads by {float(extra['gap'][:, led].min()):.1f}"
                        one_hot_rows += int(led.sum())
                rc, out2 = run_xattn(lib, fmt, False, xn, None, d, Wqp, Wop, kv, ldkv, tt, npm, n_kv, T)
                abi.check(rc, "xattn_fused")
                assert same_bits(out, out2), f"{what}: packed form != f32-operand form"
    assert one_hot_rows == 299, one_hot_rows        # the rows of _tt with text_time 1 (n_kv 50 .. 128) or 2 (n_kv 127, 128) over T = 1 .. 16


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", [256, 2048, 4096])
def test_xattn_fused_one_environment(lib, fmt, d):
    """deer_xattn_fused at batch 1 with T = 1, 16, 17, 20, 32 (one and two row tiles)"""
    for n_kv, npm in [(64, 64), (128, 64), (50, 64)]:
        Wq, Wo, Wqp, Wop, kv, ldkv = xattn_operands(lib, fmt, d, n_kv, "plain", seed=7 * n_kv + d)
        for T in (1, 16, 17, 20, 32):
            xn = nans(T + 1, d)
            xn[:T] = randn(T, d, seed=T)
            tt = _tt(T, n_kv)
            rc, out = run_xattn(lib, fmt, False, xn, None, d, Wqp, Wop, kv, ldkv, tt, npm, n_kv, T)
            abi.check(rc, "xattn_fused")
            check_xattn(out, xn, Wq, Wo, kv, tt, npm, n_kv, fmt, T, f"fused d {d} n_kv {n_kv} T {T}", f"xattn_fused/{fmt}")


def test_xattn_fused_packed_f16_edges(lib):
    """fp16: V at +-65504 on head 0, so that o sits at the top of the format (a convex combination whose P were rounded up may pass
    65504: the pair saturates, nothing is NaN); one row of xn aligned with a row of Wq at 6e4, whose q * scale passes 65504 in f32 and
    overflows at the rounding as fp16 autocast would: the inf / NaN stays in that row of that head.  K stays N(0, 1): a K near 65504 overflows
    the scores themselves (q k ~ 1e5 per term), which the reference cannot define either.  In the second launch row 5 of heads 1 .. 7 has a q of
    ~7e3 and E ~ 1e2: its bound is astronomically wide, so those seven rows are in effect only held to be finite; every other row keeps its bound"""
    fmt, d, n_kv, T = "f16", 2048, 64, 16
    Wq, Wo, Wqp, Wop, kv, ldkv = xattn_operands(lib, fmt, d, n_kv, "plain", seed=3)
    kv[:n_kv, 3 * INNER:3 * INNER + 64] = 65504.0
    kv[:n_kv:3, 3 * INNER + 32:3 * INNER + 64] = -65504.0
    xn = randn(T, d, seed=4)
    tt = torch.ones(T, dtype=torch.int32, device="cuda")
    hi, lo = split_hl(xn, fmt)
    rc, out = run_xattn(lib, fmt, True, None, (pack_frag(hi, T, fmt, "poison"), pack_frag(lo, T, fmt, "poison")), d, Wqp, Wop, kv, ldkv, tt, 64, n_kv, T)
    abi.check(rc, "xattn_fused_packed")
    assert bool(torch.isfinite(out[:, :T]).all())
    check_xattn(out, xn, Wq, Wo, kv, tt, 64, n_kv, fmt, T, "V at +-65504", f"xattn_edges/{fmt}")
    xn[5] = 6e4 * torch.sign(Wq[3].float())
    hi, lo = split_hl(xn, fmt)
    rc, out = run_xattn(lib, fmt, True, None, (pack_frag(hi, T, fmt, "poison"), pack_frag(lo, T, fmt, "poison")), d, Wqp, Wop, kv, ldkv, tt, 64, n_kv, T)
    abi.check(rc, "xattn_fused_packed")
    check_xattn(out, xn, Wq, Wo, kv, tt, 64, n_kv, fmt, T, "q * scale past 65504 in row 5 of head 0", f"xattn_edges/{fmt}", expect_qovf=1)
    assert bool(torch.isfinite(out[1:, :T]).all()) and bool(torch.isfinite(out[0, [r for r in range(T) if r != 5]]).all())


def test_xattn_fused_exit_flag_and_refusals(lib):
    for fmt in FMTS:
        d, n_kv, T = 256, 64, 9
        Wq, Wo, Wqp, Wop, kv, ldkv = xattn_operands(lib, fmt, d, n_kv, "plain", seed=9)
        xn = randn(16, d, seed=10)
        hi, lo = split_hl(xn, fmt)
        ph, pl = pack_frag(hi, T, fmt, "zero"), pack_frag(lo, T, fmt, "zero")
        tt = _tt(32, 0)
        for packed in (True, False):
            rc, out = run_xattn(lib, fmt, packed, xn, (ph, pl), d, Wqp, Wop, kv, ldkv, tt, 64, n_kv, T, ctl=ctl_block(True))
            assert rc == 0 and all_nan(out), "ALL_EXITED: something was written"
        f = fn(lib, fmt, "deer_xattn_fused_packed")
        out = nans(HEADS, 16, d)
        kvp = kv[:, 2 * INNER:]

        def call(h=ph, l=pl, d=d, wq=Wqp, kvb=kvp, ldkv=ldkv, inner=INNER, t=tt, npm=64, n_kv=n_kv, wo=Wop, o=out, stride=16 * d, T=T, heads=HEADS):
            return f(abi.ptr(h), abi.ptr(l), d, abi.ptr(wq), abi.ptr(kvb), ldkv, inner, abi.ptr(t), npm, n_kv, abi.ptr(wo), abi.ptr(o), stride, T, heads,
                     XSCALE, abi.ptr(ctl_block(True)), st())
        assert call() == 0
        for bad in (dict(T=0), dict(T=17), dict(n_kv=0), dict(n_kv=129), dict(heads=0), dict(heads=4), dict(inner=256), dict(d=192), dict(d=640),
                    dict(ldkv=ldkv + 4), dict(npm=0), dict(stride=T * d - 1), dict(h=None), dict(l=None), dict(wq=None), dict(kvb=None), dict(wo=None),
                    dict(o=None), dict(t=None)):
            assert call(**bad) == SHAPE, bad
        sync()


# ================================================================================================ 5. deer_gemm_skinny_hl at one row tile
SKINNY_SHAPES = [(256, 256), (256, 1024), (2048, 2048), (2048, 8192), (4096, 4096), (4096, 16384)]      # (N, K): out-proj / down-proj of d = 256, 2048, 4096


def run_skinny(lib, fmt, hi, lo, Wp, M, N, K, S, ctl=None):
    """slabs [S + 1][16][N]: NaN-filled, one sentinel slab behind the last; hi / lo: ROW-MAJOR planes [16, K] whose rows >= M are poisoned"""
    part = nans(S + 1, 16, N)
    rc = fn(lib, fmt, "deer_gemm_skinny_hl")(abi.ptr(hi), abi.ptr(lo), K, abi.ptr(Wp), abi.ptr(part), M, N, K, S, abi.ptr(ctl), st())
    sync()
    return rc, part


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("N,K", SKINNY_SHAPES)
def test_gemm_skinny_hl_one_row_tile(lib, fmt, N, K):
    """every T as M with the split-K of deer_skinny_hl_splitk: the slab SUM per element against fp64 on the true f32 activation with
    (ACC + PAIR) S - inside the 3e-5 norm gate tests/test_env_batch_ops.py puts on the same kernel at more rows; padded rows M .. 15 exactly
    zero in every slab; plane rows >= M poisoned; the slab behind the last untouched; two runs give the same bits; then independent hi / lo"""
    A = randn(16, K, seed=N + K)
    W, Wp = _weights(lib, fmt, N, K, seed=N + K + 1)
    ref, Sm = gemm_ref(A, W)
    e = pair_operand_err(W, Sm, fmt)
    h0, l0 = split_hl(A, fmt)
    for M in ALL_T:
        S = lib.deer_skinny_hl_splitk(M, N, K)
        hi, lo = poison(16, K, fmt), poison(16, K, fmt)
        hi[:M], lo[:M] = h0[:M], l0[:M]
        rc, part = run_skinny(lib, fmt, hi, lo, Wp, M, N, K, S)
        abi.check(rc, "gemm_skinny_hl")
        assert all_nan(part[S]), "stored past the last slab"
        assert bool((part[:S, M:] == 0).all()), f"N {N} K {K} M {M}: padded rows are not zero"
        check(part[:S, :M].double().sum(0), ref[:M], e[:M], f"N {N} K {K} M {M} S {S}: slab sum", key=f"skinny_hl/{fmt}")
        rc, part2 = run_skinny(lib, fmt, hi, lo, Wp, M, N, K, S)
        assert rc == 0 and same_bits(part, part2), f"N {N} K {K} M {M}: two runs differ"
    h2, l2 = randn(16, K, seed=N + K + 2).to(TDT[fmt]), randn(16, K, seed=N + K + 3).to(TDT[fmt])
    S = lib.deer_skinny_hl_splitk(16, N, K)
    rc, part = run_skinny(lib, fmt, h2, l2, Wp, 16, N, K, S)
    abi.check(rc, "gemm_skinny_hl")
    S2 = (h2.double().abs() + l2.double().abs()) @ W.double().abs().t()
    check(part[:S].double().sum(0), (h2.double() + l2.double()) @ W.double().t(), ACC * S2 + 1e-30, f"N {N} K {K} independent planes", key=f"skinny_hl/{fmt}")
    rc, part = run_skinny(lib, fmt, h2, l2, Wp, 16, N, K, S, ctl=ctl_block(True))
    assert rc == 0 and all_nan(part), "ALL_EXITED: something was written"


# ================================================================================================ 6. the gates bite
@pytest.mark.parametrize("fmt", FMTS)
def test_gates_reject_wrong_references(lib, fmt):
    """negative controls, one per family: the kernels' own (correct) results against a deliberately wrong reference must fail the checkers"""
    # LayerNorm: the one-pass variance E[x^2] - E[x]^2 in f32 on rows offset by 1e3; a plane with row and (k % 32) / 8 swapped in the address
    d = 2048
    x0, gamma, beta = ln_hard(d, "offset1e3", seed=5)
    x, hi, lo, y32, _ = _run_packed(lib, fmt, x0, None, 0, None, gamma, beta, 16, d, True, False)
    y, yb = ln_ref(x0, gamma, beta)
    check(y32[:16], y, yb, "unperturbed LayerNorm")
    mu = x0.mean(-1, keepdim=True)
    one_pass = (x0 - mu) * torch.rsqrt((x0 * x0).mean(-1, keepdim=True) - mu * mu + 1e-5) * gamma + beta
    with pytest.raises(AssertionError):
        check(one_pass, y, yb, "one-pass variance")
    eh, _ = split_hl(y32[:16], fmt)
    swapped = eh.view(16, d // 32, 4, 8).permute(1, 0, 2, 3).reshape(-1)[:16 * d]       # [kt][row][g][8] instead of [kt][g][row][8]
    assert same_bits(hi[:16 * d], pack_frag(eh, 16, fmt, "nan")) and not same_bits(hi[:16 * d], swapped)
    # wide GEMM: one element moved by 4x its bound; GELU planes against a reference 4 bounds away; one moment group shifted
    K, N, T = 256, 768, 16
    A = randn(16, K, seed=6)
    W, Wp = _weights(lib, fmt, N, K, seed=7)
    h, l = split_hl(A, fmt)
    ref, S = gemm_ref(A, W)
    e0 = pair_operand_err(W, S, fmt)
    ph, pl = pack_frag(h, T, fmt, "zero"), pack_frag(l, T, fmt, "zero")
    _, out, _, _, stats = _wide(lib, fmt, ph, pl, Wp, N, K, 2, T)
    _, _, oh, ol, _ = _wide(lib, fmt, ph, pl, Wp, N, K, 1, T)
    check(out[:T, :N], ref, e0, "unperturbed epi 0")
    bad = ref.clone()
    bad[11, 700] += 4 * e0[11, 700]
    with pytest.raises(AssertionError):
        check(out[:T, :N], bad, e0, "one element moved by 4 bounds")
    g = F.gelu(ref)
    eg = gelu_bound(ref, g, e0)
    check_pair(oh[:T, :N], ol[:T, :N], g, eg, fmt, "unperturbed epi 1")
    bad = g.clone()
    bad[3, 40] += 4 * (eg[3, 40] + PAIR[fmt] * g[3, 40].abs() + TINY[fmt])
    with pytest.raises(AssertionError):
        check_pair(oh[:T, :N], ol[:T, :N], bad, eg, fmt, "one GELU element moved by 4 bounds")
    with pytest.raises(AssertionError):                                   # hi alone is not the pair
        check_pair(oh[:T, :N], torch.zeros_like(ol[:T, :N]), g, eg, fmt, "lo plane dropped")
    with pytest.raises(AssertionError):                                   # a truncated hi with the matching lo is the value, but not a split
        tr = (bits(oh[:T, :N]) & ~1).view(TDT[fmt])
        check_pair(tr, (oh[:T, :N].float() + ol[:T, :N].float() - tr.float()).to(TDT[fmt]), g, eg, fmt, "hi truncated to an even significand")
    check_moments(stats, out, T, N, "unperturbed moments", fmt)
    s2 = stats.clone()
    s2[5, :, 0] += 8 * 6 * 2.0 ** -24 * out[:T, 160:192].abs().mean(-1)
    with pytest.raises(AssertionError):
        check_moments(s2, out, T, N, "one moment group shifted", fmt)
    v = out[:T, :N].reshape(T, N // 32, 32) + 100.0                       # uncentred second moment in f32 on groups 100 sigma from zero
    unc = stats.clone()
    unc[:N // 32, :, 1] = ((v * v).sum(-1) - 32 * v.mean(-1) ** 2).t()
    unc[:N // 32, :, 0] = v.mean(-1).t()
    with pytest.raises(AssertionError):
        check_moments(unc, (out[:T, :N] + 100.0), T, N, "uncentred sum of squares", fmt)
    # attention: a reference with the ALiBi slope of head h instead of h + 1; without the last key of each row's window
    d, H, T = 256, 4, 12
    qkv, gq, gk = attn_inputs("plain", T, d, H, True, seed=8)
    stats = stats_of(qkv, T, d)
    rc, ah, al = run_mpt(lib, fmt, qkv, stats, d, H, gq, gk, None, 8.0, T)
    check_mpt(ah, al, qkv, d, H, gq, gk, None, 8.0, T, fmt, "unperturbed attention", None)
    o, eo, _, _ = mpt_ref(qkv, d, H, gq, gk, None, 8.0 * (H - 1) / H, T)   # slopes 2^(-8 h' / H) with h' = (h + 1)(H - 1) / H: every head moved
    with pytest.raises(AssertionError):
        check_pair(ah[:T, :d], al[:T, :d], o, eo, fmt, "wrong ALiBi slopes")
    m = torch.ones(T, dtype=torch.uint8, device="cuda")
    m[3] = 0
    o, eo, _, _ = mpt_ref(qkv, d, H, gq, gk, m, 8.0, T)
    with pytest.raises(AssertionError):
        check_pair(ah[:T, :d], al[:T, :d], o, eo, fmt, "reference with key 3 masked")
    # cross attention: two head slabs swapped; media window off by one media
    dx, n_kv, T = 256, 128, 16
    Wq, Wo, Wqp, Wop, kv, ldkv = xattn_operands(lib, fmt, dx, n_kv, "plain", seed=9)
    xn = randn(T, dx, seed=10)
    hh, ll = split_hl(xn, fmt)
    tt = _tt(T, 0)
    rc, xo = run_xattn(lib, fmt, True, None, (pack_frag(hh, T, fmt, "zero"), pack_frag(ll, T, fmt, "zero")), dx, Wqp, Wop, kv, ldkv, tt, 64, n_kv, T)
    check_xattn(xo, xn, Wq, Wo, kv, tt, 64, n_kv, fmt, T, "unperturbed x-attn", None)
    sw = xo.clone()
    sw[[2, 5]] = xo[[5, 2]]
    with pytest.raises(AssertionError):
        check_xattn(sw, xn, Wq, Wo, kv, tt, 64, n_kv, fmt, T, "head slabs 2 and 5 swapped", None)
    with pytest.raises(AssertionError):
        check_xattn(xo, xn, Wq, Wo, kv, torch.where(tt == 1, 2, tt).int(), 64, n_kv, fmt, T, "media 1 rows read media 2", None)
    # tied keys (the bound at the level of the o pair): one element moved by 4 bounds; the reference of a kernel that drops the lo plane of o
    Wq, Wo, Wqp, Wop, kv, ldkv = xattn_operands(lib, fmt, dx, n_kv, "tied", seed=13)
    rc, xo = run_xattn(lib, fmt, True, None, (pack_frag(hh, T, fmt, "zero"), pack_frag(ll, T, fmt, "zero")), dx, Wqp, Wop, kv, ldkv, tt, 64, n_kv, T)
    y, ey, extra = check_xattn(xo, xn, Wq, Wo, kv, tt, 64, n_kv, fmt, T, "unperturbed tied x-attn", None, tied=True)
    bad = y.clone()
    bad[4, 0, 17] += 4 * ey[4, 0, 17]
    with pytest.raises(AssertionError):
        check(xo[4, :T], bad[4], ey[4], "one element of head slab 4 moved by 4 bounds")
    hi_only = extra["o"].float().to(TDT[fmt]).double() @ extra["Wo_h"]
    with pytest.raises(AssertionError):
        for h in range(HEADS):
            check(xo[h, :T], hi_only[h], ey[h], "reference with o rounded to its hi plane")
    # skinny GEMM: one element of the slab sum moved by 4x its bound
    N, K, M = 256, 1024, 16
    W, Wp = _weights(lib, fmt, N, K, seed=11)
    A = randn(16, K, seed=12)
    h, l = split_hl(A, fmt)
    S = lib.deer_skinny_hl_splitk(M, N, K)
    rc, part = run_skinny(lib, fmt, h, l, Wp, M, N, K, S)
    ref, Sm = gemm_ref(A, W)
    e = pair_operand_err(W, Sm, fmt)
    check(part[:S].double().sum(0), ref, e, "unperturbed skinny")
    ref[9, 100] -= 4 * e[9, 100]
    with pytest.raises(AssertionError):
        check(part[:S].double().sum(0), ref, e, "one element moved by 4 bounds")
    with pytest.raises(AssertionError):
        check(part[:S - 1].double().sum(0), gemm_ref(A, W)[0], e, "one slab missing")


# ================================================================================================ 7. the engine refuses what the kernel cannot do
def test_engine_refuses_a_mask_without_key_0():
    """a mask whose key 0 is masked would leave query row 0 without a visible key (NaN in deer_trunk_mpt_attn, a uniform row in the reference):
    DeerEngine.load_inputs refuses it; the right-padded mask of the same instruction is taken"""
    from deer_vla_amd import synthetic as syn
    from deer_vla_amd.config import deer_tiny
    from deer_vla_amd.engine import DeerEngine
    cfg = deer_tiny()
    eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, 1, bf16_round=True), device="cuda:0")
    rgb, grip, ids, mask = syn.synthetic_step_inputs(cfg, 0)
    right = mask.clone().reshape(1, -1)
    right[:, -2:] = 0
    r = eng.step(rgb, grip, ids, right, exit_id=3, use_graph=False)
    assert bool(torch.isfinite(r["pose"]).all())
    left = mask.clone().reshape(1, -1)
    left[:, :2] = 0
    with pytest.raises(ValueError):
        eng.step(rgb, grip, ids, left, exit_id=3, use_graph=False)
