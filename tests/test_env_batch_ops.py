"""Per-kernel tests of the env-batch trunk (several environments through one engine): the entry points the batched / window / groups
paths run at every layer, called THROUGH THE C ABI (ctypes, raw device pointers) and compared with plain fp64 torch restatements of the
same operation, in both 16-bit formats (bf16 entry point and its `_f16` twin).  Row-map (`_active`) forms are compared bit for bit with
the map-free kernel on the same environment's inputs; the compaction gather of deer_resadd_ln_rows is checked word for word.  The last
section pins the fp16 overflow edge of the hi / lo activation planes (finite |v| >= 65520)."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from deer_vla_amd import _abi as abi  # noqa: E402

CMAP_N, CMAP_SLOT_ENV, CMAP_ENV_SLOT, CMAP_WORDS = 0, 1, 17, 64     # csrc/common.h
F16_MAX = 65504.0


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(t, dt=None):
    return t.to("cuda", dtype=dt).contiguous() if dt is not None else t.to("cuda").contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rel_err(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _fmt(dt):
    """(torch dtype, suffix of the C entry points) of a 16-bit operand format"""
    return (torch.float16, "_f16") if dt == "f16" else (torch.bfloat16, "")


def _fn(lib, dt, name_bf16, name_f16):
    """the entry point of the format (both names spelled out: every call site names the bf16 entry point and its fp16 twin)"""
    assert name_f16 == name_bf16 + "_f16"
    return getattr(lib, name_f16 if dt == "f16" else name_bf16)


def _pack(lib, W):
    Wp = torch.empty_like(W)
    abi.check(lib.deer_pack_weight_mfma16(abi.ptr(W), abi.ptr(Wp), W.shape[0], W.shape[1], st()), "pack")
    return Wp


def _split_hl(a, tdt):
    """the product's hi / lo split of f32 values (csrc/common.h: split2): fp16 hi saturates at +-65504, lo = fmt(a - hi)"""
    hi = (a.clamp(-F16_MAX, F16_MAX) if tdt == torch.float16 else a).to(tdt)
    return hi, (a - hi.float()).to(tdt)


def _half_ulp(hi):
    """1/2 ulp of every element of a 16-bit tensor (fp64; the subnormal spacing at 0 / below the smallest normal)"""
    p, emin = (10, -14) if hi.dtype == torch.float16 else (7, -126)
    h = hi.double().abs()
    e = torch.floor(torch.log2(torch.where(h > 0, h, torch.ones_like(h)))).clamp(min=emin)
    e = torch.where(h > 0, e, torch.full_like(e, emin))
    return torch.exp2(e - p - 1)


def _assert_split(hi, lo):
    """the two planes are a genuine split: |lo| <= 1/2 ulp(hi) elementwise"""
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    assert bool((lo.double().abs() <= _half_ulp(hi)).all()), float((lo.double().abs() / _half_ulp(hi)).max())


def _ctl(B):
    return torch.zeros(B * abi.CTL_WORDS, dtype=torch.int32, device="cuda")


def _cmap(B, slot_env):
    """row map (csrc/common.h CMAP_*): active slots in order, env -> slot (-1 = not active)"""
    m = torch.full((CMAP_WORDS,), -1, dtype=torch.int32)
    m[CMAP_N] = len(slot_env)
    for s, e in enumerate(slot_env):
        m[CMAP_SLOT_ENV + s] = e
        m[CMAP_ENV_SLOT + e] = s
    return m.cuda()


@pytest.fixture(scope="module")
def lib():
    l = abi.lib()
    assert l.deer_hip_arch() == b"gfx950"
    return l


# ------------------------------------------------------------------------------------ MPT attention, env batch, hi / lo planes
def _mpt_attn_ref(qkv, T, d, H, qw, kw, mask):
    """fp64 MPT attention of ONE environment (causal, ALiBi with bias_max 8, right-padded key mask), qkv [T, 3d]"""
    q, k, v = qkv.double().chunk(3, -1)
    if qw is not None:
        q = torch.nn.functional.layer_norm(q, (d,), qw.double(), None, 1e-5)
        k = torch.nn.functional.layer_norm(k, (d,), kw.double(), None, 1e-5)
    hd = d // H
    q, k, v = (t.reshape(T, H, hd).transpose(0, 1) for t in (q, k, v))
    slopes = 2.0 ** (-8.0 * torch.arange(1, H + 1, device=qkv.device, dtype=torch.float64) / H)
    bias = -(T - 1 - torch.arange(T, device=qkv.device, dtype=torch.float64)).view(1, 1, T) * slopes.view(H, 1, 1)
    w = q @ k.transpose(-1, -2) * hd ** -0.5 + bias
    w = w.masked_fill(~mask.bool().view(1, 1, T), float("-inf"))
    w = w.masked_fill(torch.ones(T, T, device=qkv.device).triu(1).bool(), float("-inf"))
    return (torch.softmax(w, -1) @ v).transpose(0, 1).reshape(T, d)


def _key_masks(B, T):
    """right-padded key masks, a different valid length per environment (>= 1)"""
    m = torch.zeros(B, T, dtype=torch.uint8)
    for b in range(B):
        m[b, :T - (3 * b) % T] = 1
    assert len({int(r.sum()) for r in m}) > 1
    return m.cuda()


SENT = 1234.0          # sentinel of rows a kernel must not write (exact in bf16 and fp16)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("B,T,d,H,qk_ln", [(2, 9, 256, 2, True), (3, 14, 2048, 16, True), (8, 32, 256, 2, False), (16, 14, 4096, 32, False),
                                           (8, 9, 4096, 32, False), (2, 32, 2048, 16, False), (16, 32, 256, 2, True)])
def test_mpt_attn_small_hl_env_batch(lib, dt, B, T, d, H, qk_ln):
    """deer_mpt_attn_small_hl(_f16) over B environments with their own key masks: the planes are a split of the output, hi + lo is the
    fp64 attention to f32-level error (the gate of test_mpt_attn_small's f32 output), rows past B*T keep their sentinel"""
    tdt, _ = _fmt(dt)
    s_in, R = 2, B * T
    mpad = abi.skinny_mpad(R)
    slab = dev(rnd(s_in, mpad, 3 * d, seed=101))
    qw, kw = (dev(1 + 0.1 * rnd(d, seed=102)), dev(1 + 0.1 * rnd(d, seed=103))) if qk_ln else (None, None)
    mask = _key_masks(B, T)
    ws = torch.zeros(R, 3 * d, device="cuda")
    hi = torch.full((R + 16, d), SENT, device="cuda", dtype=tdt)
    lo = torch.full_like(hi, SENT)
    abi.check(_fn(lib, dt, "deer_mpt_attn_small_hl", "deer_mpt_attn_small_hl_f16")(abi.ptr(slab), s_in, mpad * 3 * d, d, H, abi.ptr(qw), abi.ptr(kw), 1e-5, abi.ptr(mask), 8.0,
                                                     abi.ptr(ws), abi.ptr(hi), abi.ptr(lo), d, T, B, None, st()), "mpt attn hl")
    torch.cuda.synchronize()
    assert bool((hi[R:] == SENT).all()) and bool((lo[R:] == SENT).all())
    hi, lo = hi[:R], lo[:R]
    _assert_split(hi, lo)
    qkv = slab.sum(0)[:R]
    ref = torch.cat([_mpt_attn_ref(qkv[b * T:(b + 1) * T], T, d, H, qw, kw, mask[b]) for b in range(B)])
    # every query row, padded ones included (right padding: a padded query attends to the valid keys before it, as in the reference)
    assert rel_err(hi.double() + lo.double(), ref) < 2e-5
    for b in range(B):
        n = int(mask[b].sum())
        assert rel_err(hi[b * T:b * T + n].double() + lo[b * T:b * T + n].double(), ref[b * T:b * T + n]) < 2e-5


# ------------------------------------------------------------------------------------ skinny GEMM above 128 rows
SKROWS = [(129, 6144, 2048), (129, 16384, 4096), (200, 2048, 8192), (224, 12288, 4096), (256, 4096, 16384), (384, 6144, 2048),
          (512, 16384, 4096), (512, 2048, 8192)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", SKROWS)
def test_gemm_skinny_hl_rows_trunk_shapes(lib, dt, M, N, K):
    """deer_gemm_skinny_hl_rows(_f16) (row blocks of <= 128 rows into slabs of slab_rows rows) on the 3B / 9B trunk projections against
    fp64 on the same 16-bit weights, with the gate of test_gemm_skinny_hl_env_batch_kernel; padded rows zero, the slab tail untouched"""
    tdt, _ = _fmt(dt)
    a = dev(rnd(M, K, seed=111))
    hi, lo = _split_hl(a, tdt)
    W = dev(rnd(N, K, seed=112, scale=K ** -0.5), tdt)
    Wp = _pack(lib, W)
    S = lib.deer_skinny_hl_splitk(min(M, 128), N, K)
    mpad = abi.skinny_mpad(M)
    slab_rows = mpad + 16                                      # a tail of sentinel rows in every slab
    part = torch.full((S, slab_rows, N), 7.25, device="cuda")
    abi.check(_fn(lib, dt, "deer_gemm_skinny_hl_rows", "deer_gemm_skinny_hl_rows_f16")(abi.ptr(hi), abi.ptr(lo), K, abi.ptr(Wp), abi.ptr(part), M, N, K, S, slab_rows, None, st()),
              "skinny_hl_rows")
    torch.cuda.synchronize()
    y = part[:, :M].sum(0)
    assert torch.isfinite(y).all()
    assert rel_err(y, a.double() @ W.double().t()) < 3e-5
    if mpad > M:
        assert float(part[:, M:mpad].abs().max()) == 0.0
    assert bool((part[:, mpad:] == 7.25).all())


# ------------------------------------------------------------------------------------ GELU -> hi / lo planes
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("gelu", [1, 0])
def test_slab_gelu_split_planes_are_a_split(lib, dt, gelu):
    """deer_slab_gelu_split(_f16): hi + lo = act(sum of slabs) to the precision of the pair, |lo| <= 1/2 ulp(hi); exit flag honoured"""
    tdt, _ = _fmt(dt)
    rows, C, s_in = 112, 8192, 4
    slab = dev(rnd(s_in, rows, C, seed=121))
    hi = torch.full((rows, C), SENT, device="cuda", dtype=tdt)
    lo = torch.full_like(hi, SENT)
    abi.check(_fn(lib, dt, "deer_slab_gelu_split", "deer_slab_gelu_split_f16")(abi.ptr(slab), s_in, rows * C, gelu, abi.ptr(hi), abi.ptr(lo), rows, C, None, st()), "gelu_split")
    torch.cuda.synchronize()
    s = slab.double().sum(0)
    a = torch.nn.functional.gelu(s) if gelu else s
    _assert_split(hi, lo)
    # f32 slab sum + f32 erf GELU: a few f32 ulps; the pair itself carries ~16 (bf16) / ~22 (fp16) bits
    gate = 1e-5 if dt == "bf16" else 1e-6
    assert float((hi.double() + lo.double() - a).abs().max()) < gate * float(a.abs().max())
    if not gelu:        # no transcendental: the planes are exactly the split of the f32 slab sum
        s32 = slab[0] + slab[1] + slab[2] + slab[3]
        rh, rl = _split_hl(s32, tdt)
        assert torch.equal(hi, rh) and torch.equal(lo, rl)
    ctl = _ctl(1)
    ctl[abi.CTL_ALL_EXITED] = 1
    h2 = torch.full_like(hi, SENT)
    abi.check(_fn(lib, dt, "deer_slab_gelu_split", "deer_slab_gelu_split_f16")(abi.ptr(slab), s_in, rows * C, gelu, abi.ptr(h2), abi.ptr(lo), rows, C, abi.ptr(ctl), st()), "gelu_split")
    torch.cuda.synchronize()
    assert bool((h2 == SENT).all())


# ------------------------------------------------------------------------------------ row-map (_active) forms
B_MAP, SLOT_ENV = 7, [5, 0, 3, 6]        # 4 active slots of 7 environments, permuted; environments 1, 2, 4 have left


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("d", [256, 2048, 4096])
def test_active_forms_equal_the_map_free_kernels_per_environment(lib, dt, d):
    """skinny_hl_active, slab_gelu_split_active, mpt_attn_small_hl_active and xattn_fused_active under a hand-built row map: the rows of
    active slot s (environment e) are bit for bit what the map-free kernel gives on e's inputs (key mask, text_time, media K/V read in
    ENVIRONMENT order); rows of slots >= cmap[CMAP_N] keep their sentinel"""
    tdt, _ = _fmt(dt)
    B, T, n = B_MAP, 14, len(SLOT_ENV)
    R, RA = B * T, n * T
    cmap = _cmap(B, SLOT_ENV)
    ctl = _ctl(B)
    perm = torch.tensor(SLOT_ENV, device="cuda")
    rows_of = lambda x, per: x.view(-1, per, *x.shape[1:])[perm].reshape(-1, *x.shape[1:])   # environment-ordered blocks -> slot order

    # skinny_hl_active: the wide projection of this width (M = B*T launch geometry, RA rows active)
    N, K = 3 * d, d
    a = dev(rnd(R, K, seed=131))
    hi, lo = _split_hl(a, tdt)
    Wp = _pack(lib, dev(rnd(N, K, seed=132, scale=K ** -0.5), tdt))
    S = lib.deer_skinny_hl_splitk(min(R, 128), N, K)
    slab_rows = abi.skinny_mpad(R)
    pa = torch.full((S, slab_rows, N), 7.25, device="cuda")
    pr = torch.full_like(pa, 7.25)
    abi.check(_fn(lib, dt, "deer_gemm_skinny_hl_active", "deer_gemm_skinny_hl_active_f16")(abi.ptr(hi), abi.ptr(lo), K, abi.ptr(Wp), abi.ptr(pa), R, N, K, S, slab_rows, abi.ptr(ctl),
                                                         abi.ptr(cmap), T, st()), "skinny_hl_active")
    abi.check(_fn(lib, dt, "deer_gemm_skinny_hl_rows", "deer_gemm_skinny_hl_rows_f16")(abi.ptr(hi), abi.ptr(lo), K, abi.ptr(Wp), abi.ptr(pr), RA, N, K, S, slab_rows, None, st()),
              "skinny_hl_rows")
    torch.cuda.synchronize()
    assert torch.equal(pa[:, :RA], pr[:, :RA])
    mpa = abi.skinny_mpad(RA)
    assert float(pa[:, RA:mpa].abs().max() if mpa > RA else 0.0) == 0.0     # the last active 16-row tile's padding rows are zeros
    assert bool((pa[:, mpa:] == 7.25).all())

    # slab_gelu_split_active: the down-projection operand (C = 4 d)
    C, s_in = 4 * d, 3
    gslab = dev(rnd(s_in, R, C, seed=133))
    ha, la = torch.full((R, C), SENT, device="cuda", dtype=tdt), torch.full((R, C), SENT, device="cuda", dtype=tdt)
    hr, lr = torch.empty_like(ha), torch.empty_like(la)
    abi.check(_fn(lib, dt, "deer_slab_gelu_split_active", "deer_slab_gelu_split_active_f16")(abi.ptr(gslab), s_in, R * C, 1, abi.ptr(ha), abi.ptr(la), R, C, abi.ptr(ctl), abi.ptr(cmap), T,
                                                          st()), "gelu_split_active")
    abi.check(_fn(lib, dt, "deer_slab_gelu_split", "deer_slab_gelu_split_f16")(abi.ptr(gslab), s_in, R * C, 1, abi.ptr(hr), abi.ptr(lr), RA, C, None, st()), "gelu_split")
    torch.cuda.synchronize()
    assert torch.equal(ha[:RA], hr[:RA]) and torch.equal(la[:RA], lr[:RA])
    assert bool((ha[RA:] == SENT).all()) and bool((la[RA:] == SENT).all())

    # mpt_attn_small_hl_active: slabs by slot, key masks by environment
    H = d // 128
    qslab = dev(rnd(2, R, 3 * d, seed=134))
    mask = _key_masks(B, T)
    qw, kw = (dev(1 + 0.1 * rnd(d, seed=135)), dev(1 + 0.1 * rnd(d, seed=136))) if d != 4096 else (None, None)
    ws = torch.zeros(R, 3 * d, device="cuda")
    oa, ola = torch.full((R, d), SENT, device="cuda", dtype=tdt), torch.full((R, d), SENT, device="cuda", dtype=tdt)
    orf, olr = torch.empty_like(oa), torch.empty_like(ola)
    abi.check(_fn(lib, dt, "deer_mpt_attn_small_hl_active", "deer_mpt_attn_small_hl_active_f16")(abi.ptr(qslab), 2, R * 3 * d, d, H, abi.ptr(qw), abi.ptr(kw), 1e-5, abi.ptr(mask), 8.0,
                                                            abi.ptr(ws), abi.ptr(oa), abi.ptr(ola), d, T, B, abi.ptr(ctl), abi.ptr(cmap), st()), "attn_active")
    mask_slots = mask[perm].contiguous()
    ws2 = torch.zeros(RA, 3 * d, device="cuda")
    abi.check(_fn(lib, dt, "deer_mpt_attn_small_hl", "deer_mpt_attn_small_hl_f16")(abi.ptr(qslab), 2, R * 3 * d, d, H, abi.ptr(qw), abi.ptr(kw), 1e-5, abi.ptr(mask_slots), 8.0,
                                                     abi.ptr(ws2), abi.ptr(orf), abi.ptr(olr), d, T, n, None, st()), "attn")
    torch.cuda.synchronize()
    assert torch.equal(oa[:RA], orf[:RA]) and torch.equal(ola[:RA], olr[:RA])
    assert bool((oa[RA:] == SENT).all()) and bool((ola[RA:] == SENT).all())
    assert not torch.equal(mask[:n], mask_slots)              # (a mask read by slot would have given other rows)

    # xattn_fused_active: xn by slot, text_time and media K/V by environment
    heads, inner, n_kv = 8, 512, 64
    ldkv = 2 * inner
    xn = dev(rnd(R, d, seed=137))
    Wq_p = _pack(lib, dev(rnd(inner, d, seed=138, scale=d ** -0.5), tdt))
    Wo_p = _pack(lib, dev(rnd(d, inner, seed=139, scale=inner ** -0.5), tdt))
    kv = dev(rnd(B * n_kv, ldkv, seed=140), tdt)
    tt = torch.ones(B, T, dtype=torch.int32)
    for e in range(B):
        tt[e, :e % 3] = 0                                       # tokens before the first media -> zero rows (environment-specific)
        tt[e, T - 1 - e % 4:] = 2                               # a second media chunk
    tt = tt.cuda()
    mp = abi.skinny_mpad(R)
    xa = torch.full((heads, mp, d), 7.25, device="cuda")
    xr = torch.full((heads, abi.skinny_mpad(RA), d), 7.25, device="cuda")
    abi.check(_fn(lib, dt, "deer_xattn_fused_active", "deer_xattn_fused_active_f16")(abi.ptr(xn), d, abi.ptr(Wq_p), abi.ptr(kv), ldkv, inner, abi.ptr(tt), n_kv // 2, n_kv, abi.ptr(Wo_p),
                                                      abi.ptr(xa), mp * d, T, heads, B, 64 ** -0.5, abi.ptr(ctl), abi.ptr(cmap), st()), "xattn_active")
    kv_slots, tt_slots = rows_of(kv, n_kv).contiguous(), tt[perm].contiguous()
    xn_slots = xn[:RA].contiguous()
    abi.check(_fn(lib, dt, "deer_xattn_fused", "deer_xattn_fused_f16")(abi.ptr(xn_slots), d, abi.ptr(Wq_p), abi.ptr(kv_slots), ldkv, inner, abi.ptr(tt_slots), n_kv // 2, n_kv,
                                               abi.ptr(Wo_p), abi.ptr(xr), abi.skinny_mpad(RA) * d, T, heads, n, 64 ** -0.5, None, st()), "xattn")
    torch.cuda.synchronize()
    assert torch.isfinite(xa[:, :RA]).all()
    assert torch.equal(xa[:, :RA], xr[:, :RA])
    assert bool((xa[:, RA:] == 7.25).all())


# ------------------------------------------------------------------------------------ the compaction gather
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("d,with_beta", [(256, True), (2048, True), (4096, False)])
def test_resadd_ln_rows_gather_packs_the_survivors(lib, dt, d, with_beta):
    """deer_resadd_ln_rows with x_in / cmap_old / drop_upto (the first row op of a compaction layer): environments with EXIT_FLAG and
    EXIT_LAYER <= drop_upto leave, one that exited a layer too late stays, one already gone stays gone; the new map is exact; every packed
    row is the residual of its SOURCE row (slabs read there, x_copy written there) and its LayerNorm; rows past the survivors untouched"""
    tdt, _ = _fmt(dt)
    B, T, s_in, drop_upto = 7, 6, 3, 5
    old_slot_env = [4, 0, 5, 2, 1, 6]                         # environment 3 was dropped by an earlier compaction
    ctl = _ctl(B).view(B, abi.CTL_WORDS)
    for e, lay in ((0, drop_upto), (2, drop_upto - 2), (5, drop_upto + 1), (3, 1)):   # 0, 2 leave; 5 exited too late to drop; 3 long gone
        ctl[e, abi.CTL_EXIT_FLAG] = 1
        ctl[e, abi.CTL_EXIT_LAYER] = lay
    ctl = ctl.reshape(-1).contiguous()
    cmap_old = _cmap(B, old_slot_env)
    cmap = torch.full((CMAP_WORDS,), 99, dtype=torch.int32, device="cuda")
    n_old = len(old_slot_env)
    RO = n_old * T
    x_in = dev(rnd(RO, d, seed=151))
    slab = dev(rnd(s_in, RO, d, seed=152, scale=0.5))
    gate = torch.tensor([0.7], device="cuda")
    gamma = dev(1 + 0.1 * rnd(d, seed=153))
    beta = dev(0.1 * rnd(d, seed=154)) if with_beta else None
    x = torch.full((RO, d), 7.25, device="cuda")
    hi, lo = torch.full((RO, d), SENT, device="cuda", dtype=tdt), torch.full((RO, d), SENT, device="cuda", dtype=tdt)
    y32 = torch.full((RO, d), 7.25, device="cuda")
    xc = torch.full((RO, d), 7.25, device="cuda")
    abi.check(_fn(lib, dt, "deer_resadd_ln_rows", "deer_resadd_ln_rows_f16")(abi.ptr(x), abi.ptr(slab), s_in, RO * d, abi.ptr(gate), abi.ptr(gamma), abi.ptr(beta), abi.ptr(hi),
                                                  abi.ptr(lo), abi.ptr(y32), abi.ptr(xc), RO, d, 1e-5, abi.ptr(ctl), abi.ptr(cmap), T, abi.ptr(x_in),
                                                  abi.ptr(cmap_old), B, drop_upto, st()), "resadd_ln_rows gather")
    torch.cuda.synchronize()
    # the new map, word for word
    keep = [e for e in old_slot_env if e not in (0, 2)]
    assert keep == [4, 5, 1, 6]
    cm = cmap.cpu().tolist()
    assert cm[CMAP_N] == len(keep)
    assert cm[CMAP_SLOT_ENV:CMAP_SLOT_ENV + len(keep)] == keep
    assert cm[CMAP_ENV_SLOT:CMAP_ENV_SLOT + B] == [keep.index(e) if e in keep else -1 for e in range(B)]
    # packed rows from their source rows
    src = torch.cat([torch.arange(old_slot_env.index(e) * T, (old_slot_env.index(e) + 1) * T) for e in keep]).cuda()
    RN = len(keep) * T
    xr = x_in.double()[src] + math.tanh(0.7) * slab.double().sum(0)[src]
    assert float((x[:RN].double() - xr).abs().max()) <= 1e-6 * float(xr.abs().max())
    # bit for bit: the map-free row op on the source rows
    x_ref = x_in.clone()
    y_ref = torch.empty_like(y32)
    h_ref, l_ref = torch.empty_like(hi), torch.empty_like(lo)
    abi.check(_fn(lib, dt, "deer_resadd_ln_split", "deer_resadd_ln_split_f16")(abi.ptr(x_ref), abi.ptr(slab), s_in, RO * d, abi.ptr(gate), None, abi.ptr(gamma), abi.ptr(beta),
                                                   abi.ptr(h_ref), abi.ptr(l_ref), abi.ptr(y_ref), None, RO, d, 1e-5, None, st()), "resadd_ln_split")
    torch.cuda.synchronize()
    assert torch.equal(x[:RN], x_ref[src]) and torch.equal(y32[:RN], y_ref[src])
    assert torch.equal(hi[:RN], h_ref[src]) and torch.equal(lo[:RN], l_ref[src])
    # LayerNorm against fp64 (beta = None: MPT-7B's bias-free LayerNorm)
    ln = torch.nn.functional.layer_norm(xr, (d,), gamma.double(), None if beta is None else beta.double(), 1e-5)
    assert rel_err(y32[:RN], ln) < 1e-5
    _assert_split(hi[:RN], lo[:RN])
    assert rel_err(hi[:RN].double() + lo[:RN].double(), ln) < 1e-5
    # x_copy at the SOURCE rows, nothing at the sources of the dropped environments
    assert torch.equal(xc[src], x[:RN])
    dropped = torch.tensor([r for r in range(RO) if r not in set(src.tolist())], device="cuda")
    assert bool((xc[dropped] == 7.25).all())
    # destination rows past the survivors untouched
    assert bool((x[RN:] == 7.25).all()) and bool((y32[RN:] == 7.25).all())
    assert bool((hi[RN:] == SENT).all()) and bool((lo[RN:] == SENT).all())


# ------------------------------------------------------------------------------------ fp16 overflow edge of the hi / lo planes
def _gemm_f16(lib, hi, lo, W):
    M, K = hi.shape
    N = W.shape[0]
    S = lib.deer_skinny_hl_splitk(M, N, K)
    part = torch.full((S, abi.skinny_mpad(M), N), 7.25, device="cuda")      # a finite sentinel: a NaN below comes from the kernel's arithmetic
    abi.check(lib.deer_gemm_skinny_hl_f16(abi.ptr(hi), abi.ptr(lo), K, abi.ptr(_pack(lib, W)), abi.ptr(part), M, N, K, S, None, st()), "skinny_hl_f16")
    torch.cuda.synchronize()
    assert not bool((part[:, :M] == 7.25).all(-1).any()), "slab rows not written"
    return part.sum(0)[:M]


def _check_pair_and_product(lib, hi, lo, v, W, atol=0.0):
    """the fp16 GEMM of the pair is finite, equal to fp64 on the pair with the usual gate and to fp64 on v within the pair's error; the pair
    carries v: |hi + lo - v| <= 2^-11 |v| (1/2 ulp of lo, |lo| <= |v|) + 2^-25 (1/2 of fp16's smallest subnormal) + atol (the producer's
    own f32 error on small values)"""
    y = _gemm_f16(lib, hi, lo, W)
    assert not torch.isnan(y).any(), "NaN from the hi / lo MFMA pair"
    assert torch.isfinite(y).all()
    assert torch.isfinite(hi).all() and torch.isfinite(lo).all()
    pair = hi.double() + lo.double()
    assert bool(((pair - v.double()).abs() <= 2.0 ** -11 * v.double().abs() + 2.0 ** -25 + atol).all())
    assert rel_err(y, pair @ W.double().t()) < 3e-5
    assert rel_err(y, v.double() @ W.double().t()) < 2.0 ** -11


def test_f16_planes_of_gelu_slab_sums_beyond_65504(lib):
    """slab sums in [6e4, 1.3e5] (GELU(x) = x there) through deer_slab_gelu_split_f16 into deer_gemm_skinny_hl_f16: hi saturates at 65504,
    lo = fp16(v - hi); past ~1.31e5 the pair is +-inf (as .half() gives), never NaN"""
    rows, C = 32, 2048
    g = torch.Generator().manual_seed(161)
    mag = 6e4 + 7e4 * torch.rand(rows, C, generator=g)
    sign = torch.where(torch.rand(rows, C, generator=g) < 0.5, -1.0, 1.0)
    v = mag * sign
    v[::2] = torch.randn(rows // 2, C, generator=g) * 100      # ordinary rows beside them
    slab = dev(torch.stack([v * 0.25, v * 0.75]))
    hi = torch.empty(rows, C, device="cuda", dtype=torch.float16)
    lo = torch.empty_like(hi)
    abi.check(lib.deer_slab_gelu_split_f16(abi.ptr(slab), 2, rows * C, 1, abi.ptr(hi), abi.ptr(lo), rows, C, None, st()), "gelu_split_f16")
    torch.cuda.synchronize()
    v32 = slab[0] + slab[1]
    gv = torch.nn.functional.gelu(v32.double()).float()       # = v32 exactly for x >= 6e4, 0 for x <= -6e4
    W = dev(rnd(512, C, seed=162, scale=C ** -0.5), torch.float16)
    _check_pair_and_product(lib, hi, lo, gv, W, atol=1e-4)   # (f32 erf of the ordinary rows)
    pos = v32[1::2] > 0
    rh, rl = _split_hl(v32, torch.float16)
    assert torch.equal(hi[1::2][pos], rh[1::2][pos]) and torch.equal(lo[1::2][pos], rl[1::2][pos])
    # beyond what two fp16 values can hold: +-inf, not NaN (asserted on the planes: a zero weight times inf is NaN in fp64 as well)
    big = torch.tensor([1.4e5, -1.4e5, 1.5e5, -1.5e5, 2e5, -1e6, 1e7, -3e38, 3e38, 1.32e5, -1.32e5, 6e5], device="cuda")
    bslab = big.view(1, -1).contiguous()
    n = big.numel()
    bh = torch.empty(n, device="cuda", dtype=torch.float16)
    bl = torch.empty_like(bh)
    abi.check(lib.deer_slab_gelu_split_f16(abi.ptr(bslab), 1, n, 0, abi.ptr(bh), abi.ptr(bl), 1, n, None, st()), "gelu_split_f16")
    torch.cuda.synchronize()
    s = bh.float() + bl.float()
    assert not torch.isnan(bh).any() and not torch.isnan(bl).any()
    assert torch.equal(s, torch.where(big > 0, float("inf"), float("-inf")))
    assert torch.equal(bh.float().abs(), torch.full_like(s, F16_MAX))


def test_f16_planes_of_a_layernorm_output_beyond_65504(lib):
    """deer_resadd_ln_split_f16 on rows whose LayerNorm output exceeds 65504 on one channel (large gamma) into deer_gemm_skinny_hl_f16"""
    T, d = 16, 2048
    x = rnd(T, d, seed=171)
    x[:, 7] = 4.0                                              # normalised value ~4 on channel 7 ...
    gamma = 1 + 0.1 * rnd(d, seed=172)
    gamma[7] = 2.5e4                                          # ... times 2.5e4: ~1e5 after the LayerNorm
    x, gamma, beta = dev(x), dev(gamma), dev(0.1 * rnd(d, seed=173))
    y32 = torch.empty(T, d, device="cuda")
    hi = torch.empty(T, d, device="cuda", dtype=torch.float16)
    lo = torch.empty_like(hi)
    abi.check(lib.deer_resadd_ln_split_f16(abi.ptr(x), None, 0, 0, None, None, abi.ptr(gamma), abi.ptr(beta), abi.ptr(hi), abi.ptr(lo), abi.ptr(y32),
                                           None, T, d, 1e-5, None, st()), "resadd_ln_split_f16")
    torch.cuda.synchronize()
    ln = torch.nn.functional.layer_norm(x.double(), (d,), gamma.double(), beta.double(), 1e-5)
    assert float(ln[:, 7].abs().min()) > F16_MAX
    assert rel_err(y32, ln) < 1e-5
    W = dev(rnd(1024, d, seed=174, scale=d ** -0.5), torch.float16)
    _check_pair_and_product(lib, hi, lo, y32, W)
    rh, rl = _split_hl(y32, torch.float16)
    assert torch.equal(hi, rh) and torch.equal(lo, rl)


def test_f16_attention_planes_beyond_65504(lib):
    """deer_mpt_attn_small_hl_f16 with values ~1e5 on one head (the attention output is a convex combination of them)"""
    B, T, d, H = 2, 9, 256, 2
    R = B * T
    qkv = rnd(R, 3 * d, seed=181)
    qkv[:, 2 * d:2 * d + 128] = 8e4 + 4e4 * torch.rand(R, 128, generator=torch.Generator().manual_seed(182))   # v of head 0
    slab = dev(qkv.unsqueeze(0))
    mask = _key_masks(B, T)
    ws = torch.zeros(R, 3 * d, device="cuda")
    hi = torch.empty(R, d, device="cuda", dtype=torch.float16)
    lo = torch.empty_like(hi)
    abi.check(lib.deer_mpt_attn_small_hl_f16(abi.ptr(slab), 1, R * 3 * d, d, H, None, None, 1e-5, abi.ptr(mask), 8.0, abi.ptr(ws), abi.ptr(hi), abi.ptr(lo),
                                             d, T, B, None, st()), "mpt attn hl f16")
    torch.cuda.synchronize()
    ref = torch.cat([_mpt_attn_ref(slab[0, b * T:(b + 1) * T], T, d, H, None, None, mask[b]) for b in range(B)])
    assert float(ref[:, :128].abs().min()) > F16_MAX
    W = dev(rnd(768, d, seed=183, scale=d ** -0.5), torch.float16)
    _check_pair_and_product(lib, hi, lo, ref.float(), W, atol=1e-5)
