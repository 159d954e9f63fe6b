#!/usr/bin/env python3
"""Runs the cases of tests/test_fp32_kernels.py with plain torch float32 on the CPU in place of the HIP kernels and prints, per family, the
largest error / bound against the module's fp64 references: a check of the references and bounds themselves (an f32 implementation of the
same operation has to sit inside every gate) that needs no GPU.  The operands differ from the GPU run's (another generator), the shapes,
layouts and seeds are the same.

    python tools/fp32_kernels_cpu_reference.py
"""
import importlib.util
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("fp32_kernels", os.path.join(ROOT, "tests", "test_fp32_kernels.py"))
K = importlib.util.module_from_spec(spec)
spec.loader.exec_module(K)
K.DEV = "cpu"
torch.set_num_threads(8)


def exited(ctl):
    return ctl is not None and int(ctl[K.abi.CTL_ALL_EXITED]) != 0


def k_gemm(lib, A, W, bias, C, epi):
    x = A @ W.t()
    if bias is not None:
        x = x + bias
    if epi == K.PE_QGELU:
        x = x * torch.sigmoid(1.702 * x)
    elif epi == K.PE_GELU:
        x = F.gelu(x)
    elif epi == K.PE_RESADD:
        x = C + x
    C.copy_(x)


def k_attn(lib, q, k1, v1, k2, v2, o, scale):
    batch, q_len, C = q.shape
    k, v = (k1, v1) if k2 is None else (torch.cat([k1, k2], 1), torch.cat([v1, v2], 1))
    hs = lambda t: t.reshape(batch, t.shape[1], C // 64, 64).transpose(1, 2)
    p = torch.softmax((hs(q) * scale) @ hs(k).transpose(-1, -2), -1)
    o.copy_((p @ hs(v)).transpose(1, 2).reshape(batch, q_len, C))


def k_xattn(lib, slab, stride, k, v, tt, npm, out, T, heads, scale, ctl):
    if exited(ctl):
        return
    rows = slab.shape[1]
    batch = rows // T
    n_kv = k.shape[0] // batch
    hs = lambda t, n: t.reshape(batch, n, heads, 64).transpose(1, 2)
    s = (hs(slab.sum(0), T) * scale) @ hs(k, n_kv).transpose(-1, -2)
    j = torch.arange(n_kv).view(1, 1, 1, n_kv)
    t = tt.view(batch, 1, T, 1).long()
    s = s.masked_fill(~(t == j // npm + 1), -torch.finfo(torch.float32).max)
    p = torch.softmax(s, -1).masked_fill((tt == 0).view(batch, 1, T, 1), 0.0)
    out.copy_((p @ hs(v, n_kv)).transpose(1, 2).reshape(rows, heads * 64))


def k_skinny(lib, fmt, mode, A, slab, stride, planes, part, M, N, Kd, S, ctl):
    if exited(ctl):
        return
    dt = K.TDT[fmt]
    if mode == K.A_BF16:
        hi, lo = A.float(), None
    else:
        a = A if mode == K.A_F32 else slab.sum(0)
        if mode == K.A_SLABS_GELU:
            a = F.gelu(a)
        h = (a.clamp(-K.F16_MAX, K.F16_MAX) if fmt == "f16" else a).to(dt)
        hi, lo = h.float(), (a - h.float()).to(dt).float()
    KR = Kd // S
    for p, W in enumerate(planes):
        Wf = W.float()
        for ks in range(S):
            sl = slice(ks * KR, (ks + 1) * KR)
            y = hi[:, sl] @ Wf[:, sl].t()
            if lo is not None:
                y = y + lo[:, sl] @ Wf[:, sl].t()
            part[p * S + ks, :M] = y
            part[p * S + ks, M:] = 0.0


def _mpt(slab, d, H, gq, gk, mask, bias_max, T):
    qkv = slab.sum(0)
    rows = qkv.shape[0]
    q, k, v = qkv.chunk(3, -1)
    if gq is not None:
        q, k = F.layer_norm(q, (d,), gq, None, 1e-5), F.layer_norm(k, (d,), gk, None, 1e-5)
    hd, batch = d // H, rows // T
    hs = lambda t: t.reshape(batch, T, H, hd).transpose(1, 2)
    slopes = 2.0 ** (-bias_max * torch.arange(1, H + 1, dtype=torch.float32) / H)
    alibi = (T - 1 - torch.arange(T, dtype=torch.float32)).view(1, 1, 1, T) * slopes.view(1, H, 1, 1)
    s = hs(q) @ hs(k).transpose(-1, -2) * hd ** -0.5 - alibi
    vis = torch.ones(T, T, dtype=torch.bool).tril().view(1, 1, T, T)
    if mask is not None:
        vis = vis & mask.bool().view(batch, 1, 1, T)
    return (torch.softmax(s.masked_fill(~vis, float("-inf")), -1) @ hs(v)).transpose(1, 2).reshape(rows, d)


def k_mpt(lib, slab, stride, d, H, gq, gk, mask, bias_max, out, T, ctl):
    if not exited(ctl):
        out.copy_(_mpt(slab, d, H, gq, gk, mask, bias_max, T))


def k_mpt_hl(lib, slab, stride, d, H, gq, gk, mask, bias_max, hi, lo, T):
    o = _mpt(slab, d, H, gq, gk, mask, bias_max, T)
    hi.copy_(o.bfloat16())
    lo.copy_((o - hi.float()).bfloat16())


def k_resadd(lib, x, slab, stride, gate, gamma, beta, y32, xc, ctl):
    if slab is not None:
        s = slab[0].clone()
        for i in range(1, slab.shape[0]):
            s += slab[i]
        x += (torch.tanh(gate) if gate is not None else 1.0) * s
    if xc is not None:
        xc.copy_(x)
    if gamma is not None:
        y32.copy_(F.layer_norm(x, (x.shape[1],), gamma, beta, 1e-5))


for name in ("k_gemm", "k_attn", "k_xattn", "k_skinny", "k_mpt", "k_mpt_hl", "k_resadd"):
    setattr(K, name, globals()[name])

if __name__ == "__main__":
    for epi in K.GEMM_EPI:
        K.test_gemm_f32_nt(None, epi)
    for q_len in K.ATTN_QLEN:
        K.test_attn_f32(None, q_len)
    for T in K.XATTN_T:
        K.test_xattn_f32(None, T)
    K.test_xattn_f32_exit_flag(None)
    for M in K.SK_M:
        K.test_gemm_skinny_two_planes(None, M)
    K.test_gemm_skinny_exit_flag(None)
    for d, H in K.MPT_CFG:
        for qk_ln in (True, False):
            K.test_mpt_attn_small_f32(None, d, H, qk_ln)
    K.test_mpt_attn_small_exit_flag_and_planes(None)
    for d in (96, 256, 2048):
        K.test_resadd_ln_out_f32(None, d)
    K.test_gates_reject_perturbed_results(None)
    print("torch float32 on the CPU, largest error / bound per family:")
    for k, v in sorted(K.RATIOS.items()):
        print(f"  {k:28s} {v:.3g}")
