"""Window mode of the action head: DeerEngine.head_sequence (one deer_head_sequence call, csrc/head_seq.hip) against the per-step loop
(DeerEngine._head_eval on siblings of <= 16 sequences, one evaluation per time step) at 3B and 9B head widths.

    python tools/bench_head_seq.py [--precision fp16] [--iters 20]

Prints one line per (width, N, L): microseconds per call of both forms and the effective weight rate (head weight bytes / time; the
sequence form reads W_ih and the MLP weights once per call, the loop once per step and chunk)."""
import argparse
import dataclasses
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_tiny  # noqa: E402
from deer_vla_amd.engine import DeerEngine  # noqa: E402


def head_cfg(d):
    """the 3B (d = 2048) / 9B (d = 4096) action head around a minimal trunk (the head's tensors do not depend on it)"""
    return dataclasses.replace(deer_tiny(), d_model=d, n_heads=d // 128, mlp_ratio=1, n_layers_total=4, early_exit_layer=1, head_hidden=1024,
                               lstm_num_layers=4, lstm_layernorm=True, mlp_layernorm=True, mlp_num_hidden_layers=3)


def head_weight_bytes(cfg, wbytes):
    H, d = cfg.head_hidden, cfg.d_model
    lstm = 4 * H * (d + H) + (cfg.lstm_num_layers - 1) * 4 * H * 2 * H
    dims = [H] + list(cfg.mlp_hidden_dims)
    mlp = 2 * sum(a * b for a, b in zip(dims[:-1], dims[1:])) + dims[-1] * 7
    return wbytes * (lstm + mlp)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters


def step_loop(eng, f):
    N, L = f.shape[:2]
    for n0 in range(0, N, 16):
        n = min(16, N - n0)
        w = eng.sibling(n)
        w.h_state.zero_()
        w.c_state.zero_()
        w._head_state_changed()
        for t in range(L):
            w._head_eval(f[n0:n0 + n, t].reshape(-1, f.shape[-1]), commit=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--shapes", default="16x12,64x12,192x6")
    ap.add_argument("--widths", default="2048,4096")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    wb = 4 if args.precision == "fp32" else 2
    for d in (int(v) for v in args.widths.split(",")):
        cfg = head_cfg(d)
        eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, 7), precision=args.precision)
        wbytes = head_weight_bytes(cfg, wb)
        for N, L in shapes:
            f = torch.randn(N, L, args.T, d, device=eng.dev)
            seq_us = timed(lambda: eng.head_sequence(f), args.iters)
            loop_us = timed(lambda: step_loop(eng, f), max(2, args.iters // 4))
            print(json.dumps(dict(d=d, N=N, L=L, T=args.T, precision=args.precision, seq_us=round(seq_us, 1), loop_us=round(loop_us, 1),
                                  speedup=round(loop_us / seq_us, 2), seq_weight_gbs=round(wbytes / seq_us / 1e3, 1),
                                  head_weight_mb=round(wbytes / 1e6, 1))), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
