"""Threshold calibration: the one-pass path (DeerEngine.window_exit_features + calibrate_values, csrc/calib.hip) against the existing
per-step loop (window_hidden_states + generate_values) in the same process, W = 12 windows, inputs resident on the device.

    python tools/bench_calibrate.py [--precisions fp16,bf16] [--bs 1,2,8,32] [--iters 20] [--whole 3b] [--out FILE]

Two legs, one JSON line per (leg, model, precision, bs), medians over --iters event-timed repetitions after a warm-up:
  head   the head half alone on the same hidden states: calibrate_values (on their pooled features) vs generate_values, at the 3B
         (d = 2048, 12 layers, six exits) and 9B (d = 4096, 13 layers, seven exits) head shapes around a minimal trunk
  whole  the whole batch on a full-size model (--whole: 3b and / or 9b): trunk pass + head side of both paths, and the peak extra device
         memory of each (torch.cuda.max_memory_allocated above the resident inputs + the spine's scratch, deer_model_scratch_bytes)"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_3b, deer_9b, deer_tiny  # noqa: E402
from deer_vla_amd.engine import DeerEngine  # noqa: E402

W = 12


def head_cfg(full):
    """the action head and exit layers of a full-size model around a minimal trunk of the same depth (the head's tensors do not depend on it)"""
    d = full.d_model
    return dataclasses.replace(deer_tiny(), d_model=d, n_heads=d // 128, mlp_ratio=1, n_layers_total=full.n_layers, early_exit_layer=full.early_exit_layer,
                               exit_interval=full.exit_interval, head_hidden=full.head_hidden, lstm_num_layers=full.lstm_num_layers,
                               lstm_layernorm=full.lstm_layernorm, mlp_layernorm=full.mlp_layernorm, mlp_num_hidden_layers=full.mlp_num_hidden_layers)


def timed(fn, iters):
    """median milliseconds of `iters` repetitions, each between two events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def peak_extra(eng, fn):
    """peak device bytes `fn` adds to what is resident: torch allocations + growth of the spine's scratch"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base, s0 = torch.cuda.memory_allocated(), eng.lib.deer_model_scratch_bytes(eng._h)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base + eng.lib.deer_model_scratch_bytes(eng._h) - s0


def rand_layers(exit_ids, bs, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(exit_ids)[torch.randint(0, len(exit_ids), (bs, W), generator=g)]


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def head_leg(name, full, precision, sizes, iters, T, out):
    cfg = head_cfg(full)
    eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, 7), precision=precision)
    exit_ids = cfg.exit_ids()
    layers = [0] + exit_ids
    for bs in sizes:
        hid = torch.randn(bs, W, cfg.n_layers, T, cfg.d_model, device=eng.dev)
        feats = hid[:, :, layers].amax(3) if cfg.pooling == "max" else hid[:, :, layers].mean(3)
        rl = rand_layers(exit_ids, bs)
        fused = timed(lambda: eng.calibrate_values(feats, rl, "L2"), iters)
        loop = timed(lambda: eng.generate_values(hid, rl, "L2"), iters)
        emit(dict(leg="head", model=name, precision=precision, bs=bs, W=W, T=T, fused_ms=round(fused, 3), loop_ms=round(loop, 3),
                  speedup=round(loop / fused, 2), hidden_mb=round(hid.numel() * 4 / 1e6, 1), pooled_mb=round(feats.numel() * 4 / 1e6, 2)), out)
        del hid, feats
        torch.cuda.empty_cache()


def whole_leg(name, cfg, precision, sizes, iters, out):
    eng = DeerEngine(cfg, syn.make_synthetic_state(cfg, seed=0, std="0.02", bf16_round=True), precision=precision)
    exit_ids = cfg.exit_ids()
    S = cfg.image_size
    step = syn.synthetic_step_inputs(cfg, 0)
    ids = step[2].to(eng.dev)
    T = ids.shape[-1]
    for bs in sizes:
        F = bs * W
        rgb = torch.randn(F, 3, S, S, device=eng.dev).to(eng.img_dtype)
        grip = torch.randn(F, 3, S, S, device=eng.dev).to(eng.img_dtype)
        rl = rand_layers(exit_ids, bs)

        def fused():
            f = eng.window_exit_features(rgb, grip, ids)
            return eng.calibrate_values(f.view(bs, W, *f.shape[1:]), rl, "L2")

        def loop():
            h = eng.window_hidden_states(rgb, grip, ids)
            return eng.generate_values(h.view(bs, W, *h.shape[1:]), rl, "L2")
        t_f, t_l = timed(fused, iters), timed(loop, iters)
        torch.cuda.empty_cache()
        m_l, m_f = peak_extra(eng, loop), peak_extra(eng, fused)      # scratch growth shows on the first call of a size only: measured last = 0
        emit(dict(leg="whole", model=name, precision=precision, bs=bs, W=W, T=T, fused_ms=round(t_f, 2), loop_ms=round(t_l, 2),
                  speedup=round(t_l / t_f, 3), fused_peak_mb=round(m_f / 1e6, 1), loop_peak_mb=round(m_l / 1e6, 1),
                  scratch_mb=round(eng.lib.deer_model_scratch_bytes(eng._h) / 1e6, 1)), out)
        del rgb, grip
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="fp16,bf16")
    ap.add_argument("--bs", default="1,2,8,32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--legs", default="head,whole")
    ap.add_argument("--whole", default="3b", help="full-size models of the whole-batch leg: 3b, 9b or 3b,9b")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    sizes = [int(v) for v in args.bs.split(",")]
    models = {"3b": deer_3b(), "9b": deer_9b()}
    for precision in args.precisions.split(","):
        if "head" in args.legs:
            for name, full in models.items():
                head_leg(name, full, precision, sizes, args.iters, args.T, args.out)
                torch.cuda.empty_cache()
        if "whole" in args.legs:
            for name in args.whole.split(","):
                whole_leg(name, models[name], precision, sizes, args.iters, args.out)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
