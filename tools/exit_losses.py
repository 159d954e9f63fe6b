"""Per-exit demonstration loss on synthetic windows: evaluate.exit_losses_on_windows (one static full-depth window pass +
DeerEngine.exit_outputs + DeerEngine.exit_losses per batch) on seeded frames, instructions and labels.

    python tools/exit_losses.py [--model 3b|9b|tiny] [--bs 16] [--window 12] [--batches 1] [--iters 3] [--precision fp16] [--layerwise]

Prints ONE JSON line: the per-head num / bin / loss means, the weighted total, and the median wall time of one batch (event-timed, after
a warm-up batch)."""
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
from deer_vla_amd.evaluate import exit_losses_on_windows  # noqa: E402
from deer_vla_amd.flamingo_mpt import MPTFlamingo  # noqa: E402


def synthetic_windows(cfg, bs, W, n_batches, seed=0, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    S, A = cfg.image_size, max(1, int(getattr(cfg, "multi_step_action", 1)))
    ids = syn.synthetic_step_inputs(cfg, 0)[2].reshape(1, -1).repeat(bs, 1)
    out = []
    for _ in range(n_batches):
        labels = torch.randn(bs, W, A, 7, generator=g) * 0.5
        labels[..., 6] = torch.randint(0, 2, (bs, W, A), generator=g).float() * 2 - 1
        b = dict(images=torch.randn(bs, W, 3, S, S, generator=g).to(device), gripper=torch.randn(bs, W, 3, S, S, generator=g).to(device),
                 input_ids=ids.to(device), attention_mask=torch.ones_like(ids, dtype=torch.bool).to(device),
                 labels=(labels if A > 1 else labels[:, :, 0]).to(device))
        if getattr(cfg, "use_state", False):
            st = torch.randn(bs, W, 15, generator=g)
            st[..., -1] = torch.randint(0, 2, (bs, W), generator=g).float() * 2 - 1
            b["state"] = st.to(device)
        out.append(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="3b", choices=["3b", "9b", "tiny"])
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--window", type=int, default=12)
    ap.add_argument("--batches", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--layerwise", action="store_true", help="build the per-layer heads (multi_exit checkpoints)")
    ap.add_argument("--w-bin", type=float, default=0.01)
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    cfg = {"3b": deer_3b, "9b": deer_9b, "tiny": deer_tiny}[args.model]()
    cfg = dataclasses.replace(cfg, window_size=args.window, layerwise_exit_eval=bool(args.layerwise))
    sd = syn.make_synthetic_state(cfg, seed=0, std="0.02" if args.model != "tiny" else "fanin", bf16_round=True)
    model = MPTFlamingo(cfg, sd, window_size=args.window, precision=args.precision)
    batches = synthetic_windows(cfg, args.bs, args.window, args.batches)
    gen = torch.Generator().manual_seed(1)
    res = exit_losses_on_windows(model, batches, args.w_bin, generator=gen)          # warm-up: engines, graphs and scratch come up here
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = exit_losses_on_windows(model, batches, args.w_bin, generator=gen)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / len(batches))
    rec = dict(tool="exit_losses", model=args.model, precision=args.precision, bs=args.bs, W=args.window, T=int(batches[0]["input_ids"].shape[-1]),
               layerwise=bool(args.layerwise), batch_ms=round(statistics.median(ms), 2), **res)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
