"""Exit-only fine-tuning on synthetic windows: evaluate.finetune_exit_heads (pooled exit-layer features once per batch, then
finetune.HeadTrainer's loss gradient + AdamW on the device) on seeded frames, instructions and labels - the reference's second training
stage (only_train_head, train_utils.py:487-543) with the trunk frozen.

    python tools/finetune_exit_heads.py [--model tiny|3b] [--bs 2] [--window 4] [--steps 20] [--lr 1e-3] [--precision fp16] [--layerwise]

Prints ONE JSON line: the per-head loss BEFORE and AFTER, both measured by evaluate.exit_losses_on_windows with the same layer tables (after
``commit()``: the engine's own ingested weights), the training losses of the first and last step, and the median wall time of one step."""
import argparse
import dataclasses
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_3b, deer_tiny  # noqa: E402
from deer_vla_amd.evaluate import exit_losses_on_windows, finetune_exit_heads  # noqa: E402
from deer_vla_amd.flamingo_mpt import MPTFlamingo  # noqa: E402
from exit_losses import synthetic_windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="tiny", choices=["3b", "tiny"])
    ap.add_argument("--bs", type=int, default=2)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--batches", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--layerwise", action="store_true", help="build and train the per-layer heads (multi_exit checkpoints)")
    ap.add_argument("--w-bin", type=float, default=0.01)
    args = ap.parse_args()
    cfg = {"3b": deer_3b, "tiny": deer_tiny}[args.model]()
    cfg = dataclasses.replace(cfg, window_size=args.window, layerwise_exit_eval=bool(args.layerwise))
    sd = syn.make_synthetic_state(cfg, seed=0, std="0.02" if args.model != "tiny" else "fanin", bf16_round=True)
    model = MPTFlamingo(cfg, sd, window_size=args.window, precision=args.precision)
    batches = synthetic_windows(cfg, args.bs, args.window, args.batches)

    def measure():
        random.seed(1)
        return exit_losses_on_windows(model, batches, args.w_bin, generator=torch.Generator().manual_seed(1))
    before = measure()
    random.seed(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer, history = finetune_exit_heads(model, batches, args.steps, sd, lr=args.lr, w_bin=args.w_bin, generator=torch.Generator().manual_seed(2))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    after = measure()
    ms = []
    P = None
    for _ in range(5):                                       # one more timed round per repetition on the trained heads (not committed)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if P is None:
            from deer_vla_amd.evaluate import split_labels, window_batch_inputs
            kw = window_batch_inputs(batches[0], args.window)
            bs, rgb, grip_f, ids, mask, _ = model._window_inputs(kw["vision_x"], kw["lang_x"], kw["attention_mask"], kw["vision_gripper"], None)
            pooled = model.engine.window_exit_pooled(rgb, grip_f, ids, mask)
            P = pooled.view(bs, args.window, pooled.shape[1], pooled.shape[2]).clone()
            pose, grip01 = split_labels(batches[0]["labels"], model.engine.A)
            rl, tl = model.draw_exit_layers(bs, args.window, torch.Generator().manual_seed(3))
        e0.record()
        trainer.zero_grad()
        trainer.loss_and_grads(P, rl, tl, pose, grip01, w_bin=args.w_bin)
        trainer.step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    rec = dict(tool="finetune_exit_heads", model=args.model, precision=args.precision, bs=args.bs, W=args.window, steps=args.steps, lr=args.lr,
               layerwise=bool(args.layerwise), heads=before["heads"], loss_before=before["loss"], loss_after=after["loss"],
               train_loss_first=history[0].tolist(), train_loss_last=history[-1].tolist(), step_ms=round(statistics.median(ms), 3),
               finetune_wall_s=round(wall, 3))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
