"""Operating-point sweep in ONE batched run (the reference's eval_ckpts.py loop over --exit_ratio / --max_layer, one full evaluation per
point, as one evaluate_policy_batched(operating_points=...) call): calibrates once (window-mode deltas of a few synthetic windows), solves
the thresholds of every (exit_ratio, max_layer) pair from that one value matrix, runs every chain once per point on the harness's
synthetic environments and prints one JSON line per point (ratio, cap, thresholds, avg_len, avg exit).  --compare also runs every point
alone and prints the wall time of the sweep against the sum of the single-point runs.

--avg-exit-layer X (repeatable) names the points by BUDGET instead: for every X (and cap) value_net.solve_for_budget finds the exit ratio whose
predicted average exit layer on the calibration set is the largest one not above X - on the device when the calibration left its values there
(--fused-calibration).

usage: sweep_operating_points.py (--exit_ratio 0.6 0.8 1.0 1.2 | --avg-exit-layer 3 --avg-exit-layer 4.5) [--max_layer 12 6] [--num_seq 16]
                                 [--n_envs 8] [--config tiny|3b] [--ep_len 8] [--compare] [--fused-calibration]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deer_vla_amd import rollout as ro  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_3b, deer_tiny  # noqa: E402
from deer_vla_amd.factory import create_model_and_transforms  # noqa: E402
from deer_vla_amd.value_net import ActionValueNet, controllers_from_values, generate_action_values, solve_for_budget  # noqa: E402

TASKS = ["open", "push", "turn", "lift", "move"]      # one-word instructions (the idle slots' "idle" has the same length)


def calibration_loader(cfg, proc, tok, n_windows: int, W: int):
    """synthetic CALVIN-style calibration batches (images (1, W, 3, S, S), (ids, mask), -, gripper) from seeded moving frames"""
    for k in range(n_windows):
        env = ro.SyntheticEnv(seed=100 + k)
        frames = []
        for _ in range(W):
            o = env.get_obs()
            frames.append((ro.preprocess_image([o["rgb_obs"]["rgb_static"]], proc)[0], ro.preprocess_image([o["rgb_obs"]["rgb_gripper"]], proc)[0]))
            env.step(np.zeros(7, dtype=np.float32))
        ids, mask = ro.preprocess_text_calvin([TASKS[k % len(TASKS)]], tok)
        yield (torch.stack([f[0] for f in frames]).unsqueeze(0).float(), (ids, mask), None, torch.stack([f[1] for f in frames]).unsqueeze(0).float())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--exit_ratio", type=float, nargs="+", default=None)
    ap.add_argument("--avg-exit-layer", type=float, action="append", default=None, metavar="X",
                    help="an operating point by budget (repeatable): the exit ratio is solved so that the calibration set predicts an average "
                         "exit layer of at most X (value_net.solve_for_budget); replaces --exit_ratio")
    ap.add_argument("--max_layer", type=int, nargs="*", default=None, help="DeeR-S / DeeR-B caps (the reference's --max_layer); default: every exit")
    ap.add_argument("--num_seq", type=int, default=16)
    ap.add_argument("--n_envs", type=int, default=8)
    ap.add_argument("--config", choices=["tiny", "3b"], default="tiny")
    ap.add_argument("--ep_len", type=int, default=8)
    ap.add_argument("--task_steps", type=int, default=4, help="steps after which a sub-task counts as solved")
    ap.add_argument("--calib_windows", type=int, default=2)
    ap.add_argument("--compare", action="store_true", help="also run every point alone and report both wall times")
    ap.add_argument("--fused-calibration", action="store_true",
                    help="calibrate through window_exit_features + calibrate_values (one device pass per batch) instead of the per-step loop")
    args = ap.parse_args()
    if (args.exit_ratio is None) == (args.avg_exit_layer is None):
        ap.error("give the operating points either as --exit_ratio ... or as --avg-exit-layer X [--avg-exit-layer Y ...]")

    cfg = deer_tiny() if args.config == "tiny" else deer_3b()
    sd = syn.make_synthetic_state(cfg, 0, bf16_round=True) if args.config == "tiny" else syn.make_synthetic_state(cfg, seed=0, std="0.02", bf16_round=True)
    model, proc, tok = create_model_and_transforms("ViT-L-14", "openai", "", "", window_size=cfg.window_size, use_gripper=True, fusion_mode="post",
                                                   llm_name="mpt_dolly_3b", state_dict=sd, cfg=cfg, n_envs=args.n_envs)
    exit_ids = model.get_all_exit_idx()
    vn = ActionValueNet(exit_ids, None, cfg.exit_interval, cfg.window_size, "L2")
    t0 = time.perf_counter()
    values, _ = generate_action_values(None, model, vn, calibration_loader(cfg, proc, tok, args.calib_windows, cfg.window_size),
                                       generator=torch.Generator().manual_seed(0), fused=args.fused_calibration)
    t_cal = time.perf_counter() - t0
    caps = args.max_layer or [exit_ids[-1] + 1]
    predicted = {}
    if args.avg_exit_layer is not None:
        pairs, points = [], []
        for m in caps:
            for budget in args.avg_exit_layer:
                c, r, (_, avg) = solve_for_budget(values, exit_ids, budget, max_layer=m, engine=model.engine, value_net=vn)
                pairs.append((r, m))
                points.append(c)
                predicted[len(points) - 1] = {"avg_exit_layer_budget": budget, "avg_exit_layer_predicted": avg}
    else:
        pairs = [(r, m) for m in caps for r in args.exit_ratio]
        points = controllers_from_values(vn, exit_ids, values, [r for r, _ in pairs], [m for _, m in pairs], engine=model.engine)

    rng = np.random.default_rng(0)
    seqs = [(None, [TASKS[int(i)] for i in rng.integers(0, len(TASKS), 5)]) for _ in range(args.num_seq)]
    ann = {t: [t] for t in TASKS}
    ok = ro.steps_task_checker(args.task_steps)
    envs = [ro.SyntheticEnv(seed=b) for b in range(args.n_envs)]
    w = ro.BatchedModelWrapper(model, tok, proc, torch.float32, exit_controller=points[0])
    ro.evaluate_policy_batched(w, envs, seqs[:1], ann, ok, ep_len=2, operating_points=points)     # warm-up: graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = ro.evaluate_policy_batched(w, envs, seqs, ann, ok, ep_len=args.ep_len, operating_points=points)
    t_sweep = time.perf_counter() - t0
    for p, ((r, m), c, o) in enumerate(zip(pairs, points, outs)):
        print(json.dumps({"exit_ratio": r, "max_layer": m, "thresholds": c.threshold_list(), "avg_len": o["avg_seq_len"],
                          "avg_exit": o["avg_exit"], "n_steps": o["n_steps_all"], "exit_hist": o["exit_hist"], **predicted.get(p, {})}))
    summary = {"points": len(points), "n_envs": args.n_envs, "num_seq": args.num_seq, "calibration_s": round(t_cal, 3),
               "sweep_wall_s": round(t_sweep, 3)}
    if args.compare:
        t_sep = 0.0
        for c in points:
            ws = ro.BatchedModelWrapper(model, tok, proc, torch.float32, exit_controller=c)
            ro.evaluate_policy_batched(ws, envs, seqs[:1], ann, ok, ep_len=2)                      # warm-up: graph capture
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ro.evaluate_policy_batched(ws, envs, seqs, ann, ok, ep_len=args.ep_len)
            t_sep += time.perf_counter() - t0
        summary["separate_wall_s"] = round(t_sep, 3)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
