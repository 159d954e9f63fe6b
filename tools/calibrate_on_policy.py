"""Exit thresholds for a budget from ON-POLICY values (value_net.calibrate_on_policy) on the harness's synthetic environments with synthetic
weights: calibrates once on a few synthetic windows (the demonstration-set protocol, solved for the budget on the device), then runs
--rounds rounds of [live rollout of shadow steps whose deltas are logged on the device -> solve_for_budget on the logged matrix].  Prints
one operating_point_log block per round (thresholds, average successful length - not measured here: nan -, measured average exit layer)
and one JSON line per round with the predicted and the measured exit mix.

usage: calibrate_on_policy.py --avg-exit-layer 4 [--rounds 3] [--n_samples 256] [--n_envs 8] [--config tiny|3b] [--ep_len 8] [--num_seq 16]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deer_vla_amd import rollout as ro  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_3b, deer_tiny  # noqa: E402
from deer_vla_amd.factory import create_model_and_transforms  # noqa: E402
from deer_vla_amd.value_net import ActionValueNet, calibrate_on_policy, generate_action_values, solve_for_budget  # noqa: E402
from sweep_operating_points import TASKS, calibration_loader  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--avg-exit-layer", type=float, required=True, metavar="X", help="the budget: average exit layer (layers per step)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n_samples", type=int, default=256, help="on-policy steps logged per round")
    ap.add_argument("--num_seq", type=int, default=16)
    ap.add_argument("--n_envs", type=int, default=8)
    ap.add_argument("--config", choices=["tiny", "3b"], default="tiny")
    ap.add_argument("--ep_len", type=int, default=8)
    ap.add_argument("--task_steps", type=int, default=4, help="steps after which a sub-task counts as solved")
    ap.add_argument("--calib_windows", type=int, default=2)
    args = ap.parse_args()

    cfg = deer_tiny() if args.config == "tiny" else deer_3b()
    sd = syn.make_synthetic_state(cfg, 0, bf16_round=True) if args.config == "tiny" else syn.make_synthetic_state(cfg, seed=0, std="0.02", bf16_round=True)
    model, proc, tok = create_model_and_transforms("ViT-L-14", "openai", "", "", window_size=cfg.window_size, use_gripper=True, fusion_mode="post",
                                                   llm_name="mpt_dolly_3b", state_dict=sd, cfg=cfg, n_envs=args.n_envs)
    exit_ids = model.get_all_exit_idx()
    vn = ActionValueNet(exit_ids, None, cfg.exit_interval, cfg.window_size, "L2")
    values, _ = generate_action_values(None, model, vn, calibration_loader(cfg, proc, tok, args.calib_windows, cfg.window_size),
                                       generator=torch.Generator().manual_seed(0), fused=True)
    start, ratio, (_, avg) = solve_for_budget(values, exit_ids, args.avg_exit_layer, engine=model.engine, value_net=vn)
    print(json.dumps({"round": "demonstrations", "exit_ratio": ratio, "thresholds": start.threshold_list(), "avg_exit_layer_budget": args.avg_exit_layer,
                      "avg_exit_layer_predicted": avg}))

    rng = np.random.default_rng(0)
    seqs = [(None, [TASKS[int(i)] for i in rng.integers(0, len(TASKS), 5)]) for _ in range(args.num_seq)]
    ann = {t: [t] for t in TASKS}
    envs = [ro.SyntheticEnv(seed=b) for b in range(args.n_envs)]
    w = ro.BatchedModelWrapper(model, tok, proc, torch.float32, exit_controller=start)
    _, records = calibrate_on_policy(w, envs, seqs, ann, ro.steps_task_checker(args.task_steps), start, args.n_samples, args.avg_exit_layer,
                                     rounds=args.rounds, engine=model.engine, ep_len=args.ep_len)
    for r in records:
        print(ro.operating_point_log(r["thresholds"], float("nan"), r["measured"][1]), end="")
        print(json.dumps({"round": r["round"], "exit_ratio": r["exit_ratio"], "thresholds": r["thresholds"],
                          "avg_exit_layer_budget": args.avg_exit_layer, "avg_exit_layer_collected": r["collected"][1],
                          "avg_exit_layer_predicted": r["predicted"][1], "avg_exit_layer_measured": r["measured"][1],
                          "mix_predicted": r["predicted"][0], "mix_measured": r["measured"][0]}))


if __name__ == "__main__":
    main()
