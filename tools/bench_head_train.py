"""Time of one exit-head training step on the device: finetune.HeadTrainer.loss_and_grads + step() at the 3B head shape (d = 2048,
H = 1024, four LayerNorm-LSTM layers, W = 12), three heads (the last layer's head + extra_exit on the two sampling strategies of a model
without per-layer heads count as three head runs; --layerwise trains the per-layer heads too), bs = 6 and 16.

    python tools/bench_head_train.py [--bs 6,16] [--window 12] [--iters 20] [--warmup 3] [--no-torch] [--gemm-ab]

Per batch size ONE JSON line:
  step_ms        median of --iters event-timed loss_and_grads + step() rounds after --warmup rounds
  recurrent_ms   the same number of per-step recurrent launches alone (forward deer_head_grad_lstm_step + backward
                 deer_head_grad_lstm_bwd_step, 2 * L_lstm * W launches per head run, x 3 head runs) on buffers of the same shapes, and
                 its share of step_ms
  torch_ms       for orientation only: the same step (three head runs, Huber + BCE, AdamW) as torch.nn.LSTM / nn.Linear / nn.LayerNorm
                 autograd with torch.optim.AdamW in float32 on the same GPU
  gemm_ab        --gemm-ab: the weight-gradient GEMM dW_hh = dG^T H_prev (4H x H, K = bs W) as deer_head_grad_gemm (strided tile) against
                 two explicit transposes + deer_gemm_f32_nt, median ms each
Only the head pipeline is timed: pooled features are random, no trunk is built (the model object carries the head shape only)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deer_vla_amd import _abi as abi  # noqa: E402
from deer_vla_amd.config import deer_3b  # noqa: E402
from deer_vla_amd.engine import config_to_c  # noqa: E402
from deer_vla_amd.finetune import HeadTrainer  # noqa: E402
from deer_vla_amd.synthetic import head_param_shapes  # noqa: E402


class HeadOnlyEngine:
    """what HeadTrainer needs of an engine: the head shape as a deer_model (no arena, no workspace)"""

    def __init__(self, cfg):
        self.cfg, self.lib, self.dev = cfg, abi.lib(), torch.device("cuda")
        self._h = ctypes.c_void_p()
        cc = config_to_c(cfg, 1, 32)
        abi.check(self.lib.deer_model_create(ctypes.byref(cc), ctypes.byref(self._h)), "deer_model_create")

    def close(self):
        torch.cuda.synchronize()
        self.lib.deer_model_destroy(self._h)


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fn, iters, warmup):
    for _ in range(warmup):
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


def head_state(cfg, prefix, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (shape, kind) in head_param_shapes(cfg, prefix).items():
        sd[name] = (1.0 + 0.1 * torch.randn(shape, generator=g)) if kind == "ln_w" else torch.randn(shape, generator=g) / shape[-1] ** 0.5
    return sd


class TorchHead(torch.nn.Module):
    """DeterministicDecoder's trained part in stock torch modules (LayerNorm-LSTM: one nn.LSTM + nn.LayerNorm per layer)"""

    def __init__(self, cfg):
        super().__init__()
        d, H, A = cfg.d_model, cfg.head_hidden, max(1, cfg.multi_step_action)
        self.lstm = torch.nn.ModuleList([torch.nn.LSTM(d if l == 0 else H, H, batch_first=True) for l in range(cfg.lstm_num_layers)])
        self.ln = torch.nn.ModuleList([torch.nn.LayerNorm(H) for _ in range(cfg.lstm_num_layers)]) if cfg.lstm_layernorm else None

        def mlp(n_out):
            layers, cur = [], H
            for dim in cfg.mlp_hidden_dims:
                layers += [torch.nn.Linear(cur, dim)] + ([torch.nn.LayerNorm(dim)] if cfg.mlp_layernorm else []) + [torch.nn.ReLU()]
                cur = dim
            return torch.nn.Sequential(*layers, torch.nn.Linear(cur, n_out))
        self.actions, self.gripper = mlp(6 * A), mlp(A)

    def forward(self, x):
        for l, rnn in enumerate(self.lstm):
            x = rnn(x)[0]
            if self.ln is not None:
                x = self.ln[l](x)
        return torch.tanh(self.actions(x)), self.gripper(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", default="6,16")
    ap.add_argument("--window", type=int, default=12)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layerwise", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--gemm-ab", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dataclasses
    cfg = dataclasses.replace(deer_3b(), window_size=args.window, layerwise_exit_eval=bool(args.layerwise))
    eng = HeadOnlyEngine(cfg)
    lib = eng.lib
    prefixes = ["extra_exit."] + ([p for p, _ in cfg.layerwise_heads()] if args.layerwise else [])
    sd = {}
    for i, p in enumerate(prefixes):
        sd.update(head_state(cfg, p, i))
    exits = cfg.exit_ids()
    W, d, H, Lh, A = args.window, cfg.d_model, cfg.head_hidden, cfg.lstm_num_layers, max(1, cfg.multi_step_action)
    for bs in [int(v) for v in args.bs.split(",")]:
        g = torch.Generator().manual_seed(bs)
        P = torch.randn(bs, W, len(exits), d, generator=g).cuda()
        pose = (torch.rand(bs, W, 6 * A, generator=g) * 2 - 1).cuda()
        grip = torch.randint(0, 2, (bs, W, A), generator=g).float().cuda()
        rl = torch.tensor(exits)[torch.randint(0, len(exits), (bs, W), generator=g)]
        tl = torch.tensor(exits)[torch.randint(0, len(exits), (bs, W), generator=g)]
        tr = HeadTrainer(eng, sd, lr=1e-4)
        n_runs = (len(exits) - 1 if args.layerwise else 0) + 3

        def step():
            tr.zero_grad()
            tr.loss_and_grads(P, rl, tl, pose, grip)
            tr.step()
        step_ms = timed(step, args.iters, args.warmup)
        # the per-step recurrent launches alone, on buffers of the shapes the spine uses
        R = bs * W
        G, DG = torch.randn(R, 4 * H, device="cuda"), torch.zeros(R, 4 * H, device="cuda")
        C, Y, DH = torch.randn(R, H, device="cuda"), torch.zeros(R, H, device="cuda"), torch.randn(R, H, device="cuda")
        DC = torch.zeros(bs, H, device="cuda")
        whh, bhh = sd["extra_exit.rnn.layers.0.weight_hh_l0"].cuda().contiguous(), torch.zeros(4 * H, device="cuda")
        G0 = G.clone()

        def recurrent():
            for _ in range(n_runs * Lh):
                G.copy_(G0)
                for t in range(W):
                    abi.check(lib.deer_head_grad_lstm_step(abi.ptr(G, 16 * H * t), W * 4 * H, abi.ptr(Y, 4 * H * (t - 1)) if t else None, W * H,
                                                           abi.ptr(whh), abi.ptr(bhh), abi.ptr(C, 4 * H * (t - 1)) if t else None, abi.ptr(C, 4 * H * t),
                                                           W * H, abi.ptr(Y, 4 * H * t), W * H, bs, H, st()), "lstm_step")
                for t in range(W - 1, -1, -1):
                    abi.check(lib.deer_head_grad_lstm_bwd_step(abi.ptr(DH, 4 * H * t), W * H, abi.ptr(DG, 16 * H * (t + 1)) if t < W - 1 else None,
                                                               abi.ptr(G, 16 * H * t), abi.ptr(DG, 16 * H * t), W * 4 * H, abi.ptr(whh),
                                                               abi.ptr(C, 4 * H * t), abi.ptr(C, 4 * H * (t - 1)) if t else None, W * H, abi.ptr(DC), bs, H,
                                                               st()), "lstm_bwd_step")
        rec_ms = timed(recurrent, max(3, args.iters // 4), 1)
        copy_ms = timed(lambda: [G.copy_(G0) for _ in range(n_runs * Lh)], max(3, args.iters // 4), 1)
        rec = dict(tool="bench_head_train", bs=bs, W=W, d=d, H=H, lstm_layers=Lh, head_runs=n_runs, layerwise=bool(args.layerwise),
                   step_ms=round(step_ms, 3), recurrent_ms=round(rec_ms - copy_ms, 3), recurrent_share=round((rec_ms - copy_ms) / step_ms, 3),
                   recurrent_launches=2 * n_runs * Lh * W)
        if not args.no_torch:
            heads = [TorchHead(cfg).cuda() for _ in range(len(prefixes))]
            opt = torch.optim.AdamW([p for h in heads for p in h.parameters()], lr=1e-4, weight_decay=0.0)
            Xs = [P[:, :, -1].contiguous(), P[:, :, 0].contiguous(), P[:, :, 1 % len(exits)].contiguous()]
            Xs = [P[:, :, k].contiguous() for k in range(len(exits) - 1)] + Xs if args.layerwise else Xs
            which = list(range(1, len(prefixes))) + [0, 0] if args.layerwise else [0, 0, 0]

            def torch_step():
                opt.zero_grad(set_to_none=False)
                loss = 0.0
                for hi, X in zip(which, Xs):
                    a, lg = heads[hi](X)
                    loss = loss + (torch.nn.functional.huber_loss(a, pose, reduction="none").mean(-1)
                                   + 0.01 * torch.nn.functional.binary_cross_entropy_with_logits(lg, grip, reduction="none").mean(-1)).mean()
                loss.backward()
                opt.step()
            rec["torch_ms"] = round(timed(torch_step, args.iters, args.warmup), 3)
            del heads, opt
        if args.gemm_ab:
            HP = torch.randn(R, H, device="cuda")
            out = torch.empty(4 * H, H, device="cuda")
            DGr = torch.randn(R, 4 * H, device="cuda")
            Rp = (R + 3) // 4 * 4

            def strided():
                abi.check(lib.deer_head_grad_gemm(abi.ptr(DGr), 4 * H, 1, abi.ptr(HP), H, 1, abi.ptr(out), H, 4 * H, H, R, 0, st()), "gemm")

            def transposed():
                a = torch.zeros(4 * H, Rp, device="cuda")
                b = torch.zeros(H, Rp, device="cuda")
                a[:, :R].copy_(DGr.t())
                b[:, :R].copy_(HP.t())
                abi.check(lib.deer_gemm_f32_nt(abi.ptr(a), Rp, abi.ptr(b), Rp, None, abi.ptr(out), H, 4 * H, H, Rp, 0, st()), "gemm_f32_nt")
            rec["gemm_ab"] = dict(shape=[4 * H, H, R], strided_ms=round(timed(strided, 50, 5), 4), transpose_nt_ms=round(timed(transposed, 50, 5), 4))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del tr
    eng.close()


if __name__ == "__main__":
    main()
