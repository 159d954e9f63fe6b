"""Exit-only fine-tuning through the public surface (deer_vla_amd/finetune.py HeadTrainer, evaluate.finetune_exit_heads) on the tiny model
of tests/golden/all_exits*.npz: bs = 2 windows of W = 4 steps, T = 6 tokens, three exit layers with per-layer heads.

The CPU trajectory is the oracle's autograd (tests/head_grad_ref.py) per head plus an fp64 restatement of AdamW; the parameter gate is the
kernel test's (K e32 + 16 * 2^-24 relative to the tensor's largest entry, e32 from the same trajectory in float32 with
torch.optim.AdamW), K doubled per step taken."""
import dataclasses
import random
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

import head_grad_ref as ref  # noqa: E402
from golden_util import load  # noqa: E402
from test_all_exits import HEAD_TOL  # noqa: E402
from test_head_grad_kernels import FLOOR, K  # noqa: E402
from deer_vla_amd import _abi as abi  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.evaluate import exit_losses_on_windows, finetune_exit_heads  # noqa: E402
from deer_vla_amd.flamingo_mpt import MPTFlamingo  # noqa: E402

LR = 1e-3
_models = {}


def _model(name, precision, layerwise=True, fresh=False):
    key = (name, precision, layerwise)
    if fresh or key not in _models:
        cfg, seed, g = load(name)
        if not layerwise:
            cfg = dataclasses.replace(cfg, layerwise_exit_eval=False)
        sd = syn.make_synthetic_state(cfg, seed, bf16_round=True)
        m = (cfg, g, sd, MPTFlamingo(cfg, sd, window_size=cfg.window_size, precision=precision))
        if fresh:
            return m
        _models[key] = m
    return _models[key]


def _inputs(cfg, g):
    bs, W = g["rand_layers"].shape
    P = g["pooled"].view(bs, W, *g["pooled"].shape[1:]).cuda()
    return P, g["rand_layers"], g["two_layers"], g["label_pose"], g["label_grip01"], float(g["w_bin"])


def _step_words(eng):
    """what a step computed, from its control block: exit layer, action, deltas (the other words are step counters and host pointers)"""
    words = [abi.CTL_EXIT_LAYER] + list(range(abi.CTL_OUT_ACTION, abi.CTL_OUT_ACTION + 8)) + list(range(abi.CTL_DELTAS, abi.CTL_DELTAS + 16))
    return eng.ctl.view(-1)[words].clone()


def _head_inputs(cfg, P, rl, tl):
    """[(prefix, X (bs, W, d) on the CPU in fp64)] in ``exit_outputs``' order: per-layer heads, lm_head, extra_exit on strategy 1 and 2"""
    exits = cfg.exit_ids()
    Pc = P.cpu().double()
    bi, ti = torch.meshgrid(torch.arange(P.shape[0]), torch.arange(P.shape[1]), indexing="ij")
    out = [(prefix, Pc[:, :, exits.index(layer)]) for prefix, layer in cfg.layerwise_heads()]
    for sel in (rl, tl):
        slot = torch.tensor([[exits.index(int(v)) for v in row] for row in sel])
        out.append(("extra_exit.", Pc[bi, ti, slot]))
    return out


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_losses_before_any_step_are_the_engines(precision):
    """1: the trainer (unrounded f32 parameters) against engine.exit_losses(engine.exit_outputs(...)) (ingested parameters): the head-only
    gates of tests/test_all_exits.py; the loss is 1-Lipschitz in the outputs those gates bound"""
    cfg, g, sd, model = _model("all_exits.npz", precision)
    P, rl, tl, pose, grip, w_bin = _inputs(cfg, g)
    eng = model.engine
    want = eng.exit_losses(eng.exit_outputs(P, rl, tl), pose, grip, w_bin)[2].cpu()
    tr = eng.head_trainer(sd, lr=LR)
    got = tr.loss_and_grads(P, rl, tl, pose, grip, w_bin).cpu()
    print(precision, "trainer", got.tolist(), "engine", want.tolist())
    assert got.shape == want.shape and float((got - want).abs().max()) < HEAD_TOL[precision] * max(1.0, float(want.abs().max()))


def test_three_steps_follow_the_fp64_trajectory_and_nothing_changes_until_commit():
    """2 and 3: three loss_and_grads + step() rounds against oracle autograd + AdamW on the CPU; meanwhile exit_outputs and a dynamic step
    of the engine stay bit-identical to what the engine computed before it had a trainer"""
    cfg, g, sd, model = _model("all_exits.npz", "fp32")
    P, rl, tl, pose, grip, w_bin = _inputs(cfg, g)
    eng = model.engine

    def engine_fingerprint():
        eng.reset()
        eng.step(g["rgb"][0, 0].cuda(), g["grip"][0, 0].cuda(), g["ids"][:1].long().cuda(), g["mask"][:1].bool().cuda())
        torch.cuda.synchronize()
        return eng.exit_outputs(P, rl, tl).clone(), _step_words(eng), eng.h_state.clone()
    before = engine_fingerprint()

    heads = _head_inputs(cfg, P, rl, tl)
    names = [k for k in sd if k.startswith(("extra_exit.", "lm_head.", "lm_exit_modules."))]
    p64 = OrderedDict((k, sd[k].detach().float().double()) for k in names)
    # Adam's eps for this comparison.  One update is lr g / (|g| + eps) (step 1; later steps alike): near g = 0 it turns an absolute
    # gradient error dg into lr dg / eps, so an f32 gradient - good to e max|g| per tensor, which is what the kernel gate measures - gives a
    # parameter error e (lr / eps) max|g| / max|p| relative to its tensor.  With torch's default eps = 1e-8 that factor is ~1e5 here and
    # the trajectory of ANY f32 evaluation is decided by the signs of its smallest gradient entries (two f32 evaluations on the CPU
    # differ by up to 7x e32 after one step).  eps = lr max_k(max|g_k| / max|p_k|), from the fp64 reference at the start, makes the factor
    # <= 1: the parameter gate then asks of the trajectory what the kernel gate asks of the gradient.  deer_adamw_step at eps = 1e-8 is
    # tests/test_adamw_kernel.py's.
    g0 = {k: torch.zeros_like(v) for k, v in p64.items()}
    for prefix, X in heads:
        sub = OrderedDict((k, v) for k, v in p64.items() if k.startswith(prefix))
        for k, gr in ref.loss_and_grads(sub, cfg, prefix, X, pose.double(), grip.double(), w_bin)[1].items():
            g0[k] += gr
    eps = LR * max(float(g0[k].abs().max()) / float(p64[k].abs().max()) for k in p64)
    print(f"Adam eps for the trajectory: {eps:.3e}")
    tr = eng.head_trainer(sd, lr=LR, eps=eps)
    m64 = {k: torch.zeros_like(v) for k, v in p64.items()}
    v64 = {k: torch.zeros_like(v) for k, v in p64.items()}
    p32 = OrderedDict((k, sd[k].detach().float().clone().requires_grad_(True)) for k in names)
    opt = torch.optim.AdamW(list(p32.values()), lr=LR, betas=(0.9, 0.999), eps=eps, weight_decay=0.0)
    b1, b2 = 0.9, 0.999
    for t in range(1, 4):
        tr.zero_grad()
        tr.loss_and_grads(P, rl, tl, pose, grip, w_bin)
        tr.step()
        g64 = {k: torch.zeros_like(v) for k, v in p64.items()}
        for k in p32:
            p32[k].grad = torch.zeros_like(p32[k])
        for prefix, X in heads:                                   # extra_exit appears twice: its gradients add
            sub64 = OrderedDict((k, v) for k, v in p64.items() if k.startswith(prefix))
            for k, gr in ref.loss_and_grads(sub64, cfg, prefix, X, pose.double(), grip.double(), w_bin)[1].items():
                g64[k] += gr
            sub32 = OrderedDict((k, v.detach().double()) for k, v in p32.items() if k.startswith(prefix))
            for k, gr in ref.loss_and_grads(sub32, cfg, prefix, X, pose.double(), grip.double(), w_bin, dtype=torch.float32)[1].items():
                p32[k].grad += gr
        opt.step()
        for k in p64:                                             # torch/optim/adamw.py _single_tensor_adamw, weight_decay 0
            m64[k] = m64[k] + (g64[k] - m64[k]) * (1 - b1)
            v64[k] = v64[k] * b2 + (1 - b2) * g64[k] * g64[k]
            p64[k] = p64[k] - (LR / (1 - b1 ** t)) * m64[k] / (v64[k].sqrt() / (1 - b2 ** t) ** 0.5 + eps)
        got = {k: v.cpu().double() for k, v in tr.state_dict().items()}
        assert set(got) == set(p64)
        kt, worst, bad = K * 2 ** t, 0.0, []
        for k in p64:
            scale = float(p64[k].abs().max())
            e_dev = float((got[k] - p64[k]).abs().max()) / scale
            e32 = float((p32[k].detach().double() - p64[k]).abs().max()) / scale
            worst = max(worst, e_dev / e32 if e32 > 0 else 0.0)
            if e_dev > kt * e32 + FLOOR:
                bad.append((k, e_dev, e32))
        print(f"step {t}: worst e_dev / e32 over {len(p64)} tensors {worst:.2f} (gate {kt})")
        assert not bad, bad
    after = engine_fingerprint()
    assert [torch.equal(a, b) for a, b in zip(before, after)] == [True, True, True]


def test_commit_equals_a_fresh_engine_built_from_the_trained_state_dict():
    """4: after commit(), exit_outputs of the engine - and of a sibling that shares its arena - equals, bit for bit, a fresh engine built
    from trainer.state_dict() merged into the original state dict"""
    cfg, g, sd, model = _model("all_exits.npz", "fp16", fresh=True)
    P, rl, tl, pose, grip, w_bin = _inputs(cfg, g)
    eng = model.engine
    sib = eng.sibling(2)
    old = eng.exit_outputs(P, rl, tl).clone()
    tr = eng.head_trainer(sd, lr=LR)
    for _ in range(2):
        tr.zero_grad()
        tr.loss_and_grads(P, rl, tl, pose, grip, w_bin)
        tr.step()
    tr.commit()
    new = eng.exit_outputs(P, rl, tl)
    assert not torch.equal(new, old)
    merged = dict(sd)
    merged.update({k: v.cpu() for k, v in tr.state_dict().items()})
    fresh = MPTFlamingo(cfg, merged, window_size=cfg.window_size, precision="fp16")
    assert torch.equal(new, fresh.engine.exit_outputs(P, rl, tl))
    assert torch.equal(new, sib.exit_outputs(P, rl, tl))
    # a dynamic step after the commit is the fresh engine's too (the captured pieces read the arena at replay)
    for e in (eng, fresh.engine):
        e.reset()
        e.step(g["rgb"][0, 0].cuda(), g["grip"][0, 0].cuda(), g["ids"][:1].long().cuda(), g["mask"][:1].bool().cuda())
    torch.cuda.synchronize()
    assert torch.equal(_step_words(eng), _step_words(fresh.engine)) and torch.equal(eng.h_state, fresh.engine.h_state)


def test_twenty_steps_lower_every_heads_loss_on_the_fixed_batch():
    """5: evaluate.finetune_exit_heads, 20 steps at lr 1e-3 on one batch; every head's loss, measured by the existing
    exit_losses_on_windows after commit() with the same layer tables before and after, goes down (a sign test, no rate)"""
    cfg, g, sd, model = _model("all_exits.npz", "fp16", fresh=True)
    batch = dict(images=g["rgb"], gripper=g["grip"], input_ids=g["ids"].long(), attention_mask=g["mask"].bool(), labels=g["labels"])

    def measure():
        random.seed(7)
        return exit_losses_on_windows(model, [batch], w_bin=float(g["w_bin"]), generator=torch.Generator().manual_seed(7))
    before = measure()
    random.seed(3)
    trainer, history = finetune_exit_heads(model, [batch], 20, sd, lr=LR, w_bin=float(g["w_bin"]), generator=torch.Generator().manual_seed(3))
    after = measure()
    print("loss before", before["loss"], "after", after["loss"], "heads", before["heads"])
    assert history.shape == (20, len(before["heads"])) and bool(torch.isfinite(history).all())
    assert all(a < b for a, b in zip(after["loss"], before["loss"])), (before["loss"], after["loss"])


@pytest.mark.parametrize("name,layerwise", [("all_exits.npz", True), ("all_exits_ms2.npz", True), ("all_exits.npz", False)])
def test_layerwise_multi_step_and_plain_models_take_a_step(name, layerwise):
    """6: a layerwise_exit_eval model, an A = 2 model and a model without per-layer heads (extra_exit serves the last layer too: three
    runs, one gradient) each run one round without refusal; the losses are finite and the parameters move"""
    cfg, g, sd, model = _model(name, "fp16", layerwise)
    P, rl, tl, pose, grip, w_bin = _inputs(cfg, g)
    tr = model.engine.head_trainer(sd, lr=LR)
    p0 = {k: v.clone() for k, v in tr.state_dict().items()}
    losses = tr.loss_and_grads(P, rl, tl, pose, grip, w_bin)
    tr.step()
    assert losses.shape == ((len(cfg.exit_ids()) - 1 if layerwise else 0) + 3,) and bool(torch.isfinite(losses).all())
    assert len(tr.heads) == (len(cfg.exit_ids()) + 1 if layerwise else 1)
    moved = [k for k, v in tr.state_dict().items() if not torch.equal(v, p0[k])]
    assert len(moved) == len(p0), sorted(set(p0) - set(moved))
