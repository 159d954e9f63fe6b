"""Host side of the per-exit demonstration loss (no GPU): the goldens of the reference's all-exits forward load and carry the heads in
``all_outputs`` order, evaluate.py's label handling reproduces the stored labels, the layer tables are drawn in the reference's order, the
ops.py refusals fire and the per-head (sum, count) packing survives a gloo all-reduce."""
import dataclasses
import os
import random

import pytest
import torch

from golden_util import load
from deer_vla_amd import ops
from deer_vla_amd.config import deer_tiny
from deer_vla_amd.evaluate import split_labels, window_batch_inputs

NAMES = ["all_exits.npz", "all_exits_ms2.npz", "all_exits_state.npz"]


@pytest.mark.parametrize("name", NAMES)
def test_golden_loads_with_heads_in_all_outputs_order(name):
    cfg, seed, g = load(name)
    bs, W = g["rand_layers"].shape
    A = max(1, cfg.multi_step_action)
    assert (bs, W) == (2, 4) == tuple(g["two_layers"].shape) and W == cfg.window_size and g["ids"].shape == (2, 6)
    assert int((~g["mask"].bool()).sum()) == 1                                        # one right-padded row
    n_exit = int(g["n_exit_outputs"])
    Hn = g["pose"].shape[0]
    assert n_exit == len(cfg.exit_ids()) - 1 and Hn == n_exit + 3                     # exit_outputs + [final, extra, extra2]
    if cfg.layerwise_exit_eval:
        assert ops.exit_head_count(cfg) == Hn
    else:                                                                             # use_state: this repository builds no per-layer heads with it
        assert cfg.use_state and ops.exit_head_count(cfg) == 3
    assert g["pose"].shape == (Hn, bs, W, 6 * A) and g["gprob"].shape == g["glogit"].shape == (Hn, bs, W, A)
    assert g["num"].shape == g["bin"].shape == (Hn, bs, W) and g["loss"].shape == (Hn,)
    assert g["pooled"].shape == (bs * W, len(cfg.exit_ids()), cfg.d_model)
    assert torch.allclose(torch.sigmoid(g["glogit"]), g["gprob"], atol=1e-6)
    exits = set(cfg.exit_ids())
    assert set(g["rand_layers"].reshape(-1).tolist()) <= exits and set(g["two_layers"].reshape(-1).tolist()) <= exits
    # strategy 2: constant in each of its two segments
    p = int(g["prev_len"])
    two = g["two_layers"]
    assert 1 <= p <= W and bool((two[:, :p] == two[:, :1]).all()) and (p == W or bool((two[:, p:] == two[:, p:p + 1]).all()))
    # the stored losses are what torch.nn.functional gives on the stored outputs and labels
    F = torch.nn.functional
    num = F.huber_loss(g["pose"], g["label_pose"][None].expand_as(g["pose"]), reduction="none").mean(-1)
    bin_ = F.binary_cross_entropy_with_logits(g["glogit"], g["label_grip01"][None].expand_as(g["glogit"]), reduction="none").mean(-1)
    assert torch.allclose(num, g["num"], atol=1e-6) and torch.allclose(bin_, g["bin"], atol=1e-6)
    assert torch.allclose((num + float(g["w_bin"]) * bin_).mean((1, 2)), g["loss"], atol=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_label_handling_reproduces_the_stored_labels(name):
    cfg, seed, g = load(name)
    pose, grip01 = split_labels(g["labels"], cfg.multi_step_action)
    assert torch.equal(pose, g["label_pose"]) and torch.equal(grip01, g["label_grip01"])
    assert set(grip01.reshape(-1).tolist()) <= {0.0, 1.0}
    if cfg.multi_step_action > 1:                                                     # the flat (bs, W, A * 7) layout too
        p2, g2 = split_labels(g["labels"].flatten(2), cfg.multi_step_action)
        assert torch.equal(p2, pose) and torch.equal(g2, grip01)
    with pytest.raises(ValueError):
        split_labels(g["labels"][..., :6], cfg.multi_step_action)
    W, S = cfg.window_size, cfg.image_size
    kw = window_batch_inputs(dict(images=g["rgb"], gripper=g["grip"], input_ids=g["ids"], attention_mask=g["mask"], state=g["state"]), W)
    assert kw["vision_x"].shape == (2 * W, 1, 1, 3, S, S) and kw["lang_x"].shape == (2 * W, 6) and kw["state_tensor"].shape == (2 * W, 1, 1, 15)
    assert torch.equal(kw["lang_x"][W - 1], g["ids"][0]) and torch.equal(kw["lang_x"][W], g["ids"][1])
    with pytest.raises(ValueError):
        window_batch_inputs(dict(images=g["rgb"], gripper=g["grip"], input_ids=g["ids"]), W + 1)


@pytest.mark.parametrize("name", NAMES)
def test_host_draws_equal_the_reference_tables(name):
    from deer_vla_amd.flamingo_mpt import MPTFlamingo
    cfg, seed, g = load(name)
    model = MPTFlamingo(cfg, None, window_size=cfg.window_size)                       # no engine: the draws are host work
    torch.manual_seed(int(g["torch_seed"]))
    random.seed(int(g["py_seed"]))
    rl, tl = model.draw_exit_layers(2, cfg.window_size)
    assert torch.equal(rl, g["rand_layers"]) and torch.equal(tl, g["two_layers"])


def test_ops_refusals():
    cfg = deer_tiny(layerwise_exit_eval=True)
    exits = cfg.exit_ids()
    NE, d = len(exits), cfg.d_model
    ok = torch.tensor(exits)[torch.zeros(2, 4, dtype=torch.long)]
    assert ops.exit_outputs_shapes(cfg, (2, 4, NE, d), ok, ok) == (2, 4, NE, NE + 2, 1)
    assert ops.exit_head_count(deer_tiny()) == 3
    with pytest.raises(ValueError, match="feats"):
        ops.exit_outputs_shapes(cfg, (2, 4, NE + 1, d), ok, ok)
    with pytest.raises(ValueError, match="feats"):
        ops.exit_outputs_shapes(cfg, (2, 4, NE, d + 4), ok, ok)
    with pytest.raises(ValueError, match="feats"):
        ops.exit_outputs_shapes(cfg, (8, NE, d), ok, ok)
    with pytest.raises(ValueError, match="two_layers"):
        ops.exit_outputs_shapes(cfg, (2, 4, NE, d), ok, ok[:, :3])
    bad = ok.clone()
    bad[1, 2] = exits[0] + 1 if exits[0] + 1 not in exits else 0
    with pytest.raises(ValueError, match="not exit layers"):
        ops.exit_outputs_shapes(cfg, (2, 4, NE, d), bad, ok)
    with pytest.raises(ValueError, match="not exit layers"):
        ops.exit_outputs_shapes(cfg, (2, 4, NE, d), ok, bad)
    with pytest.raises(ValueError, match="without use_state"):
        ops.exit_outputs_shapes(cfg, (2, 4, NE, d), ok, ok, torch.zeros(2, 4, 15))
    st = dataclasses.replace(deer_tiny(), use_state=True)
    with pytest.raises(ValueError, match="needs the robot state"):
        ops.exit_outputs_shapes(st, (2, 4, NE, d), ok, ok)
    with pytest.raises(ValueError, match="robot_obs row"):
        ops.exit_outputs_shapes(st, (2, 4, NE, d), ok, ok, torch.zeros(7, 15))
    assert ops.exit_outputs_shapes(st, (2, 4, NE, d), ok, ok, torch.zeros(8, 1, 1, 15))[3] == 3
    assert ops.exit_losses_shapes(cfg, (5, 2, 4, 8), (2, 4, 6), (2, 4, 1)) == (5, 8, 1)
    with pytest.raises(ValueError, match="8 A"):
        ops.exit_losses_shapes(cfg, (5, 2, 4, 7), (2, 4, 6), (2, 4, 1))
    with pytest.raises(ValueError, match="labels"):
        ops.exit_losses_shapes(cfg, (5, 2, 4, 8), (2, 3, 6), (2, 4, 1))
    with pytest.raises(ValueError, match="labels"):
        ops.exit_losses_shapes(cfg, (5, 2, 4, 8), (2, 4, 6), (2, 4, 2))


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    from deer_vla_amd import distributed as dd
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sums = torch.arange(15, dtype=torch.float64).reshape(3, 5) * (rank + 1)
    s, n = dd.reduce_exit_losses(sums, 10 * (rank + 1))
    q.put((rank, s.tolist(), n))
    dist.destroy_process_group()


def test_exit_loss_packing_round_trips_and_reduces_over_gloo():
    from deer_vla_amd import distributed as dd
    sums = torch.rand(3, 5, dtype=torch.float64)
    packed = dd.pack_exit_losses(sums, 96)
    assert packed.dtype == torch.float64 and packed.shape == (16,)
    s, n = dd.unpack_exit_losses(packed)
    assert torch.equal(s, sums) and n == 96
    s, n = dd.reduce_exit_losses(sums, 96)                                            # no process group: identity
    assert torch.equal(s, sums) and n == 96
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = [q.get(timeout=120) for _ in ps]
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    want = (torch.arange(15, dtype=torch.float64).reshape(3, 5) * 3).tolist()
    for _, s, n in got:
        assert s == want and n == 30
