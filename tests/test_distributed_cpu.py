"""N>1 path on CPU: world_size-2 gloo processes exercise the rank sharding, the single metric all-reduce and the
calibration all_gather of deer_vla_amd.distributed (the GPU path uses the same calls over RCCL)."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deer_vla_amd import distributed as dd
from deer_vla_amd.value_net import ExitController


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seqs = list(range(8))
    mine = dd.shard_sequences(seqs, rank, world)
    # fake per-chain results: chain i succeeds i % 6 subtasks; each chain takes 3 steps exiting at layer (i % 4) * 2 + 1
    results = [i % 6 for i in mine]
    exits = [(i % 4) * 2 + 1 for i in mine for _ in range(3)]
    m = dd.reduce_metrics(dd.pack_metrics(results, exits, 12, llm_time=0.5))
    vals = torch.arange(6 * 5, dtype=torch.float32).view(6, 5) + 100 * rank
    gathered = dd.all_gather_values(vals)
    ctl = ExitController(None, [1, 3, 5, 7, 9, 11], max_layer=12)
    ctl.set_threshold_from_values(gathered, 0.8)
    dist.barrier()
    q.put((rank, mine, m, tuple(gathered.shape), ctl.threshold_list()))
    dist.destroy_process_group()


def test_two_rank_gloo_sharding_and_metric_reduce():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=120) for _ in range(world)])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (r0, mine0, m0, shp0, thr0), (r1, mine1, m1, shp1, thr1) = out
    assert mine0 == [0, 1, 2, 3] and mine1 == [4, 5, 6, 7]               # contiguous rank blocks (eval_utils.py:523-527)
    assert m0 == m1                                                       # every rank sees the global metrics
    results = [i % 6 for i in range(8)]
    assert m0["n_chains"] == 8 and abs(m0["avg_seq_len"] - sum(results) / 8) < 1e-12
    assert m0["chain_sr"][0] == sum(1 for r in results if r >= 1) / 8
    assert m0["n_steps"] == 24 and abs(m0["avg_exit"] - sum((i % 4) * 2 + 2 for i in range(8)) / 8) < 1e-12
    assert sum(m0["exit_hist"]) == 24 and m0["exit_hist"][1] == 6
    assert abs(m0["llm_time"] - 1.0) < 1e-12
    assert shp0 == shp1 == (6, 10) and thr0 == thr1


def test_single_process_fallbacks():
    assert dd.world_info() == (0, 1)
    m = dd.reduce_metrics(dd.pack_metrics([5, 0], [1, 11], 12))
    assert m["avg_seq_len"] == 2.5 and m["avg_exit"] == 7.0
    m = dd.reduce_metrics(torch.cat([dd.pack_metrics([5, 0], [1, 11], 12), torch.tensor([42.0], dtype=torch.float64)]), n_extra=1)
    assert m["extra"] == [42.0] and m["avg_exit"] == 7.0 and len(m["exit_hist"]) == 12
    v = torch.ones(2, 3)
    assert dd.all_gather_values(v) is v
    try:
        dd.shard_sequences(list(range(7)), 0, 2)
        assert False
    except AssertionError:
        pass


# ---- the same helpers over RCCL (backend "nccl"): CPU tensors must be staged through the device ------------------------
import pytest  # noqa: E402


def _nccl_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        dev = rank % torch.cuda.device_count()                    # one rank per VISIBLE device (a 1-GPU box puts both on device 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
        assert dist.get_backend() == "nccl"
        m = dd.reduce_metrics(dd.pack_metrics([rank + 1], [1 + 2 * rank] * 3, 12))      # CPU tensor in, as rollout.py passes it
        vals = torch.arange(6 * 4, dtype=torch.float32).view(6, 4) + 100 * rank           # CPU deltas, as generate_values returns
        g = dd.all_gather_values(vals)
        q.put((rank, "ok", m["n_chains"], m["avg_seq_len"], tuple(g.shape), float(g[0, 4]), g.device.type))
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        q.put((rank, "error", repr(e)))


@pytest.mark.gpu
def test_two_rank_nccl_collectives_accept_cpu_tensors():
    """NCCL/RCCL cannot reduce CPU tensors; reduce_metrics / all_gather_values now stage them through the device.
    One rank per visible device: on a box with >= 2 GPUs this is a real 2-GPU RCCL run and MUST pass; with one GPU RCCL refuses
    two ranks on one device and the test skips (no RCCL collective of this repo has executed on hardware yet - DESIGN.md 6)."""
    world, port = 2, _free_port()
    multi = torch.cuda.device_count() >= 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_nccl_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        out = sorted([q.get(timeout=180) for _ in range(world)])
    except Exception:
        for p in procs:
            p.kill()
        assert not multi, "RCCL did not come up with two ranks on two devices within 180 s"
        pytest.skip("RCCL did not come up with two ranks on one device within 180 s")
    for p in procs:
        p.join(30)
        if p.is_alive():
            p.kill()
    if any(o[1] == "error" for o in out):
        msg = " | ".join(o[2] for o in out if o[1] == "error")
        if not multi and ("uplicate" in msg or "invalid usage" in msg.lower() or "ncclInvalidUsage" in msg):
            pytest.skip("RCCL refuses two ranks on one device: " + msg[:200])
        raise AssertionError(msg)
    for r, _, n_chains, avg_len, shp, g04, devtype in out:
        assert n_chains == 2 and abs(avg_len - 1.5) < 1e-12 and shp == (6, 8) and g04 == 100.0 and devtype == "cpu"


@pytest.mark.gpu
def test_bench_with_eight_ranks_through_torch_distributed_run():
    """the driver's 8-GPU command line, ``python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 ... bench.py
    --gpus 8``, end to end on whatever box this runs on: eight processes, eight model replicas, barrier-bracketed timed region, the packed
    all-reduce, the per-rank device report (``ranks`` / ``distinct_devices``).  With fewer than 8 GPUs every rank uses device 0 and the
    process group is gloo (DEER_BENCH_SINGLE_DEVICE / DEER_BENCH_BACKEND: RCCL refuses several ranks on one device); on an 8-GPU box
    the same test runs one rank per GPU over RCCL.  Reduced-dims model (``--workload tiny``): this exercises the N = 8 code path
    (rank slicing as eval_utils.py:523-527: 224 chains = 8 x 28), not performance."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    real = torch.cuda.device_count() >= 8
    env = dict(os.environ)
    if not real:
        env.update(DEER_BENCH_SINGLE_DEVICE="1", DEER_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "6", "--warmup", "2", "--workload", "tiny", "--calib-steps", "24",
           "--burn-in", "0", "--on-policy-steps", "6", "--scripted-steps", "0", "--latency-reps", "0", "--no-cpu-baseline", "--batched-envs", "0",
           "--surface-steps", "0", "--no-roofline", "--full"]
    p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 8 and out["rccl_world"] == 8 and out["scaling"] == "weak" and out["value"] > 0 and out["steps"] == 6
    assert out["backend"] == ("nccl" if real else "gloo")
    assert sorted(r["rank"] for r in out["ranks"]) == list(range(8))
    assert out["distinct_devices"] == (8 if real else 1)
    pr = out["per_rank_steps_per_s"]                              # stragglers are visible in the line
    assert 0 < pr["min"] <= pr["max"] and pr["slowest_over_fastest_time"] >= 1.0 and abs(pr["min"] * 8 - out["value"]) < 0.02 * out["value"] + 1
    assert abs(out["config"]["per_gpu_steps_per_s"] * 8 - out["value"]) < 0.05 * out["value"]
    op = out["on_policy"]                                         # the real criterion over all ranks too
    assert op["steps"] == 6 and op["value"] > 0 and 0 < op["per_rank_steps_per_s"]["min"] <= op["per_rank_steps_per_s"]["max"]
    assert abs(op["per_rank_steps_per_s"]["min"] * 8 - op["value"]) < 0.02 * op["value"] + 1 and 1.0 <= op["avg_exit_layer"] <= 12.0
    from deer_vla_amd import distributed as dd2
    seqs = list(range(224))
    assert [len(dd2.shard_sequences(seqs, r, 8)) for r in range(8)] == [28] * 8 and dd2.shard_sequences(seqs, 7, 8)[-1] == 223
