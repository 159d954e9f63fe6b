"""Operating-point sweeps on the host (no GPU): evaluate_policy_batched(operating_points=...) deals (point, chain) jobs and keeps the
bookkeeping per point (stub engine), the (k, n) metrics of all points reduce in ONE all-reduce (two gloo ranks), k controllers come from
one value matrix, and every point's report ends with the three lines the reference's Bayesian optimisation reads back."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from deer_vla_amd import distributed as dd
from deer_vla_amd import rollout as ro
from deer_vla_amd.value_net import ExitController, controllers_from_values

EXITS = [1, 3, 5, 7, 9, 11]


class _Cfg:
    n_layers = 12


class _Stub:
    """BatchedModelWrapper stand-in: every slot exits at its controller's cap minus (its step % 2) * 2 (an exit when the cap allows)
    - exits that depend on the operating point and the step inside the sub-task only, like a real env batch on constant frames"""

    def __init__(self, B, exit_controller):
        self.B = B
        self.exit_controller = exit_controller
        self.model = type("M", (), {})()
        self.model.module = type("MM", (), {})()
        self.model.module.lang_encoder = type("L", (), {"config": _Cfg()})()
        self.current_exit_layers = [-1] * B
        self.calls = []

    def reset_env(self, b):
        pass

    def check_instructions(self, goals):
        pass

    def step(self, obs_list, goals, env_steps=None, exit_controller=None):
        ctl = exit_controller if exit_controller is not None else self.exit_controller
        ctls = ctl if isinstance(ctl, list) else [ctl.module] * self.B
        self.calls.append([c.max_layer for c in ctls])
        self.current_exit_layers = [max(c.max_layer - (t % 2) * 2, EXITS[0]) for c, t in zip(ctls, env_steps)]
        return [None] * self.B


class _Env(ro.DebugEnv):
    def __init__(self):
        self.t = 0

    def step(self, action):
        self.t += 1
        return None, 0.0, False, self.t

    def reset(self, **kwargs):
        self.t = 0

    def get_obs(self):
        return None

    def get_info(self):
        return self.t


def _ctl(max_layer, thr=0.02):
    c = ExitController(None, EXITS, max_layer=max_layer)
    c._set_threshold_value([thr] * (c.real_num_exit - 1) + [1e5])
    return c


SEQS = [(None, ["a", "b", "c"]), (None, ["b", "a"]), (None, ["c"]), (None, ["a", "c", "b"]), (None, ["b", "b"])]
ANN = {"a": ["open"], "b": ["push"], "c": ["turn"]}


def _checker(start, cur, sub):                                      # sub-task "a" never succeeds within ep_len, the others after 3 steps
    return sub != "a" and cur - start >= 3


def test_sweep_deals_point_chain_jobs_and_keeps_bookkeeping_per_point(capsys):
    points = [_ctl(12), _ctl(8), _ctl(4)]
    sweep = ro.evaluate_policy_batched(_Stub(3, None), [_Env() for _ in range(3)], SEQS, ANN, _checker, ep_len=4, report=True,
                                       operating_points=points)
    text = capsys.readouterr().out
    assert isinstance(sweep, list) and len(sweep) == 3
    blocks = text.split("Operating point ")[1:]
    volatile = ("wall_s_mean", "steps_per_s")
    for p, c in enumerate(points):
        stub = _Stub(3, c)
        one = ro.evaluate_policy_batched(stub, [_Env() for _ in range(3)], SEQS, ANN, _checker, ep_len=4, report=True)
        one_text = capsys.readouterr().out
        assert {k: v for k, v in sweep[p].items() if k not in volatile} == {k: v for k, v in one.items() if k not in volatile}, p
        assert blocks[p].split("\n", 1)[1] == one_text
        assert sweep[p]["n_chains"] == len(SEQS)                          # every chain ran once for this point
        assert all(sweep[p]["exit_hist"][i] == 0 for i in range(c.max_layer + 1, 12))
    assert [s["avg_exit"] for s in sweep] != [sweep[0]["avg_exit"]] * 3   # the points differ


def test_sweep_slots_switch_point_per_job_and_idle_slots_keep_the_largest_cap():
    points = [_ctl(12), _ctl(4)]
    stub = _Stub(2, None)
    ro.evaluate_policy_batched(stub, [_Env() for _ in range(2)], SEQS[:3], ANN, _checker, ep_len=4, operating_points=points)
    caps = {c for call in stub.calls for c in call}
    assert caps == {11, 3}
    assert stub.calls[0] == [11, 3]                                        # chain 0 for point 0, then chain 0 for point 1
    assert max(stub.calls[-1]) == 11                                       # idle slots carry the largest cap (the plan stays put)


def test_controllers_from_one_value_matrix_equal_separate_calibrations():
    g = torch.Generator().manual_seed(0)
    values = torch.rand(6, 50, generator=g) * 0.1
    ratios, caps = [0.6, 0.8, 1.0, 1.2], [12, 12, 6, 8]
    ctls = controllers_from_values(None, EXITS, values, ratios, caps)
    for c, r, m in zip(ctls, ratios, caps):
        ref = ExitController(None, EXITS, max_layer=m)
        ref.set_threshold_from_values(values, r)
        assert c.max_layer == ref.max_layer and c.threshold_list() == ref.threshold_list()
    assert [c.max_layer for c in controllers_from_values(None, EXITS, values, ratios[:2], 6)] == [5, 5]
    with pytest.raises(ValueError):
        controllers_from_values(None, EXITS, values, ratios, [12])


def get_observation(lines):
    """bayesian_optimization.get_observation, restated: the last three lines of an evaluation log are the thresholds (comma separated),
    the average successful length and the average exit layer"""
    thresholds = list(map(float, lines[-3].split(",")))
    return thresholds, float(lines[-2]), float(lines[-1])


def test_point_report_parses_like_the_references_log(tmp_path):
    c = _ctl(8, thr=0.0123)
    log = tmp_path / "point.log"
    log.write_text("Results for Epoch 0:\n...\n" + ro.operating_point_log(c.threshold_list(), 2.4, 5.75))
    with open(log) as fh:
        thr, avg_len, avg_exit = get_observation(fh.readlines())
    assert thr == c.threshold_list() and avg_len == 2.4 and avg_exit == 5.75


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
    k = 3
    rows, singles = [], []
    for p in range(k):
        results = [(rank + p + i) % 6 for i in range(4)]
        exits = [(rank * 3 + p + i) % 12 for i in range(7)]
        row = torch.cat([dd.pack_metrics(results, exits, 12, llm_time=0.25 * (p + 1)), torch.tensor([float(10 * p + rank)], dtype=torch.float64)])
        rows.append(row)
        singles.append(dd.reduce_metrics(row, n_extra=1))               # k collectives, one per point
    calls = []
    orig = dist.all_reduce

    def counting(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    dist.all_reduce = counting
    try:
        packed = dd.reduce_metrics_points(torch.stack(rows), n_extra=1)   # ONE collective for all points
    finally:
        dist.all_reduce = orig
    q.put((rank, packed, singles, len(calls)))
    dist.destroy_process_group()


def test_two_rank_gloo_packed_point_reduce_equals_single_point_reduces():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=120) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, packed, singles, n_calls in out:
        assert n_calls == 1
        assert packed == singles
    assert out[0][1] == out[1][1]
    assert out[0][1][2]["extra"] == [41.0] and out[0][1][0]["n_chains"] == 8
