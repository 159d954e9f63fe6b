"""Host-side mirror of robot_flamingo/models/value_net.py for the native engine.

``ExitController`` / ``ActionValueNet`` keep the reference's names, constructor arguments, attributes
(``thresholds`` dict, ``exit_id_list``, ``max_layer``, ``steps_per_stage``, ``cur_exit_id``, ``.module``) and
methods (``set_timestep``, ``_set_threshold_value``, ``set_threshold``), but the criterion itself
(value_net.py:105-133,277-297) is evaluated ON THE DEVICE by ``head_final_kernel``: when a model built by
``deer_vla_amd.factory`` receives one of these controllers it passes thresholds / max_layer / steps_per_stage to
the engine and the Python callable is bypassed (SURVEY §8b "exit-controller protocol").  Calling the controller
like the reference does (``ctl(all_hidden_states, b_idx) -> bool``) still works - it then drives the head kernels
eagerly and syncs once per exit check (slow host loop, used by tests and by foreign LLM loops).
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import torch


def exit_counts(n_sample: int, real_num_exit: int, exit_ratio: float, exit_dist: str = "exp",
                model_name: str = "mpt_dolly_3b") -> List[int]:
    """How many calibration samples every exit is to take (value_net.py:214-244): ``floor(n_sample * probs[k])`` with probs ~
    exit_ratio**k ('exp'), gaussian or gamma, normalised, in the reference's f32 torch arithmetic - the one place where these integers
    come from, for the host solver and for the device solver (``DeerEngine.solve_thresholds``) alike.  Returns real_num_exit ints; the
    last exit takes whoever is left, its entry is 0 and no solver reads it."""
    if exit_dist == "exp":
        probs = torch.tensor([float(exit_ratio) ** k for k in range(1, real_num_exit + 1)], dtype=torch.float32)
    elif exit_dist == "gauss":
        probs = torch.tensor([math.exp(-(i - exit_ratio) ** 2 / 2.0) for i in range(real_num_exit)], dtype=torch.float32)
    elif exit_dist == "gamma":
        import scipy.stats
        probs = torch.tensor([scipy.stats.gamma.pdf(float(v), exit_ratio, scale=2.0) for v in range(1, real_num_exit + 1)],
                             dtype=torch.float32)
    else:
        raise ValueError("Unsupported exit distribution")
    if "mpt_9b" in model_name:
        probs[0] = 0                     # value_net.py:235-236
    probs = probs / probs.sum()
    return [math.floor(n_sample * probs[k]) for k in range(real_num_exit - 1)] + [0]


def solve_from_counts(values: torch.Tensor, counts: Sequence[int], leq: bool = True):
    """The selection loop of ``ExitController.set_threshold`` (value_net.py:242-262) for given counts (``exit_counts``), on the host:
    for every exit k but the last the threshold is the value of the counts[k]-th not-yet-exited sample of values[k] in sorted order,
    after which every sample with value <= T[k] (>= for not leq) counts as exited.  Returns (T (n_exit,) f32, the number of samples
    that left at every exit - the last one's are those still alive)."""
    values = values.detach().to("cpu", torch.float32)
    real_num_exit, n_sample = len(counts), values.shape[1]
    T = torch.full((real_num_exit,), -1e8 if leq else 1e8, dtype=torch.float32)
    filtered = torch.zeros(n_sample, dtype=torch.bool)
    left = []
    for k in range(real_num_exit - 1):
        out_n = counts[k]
        order = values[k].argsort(descending=not leq, stable=True)
        alive = ~filtered[order]
        rank = alive.cumsum(0)
        hit = (alive & (rank == out_n)).nonzero()
        if out_n > 0 and hit.numel() > 0:
            T[k] = values[k][order[hit[0, 0]]]
        before = int(filtered.sum())
        filtered |= (values[k] <= T[k]) if leq else (values[k] >= T[k])
        left.append(int(filtered.sum()) - before)
    T[real_num_exit - 1] = 1e8 if leq else -1e8
    return T, left + [n_sample - int(filtered.sum())]


def solve_thresholds(values: torch.Tensor, real_num_exit: int, exit_ratio: float, exit_dist: str = "exp",
                     leq: bool = True, model_name: str = "mpt_dolly_3b") -> torch.Tensor:
    """Threshold solver of ``ExitController.set_threshold`` (value_net.py:203-260), vectorised.

    values: (n_stage, n_sample) deltas gathered over the calibration set.  For every exit k (except the last)
    the threshold is the value of the ``floor(n * probs[k])``-th not-yet-exited sample in sorted order, after
    which every sample with value <= T[k] counts as exited.  probs ~ exit_ratio**k ('exp'), gaussian or gamma.
    """
    return solve_from_counts(values, exit_counts(values.shape[1], real_num_exit, exit_ratio, exit_dist, model_name), leq)[0]


def _solve_points(values: torch.Tensor, counts: Sequence[Sequence[int]], leq: bool, engine=None):
    """Thresholds and exit mixes of k points with the same number of exits: rows of floats, rows of ints.  With an engine and device
    values: ONE ``DeerEngine.solve_thresholds`` call and ONE read of its k x (2 n_exit + 1) words, after which the kernel's NaN count is
    checked; else the host solver, point by point."""
    if engine is None or not values.is_cuda:
        solved = [solve_from_counts(values[: len(c)], c, leq) for c in counts]
        return [t.tolist() for t, _ in solved], [n for _, n in solved]
    k, n_exit = len(counts), len(counts[0])
    T, left, status = engine.solve_thresholds(values, torch.tensor(counts, dtype=torch.int32), leq, return_status=True)
    words = torch.cat([T.view(torch.int32).reshape(-1), left.reshape(-1), status]).cpu()
    if int(words[2 * k * n_exit:].sum()) != 0:
        raise ValueError("NaN in calibration values")
    return (words[: k * n_exit].view(torch.float32).view(k, n_exit).tolist(),
            words[k * n_exit: 2 * k * n_exit].view(k, n_exit).tolist())


def predicted_exit_mix(exit_counts: Sequence[int], exit_id_list: Sequence[int]):
    """(fractions, average_exit_layer) of an operating point ON THE CALIBRATION SET: exit_counts[e] samples of the calibration matrix
    leave at exit ``exit_id_list[e]`` under the solved thresholds, so the average is sum(count_e * (exit_id_e + 1)) / n_sample layers
    (the "average exit layer" the reference's bayesian_optimization.py:75-79 names as its budget).  This is what the calibration samples
    predict, not an on-policy promise: in a rollout the LSTM history comes from the exits actually taken, and VERDICT.md weak #11 records
    that the two differ on the synthetic episodes.  ``calibrate_on_policy`` solves from values logged in a rollout instead and reports
    this prediction beside the mix the next rollout measured (``measured_exit_mix``)."""
    counts = [int(c) for c in exit_counts]
    n_sample = sum(counts)
    if len(counts) > len(exit_id_list) or n_sample < 1:
        raise ValueError(f"{len(counts)} exit counts (sum {n_sample}) for the exits {list(exit_id_list)}")
    return [c / n_sample for c in counts], sum(c * (int(e) + 1) for c, e in zip(counts, exit_id_list)) / n_sample


def measured_exit_mix(taken, exit_id_list: Sequence[int]):
    """(fractions, average_exit_layer) MEASURED in a rollout: ``taken`` holds the exit layer of every logged step
    (``evaluate.on_policy_values``); ``predicted_exit_mix`` of its histogram over the exits."""
    bc = torch.bincount(torch.as_tensor(taken).detach().to("cpu", torch.int64), minlength=int(max(exit_id_list)) + 1)
    if int(bc.sum()) != sum(int(bc[int(e)]) for e in exit_id_list):
        raise ValueError(f"exit layers outside the exits {list(exit_id_list)} among the logged steps")
    return predicted_exit_mix([int(bc[int(e)]) for e in exit_id_list], exit_id_list)


class ActionValueNet:
    """value_net.py:72-160 (constructor surface).  ``exit_head`` is the model's ``extra_exit``."""

    def __init__(self, exit_list, exit_head, interval, window_size, threshold_type="L2"):
        self.exit_list = list(exit_list)
        self.exit_head = exit_head
        self.interval = interval
        self.window_size = window_size
        self.threshold_type = threshold_type
        self.action_list: list = []
        self.hidden_state = None          # attributes the harness resets (eval_utils.py:275-277)
        self.history_memory: list = []

    def reset_actions(self):
        """value_net.py:82-83.  The per-step action list lives on the device (control block: CTL_PREV_ACTION / CTL_PREV_REAL); the
        harness calls this after reading the ensemble of a step (eval_utils.py:460-461)."""
        self.action_list = []
        self._ensemble = None

    def get_ensemble_action(self):
        """value_net.py:92-95: mean over ``action_list[-2:]`` - the actions of the last two exit checks of the current step (the
        pseudo action the first check is compared with is not a member, value_net.py:120-130).  Computed by the exit check on the
        device (``head_final``: CTL_ENS_ACTION) and handed over by ``MPTFlamingo.forward`` with the step's verdict; returns
        (pose (1, 1, 6), gripper probability (1, 1, 1)) like the reference's head outputs."""
        ens = getattr(self, "_ensemble", None)
        if ens is None and self.action_list:       # slow path (the controller was CALLED, see forward): the reference's own formula
            actions, grippers = zip(*self.action_list[-2:])
            return torch.stack(actions, dim=0).mean(0), torch.stack(grippers, dim=0).mean(0)
        assert ens is not None and ens[2] > 0, "no exit check ran since the last reset_actions() (value_net.py:93)"
        return ens[0].view(1, 1, 6), torch.tensor([ens[1]], dtype=torch.float32).view(1, 1, 1)

    def _delta(self, a1: torch.Tensor, a2: torch.Tensor) -> torch.Tensor:
        """``get_delta`` (value_net.py:105-117)."""
        delta = torch.abs(a1 - a2)
        if self.threshold_type == "mean":
            return delta.mean(-1)
        if self.threshold_type == "L2":
            return delta.pow(2).mean(-1).pow(0.5)
        if self.threshold_type == "max":
            return delta.max(-1)[0]
        if self.threshold_type == "cosine":
            return 1 - torch.nn.functional.cosine_similarity(a1, a2, dim=-1, eps=1e-5)
        raise NotImplementedError(self.threshold_type)

    def forward(self, feats, i=None, mode="infer", rand_layer_feat=None):
        """``ActionValueNet.forward(mode='infer')`` (value_net.py:120-133) on the HOST: the slow path a caller takes when it invokes
        the controller like the reference's LLM loop does (mosaic_gpt_3b.py:438-439) instead of handing it to ``MPTFlamingo.forward``
        (where the same criterion runs on the device).  ``feats``: tuple of hidden states (1, T, d), ``exit_head``: the model's
        ``extra_exit`` handle - every call is one head evaluation on the engine + one synchronisation."""
        if mode != "infer":
            raise NotImplementedError("mode='generate' runs through generate_action_values / DeerEngine.generate_values")
        assert i > 0, "the first layer similarity is not implemented yet"
        if i - self.interval < 0:                   # no action before the first exit: pseudo action from the previous layer's feature
            prev_action = self.exit_head(feats[i - 1], update_hidden_state=False)
        else:
            prev_action = self.action_list[-1]
        action = self.exit_head(feats[i], update_hidden_state=False)
        self.action_list.append(action)
        self._ensemble = None
        return self._delta(action[0], prev_action[0])

    __call__ = forward


class ExitController:
    """value_net.py:163-297."""

    def __init__(self, value_net: Optional[ActionValueNet], exit_id_list: Sequence[int], steps_per_stage: int = 1,
                 exit_dist: str = "exp", leq: bool = True, max_layer: int = 12):
        self.value_net = value_net
        self.thresholds = None
        self.leq = leq
        self.exit_id_list = list(exit_id_list)
        self.num_exit = len(self.exit_id_list)
        self.steps_per_stage = steps_per_stage
        self.exit_dist = exit_dist
        self.max_layer = min(max_layer - 1, self.exit_id_list[-1])          # value_net.py:173
        self.cur_step = 0
        self.cur_exit_id = None
        self.module = self                                                     # DDP-style indirection (eval_utils.py:662)
        self._version = 0

    @property
    def real_num_exit(self) -> int:
        return len([x for x in self.exit_id_list if x <= self.max_layer])

    def _set_threshold_value(self, thresholds):
        assert len(thresholds) == self.real_num_exit
        self.thresholds = {self.exit_id_list[i]: float(thresholds[i]) for i in range(self.real_num_exit)}
        self._version += 1

    def set_threshold_from_values(self, values: torch.Tensor, exit_ratio: float, model_name: str = "mpt_dolly_3b", engine=None):
        """The ``values is not None`` branch of ``set_threshold`` (value_net.py:185-264).  engine: a ``DeerEngine``; with it and values on
        the device the solver runs there (``DeerEngine.solve_thresholds``) and only the thresholds come back."""
        if engine is not None and values.is_cuda:
            counts = exit_counts(values.shape[1], self.real_num_exit, exit_ratio, self.exit_dist, model_name)
            self._set_threshold_value(_solve_points(values, [counts], self.leq, engine)[0][0])
            return values
        T = solve_thresholds(values[: self.real_num_exit], self.real_num_exit, exit_ratio, self.exit_dist, self.leq, model_name)
        self.thresholds = {self.exit_id_list[i]: float(T[i]) for i in range(self.real_num_exit)}
        self._version += 1
        return values

    def set_threshold(self, args, model, dataloader, exit_ratio, model_name, values=None, fused=False):
        """value_net.py:185-264: deltas over the calibration loader (every rank its share, all-gathered), then the solver.
        fused=True: the calibration as one device pass per batch (``generate_action_values(fused=True)``)."""
        if values is None:
            from .distributed import all_gather_values
            pred, _ = generate_action_values(args, model, self.value_net, dataloader, device_id=None, fused=fused)
            values = all_gather_values(pred)
        return self.set_threshold_from_values(values, exit_ratio, model_name)

    def set_timestep(self, t):
        self.cur_step = t

    @torch.no_grad()
    def forward(self, x, i):
        """``ExitController.forward`` (value_net.py:277-297), the reference's protocol ``ctl(all_hidden_states, b_idx) -> bool`` as
        the LLM loop calls it (mosaic_gpt_3b.py:438-439).  Host-side slow path: ``MPTFlamingo.forward`` never comes here with a
        native controller (it configures the device-side gate instead); a foreign LLM loop, ``lang_encoder(...)`` called directly
        with this controller, and the tests do."""
        assert self.thresholds is not None, "Please set thresholds before calling forward"
        assert isinstance(i, int), f"the layer index must be an int, got {type(i).__name__}"
        if i not in self.exit_id_list:
            return False
        if self.cur_step % self.steps_per_stage != 0:            # still in a stage: reuse the previous exit id
            return i >= self.cur_exit_id
        if not isinstance(self.value_net, ActionValueNet):
            raise NotImplementedError
        value = self.value_net(x, i)
        if bool(value <= self.thresholds[i]) is self.leq or i >= self.max_layer:   # both true or both false
            self.cur_exit_id = i
            return True
        return False

    __call__ = forward

    def threshold_list(self) -> List[float]:
        return [self.thresholds[e] for e in self.exit_id_list[: self.real_num_exit]]

    def eval(self):
        return self

    def to(self, *a, **k):
        return self


def controllers_from_values(value_net: Optional[ActionValueNet], exit_id_list: Sequence[int], values: torch.Tensor,
                            exit_ratios: Sequence[float], max_layers=None, steps_per_stage: int = 1, exit_dist: str = "exp",
                            leq: bool = True, model_name: str = "mpt_dolly_3b", engine=None) -> List[ExitController]:
    """k operating points from ONE calibration: the ``values=`` branch of ``set_threshold`` (value_net.py:185-264) solved once per point
    on the same (n_exit, n_sample) value matrix.  max_layers: None (every exit reachable), one int for all points, or one per exit ratio
    (the reference's ``--max_layer``: DeeR-S vs DeeR-B).  Returns one ExitController per point, in order - a list that
    ``MPTFlamingo.step_env_batch`` / ``evaluate_policy_batched(operating_points=...)`` take.
    engine: a ``DeerEngine``; with it and values on the device (``generate_action_values(fused=True)``) the matrix stays there: the
    points that share a number of reachable exits are solved in one ``DeerEngine.solve_thresholds`` call and one read of k x n_exit
    thresholds (points with different max_layer: one call per group)."""
    ratios = [float(r) for r in exit_ratios]
    if max_layers is None or isinstance(max_layers, int):
        caps = [max_layers if max_layers is not None else list(exit_id_list)[-1] + 1] * len(ratios)
    else:
        caps = [int(m) for m in max_layers]
        if len(caps) != len(ratios):
            raise ValueError(f"{len(caps)} max_layer values for {len(ratios)} exit ratios (pass one per point)")
    out = []
    for r, cap in zip(ratios, caps):
        c = ExitController(value_net, exit_id_list, steps_per_stage=steps_per_stage, exit_dist=exit_dist, leq=leq, max_layer=cap)
        if engine is None or not values.is_cuda:
            c.set_threshold_from_values(values, r, model_name)
        out.append(c)
    if engine is not None and values.is_cuda:
        for n_exit in sorted({c.real_num_exit for c in out}):
            group = [i for i, c in enumerate(out) if c.real_num_exit == n_exit]
            counts = [exit_counts(values.shape[1], n_exit, ratios[i], exit_dist, model_name) for i in group]
            for i, row in zip(group, _solve_points(values, counts, leq, engine)[0]):
                out[i]._set_threshold_value(row)
    return out


def budget_ratio_grid(exit_dist: str, real_num_exit: int, grid: int, lo: Optional[float] = None, hi: Optional[float] = None) -> List[float]:
    """``grid`` exit ratios over [lo, hi], by default the range in which the distribution still changes: 'exp' (probs ~ r**k) geometric
    over [1/64, 64] - beyond, more than 98 % of the mass sits on the first / last exit; 'gauss' (mean exit index r, unit variance) linear
    over [-3, n_exit + 2]; 'gamma' (shape r, scale 2, at 1 .. n_exit) linear over [0.05, n_exit + 2] - from nearly its most front-loaded
    member (shape -> 0) to a mean 2 r well past the last exit."""
    if exit_dist not in ("exp", "gauss", "gamma"):
        raise ValueError("Unsupported exit distribution")
    d_lo, d_hi = {"exp": (1.0 / 64, 64.0), "gauss": (-3.0, real_num_exit + 2.0), "gamma": (0.05, real_num_exit + 2.0)}[exit_dist]
    lo, hi = float(d_lo if lo is None else lo), float(d_hi if hi is None else hi)
    if grid < 2 or lo == hi:
        return [lo]
    if exit_dist == "exp":
        return [lo * (hi / lo) ** (i / (grid - 1)) for i in range(grid)]
    return [lo + (hi - lo) * i / (grid - 1) for i in range(grid)]


def solve_for_budget(values: torch.Tensor, exit_id_list: Sequence[int], avg_exit_layer: float, max_layer: Optional[int] = None,
                     exit_dist: str = "exp", leq: bool = True, model_name: str = "mpt_dolly_3b", engine=None, grid: int = 64,
                     rounds: int = 2, value_net: Optional[ActionValueNet] = None, steps_per_stage: int = 1, trace: Optional[list] = None):
    """The operating point for a BUDGET instead of a guessed exit ratio: the exit ratio whose predicted average exit layer
    (``predicted_exit_mix``: layers per step on the calibration set, i.e. average LLM FLOPs) is the largest one not above
    ``avg_exit_layer``.  Round 1 solves a grid of ``grid`` ratios over the distribution's range (``budget_ratio_grid``) on the one value
    matrix and keeps the best point; every further round solves a grid between that point's two neighbours and keeps the better of the
    two (ties: the earlier one, then the smaller ratio).  With an engine and values on the device every round is one
    ``DeerEngine.solve_thresholds`` call and one small read - two of each for the default rounds = 2; engine=None runs the same search on
    the host solver, point by point.  The prediction is that of the calibration samples, see ``predicted_exit_mix``.
    Returns (ExitController with its thresholds set, the chosen exit ratio, (fractions, average_exit_layer)).  Raises ValueError naming
    the reachable range when even the smallest average of round 1 lies above the budget.  trace: a list that receives one
    (ratios, averages) pair per round."""
    cap = max_layer if max_layer is not None else list(exit_id_list)[-1] + 1
    ctl = ExitController(value_net, exit_id_list, steps_per_stage=steps_per_stage, exit_dist=exit_dist, leq=leq, max_layer=cap)
    n_exit, n_sample = ctl.real_num_exit, values.shape[1]
    ratios = budget_ratio_grid(exit_dist, n_exit, grid)
    best = None                                      # (average, ratio, thresholds, exit counts)
    for rnd in range(max(1, rounds)):
        counts = [exit_counts(n_sample, n_exit, r, exit_dist, model_name) for r in ratios]
        T, left = _solve_points(values, counts, leq, engine)
        avgs = [predicted_exit_mix(n, ctl.exit_id_list)[1] for n in left]
        if trace is not None:
            trace.append((list(ratios), avgs))
        ok = [i for i in range(len(ratios)) if avgs[i] <= avg_exit_layer]
        if rnd == 0 and not ok:
            raise ValueError(f"avg_exit_layer = {avg_exit_layer} is not reachable: '{exit_dist}' exit ratios {ratios[0]:.4g} .. {ratios[-1]:.4g} "
                             f"predict average exit layers {min(avgs):.4g} .. {max(avgs):.4g} on this calibration set")
        i = max(ok, key=lambda j: (avgs[j], -ratios[j])) if ok else None
        if i is not None and (best is None or avgs[i] > best[0]):
            best = (avgs[i], ratios[i], T[i], left[i])
            lo, hi = ratios[max(i - 1, 0)], ratios[min(i + 1, len(ratios) - 1)]
        elif rnd > 0:
            break                                    # nothing better between the neighbours: the same interval again would repeat this grid
        ratios = budget_ratio_grid(exit_dist, n_exit, grid, lo, hi)
    ctl._set_threshold_value(best[2])
    return ctl, best[1], predicted_exit_mix(best[3], ctl.exit_id_list)


def calibrate_on_policy(wrapper, envs, eval_sequences, annotations, task_checker, controller: ExitController, n_samples: int,
                        avg_exit_layer: float, rounds: int = 3, engine=None, ep_len: Optional[int] = None, exit_dist: Optional[str] = None,
                        model_name: str = "mpt_dolly_3b", grid: int = 64, measure_last: bool = True):
    """Thresholds for a budget from ON-POLICY values - the reference's second way to an operating point (bayesian_optimization.py, budget
    = average exit layer, :75-79) without its Gaussian process: every round collects ``n_samples`` exit values in a live rollout under
    the current thresholds (``evaluate.on_policy_values``: shadow steps, LSTM history from the exits actually taken) and solves the
    budget on that matrix (``solve_for_budget(values, ..., engine=engine)``: with an engine the logged matrix never leaves the GPU).
    Round 0 starts from ``controller`` (thresholds set; normally the demonstration-set one, ``set_threshold`` / ``solve_for_budget``).
    Returns (the last round's ExitController, records): one dict per round with ``thresholds``, ``exit_ratio``, ``predicted`` - the
    (fractions, average exit layer) the solver predicts on the round's matrix - ``collected`` - the mix measured while that matrix was
    collected, i.e. under the thresholds the round STARTED from - and ``measured`` - the mix measured from the exit layers taken under
    the round's own thresholds, i.e. the next round's ``collected`` (the last round's comes from one more collection; None with
    measure_last=False) - plus the round's ``values`` and ``taken`` and the ``measured_taken`` behind ``measured`` (device tensors).  Whether the rounds close the gap between
    predicted and measured is a property of the policy, not promised here."""
    from .evaluate import on_policy_values
    ctl = getattr(controller, "module", controller)
    records = []
    for rnd in range(max(1, int(rounds)) + (1 if measure_last else 0)):
        values, taken, mix = on_policy_values(wrapper, envs, eval_sequences, annotations, task_checker, ctl, n_samples, ep_len=ep_len)
        if records:
            records[-1]["measured"], records[-1]["measured_taken"] = mix, taken
        if rnd == max(1, int(rounds)):
            break
        ctl, ratio, predicted = solve_for_budget(values, ctl.exit_id_list, avg_exit_layer, max_layer=ctl.max_layer + 1,
                                                 exit_dist=exit_dist or ctl.exit_dist, leq=ctl.leq, model_name=model_name, engine=engine,
                                                 grid=grid, value_net=ctl.value_net, steps_per_stage=ctl.steps_per_stage)
        records.append(dict(round=rnd, thresholds=ctl.threshold_list(), exit_ratio=ratio, predicted=predicted, collected=mix, measured=None,
                            measured_taken=None, values=values, taken=taken))
    return ctl, records


def generate_action_values(args, model, value_net: ActionValueNet, calvin_loader, device_id=None, generator=None, fused=False):
    """value_net.py:301-397 on the native engine.  ``calvin_loader`` yields the reference's CALVIN batches:
    ``batch[0]`` images (bs, W, 3, S, S), ``batch[1]`` = (input_ids (bs, T), attention_mask (bs, T)), ``batch[3]`` gripper
    frames (bs, W, 3, S, S); W must equal ``value_net.window_size``.  For every window the trunk is run at full depth on each
    frame pair, the history fed to the head comes from a random exit layer per time step (flamingo_mpt.py:486-490,
    ``generator`` seeds the choice) and ``DeerEngine.generate_values`` evaluates the window-mode deltas.
    Returns (values (n_exit, n_windows * (W - W/2)), None) like the reference.
    fused=True: the same random layers (same generator calls), but every batch keeps only the pooled features of layer 0 and the exit
    layers (``DeerEngine.window_exit_features``) and the head side runs as one device pass (``DeerEngine.calibrate_values``, csrc/calib.hip);
    the values then stay on the device."""
    eng = model.module.engine
    exit_ids = list(value_net.exit_list)
    W = value_net.window_size
    out = []
    for batch in calvin_loader:
        images, (input_ids, attention_mask), gripper = batch[0], batch[1], batch[3]
        assert images.shape[1] == W, (images.shape, W)
        bs = images.shape[0]
        S = images.shape[-1]
        # the random exit layer of every (window, time step) - drawn window by window, like one flamingo_mpt.py:485-490 call per window
        rand_layers = torch.stack([torch.tensor([exit_ids[int(i)] for i in torch.randint(0, len(exit_ids), (W,), generator=generator)])
                                   for _ in range(bs)])
        # (bs, W) frames -> bs*W batch rows with the instruction repeated per frame (value_net.py:333-358)
        ids = input_ids.to(eng.dev).unsqueeze(1).expand(bs, W, input_ids.shape[-1]).reshape(bs * W, -1)
        mask = None
        if attention_mask is not None:
            mask = attention_mask.to(eng.dev).unsqueeze(1).expand(bs, W, attention_mask.shape[-1]).reshape(bs * W, -1)
        if fused:
            feats = eng.window_exit_features(images.reshape(bs * W, 3, S, S).to(eng.dev, eng.img_dtype),
                                             gripper.reshape(bs * W, 3, S, S).to(eng.dev, eng.img_dtype), ids, mask)
            out.append(eng.calibrate_values(feats.view(bs, W, *feats.shape[1:]), rand_layers, value_net.threshold_type))
            continue
        hid = eng.window_hidden_states(images.reshape(bs * W, 3, S, S).to(eng.dev, eng.img_dtype),
                                       gripper.reshape(bs * W, 3, S, S).to(eng.dev, eng.img_dtype), ids, mask)
        hid = hid.view(bs, W, *hid.shape[1:])
        out.append(eng.generate_values(hid, rand_layers, value_net.threshold_type))
    return torch.cat(out, dim=1), None
