"""deer_head_loss_grad (csrc/model.hip over csrc/head_grad.hip) against the fp64 yardstick of tests/head_grad_ref.py, one verdict per
parameter tensor.

Gate.  Per tensor e_dev = max|g_dev - g64| / max|g64| must stay below K * e32 + 16 * 2^-24, where e32 is the same quantity for the ORACLE
evaluated in float32 on the CPU on the same case, in the same test: both are f32 evaluations of the same expression that differ in
summation order and in the expf / tanhf implementation, which is what the factor K is for.  Nothing in the gate comes from the device's
own result.  Every case's inputs keep the ReLU inputs away from 0 (RELU_MARGIN: the gradient is discontinuous there); the Huber kink
|e| = 1 IS planted, both of its sides having the same derivative.  A tensor whose exact gradient is zero (W_hh at L = 1: h_{-1} = 0) must come back as exact zeros.

Measured on an MI355X, worst e_dev / e32 per tensor family over all cases below: 2.4 .. 4.4, gripper Linear biases 8.7 (inside the
floor: e_dev 2.1e-7) - DESIGN.md 5.5b.  Ratios exceed 2, so K stays 8."""
import ctypes
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

import head_grad_ref as ref  # noqa: E402
from deer_vla_amd import _abi as abi  # noqa: E402
from deer_vla_amd.config import deer_tiny  # noqa: E402
from deer_vla_amd.engine import config_to_c  # noqa: E402
from deer_vla_amd.ops import head_param_table  # noqa: E402

K = 8
FLOOR = 16 * 2.0 ** -24
W_BIN = 0.01
PREFIX = "extra_exit."
RELU_MARGIN = 1e-5                       # ~60 x the error of an f32 forward on the O(1) LayerNorm outputs that feed the ReLUs
GUARD = 256                              # NaN floats on either side of the gradient buffer

_handles = {}
_cases = {}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cfg(A, lstm_ln, mlp_ln, n_hidden):
    return deer_tiny(multi_step_action=A, lstm_layernorm=lstm_ln, mlp_layernorm=mlp_ln, mlp_num_hidden_layers=n_hidden)


def _handle(key):
    """a deer_model per head shape: host object only (no arena, no workspace - the gradient call needs neither)"""
    if key not in _handles:
        h = ctypes.c_void_p()
        cc = config_to_c(_cfg(*key), 1, 32)
        abi.check(abi.lib().deer_model_create(ctypes.byref(cc), ctypes.byref(h)), "deer_model_create")
        _handles[key] = h
    return _handles[key]


def _case(key, N, L, mode="normal", seed=0):
    """(cfg, sd64, X, label_pose, label_grip, g64, g32, loss64), computed once per case and shared READ-ONLY.  mode: the gripper's output
    layer - "normal"; "zero": weights x 1e-3, bias 0 (logits near +-0); "sat": bias +40 / -40 alternating over the rows' outputs, or by
    seed parity for A = 1 (logits near +-40)."""
    ck = (key, N, L, mode, seed)
    if ck in _cases:
        return _cases[ck]
    cfg = _cfg(*key)
    # the first seed whose inputs keep every ReLU input RELU_MARGIN away from 0 in fp64: at the kink the gradient jumps, and an input within
    # an f32 forward's error of it (seed 0 of (A = 1, N = 3, L >= 2): -3.4e-9 in fp64, +1.5e-7 in float32) has its mask decided by rounding
    while ref.relu_margin(ref.head_state(cfg, PREFIX, seed), cfg, PREFIX, ref.planted_case(cfg, N, L, seed)) < RELU_MARGIN:
        seed += 1
    sd = ref.head_state(cfg, PREFIX, seed)
    wn, bn = [k for k in sd if k.startswith(PREFIX + "gripper.mlp.")][-2:]
    if mode == "zero":
        sd[wn] = (sd[wn] * 1e-3).float().double()
        sd[bn] = torch.zeros_like(sd[bn])
    elif mode in ("sat", "sat-"):
        sign = 1.0 if mode == "sat" else -1.0
        sd[bn] = torch.tensor([sign * 40.0 * (-1.0) ** i for i in range(sd[bn].numel())], dtype=torch.float64)
    X = ref.planted_case(cfg, N, L, seed)
    with torch.no_grad():
        pose, logit = ref.window_forward(sd, cfg, PREFIX, X)
    label, grip = ref.plant_labels(pose, seed)
    loss64, g64 = ref.loss_and_grads(sd, cfg, PREFIX, X, label, grip, W_BIN)
    _, g32 = ref.loss_and_grads(sd, cfg, PREFIX, X, label, grip, W_BIN, dtype=torch.float32)
    _cases[ck] = (cfg, sd, X, label, grip, g64, g32, float(loss64), logit)
    return _cases[ck]


def _flat(handle, sd, fill=0.0):
    tab, total = head_param_table(abi.lib(), handle, 0)
    buf = torch.full((total,), fill, dtype=torch.float32)
    for name, off, numel, _ in tab:
        buf[off:off + numel] = sd[name].reshape(-1).float()
    return tab, total, buf.cuda()


def _device(handle, sd, X, label, grip, scale=1.0, accumulate=False, grad=None):
    """one deer_head_loss_grad call.  The gradient buffer sits between NaN guards and starts as NaN itself (accumulate = 0 stores every
    entry and must leave the padding between the tensors alone).  Returns ({name: grad f64 on the CPU}, loss, raw guarded buffer)."""
    lib = abi.lib()
    tab, total, params = _flat(handle, sd)
    if grad is None:
        grad = torch.full((total + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    loss = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    N, L = X.shape[:2]
    Xd, pd, gd = X.float().cuda().contiguous(), label.float().cuda().contiguous(), grip.float().cuda().contiguous()
    abi.check(lib.deer_head_loss_grad(handle, 0, abi.ptr(params), abi.ptr(Xd), N, L, abi.ptr(pd), abi.ptr(gd), W_BIN, scale, abi.ptr(grad, 4 * GUARD),
                                      1 if accumulate else 0, abi.ptr(loss, 4), _stream()), "deer_head_loss_grad")
    torch.cuda.synchronize()
    g = grad.cpu()
    assert torch.isnan(g[:GUARD]).all() and torch.isnan(g[GUARD + total:]).all(), "guard around grad overwritten"
    lo = loss.cpu()
    assert torch.isnan(lo[0]) and torch.isnan(lo[2]) and torch.isfinite(lo[1])
    body = g[GUARD:GUARD + total]
    covered = torch.zeros(total, dtype=torch.bool)
    out = OrderedDict()
    for name, off, numel, _ in tab:
        covered[off:off + numel] = True
        out[name] = body[off:off + numel].double().reshape(sd[name].shape)
        assert torch.isfinite(out[name]).all(), name
    return out, float(lo[1]), grad, covered


def _family(name):
    n = name[len(PREFIX):]
    if n.startswith("rnn"):
        if "weight_ih" in n or "weight_hh" in n or "bias_" in n:
            return "lstm." + n.split(".")[-1].rsplit("_l", 1)[0]
        return "lstm.ln"
    head, _, idx, kind = n.split(".")
    return f"{head}.{'ln' if int(idx) % 4 == 2 else 'linear'}.{kind}"


def _errors(g, g64):
    return {k: (float((g[k].double() - g64[k]).abs().max()) / float(g64[k].abs().max()) if float(g64[k].abs().max()) > 0 else
                (0.0 if float(g[k].abs().max()) == 0 else float("inf"))) for k in g64}


def _verdict(g_dev, g64, g32, k=K):
    """per tensor: (name, e_dev, e32, passes)"""
    e_dev, e32 = _errors(g_dev, g64), _errors(g32, g64)
    return [(n, e_dev[n], e32[n], e_dev[n] <= k * e32[n] + FLOOR) for n in g64]


def _report(tag, verdict):
    fam = {}
    for n, ed, e3, _ in verdict:
        r = ed / e3 if e3 > 0 else (0.0 if ed == 0 else float("inf"))
        f = _family(n)
        if f not in fam or r > fam[f][0]:
            fam[f] = (r, ed, e3)
    print(f"{tag}: e_dev / e32 per family: " + ", ".join(f"{f} {r:.2f} ({ed:.1e}/{e3:.1e})" for f, (r, ed, e3) in sorted(fam.items())))
    return fam


BASE = (1, True, True, 2)
SHAPES = [(N, L) for N in (1, 3) for L in (1, 2, 4)]
CASES = [((A, True, True, 2), N, L, "normal") for A in (1, 2) for (N, L) in SHAPES]
CASES += [((A, lln, mln, nh), N, L, "normal") for lln in (True, False) for mln in (True, False) for nh in (2, 3)
          for (A, N, L) in ((2, 3, 4), (1, 1, 2)) if (lln, mln, nh) != (True, True, 2)]
CASES += [((2, True, True, 2), 3, 4, "zero"), ((2, True, True, 2), 3, 4, "sat"), ((1, True, True, 2), 3, 4, "sat"), ((1, True, True, 2), 3, 4, "sat-")]


@pytest.mark.parametrize("key,N,L,mode", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gradient_matches_fp64_oracle_per_tensor(key, N, L, mode):
    cfg, sd, X, label, grip, g64, g32, loss64, logit = _case(key, N, L, mode)
    A = max(1, cfg.multi_step_action)
    # the planted inputs are what the case says they are
    with torch.no_grad():
        pose, _ = ref.window_forward(sd, cfg, PREFIX, X)
    e = (pose - label).abs().reshape(-1)
    if e.numel() >= 7:
        assert (e < 0.5).any() and (e > 1.5).any() and ((e - 1).abs() < 1e-6).any()
    if mode == "zero":
        assert float(logit.abs().max()) < 0.05 and (logit > 0).any() and (logit < 0).any()
    if mode.startswith("sat"):
        assert float(logit.abs().min()) > 30 and (A == 1 or ((logit > 0).any() and (logit < 0).any()))
    g, loss, _, _ = _device(_handle(key), sd, X, label, grip)
    # the loss is 1-Lipschitz in the head's outputs: the fp32 head-only gate of tests/test_all_exits.py (HEAD_TOL, 2e-5) bounds it
    assert abs(loss - loss64) <= 2e-5 * max(1.0, abs(loss64)), (loss, loss64)
    verdict = _verdict(g, g64, g32)
    _report(f"{key} N={N} L={L} {mode}", verdict)
    bad = [(n, f"{ed:.2e}", f"{e3:.2e}") for n, ed, e3, ok in verdict if not ok]
    assert not bad, bad
    if L == 1:                                   # no recurrence: d W_hh is exactly zero
        assert all(float(g[n].abs().max()) == 0 for n in g if "weight_hh" in n)
    # two runs are bit-identical
    g2, loss2, _, _ = _device(_handle(key), sd, X, label, grip)
    assert loss2 == loss and all(torch.equal(g[n], g2[n]) for n in g)


def test_gate_rejects_a_gradient_without_one_recurrent_term():
    """the gate can fail: the yardstick's own gradient with dh_{t-1} += dgates_t W_hh dropped at ONE step of ONE layer (L = 4) is
    rejected, for every (layer, step) that has a recurrent term"""
    key = (2, True, True, 2)
    cfg, sd, X, label, grip, g64, g32, _, _ = _case(key, 3, 4)
    for drop in ((0, 1), (1, 2), (3, 3), (2, 1)):
        _, gd = ref.loss_and_grads(sd, cfg, PREFIX, X, label, grip, W_BIN, drop=drop)
        verdict = _verdict(gd, g64, g32, k=8)                                # even at the starting K
        assert any(not ok for _, _, _, ok in verdict), drop


def test_accumulate_over_two_chunks_equals_one_call():
    """N = 3 windows as chunks of 2 + 1 with scale = rows / all rows and accumulate = 1 on the second: the same gate against the fp64
    gradient of the whole batch.  Not bitwise: a chunk's rows are scaled by its share before the row sums, and the sums of two chunks
    are added instead of running through one chain; the difference to the one-call result is printed."""
    key = (2, True, True, 2)
    cfg, sd, X, label, grip, g64, g32, loss64, _ = _case(key, 3, 4)
    h = _handle(key)
    one, loss_one, _, _ = _device(h, sd, X, label, grip)
    _, l1, buf, covered = _device(h, sd, X[:2], label[:2], grip[:2], scale=2 / 3)
    two, l2, buf, _ = _device(h, sd, X[2:], label[2:], grip[2:], scale=1 / 3, accumulate=True, grad=buf)
    body = buf.cpu()[GUARD:GUARD + covered.numel()]
    assert torch.isnan(body[~covered]).all() and torch.isfinite(body[covered]).all()       # the padding between the tensors is never written
    assert abs((2 * l1 + l2) / 3 - loss_one) <= 8 * 2.0 ** -24 * max(1.0, abs(loss_one))
    verdict = _verdict(two, g64, g32)
    _report("accumulate 2 + 1", verdict)
    assert all(ok for _, _, _, ok in verdict), [v for v in verdict if not v[3]]
    print("one call vs 2 + 1 chunks, max |d| / max |g64|: %.2e" % max(float((one[n] - two[n]).abs().max()) / float(g64[n].abs().max()) for n in one))


def test_taped_step_keeps_its_tape_inside_its_rows():
    """deer_head_grad_lstm_step on caller-owned tape buffers with NaN between the rows (pitch > row) and around them: gates, c_t and h_t
    land in their rows, every guard stays NaN, and the values are those of the oracle's lstm_cell expression in fp64"""
    lib = abi.lib()
    N, H, L = 3, 128, 2
    g = torch.Generator().manual_seed(3)
    w_hh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).float()
    b_hh = (0.1 * torch.randn(4 * H, generator=g)).float()
    pre = torch.randn(N, 4 * H, generator=g).float()
    h_prev, c_prev = torch.tanh(torch.randn(N, H, generator=g)).float(), torch.randn(N, H, generator=g).float()
    ld_g, ld_s = L * 4 * H, L * H

    def guarded(rows, ld, width, src=None):
        t = torch.full((GUARD + rows * ld + GUARD,), float("nan"), dtype=torch.float32)
        v = t[GUARD:GUARD + rows * ld].view(rows, ld)
        if src is not None:
            v[:, :width] = src
        return t.cuda()
    G = guarded(N, ld_g, 4 * H, pre)
    C, Y = guarded(N, ld_s, H), guarded(N, ld_s, H)
    hp, cp = guarded(N, ld_s, H, h_prev), guarded(N, ld_s, H, c_prev)
    wd, bd = w_hh.cuda(), b_hh.cuda()                     # kept alive until the launch has run
    abi.check(lib.deer_head_grad_lstm_step(abi.ptr(G, 4 * GUARD), ld_g, abi.ptr(hp, 4 * GUARD), ld_s, abi.ptr(wd), abi.ptr(bd),
                                           abi.ptr(cp, 4 * GUARD), abi.ptr(C, 4 * GUARD), ld_s, abi.ptr(Y, 4 * GUARD), ld_s, N, H, _stream()),
              "deer_head_grad_lstm_step")
    torch.cuda.synchronize()
    # orc.lstm_cell's arithmetic with x W_ih^T + b_ih = pre
    gates = pre.double() + h_prev.double() @ w_hh.double().T + b_hh.double()
    i, f, gg, o = gates.chunk(4, dim=-1)
    want_g = torch.cat([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)], dim=-1)
    c2 = torch.sigmoid(f) * c_prev.double() + torch.sigmoid(i) * torch.tanh(gg)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    for buf, ld, width, want in ((G, ld_g, 4 * H, want_g), (C, ld_s, H, c2), (Y, ld_s, H, h2)):
        t = buf.cpu()
        assert torch.isnan(t[:GUARD]).all() and torch.isnan(t[-GUARD:]).all()
        v = t[GUARD:-GUARD].view(N, ld)
        assert torch.isnan(v[:, width:]).all()
        assert float((v[:, :width].double() - want).abs().max()) < 64 * 2.0 ** -24
