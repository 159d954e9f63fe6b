"""The entry points of csrc/exit_eval.hip one by one against float64 (the pooling of the all-exits pass is deer_calib_pool_layers, covered
by tests/test_calib_kernels.py).

 * deer_window_gather_layers: a pure copy - bit for bit against torch indexing; every slot hit, a layer without a slot and a layer index
   outside the table give NaN rows.
 * deer_exit_losses: Huber(delta = 1) / BCE-with-logits per (head, row) and the per-head mean, against float64 on the same f32 inputs, with
   planted pose errors on both Huber branches and exactly at |e| = 1, logits +-0, +-40, +-90 and targets 0 / 1.  Gates: a sequential f32
   sum of n terms is within n u sum|terms| of the exact sum (u = 2^-24); c more units cover what produces a term.  From the arithmetic,
   to first order in u: a Huber term is e = fl(|a - p|) (u), then 0.5 e e (2 u) or e - 0.5 (<= 3 u of the term, as e <= 2 (e - 0.5) for
   e >= 1), and the division by n (u): C_NUM = 4.  A BCE term is max(x, 0) - x y (exact for y in {0, 1}) + log1pf(expf(-|x|)) with both
   functions within 1 ulp = 2 u and log1p's condition number <= 1 (4 u), the sum (u) and the division (u): C_BIN = 6.  A term below the
   smallest normal f32 (exp(-90) = 8e-40, the planted logit 90 against target 1) has no relative precision in the format and may be
   flushed to zero: the gates allow 2^-126 of absolute error on top.  Every case prints
   its measured excess; DESIGN.md 5.5 records the worst.  loss[h] adds the row sum (n = R) on top of the per-row bound and the two
   roundings of num + w_bin bin."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from deer_vla_amd import _abi as abi  # noqa: E402

U = 2.0 ** -24
FLOOR = 2.0 ** -126           # f32 carries no relative precision below its smallest normal (a BCE term at logit 90 is exp(-90) = 8e-40)
C_NUM, C_BIN = 4.0, 6.0


def _stream():
    from deer_vla_amd.ops import _stream as s
    return s()


@pytest.mark.parametrize("bs", [1, 3])
@pytest.mark.parametrize("W", [2, 5])
def test_gather_is_a_bit_exact_copy_with_nan_rows_for_slotless_layers(bs, W):
    lib = abi.lib()
    import ctypes
    d, NL, n_layers, S = 256, 3, 6, 2
    slot_of = [-1, 0, -1, 1, -1, 2]
    g = torch.Generator().manual_seed(bs * 10 + W)
    P = torch.randn(bs * W, NL, d, generator=g).cuda()
    lay = torch.tensor([1, 3, 5])
    sel = lay[torch.randint(0, 3, (S, bs, W), generator=g)]
    sel[0].view(-1)[:min(3, bs * W)] = lay[:min(3, bs * W)]          # every slot
    sel[1, -1, -1] = 0                                              # a layer without a slot
    sel[1, 0, 0] = 77                                               # outside the table
    if bs * W > 2:
        sel[1, 0, 1] = -1
    X = torch.full((S, bs * W, d), 7.0, device="cuda")
    arr = (ctypes.c_int * n_layers)(*slot_of)
    rc = lib.deer_window_gather_layers(abi.ptr(P), abi.ptr(sel.to(torch.int32).cuda()), arr, n_layers, abi.ptr(X), S, bs, W, NL, d, _stream())
    assert rc == 0
    X = X.cpu()
    Pc = P.cpu()
    seen = set()
    for s in range(S):
        for r in range(bs * W):
            layer = int(sel[s].reshape(-1)[r])
            slot = slot_of[layer] if 0 <= layer < n_layers else -1
            if slot < 0:
                assert bool(torch.isnan(X[s, r]).all()), (s, r)
            else:
                seen.add(slot)
                assert torch.equal(X[s, r], Pc[r, slot]), (s, r)
    assert seen == {0, 1, 2} or bs * W < 3
    # bad arguments are refused before any launch
    assert lib.deer_window_gather_layers(abi.ptr(P), abi.ptr(sel.to(torch.int32).cuda()), arr, n_layers, abi.ptr(X.cuda()), S, bs, W, NL, 254, _stream()) != 0
    bad = (ctypes.c_int * n_layers)(0, 1, 2, 3, 4, 5)
    assert lib.deer_window_gather_layers(abi.ptr(P), abi.ptr(sel.to(torch.int32).cuda()), bad, n_layers, abi.ptr(X.cuda()), S, bs, W, NL, d, _stream()) != 0


def loss_case(A, R, Hn=3, seed=0):
    """actions (Hn, R, 8 A), pose labels (R, 6 A), gripper targets (R, A) with the planted values in the first rows of every head"""
    g = torch.Generator().manual_seed(seed + 100 * A + R)
    pose = (torch.randint(-8, 9, (R, 6 * A), generator=g).float() / 8)                       # multiples of 1/8: planted errors are exact
    act = torch.zeros(Hn, R, 8 * A)
    act[..., :6 * A] = pose[None] + 1.2 * torch.randn(Hn, R, 6 * A, generator=g)
    act[..., 7 * A:] = 6 * torch.randn(Hn, R, A, generator=g)
    grip = torch.randint(0, 2, (R, A), generator=g).float()
    errs = torch.tensor([0.0, 0.5, 1.0, -1.0, 1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20, 1.5, -3.0, 0.125, -0.875, 2.0, 1e-20])
    logits = torch.tensor([0.0, -0.0, 40.0, -40.0, 90.0, -90.0])
    for h in range(Hn):
        k = 0
        for r in range(R):
            for j in range(6 * A):
                act[h, r, j] = pose[r, j] + errs[(k + h) % len(errs)]
                k += 1
            if k >= 2 * len(errs):
                break
        k = 0
        for r in range(R):
            for j in range(A):
                act[h, r, 7 * A + j] = logits[(k // 2 + h) % len(logits)]
                if h == 0:
                    grip[r, j] = float(k % 2)                                                # each planted logit meets target 0 and target 1
                k += 1
            if k >= 2 * len(logits):
                break
    return act, pose, grip


def loss_reference(act, pose, grip, A, w_bin):
    """float64 on the same f32 inputs: per-element terms, per-row means, per-head mean"""
    a, p, y = act.double(), pose.double(), grip.double()
    e = (a[..., :6 * A] - p[None]).abs()
    hub = torch.where(e < 1, 0.5 * e * e, e - 0.5)
    x = a[..., 7 * A:]
    bce = x.clamp(min=0) - x * y[None] + torch.log1p(torch.exp(-x.abs()))
    return hub, bce, (hub.mean(-1) + w_bin * bce.mean(-1)).mean(-1)


def run_losses(act, pose, grip, A, w_bin):
    lib = abi.lib()
    Hn, R = act.shape[:2]
    a, p, y = act.cuda().contiguous(), pose.cuda().contiguous(), grip.cuda().contiguous()
    num, bin_, loss = torch.empty(Hn, R, device="cuda"), torch.empty(Hn, R, device="cuda"), torch.empty(Hn, device="cuda")
    assert lib.deer_exit_losses(abi.ptr(a), abi.ptr(p), abi.ptr(y), Hn, R, A, w_bin, abi.ptr(num), abi.ptr(bin_), abi.ptr(loss), _stream()) == 0
    return num.cpu(), bin_.cpu(), loss.cpu()


def excess_units(got, terms):
    """worst (|got - mean(terms)| / (u sum|terms| / n)) - n over the rows: the c a gate of the form (n + c) u sum|terms| needs"""
    n = terms.shape[-1]
    err = ((got.double() - terms.mean(-1)).abs() - FLOOR).clamp(min=0)
    scale = U * terms.abs().sum(-1) / n
    ok = scale > 0
    assert bool((err[~ok] == 0).all())
    return float((err[ok] / scale[ok]).max()) - n if bool(ok.any()) else -float(n)


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("R", [1, 7, 2049])
def test_exit_losses_match_float64_and_are_deterministic(A, R):
    w_bin = 0.01
    act, pose, grip = loss_case(A, R)
    hub, bce, ref_loss = loss_reference(act, pose, grip, A, w_bin)
    num, bin_, loss = run_losses(act, pose, grip, A, w_bin)
    c_num, c_bin = excess_units(num, hub), excess_units(bin_, bce)
    print(f"A={A} R={R}: excess over the n-term sum bound, in units of u sum|terms|: num {c_num:.2f}, bin {c_bin:.2f}")
    assert torch.isfinite(num).all() and torch.isfinite(bin_).all() and torch.isfinite(loss).all()
    assert c_num <= C_NUM, c_num
    assert c_bin <= C_BIN, c_bin
    rows = hub.mean(-1) + w_bin * bce.mean(-1)                                                # (Hn, R) float64, all >= 0
    bound = (R + 6 * A + max(C_NUM, C_BIN) + 3) * U * rows.abs().sum(-1) / R + FLOOR
    assert bool(((loss.double() - ref_loss).abs() <= bound).all()), ((loss.double() - ref_loss).abs(), bound)
    num2, bin2, loss2 = run_losses(act, pose, grip, A, w_bin)
    assert torch.equal(num, num2) and torch.equal(bin_, bin2) and torch.equal(loss, loss2)


def test_exit_losses_refuse_bad_arguments():
    lib = abi.lib()
    t = torch.zeros(64, device="cuda")
    for Hn, R, A in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 9)):
        assert lib.deer_exit_losses(abi.ptr(t), abi.ptr(t), abi.ptr(t), Hn, R, A, 0.01, abi.ptr(t), abi.ptr(t), abi.ptr(t), _stream()) != 0
    assert lib.deer_exit_losses(None, abi.ptr(t), abi.ptr(t), 1, 1, 1, 0.01, abi.ptr(t), abi.ptr(t), abi.ptr(t), _stream()) != 0
