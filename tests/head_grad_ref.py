"""The yardstick of the head-gradient tests (not a test file): the oracle's action head (oracle/deer_oracle.py, pinned to the reference by
the goldens) on a copy of a head's state dict with ``requires_grad``, the reference's loss expression (train_utils.py:519-540) on top,
gradients by autograd - in float64 (the yardstick) or float32 (the measure of what an f32 evaluation can reach).

``window_forward`` restates ``OracleHead.__call__``'s window branch from the oracle's own pieces (``lstm_cell``, ``_ln``, ``head_mlp``) so
that a test can break it on purpose: ``drop=(layer, t)`` detaches h_{t-1} where step t of that layer multiplies it with W_hh, i.e. the
gradient loses the recurrent term dh_{t-1} += dgates_t W_hh of exactly one step (a debug argument of this reference, not of the library).
tests/test_head_grad_oracle_cpu.py proves that the restatement equals ``OracleHead`` bit for bit and that autograd's gradient equals
central differences."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from deer_vla_amd import synthetic as syn
from oracle import deer_oracle as orc


def head_state(cfg, prefix="extra_exit.", seed=0, dtype=torch.float64):
    """a random head: Linear / LSTM weights N(0, 1 / fan_in), biases N(0, 0.1^2), LayerNorm weights 1 + N(0, 0.1^2); every value exactly
    representable in float32"""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for name, (shape, kind) in syn.head_param_shapes(cfg, prefix).items():
        if kind == syn.LINEAR:
            t = torch.randn(shape, generator=g) / shape[-1] ** 0.5
        elif kind == syn.LN_W:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = 0.1 * torch.randn(shape, generator=g)
        sd[name] = t.float().to(dtype)
    return sd


def window_forward(sd, cfg, prefix, X, drop=None):
    """X (N, L, d) pooled rows -> (pose (N, L, 6 A), logit (N, L, A)) from a zero state, dtype of X / sd"""
    x = _lstm_out(sd, cfg, prefix, X, drop)
    pose = orc.head_mlp(sd, cfg, prefix + "actions.", x, "tanh")
    _, logit = orc.head_mlp(sd, cfg, prefix + "gripper.", x, "sigmoid", True)
    return pose, logit


def _lstm_out(sd, cfg, prefix, X, drop=None):
    """the (LayerNorm-)LSTM of the head along the sequence from a zero state: (N, L, H)"""
    N, L, _ = X.shape
    Lh, H = cfg.lstm_num_layers, cfg.head_hidden
    h = [X.new_zeros(N, H) for _ in range(Lh)]
    c = [X.new_zeros(N, H) for _ in range(Lh)]
    outs = []
    for t in range(L):
        x = X[:, t]
        for l in range(Lh):
            r, sfx = (f"{prefix}rnn.layers.{3 * l}.", "_l0") if cfg.lstm_layernorm else (f"{prefix}rnn.", f"_l{l}")
            hp = h[l].detach() if drop == (l, t) else h[l]
            h[l], c[l] = orc.lstm_cell(x, hp, c[l], sd[r + "weight_ih" + sfx], sd[r + "weight_hh" + sfx], sd[r + "bias_ih" + sfx], sd[r + "bias_hh" + sfx])
            x = h[l]
            if cfg.lstm_layernorm:
                x = orc._ln(x, sd[f"{prefix}rnn.layers.{3 * l + 1}.weight"], sd[f"{prefix}rnn.layers.{3 * l + 1}.bias"])
        outs.append(x)
    return torch.stack(outs, dim=1)


def relu_margin(sd, cfg, prefix, X):
    """the smallest |input| any ReLU of the two MLP heads sees on X (fp64).  The gradient is discontinuous where such an input is 0: a case
    whose margin is below what an f32 forward can resolve has no gradient to compare against (the mask is decided by rounding)."""
    N, L, _ = X.shape
    with torch.no_grad():
        zero = {k: v.detach() for k, v in sd.items()}
        x = _lstm_out(zero, cfg, prefix, X)
        margin = float("inf")
        for head in ("actions.", "gripper."):
            p, y = prefix + head, x
            for i in range(cfg.mlp_num_hidden_layers):
                y = orc._lin(y, zero[f"{p}mlp.{1 + 4 * i}.weight"], zero[f"{p}mlp.{1 + 4 * i}.bias"])
                if cfg.mlp_layernorm:
                    y = orc._ln(y, zero[f"{p}mlp.{2 + 4 * i}.weight"], zero[f"{p}mlp.{2 + 4 * i}.bias"])
                margin = min(margin, float(y.abs().min()))
                y = F.relu(y)
    return margin


def reference_loss(pose, logit, label_pose, label_grip01, w_bin):
    """train_utils.py:519-540 for one head: mean over the rows of Huber(delta = 1).mean(-1) + w_bin BCE-with-logits.mean(-1)"""
    num = F.huber_loss(pose, label_pose, reduction="none").mean(-1)
    bin_ = F.binary_cross_entropy_with_logits(logit, label_grip01, reduction="none").mean(-1)
    return (num + bin_ * w_bin).mean()


def loss_and_grads(sd64, cfg, prefix, X, label_pose, label_grip01, w_bin, dtype=torch.float64, drop=None, scale=1.0):
    """(loss, {name: d (scale loss) / d tensor}) with every input cast to ``dtype`` first"""
    sd = OrderedDict((k, v.detach().to(dtype).requires_grad_(True)) for k, v in sd64.items())
    pose, logit = window_forward(sd, cfg, prefix, X.to(dtype), drop)
    N, L = X.shape[:2]
    loss = reference_loss(pose, logit, label_pose.to(dtype).reshape(N, L, -1), label_grip01.to(dtype).reshape(N, L, -1), w_bin)
    grads = torch.autograd.grad(loss * scale, list(sd.values()))
    return loss.detach(), OrderedDict(zip(sd.keys(), grads))


def planted_case(cfg, N, L, seed, dtype=torch.float64):
    """inputs and labels of one case: pooled rows X (N, L, d) and labels planted against the head's own outputs (computed by the caller's
    ``plant``) - see ``plant_labels``"""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(N, L, cfg.d_model, generator=g).float().to(dtype)


def plant_labels(pose, seed):
    """pose labels placed relative to the head's f64 outputs so that both Huber branches and |e| = 1 occur: errors cycle through
    0.25 (quadratic), 1.75 (linear, label outside [-1, 1] like an unnormalised demonstration), -1 and +1 up to rounding (the kink;
    torch's backward takes e there on the quadratic side and sign(e) on the other - both are +-1), the rest random in (-2, 2).
    Gripper targets alternate 0 / 1."""
    g = torch.Generator().manual_seed(2000 + seed)
    flat = pose.detach().double().reshape(-1)
    e = 4.0 * torch.rand(flat.shape, generator=g, dtype=torch.float64) - 2.0
    e[0::7] = 0.25
    e[1::7] = 1.75
    e[2::7] = -1.0
    e[3::7] = 1.0
    label = (flat - e).float().double().reshape(pose.shape)              # float32-representable labels
    n_grip = pose.shape[0] * pose.shape[1] * (pose.shape[2] // 6)
    grip = (torch.arange(n_grip) % 2).double().reshape(pose.shape[0], pose.shape[1], -1)
    return label, grip
