"""The yardstick of the head-gradient tests, proven without a GPU (tests/head_grad_ref.py): its window forward equals ``OracleHead`` bit
for bit, autograd's gradient of the reference loss equals central differences in float64 (LayerNorm-LSTM and plain LSTM), and the
spine's parameter table (``deer_head_param_entry``) equals the state-dict names / shapes of the synthetic weights."""
import ctypes
import math

import pytest
import torch

import head_grad_ref as ref
from deer_vla_amd import _abi as abi
from deer_vla_amd.config import deer_tiny
from deer_vla_amd.engine import config_to_c
from deer_vla_amd.ops import head_param_table
from deer_vla_amd.synthetic import LN_B, LN_W, param_shapes
from oracle import deer_oracle as orc

W_BIN = 0.01


def _case(cfg, N=2, L=3, seed=0):
    sd = ref.head_state(cfg, "extra_exit.", seed)
    X = ref.planted_case(cfg, N, L, seed)
    with torch.no_grad():
        pose, _ = ref.window_forward(sd, cfg, "extra_exit.", X)
    label, grip = ref.plant_labels(pose, seed)
    return sd, X, label, grip


@pytest.mark.parametrize("lstm_layernorm", [True, False])
def test_window_forward_is_the_oracle_head(lstm_layernorm):
    cfg = deer_tiny(lstm_layernorm=lstm_layernorm, mlp_layernorm=lstm_layernorm)
    sd, X, _, _ = _case(cfg)
    N, L, d = X.shape
    head = orc.OracleHead(sd, cfg, "extra_exit.")
    z = torch.zeros(cfg.lstm_num_layers, N, cfg.head_hidden, dtype=torch.float64)
    pose_o, (_, logit_o) = head(X.reshape(N, L, 1, d), h_0=(z, z.clone()), with_gripper_logits=True)
    pose, logit = ref.window_forward(sd, cfg, "extra_exit.", X)
    assert torch.equal(pose, pose_o) and torch.equal(logit, logit_o)


@pytest.mark.parametrize("lstm_layernorm", [True, False])
def test_autograd_gradient_equals_central_differences(lstm_layernorm):
    """fp64, tiny head (H = 128), N = 2, L = 3: per tensor, the directional derivative along a random unit direction and eight single entries
    (step 1e-6: truncation ~1e-12, rounding of the O(1) loss ~1e-10; gate 1e-5 of the tensor's largest gradient entry).
    The labels keep |e| away from the Huber kink here (a finite difference straddling it measures the kink, not the gradient)."""
    cfg = deer_tiny(lstm_layernorm=lstm_layernorm, mlp_layernorm=lstm_layernorm)
    sd, X, label, grip = _case(cfg)
    with torch.no_grad():
        pose, _ = ref.window_forward(sd, cfg, "extra_exit.", X)
    e = pose - label
    label = torch.where((e.abs() - 1).abs() < 1e-3, label + 0.3, label)
    _, grads = ref.loss_and_grads(sd, cfg, "extra_exit.", X, label, grip, W_BIN)

    def loss_of(sd2):
        with torch.no_grad():
            p, lg = ref.window_forward(sd2, cfg, "extra_exit.", X)
            return float(ref.reference_loss(p, lg, label, grip, W_BIN))

    g = torch.Generator().manual_seed(5)
    eps = 1e-6
    for name, t in sd.items():
        direction = torch.randn(t.shape, generator=g, dtype=torch.float64)
        probes = [direction / direction.norm()]                # unit steps: a long step crosses ReLU kinks and measures those
        flat = torch.randperm(t.numel(), generator=g)[:8]
        for i in flat:
            one = torch.zeros(t.numel(), dtype=torch.float64)
            one[i] = 1.0
            probes.append(one.reshape(t.shape))
        scale = float(grads[name].abs().max()) + 1e-30
        for v in probes:
            plus, minus = dict(sd), dict(sd)
            plus[name], minus[name] = t + eps * v, t - eps * v
            fd = (loss_of(plus) - loss_of(minus)) / (2 * eps)
            an = float((grads[name] * v).sum())
            assert abs(fd - an) <= 1e-5 * max(abs(an), scale) + 1e-9, (name, fd, an)


def test_dropping_one_recurrent_term_changes_the_gradient():
    cfg = deer_tiny()
    sd, X, label, grip = _case(cfg, N=3, L=4)
    _, g = ref.loss_and_grads(sd, cfg, "extra_exit.", X, label, grip, W_BIN)
    _, gd = ref.loss_and_grads(sd, cfg, "extra_exit.", X, label, grip, W_BIN, drop=(1, 2))
    k = "extra_exit.rnn.layers.3.weight_hh_l0"
    assert float((g[k] - gd[k]).abs().max()) > 1e-3 * float(g[k].abs().max())


@pytest.mark.parametrize("kw", [dict(), dict(lstm_layernorm=False, mlp_layernorm=False), dict(layerwise_exit_eval=True),
                                dict(multi_step_action=2, mlp_num_hidden_layers=3)])
def test_spine_parameter_table_is_the_state_dict(kw):
    """extra_exit, lm_head and lm_exit_modules.j: names, order and sizes of deer_vla_amd.synthetic.param_shapes; offsets ascending,
    64-float aligned, no overlap; decays = weights of Linear / LSTM only"""
    cfg = deer_tiny(**kw)
    lib = abi.build() and abi.lib()
    h = ctypes.c_void_p()
    cc = config_to_c(cfg, 1, 32)
    assert lib.deer_model_create(ctypes.byref(cc), ctypes.byref(h)) == 0
    try:
        ps = param_shapes(cfg)
        prefixes = ["extra_exit."] + ([p for p, _ in cfg.layerwise_heads()] if cfg.layerwise_exit_eval else [])
        if cfg.layerwise_exit_eval:
            assert prefixes[-1] == "lm_head." and prefixes[1] == "lm_exit_modules.0."
        for head, prefix in enumerate(prefixes):
            tab, total = head_param_table(lib, h, head)
            want = [(k, v) for k, v in ps.items() if k.startswith(prefix)]
            assert [t[0] for t in tab] == [k for k, _ in want]
            end = 0
            for (name, off, numel, decays), (_, (shape, kind)) in zip(tab, want):
                assert numel == math.prod(shape) and off >= end and off % 64 == 0
                end = off + numel
                assert decays == (len(shape) == 2) and (decays or "bias" in name or kind in (LN_W, LN_B))
            assert end <= total and total % 64 == 0
        assert lib.deer_head_param_count(h, len(prefixes)) == -1 and lib.deer_head_param_count(h, -1) == -1
    finally:
        lib.deer_model_destroy(h)
