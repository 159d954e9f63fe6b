"""CPU-side checks of the head's window mode: the fake (meta) implementation of torch.ops.deer.action_head_sequence and the shape checks
of the reference-shaped handle, which reject a malformed call before any device is touched."""
import dataclasses
from types import SimpleNamespace

import pytest
import torch

from golden_util import load
from deer_vla_amd import ops
from deer_vla_amd.action_head import DeterministicDecoder


def _cfg(**kw):
    return dataclasses.replace(load("head_ln.npz")[0], **kw)


@pytest.fixture
def stub_model():
    """a model handle the fake implementation can resolve (it reads the shape description only)"""
    handle = 0x5EED0
    cfg = _cfg(multi_step_action=3)
    ops._MODELS[handle] = SimpleNamespace(cfg=cfg)
    yield handle, cfg
    ops._MODELS.pop(handle, None)


def test_action_head_sequence_fake_shapes(stub_model):
    handle, cfg = stub_model
    from torch._subclasses.fake_tensor import FakeTensorMode
    Lh, H = cfg.lstm_num_layers, cfg.head_hidden
    with FakeTensorMode():
        f = torch.empty(5, 7, 4, cfg.d_model, device="meta")
        a, h, c = torch.ops.deer.action_head_sequence(f, None, None, handle, 0, False)
        assert a.shape == (5, 7, 24) and h.shape == c.shape == (Lh, 5, H)
        h0 = torch.empty(Lh, 5, H, device="meta")
        a, h, c = torch.ops.deer.action_head_sequence(f, h0, h0, handle, 0, True)
        assert a.shape == (5, 1, 24) and a.dtype == torch.float32
        with pytest.raises(ValueError):
            torch.ops.deer.action_head_sequence(f, h0[:, :2], h0[:, :2], handle, 0, False)


def test_head_sequence_shape_checks():
    cfg = _cfg()
    assert ops.head_sequence_shapes(cfg, (2, 12, 7, cfg.d_model))[3:] == ((2, 12, 8), (cfg.lstm_num_layers, 2, cfg.head_hidden))
    with pytest.raises(ValueError):
        ops.head_sequence_shapes(cfg, (2, 12, 7, cfg.d_model + 1))
    with pytest.raises(ValueError):
        ops.head_sequence_shapes(cfg, (2, 12, 7, cfg.d_model), h0=torch.zeros(1))
    st = _cfg(use_state=True)
    with pytest.raises(ValueError):
        ops.head_sequence_shapes(st, (2, 12, 7, cfg.d_model))                       # state missing on a use_state head
    ops.head_sequence_shapes(st, (2, 12, 7, cfg.d_model), state=torch.zeros(24, 15))
    with pytest.raises(ValueError):
        ops.head_sequence_shapes(st, (2, 12, 7, cfg.d_model), state=torch.zeros(23, 15))


def test_handle_rejects_malformed_windows_before_the_device():
    cfg = _cfg()
    eng = SimpleNamespace(cfg=cfg, B=1, A=1)              # no device behind it: every check must fire before one is needed
    head = DeterministicDecoder(eng, window_size=12)
    with pytest.raises(ValueError, match="window_size 12"):
        head(torch.zeros(25, 7, cfg.d_model))               # bs * L not divisible by window_size
    with pytest.raises(ValueError):
        head(torch.zeros(2, 12, 7, cfg.d_model + 4))        # wrong feature width
    with pytest.raises(ValueError):
        head(torch.zeros(2, 12, 7, cfg.d_model), h_0=(torch.zeros(4, 3, 16), torch.zeros(4, 3, 16)))   # h_0 for another batch
    with pytest.raises(ValueError):
        DeterministicDecoder(SimpleNamespace(cfg=_cfg(use_state=True), B=1, A=1), 12)(torch.zeros(24, 7, cfg.d_model))
