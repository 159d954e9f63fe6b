"""Goldens of the all-exits window forward: the reference's own ``MPTFlamingo.forward`` in the branch it falls through to without
``exit_id`` / a dynamic controller ("output actions by all exits", flamingo_mpt.py:463-517) with ``multi_exit=True``, on this
repository's seeded tensors and stand-ins (make_golden.py's builders; the reference is imported from where it lies, see ref_import.py).

    python tests/golden/make_all_exits_golden.py

Writes all_exits.npz (A = 1), all_exits_ms2.npz (multi_step_action = 2) and all_exits_state.npz (use_state): bs = 2 windows of W = 4
steps, T = 6 tokens with one right-padded row.  ``torch.randint`` / ``random.randint`` are wrapped during the call, so the layer tables
the reference drew are stored next to the outputs of every head in ``all_outputs`` order (train_utils.py:503), the pooled features of
the exit layers (the heads' inputs; no hidden states) and the per-head Huber / BCE-with-logits losses of seeded labels computed with
torch.nn.functional (train_utils.py:519-540)."""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import MPTFlamingo, FlamingoLMMixin, extend_instance, seeded, syn  # noqa: E402

TORCH_SEED, PY_SEED, W_BIN = 4321, 4321, 0.01


def build(cfg, sd, multi_step_action, use_state):
    lm, _ = mg.build_ref_lang_encoder(cfg, sd)
    extend_instance(lm, FlamingoLMMixin)
    lm.set_decoder_layers_attr_name("transformer.blocks")
    venc = nn.Module()
    venc.visual = mg._OracleVisual(cfg, sd)
    torch.manual_seed(99)                                # heads this repository's inventory lacks (use_state variant) keep a seeded init
    model = MPTFlamingo(venc, lm, cfg.eoc_token_id, cfg.media_token_id, vis_dim=cfg.vit_width,
                        cross_attn_every_n_layers=cfg.cross_attn_every_n_layers, window_size=cfg.window_size, use_gripper=True,
                        fusion_mode="post", llm="mpt_dolly_3b", pooling="max", use_state=use_state, early_exit_layer=cfg.early_exit_layer,
                        multi_exit=True, layerwise_exit_eval=True, multi_step_action=multi_step_action, exit_interval=cfg.exit_interval,
                        mlp_layernorm=True, lstm_layernorm=True, mlp_num_hidden_layers=2, lstm_num_layers=4).eval()
    missing, unexpected = model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("vision_encoder.")}, strict=False)
    assert not unexpected, unexpected
    assert not any(k.startswith("extra_exit.") for k in missing), missing
    if not use_state:
        assert not any(k.startswith(("lm_exit_modules.", "lm_head.")) for k in missing), missing
    return model


def gen(name, multi_step_action=1, use_state=False):
    mg._dist_init()
    A = multi_step_action
    cfg = mg.llm_cfg(window_size=4, multi_step_action=A, use_state=use_state, layerwise_exit_eval=not use_state)
    seed = 11
    sd = syn.make_synthetic_state(cfg, seed, bf16_round=True)
    model = build(cfg, sd, A, use_state)
    W, bs, S, T = cfg.window_size, 2, cfg.image_size, 6
    lens = [6, 5]
    body = [[5, 17, 3], [9, 33]]
    ids = torch.full((bs, T), 96, dtype=torch.long)
    mask = torch.zeros(bs, T, dtype=torch.bool)
    for b in range(bs):
        row = [cfg.media_token_id] + body[b] + [cfg.eoc_token_id, 0]
        assert len(row) == lens[b]
        ids[b, :lens[b]] = torch.tensor(row)
        mask[b, :lens[b]] = True
    rgb = seeded("allx.rgb", (bs, W, 3, S, S))
    grip = seeded("allx.grip", (bs, W, 3, S, S))
    state = seeded("allx.state", (bs, W, 15))
    state[..., -1] = torch.tensor([[1.0, -1.0, 1.0, 1.0], [-1.0, -1.0, 1.0, -1.0]])
    labels = seeded("allx.labels", (bs, W, A, 7), scale=0.7)
    labels[..., 6] = torch.where(seeded("allx.gripcmd", (bs, W, A)) > 0, 1.0, -1.0)
    # the harness's reshaping (train_utils.py:470-478)
    images = rgb.unsqueeze(2).unsqueeze(2).flatten(0, 1)
    gripper = grip.unsqueeze(2).unsqueeze(2).flatten(0, 1)
    input_ids = ids.unsqueeze(1).repeat(1, W, 1).flatten(0, 1)
    attention_mask = mask.unsqueeze(1).repeat(1, W, 1).flatten(0, 1)
    state_tensor = state.unsqueeze(2).unsqueeze(2).flatten(0, 1) if use_state else None
    draws = []
    t_randint, p_randint = torch.randint, random.randint

    def rec_t(*a, **k):
        r = t_randint(*a, **k)
        draws.append(("torch", r.clone()))
        return r

    def rec_p(*a, **k):
        r = p_randint(*a, **k)
        draws.append(("random", r))
        return r
    torch.manual_seed(TORCH_SEED)
    random.seed(PY_SEED)
    torch.randint, random.randint = rec_t, rec_p
    try:
        final, exit_outputs, extra, extra2 = model(vision_x=images, lang_x=input_ids, attention_mask=attention_mask, vision_gripper=gripper,
                                                   state_tensor=state_tensor, with_gripper_logits=True, return_feature=False)
    finally:
        torch.randint, random.randint = t_randint, p_randint
    assert [k for k, _ in draws] == ["torch", "random", "torch"], [k for k, _ in draws]
    exit_ids = torch.tensor(model.get_all_exit_idx())
    idx1, prev_len, idx2 = draws[0][1], int(draws[1][1]), draws[2][1]
    rand_layers = exit_ids[idx1]
    two_layers = exit_ids[torch.cat([idx2[:, :1].expand(bs, prev_len), idx2[:, 1:].expand(bs, W - prev_len)], dim=1)]
    all_outputs = exit_outputs + [final.logits, extra, extra2]
    pose = torch.stack([o[0] for o in all_outputs])                  # (Hn, bs, W, 6 A)
    gprob = torch.stack([o[1][0] for o in all_outputs])              # (Hn, bs, W, A)
    glogit = torch.stack([o[1][1] for o in all_outputs])
    pooled = torch.stack([final.hidden_states[int(l)].amax(1) for l in exit_ids], dim=1)      # (bs W, NE, d): AdaptiveMaxPool1d over all T rows
    # train_utils.py:485,519-540 on the seeded labels
    lab = [labels[..., :6], (labels[..., 6:] + 1) // 2]
    num = torch.nn.functional.huber_loss(pose.reshape(-1, bs, W, A, 6), lab[0][None].expand(len(all_outputs), -1, -1, -1, -1),
                                         reduction="none").mean(-1)
    bins = torch.nn.functional.binary_cross_entropy_with_logits(glogit.reshape(-1, bs, W, A, 1), lab[1][None].expand(len(all_outputs), -1, -1, -1, -1),
                                                                reduction="none").mean(-1)
    loss = (num + bins * W_BIN).mean(dim=(1, 2, 3))
    print(f"  {name}: heads {len(all_outputs)}, rand {rand_layers.tolist()}, prev_len {prev_len}, two {two_layers.tolist()}, loss {loss.tolist()}")
    mg.save(name, cfg, seed, ids=ids, mask=mask, rgb=rgb, grip=grip, state=state, labels=labels if A > 1 else labels[:, :, 0],
            rand_layers=rand_layers, two_layers=two_layers, prev_len=np.asarray(prev_len), torch_seed=np.asarray(TORCH_SEED),
            py_seed=np.asarray(PY_SEED), n_exit_outputs=np.asarray(len(exit_outputs)), pose=pose, gprob=gprob, glogit=glogit, pooled=pooled,
            label_pose=lab[0].reshape(bs, W, 6 * A), label_grip01=lab[1].reshape(bs, W, A), num=num.mean(-1), bin=bins.mean(-1), loss=loss,
            w_bin=np.asarray(W_BIN), lens=np.asarray(lens), bf16_round=1)


if __name__ == "__main__":
    gen("all_exits.npz")
    gen("all_exits_ms2.npz", multi_step_action=2)
    gen("all_exits_state.npz", use_state=True)
