"""The graph pieces of the segmented schedules come from the spine (include/deer_model.h deer_step_piece) and are the one-shot step
(deer_step_enqueue) cut into parts: the same launches in the same order with bit-identical results, for the dynamic plan and for a static
exit; the stored dynamic plan follows the three calls that change it; a piece the plan does not have is refused before anything is
launched."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from deer_vla_amd import _abi as abi  # noqa: E402
from deer_vla_amd import synthetic as syn  # noqa: E402
from deer_vla_amd.config import deer_tiny  # noqa: E402
from deer_vla_amd.engine import DeerEngine, _cur_stream  # noqa: E402

ERR_SHAPE = 1                                     # include/deer_hip.h DEER_ERR_SHAPE


@pytest.fixture(scope="module")
def owner():
    """one copy of the tiny model's weights (exits 1, 3, 5 of 6 layers); the env batches of the cases are siblings over it"""
    cfg = deer_tiny()
    return DeerEngine(cfg, syn.make_synthetic_state(cfg, 1, bf16_round=True))


def read_plan(eng):
    n = eng.cfg.n_layers
    a, b, c = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int * n)()
    k = eng.lib.deer_dynamic_plan(eng._h, a, b, c, n)
    return [(a[i], b[i], c[i]) for i in range(k)]


def load(eng, T):
    """seeded frames and a T-token instruction per environment; an env batch gets one right-padded instruction (the padding-mask rule)"""
    per = [syn.synthetic_step_inputs(eng.cfg, 0, rank=b, text_len=T, text_seed=7 + b) for b in range(eng.B)]
    rgb, grip = (torch.stack([p[k].reshape(3, eng.cfg.image_size, -1) for p in per]).to(eng.dev, eng.img_dtype) for k in (0, 1))
    ids = torch.cat([p[2] for p in per]).to(eng.dev)
    mask = None
    if eng.B > 1:
        mask = torch.ones(eng.B, T, dtype=torch.bool, device=eng.dev)
        mask[1, T - 1] = False
    return eng.load_inputs(rgb, grip, ids, mask)


def run(eng, T, use_mask, enqueue, layers):
    """From the episode start and cleared result buffers: `enqueue` under the in-situ profiler -> (kernel classes, results)"""
    eng.reset()
    for t in (eng.hidden, eng.h_tmp, eng.c_tmp, eng.action_dbg):
        t.zero_()
    eng.hold_dev.copy_(torch.tensor([0, 1, 0, 0], dtype=torch.int32))      # {hold mask, sequence number, no host mirror}
    eng.prof_begin()
    enqueue()
    names = [r[0] for r in eng.prof_end()]
    rows = eng.B * T
    out = {n: getattr(eng, n).clone() for n in ("ctl", "action_dbg", "h_tmp", "c_tmp", "h_state", "c_state")}
    out["hidden"] = eng.hidden[layers, :rows].clone()
    return names, out


def piece(eng, which, index, T, use_mask):
    return eng.lib.deer_step_piece(eng._h, which, index, T, 1 if use_mask else 0, _cur_stream())


def begin_and_vision(eng):
    abi.check(eng.lib.deer_begin_step(eng._h, None, _cur_stream()), "deer_begin_step")
    eng.enqueue_vision("all", chain=-1, kv_all=False)


# one environment of <= 16 rows (the twelve-launch layer); an env batch of 15 rows without compaction; an env batch of 56 rows with
# compaction, every environment leaving at another exit, so that rows are really gathered and both row maps are in use
@pytest.mark.parametrize("B,T,compaction", [(1, 5, False), (3, 5, False), (4, 14, True)])
def test_pieces_are_the_one_shot_step_launch_for_launch(owner, B, T, compaction):
    eng = owner.sibling(B)
    real = eng.real_num_exit
    if B > 1:
        eng.set_compaction(compaction)
    if compaction:      # environment b never passes a check before exit min(b, last) and always passes that one
        eng.set_env_exit([[-1.0] * min(b, real - 1) + [1e8] * (real - min(b, real - 1)) for b in range(B)], [eng.exit_ids[-1]] * B)
    else:
        eng.set_thresholds([-1.0] * (real - 1) + [1e5])
    T_, use_mask = load(eng, T)
    assert T_ == T and use_mask == (B > 1)
    plan = eng.dynamic_plan()
    fin = [i for i, need_pseudo, is_exit, _ in plan if need_pseudo or is_exit]

    def pieces():
        begin_and_vision(eng)
        for i, need_pseudo, is_exit, _ in plan:
            abi.check(piece(eng, abi.PIECE_MAIN, i, T, use_mask), "MAIN")
            if need_pseudo or is_exit:
                abi.check(piece(eng, abi.PIECE_HEADS, i, T, use_mask), "HEADS")

    names1, out1 = run(eng, T, use_mask, lambda: eng._enqueue_step(T, use_mask, None), fin)
    names2, out2 = run(eng, T, use_mask, pieces, fin)
    assert len(names1) > 50 and names1 == names2
    for k in out1:
        assert torch.equal(out1[k], out2[k]), k
    exits = eng.ctl.view(B, abi.CTL_WORDS)[:, abi.CTL_EXIT_LAYER].tolist()
    assert exits == ([eng.exit_ids[min(b, real - 1)] for b in range(B)] if compaction else [eng.exit_ids[-1]] * B)

    static = list(range(eng.exit_ids[1] + 1))

    def static_piece():
        begin_and_vision(eng)
        abi.check(piece(eng, abi.PIECE_STATIC, static[-1], T, use_mask), "STATIC")

    names1, out1 = run(eng, T, use_mask, lambda: eng._enqueue_step(T, use_mask, static[-1]), static)
    names2, out2 = run(eng, T, use_mask, static_piece, static)
    assert len(names1) > 50 and names1 == names2
    for k in out1:
        assert torch.equal(out1[k], out2[k]), k
    if compaction:
        eng.clear_env_exit()


def plan_rule(cfg, exit_ids, max_layer):
    """mosaic_gpt_3b.py:397-443 with value_net.py:122-125: layer i runs while i <= max_layer; it is checked when it is an exit; its pseudo
    action is needed when the NEXT layer is an exit that has no earlier exit to compare with"""
    rows = []
    for i in range(max_layer + 1):
        need_pseudo = (i + 1) in exit_ids and i + 1 < cfg.exit_interval and i + 1 <= max_layer
        is_exit = i in exit_ids
        rows.append((int(need_pseudo), int(is_exit), exit_ids.index(i) if is_exit else -1))
    return rows


def test_the_stored_plan_follows_its_setters(owner):
    eng = owner.sibling(2)
    cfg, ids = eng.cfg, list(eng.cfg.exit_ids())
    eng.configure_exit(ids, ids[-1] + 1)
    first = read_plan(eng)
    assert first == plan_rule(cfg, ids, ids[-1]) and len(first) == ids[-1] + 1
    eng.set_env_exit([[1e8] * 3, [1e8] * 3], [ids[0], ids[1]])            # caps below the configured maximum
    capped = read_plan(eng)
    assert capped == plan_rule(cfg, ids, ids[1]) and len(capped) == ids[1] + 1
    eng.clear_env_exit()
    assert read_plan(eng) == first
    eng.configure_exit(ids, ids[1] + 1)                                    # the controller's own cap
    assert read_plan(eng) == capped
    eng.configure_exit(ids, ids[-1] + 1)


def refused(eng, which, index, T=5):
    eng.prof_begin()
    rc = piece(eng, which, index, T, False)
    return rc == ERR_SHAPE and eng.prof_end() == []


def test_a_piece_outside_the_plan_is_refused_before_any_launch(owner):
    eng = owner.sibling(2)
    ids = list(eng.cfg.exit_ids())
    eng.configure_exit(ids, ids[1] + 1)                                    # plan: layers 0 .. ids[1] of the model's ids[-1] + 1
    plan = read_plan(eng)
    no_eval = [i for i, (need_pseudo, is_exit, _) in enumerate(plan) if not (need_pseudo or is_exit)]
    assert no_eval and len(plan) < eng.cfg.n_layers
    load(eng, 5)
    assert refused(eng, abi.PIECE_HEADS, no_eval[0])
    assert refused(eng, abi.PIECE_MAIN, len(plan)) and refused(eng, abi.PIECE_HEADS, len(plan))
    assert refused(eng, abi.PIECE_MAIN, -1) and refused(eng, abi.PIECE_STATIC, eng.cfg.n_layers) and refused(eng, 3, 0)
    assert refused(eng, abi.PIECE_MAIN, 0, T=eng.max_T + 1)
    eng.configure_exit(ids, ids[-1] + 1)
    cfg = deer_tiny(use_state=True)
    st = DeerEngine(cfg, syn.make_synthetic_state(cfg, 1, bf16_round=True))
    assert refused(st, abi.PIECE_MAIN, 0) and refused(st, abi.PIECE_HEADS, 1)
