"""The reference's Python surface on top of the HIP engine: factory -> MPTFlamingo.forward with (a) a static exit_id,
(b) the native ExitController (device-side exit, one graph replay per step) and (c) a FOREIGN controller written
against the reference protocol `ctl(all_hidden_states, b_idx) -> bool` that calls `exit_head(feats[i],
update_hidden_state=False)` (here: the oracle's restatement of ActionValueNet/ExitController, pinned to the
reference) - all three against the golden outputs of the reference's own MPTFlamingo.forward."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load  # noqa: E402
from deer_vla_amd import factory, synthetic as syn  # noqa: E402
from deer_vla_amd.value_net import ActionValueNet, ExitController  # noqa: E402
from oracle import deer_oracle as orc  # noqa: E402

TOL = 1e-2


@pytest.fixture(scope="module")
def setup():
    cfg, seed, g = load("deer_forward.npz")
    sd = syn.make_synthetic_state(cfg, seed, bf16_round=True)
    model, image_processor, tok = factory.create_model_and_transforms(
        "ViT-L-14", "openai", "", "", cross_attn_every_n_layers=1, window_size=12, use_gripper=True, fusion_mode="post",
        llm_name="mpt_dolly_3b", state_dict=sd, cfg=cfg)
    return cfg, g, model


def test_static_exit_matches_reference_forward(setup):
    cfg, g, model = setup
    ids, mask = g["ids"].long().cuda(), g["mask"].cuda()
    for eid in (3, 4, -1):
        model.clear_all_exit_memory()
        o = model(vision_x=g["rgb"][0].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=g["grip"][0].cuda(),
                  state_tensor=torch.zeros(1, 1, 1, 15).cuda(), return_feature=True, deterministic=True, exit_id=eid)
        tag = f"static{eid}"
        assert o.exit_layer == int(g[tag + "_exit"]) and len(o.hidden_states) == o.exit_layer + 1
        assert o.logits[0].shape == (1, 1, 6) and o.logits[1].shape == (1, 1, 1)
        assert float((o.logits[0].cpu() - g[tag + "_pose"]).abs().max()) < TOL
        assert float((o.logits[1].cpu() - g[tag + "_grip"]).abs().max()) < TOL
        ref_h = g[tag + "_hidden"][-1]
        assert float((o.hidden_states[-1].cpu() - ref_h).abs().max() / ref_h.abs().max()) < 2e-2
    assert model.lang_encoder.is_conditioned()


@pytest.mark.parametrize("tag", ["dyn", "dynS"])
def test_native_controller_matches_reference_dynamic_exit(setup, tag):
    cfg, g, model = setup
    ids, mask = g["ids"].long().cuda(), g["mask"].cuda()
    model.clear_all_exit_memory()
    vn = ActionValueNet(model.get_all_exit_idx(), model.extra_exit, cfg.exit_interval, cfg.window_size, "L2")
    ctl = ExitController(vn, model.get_all_exit_idx(), steps_per_stage=1, leq=True, exit_dist="exp", max_layer=int(g[tag + "_max_layer"]))
    ctl._set_threshold_value([float(t) for t in g[tag + "_thr"]])
    for s in range(g["rgb"].shape[0]):
        ctl.module.set_timestep(s)                      # eval_utils.py:662-663
        o = model(vision_x=g["rgb"][s].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=g["grip"][s].cuda(),
                  return_feature=True, deterministic=True, exit_id=None, dynamic_early_exit=True, exit_controller=ctl)
        assert o.exit_layer == int(g[tag + "_exit"][s]), (tag, s)
        assert float((o.logits[0].cpu() - g[tag + "_pose"][s]).abs().max()) < TOL
        assert float((o.logits[1].cpu() - g[tag + "_grip"][s]).abs().max()) < TOL
        assert ctl.cur_exit_id == o.exit_layer
        # ActionValueNet.get_ensemble_action (value_net.py:92-95; eval_utils.py:457-461): mean of the last two exit-check actions of
        # the step, computed by the exit check on the device - against the reference's own output
        ep, eg = vn.get_ensemble_action()
        assert ep.shape == (1, 1, 6) and eg.shape == (1, 1, 1)
        assert vn._ensemble[2] == int(g[tag + "_ens_count"][s]), (tag, s)
        assert float((ep - g[tag + "_ens_pose"][s]).abs().max()) < TOL
        assert float((eg - g[tag + "_ens_grip"][s]).abs().max()) < TOL
        vn.reset_actions()
        with pytest.raises(AssertionError):                        # value_net.py:93
            vn.get_ensemble_action()


def test_foreign_controller_protocol(setup):
    """A controller that is NOT ours: the oracle's ExitController/ValueNet drive our `extra_exit` head object through
    the reference protocol (slow host loop, one sync per exit check)."""
    cfg, g, model = setup
    ids, mask = g["ids"].long().cuda(), g["mask"].cuda()
    tag = "dyn"
    model.clear_all_exit_memory()
    head = model.extra_exit

    class HeadAdapter:                                   # the oracle value net calls head(feats, update_hidden_state=...)
        def __call__(self, feats, update_hidden_state=True, **kw):
            a, gr = head(feats, update_hidden_state=update_hidden_state)
            return a.cpu(), gr.cpu()
    vn = orc.OracleValueNet(model.get_all_exit_idx(), HeadAdapter(), cfg.exit_interval, cfg.window_size, "L2")
    ctl = orc.OracleExitController(vn, model.get_all_exit_idx(), steps_per_stage=1, max_layer=int(g[tag + "_max_layer"]))
    ctl._set_threshold_value([float(t) for t in g[tag + "_thr"]])
    for s in range(g["rgb"].shape[0]):
        ctl.set_timestep(s)
        o = model(vision_x=g["rgb"][s].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=g["grip"][s].cuda(),
                  return_feature=True, deterministic=True, exit_id=None, dynamic_early_exit=True, exit_controller=ctl)
        assert o.exit_layer == int(g[tag + "_exit"][s]), s
        assert float((o.logits[0].cpu() - g[tag + "_pose"][s]).abs().max()) < TOL


def test_native_controller_called_through_the_llm_loop(setup):
    """the NATIVE controller invoked with the reference protocol - ``lang_encoder(ids, mask, exit_controller=ctl)``
    runs the reference's host loop (mosaic_gpt_3b.py:397-443), which calls ``ctl(all_hidden_states, b_idx)`` after every layer; the
    controller's ``forward`` (value_net.py:277-297) then evaluates ``ActionValueNet.forward`` -> ``extra_exit(feats[i],
    update_hidden_state=False)`` on the engine's head kernels.  Exit layers and actions against the reference's own dynamic-exit
    goldens, and identical to what the device-side gate decides for the same controller."""
    cfg, g, model = setup
    ids, mask = g["ids"].long().cuda(), g["mask"].cuda()
    tag = "dyn"
    model.clear_all_exit_memory()
    e = model.engine
    vn = ActionValueNet(model.get_all_exit_idx(), model.extra_exit, cfg.exit_interval, 1, "L2")
    ctl = ExitController(vn, model.get_all_exit_idx(), steps_per_stage=1, leq=True, exit_dist="exp", max_layer=int(g[tag + "_max_layer"]))
    ctl._set_threshold_value([float(t) for t in g[tag + "_thr"]])
    for s in range(g["rgb"].shape[0]):
        ctl.set_timestep(s)
        e.load_inputs(g["rgb"][s].cuda(), g["grip"][s].cuda(), ids, mask)
        e.enqueue_vision()
        out = model.lang_encoder(ids, mask, exit_controller=ctl)
        assert out.exit_layer == int(g[tag + "_exit"][s]) == ctl.cur_exit_id, s
        assert len(out.hidden_states) == out.exit_layer + 1
        pose, grip = model.extra_exit(out.hidden_states[out.exit_layer], update_hidden_state=True)      # flamingo_mpt.py:459
        assert float((pose.cpu() - g[tag + "_pose"][s]).abs().max()) < TOL
        ep, eg = vn.get_ensemble_action()                      # host-side action list of the slow path (value_net.py:92-95)
        assert float((ep.cpu() - g[tag + "_ens_pose"][s]).abs().max()) < TOL
        vn.reset_actions()


def test_forward_argument_errors(setup):
    cfg, g, model = setup
    ids, mask = g["ids"].long().cuda(), g["mask"].cuda()
    with pytest.raises(ValueError):
        model(vision_x=g["rgb"][0].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=None, exit_id=1)
    with pytest.raises(NotImplementedError):                       # training branch is out of scope
        model(vision_x=g["rgb"][0].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=g["grip"][0].cuda())
    with pytest.raises(AssertionError):                            # mosaic_gpt_3b.py:300
        model.lang_encoder(ids, mask, exit_controller=lambda h, b: True, exit_id=1)


@pytest.mark.gpu
def test_eval_time_hook_reports_per_stage_gpu_times():
    """flamingo_mpt.py:386-417: ``eval_time=True`` -> ``llm_inference_time`` = time of the lang_encoder call (here: GPU time of the
    trunk + exit checks of the step), with the vision tower reported beside it."""
    from deer_vla_amd import synthetic as syn
    from deer_vla_amd.config import deer_tiny
    from deer_vla_amd.flamingo_mpt import MPTFlamingo
    cfg = deer_tiny()
    model = MPTFlamingo(cfg, syn.make_synthetic_state(cfg, 3, bf16_round=True))
    rgb, grip, ids, mask = syn.synthetic_step_inputs(cfg, 0)
    for _ in range(3):                                       # graphs are captured on the first calls
        o = model(vision_x=rgb.cuda(), lang_x=ids.cuda(), attention_mask=mask.cuda(), vision_gripper=grip.cuda(), exit_id=3, eval_time=True)
    assert o.exit_layer == 3
    assert 0.0 < model.llm_inference_time < model.forward_time and 0.0 < model.vision_time < model.forward_time


def test_eval_time_hook_on_a_dynamic_step_times_the_stages_and_leaves_the_results_unchanged():
    """``eval_time=True`` on a DYNAMIC step (native ExitController, exit decided on the device): the pipelined step reports the GPU
    time of the vision tower and of the trunk + exit checks like the static step does, and timing a step changes nothing of what
    it computes - exit layer and action bit-equal to a freshly built second model fed the same steps with ``eval_time=False``.
    Thresholds [0, 1e5, 1e5] with the "<=" criterion: the first check (an L2 distance <= 0) does not fire, the second always
    does, so every step ends at the inner exit layer 3 of deer_tiny's exits [1, 3, 5], not at the forced last one."""
    from deer_vla_amd.config import deer_tiny
    from deer_vla_amd.flamingo_mpt import MPTFlamingo
    cfg = deer_tiny()
    assert cfg.exit_ids() == [1, 3, 5]
    sd = syn.make_synthetic_state(cfg, 3, bf16_round=True)
    steps = [syn.synthetic_step_inputs(cfg, s) for s in range(4)]         # the first call captures the graph pieces

    def run(eval_time):
        model = MPTFlamingo(cfg, sd)
        vn = ActionValueNet(model.get_all_exit_idx(), model.extra_exit, cfg.exit_interval, cfg.window_size, "L2")
        ctl = ExitController(vn, model.get_all_exit_idx(), steps_per_stage=1, leq=True, exit_dist="exp", max_layer=12)
        ctl._set_threshold_value([0.0, 1e5, 1e5])
        outs = []
        for s, (rgb, grip, ids, mask) in enumerate(steps):
            ctl.module.set_timestep(s)
            o = model(vision_x=rgb.cuda(), lang_x=ids.cuda(), attention_mask=mask.cuda(), vision_gripper=grip.cuda(), exit_id=None,
                      dynamic_early_exit=True, exit_controller=ctl, eval_time=eval_time)
            outs.append((o.exit_layer, o.logits[0].cpu().clone(), o.logits[1].cpu().clone()))
        return model, outs

    timed, a = run(True)
    assert 0.0 < timed.llm_inference_time < timed.forward_time and 0.0 < timed.vision_time < timed.forward_time
    _, b = run(False)
    for s in range(4):
        assert a[s][0] == b[s][0] == 3, s
        assert torch.equal(a[s][1], b[s][1]) and torch.equal(a[s][2], b[s][2]), s


@pytest.mark.parametrize("name,precision", [("deer_forward_state.npz", "fp16"), ("deer_forward_sep.npz", "fp16"), ("deer_forward_sep.npz", "bf16"),
                                            ("deer_forward_state.npz", "fp32"), ("deer_forward_sep.npz", "fp32")])
def test_use_state_and_sep_resampler_variants_match_reference_forward(name, precision):
    """the two variants the reference parses from checkpoint names (eval_calvin.py:355-377) through the factory's own
    keywords - ``use_state`` (robot-state embedding in the action head, action_head.py:524-536; static exits only: the reference's
    dynamic exit raises with it, and so does this surface) and ``sep_resampler`` (own PerceiverResampler for the gripper camera,
    flamingo_mpt.py:132-134,656-659) - against the golden outputs of the reference's own MPTFlamingo.forward."""
    cfg, seed, g = load(name)
    tol = TOL if precision != "fp32" else 1e-3
    sd = syn.make_synthetic_state(cfg, seed, bf16_round=True)
    model, _, _ = factory.create_model_and_transforms(
        "ViT-L-14", "openai", "", "", cross_attn_every_n_layers=1, window_size=12, use_gripper=True, fusion_mode="post",
        llm_name="mpt_dolly_3b", state_dict=sd, cfg=cfg, use_state=cfg.use_state, sep_resampler=cfg.sep_resampler, precision=precision)
    assert model.use_state == cfg.use_state and model.sep_resampler == cfg.sep_resampler
    ids, mask = g["ids"].long().cuda(), g["mask"].cuda()
    n = g["rgb"].shape[0]
    for eid in (3, 4):
        model.clear_all_exit_memory()
        for s in range(n):
            o = model(vision_x=g["rgb"][s].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=g["grip"][s].cuda(),
                      state_tensor=g["state"][s].cuda(), return_feature=True, deterministic=True, exit_id=eid)
            assert float((o.logits[0].cpu() - g[f"static{eid}_pose"][s]).abs().max()) < tol, (eid, s)
            assert float((o.logits[1].cpu() - g[f"static{eid}_grip"][s]).abs().max()) < tol, (eid, s)
    ref_vis = g["vis_x"].reshape(-1, cfg.vit_width)
    vis = model.engine.vis_x_f32.cpu()
    assert float((vis - ref_vis).abs().max() / ref_vis.abs().max()) < (2e-2 if precision != "fp32" else 1e-4)
    vn = ActionValueNet(model.get_all_exit_idx(), model.extra_exit, cfg.exit_interval, cfg.window_size, "L2")
    if cfg.use_state:
        assert int(g["dynamic_raises"]) == 1                      # the reference raises TypeError here (fixture)
        ctl = ExitController(vn, model.get_all_exit_idx(), steps_per_stage=1, max_layer=12)
        ctl._set_threshold_value([1e5] * ctl.real_num_exit)
        with pytest.raises(NotImplementedError):
            model(vision_x=g["rgb"][0].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=g["grip"][0].cuda(),
                  state_tensor=g["state"][0].cuda(), exit_id=None, dynamic_early_exit=True, exit_controller=ctl)
        return
    model.clear_all_exit_memory()
    ctl = ExitController(vn, model.get_all_exit_idx(), steps_per_stage=1, leq=True, exit_dist="exp", max_layer=int(g["dyn_max_layer"]))
    ctl._set_threshold_value([float(t) for t in g["dyn_thr"]])
    for s in range(n):
        ctl.module.set_timestep(s)
        o = model(vision_x=g["rgb"][s].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=g["grip"][s].cuda(),
                  return_feature=True, deterministic=True, exit_id=None, dynamic_early_exit=True, exit_controller=ctl)
        assert o.exit_layer == int(g["dyn_exit"][s]), s
        assert float((o.logits[0].cpu() - g["dyn_pose"][s]).abs().max()) < tol
        assert float((o.logits[1].cpu() - g["dyn_grip"][s]).abs().max()) < tol


@pytest.mark.parametrize("name", ["deer_forward_lw.npz", "deer_forward_ms2.npz", "deer_forward_lw_ms3.npz"])
def test_layerwise_exit_eval_and_multi_step_action_match_reference_forward(name):
    """``layerwise_exit_eval`` (the action of exit layer k from that layer's own head lm_exits[k] / lm_head with
    its own LSTM history, flamingo_mpt.py:253-261,450-457; the exit decision stays with extra_exit, whose state nobody commits) and
    ``multi_step_action`` (6 A pose + A gripper values per head call, action_head.py:458,472-473; the criterion's delta over all 6 A pose
    values) through the factory's own keywords, against golden outputs of the REFERENCE's MPTFlamingo.forward
    (tests/golden/make_golden.py::gen_round5_variants): static exits with LSTM carry and a dynamic episode."""
    cfg, seed, g = load(name)
    A = cfg.multi_step_action
    sd = syn.make_synthetic_state(cfg, seed, bf16_round=True)
    model, _, _ = factory.create_model_and_transforms(
        "ViT-L-14", "openai", "", "", cross_attn_every_n_layers=1, window_size=12, use_gripper=True, fusion_mode="post",
        llm_name="mpt_dolly_3b", state_dict=sd, cfg=cfg, multi_step_action=A, layerwise_exit_eval=cfg.layerwise_exit_eval,
        multi_exit=cfg.layerwise_exit_eval)
    assert model.act_step == A and model.layerwise_exit_eval == cfg.layerwise_exit_eval
    ids, mask = g["ids"].long().cuda(), g["mask"].cuda()
    n = g["rgb"].shape[0]
    for eid in (3, 4):
        model.clear_all_exit_memory()
        for s in range(n):
            o = model(vision_x=g["rgb"][s].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=g["grip"][s].cuda(),
                      return_feature=True, deterministic=True, exit_id=eid)
            assert tuple(o.logits[0].shape) == (1, 1, 6 * A) and tuple(o.logits[1].shape) == (1, 1, A)
            assert float((o.logits[0].cpu() - g[f"static{eid}_pose"][s]).abs().max()) < TOL, (eid, s)
            assert float((o.logits[1].cpu() - g[f"static{eid}_grip"][s]).abs().max()) < TOL, (eid, s)
    vn = ActionValueNet(model.get_all_exit_idx(), model.extra_exit, cfg.exit_interval, cfg.window_size, "L2")
    model.clear_all_exit_memory()
    ctl = ExitController(vn, model.get_all_exit_idx(), steps_per_stage=1, leq=True, exit_dist="exp", max_layer=int(g["dyn_max_layer"]))
    ctl._set_threshold_value([float(t) for t in g["dyn_thr"]])
    for s in range(n):
        ctl.module.set_timestep(s)
        o = model(vision_x=g["rgb"][s].cuda(), lang_x=ids, attention_mask=mask, vision_gripper=g["grip"][s].cuda(),
                  return_feature=True, deterministic=True, exit_id=None, dynamic_early_exit=True, exit_controller=ctl)
        assert o.exit_layer == int(g["dyn_exit"][s]), s
        assert float((o.logits[0].cpu() - g["dyn_pose"][s]).abs().max()) < TOL
        assert float((o.logits[1].cpu() - g["dyn_grip"][s]).abs().max()) < TOL
    # through the harness wrapper: A actions per call, the first multi_execution of them executed (eval_utils.py:466-475)
    from deer_vla_amd import rollout as ro
    if A > 1:
        tok = factory.SyntheticTokenizer(cfg)
        w = ro.ModelWrapper(model, tok, factory.ClipImageProcessor(cfg.image_size), torch.float32, exit_id=3, multi_execution=2)
        env = ro.SyntheticEnv(seed=0)
        act = w.step(env.get_obs(), "push the block")
        assert act.shape == (2, 7) and act.dtype == np.float16 and set(np.unique(act[:, -1])) <= {-1.0, 1.0}


def test_sep_resampler_env_batch_matches_single_environment_runs():
    """sep_resampler with an env batch: frames are ordered camera-major inside the engine (one vision chain per camera, own Perceiver
    weights) and the media tokens are scattered back env-major - every environment must equal its own one-environment run bit for bit
    on the media tokens and within rounding on the action."""
    from deer_vla_amd.config import deer_tiny
    from deer_vla_amd.engine import DeerEngine
    cfg = deer_tiny(sep_resampler=True)
    sd = syn.make_synthetic_state(cfg, 5, bf16_round=True)
    B = 3
    one = DeerEngine(cfg, sd, n_envs=1)
    bat = DeerEngine(cfg, sd, n_envs=B)
    inp = [syn.synthetic_step_inputs(cfg, 0, rank=e, text_len=11, text_seed=7) for e in range(B)]
    rgb = torch.stack([p[0] for p in inp]).cuda()
    grip = torch.stack([p[1] for p in inp]).cuda()
    ids = torch.cat([p[2] for p in inp]).cuda()
    rb = bat.step(rgb, grip, ids, None, exit_id=3)
    vis_b = bat.vis_x_f32.clone().view(B, 2 * cfg.perc_latents, cfg.vit_width)
    for e in range(B):
        one.reset()
        r1 = one.step(inp[e][0].cuda(), inp[e][1].cuda(), inp[e][2].cuda(), None, exit_id=3)
        assert torch.equal(one.vis_x_f32.view(2 * cfg.perc_latents, cfg.vit_width), vis_b[e]), e
        assert float((r1["pose"] - rb[e]["pose"]).abs().max()) < 1e-3
