"""Sliding temporal context windows on the MI355X: cfg_ddim_step_windows_kernel against the fp64 restatement and against
cfg_ddim_step_kernel, the windowed pipeline against a hand-written per-window loop on the real kernels, the captured windowed
step against the eager one, one windowed step against the fp32 oracle, and a clip longer than the motion modules' PE table."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import record as _record, rel  # noqa: E402
from imagine360_amd import configs, kernels as K, synthetic as S  # noqa: E402
from imagine360_amd.context import WindowPlan, context_weights, context_windows, ip_cache_slots  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler  # noqa: E402
from test_context_windows import (TOL, capture_loop_inputs, hand_written_windowed_loop, host_windows_step, pipe_kw,  # noqa: E402
                                  windows_case)

torch.set_grad_enabled(False)

# (sample shape, L, starts): 16-byte lanes (inner % 8 == 0) and the scalar path, element counts that are no multiple of the
# 256-thread block, 1 / 2 / 3 / 5 windows, frames covered by three windows
KERNEL_CASES = [((1, 4, 12, 4, 8), 8, [0, 4]),                  # panorama, inner 32: 192 lanes
                ((1, 4, 8, 5, 7), 8, [0]),                      # one window, inner 35: scalar path, 1120 elements
                ((1, 3, 4, 12, 3, 5), 8, [0, 2, 4]),            # perspective, inner 15, frames 4 .. 7 in three windows
                ((1, 4, 20, 6, 4), 8, [0, 3, 6, 9, 12])]        # five windows (context_windows(20, 8, 5)), inner 24


def _sched():
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    return sch, sch._timesteps_host[8]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_windows_kernel_all_modes_vs_fp64(dt):
    sch, t = _sched()
    assert context_windows(20, 8, 5) == KERNEL_CASES[3][2]
    errs = {}
    for ci, (shape, L, starts) in enumerate(KERNEL_CASES):
        preds, x, z = windows_case(shape, L, starts, dt, seed=60 + ci)
        dp, dx, dz = preds.cuda(), x.cuda(), z.cuda()
        st = torch.tensor(starts, dtype=torch.int32, device="cuda")
        for kind in ("uniform", "pyramid"):
            w = context_weights(L, kind)
            dw = w.cuda()
            for eta in (0.0, 0.8):
                coefs = sch.step_coefficients(t, eta, 7.5)
                coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
                for pred in (0, 1, 2):
                    for extra in (0, 4, 8, 12):
                        mode = pred | extra
                        noise, dnoise = (z, dz) if eta > 0 else (None, None)
                        ref = host_windows_step(preds, x, noise, starts, w, mode, coefs)
                        out = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs)
                        assert out.dtype == dt and out.shape == x.shape
                        errs[f"case{ci}_{kind}_eta{eta}_mode{mode}"] = e = rel(out, ref)
                        assert e < TOL[dt], (ci, kind, eta, mode, e)
                        out2 = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, (0.0,) * 6, coef_dev=coef_dev)
                        assert torch.equal(out2, out), (ci, kind, eta, mode)
    # grid-stride loop: more 16-byte lanes than the 4096-block grid covers in one pass
    shape, L, starts = (1, 4, 33, 256, 256), 16, [0, 9, 17]
    preds, x, z = windows_case(shape, L, starts, dt, seed=70)
    assert x.numel() // 8 > 4096 * 256
    w = context_weights(L, "pyramid")
    coefs = sch.step_coefficients(t, 1.0, 7.5)
    out = K.cfg_ddim_step_windows(preds.cuda(), x.cuda(), z.cuda(), torch.tensor(starts, dtype=torch.int32, device="cuda"),
                                  w.cuda(), 1 | 4, coefs)
    errs["grid_stride"] = e = rel(out, host_windows_step(preds, x, z, starts, w, 1 | 4, coefs))
    assert e < TOL[dt] and torch.isfinite(out.float()).all()
    _record(f"cfg_ddim_step_windows_{str(dt).split('.')[-1]}", max_rel=max(errs.values()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_one_uniform_window_is_cfg_ddim_step_bit_for_bit(dt):
    sch, t = _sched()
    for shape in ((1, 4, 5, 7, 24), (1, 3, 4, 5, 4, 8)):              # panorama / perspective, 3360 / 1920 elements
        L = shape[-3]
        preds, x, z = windows_case(shape, L, [0], dt, seed=80)
        preds[0, 0].view(-1)[:64] = 0.0                                 # exact zeros of both signs through the blend
        preds[0, 1].view(-1)[:64] = 0.0
        preds[0, 1].view(-1)[:32] = -0.0
        dp, dx, dz = preds.cuda(), x.cuda(), z.cuda()
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        w = context_weights(L, "uniform").cuda()
        for eta in (0.0, 0.8):
            coefs = sch.step_coefficients(t, eta, 7.5)
            noise = dz if eta > 0 else None
            for pred in (0, 1, 2):
                for extra in (0, 4, 8, 12):
                    mode = pred | extra
                    a = K.cfg_ddim_step_windows(dp, dx, noise, st, w, mode, coefs)
                    b = K.cfg_ddim_step(dp[0, 0:1].contiguous(), dp[0, 1:2].contiguous(), dx, noise, mode, coefs)
                    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (shape, eta, mode)


def test_windows_kernel_rejects_bad_arguments():
    a = torch.zeros(1, 4, 4, 2, 8, dtype=torch.bfloat16, device="cuda")
    p = torch.zeros(2, 2, 4, 2, 2, 8, dtype=torch.bfloat16, device="cuda")
    st, w = torch.tensor([0, 2], dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    coefs = (7.5, 0.5, 0.8, 0.6, 0.7, 0.1)
    with pytest.raises(ValueError, match="noise"):
        K.cfg_ddim_step_windows(p, a, None, st, w, 1, coefs)
    with pytest.raises(RuntimeError, match="mode 3 unsupported"):
        K.cfg_ddim_step_windows(p, a, a, st, w, 3, coefs)
    with pytest.raises(AssertionError):
        K.cfg_ddim_step_windows(p[:, :, :, :1], a, a, st, torch.ones(1, device="cuda"), 1, coefs)      # not contiguous
    with pytest.raises(AssertionError):
        K.cfg_ddim_step_windows(p, a, a, st.long(), w, 1, coefs)
    ptr = a.data_ptr()
    rc = K.lib().im360_cfg_ddim_step_windows(p.data_ptr(), ptr, ptr, ptr, st.data_ptr(), w.data_ptr(), 2, 4, 4, 5, 16, *coefs, 1, 0, None, None)
    assert rc != 0 and b"out of range" in K.lib().im360_last_error()                                      # L > F
    rc = K.lib().im360_cfg_ddim_step_windows(p.data_ptr(), ptr, ptr, ptr, st.data_ptr(), w.data_ptr(), 2, 4, 4, 2, 16, *coefs, 1, 7, None, None)
    assert rc != 0 and b"dtype 7 unsupported" in K.lib().im360_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def gpu_pipe():
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
    pipe._no_progress = True
    return pipe


def _run(pipe, vb, cond, use_graph, seed=33, steps=2, **kw):
    pipe.use_graph = use_graph
    torch.manual_seed(seed)
    random.seed(seed)
    args = pipe_kw(cond, vb, latents_dtype=torch.bfloat16, **kw)
    args["num_inference_steps"] = steps
    vid = pipe("synthetic", **args).videos
    torch.cuda.synchronize()
    return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone()


def test_windowed_pipeline_equals_hand_written_loop_on_the_kernels(gpu_pipe):
    """F = 24, L = 16, overlap 8 (windows at 0 and 8), eager, device RNG: bit-identical to slicing by hand, calling the model
    per window in order and blending with the kernel -- every window forward is the same launch sequence on the same numbers."""
    pipe = gpu_pipe
    vb = S.video_batch(frames=24, pano_hw=(128, 256), seed=7)
    cond = S.conditioning(frames=24, seed=7)
    st = {}
    capture_loop_inputs(pipe, st)
    try:
        vid, pano, pers = _run(pipe, vb, cond, False, context_frames=16, context_overlap=8)
    finally:
        del pipe._windowed_loop
    assert vid.shape == (1, 3, 24, 128, 256) and torch.isfinite(vid).all()
    assert context_windows(24, 16, 8) == [0, 8]
    random.setstate(st["py_rng"])
    torch.cuda.set_rng_state(st["cuda_rng"])
    h_pano, h_pers = hand_written_windowed_loop(pipe.mv_base_model, pipe.scheduler, st, [0, 8], 16, context_weights(16, "pyramid"),
                                                K.cfg_ddim_step_windows)
    errs = dict(pano=rel(pano, h_pano), pers=rel(pers, h_pers))
    _record("windowed_pipeline_vs_hand_loop", **errs)
    assert torch.equal(pano, h_pano) and torch.equal(pers, h_pers), errs
    # the windows matter: the unwindowed 24-frame run from the same seeds is a different clip
    _, full_pano, _ = _run(pipe, vb, cond, False)
    assert rel(pano, full_pano) > 1e-2


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_graphed_windowed_steps_equal_eager_bit_for_bit(gpu_pipe, eta, monkeypatch):
    from imagine360_amd import graph_step
    replays = []
    orig = graph_step.GraphedWindowedStep.step
    monkeypatch.setattr(graph_step.GraphedWindowedStep, "step", lambda self, t: (replays.append(t), orig(self, t))[1])
    pipe = gpu_pipe
    vb = S.video_batch(frames=24, pano_hw=(128, 256), seed=8)
    cond = S.conditioning(frames=24, seed=8)
    out, states = {}, {}
    for graph in (True, False):
        gen = torch.Generator(device="cuda").manual_seed(77) if eta > 0 else None
        kw = dict(eta=eta, generator=gen) if eta > 0 else {}
        out[graph] = _run(pipe, vb, cond, graph, steps=3, context_frames=16, context_overlap=8, **kw)
        states[graph] = (random.getstate(), torch.cuda.get_rng_state(), gen.get_state() if gen is not None else None)
    assert len(replays) == 3
    errs = dict(pano=rel(out[True][1], out[False][1]), pers=rel(out[True][2], out[False][2]))
    _record(f"graphed_vs_eager_windows_eta{int(eta)}", **errs)
    assert all(torch.equal(a, b) for a, b in zip(out[True], out[False])), errs
    assert all(torch.isfinite(v.float()).all() for v in out[True])
    assert states[True][0] == states[False][0], "Python RNG (WarpAttn coins)"
    assert torch.equal(states[True][1], states[False][1]), "device RNG (IP-adapter noise)"
    if eta > 0:
        assert torch.equal(states[True][2], states[False][2]), "user generator (variance noise)"


@pytest.mark.parametrize("dt,tol", [(torch.bfloat16, 3e-2), (torch.float16, 4e-3)])
def test_windowed_step_vs_oracle(dt, tol):
    """One windowed step (F = 24, L = 16, overlap 8; 16 is the shortest window the IP adapter's two 4x temporal poolings of the
    SAM features accept) of the reduced-width model of test_model_gpu.py::test_mv_forward_vs_oracle:
    expected = the fp32 oracle's forward per window, blended and stepped in fp64 here.  Same bound as that test: the blend is a
    convex combination of per-window predictions that each meet it."""
    from im360_oracle import mv as OMV
    from im360_oracle.cfg import sd21_unet_cfg
    dev = torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    mv.noise_on_host = True
    F, L = 24, 16
    inp = S.mv_inputs(frames=F, pano_hw=(32, 64), pers_hw=(16, 16), seed=0, sam_frames=F)
    cams = S.icosahedron_cameras(90, 128)
    dinp = S.cast_mv_inputs(inp, dev, dt)
    sch, t = _sched()
    dinp["timestep"] = inp["timestep"] = torch.tensor([t], dtype=torch.int64)
    plan = WindowPlan(F, L, 8, "pyramid", dev)
    assert plan.starts == [0, 8]
    pano_lat, pers_lat = dinp["pano_latent"][:1, :4].contiguous(), dinp["latents"][:1, :, :4].contiguous()
    preds_pers, preds_pano = plan.pred_buffers(pano_lat, pers_lat)
    torch.manual_seed(7)
    random.seed(7)
    with ip_cache_slots(mv, len(plan)):
        plan.forward(mv, dinp, plan.static_inputs(dinp), cams, dinp["timestep"].to(dev), True, preds_pers, preds_pano)
    new_pano = sch.fused_cfg_step_windows(preds_pano, plan.starts_dev, plan.weights, 7.5, t, pano_lat)
    new_pers = sch.fused_cfg_step_windows(preds_pers, plan.starts_dev, plan.weights, 7.5, t, pers_lat)
    torch.cuda.synchronize()

    cfg = sd21_unet_cfg(5)
    cfg.xformers = True
    sd = {k: v.float().cpu() for k, v in mv.state_dict().items()}
    q = lambda v: v.to(dt).float() if torch.is_floating_point(v) else v
    torch.manual_seed(7)
    random.seed(7)
    masks, o_pers, o_pano = {}, [], []
    for s in plan.starts:
        e = s + L
        op, on = OMV.mv_forward(sd, cfg, q(inp["latents"][:, :, :, s:e]), q(inp["pano_latent"][:, :, s:e]), inp["timestep"],
                                q(inp["prompt_embd"]), q(inp["pano_prompt_embd"]), cams, inp["fps_tensor_pano"],
                                inp["fps_tensor_pers"], q(inp["reference_images_clip_feat_pano"][:, s:e]),
                                q(inp["reference_images_clip_feat_pers"][:, :, s:e]), inp["relative_position_tensor"][:, s:e],
                                inp["pitchs_tensor"][:, s:e], mask_cache=masks)
        o_pers.append(op)
        o_pano.append(on)
    coefs = sch.step_coefficients(t, 0.0, 7.5)
    w = context_weights(L, "pyramid")
    e_pano = host_windows_step(torch.stack(o_pano), q(inp["pano_latent"])[:1, :4], None, plan.starts, w, sch.kernel_mode(), coefs)
    e_pers = host_windows_step(torch.stack(o_pers), q(inp["latents"])[:1, :, :4], None, plan.starts, w, sch.kernel_mode(), coefs)
    errs = dict(pano_latent=rel(new_pano, e_pano), pers_latent=rel(new_pers, e_pers),
                pano_pred_w0=rel(preds_pano[0], o_pano[0]), pano_pred_w1=rel(preds_pano[1], o_pano[1]),
                pers_pred_w0=rel(preds_pers[0], o_pers[0]), pers_pred_w1=rel(preds_pers[1], o_pers[1]))
    _record(f"windowed_step_vs_oracle_{str(dt).split('.')[-1]}", **errs)
    assert max(errs.values()) < tol, errs


def test_80_frames_run_in_windows_of_16_and_not_without(gpu_pipe):
    """80 frames exceed temporal_position_encoding_max_len = 64: with context_frames = 16 every forward sees positions 0 .. 15
    (7 windows); the same call without the keyword still raises (in the SAM temporal projection's attention when the SAM features
    cover the 80 frames -- the pipeline never gets as far as the motion modules, whose frame_pe still raises the
    temporal_position_encoding_max_len ValueError for 80 positions)."""
    pipe = gpu_pipe
    vb = S.video_batch(frames=80, pano_hw=(128, 256), seed=9)
    cond = S.conditioning(frames=80, seed=9)
    vid, pano, pers = _run(pipe, vb, cond, True, steps=1, context_frames=16)
    assert vid.shape == (1, 3, 80, 128, 256) and torch.isfinite(vid).all()
    assert pano.shape == (1, 4, 80, 16, 32) and pers.shape == (1, 20, 4, 80, 8, 8)
    assert torch.isfinite(pano.float()).all() and torch.isfinite(pers.float()).all()
    assert len(context_windows(80, 16, 4)) == 7
    # the same call without the keyword: with SAM features of all 80 frames the first module that attends over time is the
    # IP adapter's temporal projection, whose attention kernel refuses more than 64 frames before any motion module is reached
    with pytest.raises(RuntimeError, match="80 frames > 64"):
        _run(pipe, vb, cond, True, steps=1)
    # ... and the motion modules behind it still refuse 80 frame positions: the ceiling itself is unchanged
    from imagine360_amd.unet3d import VersatileAttention
    mms = [m for m in pipe.mv_base_model.modules() if isinstance(m, VersatileAttention) and m.pos_encoder is not None]
    assert mms and mms[0].frame_pe(16, torch.bfloat16).shape[0] == 16
    with pytest.raises(ValueError, match="temporal_position_encoding_max_len"):
        mms[0].frame_pe(80, torch.bfloat16)
    torch.cuda.synchronize()
