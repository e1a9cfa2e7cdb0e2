"""Sliding temporal context windows on CPU: the window plan's properties, the torch stand-in of the blend + CFG + DDIM kernel
against an fp64 restatement of its formula, and the windowed pipeline under emulated kernels against a loop written out by hand."""
import math
import random

import pytest
import torch

import _emu_ctx_step as EC
import _emu_ddim_step as ES
import _emu_kernels as E
from helpers import rel
from imagine360_amd import configs, synthetic as S
from imagine360_amd.context import context_weights, context_windows
from imagine360_amd.scheduler import DDIMScheduler

torch.set_grad_enabled(False)
TOL = {torch.bfloat16: 1e-2, torch.float16: 3e-3}          # the table of cfg_ddim_step (test_ddim_stochastic_gpu.py)


# ------------------------------------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("frames", [1, 7, 8, 16, 17, 24, 48, 64, 80, 96])
@pytest.mark.parametrize("length", [8, 16])
def test_window_plan_properties(frames, length):
    for overlap in (0, 4, length - 1):
        starts = context_windows(frames, length, overlap)
        L = min(frames, length)
        assert starts == sorted(starts) and len(set(starts)) == len(starts) and starts[0] == 0
        assert all(isinstance(s, int) and 0 <= s <= frames - L for s in starts)
        assert starts[-1] + L == frames                                     # the last window ends on the last frame
        cov = [sum(1 for s in starts if s <= f < s + L) for f in range(frames)]
        assert min(cov) >= 1
        assert max(cov) <= math.ceil(length / (length - overlap)) + 1
        if length >= frames:
            assert starts == [0]
        else:
            stride = length - overlap
            assert starts[:-1] == [k * stride for k in range(len(starts) - 1)]
            assert all(s + length < frames for s in starts[:-1])


def test_window_plan_examples_and_errors():
    assert context_windows(48, 16, 4) == [0, 12, 24, 32]
    assert context_windows(24, 16, 8) == [0, 8]
    assert context_windows(12, 8, 4) == [0, 4]
    assert context_windows(17, 16, 0) == [0, 1]
    assert context_windows(80, 16, 4) == [0, 12, 24, 36, 48, 60, 64]
    for bad in (-1, 16, 17):
        with pytest.raises(ValueError):
            context_windows(48, 16, bad)
    assert torch.equal(context_weights(4, "uniform"), torch.ones(4))
    assert context_weights(5, "pyramid").tolist() == [1, 2, 3, 2, 1] and context_weights(6, "pyramid").tolist() == [1, 2, 3, 3, 2, 1]
    assert context_weights(16, "pyramid").dtype == torch.float32
    with pytest.raises(ValueError):
        context_weights(8, "triangle")


# ------------------------------------------------------------------------------------------------ 2. the kernel's formula
def host_windows_step(preds, x, z, starts, weights, mode, coefs):
    """fp64 restatement of the windowed step, frame by frame: m = sum_k w[f - s_k] (u_k + g (c_k - u_k)) / sum_k w[f - s_k] over
    the windows covering frame f, then DDIMScheduler.step on m (scheduling_ddim.py:300-368)."""
    g, sa, sb, sap, direction, sigma = coefs
    fd = x.dim() - 3
    L = preds.shape[fd + 1]
    x = x.double()
    out = torch.empty_like(x)
    for f in range(x.shape[fd]):
        num, den = 0.0, 0.0
        for k, s in enumerate(int(v) for v in starts):
            if s <= f < s + L:
                u, c = preds[k, 0].double().select(fd - 1, f - s), preds[k, 1].double().select(fd - 1, f - s)
                num = num + float(weights[f - s]) * (u + g * (c - u))
                den = den + float(weights[f - s])
        m = (num / den).unsqueeze(0)
        xf = x.select(fd, f)
        pred = mode & 3
        if pred == 0:
            x0, e = (xf - sb * m) / sa, m
        elif pred == 1:
            x0, e = sa * xf - sb * m, sa * m + sb * xf
        else:
            x0, e = m, m
        if mode & 4:
            x0 = x0.clamp(-1, 1)
        if mode & 8:
            e = (xf - sa * x0) / sb
        o = sap * x0 + direction * e
        if z is not None:
            o = o + sigma * z.double().select(fd, f)
        out.select(fd, f).copy_(o)
    return out


def windows_case(shape, L, starts, dt, seed=51):
    """Seeded predictions [nW, 2, ...] / sample / noise of one view shape, a guided x0 partly inside, partly outside [-1, 1]."""
    gen = torch.Generator().manual_seed(seed)
    fd = len(shape) - 3
    pshape = list(shape)
    pshape[fd] = L
    preds = (torch.randn(len(starts), 2, *pshape[1:], generator=gen) * 0.25).to(dt)
    x, z = (torch.randn(shape, generator=gen).to(dt) for _ in range(2))
    return preds, x, z


VIEW_SHAPES = [((1, 4, 12, 4, 8), 8, [0, 4]), ((1, 3, 4, 12, 3, 5), 8, [0, 2, 4])]       # panorama / perspective latent


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["uniform", "pyramid"])
def test_stand_in_against_fp64_restatement(dt, kind):
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    t = sch._timesteps_host[8]
    for shape, L, starts in VIEW_SHAPES:
        preds, x, z = windows_case(shape, L, starts, dt)
        w = context_weights(L, kind)
        st = torch.tensor(starts, dtype=torch.int32)
        for eta in (0.0, 0.8):
            coefs = sch.step_coefficients(t, eta, 7.5)
            for pred in (0, 1, 2):
                for extra in (0, 4, 8, 12):
                    mode = pred | extra
                    noise = z if eta > 0 else None
                    out = EC.cfg_ddim_step_windows(preds, x, noise, st, w, mode, coefs)
                    ref = host_windows_step(preds, x, noise, starts, w, mode, coefs)
                    assert out.dtype == dt and out.shape == x.shape
                    e = rel(out, ref)
                    assert e < TOL[dt], (shape, eta, mode, kind, e)
                    out2 = EC.cfg_ddim_step_windows(preds, x, noise, st, w, mode, (0.0,) * 6, coef_dev=torch.tensor(coefs))
                    assert rel(out2, out) < 1e-6
    # one window, uniform weights: the unwindowed stand-in, bit for bit
    preds, x, z = windows_case((1, 4, 8, 4, 8), 8, [0], dt)
    coefs = sch.step_coefficients(t, 0.8, 7.5)
    one = EC.cfg_ddim_step_windows(preds, x, z, torch.zeros(1, dtype=torch.int32), context_weights(8, "uniform"), 1, coefs)
    assert torch.equal(one, ES.cfg_ddim_step(preds[0, 0:1], preds[0, 1:2], x, z, 1, coefs))
    with pytest.raises(ValueError, match="noise"):
        EC.cfg_ddim_step_windows(preds, x, None, torch.zeros(1, dtype=torch.int32), context_weights(8, "uniform"), 1, coefs)


# ------------------------------------------------------------------------------------------------ 3. host logic
def pipe_kw(cond, vb, **extra):
    return dict(num_inference_steps=2, guidance_scale_text=7.5, negative_prompt="", video_batch=vb, use_outpaint=True,
                use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video",
                prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **extra)


def capture_loop_inputs(pipe, store):
    """Wrap ``pipe._windowed_loop`` so that the state the windowed loop starts from -- the whole-clip model inputs, the initial
    latents, the timesteps and the RNG states -- is recorded in ``store`` (cloned) before the loop runs."""
    orig = pipe._windowed_loop

    def spy(plan, inputs, cameras, pano_latent, pers_latent, steps_host, ts_dev, *rest):
        store.update(inputs={k: (v.clone() if torch.is_tensor(v) else v) for k, v in inputs.items()}, cameras=cameras,
                     pano=pano_latent.clone(), pers=pers_latent.clone(), steps=list(steps_host), ts_dev=ts_dev,
                     py_rng=random.getstate(), cpu_rng=torch.get_rng_state(),
                     cuda_rng=torch.cuda.get_rng_state() if pano_latent.is_cuda else None)
        return orig(plan, inputs, cameras, pano_latent, pers_latent, steps_host, ts_dev, *rest)
    pipe._windowed_loop = spy


def hand_written_windowed_loop(mv, sch, st, starts, L, weights, blend, eta=0.0, noise_fn=None, g=7.5):
    """The windowed loop written out: per step and per window (ascending) slice the frame axis of everything that is indexed
    by frame, call the model, keep the prediction; then blend + step each branch with ``blend`` (panorama first).
    ``noise_fn(latent, frame_dim)``: the variance noise of one branch (eta > 0)."""
    inp, pano, pers = st["inputs"], st["pano"].clone(), st["pers"].clone()
    dev = pano.device
    sdev, wdev = torch.tensor(starts, dtype=torch.int32, device=dev), weights.to(dev)
    for i, t in enumerate(st["steps"]):
        inp["pano_latent"][:, :4] = pano
        inp["latents"][:, :, :4] = pers
        pp, pn = [], []
        for s in starts:
            e = s + L
            feat_pers = inp["reference_images_clip_feat_pers"]          # one feature tensor shared by all views (stride 0)
            pred_pers, pred_pano = mv(
                latents=inp["latents"][:, :, :, s:e], pano_latent=inp["pano_latent"][:, :, s:e], timestep=st["ts_dev"][i],
                prompt_embd=inp["prompt_embd"], pano_prompt_embd=inp["pano_prompt_embd"], cameras=st["cameras"],
                use_fps_condition=True, use_ip_plus_cross_attention=True, fps_tensor_pano=inp["fps_tensor_pano"],
                fps_tensor_pers=inp["fps_tensor_pers"],
                reference_images_clip_feat_pano=inp["reference_images_clip_feat_pano"][:, s:e].contiguous(),
                reference_images_clip_feat_pers=feat_pers[:, 0, s:e].contiguous().unsqueeze(1).expand(-1, feat_pers.shape[1], -1, -1, -1),
                relative_position_tensor=inp["relative_position_tensor"][:, s:e], pitchs_tensor=inp["pitchs_tensor"][:, s:e])
            pp.append(pred_pers.to(pers.dtype))
            pn.append(pred_pano.to(pano.dtype))
        coefs = sch.step_coefficients(t, eta, g)
        mode = sch.kernel_mode()
        z = noise_fn(pano, 2) if eta > 0 else None
        pano = blend(torch.stack(pn).contiguous(), pano, z, sdev, wdev, mode, coefs)
        z = noise_fn(pers, 3) if eta > 0 else None
        pers = blend(torch.stack(pp).contiguous(), pers, z, sdev, wdev, mode, coefs)
    return pano, pers


@pytest.fixture(scope="module")
def cpu_pipe():
    from imagine360_amd.pipeline import AnimationPipeline
    mv = configs.build_mv_model(5, device="cpu", dtype=torch.float32, xformers=False)
    vae = configs.build_vae(4, device="cpu", dtype=torch.float32)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM")
    pipe.rng, pipe._no_progress = "host", True
    pipe.enable_vae_slicing()
    return pipe


@pytest.mark.parametrize("eta", [0.0, 0.8])
def test_windowed_pipeline_equals_hand_written_loop(cpu_pipe, eta):
    """F = 12, L = 8, overlap 4 (windows at 0 and 4), 2 steps, host RNG: the pipeline's latents equal the hand-written loop's bit
    for bit, and the RNG streams end in the same state (nW forwards per step, then the whole clip's two variance noises)."""
    pipe = cpu_pipe
    vb = S.video_batch(frames=12, pano_hw=(128, 256), seed=5)
    cond = S.conditioning(frames=12, seed=5)
    st = {}
    with E.patched_kernels(), ES.patched_step_kernel(), EC.patched_windows_kernel():
        capture_loop_inputs(pipe, st)
        try:
            torch.manual_seed(17)
            random.seed(17)
            trace = []
            vid = pipe("synthetic", eta=eta, latents_dtype=torch.float32, context_frames=8, context_overlap=4, trace=trace,
                       **pipe_kw(cond, vb)).videos
        finally:
            del pipe._windowed_loop
        got = [v.clone() for v in pipe.last_latents]
        end_state = (random.getstate(), torch.get_rng_state())
        assert vid.shape == (1, 3, 12, 128, 256) and torch.isfinite(vid).all() and len(trace) == 2
        assert torch.equal(trace[-1], got[0])
        random.setstate(st["py_rng"])
        torch.set_rng_state(st["cpu_rng"])
        mv = pipe.mv_base_model
        noise = lambda lat, fd: torch.randn(lat.shape, dtype=torch.float32)
        pano, pers = hand_written_windowed_loop(mv, pipe.scheduler, st, [0, 4], 8, context_weights(8, "pyramid"),
                                                EC.cfg_ddim_step_windows, eta, noise)
        assert torch.equal(got[0], pano) and torch.equal(got[1], pers)
        assert random.getstate() == end_state[0] and torch.equal(torch.get_rng_state(), end_state[1])
        assert mv.unet.ip_cache_entries == 1 and mv.pano_unet.ip_cache_entries == 1


def test_context_frames_at_least_the_clip_is_the_plain_call_and_frame_shard_is_refused(cpu_pipe):
    from imagine360_amd.dist import FrameShard
    pipe = cpu_pipe
    vb = S.video_batch(frames=4, pano_hw=(128, 256), seed=6)
    cond = S.conditioning(frames=16, seed=6)
    outs = []
    with E.patched_kernels(), ES.patched_step_kernel(), EC.patched_windows_kernel():
        for extra in ({}, dict(context_frames=4), dict(context_frames=16, context_overlap=4, context_weights="uniform")):
            torch.manual_seed(3)
            random.seed(3)
            pipe("synthetic", latents_dtype=torch.float32, **pipe_kw(cond, vb), **extra)
            outs.append([v.clone() for v in pipe.last_latents])
        with pytest.raises(ValueError, match="frame_shard"):
            pipe("synthetic", latents_dtype=torch.float32, frame_shard=FrameShard(4, rank=0, world=1), context_frames=2, context_overlap=1,
                 **pipe_kw(cond, vb))
        with pytest.raises(ValueError, match="overlap"):
            pipe("synthetic", latents_dtype=torch.float32, context_frames=2, context_overlap=2, **pipe_kw(cond, vb))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
