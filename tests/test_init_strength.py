"""Starting the denoising from a given clip, on CPU: the scheduler's ``add_noise`` / ``get_velocity`` / ``__len__`` against a restatement
of the reference formulas (scheduling_ddim.py:375-419), ``timesteps_for_strength`` and ``noise_coefficients``, the torch stand-in of
``kernels.noise_latents`` against an fp64 composition (add_noise, then gather, then mask), and the pipeline's ``init_latents`` /
``init_video`` / ``strength`` keywords under emulated kernels."""
import random

import pytest
import torch

import _emu_ddim_step as ES
import _emu_kernels as E
import _emu_noise_latents as EN
from _emu_noise_latents import TOL, fp64_composition, gathered, noise_case, same_bits
from helpers import rel
from imagine360_amd import configs, synthetic as S
from imagine360_amd.scheduler import DDIMScheduler

torch.set_grad_enabled(False)


def _sched(n=25):
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(n)
    return sch


# ------------------------------------------------------------------------------------------------ 1. the scheduler
def _factor(abar, t, like):
    """The reference's coefficient: the table cast to the samples' dtype, indexed, ``** 0.5`` by the caller's expression, flattened and
    given trailing axes until it broadcasts from the left."""
    v = abar.flatten()
    while v.dim() < like.dim():
        v = v.unsqueeze(-1)
    return v


def ref_add_noise(alphas_cumprod, x, noise, t):
    abar = alphas_cumprod.to(device=x.device, dtype=x.dtype)
    return _factor(abar[t] ** 0.5, t, x) * x + _factor((1 - abar[t]) ** 0.5, t, x) * noise


def ref_get_velocity(alphas_cumprod, x, noise, t):
    abar = alphas_cumprod.to(device=x.device, dtype=x.dtype)
    return _factor(abar[t] ** 0.5, t, x) * noise - _factor((1 - abar[t]) ** 0.5, t, x) * x


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ts", [[481], [0, 999, 481]])
def test_add_noise_get_velocity_len_against_the_reference_formulas(dt, ts):
    sch = _sched()
    table = sch.alphas_cumprod.clone()
    g = torch.Generator().manual_seed(5)
    b = len(ts) if len(ts) > 1 else 2                        # a 1-element timestep tensor broadcasts over the batch
    x, n = (torch.randn(b, 4, 3, 5, 6, generator=g).to(dt) for _ in range(2))
    t = torch.tensor(ts, dtype=torch.int64)
    got_a, got_v = sch.add_noise(x, n, t), sch.get_velocity(x, n, t)
    want_a, want_v = ref_add_noise(table, x, n, t), ref_get_velocity(table, x, n, t)
    assert got_a.dtype == dt and got_a.shape == x.shape and got_v.dtype == dt and got_v.shape == x.shape
    assert torch.equal(got_a, want_a) and torch.equal(got_v, want_v)          # the same torch ops: the same bits, in fp32 and in bf16
    if dt == torch.float32:          # (in bf16 the reference's own cast of the table dominates: a_0 = 0.99915 becomes 1, so no fp64 bound there)
        assert rel(got_a, ref_add_noise(table, x.double(), n.double(), t)) < 1e-6
    assert len(sch) == sch.config.num_train_timesteps == 1000
    # the table is not moved or re-typed (the reference re-types the attribute in place): _alphas still reads fp32 on the host
    assert sch.alphas_cumprod.dtype == torch.float32 and sch.alphas_cumprod.device.type == "cpu" and torch.equal(sch.alphas_cumprod, table)
    out = sch.step(n.float(), sch._timesteps_host[3], x.float())
    assert torch.isfinite(out.prev_sample).all()


def test_timesteps_for_strength():
    sch = _sched(25)
    host = list(sch._timesteps_host)
    assert sch.timesteps_for_strength(1.0) == (0, host)
    i0, steps = sch.timesteps_for_strength(0.5)
    assert i0 == 13 and len(steps) == 12 and steps == host[13:]
    i0, steps = sch.timesteps_for_strength(0.04)
    assert i0 == 24 and steps == host[24:] and len(steps) == 1
    with pytest.raises(ValueError, match=r"25.*0\.03|0\.03.*25"):
        sch.timesteps_for_strength(0.03)
    for bad in (0, -0.1, 1.2):
        with pytest.raises(ValueError, match="strength"):
            sch.timesteps_for_strength(bad)
    sch.set_timesteps(3)
    assert sch.timesteps_for_strength(2 / 3) == (1, sch._timesteps_host[1:])


def test_noise_coefficients_are_the_step_coefficients():
    sch = _sched(25)
    for t in sch._timesteps_host:
        sa, sb = sch.noise_coefficients(t)
        _, want_a, want_b, *_ = sch.step_coefficients(t, 0.3, 7.5)
        assert isinstance(sa, float) and isinstance(sb, float) and sa == want_a and sb == want_b
        a = float(sch.alphas_cumprod[t])
        assert sa == a ** 0.5 and sb == (1.0 - a) ** 0.5


# ------------------------------------------------------------------------------------------------ 2. the kernel's contract
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(3, 4, 5, 12, 3, 4, 6), (2, 4, 8, 24, 2, 3, 5)])
def test_stand_in_against_fp64_composition(dt, shape):
    sch = _sched(25)
    t = sch.timesteps_for_strength(0.5)[1][0]
    x0, noise, idx, ok = noise_case(*shape, dt)
    pano, pers = EN.noise_latents(x0, noise, idx, ok, *sch.noise_coefficients(t))
    F, C, h, w, M, ph, pw = shape
    assert pano.shape == (1, C, F, h, w) and pers.shape == (1, M, C, F, ph, pw) and pano.dtype == pers.dtype == dt
    want_pano, want_pers = fp64_composition(sch, t, x0, noise, idx, ok)
    assert rel(pano, want_pano) < TOL[dt] and rel(pers, want_pers) < TOL[dt]
    assert same_bits(pers, gathered(pano, idx, ok))                      # the gather of the ROUNDED panorama start, exactly
    assert (pers.permute(0, 2, 3, 1, 4, 5)[..., ok == 0] == 0).all() and (ok == 0).any()


# ------------------------------------------------------------------------------------------------ 3. the pipeline's host logic
@pytest.fixture(scope="module")
def cpu_pipe():
    from imagine360_amd.pipeline import AnimationPipeline
    mv = configs.build_mv_model(5, device="cpu", dtype=torch.float32, xformers=False)
    vae = configs.build_vae(4, device="cpu", dtype=torch.float32)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM")
    pipe.rng, pipe._no_progress = "host", True
    pipe.enable_vae_slicing()
    return pipe


@pytest.fixture(scope="module")
def clip4():
    return S.video_batch(frames=4, pano_hw=(128, 256), seed=6), S.conditioning(frames=16, seed=6)


def pipe_kw(cond, vb, steps, **extra):
    return dict(num_inference_steps=steps, guidance_scale_text=7.5, negative_prompt="", video_batch=vb, use_outpaint=True,
                use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video", latents_dtype=torch.float32,
                prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **extra)


def _run(pipe, seed=3, **kw):
    torch.manual_seed(seed)
    random.seed(seed)
    vid = pipe("synthetic", **kw).videos
    return vid, [v.clone() for v in pipe.last_latents]


@pytest.fixture(scope="module")
def first_call(cpu_pipe, clip4):
    """Three steps from pure noise, without the new keywords, inside the counting patch: (latents, calls of noise_latents)."""
    vb, cond = clip4
    with E.patched_kernels(), ES.patched_step_kernel(), EN.patched_noise_latents() as calls:
        _, lat = _run(cpu_pipe, **pipe_kw(cond, vb, 3))
        return lat, len(calls)


def test_without_an_init_the_call_is_the_one_without_the_keywords(cpu_pipe, clip4, first_call):
    vb, cond = clip4
    lat0, calls0 = first_call
    with E.patched_kernels(), ES.patched_step_kernel(), EN.patched_noise_latents() as calls:
        _, lat = _run(cpu_pipe, **pipe_kw(cond, vb, 3, init_latents=None, init_video=None, strength=1.0))
    assert calls0 == 0 and calls == []                                  # noise_latents is never reached
    assert torch.equal(lat[0], lat0[0]) and torch.equal(lat[1], lat0[1])


def test_strength_runs_the_last_steps_only(cpu_pipe, clip4, first_call):
    """num_inference_steps = 3, strength = 2/3 from the first call's latent: two steps, the last two timesteps, counted from 0; the
    start latents are the stand-in's on init_noise's own panorama noise draw."""
    vb, cond = clip4
    x0 = first_call[0][0]
    trace, seen = [], []
    with E.patched_kernels(), ES.patched_step_kernel(), EN.patched_noise_latents() as starts:
        vid, lat = _run(cpu_pipe, **pipe_kw(cond, vb, 3, init_latents=x0, strength=2 / 3, trace=trace,
                                            callback=lambda i, t, latent: seen.append((i, t))))
    assert len(starts) == 1                                              # one call of noise_latents: its (pano, pers)
    host = cpu_pipe.scheduler._timesteps_host
    assert len(host) == 3 and len(trace) == 2
    assert seen == [(0, host[1]), (1, host[2])]
    assert vid.shape == (1, 3, 4, 128, 256) and torch.isfinite(vid).all()
    assert torch.equal(trace[-1], lat[0]) and not torch.equal(lat[0], x0)
    # the start: x0 noised to host[1] with the panorama noise init_noise draws first thing in the call, from the same seed
    torch.manual_seed(3)
    noise = torch.randn(1, 4, 1, 4, 16, 32).squeeze(2).permute(0, 2, 1, 3, 4)
    sa, sb = cpu_pipe.scheduler.noise_coefficients(host[1])
    assert rel(starts[0][0], sa * x0.double() + sb * noise.double()) < 1e-6
    assert starts[0][1].shape == (1, 20, 4, 4, 8, 8)


def test_bad_combinations_are_refused(cpu_pipe, clip4, first_call):
    from imagine360_amd.dist import FrameShard
    vb, cond = clip4
    x0 = first_call[0][0]
    video = vb["pano_pixel_values"]
    with E.patched_kernels(), ES.patched_step_kernel(), EN.patched_noise_latents():
        with pytest.raises(ValueError, match="strength=0.5 needs init_latents or init_video"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, 3, strength=0.5))
        with pytest.raises(ValueError, match="at most one of init_latents and init_video"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, 3, init_latents=x0, init_video=video, strength=0.5))
        for init in (dict(init_latents=x0), dict(init_video=video)):
            with pytest.raises(ValueError, match="cannot be combined with frame_shard.*not implemented"):
                cpu_pipe("synthetic", **pipe_kw(cond, vb, 3, frame_shard=FrameShard(4, rank=0, world=1), strength=0.5, **init))
        with pytest.raises(ValueError, match="strength"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, 3, init_latents=x0, strength=0.2))        # int(3 * 0.2) = 0 steps
        with pytest.raises(ValueError, match=r"\[1, 4, 4, 16, 32\]"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, 3, init_latents=x0[:, :, :2], strength=0.5))


def test_init_video_draws_nothing_from_the_rng(cpu_pipe, clip4):
    """The encode of an init clip takes the posterior's mode: Python's and torch's generators are where they were, and a call with
    ``init_video`` is the call with ``init_latents`` = its encoding, bit for bit."""
    from imagine360_amd.pipeline import VAE_SCALE
    vb, cond = clip4
    video = vb["pano_pixel_values"]                                       # [1, 4, 3, 128, 256] in [-1, 1]
    with E.patched_kernels(), ES.patched_step_kernel(), EN.patched_noise_latents():
        torch.manual_seed(9)
        random.seed(9)
        state = (random.getstate(), torch.get_rng_state())
        x0 = cpu_pipe.encode_init_video(video)
        assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])
        assert x0.shape == (1, 4, 4, 16, 32)
        mode = torch.cat([cpu_pipe.vae.encode(video[0, i:i + 1], 1).latent_dist.mode() for i in range(4)])
        assert rel(x0, mode.unsqueeze(0).permute(0, 2, 1, 3, 4) * VAE_SCALE) < 1e-5
        _, a = _run(cpu_pipe, **pipe_kw(cond, vb, 2, init_video=video, strength=0.5))
        _, b = _run(cpu_pipe, **pipe_kw(cond, vb, 2, init_latents=x0, strength=0.5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
