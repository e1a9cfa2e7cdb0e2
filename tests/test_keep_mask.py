"""Regenerating part of a given clip, on CPU: ``DDIMScheduler.keep_coefficients`` against the schedule, the torch stand-in of
``kernels.keep_latents`` against an fp64 composition built from ``add_noise`` (and its two exact ends), and the pipeline's
``regenerate_mask`` keyword under emulated kernels: the refusals, the resize and polarity of the mask, and the loop (one block and
context windows) with an all-1, an all-0 and a half mask."""
import random

import pytest
import torch

import _emu_ctx_step as EC
import _emu_ddim_step as ES
import _emu_keep_latents as EK
import _emu_kernels as E
import _emu_noise_latents as EN
from _emu_keep_latents import fp64_composition, half_mask, keep_case, kept, mask_at_views
from _emu_noise_latents import TOL, gathered, same_bits
from helpers import rel
from imagine360_amd import configs, synthetic as S
from imagine360_amd.scheduler import DDIMScheduler

torch.set_grad_enabled(False)


def _sched(n=25):
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(n)
    return sch


# ------------------------------------------------------------------------------------------------ 1. the scheduler
@pytest.mark.parametrize("n,strength", [(25, 1.0), (25, 0.5), (3, 1.0), (3, 2 / 3), (3, 0.34)])
def test_keep_coefficients_follow_the_schedule(n, strength):
    """After step i the kept region is at the level of steps[i + 1], the timestep the NEXT step denoises from -- not at steps[i], the
    level the step has just left -- and clean after the last step."""
    sch = _sched(n)
    _, steps = sch.timesteps_for_strength(strength)
    assert len(steps) == min(int(n * strength), n)
    for i in range(len(steps) - 1):
        got = sch.keep_coefficients(steps, i)
        a = float(sch.alphas_cumprod[steps[i + 1]])
        assert got == sch.noise_coefficients(steps[i + 1]) == (a ** 0.5, (1.0 - a) ** 0.5)
        assert got != sch.noise_coefficients(steps[i]) and got[0] > sch.noise_coefficients(steps[i])[0]       # one level cleaner
        assert all(isinstance(v, float) for v in got)
    assert sch.keep_coefficients(steps, len(steps) - 1) == (1.0, 0.0)
    for bad in (-1, len(steps)):
        with pytest.raises(ValueError, match="keep_coefficients"):
            sch.keep_coefficients(steps, bad)


# ------------------------------------------------------------------------------------------------ 2. the kernel's contract
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(3, 4, 5, 12, 3, 4, 6), (2, 4, 8, 24, 2, 3, 5)])
def test_stand_in_against_fp64_composition(dt, shape):
    sch = _sched(25)
    steps = sch.timesteps_for_strength(0.5)[1]
    sa, sb = sch.keep_coefficients(steps, 0)
    pano, pers, x0, noise, mask, idx, ok = keep_case(*shape, dt)
    assert all(((mask[f] == 0).any() and (mask[f] == 1).any() and ((mask[f] > 0) & (mask[f] < 1)).any()) for f in range(shape[0]))
    assert not torch.equal(mask[0], mask[1]) and (ok == 0).any()
    want_pano, want_pers = fp64_composition(sch, steps[1], pano, pers, x0, noise, mask, idx, ok)
    got_pano, got_pers = pano.clone(), pers.clone()
    out = EK.keep_latents(got_pano, got_pers, x0, noise, mask, idx, ok, sa, sb)
    assert out[0] is got_pano and out[1] is got_pers                                       # in place
    assert rel(got_pano, want_pano) < TOL[dt] and rel(got_pers, want_pers) < TOL[dt]
    # the exact ends: mask 1 keeps the input bits, mask 0 is the noised clip (the gather of it in the views), unseen pixels stay
    k = EK.known(x0, noise, sa, sb)
    w5 = mask[None, None].expand_as(pano)
    assert same_bits(got_pano[w5 >= 1], pano[w5 >= 1]) and same_bits(got_pano[w5 <= 0], k[w5 <= 0])
    wg = mask_at_views(mask, idx, ok).expand_as(pers)
    seen = ok.bool()[None, :, None, None].expand_as(pers)
    assert same_bits(got_pers[wg >= 1], pers[wg >= 1]) and same_bits(got_pers[~seen], pers[~seen])
    assert same_bits(got_pers[seen & (wg <= 0)], gathered(k, idx, ok)[seen & (wg <= 0)])
    assert (seen & (wg <= 0)).any() and (seen & (wg > 0) & (wg < 1)).any()
    # (1, 0) with an all-0 mask returns x0 itself, and coefficients from a tensor are the host coefficients
    p2, v2 = pano.clone(), pers.clone()
    EK.keep_latents(p2, v2, x0, noise, torch.zeros_like(mask), idx, ok, 1.0, 0.0)
    assert same_bits(p2, x0) and same_bits(v2[seen], gathered(x0, idx, ok)[seen]) and same_bits(v2[~seen], pers[~seen])
    p3, v3 = pano.clone(), pers.clone()
    EK.keep_latents(p3, v3, x0, noise, mask, idx, ok, 0.0, 0.0, coef_dev=torch.tensor([sa, sb], dtype=torch.float32))
    assert same_bits(p3, got_pano) and same_bits(v3, got_pers)


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


def patches():
    import contextlib
    st = contextlib.ExitStack()
    for cm in (E.patched_kernels(), ES.patched_step_kernel(), EC.patched_windows_kernel(), EN.patched_noise_latents()):
        st.enter_context(cm)
    return st


@pytest.fixture(scope="module")
def first_call(cpu_pipe, clip4):
    """Three steps from pure noise: the clean clip the other tests start from."""
    vb, cond = clip4
    with patches(), EK.patched_keep_latents() as calls:
        _, lat = _run(cpu_pipe, **pipe_kw(cond, vb, 3))
    assert calls == []
    return lat


def test_bad_combinations_are_refused(cpu_pipe, clip4, first_call):
    from imagine360_amd.dist import FrameShard
    vb, cond = clip4
    x0, mask = first_call[0], vb["pano_mask"]
    with patches(), EK.patched_keep_latents() as calls:
        with pytest.raises(ValueError, match="regenerate_mask needs init_latents or init_video"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, 3, regenerate_mask=mask))
        with pytest.raises(ValueError, match="regenerate_mask has 3 frames.*video_length = 4"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, 3, init_latents=x0, strength=2 / 3, regenerate_mask=mask[:, :3]))
        with pytest.raises(ValueError, match=r"regenerate_mask must be \[1, F, 1, H, W\]"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, 3, init_latents=x0, strength=2 / 3, regenerate_mask=mask[0]))
        with pytest.raises(ValueError, match="regenerate_mask cannot be combined with frame_shard.*not implemented"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, 3, init_latents=x0, strength=2 / 3, regenerate_mask=mask,
                                            frame_shard=FrameShard(4, rank=0, world=1)))
    assert calls == []


def test_mask_resize_and_polarity_are_those_of_the_pano_mask(cpu_pipe, clip4):
    """The resize is the call ``prepare_masked_latents_pano`` makes on ``video_batch["pano_mask"]``; 1 stays 1 (regenerate), 0 stays 0
    (keep), values outside [0, 1] are clamped."""
    vb, _ = clip4
    mask = vb["pano_mask"]                                                 # [1, 4, 1, 128, 256]
    assert mask.shape == (1, 4, 1, 128, 256) and (mask == 0).any() and (mask == 1).any()
    with patches():
        torch.manual_seed(1)
        _, want = cpu_pipe.prepare_masked_latents_pano(4, vb["pano_pixel_values"] * (mask < 0.5), mask)
    got = cpu_pipe.prepare_regenerate_mask(mask, 4, 16, 32, "cpu")
    assert got.shape == (4, 16, 32) and got.dtype == torch.float32 and got.is_contiguous()
    assert torch.equal(got, want[0, 0].float())
    ragged = half_mask(4, 100, 250) * 0.5                                  # not a multiple of the stride, fractional
    want = torch.nn.functional.interpolate(ragged.transpose(2, 1), size=(4, 16, 32))[0, 0]
    assert torch.equal(cpu_pipe.prepare_regenerate_mask(ragged, 4, 16, 32, "cpu"), want) and set(want.unique().tolist()) == {0.0, 0.5}
    wild = torch.tensor([-2.0, 0.25, 3.0]).reshape(1, 1, 1, 1, 3).expand(1, 4, 1, 16, 3)
    assert cpu_pipe.prepare_regenerate_mask(wild, 4, 16, 3, "cpu")[0, 0].tolist() == [0.0, 0.25, 1.0]


@pytest.mark.parametrize("windows", [{}, dict(context_frames=2, context_overlap=1)], ids=["one_block", "windows"])
def test_loop_blends_after_every_step(cpu_pipe, clip4, first_call, windows):
    """3 steps, strength 2/3: two steps, one ``keep_latents`` call after each, at ``keep_coefficients``; an all-1 mask is the call
    without the keyword, an all-0 mask returns the init clip, a half mask keeps its region and ``trace`` sees the blended latent."""
    vb, cond = clip4
    x0 = first_call[0]
    kw = lambda **extra: pipe_kw(cond, vb, 3, init_latents=x0, strength=2 / 3, **windows, **extra)
    ones = torch.ones(1, 4, 1, 128, 256)
    half = half_mask(4, 128, 256)
    with patches(), EK.patched_keep_latents() as calls:
        vid0, plain = _run(cpu_pipe, **kw())
        assert calls == []                                                 # without the keyword nothing new runs
        vid1, all1 = _run(cpu_pipe, **kw(regenerate_mask=ones))
        sch = cpu_pipe.scheduler
        steps = sch._timesteps_host[1:]
        assert [c[:2] for c in calls] == [sch.keep_coefficients(steps, 0), sch.keep_coefficients(steps, 1)]
        assert calls[0][:2] == sch.noise_coefficients(steps[1]) and calls[1][:2] == (1.0, 0.0)
        assert torch.equal(vid0, vid1) and torch.equal(plain[0], all1[0]) and torch.equal(plain[1], all1[1])
        del calls[:]
        _, all0 = _run(cpu_pipe, **kw(regenerate_mask=1 - ones))
        assert len(calls) == 2 and torch.equal(all0[0], x0)
        from imagine360_amd import pano_geometry as G
        idx, ok = G.nearest_e2p_index(16, 32, vb["pers_size"] // 8, vb["pers_size"] // 8, vb["cameras"])
        seen = ok.bool()[None, :, None, None].expand_as(all0[1])
        assert torch.equal(all0[1][seen], gathered(x0, idx, ok.to(torch.uint8))[seen])
        del calls[:]
        trace, seen_cb = [], []
        _, got = _run(cpu_pipe, **kw(regenerate_mask=half, trace=trace, callback=lambda i, t, lat: seen_cb.append(lat.clone())))
        keep = kept(half, 16, 32).expand_as(x0)
        assert keep.any() and not keep.all() and not torch.equal(keep[:, :, 0], keep[:, :, 1])
        assert torch.equal(got[0][keep], x0[keep]) and not torch.equal(got[0][~keep], x0[~keep])
        assert len(trace) == 2 and torch.equal(trace[0], calls[0][2]) and torch.equal(trace[1], got[0]) and torch.equal(seen_cb[0], trace[0])
        # after the first step the kept region is the clip noised to the NEXT timestep with the call's first noise draw
        torch.manual_seed(3)
        noise = torch.randn(1, 4, 1, 4, 16, 32).squeeze(2).permute(0, 2, 1, 3, 4)
        sa, sb = sch.noise_coefficients(steps[1])
        assert rel(trace[0][keep], (sa * x0.double() + sb * noise.double())[keep]) < 1e-6
        wrong = sch.noise_coefficients(steps[0])
        assert rel(trace[0][keep], (wrong[0] * x0.double() + wrong[1] * noise.double())[keep]) > 1e-2
