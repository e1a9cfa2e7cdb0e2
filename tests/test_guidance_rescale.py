"""Guidance rescale (arXiv 2305.08891, section 3.4) on CPU: ``rescale_noise_cfg`` against an fp64 restatement of its formula, the
routing of ``guidance_rescale`` to the kernels, the torch stand-in of the rescaled step kernels, and the pipeline keyword under
emulated kernels against a hand-written CFG + rescale + ``scheduler.step``."""
import random

import pytest
import torch

import _emu_ctx_step as EC
import _emu_ddim_step as ES
import _emu_kernels as E
import _emu_rescale_step as ER
from helpers import rel
from imagine360_amd import configs, synthetic as S
from imagine360_amd.context import context_weights
from imagine360_amd.scheduler import DDIMScheduler, rescale_noise_cfg

torch.set_grad_enabled(False)

# rescale_noise_cfg runs in the inputs' dtype like diffusers' function: two standard deviations, their quotient, the factor and the
# product are each rounded to it (torch.std accumulates wider and rounds once), so the result carries a handful of roundings of
# relative size eps / 2 each.  Bound: 4 eps of the dtype on the norm-relative error.
EPS = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def host_rescale(noise_cfg, text, phi):
    """fp64 restatement: m' = m (phi std(c) / std(m) + 1 - phi), std with correction 1 over every dimension but the batch."""
    m, c = noise_cfg.double(), text.double()
    out = torch.empty_like(m)
    for b in range(m.shape[0]):
        n = m[b].numel()
        std = lambda v: (((v - v.mean()) ** 2).sum() / (n - 1)).sqrt()
        out[b] = m[b] * (phi * std(c[b]) / std(m[b]) + (1.0 - phi))
    return out


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(1, 4, 5, 7, 24), (1, 3, 4, 5, 4, 8), (2, 4, 3, 4, 8)])
def test_rescale_noise_cfg_against_fp64_formula(dt, shape):
    gen = torch.Generator().manual_seed(11)
    u, c = (torch.randn(shape, generator=gen) * 0.25).to(dt), (torch.randn(shape, generator=gen) * 0.25 + 0.5).to(dt)
    m = (u.float() + 7.5 * (c.float() - u.float())).to(dt)
    for phi in (0.7, 1.0, 0.25):
        out = rescale_noise_cfg(m, c, phi)
        assert out.dtype == dt and out.shape == m.shape
        e = rel(out, host_rescale(m, c, phi))
        assert e < 4 * EPS[dt], (dt, shape, phi, e)
    full = rescale_noise_cfg(m.float(), c.float(), 1.0)                     # phi = 1: the result has the text prediction's std
    assert abs(float(full[0].std() / c[0].float().std()) - 1.0) < 1e-5
    assert rescale_noise_cfg(m, c, 0.0) is m and rescale_noise_cfg(m, c) is m        # phi = 0: the input itself


def test_degenerate_inputs_give_what_the_formula_gives():
    c = torch.randn(1, 4, 8)
    assert torch.isnan(rescale_noise_cfg(torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), 0.7)).all()          # 0 / 0
    assert torch.isinf(rescale_noise_cfg(torch.ones(1, 4, 8), c, 0.7)).all()                              # std(m) = 0
    assert torch.isnan(rescale_noise_cfg(torch.ones(1, 1), torch.ones(1, 1), 0.7)).all()                  # n = 1


def _sched():
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    return sch, sch._timesteps_host[3]


def test_guidance_rescale_routing():
    """phi = 0 calls exactly what is called without the keyword, with the same arguments; phi > 0 goes to the six-coefficient step
    kernel with rescale = phi, for eta = 0 too; the same for the windows path."""
    from imagine360_amd import kernels
    calls = []
    saved = kernels.cfg_ddim_update, kernels.cfg_ddim_step, kernels.cfg_ddim_step_windows
    kernels.cfg_ddim_update = lambda *a, **k: calls.append(("update", a[3:], k))
    kernels.cfg_ddim_step = lambda *a, **k: calls.append(("step", a[3:], k))
    kernels.cfg_ddim_step_windows = lambda *a, **k: calls.append(("windows", a[2:], k))
    try:
        x = torch.zeros(8)
        sch, t = _sched()
        assert sch.uses_step_kernel() is False and sch.uses_step_kernel(0.0, False) is False
        assert sch.uses_step_kernel(guidance_rescale=0.0) is False and sch.uses_step_kernel(guidance_rescale=0.7) is True
        sch.fused_cfg_step(x, x, 7.5, t, x)
        sch.fused_cfg_step(x, x, 7.5, t, x, guidance_rescale=0.0)
        sch.fused_cfg_step(x, x, 7.5, t, x, guidance_rescale=0.7)
        sch.fused_cfg_step(x, x, 7.5, None, x, coef_dev=x[:6], guidance_rescale=0.7)
        sch.fused_cfg_step(x, x, 7.5, t, x, eta=1.0, noise=x)
        sch.fused_cfg_step(x, x, 7.5, t, x, eta=1.0, noise=x, guidance_rescale=0.0)
        sch.fused_cfg_step(x, x, 7.5, t, x, eta=1.0, noise=x, guidance_rescale=0.7)
        p, st, w = torch.zeros(1, 2, 4, 2, 1, 1), torch.zeros(1, dtype=torch.int32), torch.ones(2)
        lat = torch.zeros(1, 4, 2, 1, 1)
        sch.fused_cfg_step_windows(p, st, w, 7.5, t, lat)
        sch.fused_cfg_step_windows(p, st, w, 7.5, t, lat, guidance_rescale=0.0)
        sch.fused_cfg_step_windows(p, st, w, 7.5, t, lat, guidance_rescale=0.7)
        sch.fused_cfg_step_windows(p, st, w, 7.5, t, lat, eta=1.0, noise=lat, guidance_rescale=0.7)
    finally:
        kernels.cfg_ddim_update, kernels.cfg_ddim_step, kernels.cfg_ddim_step_windows = saved
    cx, cv = sch.coefficients(t)
    assert calls[0] == calls[1] == ("update", (7.5, cx, cv), {"coef_dev": None})
    assert calls[2] == ("step", (None, 1, sch.step_coefficients(t, 0.0, 7.5)), {"coef_dev": None, "rescale": 0.7})
    assert calls[3][0] == "step" and calls[3][1] == (None, 1, (0.0,) * 6) and calls[3][2]["rescale"] == 0.7
    assert calls[3][2]["coef_dev"].data_ptr() == x.data_ptr()
    assert calls[4][0] == "step" and calls[4][2] == {"coef_dev": None} and calls[4][1][1:] == (1, sch.step_coefficients(t, 1.0, 7.5))
    assert calls[5][1][1:] == calls[4][1][1:] and calls[5][2] == calls[4][2]
    assert calls[6][0] == "step" and calls[6][1][1:] == calls[4][1][1:] and calls[6][2] == {"coef_dev": None, "rescale": 0.7}
    assert calls[7][0] == "windows" and calls[7][2] == {"coef_dev": None}
    assert calls[8][2] == calls[7][2] and calls[8][1][1:] == calls[7][1][1:]
    assert calls[9][0] == "windows" and calls[9][1][1:] == calls[7][1][1:] and calls[9][2] == {"coef_dev": None, "rescale": 0.7}
    assert calls[10][2] == {"coef_dev": None, "rescale": 0.7} and calls[10][1][-1] == sch.step_coefficients(t, 1.0, 7.5)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_stand_in_is_rescale_then_step(dt):
    """The stand-in of the rescaled kernels == rescale_noise_cfg on the fp32 combination, then the unrescaled stand-in's step; one
    uniform window with L = F is the plain stand-in; rescale = 0 is the stand-in of the shipped kernels."""
    sch, t = _sched()
    gen = torch.Generator().manual_seed(5)
    shape = (1, 4, 5, 7, 24)
    u, c, x, z = (torch.randn(shape, generator=gen).to(dt) for _ in range(4))
    u, c = u * 0.25, c * 0.25 + 0.5
    for eta in (0.0, 0.8):
        coefs = sch.step_coefficients(t, eta, 7.5)
        noise = z if eta > 0 else None
        for mode in (0, 1, 2 | 4, 1 | 12):
            m = u.float() + 7.5 * (c.float() - u.float())
            mr = rescale_noise_cfg(m, c.float(), 0.7)
            want = ES.cfg_ddim_step(mr, mr, x.float(), None if noise is None else noise.float(), mode, [1.0, *coefs[1:]]).to(dt)
            got = ER.cfg_ddim_step(u, c, x, noise, mode, coefs, rescale=0.7)
            assert got.dtype == dt and rel(got, want) < 1e-6, (eta, mode)
            assert torch.equal(ER.cfg_ddim_step(u, c, x, noise, mode, (0.0,) * 6, coef_dev=torch.tensor(coefs), rescale=0.7), got)
            assert torch.equal(ER.cfg_ddim_step(u, c, x, noise, mode, coefs, rescale=0.0), ES.cfg_ddim_step(u, c, x, noise, mode, coefs))
            preds = torch.stack([torch.cat([u, c])])
            st, w = torch.zeros(1, dtype=torch.int32), context_weights(shape[2], "uniform")
            assert torch.equal(ER.cfg_ddim_step_windows(preds, x, noise, st, w, mode, coefs, rescale=0.7), got)
            assert torch.equal(ER.cfg_ddim_step_windows(preds, x, noise, st, w, mode, coefs),
                               EC.cfg_ddim_step_windows(preds, x, noise, st, w, mode, coefs))
    r = ER.cfg_rescale_factor(u, c, 7.5, 0.7)
    m = u.double() + 7.5 * (c.double() - u.double())
    assert r.dtype == torch.float32 and abs(float(r) / (0.7 * float(c.double().std() / m.std()) + 0.3) - 1.0) < 1e-5


# ------------------------------------------------------------------------------------------------ pipeline
def _pipe_kw(cond, vb, **extra):
    return dict(num_inference_steps=2, guidance_scale_text=7.5, negative_prompt="", latents_dtype=torch.float32,
                video_batch=vb, use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True,
                ip_plus_condition="video", prompt_embeds=(cond["text_pano"], cond["text_pers"]),
                sam_features=(cond["sam_pano"], cond["sam_pers"]), **extra)


@pytest.fixture(scope="module")
def cpu_runs():
    """The w/5 synthetic pipeline, 2 steps, host RNG, emulated kernels: run(**keywords) -> (panorama latent, perspective latent)."""
    from imagine360_amd.pipeline import AnimationPipeline
    mv = configs.build_mv_model(5, device="cpu", dtype=torch.float32, xformers=False)
    vae = configs.build_vae(4, device="cpu", dtype=torch.float32)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM")
    pipe.rng, pipe._no_progress = "host", True
    pipe.enable_vae_slicing()
    cache = {}

    def run(frames=4, **kw):
        if frames not in cache:
            cache[frames] = S.video_batch(frames=frames, pano_hw=(128, 256), seed=4), S.conditioning(frames=max(frames, 16), seed=4)
        vb, cond = cache[frames]
        with E.patched_kernels(), ER.patched_rescale_kernels():
            torch.manual_seed(13)
            random.seed(13)
            pipe("synthetic", **_pipe_kw(cond, vb, **kw))
        return [v.clone() for v in pipe.last_latents]
    run.pipe = pipe
    return run


def _hand_written_steps(pipe, phi, eta=0.0):
    """Replace the fused CFG step of ``pipe``'s scheduler by the chain written out: combine, rescale_noise_cfg, scheduler.step."""
    sch = pipe.scheduler

    def step(u, c, g, t, x, coef_dev=None, *, eta=0.0, noise=None, **kw):
        m = rescale_noise_cfg(u + g * (c - u), c, phi)
        extra = dict(eta=eta, variance_noise=noise) if eta > 0 else {}
        return sch.step(m, t, x, **extra).prev_sample
    sch.fused_cfg_step = step


def test_pipeline_guidance_rescale_zero_is_the_call_without_it(cpu_runs):
    base = cpu_runs()
    zero = cpu_runs(guidance_rescale=0.0)
    assert torch.equal(zero[0], base[0]) and torch.equal(zero[1], base[1])


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_pipeline_guidance_rescale_equals_hand_written_loop(cpu_runs, eta):
    """guidance_rescale = 0.7 == per branch u + g (c - u) -> rescale_noise_cfg -> scheduler.step, in fp32 (the bound of
    test_ddim_stochastic.py::test_pipeline_eta1_against_reference for latents after two steps); and it is not the unrescaled run."""
    kw = dict(eta=eta) if eta > 0 else {}
    got = cpu_runs(guidance_rescale=0.7, **kw)
    pipe = cpu_runs.pipe
    _hand_written_steps(pipe, 0.7)
    try:
        want = cpu_runs(**kw)
    finally:
        del pipe.scheduler.fused_cfg_step
    plain = cpu_runs(**kw)
    for a, b, p in zip(got, want, plain):
        assert torch.isfinite(a).all() and rel(a, b) < 1e-4, rel(a, b)
        assert rel(a, p) > 1e-2          # the factor is used


def test_windowed_pipeline_guidance_rescale(cpu_runs):
    """Context windows (F = 12, L = 8, overlap 4): phi = 0 is the call without the keyword; phi = 0.7 is a different clip whose
    update is the windows stand-in with rescale (the routing test covers the arguments)."""
    ctx = dict(frames=12, context_frames=8, context_overlap=4)
    base, zero, on = cpu_runs(**ctx), cpu_runs(guidance_rescale=0.0, **ctx), cpu_runs(guidance_rescale=0.7, **ctx)
    assert torch.equal(zero[0], base[0]) and torch.equal(zero[1], base[1])
    assert all(torch.isfinite(v).all() for v in on) and rel(on[0], base[0]) > 1e-2 and rel(on[1], base[1]) > 1e-2


def test_guidance_rescale_with_frame_shard_is_refused(cpu_runs):
    from imagine360_amd.dist import FrameShard
    with pytest.raises(ValueError, match="guidance_rescale cannot be combined with frame_shard.*all-reduce"):
        cpu_runs(guidance_rescale=0.7, frame_shard=FrameShard(4, rank=0, world=1))
