"""Stochastic DDIM sampling (eta > 0) on CPU: DDIMScheduler.step against the REAL reference's scheduler over its whole
contract (tests/golden/ddim_full.npz), the fused CFG + step path with the kernel emulated in torch, the pipeline with
eta = 1.0 against the reference pipeline (tests/golden/pipeline_eta_w5.npz) and its frame-sharded run.  Fixtures:
tools/gen_ddim_goldens.py."""
import random

import pytest
import torch

import _emu_ddim_step as ES
import _emu_kernels as E
from helpers import gold, rel
from imagine360_amd import configs, synthetic as S
from imagine360_amd.scheduler import DDIMScheduler

torch.set_grad_enabled(False)

# must match tools/gen_ddim_goldens.py
DDIM_CONFIGS = {
    "yaml": dict(configs.NOISE_SCHEDULER_KWARGS),
    "default": {},
    "sample": dict(prediction_type="sample"),
    "scaled": dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012, set_alpha_to_one=False,
                   steps_offset=1, clip_sample=False),
    "cos": dict(beta_schedule="squaredcos_cap_v2"),
}
DDIM_IDX = (0, 12, 24)
DDIM_CASES = [(0.0, False, "vn"), (0.0, True, "vn"), (0.5, False, "vn"), (0.5, True, "vn"), (1.0, False, "vn"),
              (1.0, True, "vn"), (1.0, False, "gen")]
GEN_SEED = 1234


def _key(cfg, idx, eta, clipped, src):
    return f"{cfg}_i{idx}_e{int(eta * 10)}_c{int(clipped)}_{src}"


@pytest.fixture(scope="module")
def ddim_gold():
    return gold("ddim_full.npz")


@pytest.mark.parametrize("cfg", list(DDIM_CONFIGS))
def test_step_matches_reference_scheduler(ddim_gold, cfg):
    g = ddim_gold
    x, v, noise = g["x"], g["model_output"], g["noise"]
    sch = DDIMScheduler(**DDIM_CONFIGS[cfg])
    assert torch.equal(sch.alphas_cumprod, g[f"{cfg}_alphas_cumprod"])
    sch.set_timesteps(25)
    assert torch.equal(sch.timesteps, g[f"{cfg}_timesteps"])
    for idx in DDIM_IDX:
        t = sch.timesteps[idx]
        for eta, clipped, src in DDIM_CASES:
            extra = dict(variance_noise=noise) if src == "vn" else dict(generator=torch.Generator().manual_seed(GEN_SEED))
            o = sch.step(v, t, x, eta=eta, use_clipped_model_output=clipped, **extra)
            k = _key(cfg, idx, eta, clipped, src)
            assert rel(o.prev_sample, g[k + "_prev"]) < 1e-5, k
            assert rel(o.pred_original_sample, g[f"{cfg}_i{idx}_x0"]) < 1e-5, k
            assert torch.isfinite(o.prev_sample).all(), k
        # the generator path draws the noise variance_noise would give: same as passing the seeded draw explicitly
        z = torch.randn(x.shape, generator=torch.Generator().manual_seed(GEN_SEED))
        a = sch.step(v, t, x, eta=1.0, generator=torch.Generator().manual_seed(GEN_SEED)).prev_sample
        assert torch.equal(a, sch.step(v, t, x, eta=1.0, variance_noise=z).prev_sample)
        # tuple form
        assert torch.equal(sch.step(v, t, x, eta=1.0, variance_noise=z, return_dict=False)[0], a)
    with pytest.raises(ValueError, match="generator and variance_noise"):
        sch.step(v, sch.timesteps[0], x, eta=1.0, generator=torch.Generator(), variance_noise=noise)


def test_step_defaults_and_quirks():
    """The constructor's defaults (clip_sample=True) step out of the box; the "sample" direction term multiplies x0 itself;
    a negative radicand (eta > 1) gives NaN like torch.sqrt in the reference, never a Python complex number."""
    gen = torch.Generator().manual_seed(3)
    x, v = torch.randn(2, 4, 8, generator=gen), torch.randn(2, 4, 8, generator=gen)
    sch = DDIMScheduler()
    sch.set_timesteps(10)
    t = int(sch.timesteps[2])
    out = sch.step(v, t, x)
    assert torch.isfinite(out.prev_sample).all() and out.pred_original_sample.abs().max() <= 1.0
    smp = DDIMScheduler(prediction_type="sample", clip_sample=False)
    smp.set_timesteps(10)
    a_t, a_prev = smp._alphas(t)
    assert torch.allclose(smp.step(v, t, x).prev_sample, (a_prev ** 0.5 + (1 - a_prev) ** 0.5) * v, atol=1e-6)
    coefs = sch.step_coefficients(t, eta=50.0)
    assert all(isinstance(c, float) for c in coefs) and coefs[4] != coefs[4]          # dir = sqrt(negative) = NaN
    assert torch.isnan(sch.step(v, t, x, eta=50.0, variance_noise=torch.zeros_like(x)).prev_sample).all()
    # eta < 0: the reference adds no noise (only eta > 0 does) but still uses sigma^2 in the direction term
    neg = sch.step_coefficients(t, eta=-0.5)
    assert neg[5] == 0.0 and neg[4] == sch.step_coefficients(t, eta=0.5)[4]
    assert torch.equal(sch.step(v, t, x, eta=-0.5).prev_sample, sch.step(v, t, x, eta=-0.5, variance_noise=x).prev_sample)
    with pytest.raises(ValueError):
        DDIMScheduler(prediction_type="bogus").kernel_mode()


@pytest.mark.parametrize("cfg", list(DDIM_CONFIGS))
def test_fused_step_equals_guidance_then_step(ddim_gold, cfg):
    """fused_cfg_step(eta, noise) through the kernel's formulas (tests/_emu_ddim_step.py) == step(u + g (c - u)) with the
    same noise, for every configuration, eta and clipped-output setting."""
    gen = torch.Generator().manual_seed(8)
    x = ddim_gold["x"]
    u, c = torch.randn(x.shape, generator=gen) * 0.3, torch.randn(x.shape, generator=gen) * 0.3
    z = torch.randn(x.shape, generator=gen)
    sch = DDIMScheduler(**DDIM_CONFIGS[cfg])
    sch.set_timesteps(25)
    with E.patched_kernels(), ES.patched_step_kernel():
        for t in sch._timesteps_host[::6]:
            for eta in (0.0, 0.5, 1.0):
                for clipped in (False, True):
                    got = sch.fused_cfg_step(u, c, 7.5, t, x, eta=eta, noise=z, use_clipped_model_output=clipped)
                    want = sch.step(u + 7.5 * (c - u), t, x, eta=eta, variance_noise=z, use_clipped_model_output=clipped).prev_sample
                    assert rel(got, want) < 1e-5, (cfg, t, eta, clipped)
        with pytest.raises(ValueError, match="variance noise"):
            sch.fused_cfg_step(u, c, 7.5, sch._timesteps_host[0], x, eta=1.0)


def test_default_update_stays_on_the_eta0_kernel():
    """eta = 0 with the pipeline's configuration dispatches to cfg_ddim_update with the same arguments as before; anything
    else to cfg_ddim_step with the mode bits of the configuration."""
    from imagine360_amd import kernels
    calls = []
    saved = kernels.cfg_ddim_update, kernels.cfg_ddim_step
    kernels.cfg_ddim_update = lambda *a, **k: calls.append(("update", a[3:], k))
    kernels.cfg_ddim_step = lambda *a, **k: calls.append(("step", a[3:], k))
    try:
        x = torch.zeros(8)
        sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
        sch.set_timesteps(25)
        t = sch._timesteps_host[3]
        sch.fused_cfg_step(x, x, 7.5, t, x)
        sch.fused_cfg_step(x, x, 7.5, t, x, eta=0.0)
        sch.fused_cfg_step(x, x, 7.5, None, x, coef_dev=x[:3])
        sch.fused_cfg_step(x, x, 7.5, t, x, eta=1.0, noise=x)
        sch.fused_cfg_step(x, x, 7.5, t, x, use_clipped_model_output=True)
        d = DDIMScheduler()
        d.set_timesteps(25)
        d.fused_cfg_step(x, x, 7.5, t, x)
    finally:
        kernels.cfg_ddim_update, kernels.cfg_ddim_step = saved
    cx, cv = sch.coefficients(t)
    assert calls[0] == calls[1] == ("update", (7.5, cx, cv), {"coef_dev": None})
    assert calls[2][0] == "update" and calls[2][1] == (7.5, 0.0, 0.0)
    assert calls[3][0] == "step" and calls[3][1][1] == 1 and calls[3][1][2] == sch.step_coefficients(t, 1.0, 7.5)
    assert calls[4][0] == "step" and calls[4][1][0] is None and calls[4][1][1] == 1 | 8
    assert calls[5][0] == "step" and calls[5][1][1] == 0 | 4


def _pipe_kw(cond, vb, **extra):
    return dict(num_inference_steps=2, guidance_scale_text=7.5, negative_prompt="", latents_dtype=torch.float32,
                video_batch=vb, use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True,
                ip_plus_condition="video", prompt_embeds=(cond["text_pano"], cond["text_pers"]),
                sam_features=(cond["sam_pano"], cond["sam_pers"]), **extra)


def test_pipeline_eta1_against_reference():
    """AnimationPipeline(eta=1.0) with host RNG and emulated kernels against the reference pipeline with eta = 1.0 for the
    same seeds: the variance noises are drawn after the model's IP-adapter noise, panorama first (bounds of
    test_host_logic.py::test_pipeline_against_reference)."""
    from imagine360_amd.pipeline import AnimationPipeline
    g = gold("pipeline_eta_w5.npz")
    mv = configs.build_mv_model(5, device="cpu", dtype=torch.float32, xformers=False)
    vae = configs.build_vae(4, device="cpu", dtype=torch.float32)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM")
    pipe.rng, pipe._no_progress = "host", True
    pipe.enable_vae_slicing()
    vb = S.video_batch(frames=16, pano_hw=(256, 512), seed=0)
    cond = S.conditioning(frames=16, seed=0)
    trace = []
    with E.patched_kernels(), ES.patched_step_kernel():
        torch.manual_seed(21)
        random.seed(21)
        vid = pipe("synthetic", eta=1.0, trace=trace, **_pipe_kw(cond, vb)).videos
    assert len(trace) == 2
    for i, t in enumerate(trace):
        assert rel(t, g[f"pano_latent_{i}"]) < 1e-4, i
    assert rel(vid[:, :, ::3, ::4, ::4], g["video_sub"]) < 1e-3
    st = torch.stack([vid.mean(dim=(0, 1, 3, 4)), vid.std(dim=(0, 1, 3, 4))])
    assert rel(st, g["video_frame_stats"]) < 1e-4


def _sharded_eta_job(rank, world):
    import _emu_ddim_step as ES
    import _emu_kernels as E
    from imagine360_amd import configs, synthetic as S
    from imagine360_amd.dist import FrameShard
    from imagine360_amd.pipeline import AnimationPipeline
    from imagine360_amd.scheduler import DDIMScheduler
    mv = configs.build_mv_model(10, device="cpu", dtype=torch.float32, xformers=True, motion_heads=4)
    vae = configs.build_vae(4, device="cpu", dtype=torch.float32)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM")
    pipe.rng, pipe._no_progress, pipe.use_graph = "host", True, False
    frames = 4
    vb = S.video_batch(frames=frames, pano_hw=(128, 256), seed=3)
    cond = S.conditioning(frames=16, seed=3)
    out = {}
    with E.patched_kernels(), ES.patched_step_kernel():
        for name, eta, sh in (("full", 1.0, None), ("part", 1.0, FrameShard(frames)), ("eta0", 0.0, None)):
            torch.manual_seed(9)
            random.seed(9)
            vid = pipe("synthetic", eta=eta, frame_shard=sh, **_pipe_kw(cond, vb)).videos
            out[name] = (vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone())
    r = lambda a, b: float((a - b).norm() / b.norm())
    f, p, z = out["full"], out["part"], out["eta0"]
    return [r(p[0], f[0]), r(p[1], f[1]), r(p[2], f[2]), r(z[1], f[1]), r(z[2], f[2])]


def test_frame_sharded_eta1_pipeline_matches_unsharded():
    """gloo, world size 2: the frame-sharded eta = 1 pipeline draws the whole clip's variance noise and cuts it like the
    initial noise, so it equals the unsharded eta = 1 run; both differ clearly from the eta = 0 run (the noise is used)."""
    from test_dist_cpu import _run
    out = _run(_sharded_eta_job)
    for r in range(2):
        assert max(out[r][:3]) <= 1e-5, out[r]
        assert min(out[r][3:]) > 1e-2, out[r]
