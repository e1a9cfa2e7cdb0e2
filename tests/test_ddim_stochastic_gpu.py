"""Stochastic DDIM sampling on the MI355X: the fused CFG + DDIM step kernel (cfg_ddim_step_kernel) against an fp64 host
restatement for every mode, the eta = 1 pipeline against the REAL reference's fixture, and the captured hipGraph step
against the eager loop with the variance noise drawn inside the graph."""
import ctypes
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import gold, record as _record, rel  # noqa: E402
from imagine360_amd import configs, kernels as K, synthetic as S  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler  # noqa: E402

torch.set_grad_enabled(False)
TOL = {torch.bfloat16: 1e-2, torch.float16: 3e-3}          # as test_kernels_gpu.py::test_circular_pad_and_cfg_ddim


def _host_step(u, c, x, z, mode, coefs):
    """fp64 restatement of DDIMScheduler.step on the CFG combination (scheduling_ddim.py:300-368)."""
    g, sa, sb, sap, direction, sigma = coefs
    u, c, x = u.double(), c.double(), x.double()
    m = u + g * (c - u)
    pred = mode & 3
    if pred == 0:
        x0, e = (x - sb * m) / sa, m
    elif pred == 1:
        x0, e = sa * x - sb * m, sa * m + sb * x
    else:
        x0, e = m, m
    if mode & 4:
        x0 = x0.clamp(-1, 1)
    if mode & 8:
        e = (x - sa * x0) / sb
    out = sap * x0 + direction * e
    return out if z is None else out + sigma * z.double()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_cfg_ddim_step_kernel_all_modes(dt):
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    t = sch._timesteps_host[8]
    gen = torch.Generator().manual_seed(51)
    shape = (1, 4, 5, 7, 24)                 # 3360 elements: 420 lanes of 8, not a multiple of the 256-thread block
    u, c, x, z = (torch.randn(shape, generator=gen).to(dt) for _ in range(4))
    u, c = u * 0.25, c * 0.25                # a guided x0 partly inside, partly outside [-1, 1]
    dev = [v.cuda() for v in (u, c, x, z)]
    errs = {}
    for eta in (0.0, 0.8):
        coefs = sch.step_coefficients(t, eta, 7.5)
        for pred in (0, 1, 2):
            for extra in (0, 4, 8, 12):
                mode = pred | extra
                noise = dev[3] if eta > 0 else None
                ref = _host_step(u, c, x, z if eta > 0 else None, mode, coefs)
                out = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs)
                assert out.dtype == dt and out.shape == shape
                errs[f"eta{eta}_mode{mode}"] = e = rel(out, ref)
                assert e < TOL[dt], (eta, mode, e)
                coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
                out2 = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, (0.0,) * 6, coef_dev=coef_dev)
                assert torch.equal(out2, out), (eta, mode)           # same fp32 values, same arithmetic
    # grid-stride tail: more lanes than the 4096-block grid covers
    n8 = 4096 * 256 + 300
    big = [torch.randn(n8 * 8, generator=gen).to(dt) for _ in range(4)]
    coefs = sch.step_coefficients(t, 1.0, 7.5)
    out = K.cfg_ddim_step(*(v.cuda() for v in big), 1 | 4, coefs)
    errs["grid_stride"] = e = rel(out, _host_step(*big, 1 | 4, coefs))
    assert e < TOL[dt] and torch.isfinite(out.float()).all()
    _record(f"cfg_ddim_step_{str(dt).split('.')[-1]}", max_rel=max(errs.values()))


def test_cfg_ddim_step_rejects_bad_arguments():
    a = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    coefs = (7.5, 0.5, 0.8, 0.6, 0.7, 0.1)
    with pytest.raises(ValueError, match="noise"):
        K.cfg_ddim_step(a, a, a, None, 1, coefs)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        K.cfg_ddim_step(a[:12], a[:12], a[:12], a[:12], 1, coefs)
    with pytest.raises(RuntimeError, match="misaligned"):
        K.cfg_ddim_step(a[1:9], a[1:9], a[1:9], a[1:9], 1, coefs)
    with pytest.raises(RuntimeError, match="mode 3 unsupported"):
        K.cfg_ddim_step(a, a, a, a, 3, coefs)
    with pytest.raises(TypeError):
        K.cfg_ddim_step(a.float(), a.float(), a.float(), a.float(), 1, coefs)
    # the C entry point itself: a null noise with sigma > 0 and scalar coefficients, an unknown dtype
    p = a.data_ptr()
    rc = K.lib().im360_cfg_ddim_step(p, p, p, None, p, 16, *coefs, 1, 0, None, None)
    assert rc != 0 and b"needs a noise tensor" in K.lib().im360_last_error()
    rc = K.lib().im360_cfg_ddim_step(p, p, p, p, p, 16, *coefs, 1, 7, None, None)
    assert rc != 0 and b"dtype 7 unsupported" in K.lib().im360_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt,tol", [(torch.bfloat16, 1e-1), (torch.float16, 3e-2)])
def test_pipeline_eta1_vs_reference_fixture(dt, tol):
    """Two stochastic DDIM steps (eta = 1.0) + VAE decode on the GPU with host RNG against the REAL reference's eta = 1.0
    run for the same seeds (bounds of test_model_gpu.py::test_pipeline_vs_reference_fixture)."""
    from imagine360_amd.pipeline import AnimationPipeline
    dev = torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=False)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
    pipe.rng, pipe._no_progress = "host", True
    vb = S.video_batch(frames=16, pano_hw=(256, 512), seed=0)
    cond = S.conditioning(frames=16, seed=0)
    g = gold("pipeline_eta_w5.npz")
    trace = []
    torch.manual_seed(21)
    random.seed(21)
    vid = pipe("synthetic", num_inference_steps=2, guidance_scale_text=7.5, negative_prompt="", eta=1.0, latents_dtype=dt,
               video_batch=vb, use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True,
               ip_plus_condition="video", prompt_embeds=(cond["text_pano"], cond["text_pers"]),
               sam_features=(cond["sam_pano"], cond["sam_pers"]), trace=trace).videos
    assert vid.shape == (1, 3, 16, 256, 512) and vid.dtype == torch.float32 and torch.isfinite(vid).all()
    errs = {f"latent_step_{i}": rel(t, g[f"pano_latent_{i}"]) for i, t in enumerate(trace)}
    errs["video"] = rel(vid[:, :, ::3, ::4, ::4], g["video_sub"])
    _record(f"pipeline_eta1_2_steps_w5_{str(dt).split('.')[-1]}", **errs)
    assert len(trace) == 2 and max(errs.values()) < tol, errs


@pytest.fixture(scope="module")
def small_pipe():
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    vb = S.video_batch(frames=8, pano_hw=(256, 512), seed=2)
    cond = S.conditioning(frames=16, seed=2)

    def run(use_graph, seed=33, **kw):
        pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
        pipe._no_progress, pipe.use_graph = True, use_graph
        torch.manual_seed(seed)
        random.seed(seed)
        vid = pipe("synthetic", num_inference_steps=3, guidance_scale_text=7.5, negative_prompt="", video_batch=vb,
                   use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video",
                   prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **kw).videos
        return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone()
    return run


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_graphed_stochastic_steps_equal_eager_bit_for_bit(small_pipe, monkeypatch):
    """eta = 1.0 with device RNG: the captured step (variance noises drawn inside the graph, panorama then perspective,
    after the IP-adapter noise) replays exactly the eager loop's numbers, from the global CUDA generator and from a seeded
    user generator; building the graph consumes no randomness of either."""
    from imagine360_amd import graph_step
    replays = []
    orig = graph_step.GraphedDenoiseStep.step
    monkeypatch.setattr(graph_step.GraphedDenoiseStep, "step", lambda self, t: (replays.append(t), orig(self, t))[1])
    cuda_gen = lambda s: torch.Generator(device="cuda").manual_seed(s)
    errs = {}
    g_none = small_pipe(True, eta=1.0)
    assert len(replays) == 3
    e_none = small_pipe(False, eta=1.0)
    assert len(replays) == 3
    errs["global_generator_latent"] = rel(g_none[1], e_none[1])
    g_user = small_pipe(True, eta=1.0, generator=cuda_gen(77))
    assert len(replays) == 6
    e_user = small_pipe(False, eta=1.0, generator=cuda_gen(77))
    errs["user_generator_latent"] = rel(g_user[1], e_user[1])
    g_again = small_pipe(True, eta=1.0, generator=cuda_gen(77))
    g_other = small_pipe(True, eta=1.0, generator=cuda_gen(78))
    errs["other_seed_latent"] = rel(g_other[1], g_user[1])
    errs["user_vs_global_latent"] = rel(g_user[1], g_none[1])
    _record("graphed_vs_eager_eta1", **errs)
    assert _same(g_none, e_none), errs
    assert _same(g_user, e_user), errs
    assert _same(g_again, g_user)
    assert errs["other_seed_latent"] > 1e-2 and errs["user_vs_global_latent"] > 1e-2, errs
    assert all(torch.isfinite(v.float()).all() for v in g_user)


def test_eta0_pipeline_unchanged(small_pipe):
    """Guard: passing eta = 0.0 is the call without eta, bit for bit (same kernel, same graph)."""
    assert _same(small_pipe(True), small_pipe(True, eta=0.0))
