"""Starting the denoising from a given clip on the MI355X: ``kernels.noise_latents`` (csrc/noise_latents.hip) against the fp64
composition add_noise -> gather -> mask on every path of its launcher, the same cases between guard bands, the refusals of the wrapper
and of the C entry point, and the small pipeline with ``init_latents`` / ``strength``: graph replay against the eager loop, plain and
over looping context windows with eta > 0 and guidance rescale."""
import functools
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from _emu_noise_latents import TOL, fp64_composition, gathered, noise_case, same_bits  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record as _record, rel  # noqa: E402
from imagine360_amd import configs, kernels as K, synthetic as S  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler  # noqa: E402

torch.set_grad_enabled(False)

LDS_PLANE = 32768          # elements of the largest plane the kernel keeps in LDS (64 KiB; kPlaneLdsBytes of csrc/latent_plane.h)

# (F, C, h, w, M, ph, pw), byte offset of x0 from its alignment: one case on each side of every choice the launcher makes
CASES = {
    "scalar_hw60": ((3, 4, 5, 12, 3, 4, 6), 0),                      # HW = 60: not a multiple of 8 -> scalar lanes, plane in LDS
    "vector_hw192": ((3, 4, 8, 24, 3, 4, 6), 0),                     # HW = 192, Q = 24: 16-byte lanes (24 and 9 of a 256-thread block busy)
    "scalar_q15": ((2, 4, 8, 24, 2, 3, 5), 0),                       # HW % 8 == 0 but Q = 15 -> scalar lanes
    "scalar_misaligned_x0": ((3, 4, 8, 24, 3, 4, 6), 2),             # vector sizes, x0 off its 16 bytes -> scalar lanes
    "lds_budget_exact": ((1, 1, 128, 256, 1, 2, 4), 0),              # 2 * HW = 64 KiB: the largest plane in LDS
    "global_vector": ((1, 1, 1, LDS_PLANE + 8, 1, 2, 4), 0),         # the smallest plane above the budget with 16-byte lanes
    "global_scalar": ((1, 1, 1, LDS_PLANE + 1, 1, 2, 4), 0),         # the smallest plane above the budget: recomputed gathers, scalar
}


def _sched():
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    return sch


@functools.lru_cache(maxsize=None)
def case(name, dt):
    """Host inputs, coefficients and the fp64 reference of one case (computed once, never written to)."""
    shape, _ = CASES[name]
    sch = _sched()
    t = sch.timesteps_for_strength(0.5)[1][0]
    inputs = noise_case(*shape, dt, seed=11 + len(name))
    return inputs, sch.noise_coefficients(t), fp64_composition(sch, t, *inputs)


def off_alignment(t, nbytes):
    """A contiguous copy of ``t`` that starts ``nbytes`` past a 256-byte aligned address."""
    n, k = t.numel(), nbytes // t.element_size()
    buf = torch.empty(n + k, dtype=t.dtype, device=t.device)
    view = buf[k:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == nbytes % 16
    return view


def check_case(name, dt, pano, pers):
    (x0, noise, idx, ok), _, (want_pano, want_pers) = case(name, dt)
    F, C, h, w, M, ph, pw = CASES[name][0]
    assert pano.shape == (1, C, F, h, w) and pers.shape == (1, M, C, F, ph, pw) and pano.dtype == pers.dtype == dt
    errs = dict(pano=rel(pano, want_pano), pers=rel(pers, want_pers))
    print("noise_latents", name, dt, errs, flush=True)
    assert errs["pano"] < TOL[dt] and errs["pers"] < TOL[dt], (name, errs)
    assert same_bits(pers.cpu(), gathered(pano.cpu(), idx, ok)), name          # the contract: the gather of the rounded panorama start
    zero = pers.cpu().permute(0, 2, 3, 1, 4, 5)[..., ok == 0]
    assert zero.numel() > 0 and (zero.view(torch.int16) == 0).all(), name     # +0 where a view sees nothing
    assert torch.isfinite(pano.float()).all() and torch.isfinite(pers.float()).all()
    return errs


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_noise_latents_parity(dt):
    errs = {}
    for name, (_, mis) in CASES.items():
        (x0, noise, idx, ok), (sa, sb), _ = case(name, dt)
        dx0 = off_alignment(x0.cuda(), mis) if mis else x0.cuda()
        pano, pers = K.noise_latents(dx0, noise.cuda(), idx.cuda(), ok.cuda(), sa, sb)
        e = check_case(name, dt, pano, pers)
        errs[name] = max(e.values())
    # scalar lanes on vector sizes round like the 16-byte lanes: one expression, one rounding
    (x0, noise, idx, ok), (sa, sb), _ = case("vector_hw192", dt)
    a = K.noise_latents(x0.cuda(), noise.cuda(), idx.cuda(), ok.cuda(), sa, sb)
    b = K.noise_latents(off_alignment(x0.cuda(), 2), noise.cuda(), idx.cuda(), ok.cuda(), sa, sb)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    _record(f"noise_latents_{str(dt).split('.')[-1]}", max_rel=max(errs.values()), **errs)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(CASES))
def test_noise_latents_between_guard_bands(name, dt):
    """Inputs, tables and both results between poisoned guards: nothing written outside, every element of both results written
    (no sentinel left), zeros where ``ok`` is 0."""
    (x0, noise, idx, ok), (sa, sb), _ = case(name, dt)
    g = Guarded(K)
    args = (g.guard(x0.cuda(), misalign=CASES[name][1]), g.guard(noise.cuda()), g.guard(idx.cuda()), g.guard(ok.cuda()))
    with g:
        pano, pers = g.out(*K.noise_latents(*args, sa, sb))
    check_case(name, dt, pano, pers)


def test_noise_latents_rejects_bad_arguments():
    (x0, noise, idx, ok), (sa, sb), _ = case("vector_hw192", torch.bfloat16)
    x0, noise, idx, ok = x0.cuda(), noise.cuda(), idx.cuda(), ok.cuda()
    with pytest.raises(TypeError, match="bfloat16/float16"):
        K.noise_latents(x0.float(), noise, idx, ok, sa, sb)
    with pytest.raises(TypeError, match="noise must be float32"):
        K.noise_latents(x0, noise.to(torch.bfloat16), idx, ok, sa, sb)
    with pytest.raises(TypeError, match="idx must be int32"):
        K.noise_latents(x0, noise, idx.long(), ok, sa, sb)
    with pytest.raises(ValueError, match="noise must be"):
        K.noise_latents(x0, noise.permute(0, 2, 1, 3, 4).contiguous()[:, :, :2], idx, ok, sa, sb)
    with pytest.raises(ValueError, match="contiguous"):
        K.noise_latents(x0, noise, idx.transpose(1, 2).contiguous().transpose(1, 2), ok, sa, sb)
    with pytest.raises(ValueError, match="one \\[M, ph, pw\\]"):
        K.noise_latents(x0, noise, idx, ok[:1], sa, sb)
    # the C entry point itself
    F, C, h, w, M, ph, pw = CASES["vector_hw192"][0]
    pano, pers = torch.empty_like(x0), torch.empty(1, M, C, F, ph, pw, dtype=x0.dtype, device="cuda")
    ptrs = [t.data_ptr() for t in (x0, noise, idx, ok, pano, pers)]
    sizes = [F, C, h * w, M, ph * pw]
    fn, err = K.lib().im360_noise_latents, K.lib().im360_last_error
    for i in range(6):
        bad = list(ptrs)
        bad[i] = None
        assert fn(*bad, *sizes, sa, sb, 0, None) != 0 and b"null pointer" in err(), i
    for i in range(5):
        for v in (0, -3):
            bad = list(sizes)
            bad[i] = v
            assert fn(*ptrs, *bad, sa, sb, 0, None) != 0 and b"must be positive" in err(), (i, v)
    assert fn(*ptrs, *sizes, sa, sb, 7, None) != 0 and b"dtype 7 unsupported" in err()
    assert fn(*ptrs, F, C, 1 << 31, M, ph * pw, sa, sb, 0, None) != 0 and b"2^31" in err()
    assert fn(*ptrs, 1 << 16, 1 << 15, h * w, M, ph * pw, sa, sb, 0, None) != 0 and b"2^31" in err()
    assert fn(*ptrs, F, C, h * w, 1 << 16, 1 << 15, sa, sb, 0, None) != 0 and b"2^31" in err()
    bad = list(ptrs)
    bad[1] += 2
    assert fn(*bad, *sizes, sa, sb, 0, None) != 0 and b"misaligned noise" in err()
    torch.cuda.synchronize()
    assert fn(*ptrs, *sizes, sa, sb, 0, None) == 0             # and the same arguments unbroken are accepted
    torch.cuda.synchronize()
    assert same_bits(pano, K.noise_latents(x0, noise, idx, ok, sa, sb)[0])


# ------------------------------------------------------------------------------------------------ the small pipeline
@pytest.fixture(scope="module")
def small_pipe():
    """The recipe of test_ddim_stochastic_gpu.py::small_pipe: 8 frames, 256 x 512, width-5 model, 3 steps."""
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
                   latents_dtype=dt, prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]),
                   **kw).videos
        return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone()
    return run


@pytest.fixture(scope="module")
def first_call(small_pipe):
    return small_pipe(True)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_refinement_pass_graph_equals_eager_bit_for_bit(small_pipe, first_call, monkeypatch):
    from imagine360_amd import graph_step
    replays = []
    orig = graph_step.GraphedDenoiseStep.step
    monkeypatch.setattr(graph_step.GraphedDenoiseStep, "step", lambda self, t: (replays.append(t), orig(self, t))[1])
    x0 = first_call[1]
    graphed = small_pipe(True, init_latents=x0, strength=2 / 3)
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(3)
    assert replays == sch._timesteps_host[1:]               # two replays, at the last two timesteps
    trace = []
    eager = small_pipe(False, init_latents=x0, strength=2 / 3, trace=trace)
    assert len(replays) == 2 and len(trace) == 2
    errs = dict(graph_vs_eager_latent=rel(graphed[1], eager[1]), refined_vs_first_latent=rel(graphed[1], first_call[1]),
                refined_vs_first_video=rel(graphed[0], first_call[0]))
    _record("init_strength_refinement", **errs)
    assert _same(graphed, eager), errs
    assert torch.equal(trace[-1], eager[1])
    assert graphed[0].shape == first_call[0].shape and torch.isfinite(graphed[0]).all()
    assert all(torch.isfinite(v.float()).all() for v in graphed)
    assert not torch.equal(graphed[0], first_call[0]) and not torch.equal(graphed[1], first_call[1])


def test_refinement_over_looping_windows_graph_equals_eager(small_pipe, first_call):
    """Windows of 4 frames with overlap 2 on a ring, guidance rescale 0.7, eta = 0.5 from a seeded device generator."""
    x0 = first_call[1]
    cuda_gen = lambda s: torch.Generator(device="cuda").manual_seed(s)
    kw = dict(init_latents=x0, strength=2 / 3, context_frames=4, context_overlap=2, context_loop=True, guidance_rescale=0.7, eta=0.5)
    graphed = small_pipe(True, generator=cuda_gen(77), **kw)
    eager = small_pipe(False, generator=cuda_gen(77), **kw)
    errs = dict(graph_vs_eager_latent=rel(graphed[1], eager[1]), windows_vs_first_latent=rel(graphed[1], first_call[1]))
    _record("init_strength_ring_windows", **errs)
    assert _same(graphed, eager), errs
    assert all(torch.isfinite(v.float()).all() for v in graphed)


def test_a_call_without_an_init_afterwards_is_the_first_call(small_pipe, first_call):
    """No state leaks from the runs with an init (this file's order: after them) into a run from pure noise."""
    assert _same(small_pipe(True), first_call)
