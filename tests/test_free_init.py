"""FreeInit passes on CPU: the operator ``pano_geometry.free_init_operator`` (rows sum to 1, symmetric, the FFT low-pass on a ring, the
diffusers mask formula for even sizes, mirror-extend / filter / crop for an open axis, its two limits), the definition
``pano_geometry.free_init_noise`` (the identity it is named after, identity operators), the fp32 stand-in against the derived bound the
GPU test holds the kernel to -- and perturbed copies of it outside that bound -- and the pipeline's host logic under emulated kernels:
``free_init_iters=1`` is the call without the keyword, the calls of N = 3 passes and their arguments, the RNG order, the refusals."""
import contextlib
import math
import random

import pytest
import torch

import _emu_ddim_step as ES
import _emu_free_init as EF
import _emu_kernels as E
import _emu_noise_latents as EN
import _emu_ring_step as EG
from imagine360_amd import configs, pano_geometry as G, synthetic as S
from imagine360_amd.scheduler import DDIMScheduler

torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ 1. the operator
def gain(n, d):
    k = torch.fft.fftfreq(n, 1.0 / n, dtype=torch.float64)
    return torch.exp(-(2.0 * k / n) ** 2 / (2.0 * d * d))


@pytest.mark.parametrize("periodic", [True, False])
def test_operator_rows_sum_to_one_and_it_is_symmetric(periodic):
    for n in range(1, 65):
        for d in (0.05, 0.25, 0.4, 4.0):
            L = G.free_init_operator(n, d, periodic)
            assert L.shape == (n, n) and L.dtype == torch.float64
            assert float((L.sum(dim=1) - 1.0).abs().max()) < 1e-13, (n, d)
            assert float((L - L.t()).abs().max()) < 1e-15, (n, d)
    assert torch.equal(G.free_init_operator(1, 0.25, periodic), torch.ones(1, 1, dtype=torch.float64))


@pytest.mark.parametrize("shape", [(16, 8, 16), (5, 7, 9), (4, 3, 6), (1, 6, 5)])
def test_periodic_operators_are_the_fft_low_pass(shape):
    """ifftn(fftn(x) . g_F g_h g_w) in fp64, even and odd sizes; the result of the operators is real by construction."""
    F, h, w = shape
    d_s, d_t = 0.25, 0.4
    g = torch.Generator().manual_seed(1)
    x = torch.randn(F, h, w, generator=g, dtype=torch.float64)
    Lf, Lh, Lw = G.free_init_operator(F, d_t, True), G.free_init_operator(h, d_s, True), G.free_init_operator(w, d_s, True)
    got = torch.einsum("ai,bj,ck,ijk->abc", Lf, Lh, Lw, x)
    mask = gain(F, d_t)[:, None, None] * gain(h, d_s)[None, :, None] * gain(w, d_s)[None, None, :]
    want = torch.fft.ifftn(torch.fft.fftn(x) * mask)
    assert float(want.imag.abs().max()) < 1e-14                            # the symmetric gain keeps a real clip real
    assert float((got - want.real).abs().max()) < 1e-13, shape


def test_even_periodic_operators_are_the_diffusers_mask():
    """diffusers' ``_get_free_init_freq_filter`` (gaussian) + ``_apply_freq_filter`` restated: mask[t, y, x] = exp(-d^2 / (2 d_s^2)),
    d^2 = ((d_s / d_t)(2 t / T - 1))^2 + (2 y / H - 1)^2 + (2 x / W - 1)^2, applied between fftshift and ifftshift."""
    T, H, W = 16, 8, 16
    d_s, d_t = 0.25, 0.4
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T, H, W, generator=g, dtype=torch.float64)
    t, y, xx = torch.meshgrid(torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij")
    d2 = ((d_s / d_t) * (2.0 * t / T - 1)) ** 2 + (2.0 * y / H - 1) ** 2 + (2.0 * xx / W - 1) ** 2
    mask = torch.exp(-d2.double() / (2 * d_s ** 2))
    freq = torch.fft.fftshift(torch.fft.fftn(x), dim=(-3, -2, -1))
    want = torch.fft.ifftn(torch.fft.ifftshift(freq * mask, dim=(-3, -2, -1))).real
    Lf, Lh, Lw = G.free_init_operator(T, d_t, True), G.free_init_operator(H, d_s, True), G.free_init_operator(W, d_s, True)
    got = torch.einsum("ai,bj,ck,ijk->abc", Lf, Lh, Lw, x)
    assert float((got - want).abs().max()) < 1e-14


@pytest.mark.parametrize("n", [1, 2, 3, 8, 13])
def test_mirrored_operator_is_mirror_extend_filter_crop(n):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 5, generator=g, dtype=torch.float64)
    for d in (0.1, 0.25, 1.0):
        ring = torch.cat([x, x.flip(0)])                                   # half-sample mirror: x_0 .. x_{n-1}, x_{n-1} .. x_0
        want = torch.fft.ifft(torch.fft.fft(ring, dim=0) * gain(2 * n, d)[:, None], dim=0).real[:n]
        got = G.free_init_operator(n, d, False) @ x
        assert float((got - want).abs().max()) < 1e-14, (n, d)
    # ... and it is not the periodic one: the last sample does not leak into the first
    if n >= 3:
        assert float((G.free_init_operator(n, 0.25, False) - G.free_init_operator(n, 0.25, True)).abs().max()) > 1e-3


@pytest.mark.parametrize("periodic", [True, False])
def test_operator_limits_and_refusals(periodic):
    for n in (1, 2, 5, 8):
        assert float((G.free_init_operator(n, 1e6, periodic) - torch.eye(n, dtype=torch.float64)).abs().max()) < 1e-10
        assert float((G.free_init_operator(n, 1e-3, periodic) - 1.0 / n).abs().max()) < 1e-15
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="n must be a positive int"):
            G.free_init_operator(bad, 0.25, periodic)
    for bad in (0.0, -0.25, float("nan")):
        with pytest.raises(ValueError, match="must be positive"):
            G.free_init_operator(4, bad, periodic)


# ------------------------------------------------------------------------------------------------ 2. the definition
def test_definition_is_low_pass_of_the_noised_clip_plus_high_pass_of_the_fresh_noise():
    F, h, w = 5, 6, 8
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(1, 4, F, h, w, generator=g, dtype=torch.float64)
    n1, n2 = (torch.randn(1, F, 4, h, w, generator=g, dtype=torch.float64) for _ in range(2))
    sa, sb = 0.3, math.sqrt(1 - 0.09)
    for loop in (False, True):
        Lf, Lh, Lw = G.free_init_operator(F, 0.4, loop), G.free_init_operator(h, 0.25, False), G.free_init_operator(w, 0.25, True)
        n_eff = G.free_init_noise(x0, n1, n2, sa, sb, Lf, Lh, Lw)
        assert n_eff.shape == n1.shape and n_eff.dtype == torch.float64
        xf = x0.permute(0, 2, 1, 3, 4)
        lpf = lambda v: torch.einsum("ai,bj,ck,zinjk->zanbc", Lf, Lh, Lw, v)
        noised = sa * xf + sb * n1
        assert float((sa * xf + sb * n_eff - (n2 + lpf(noised - n2))).abs().max()) < 1e-13
        assert float((sa * xf + sb * n_eff - (lpf(noised) + (n2 - lpf(n2)))).abs().max()) < 1e-13
    eye = lambda n: torch.eye(n, dtype=torch.float64)
    assert torch.equal(G.free_init_noise(x0, n1, n2, sa, sb, eye(F), eye(h), eye(w)), n1)
    x32, a32, b32 = x0.to(torch.bfloat16), n1.float(), n2.float()
    got = G.free_init_noise(x32, a32, b32, sa, sb, eye(F).float(), eye(h).float(), eye(w).float())
    assert got.dtype == torch.float32 and torch.equal(got, a32)
    for bad in (0.0, -0.5):
        with pytest.raises(ValueError, match="sb=.* must be positive"):
            G.free_init_noise(x0, n1, n2, sa, bad, Lf, Lh, Lw)
    with pytest.raises(ValueError, match=r"n1, n2 \[1, F, C, h, w\] expected"):
        G.free_init_noise(x0, n1.permute(0, 2, 1, 3, 4), n2, sa, sb, Lf, Lh, Lw)


# ------------------------------------------------------------------------------------------------ 3. the stand-in and the bound
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_stand_in_is_inside_the_bound(dt):
    worst = {}
    for name, (F, h, w, loop, d_s, d_t) in EF.CASES.items():
        x0, n1, n2, Lf, Lh, Lw = EF.case(name, dt)
        got = EF.free_init_noise(x0, n1, n2, Lf, Lh, Lw, EF.SA, EF.SB)
        assert got.shape == (1, F, EF.C, h, w) and got.dtype == torch.float32
        worst[name] = EF.worst_ratio(got, name, dt)
    print("free_init_noise fp32 evaluation / bound", dt, worst)
    assert max(worst.values()) < 1.0, worst
    # the table of the issue is all there, each shape mirrored in time and at least four also as a ring
    shapes = {v[:3] for v in EF.CASES.values()}
    assert {(2, 3, 5), (3, 4, 8), (1, 4, 8), (4, 1, 8), (16, 2, 8), (2, 64, 8), (2, 2, 128), (70, 2, 8), (5, 130, 8), (2, 2, 300)} <= shapes
    assert all(any(v[:4] == (*s, False) for v in EF.CASES.values()) for s in shapes)
    assert sum(v[3] for v in EF.CASES.values()) >= 4 and EF.D_S != EF.D_T
    assert {v[4] for v in EF.CASES.values()} >= {0.05, 4.0}


def _perturbed(kind, name, dt):
    """A wrong implementation's result on one case, or None where the perturbation cannot change this case."""
    F, h, w, loop, d_s, d_t = EF.CASES[name]
    x0, n1, n2, Lf, Lh, Lw = EF.case(name, dt)
    sa, sb = EF.SA, EF.SB
    if kind == "Lh_Lw_swapped":
        if h != w:
            return None
        return EF.free_init_noise(x0, n1, n2, Lf, Lw, Lh, sa, sb)
    if kind in ("frames_kind", "rows_kind", "cols_kind"):
        kinds = [bool(loop), False, True]
        axis = ("frames_kind", "rows_kind", "cols_kind").index(kind)
        if (F, h, w)[axis] < 2:
            return None                                                     # [[1]] either way
        kinds[axis] = not kinds[axis]
        return EF.free_init_noise(x0, n1, n2, *EF.operators(F, h, w, loop, d_s, d_t, kinds), sa, sb)
    if kind == "n1_n2_swapped":
        return EF.free_init_noise(x0, n2, n1, Lf, Lh, Lw, sa, sb)
    if kind == "sa_off":
        return EF.free_init_noise(x0, n1, n2, Lf, Lh, Lw, sa * 1.005, sb)
    if kind == "no_division":
        y = EF.free_init_noise(x0, n1, n2, Lf, Lh, Lw, sa, sb)
        return n1 + (y - n1) * sb                                           # n1 + (y - d), the 1 / sb forgotten
    if kind == "d_t_for_d_s":
        if h * w == 1 or d_s == d_t:
            return None
        return EF.free_init_noise(x0, n1, n2, *EF.operators(F, h, w, loop, d_t, d_t), sa, sb)
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["Lh_Lw_swapped", "frames_kind", "rows_kind", "cols_kind", "n1_n2_swapped", "sa_off", "no_division",
                                  "d_t_for_d_s"])
def test_perturbed_stand_ins_are_outside_the_bound(kind):
    """Each wrong implementation misses the bound on EVERY case it changes (and changes at least one).  The cases are those at the
    standard cut-offs: at the two extremes the operators are the mean or the identity to rounding whatever their kind or cut-off
    axis, and a swap there changes the last bits only."""
    dt = torch.bfloat16
    ratios = {}
    for name in (n for n, v in EF.CASES.items() if v[4:] == (EF.D_S, EF.D_T)):
        got = _perturbed(kind, name, dt)
        if got is None:
            continue
        x0, n1, n2, Lf, Lh, Lw = EF.case(name, dt)
        if torch.equal(got, EF.free_init_noise(x0, n1, n2, Lf, Lh, Lw, EF.SA, EF.SB)):
            continue
        ratios[name] = EF.worst_ratio(got, name, dt)
    print("perturbed", kind, ratios)
    assert ratios and min(ratios.values()) > 1.0, (kind, ratios)
    if kind != "Lh_Lw_swapped":
        assert len(ratios) >= 8


# ------------------------------------------------------------------------------------------------ 4. the pipeline's host logic
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
def clip6():
    """6 frames at 128 x 256 pixels, a 16 x 32 latent."""
    return S.video_batch(frames=6, pano_hw=(128, 256), seed=6), S.conditioning(frames=16, seed=6)


def pipe_kw(cond, vb, steps, **extra):
    return dict(num_inference_steps=steps, guidance_scale_text=7.5, negative_prompt="", video_batch=vb, use_outpaint=True,
                use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video", latents_dtype=torch.float32,
                prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **extra)


def _run(pipe, seed=3, **kw):
    torch.manual_seed(seed)
    random.seed(seed)
    vid = pipe("synthetic", **kw).videos
    return vid, [v.clone() for v in pipe.last_latents]


@contextlib.contextmanager
def patches():
    """Every emulated kernel; yields (starts, filters): the records of noise_latents and free_init_noise."""
    with contextlib.ExitStack() as st:
        for cm in (E.patched_kernels(), ES.patched_step_kernel(), EG.patched_ring_kernels()):
            st.enter_context(cm)
        yield st.enter_context(EN.patched_noise_latents()), st.enter_context(EF.patched_free_init_noise())


def test_one_pass_is_the_call_without_the_keyword(cpu_pipe, clip6):
    vb, cond = clip6
    with patches() as (starts, filters):
        plain = _run(cpu_pipe, **pipe_kw(cond, vb, 2))
        one = _run(cpu_pipe, **pipe_kw(cond, vb, 2, free_init_iters=1, free_init_d_s=0.1, free_init_d_t=0.9))
        assert starts == [] and filters == []
    assert torch.equal(plain[0], one[0]) and all(torch.equal(a, b) for a, b in zip(plain[1], one[1]))
    assert len(cpu_pipe.free_init_passes) == 1 and torch.equal(cpu_pipe.free_init_passes[0], one[1][0])


@pytest.mark.parametrize("windows", [{}, dict(context_frames=4, context_overlap=2), dict(context_frames=4, context_overlap=2, context_loop=True)],
                         ids=["one_block", "windows", "ring"])
def test_three_passes_make_two_calls_with_the_stated_arguments(cpu_pipe, clip6, windows):
    vb, cond = clip6
    F, h, w = 6, 16, 32
    with patches() as (starts, filters):
        plain = _run(cpu_pipe, **pipe_kw(cond, vb, 2, **windows))
        assert starts == [] and filters == []
        trace = []
        vid, lat = _run(cpu_pipe, **pipe_kw(cond, vb, 2, free_init_iters=3, free_init_d_s=0.3, free_init_d_t=0.45, trace=trace, **windows))
        passes = cpu_pipe.free_init_passes
        assert len(filters) == 2 and len(starts) == 2 and len(passes) == 3 and len(trace) == 6
        # pass 0 is the plain call, the last pass is the result
        assert torch.equal(passes[0], plain[1][0]) and torch.equal(passes[2], lat[0]) and torch.equal(trace[1], passes[0])
        assert vid.shape == plain[0].shape and torch.isfinite(vid).all() and not torch.equal(lat[0], plain[1][0])
        # the fp32 noise of pass 0: the first draw of the call
        torch.manual_seed(3)
        noise1 = torch.randn(1, F, 1, 4, h, w).squeeze(2)
        steps = cpu_pipe.scheduler._timesteps_host
        sa, sb = cpu_pipe.scheduler.noise_coefficients(steps[0])
        loop = bool(windows.get("context_loop"))
        want_ops = [G.free_init_operator(F, 0.45, loop).float(), G.free_init_operator(h, 0.3, False).float(),
                    G.free_init_operator(w, 0.3, True).float()]
        idx, ok = G.nearest_e2p_index(h, w, vb["pers_size"] // 8, vb["pers_size"] // 8, vb["cameras"])
        for k, (x0, n1, n2, Lf, Lh, Lw, a, b, n_eff) in enumerate(filters):
            assert torch.equal(x0, passes[k]) and x0.shape == (1, 4, F, h, w)
            assert n1.dtype == torch.float32 and torch.equal(n1, noise1) and n2.shape == n1.shape and n2.dtype == torch.float32
            assert (a, b) == (sa, sb) and b > 0
            assert all(torch.equal(L, W) for L, W in zip((Lf, Lh, Lw), want_ops))
            # the returned noise is what noise_latents receives, with the clean clip and the tables of pass 0
            want = EN.noise_latents(x0, n_eff, idx.to(torch.int32), ok.to(torch.uint8), sa, sb)
            assert torch.equal(starts[k][0], want[0]) and torch.equal(starts[k][1], want[1])
        assert not torch.equal(filters[0][2], filters[1][2]) and not torch.equal(filters[0][2], noise1)
        assert loop == (not torch.equal(want_ops[0], G.free_init_operator(F, 0.45, False).float()))
        n2_first = filters[0][2]
        # the RNG order: the fresh noise is the first draw behind the last step of the pass before it
        del filters[:], starts[:]
        state = {}

        def after_pass(i, t, latent):
            if i == 1 and "rng" not in state:
                state["rng"] = torch.get_rng_state()
        _run(cpu_pipe, **pipe_kw(cond, vb, 2, free_init_iters=2, free_init_d_s=0.3, free_init_d_t=0.45, callback=after_pass, **windows))
        torch.set_rng_state(state["rng"])
        assert torch.equal(filters[0][2], torch.randn(1, F, 1, 4, h, w).squeeze(2)) and torch.equal(filters[0][2], n2_first)


def test_refusals(cpu_pipe, clip6):
    from imagine360_amd.dist import FrameShard
    vb, cond = clip6
    x0 = torch.zeros(1, 4, 6, 16, 32)
    with patches() as (starts, filters):
        for bad in (0, -1, 2.0, True, None):
            with pytest.raises(ValueError, match="free_init_iters counts the passes in total"):
                cpu_pipe("synthetic", **pipe_kw(cond, vb, 2, free_init_iters=bad))
        for extra in (dict(init_latents=x0, strength=0.5), dict(init_latents=x0), dict(init_video=torch.zeros(1, 6, 3, 128, 256)),
                      dict(strength=0.5), dict(init_latents=x0, strength=0.5, regenerate_mask=vb["pano_mask"])):
            with pytest.raises(ValueError, match="free_init_iters > 1 cannot be combined with init_latents.*pure noise"):
                cpu_pipe("synthetic", **pipe_kw(cond, vb, 2, free_init_iters=2, **extra))
        with pytest.raises(ValueError, match="free_init_iters > 1 cannot be combined with frame_shard.*not implemented"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, 2, free_init_iters=2, frame_shard=FrameShard(6, rank=0, world=1)))
        for extra in (dict(free_init_d_s=0.0), dict(free_init_d_t=-1.0)):
            with pytest.raises(ValueError, match="must be positive"):
                cpu_pipe("synthetic", **pipe_kw(cond, vb, 2, free_init_iters=2, **extra))
        assert starts == [] and filters == []
