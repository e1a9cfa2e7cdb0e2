"""Regenerating part of a given clip on the MI355X: ``kernels.keep_latents`` (csrc/keep_latents.hip) against the fp64 composition
add_noise -> gather -> blend on every path of its launcher, its exact ends against the input bits and against ``kernels.noise_latents``,
the same cases between guard bands, the refusals of the wrapper and of the C entry point, and the small pipeline with
``regenerate_mask``: an all-1, an all-0 and a half mask, graph replay against the eager loop, plain and over looping context windows."""
import functools
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from _emu_keep_latents import fp64_composition, half_mask, keep_case, kept, mask_at_views  # noqa: E402
from _emu_noise_latents import TOL, gathered, same_bits  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record as _record, rel  # noqa: E402
from imagine360_amd import configs, kernels as K, pano_geometry as G, synthetic as S  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler  # noqa: E402

torch.set_grad_enabled(False)

LDS_PLANE = 32768          # elements of the largest plane the kernel keeps in LDS (64 KiB; kPlaneLdsBytes of csrc/latent_plane.h)

# (F, C, h, w, M, ph, pw), byte offset of x0 from its alignment: one case on each side of every choice the launcher makes
CASES = {
    "scalar_hw60": ((3, 4, 5, 12, 3, 4, 6), 0),                      # HW = 60: not a multiple of 8 -> scalar lanes, plane in LDS
    "vector_hw192": ((3, 4, 8, 24, 3, 4, 6), 0),                     # HW = 192, Q = 24: 16-byte lanes
    "scalar_q15": ((2, 4, 8, 24, 2, 3, 5), 0),                       # HW % 8 == 0 but Q = 15 -> scalar lanes
    "scalar_misaligned_x0": ((3, 4, 8, 24, 3, 4, 6), 2),             # vector sizes, x0 off its 16 bytes -> scalar lanes
    "lds_budget_exact": ((2, 1, 128, 256, 1, 2, 4), 0),              # 2 * HW = 64 KiB: the largest plane in LDS
    "global_vector": ((2, 1, 1, LDS_PLANE + 8, 1, 2, 4), 0),         # the smallest plane above the budget with 16-byte lanes
    "global_scalar": ((2, 1, 1, LDS_PLANE + 1, 1, 2, 4), 0),         # the smallest plane above the budget: recomputed, scalar
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
    steps = sch.timesteps_for_strength(0.5)[1]
    inputs = keep_case(*shape, dt, seed=11 + len(name))
    return inputs, sch.keep_coefficients(steps, 0), fp64_composition(sch, steps[1], *inputs)


def off_alignment(t, nbytes):
    """A contiguous copy of ``t`` that starts ``nbytes`` past a 256-byte aligned address."""
    n, k = t.numel(), nbytes // t.element_size()
    buf = torch.empty(n + k, dtype=t.dtype, device=t.device)
    view = buf[k:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == nbytes % 16
    return view


def device_inputs(name, dt):
    """Fresh device copies of a case's inputs (the two latents are written): (pano, pers, x0, noise, mask, idx, ok)."""
    inputs, _, _ = case(name, dt)
    dev = [t.cuda() for t in inputs]
    if CASES[name][1]:
        dev[2] = off_alignment(dev[2], CASES[name][1])
    return dev


def check_case(name, dt, pano, pers, noised):
    """``pano`` / ``pers``: the blended latents of case ``name``; ``noised``: ``K.noise_latents`` of the case at the same coefficients."""
    (pano0, pers0, x0, noise, mask, idx, ok), _, (want_pano, want_pers) = case(name, dt)
    pano, pers, noised = pano.cpu(), pers.cpu(), [t.cpu() for t in noised]
    assert pano.shape == pano0.shape and pers.shape == pers0.shape and pano.dtype == pers.dtype == dt
    errs = dict(pano=rel(pano, want_pano), pers=rel(pers, want_pers))
    print("keep_latents", name, dt, errs, flush=True)
    assert errs["pano"] < TOL[dt] and errs["pers"] < TOL[dt], (name, errs)
    w5 = mask[None, None].expand_as(pano)
    wg = mask_at_views(mask, idx, ok).expand_as(pers)
    seen = ok.bool()[None, :, None, None].expand_as(pers)
    assert (w5 >= 1).any() and (w5 <= 0).any() and ((w5 > 0) & (w5 < 1)).any() and (~seen).any(), name
    assert (seen & (wg >= 1)).any() and (seen & (wg <= 0)).any() and (seen & (wg > 0) & (wg < 1)).any(), name
    # mask 1: the input bits;  mask 0: what noise_latents writes at the same coefficients, bit for bit;  unseen pixels: the input bits
    assert same_bits(pano[w5 >= 1], pano0[w5 >= 1]), name
    assert same_bits(pano[w5 <= 0], noised[0][w5 <= 0]), name
    assert same_bits(pers[seen & (wg >= 1)], pers0[seen & (wg >= 1)]), name
    assert same_bits(pers[seen & (wg <= 0)], noised[1][seen & (wg <= 0)]), name
    assert same_bits(pers[~seen], pers0[~seen]), name
    assert torch.isfinite(pano.float()).all() and torch.isfinite(pers.float()).all()
    return errs


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_keep_latents_parity(dt):
    errs = {}
    for name in CASES:
        _, (sa, sb), _ = case(name, dt)
        pano, pers, x0, noise, mask, idx, ok = device_inputs(name, dt)
        noised = K.noise_latents(x0, noise, idx, ok, sa, sb)
        out = K.keep_latents(pano, pers, x0, noise, mask, idx, ok, sa, sb)
        assert out[0] is pano and out[1] is pers                           # in place
        e = check_case(name, dt, pano, pers, noised)
        errs[name] = max(e.values())
        # coefficients read from the device: the same bits
        p2, v2 = (t.cuda() for t in case(name, dt)[0][:2])
        K.keep_latents(p2, v2, x0, noise, mask, idx, ok, 0.0, 0.0, coef_dev=torch.tensor([sa, sb], dtype=torch.float32, device="cuda"))
        assert same_bits(p2, pano) and same_bits(v2, pers), name
        # the clean clip under an all-0 mask: x0 itself, and its gather where a view sees the panorama
        p3, v3 = (t.cuda() for t in case(name, dt)[0][:2])
        K.keep_latents(p3, v3, x0, noise, torch.zeros_like(mask), idx, ok, 1.0, 0.0)
        seen = ok.bool()[None, :, None, None].expand_as(v3)
        assert same_bits(p3, x0.contiguous()), name
        assert same_bits(v3[seen], gathered(x0, idx, ok)[seen]) and same_bits(v3[~seen], case(name, dt)[0][1].cuda()[~seen]), name
    # scalar lanes on vector sizes give the bits of the 16-byte lanes: the two cases differ in the alignment of x0 only
    _, (sa, sb), _ = case("vector_hw192", dt)
    a = device_inputs("vector_hw192", dt)
    b = [t.clone() for t in a]
    b[2] = off_alignment(a[2], 2)
    K.keep_latents(*a, sa, sb)
    K.keep_latents(*b, sa, sb)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    _record(f"keep_latents_{str(dt).split('.')[-1]}", max_rel=max(errs.values()), **errs)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(CASES))
def test_keep_latents_between_guard_bands(name, dt):
    """Both latents, the inputs and the tables between poisoned guards: nothing written outside, no input modified."""
    inputs, (sa, sb), _ = case(name, dt)
    g = Guarded(K)
    dev = [g.guard(t.cuda(), misalign=CASES[name][1] if i == 2 else 0) for i, t in enumerate(inputs)]
    noised = K.noise_latents(*dev[2:4], *dev[5:7], sa, sb)
    with g:
        pano, pers = g.out(*K.keep_latents(*dev, sa, sb))
    for t, host in zip(dev[2:], inputs[2:]):
        assert torch.equal(t.cpu().view(torch.uint8), host.contiguous().view(torch.uint8)), name       # inputs untouched
    check_case(name, dt, pano, pers, noised)


def test_keep_latents_rejects_bad_arguments():
    inputs, (sa, sb), _ = case("vector_hw192", torch.bfloat16)
    pano, pers, x0, noise, mask, idx, ok = (t.cuda() for t in inputs)
    args = lambda **kw: [kw.get(n, v) for n, v in zip(("pano", "pers", "x0", "noise", "mask", "idx", "ok"), (pano, pers, x0, noise, mask, idx, ok))]
    with pytest.raises(TypeError, match="bfloat16/float16"):
        K.keep_latents(*args(pano=pano.float()), sa, sb)
    with pytest.raises(TypeError, match="must have one dtype"):
        K.keep_latents(*args(x0=x0.half()), sa, sb)
    with pytest.raises(TypeError, match="noise and mask must be float32"):
        K.keep_latents(*args(mask=mask.to(torch.bfloat16)), sa, sb)
    with pytest.raises(TypeError, match="idx must be int32"):
        K.keep_latents(*args(idx=idx.long()), sa, sb)
    with pytest.raises(TypeError, match="coef_dev must be float32"):
        K.keep_latents(*args(), sa, sb, coef_dev=torch.zeros(2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="coef_dev must be a contiguous float32\\[2\\]"):
        K.keep_latents(*args(), sa, sb, coef_dev=torch.zeros(6, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="x0 must be"):
        K.keep_latents(*args(x0=x0[:, :2].contiguous()), sa, sb)
    with pytest.raises(ValueError, match="noise must be"):
        K.keep_latents(*args(noise=noise.permute(0, 2, 1, 3, 4).contiguous()[:, :, :2]), sa, sb)
    with pytest.raises(ValueError, match="mask must be"):
        K.keep_latents(*args(mask=mask[None]), sa, sb)
    with pytest.raises(ValueError, match="pers must be"):
        K.keep_latents(*args(pers=pers[:, :2].contiguous()), sa, sb)
    with pytest.raises(ValueError, match="contiguous"):
        K.keep_latents(*args(idx=idx.transpose(1, 2).contiguous().transpose(1, 2)), sa, sb)
    with pytest.raises(ValueError, match="one \\[M, ph, pw\\]"):
        K.keep_latents(*args(ok=ok[:1]), sa, sb)
    with pytest.raises(ValueError, match="x0 aliases pano"):
        K.keep_latents(*args(x0=pano), sa, sb)
    torch.cuda.synchronize()
    assert same_bits(pano.cpu(), inputs[0]) and same_bits(pers.cpu(), inputs[1])                    # no refused call wrote anything
    # the C entry point itself
    F, C, h, w, M, ph, pw = CASES["vector_hw192"][0]
    ptrs = [t.data_ptr() for t in (pano, pers, x0, noise, mask, idx, ok)]
    sizes = [F, C, h * w, M, ph * pw]
    fn, err = K.lib().im360_keep_latents, K.lib().im360_last_error
    for i in range(7):
        bad = list(ptrs)
        bad[i] = None
        assert fn(*bad, *sizes, sa, sb, 0, None, None) != 0 and b"null pointer" in err(), i
    for i in range(5):
        for v in (0, -3):
            bad = list(sizes)
            bad[i] = v
            assert fn(*ptrs, *bad, sa, sb, 0, None, None) != 0 and b"must be positive" in err(), (i, v)
    assert fn(*ptrs, *sizes, sa, sb, 7, None, None) != 0 and b"dtype 7 unsupported" in err()
    assert fn(*ptrs, F, C, 1 << 31, M, ph * pw, sa, sb, 0, None, None) != 0 and b"2^31" in err()
    assert fn(*ptrs, 1 << 16, 1 << 15, h * w, M, ph * pw, sa, sb, 0, None, None) != 0 and b"2^31" in err()
    assert fn(*ptrs, F, C, h * w, 1 << 16, 1 << 15, sa, sb, 0, None, None) != 0 and b"2^31" in err()
    for i in (3, 4, 5):
        bad = list(ptrs)
        bad[i] += 2
        assert fn(*bad, *sizes, sa, sb, 0, None, None) != 0 and b"misaligned noise, mask, idx or coef_dev" in err(), i
    coef = torch.tensor([0.0, sa, sb], dtype=torch.float32, device="cuda")
    assert fn(*ptrs, *sizes, sa, sb, 0, None, coef.data_ptr() + 2) != 0 and b"misaligned noise, mask, idx or coef_dev" in err()
    bad = list(ptrs)
    bad[2] = ptrs[0]
    assert fn(*bad, *sizes, sa, sb, 0, None, None) != 0 and b"x0 aliases pano" in err()
    torch.cuda.synchronize()
    assert same_bits(pano.cpu(), inputs[0]) and same_bits(pers.cpu(), inputs[1])
    assert fn(*ptrs, *sizes, 0.0, 0.0, 0, None, coef.data_ptr() + 4) == 0          # and the same arguments unbroken are accepted
    torch.cuda.synchronize()
    p2, v2 = inputs[0].cuda(), inputs[1].cuda()
    K.keep_latents(p2, v2, x0, noise, mask, idx, ok, sa, sb)
    assert same_bits(pano, p2) and same_bits(pers, v2)


# ------------------------------------------------------------------------------------------------ the small pipeline
STEPS, STRENGTH = 3, 2 / 3


@pytest.fixture(scope="module")
def clip():
    return S.video_batch(frames=8, pano_hw=(256, 512), seed=2)


@pytest.fixture(scope="module")
def small_pipe(clip):
    """The recipe of test_init_strength_gpu.py::small_pipe: 8 frames, 256 x 512, width-5 model, 3 steps."""
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    cond = S.conditioning(frames=16, seed=2)

    def run(use_graph, seed=33, **kw):
        pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
        pipe._no_progress, pipe.use_graph = True, use_graph
        torch.manual_seed(seed)
        random.seed(seed)
        vid = pipe("synthetic", num_inference_steps=STEPS, guidance_scale_text=7.5, negative_prompt="", video_batch=clip,
                   use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video",
                   latents_dtype=dt, prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]),
                   **kw).videos
        return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone()
    return run


@pytest.fixture(scope="module")
def first_call(small_pipe):
    return small_pipe(True)


@pytest.fixture(scope="module")
def refined(small_pipe, first_call):
    """The call with ``init_latents`` / ``strength`` and no mask."""
    return small_pipe(True, init_latents=first_call[1], strength=STRENGTH)


@pytest.fixture(scope="module")
def half(clip):
    """The half mask at pixel resolution and the latent pixels it keeps, bool [1, 4, 8, 32, 64] on the device."""
    m = half_mask(8, clip["pano_H"], clip["pano_W"])
    k = kept(m, clip["pano_H"] // 8, clip["pano_W"] // 8).expand(1, 4, -1, -1, -1).cuda()
    assert k.any() and not k.all() and not torch.equal(k[:, :, 0], k[:, :, 1]) and k[0, 0, 1, 16, 0] and k[0, 0, 1, 16, -1]
    return m, k


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_mask_all_one_is_the_call_without_the_keyword(small_pipe, first_call, refined):
    m = torch.ones(1, 8, 1, 256, 512)
    got = small_pipe(True, init_latents=first_call[1], strength=STRENGTH, regenerate_mask=m)
    assert _same(got, refined)


def test_mask_all_zero_returns_the_init_clip(small_pipe, first_call, clip):
    x0 = first_call[1]
    got = small_pipe(True, init_latents=x0, strength=STRENGTH, regenerate_mask=torch.zeros(1, 8, 1, 256, 512))
    assert same_bits(got[1], x0)
    ps = clip["pers_size"] // 8
    idx, ok = G.nearest_e2p_index(32, 64, ps, ps, clip["cameras"])
    idx, ok = idx.cuda(), ok.cuda().to(torch.uint8)
    seen = ok.bool()[None, :, None, None].expand_as(got[2])
    assert seen.any() and same_bits(got[2][seen], gathered(x0, idx, ok)[seen])


def test_half_mask_keeps_its_region_graph_equals_eager(small_pipe, first_call, refined, half):
    """Also the off-by-one-timestep check: after the first of the two steps the kept region is the clip noised to the timestep the
    SECOND step starts from, with the call's first noise draw."""
    x0 = first_call[1]
    m, k = half
    graphed = small_pipe(True, init_latents=x0, strength=STRENGTH, regenerate_mask=m)
    trace = []
    eager = small_pipe(False, init_latents=x0, strength=STRENGTH, regenerate_mask=m, trace=trace)
    errs = dict(graph_vs_eager_latent=rel(graphed[1], eager[1]), regenerated_vs_init=rel(graphed[1][~k], x0[~k]),
                masked_vs_unmasked_refinement=rel(graphed[1], refined[1]))
    _record("keep_mask_half", **errs)
    assert _same(graphed, eager), errs
    assert same_bits(graphed[1][k], x0[k])
    assert not torch.equal(graphed[1][~k], x0[~k]) and not torch.equal(graphed[1], refined[1])
    assert all(torch.isfinite(v.float()).all() for v in graphed)
    assert len(trace) == 2 and torch.equal(trace[1], eager[1])
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(STEPS)
    steps = sch.timesteps_for_strength(STRENGTH)[1]
    assert len(steps) == 2
    torch.manual_seed(33)
    noise = torch.randn((1, 8, 1, 4, 32, 64), device="cuda").squeeze(2)                 # init_noise's draw, the first of the call
    sa, sb = sch.keep_coefficients(steps, 0)
    idx, ok = torch.zeros(1, 1, 8, dtype=torch.int32, device="cuda"), torch.ones(1, 1, 8, dtype=torch.uint8, device="cuda")
    want = K.noise_latents(x0, noise, idx, ok, sa, sb)[0]                               # T(sa x0 + sb noise), one rounding
    want64 = sch.add_noise(x0.double(), noise.double().permute(0, 2, 1, 3, 4), torch.tensor([steps[1]]))
    assert rel(want, want64) < TOL[torch.bfloat16]
    assert same_bits(trace[0][k], want[k])
    own_level = K.noise_latents(x0, noise, idx, ok, *sch.noise_coefficients(steps[0]))[0]
    assert not torch.equal(trace[0][k], own_level[k])


def test_half_mask_over_ring_windows_graph_equals_eager(small_pipe, first_call, half):
    """Windows of 4 frames with overlap 2 on a ring, guidance rescale 0.7, eta = 0.5 from a seeded device generator."""
    x0 = first_call[1]
    m, k = half
    cuda_gen = lambda s: torch.Generator(device="cuda").manual_seed(s)
    kw = dict(init_latents=x0, strength=STRENGTH, regenerate_mask=m, context_frames=4, context_overlap=2, context_loop=True,
              guidance_rescale=0.7, eta=0.5)
    graphed = small_pipe(True, generator=cuda_gen(77), **kw)
    eager = small_pipe(False, generator=cuda_gen(77), **kw)
    errs = dict(graph_vs_eager_latent=rel(graphed[1], eager[1]), regenerated_vs_init=rel(graphed[1][~k], x0[~k]))
    _record("keep_mask_ring_windows", **errs)
    assert _same(graphed, eager), errs
    assert same_bits(graphed[1][k], x0[k]) and not torch.equal(graphed[1][~k], x0[~k])
    assert all(torch.isfinite(v.float()).all() for v in graphed)


def test_a_call_without_the_keyword_afterwards_is_the_first_call(small_pipe, first_call):
    """No state leaks from the runs with a mask (this file's order: after them) into a run from pure noise."""
    assert _same(small_pipe(True), first_call)
