"""Release mode of ``regenerate_mask`` on the MI355X: ``kernels.keep_latents_release`` (csrc/keep_latents.hip, the RELEASE instantiation)
on every path of its launcher, bit for bit -- every element is its input bits or the bits ``kernels.noise_latents`` writes at the same
coefficients -- the same cases between guard bands, the refusals of the wrapper and of the C entry point, and the small pipeline with
``regenerate_mode="release"``: graph replay against the eager loop (plain, over ring windows, with DPM-Solver++ 2M), the pinned bits
after every step, a 0 / 1 mask against blend mode."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _release_pipe as RP  # noqa: E402
from _emu_keep_latents import half_mask, kept, mask_at_views  # noqa: E402
from _emu_keep_release import TAU, band_map, release_case  # noqa: E402
from _emu_noise_latents import TOL, fp64_composition as noise_fp64, gathered, same_bits  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import rel  # noqa: E402
from imagine360_amd import configs, kernels as K, pano_geometry as G  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402

torch.set_grad_enabled(False)

LDS_PLANE = 32768          # elements of the largest plane the kernel keeps in LDS (64 KiB; kPlaneLdsBytes of csrc/latent_plane.h)

# (F, C, h, w, M, ph, pw), byte offset of x0 from its alignment: the seven cases of tests/test_keep_mask_gpu.py, one on each side of
# every choice the launcher makes
CASES = {
    "scalar_hw60": ((3, 4, 5, 12, 3, 4, 6), 0),                      # HW = 60: not a multiple of 8 -> scalar lanes, plane in LDS
    "vector_hw192": ((3, 4, 8, 24, 3, 4, 6), 0),                     # HW = 192, Q = 24: 16-byte lanes
    "scalar_q15": ((2, 4, 8, 24, 2, 3, 5), 0),                       # HW % 8 == 0 but Q = 15 -> scalar lanes
    "scalar_misaligned_x0": ((3, 4, 8, 24, 3, 4, 6), 2),             # vector sizes, x0 off its 16 bytes -> scalar lanes
    "lds_budget_exact": ((2, 1, 128, 256, 1, 2, 4), 0),              # 2 * HW = 64 KiB: the largest plane in LDS
    "global_vector": ((2, 1, 1, LDS_PLANE + 8, 1, 2, 4), 0),         # the smallest plane above the budget with 16-byte lanes
    "global_scalar": ((2, 1, 1, LDS_PLANE + 1, 1, 2, 4), 0),         # the smallest plane above the budget: recomputed, scalar
}


@functools.lru_cache(maxsize=None)
def case(name, dt):
    """Host inputs and coefficients of one case (computed once, never written to)."""
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    steps = sch.timesteps_for_strength(0.5)[1]
    return release_case(*CASES[name][0], dt, seed=11 + len(name)), sch.keep_coefficients(steps, 0), (sch, steps[1])


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
    dev = [t.cuda() for t in case(name, dt)[0]]
    if CASES[name][1]:
        dev[2] = off_alignment(dev[2], CASES[name][1])
    return dev


def expected(name, dt, noised, tau):
    """The definition on the host: the pinned elements from ``noised`` (``K.noise_latents`` at the same coefficients), every other one its
    input bits.  -> (pano, pers, pin, pin at the views)"""
    pano0, pers0, x0, noise, s, idx, ok = case(name, dt)[0]
    pin = (s <= torch.tensor(tau, dtype=torch.float32))[None, None].expand_as(pano0)
    pin_v = (mask_at_views(s, idx, ok) <= torch.tensor(tau, dtype=torch.float32)).expand_as(pers0) & ok.bool()[None, :, None, None].expand_as(pers0)
    return torch.where(pin, noised[0].cpu(), pano0), torch.where(pin_v, noised[1].cpu(), pers0), pin, pin_v


def check_case(name, dt, pano, pers, noised, tau=TAU):
    (pano0, pers0, x0, noise, s, idx, ok), _, _ = case(name, dt)
    want_pano, want_pers, pin, pin_v = expected(name, dt, noised, tau)
    pano, pers = pano.cpu(), pers.cpu()
    assert pano.shape == pano0.shape and pers.shape == pers0.shape and pano.dtype == pers.dtype == dt
    # the map holds every kind: exact 0 and 1, below, AT and above the threshold, in the panorama and where a view sees it
    if tau == TAU:
        for sel in (s == 0, s == 1, (s > 0) & (s < tau - 0.05), s == tau, (s > tau + 0.05) & (s < 1)):
            assert sel.any(), name
        assert pin_v.any() and (~pin_v & ok.bool()[None, :, None, None].expand_as(pers0)).any() and (ok == 0).any(), name
    assert same_bits(pano, want_pano), (name, int((pano.view(torch.int16) != want_pano.view(torch.int16)).sum()))
    assert same_bits(pers, want_pers), (name, int((pers.view(torch.int16) != want_pers.view(torch.int16)).sum()))
    assert not same_bits(pano, pano0) and not same_bits(pers, pers0)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_keep_latents_release_parity(dt):
    for name in CASES:
        inputs, (sa, sb), (sch, t) = case(name, dt)
        pano, pers, x0, noise, s, idx, ok = device_inputs(name, dt)
        noised = K.noise_latents(x0, noise, idx, ok, sa, sb)
        ref = noise_fp64(sch, t, inputs[2], inputs[3], inputs[5], inputs[6])                   # ... which is add_noise in fp64
        assert rel(noised[0].cpu(), ref[0]) < TOL[dt] and rel(noised[1].cpu(), ref[1]) < TOL[dt]
        out = K.keep_latents_release(pano, pers, x0, noise, s, idx, ok, sa, sb, TAU)
        assert out[0] is pano and out[1] is pers                                               # in place
        check_case(name, dt, pano, pers, noised)
        # coefficients read from the device: the same bits
        p2, v2 = (t_.cuda() for t_ in inputs[:2])
        K.keep_latents_release(p2, v2, x0, noise, s, idx, ok, 0.0, 0.0, -1.0, coef_dev=torch.tensor([sa, sb, TAU], dtype=torch.float32, device="cuda"))
        assert same_bits(p2, pano) and same_bits(v2, pers), name
        # a negative threshold pins nothing
        p3, v3 = (t_.cuda() for t_ in inputs[:2])
        K.keep_latents_release(p3, v3, x0, noise, s, idx, ok, sa, sb, -1.0)
        assert same_bits(p3.cpu(), inputs[0]) and same_bits(v3.cpu(), inputs[1]), name
        # after the last step (tau = 0, the clean clip): the s = 0 region is x0 itself and its gather where a view sees it, the rest untouched
        p4, v4 = (t_.cuda() for t_ in inputs[:2])
        K.keep_latents_release(p4, v4, x0, noise, s, idx, ok, 1.0, 0.0, 0.0)
        zero = (s == 0)[None, None].expand_as(p4)
        zero_v = (mask_at_views(s, idx, ok).cuda() == 0).expand_as(v4) & ok.bool()[None, :, None, None].expand_as(v4)
        assert zero.any() and zero_v.any()
        assert same_bits(p4[zero], x0.contiguous()[zero]) and same_bits(p4[~zero].cpu(), inputs[0][~zero.cpu()]), name
        assert same_bits(v4[zero_v], gathered(x0, idx, ok)[zero_v]) and same_bits(v4[~zero_v].cpu(), inputs[1][~zero_v.cpu()]), name
        # a 0 / 1 map: the bits of blend mode
        binary = (s > TAU).float()
        p5, v5 = (t_.cuda() for t_ in inputs[:2])
        p6, v6 = (t_.cuda() for t_ in inputs[:2])
        K.keep_latents_release(p5, v5, x0, noise, binary, idx, ok, sa, sb, TAU)
        K.keep_latents(p6, v6, x0, noise, binary, idx, ok, sa, sb)
        assert same_bits(p5, p6) and same_bits(v5, v6) and same_bits(p5, pano) and same_bits(v5, pers), name
    # scalar lanes on vector sizes give the bits of the 16-byte lanes: the two cases differ in the alignment of x0 only
    _, (sa, sb), _ = case("vector_hw192", dt)
    a = device_inputs("vector_hw192", dt)
    b = [t_.clone() for t_ in a]
    b[2] = off_alignment(a[2], 2)
    K.keep_latents_release(*a, sa, sb, TAU)
    K.keep_latents_release(*b, sa, sb, TAU)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(CASES))
def test_keep_latents_release_between_guard_bands(name, dt):
    """Both latents, the inputs and the tables between poisoned guards: nothing written outside (a group of eight that changes nothing
    is not stored, into a guard neither), no input modified."""
    inputs, (sa, sb), _ = case(name, dt)
    g = Guarded(K)
    dev = [g.guard(t.cuda(), misalign=CASES[name][1] if i == 2 else 0) for i, t in enumerate(inputs)]
    noised = K.noise_latents(*dev[2:4], *dev[5:7], sa, sb)
    with g:
        pano, pers = g.out(*K.keep_latents_release(*dev, sa, sb, TAU))
    for t, host in zip(dev[2:], inputs[2:]):
        assert torch.equal(t.cpu().view(torch.uint8), host.contiguous().view(torch.uint8)), name       # inputs untouched
    check_case(name, dt, pano, pers, noised)


def test_keep_latents_release_rejects_bad_arguments():
    inputs, (sa, sb), _ = case("vector_hw192", torch.bfloat16)
    pano, pers, x0, noise, mask, idx, ok = (t.cuda() for t in inputs)
    args = lambda **kw: [kw.get(n, v) for n, v in zip(("pano", "pers", "x0", "noise", "mask", "idx", "ok"), (pano, pers, x0, noise, mask, idx, ok))]
    R = K.keep_latents_release
    with pytest.raises(TypeError, match="bfloat16/float16"):
        R(*args(pano=pano.float()), sa, sb, TAU)
    with pytest.raises(TypeError, match="keep_latents_release: pano, pers and x0 must have one dtype"):
        R(*args(x0=x0.half()), sa, sb, TAU)
    with pytest.raises(TypeError, match="noise and mask must be float32"):
        R(*args(mask=mask.to(torch.bfloat16)), sa, sb, TAU)
    with pytest.raises(TypeError, match="idx must be int32"):
        R(*args(idx=idx.long()), sa, sb, TAU)
    with pytest.raises(TypeError, match="coef_dev must be float32"):
        R(*args(), sa, sb, TAU, coef_dev=torch.zeros(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="coef_dev must be a contiguous float32\\[3\\]"):
        R(*args(), sa, sb, TAU, coef_dev=torch.zeros(2, dtype=torch.float32, device="cuda"))           # the two floats of blend mode
    with pytest.raises(ValueError, match="x0 must be"):
        R(*args(x0=x0[:, :2].contiguous()), sa, sb, TAU)
    with pytest.raises(ValueError, match="noise must be"):
        R(*args(noise=noise.permute(0, 2, 1, 3, 4).contiguous()[:, :, :2]), sa, sb, TAU)
    with pytest.raises(ValueError, match="mask must be"):
        R(*args(mask=mask[None]), sa, sb, TAU)
    with pytest.raises(ValueError, match="pers must be"):
        R(*args(pers=pers[:, :2].contiguous()), sa, sb, TAU)
    with pytest.raises(ValueError, match="contiguous"):
        R(*args(idx=idx.transpose(1, 2).contiguous().transpose(1, 2)), sa, sb, TAU)
    with pytest.raises(ValueError, match="one \\[M, ph, pw\\]"):
        R(*args(ok=ok[:1]), sa, sb, TAU)
    with pytest.raises(ValueError, match="x0 aliases pano"):
        R(*args(x0=pano), sa, sb, TAU)
    with pytest.raises(ValueError, match="coef_dev must be a contiguous float32\\[2\\]"):
        K.keep_latents(*args(), sa, sb, coef_dev=torch.zeros(3, dtype=torch.float32, device="cuda"))   # and blend mode keeps its two
    torch.cuda.synchronize()
    assert same_bits(pano.cpu(), inputs[0]) and same_bits(pers.cpu(), inputs[1])                    # no refused call wrote anything
    # the C entry point itself
    F, C, h, w, M, ph, pw = CASES["vector_hw192"][0]
    ptrs = [t.data_ptr() for t in (pano, pers, x0, noise, mask, idx, ok)]
    sizes = [F, C, h * w, M, ph * pw]
    fn, err = K.lib().im360_keep_latents_release, K.lib().im360_last_error
    for i in range(7):
        bad = list(ptrs)
        bad[i] = None
        assert fn(*bad, *sizes, sa, sb, TAU, 0, None, None) != 0 and b"keep_latents_release: null pointer" in err(), i
    for i in range(5):
        for v in (0, -3):
            bad = list(sizes)
            bad[i] = v
            assert fn(*ptrs, *bad, sa, sb, TAU, 0, None, None) != 0 and b"must be positive" in err(), (i, v)
    assert fn(*ptrs, *sizes, sa, sb, TAU, 7, None, None) != 0 and b"dtype 7 unsupported" in err()
    assert fn(*ptrs, F, C, 1 << 31, M, ph * pw, sa, sb, TAU, 0, None, None) != 0 and b"2^31" in err()
    assert fn(*ptrs, 1 << 16, 1 << 15, h * w, M, ph * pw, sa, sb, TAU, 0, None, None) != 0 and b"2^31" in err()
    assert fn(*ptrs, F, C, h * w, 1 << 16, 1 << 15, sa, sb, TAU, 0, None, None) != 0 and b"2^31" in err()
    for i in (3, 4, 5):
        bad = list(ptrs)
        bad[i] += 2
        assert fn(*bad, *sizes, sa, sb, TAU, 0, None, None) != 0 and b"misaligned noise, mask, idx or coef_dev" in err(), i
    coef = torch.tensor([0.0, sa, sb, TAU], dtype=torch.float32, device="cuda")
    assert fn(*ptrs, *sizes, sa, sb, TAU, 0, None, coef.data_ptr() + 2) != 0 and b"misaligned noise, mask, idx or coef_dev" in err()
    bad = list(ptrs)
    bad[2] = ptrs[0]
    assert fn(*bad, *sizes, sa, sb, TAU, 0, None, None) != 0 and b"x0 aliases pano" in err()
    torch.cuda.synchronize()
    assert same_bits(pano.cpu(), inputs[0]) and same_bits(pers.cpu(), inputs[1])
    assert fn(*ptrs, *sizes, 0.0, 0.0, -1.0, 0, None, coef.data_ptr() + 4) == 0        # and the same arguments unbroken are accepted
    torch.cuda.synchronize()
    p2, v2 = inputs[0].cuda(), inputs[1].cuda()
    R(p2, v2, x0, noise, mask, idx, ok, sa, sb, TAU)
    assert same_bits(pano, p2) and same_bits(pers, v2)


# ------------------------------------------------------------------------------------------------ the small pipeline
@pytest.fixture(scope="module")
def clip():
    return RP.make_clip()


@pytest.fixture(scope="module")
def small_pipe(clip):
    return RP.make_runner(clip)


@pytest.fixture(scope="module")
def first_call(small_pipe):
    return small_pipe(True)


@pytest.fixture(scope="module")
def smap(clip):
    """The band map (0, 1, 1/6, 1/2, 5/6: none on a threshold of the three steps) and its latent-resolution values [F, h, w]."""
    m = band_map(RP.FRAMES, clip["pano_H"], clip["pano_W"], 3)
    s = torch.nn.functional.interpolate(m.transpose(2, 1), size=(RP.FRAMES, *RP.LAT_HW))[0, 0]
    _, _, taus = RP.run_thresholds()
    assert len(taus) == 3 and all(abs(float(v) - tau) > 0.1 for tau in taus for v in s.unique() if 0 < v < 1)
    return m, s


def test_release_graph_equals_eager_and_pins_per_step(small_pipe, first_call, smap):
    x0 = first_call[1]
    m, s = smap
    kw = dict(init_latents=x0, strength=RP.STRENGTH, regenerate_mask=m, regenerate_mode="release")
    graphed = small_pipe(True, **kw)
    trace = []
    eager = small_pipe(False, trace=trace, **kw)
    assert RP.same(graphed, eager), rel(graphed[1], eager[1])
    assert all(torch.isfinite(v.float()).all() for v in graphed)
    sch, steps, taus = RP.run_thresholds()
    assert len(trace) == 3 and torch.equal(trace[-1], eager[1])
    torch.manual_seed(33)
    noise = torch.randn((1, RP.FRAMES, 1, 4, *RP.LAT_HW), device="cuda").squeeze(2)     # init_noise's draw, the first of the call
    idx, ok = torch.zeros(1, 1, 8, dtype=torch.int32, device="cuda"), torch.ones(1, 1, 8, dtype=torch.uint8, device="cuda")
    s5 = s.cuda()[None, None].expand_as(x0)
    counts = []
    for i, tau in enumerate(taus):
        known = K.noise_latents(x0, noise, idx, ok, *sch.keep_coefficients(steps, i))[0]
        pin = s5 <= tau
        counts.append(int(pin.sum()))
        assert same_bits(trace[i][pin], known[pin])                                   # pinned: the noised clip, bit for bit
        assert not torch.equal(trace[i][~pin], known[~pin])                           # free: left as the step wrote it
    assert counts[0] > counts[1] > counts[2] > 0
    zero, one = s5 == 0, s5 == 1
    assert same_bits(graphed[1][zero], x0[zero])                                      # the s = 0 region is the init, bit for bit
    assert not torch.equal(graphed[1][one], x0[one])
    # and release mode is not blend mode on a fractional map
    blended = small_pipe(True, init_latents=x0, strength=RP.STRENGTH, regenerate_mask=m)
    assert not torch.equal(blended[1], graphed[1]) and same_bits(blended[1][zero], x0[zero])


def test_release_over_ring_windows_graph_equals_eager(small_pipe, first_call, smap):
    """Windows of 4 frames with overlap 2 on a ring, guidance rescale 0.7, eta = 0.5 from a seeded device generator."""
    x0 = first_call[1]
    m, s = smap
    cuda_gen = lambda sd: torch.Generator(device="cuda").manual_seed(sd)
    kw = dict(init_latents=x0, strength=RP.STRENGTH, regenerate_mask=m, regenerate_mode="release", context_frames=4, context_overlap=2,
              context_loop=True, guidance_rescale=0.7, eta=0.5)
    graphed = small_pipe(True, generator=cuda_gen(77), **kw)
    eager = small_pipe(False, generator=cuda_gen(77), **kw)
    assert RP.same(graphed, eager), rel(graphed[1], eager[1])
    zero = (s.cuda() == 0)[None, None].expand_as(x0)
    assert same_bits(graphed[1][zero], x0[zero]) and not torch.equal(graphed[1][~zero], x0[~zero])
    assert all(torch.isfinite(v.float()).all() for v in graphed)


def test_release_with_dpm_solver_graph_equals_eager(small_pipe, first_call, smap):
    x0 = first_call[1]
    m, s = smap
    dpm = lambda: DPMSolverMultistepScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    kw = dict(init_latents=x0, strength=RP.STRENGTH, regenerate_mask=m, regenerate_mode="release")
    graphed = small_pipe(True, scheduler=dpm(), **kw)
    eager = small_pipe(False, scheduler=dpm(), **kw)
    assert RP.same(graphed, eager), rel(graphed[1], eager[1])
    zero = (s.cuda() == 0)[None, None].expand_as(x0)
    assert same_bits(graphed[1][zero], x0[zero]) and not torch.equal(graphed[1][~zero], x0[~zero])


def test_binary_mask_in_release_mode_is_blend_mode(small_pipe, first_call, clip):
    x0 = first_call[1]
    m = half_mask(RP.FRAMES, clip["pano_H"], clip["pano_W"])
    k = kept(m, *RP.LAT_HW).expand(1, 4, -1, -1, -1).cuda()
    blend = small_pipe(True, init_latents=x0, strength=RP.STRENGTH, regenerate_mask=m)
    release = small_pipe(True, init_latents=x0, strength=RP.STRENGTH, regenerate_mask=m, regenerate_mode="release")
    assert RP.same(blend, release)
    assert k.any() and not k.all() and same_bits(release[1][k], x0[k]) and not torch.equal(release[1][~k], x0[~k])


def test_a_call_without_the_keywords_afterwards_is_the_first_call(small_pipe, first_call):
    """No state leaks from the runs in release mode (this file's order: after them) into a run from pure noise."""
    assert RP.same(small_pipe(True), first_call)
