"""The spherical feather on the MI355X: ``kernels.sphere_distance2`` (csrc/sphere_distance.hip) against the definition in fp64 on the
same fp32 vector table, the same cases between guard bands, the refusals, and the pipeline with ``regenerate_feather`` against the
pipeline given the eagerly feathered map."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _release_pipe as RP  # noqa: E402
from _emu_keep_latents import half_mask  # noqa: E402
from _emu_sphere_distance import BOUND, chord2_fp64  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record as _record  # noqa: E402
from imagine360_amd import kernels as K, pano_geometry as G  # noqa: E402

torch.set_grad_enabled(False)

# (F, h, w): HW = 72 (one ragged block), 65 (odd), 512 (one block of 512 pixels exactly), 1152 (three blocks, the last ragged, and two
# LDS candidate tiles of 1024, the second ragged)
SHAPES = [(2, 6, 12), (2, 5, 13), (3, 16, 32), (3, 24, 48)]


@functools.lru_cache(maxsize=None)
def case(shape):
    """keep uint8 [F, h, w] -- frame 0 sparse random, frame 1 without a kept pixel (the first two shapes: the second of them all kept
    instead), frame 2 all kept -- the fp32 table, and the fp64 definition on that table (computed once)."""
    F, h, w = shape
    keep = (torch.rand(F, h, w, generator=torch.Generator().manual_seed(h * w)) < 0.1).to(torch.uint8)
    keep[0, h // 2, 0] = 1
    keep[1] = 1 if shape == (2, 5, 13) else 0
    if F > 2:
        keep[2] = 1
    dirs = G.pixel_directions(h, w)
    return keep, dirs, chord2_fp64(keep, dirs)


def check(shape, got):
    keep, _, ref = case(shape)
    got = got.cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    none = ~keep.flatten(1).bool().any(dim=1)
    assert torch.equal(torch.isinf(got), none[:, None, None].expand_as(got)) and (got >= 0).all()       # +inf exactly on the frames that keep nothing
    assert (got[keep.bool()] == 0).all()
    fin = torch.isfinite(ref)
    err = (got.double()[fin] - ref[fin]).abs()
    ratio = float((err / (BOUND * ref[fin]).clamp(min=1e-300)).max()) if fin.any() else 0.0
    print(f"sphere_distance2 {shape}: worst |d2 - ref| / (8 * 2^-24 * ref) = {ratio:.3f}", flush=True)
    assert (err <= BOUND * ref[fin]).all(), (shape, ratio)
    return ratio


def test_sphere_distance2_parity():
    worst = {}
    seen_inf = seen_all = False
    for shape in SHAPES:
        keep, dirs, _ = case(shape)
        got = K.sphere_distance2(keep.cuda(), dirs.cuda())
        worst[str(shape)] = check(shape, got)
        seen_inf |= bool(torch.isinf(got).any())
        seen_all |= bool((keep.flatten(1).sum(1) == keep[0].numel()).any())
        assert torch.equal(K.sphere_distance2(keep.bool().cuda(), dirs.cuda()), got)               # a bool map is the uint8 map
    assert seen_inf and seen_all
    _record("sphere_distance2", max_ratio_of_bound=max(worst.values()), **worst)


@pytest.mark.parametrize("shape", SHAPES)
def test_sphere_distance2_between_guard_bands(shape):
    keep, dirs, _ = case(shape)
    g = Guarded(K)
    dk, dd = g.guard(keep.cuda()), g.guard(dirs.cuda())
    with g:
        out = g.out(K.sphere_distance2(dk, dd))
    assert torch.equal(dk.cpu(), keep) and torch.equal(dd.cpu(), dirs)                              # inputs untouched
    check(shape, out)


def test_sphere_distance2_rejects_bad_arguments():
    keep, dirs, _ = case((2, 6, 12))
    keep, dirs = keep.cuda(), dirs.cuda()
    with pytest.raises(TypeError, match="keep must be bool or uint8 and dirs float32"):
        K.sphere_distance2(keep.float(), dirs)
    with pytest.raises(TypeError, match="keep must be bool or uint8 and dirs float32"):
        K.sphere_distance2(keep, dirs.double())
    with pytest.raises(ValueError, match=r"keep must be a non-empty \[F, h, w\]"):
        K.sphere_distance2(keep[0], dirs)
    with pytest.raises(ValueError, match="dirs must be"):
        K.sphere_distance2(keep, dirs[:-1])
    with pytest.raises(ValueError, match="contiguous"):
        K.sphere_distance2(keep.transpose(1, 2), G.pixel_directions(12, 6).cuda())
    with pytest.raises(RuntimeError, match="need tensors on the MI355X"):
        K.sphere_distance2(keep.cpu(), dirs.cpu())
    fn, err = K.lib().im360_sphere_distance2, K.lib().im360_last_error
    out = torch.full((2, 72), -1.0, device="cuda")
    ptrs = [keep.data_ptr(), dirs.data_ptr(), out.data_ptr()]
    for i in range(3):
        bad = list(ptrs)
        bad[i] = None
        assert fn(*bad, 2, 72, None) != 0 and b"null pointer" in err(), i
    for F_, HW in ((0, 72), (2, 0), (-1, 72)):
        assert fn(*ptrs, F_, HW, None) != 0 and b"must be positive" in err()
    assert fn(*ptrs, 2, 1 << 31, None) != 0 and b"2^31" in err()
    assert fn(*ptrs, 1 << 24, 72, None) != 0 and b"2^24 workgroups" in err()
    assert fn(ptrs[0], ptrs[1] + 2, ptrs[2], 2, 72, None) != 0 and b"misaligned dirs or d2" in err()
    assert fn(ptrs[0], ptrs[1], ptrs[1], 2, 72, None) != 0 and b"d2 overlaps keep or dirs" in err()
    torch.cuda.synchronize()
    assert (out == -1).all()                                                                        # no refused call wrote anything


# ------------------------------------------------------------------------------------------------ the small pipeline
THETA = 23.0             # degrees; see test_feathered_pipeline_is_the_pipeline_on_the_eager_map for why no value lands on a threshold


def test_feathered_pipeline_is_the_pipeline_on_the_eager_map():
    """``regenerate_feather`` feathers with the kernel's distances, the eager map with torch's: the two ramps differ in their last
    bits, which changes the run only where a value crosses a threshold.  Asserted first, on the CPU, on the eager map: no value within
    1e-4 of a threshold -- so both runs pin the same pixels at every step and must agree bit for bit."""
    clip = RP.make_clip()
    half = half_mask(RP.FRAMES, clip["pano_H"], clip["pano_W"])
    hard = torch.nn.functional.interpolate(half.transpose(2, 1), size=(RP.FRAMES, *RP.LAT_HW))[0, 0].clamp(0, 1).contiguous()
    soft = G.feather_pano_mask(hard, THETA)                                                         # eager, CPU
    _, _, taus = RP.run_thresholds()
    gap = min(float((soft - tau).abs().min()) for tau in taus if tau > 0)
    print(f"feather {THETA} degrees: nearest map value to a threshold {taus}: {gap:.3g}", flush=True)
    assert gap > 1e-4 and ((soft > 0) & (soft < 1)).any() and (soft == 0).any() and (soft == 1).any()
    for tau in taus:
        assert (soft <= tau).any() and not (soft <= tau).all()
    run = RP.make_runner(clip)
    on_device = run.prepare_mask(half, feather=THETA).cpu()
    diff = float((on_device - soft).abs().max())
    # d ramp / d d2 = 1 / (Theta sqrt(d2 (1 - d2 / 4))); d2 differs by BOUND * d2 at most between the two (each within BOUND / 2 ... BOUND of
    # the fp64 value), so the ramp by about 2 * BOUND * sqrt(d2) / Theta <= 2 * BOUND * 2 sin(Theta / 2) / Theta < 2 * BOUND -- far below 1e-4
    print(f"feathered map, kernel distances against eager: max |difference| = {diff:.3g}", flush=True)
    assert diff <= 1e-5 and torch.equal(on_device == 0, soft == 0)
    assert all(torch.equal(on_device <= tau, soft <= tau) for tau in taus)                          # the same pixels are pinned
    x0 = run(True)[1]
    kw = dict(init_latents=x0, strength=RP.STRENGTH, regenerate_mode="release")
    feathered = run(True, regenerate_mask=half, regenerate_feather=THETA, **kw)
    given = run(True, regenerate_mask=soft[None, :, None], **kw)                                    # at latent size: the resize is the identity
    assert RP.same(feathered, given)
    zero = (soft == 0)[None, None].expand_as(x0).cuda()
    assert torch.equal(feathered[1][zero], x0[zero]) and not torch.equal(feathered[1][~zero], x0[~zero])
    hard_run = run(True, regenerate_mask=half, **kw)
    assert not torch.equal(hard_run[1], feathered[1])                                               # and the feather does change the run
    _record("sphere_feather_pipeline", nearest_value_to_a_threshold=gap, map_max_abs_diff=diff)
