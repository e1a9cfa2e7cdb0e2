"""The hi-res pass on the MI355X: ``kernels.resize_pano_latent`` (csrc/resize_latents.hip) against the fp64 definition
``pano_geometry.resize_pano_latent`` per element on every path of its launcher, its bit contracts (16-byte and scalar stores give the same
bits, a roll of the input is a roll of the result, equal sizes return the input), the same cases between guard bands, the refusals of
the wrapper and of the C entry point, and the small pipeline: a clip generated at 256 x 512 refined at 512 x 1024, graph replay against
the eager loop, with ``regenerate_mask``, and a call at the small size afterwards."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from _emu_keep_latents import half_mask, kept  # noqa: E402
from _emu_resize_latents import C, CASES, F, MODES, case, reference, same_bits, worst_ratio  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record as _record, rel  # noqa: E402
from imagine360_amd import configs, kernels as K, synthetic as S  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler  # noqa: E402

torch.set_grad_enabled(False)


def off_alignment(t, nbytes=2):
    """A contiguous copy of ``t`` that starts ``nbytes`` past a 256-byte aligned address: the launcher takes the scalar path."""
    n, k = t.numel(), nbytes // t.element_size()
    buf = torch.empty(n + k, dtype=t.dtype, device=t.device)
    view = buf[k:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == nbytes % 16
    return view


def check_case(name, dt, mode, got):
    x = case(name, dt)
    _, (H, W) = CASES[name]
    assert got.shape == (1, C, F, H, W) and got.dtype == dt
    assert torch.isfinite(got.float()).all(), name
    ratio = worst_ratio(got, reference(name, dt, mode), x, dt)
    print("resize_pano_latent", name, dt, mode, "worst |error| / tolerance", ratio, flush=True)
    assert ratio < 1.0, (name, mode, ratio)
    if name == "identity":
        assert same_bits(got.cpu(), x), (name, mode)
    return ratio


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_resize_pano_latent_parity(dt):
    """Per element within 0.5 ulp_T(reference) + 2^-17 max|x| of the fp64 definition, both modes, every case."""
    worst = {}
    for mode in MODES:
        for name, (_, (H, W)) in CASES.items():
            got = K.resize_pano_latent(case(name, dt).cuda(), H, W, mode)
            worst[f"{name}_{mode}"] = check_case(name, dt, mode, got)
    _record(f"resize_pano_latent_{str(dt).split('.')[-1]}", worst_ratio=max(worst.values()), **worst)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", MODES)
def test_vector_and_scalar_paths_give_the_same_bits(mode, dt):
    """The cases with W % 8 == 0 once aligned (16-byte stores) and once with the input one element off its alignment (scalar stores)."""
    for name in ("vector_x2", "vector_ragged_scale", "vector_three_tiles", "vector_looped", "identity"):
        _, (H, W) = CASES[name]
        x = case(name, dt).cuda()
        assert W % 8 == 0 and x.data_ptr() % 16 == 0
        a = K.resize_pano_latent(x, H, W, mode)
        b = K.resize_pano_latent(off_alignment(x), H, W, mode)
        assert a.data_ptr() % 16 == 0 and same_bits(a, b), (name, mode)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", MODES)
def test_rolling_the_input_rolls_the_result_bit_for_bit(mode, dt):
    """Integer scales 2 and 3: t is periodic in the output column, the taps wrap, so the seam is a column like every other.  On the
    16-byte path (W = 16, 24) and, with W = 3 * 5, on the scalar one."""
    g = torch.Generator().manual_seed(41)
    for s, (h, w) in ((2, (4, 8)), (3, (5, 8)), (3, (4, 5))):
        x = (1.5 * torch.randn(1, C, F, h, w, generator=g)).to(dt).cuda()
        base = K.resize_pano_latent(x, s * h, s * w, mode)
        for k in (1, 3, w - 1):
            got = K.resize_pano_latent(x.roll(k, dims=-1).contiguous(), s * h, s * w, mode)
            assert same_bits(got, base.roll(s * k, dims=-1).contiguous()), (s, h, w, k)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["scalar_ragged", "vector_x2", "vector_three_tiles", "one_pixel"])
def test_resize_between_guard_bands(name, mode, dt):
    """Input and result between poisoned guards: no store outside the result, no element left unwritten, the input untouched, and
    no guard NaN reaching the result through a wrapped or clamped tap (``check_case``: finite and within the tolerance)."""
    x = case(name, dt)
    _, (H, W) = CASES[name]
    g = Guarded(K)
    xg = g.guard(x.cuda())
    with g:
        got = g.out(K.resize_pano_latent(xg, H, W, mode))
    assert same_bits(xg.cpu(), x)
    check_case(name, dt, mode, got)


def test_resize_pano_latent_rejects_bad_arguments():
    dt = torch.bfloat16
    x = case("vector_x2", dt).cuda()
    (h, w), (H, W) = CASES["vector_x2"]
    with pytest.raises(TypeError, match="bfloat16/float16"):
        K.resize_pano_latent(x.float(), H, W)
    with pytest.raises(RuntimeError, match="need tensors on the MI355X"):
        K.resize_pano_latent(x.cpu(), H, W)
    with pytest.raises(ValueError, match="mode must be one of"):
        K.resize_pano_latent(x, H, W, "nearest")
    with pytest.raises(ValueError, match=r"x must be \[1, C, F, h, w\]"):
        K.resize_pano_latent(x[0], H, W)
    with pytest.raises(ValueError, match=r"x must be \[1, C, F, h, w\]"):
        K.resize_pano_latent(torch.cat([x, x]), H, W)
    with pytest.raises(TypeError, match="H and W must be ints"):
        K.resize_pano_latent(x, 8.0, W)
    with pytest.raises(ValueError, match="must not be empty"):
        K.resize_pano_latent(x[:, :, :0], H, W)
    with pytest.raises(ValueError, match="shrinks"):
        K.resize_pano_latent(x, h - 1, W)
    with pytest.raises(ValueError, match="shrinks"):
        K.resize_pano_latent(x, H, w - 1)
    with pytest.raises(ValueError, match="contiguous"):
        K.resize_pano_latent(x.transpose(3, 4).contiguous().transpose(3, 4), H, W)
    # the C entry point itself
    out = torch.full((1, C, F, H, W), 7.0, dtype=dt, device="cuda")
    before = out.clone()
    ptrs, sizes = [x.data_ptr(), out.data_ptr()], [C, F, h, w, H, W]
    fn, err = K.lib().im360_resize_pano_latent, K.lib().im360_last_error
    for i in range(2):
        bad = list(ptrs)
        bad[i] = None
        assert fn(*bad, *sizes, 1, 0, None) != 0 and b"null pointer" in err(), i
    for i in range(6):
        for v in (0, -3):
            bad = list(sizes)
            bad[i] = v
            assert fn(*ptrs, *bad, 1, 0, None) != 0 and b"must be positive" in err(), (i, v)
    assert fn(*ptrs, C, F, 1 << 31, w, 1 << 31, W, 1, 0, None) != 0 and b"2^31" in err()          # a row index
    assert fn(*ptrs, C, F, h, w, H, 1 << 28, 1, 0, None) != 0 and b"2^31" in err()                # a unit index inside a tile
    assert fn(*ptrs, 1 << 16, 1 << 15, h, w, H, W, 1, 0, None) != 0 and b"2^31" in err()          # the planes
    assert fn(*ptrs, 1 << 12, 1 << 12, h, w, H, W, 1, 0, None) != 0 and b"2^24 workgroups" in err()          # the grid: 2^32 threads
    assert fn(*ptrs, 1 << 12, 1 << 11, h, w, 16, W, 1, 0, None) != 0 and b"2^24 workgroups" in err()         # ... with its row tiles
    for i in range(2):
        bad = list(ptrs)
        bad[i] += 1
        assert fn(*bad, *sizes, 1, 0, None) != 0 and b"misaligned 16-bit tensor" in err(), i
    assert fn(ptrs[0], ptrs[0], *sizes, 1, 0, None) != 0 and b"x aliases out" in err()
    assert fn(*ptrs, C, F, h, w, h - 1, W, 1, 0, None) != 0 and b"shrinks" in err()
    assert fn(*ptrs, C, F, h, w, H, w - 1, 1, 0, None) != 0 and b"shrinks" in err()
    for m in (-1, 2):
        assert fn(*ptrs, *sizes, m, 0, None) != 0 and b"mode" in err() and b"unknown" in err(), m
    assert fn(*ptrs, *sizes, 1, 7, None) != 0 and b"dtype 7 unsupported" in err()
    torch.cuda.synchronize()
    assert same_bits(out, before) and same_bits(x.cpu(), case("vector_x2", dt))                   # no refused call wrote anything
    stream = torch.cuda.current_stream().cuda_stream
    assert fn(*ptrs, *sizes, 1, 0, stream) == 0                                                   # and the same arguments unbroken are accepted
    torch.cuda.synchronize()
    assert same_bits(out, K.resize_pano_latent(x, H, W, "bicubic"))


# ------------------------------------------------------------------------------------------------ the small pipeline
STEPS, STRENGTH = 3, 2 / 3


@pytest.fixture(scope="module")
def clips():
    """The clip at the size of the first pass and at twice that size."""
    return S.video_batch(frames=8, pano_hw=(256, 512), seed=2), S.video_batch(frames=8, pano_hw=(512, 1024), seed=2)


@pytest.fixture(scope="module")
def small_pipe():
    """The recipe of test_init_strength_gpu.py::small_pipe (8 frames, width-5 model, width-4 VAE, 3 steps), the clip an argument."""
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    cond = S.conditioning(frames=16, seed=2)

    def run(use_graph, clip, seed=33, **kw):
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
def first_call(small_pipe, clips):
    """The first pass: from pure noise at 256 x 512."""
    return small_pipe(True, clips[0])


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_hires_pass_graph_equals_eager(small_pipe, clips, first_call):
    x0 = first_call[1]
    assert x0.shape == (1, 4, 8, 32, 64)
    graphed = small_pipe(True, clips[1], init_latents=x0, strength=STRENGTH)
    eager = small_pipe(False, clips[1], init_latents=x0, strength=STRENGTH)
    big = K.resize_pano_latent(x0, 64, 128)
    errs = dict(graph_vs_eager_latent=rel(graphed[1], eager[1]), refined_vs_upscaled_init=rel(graphed[1], big))
    _record("hires_pass", **errs)
    assert _same(graphed, eager), errs
    assert graphed[0].shape == (1, 3, 8, 512, 1024) and graphed[1].shape == (1, 4, 8, 64, 128) and graphed[2].shape == (1, 20, 4, 8, 32, 32)
    assert all(torch.isfinite(v.float()).all() for v in graphed)
    assert not torch.equal(graphed[1], big)                                # two steps were run on it
    bilinear = small_pipe(True, clips[1], init_latents=x0, strength=STRENGTH, init_resize="bilinear")
    assert not torch.equal(bilinear[1], graphed[1]) and torch.isfinite(bilinear[0]).all()


def test_hires_pass_keeps_the_upscaled_clean_latent_under_a_mask(small_pipe, clips, first_call):
    """Half of the panorama kept (even frames: the left half; odd frames: a rectangle across the seam): the kept region of the result is
    the UPSCALED clean latent bit for bit, graph replay as the eager loop."""
    x0 = first_call[1]
    m = half_mask(8, 512, 1024)
    k = kept(m, 64, 128).expand(1, 4, -1, -1, -1).cuda()
    assert k.any() and not k.all() and k[0, 0, 1, 32, 0] and k[0, 0, 1, 32, -1]
    graphed = small_pipe(True, clips[1], init_latents=x0, strength=STRENGTH, regenerate_mask=m)
    eager = small_pipe(False, clips[1], init_latents=x0, strength=STRENGTH, regenerate_mask=m)
    big = K.resize_pano_latent(x0, 64, 128)
    assert _same(graphed, eager)
    assert same_bits(graphed[1][k], big[k]) and not torch.equal(graphed[1][~k], big[~k])
    assert all(torch.isfinite(v.float()).all() for v in graphed)


def test_a_call_without_an_init_at_the_small_size_afterwards_is_the_first_call(small_pipe, clips, first_call):
    """No state leaks from the runs at the large size (this file's order: after them) into a run from pure noise at the small one."""
    assert _same(small_pipe(True, clips[0]), first_call)
