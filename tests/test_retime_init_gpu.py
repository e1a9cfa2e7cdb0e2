"""The frame-interpolation pass on the MI355X: ``kernels.retime_pano_latent`` (csrc/retime_latents.hip) against the fp64 definition
``pano_geometry.retime_pano_latent`` per element on every path of its launcher, its bit contracts (16-byte and scalar stores give the same
bits, keyframes are the source frames, a roll of a ring is a roll of the result, equal frame counts return the input), the same cases
between guard bands, the refusals of the wrapper and of the C entry point, and the small pipeline: a clip of 8 frames generated at
128 x 256 retimed to 15 frames and refined in windows of 8, graph replay against the eager loop, with ``keyframe_mask``, as a ring of 16
frames, from an init that is smaller as well, and a call of the first kind afterwards."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from _emu_retime_latents import C, CASES, MODES, case, reference, same_bits, worst_ratio  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record as _record, rel  # noqa: E402
from imagine360_amd import configs, context, kernels as K, synthetic as S  # noqa: E402
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
    f, F, (h, w), loop = CASES[name]
    assert got.shape == (1, C, F, h, w) and got.dtype == dt
    assert torch.isfinite(got.float()).all(), name
    ratio = worst_ratio(got, reference(name, dt, mode), x, dt)
    print("retime_pano_latent", name, dt, mode, "worst |error| / tolerance", ratio, flush=True)
    assert ratio < 1.0, (name, mode, ratio)
    keys = context.keyframe_frames(f, F, loop)
    src = [j * f // F if loop else j * (f - 1) // max(F - 1, 1) for j in keys]
    assert same_bits(got[:, :, keys].cpu(), x[:, :, src].contiguous()), (name, mode)               # (the identity: every frame)
    return ratio


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_retime_pano_latent_parity(dt):
    """Per element within 0.5 ulp_T(reference) + 2^-17 max|x| of the fp64 definition, both modes, every case: once on 16-byte aligned
    input (the 16-byte path where hw % 8 == 0) and once with the input one element off its alignment (the scalar path) -- the same
    bits."""
    worst = {}
    for mode in MODES:
        for name, (f, F, (h, w), loop) in CASES.items():
            x = case(name, dt).cuda()
            assert x.data_ptr() % 16 == 0
            got = K.retime_pano_latent(x, F, mode, loop)
            worst[f"{name}_{mode}"] = check_case(name, dt, mode, got)
            off = K.retime_pano_latent(off_alignment(x), F, mode, loop)
            worst[f"{name}_{mode}_off"] = check_case(name, dt, mode, off)
            assert got.data_ptr() % 16 == 0 and same_bits(got, off), (name, mode)
    _record(f"retime_pano_latent_{str(dt).split('.')[-1]}", worst_ratio=max(worst.values()), **worst)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", MODES)
def test_keyframes_are_the_source_frames_bit_for_bit(mode, dt):
    """NaN and -0.0 planted in a source frame: a keyframe is a copy on both store paths (hw = 32 and hw = 15), the identity too."""
    g = torch.Generator().manual_seed(43)
    for h, w in ((4, 8), (3, 5)):
        x = (1.5 * torch.randn(1, C, 4, h, w, generator=g)).to(dt)
        x[0, 0, 1, 0, 0], x[0, 1, 1, 2, 4], x[0, 2, 2, 1, 1] = float("nan"), -0.0, float("nan")
        xd = x.cuda()
        for F, loop in ((7, False), (8, True), (10, False), (4, False), (4, True)):
            got = K.retime_pano_latent(xd, F, mode, loop)
            keys = context.keyframe_frames(4, F, loop)
            src = [j * 4 // F if loop else j * 3 // (F - 1) for j in keys]
            assert len(keys) == 4 and same_bits(got[:, :, keys].cpu(), x[:, :, src].contiguous()), (h, w, F, loop)
            assert torch.isfinite(got[0, 3].float()).all()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", MODES)
def test_rolling_a_ring_rolls_the_result_bit_for_bit(mode, dt):
    """Integer scales 2 and 3: t is periodic in the output frame and the taps wrap, so the loop point is a frame like every other.  On
    the 16-byte path (hw = 32) and on the scalar one (hw = 15)."""
    g = torch.Generator().manual_seed(41)
    for s, (h, w) in ((2, (4, 8)), (3, (4, 8)), (3, (3, 5))):
        x = (1.5 * torch.randn(1, C, 5, h, w, generator=g)).to(dt).cuda()
        base = K.retime_pano_latent(x, s * 5, mode, True)
        for k in (1, 2, 4):
            got = K.retime_pano_latent(x.roll(k, dims=2).contiguous(), s * 5, mode, True)
            assert same_bits(got, base.roll(s * k, dims=2).contiguous()), (s, h, w, k)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["vector_keyframes", "scalar_keyframes", "ring_ragged", "one_frame", "one_frame_ring", "vector_two_tiles",
                                  "scalar_two_tiles"])
def test_retime_between_guard_bands(name, mode, dt):
    """Input and result between poisoned guards: no store outside the result, no element left unwritten, the input untouched, and
    no guard NaN reaching the result through a clamped or wrapped tap (``check_case``: finite and within the tolerance)."""
    x = case(name, dt)
    _, F, _, loop = CASES[name]
    g = Guarded(K)
    xg = g.guard(x.cuda())
    with g:
        got = g.out(K.retime_pano_latent(xg, F, mode, loop))
    assert same_bits(xg.cpu(), x)
    check_case(name, dt, mode, got)


def test_retime_pano_latent_rejects_bad_arguments():
    dt = torch.bfloat16
    x = case("vector_keyframes", dt).cuda()
    f, F, (h, w), _ = CASES["vector_keyframes"]
    with pytest.raises(TypeError, match="bfloat16/float16"):
        K.retime_pano_latent(x.float(), F)
    with pytest.raises(RuntimeError, match="need tensors on the MI355X"):
        K.retime_pano_latent(x.cpu(), F)
    with pytest.raises(ValueError, match="mode must be one of"):
        K.retime_pano_latent(x, F, "bicubic")
    with pytest.raises(ValueError, match=r"x must be \[1, C, f, h, w\]"):
        K.retime_pano_latent(x[0], F)
    with pytest.raises(ValueError, match=r"x must be \[1, C, f, h, w\]"):
        K.retime_pano_latent(torch.cat([x, x]), F)
    for bad in (3.0, True):
        with pytest.raises(TypeError, match="F must be an int"):
            K.retime_pano_latent(x, bad)
    with pytest.raises(ValueError, match="must not be empty"):
        K.retime_pano_latent(x[:, :, :0], F)
    with pytest.raises(ValueError, match="shrinks"):
        K.retime_pano_latent(x, f - 1)
    with pytest.raises(ValueError, match="contiguous"):
        K.retime_pano_latent(x.transpose(3, 4).contiguous().transpose(3, 4), F)
    # the C entry point itself
    out = torch.full((1, C, F, h, w), 7.0, dtype=dt, device="cuda")
    before = out.clone()
    ptrs, sizes = [x.data_ptr(), out.data_ptr()], [C, f, F, h * w]
    fn, err = K.lib().im360_retime_pano_latent, K.lib().im360_last_error
    for i in range(2):
        bad = list(ptrs)
        bad[i] = None
        assert fn(*bad, *sizes, 1, 0, 0, None) != 0 and b"null pointer" in err(), i
    for i in range(4):
        for v in (0, -3):
            bad = list(sizes)
            bad[i] = v
            assert fn(*ptrs, *bad, 1, 0, 0, None) != 0 and b"must be positive" in err(), (i, v)
    assert fn(*ptrs, C, 1 << 31, 1 << 31, h * w, 1, 0, 0, None) != 0 and b"2^31" in err()          # a frame index
    assert fn(*ptrs, C, f, F, (1 << 31) - 4096, 1, 0, 0, None) != 0 and b"2^31" in err()          # an element index inside the last tile
    assert fn(*ptrs, 1 << 16, f, 1 << 15, h * w, 1, 0, 0, None) != 0 and b"2^31" in err()         # the (channel, frame) pairs
    assert fn(*ptrs, 1 << 12, f, 1 << 12, h * w, 1, 0, 0, None) != 0 and b"2^24 workgroups" in err()        # the grid: 2^32 threads
    assert fn(*ptrs, 1 << 12, f, 1 << 11, 4097, 1, 0, 0, None) != 0 and b"2^24 workgroups" in err()         # ... with its tiles
    for i in range(2):
        bad = list(ptrs)
        bad[i] += 1
        assert fn(*bad, *sizes, 1, 0, 0, None) != 0 and b"misaligned 16-bit tensor" in err(), i
    assert fn(ptrs[0], ptrs[0], *sizes, 1, 0, 0, None) != 0 and b"x aliases out" in err()
    assert fn(*ptrs, C, f, f - 1, h * w, 1, 0, 0, None) != 0 and b"shrinks" in err()
    for m in (-1, 2):
        assert fn(*ptrs, *sizes, m, 0, 0, None) != 0 and b"mode" in err() and b"unknown" in err(), m
        assert fn(*ptrs, *sizes, 1, m, 0, None) != 0 and b"loop" in err() and b"unknown" in err(), m
    assert fn(*ptrs, *sizes, 1, 0, 7, None) != 0 and b"dtype 7 unsupported" in err()
    torch.cuda.synchronize()
    assert same_bits(out, before) and same_bits(x.cpu(), case("vector_keyframes", dt))            # no refused call wrote anything
    stream = torch.cuda.current_stream().cuda_stream
    assert fn(*ptrs, *sizes, 1, 0, 0, stream) == 0                                                # and the same arguments unbroken are accepted
    torch.cuda.synchronize()
    assert same_bits(out, K.retime_pano_latent(x, F, "cubic"))


# ------------------------------------------------------------------------------------------------ the small pipeline
STEPS, STRENGTH = 4, 0.5                 # two of four steps are run
WINDOWS = dict(context_frames=8, context_overlap=4)


@pytest.fixture(scope="module")
def clips():
    """The clip of the first pass (8 frames), of the interpolation pass (15 = 2 * 8 - 1) and of the looping one (16 = 2 * 8), all at
    128 x 256 pixels: a 16 x 32 latent."""
    return {n: S.video_batch(frames=n, pano_hw=(128, 256), seed=2) for n in (8, 15, 16)}


@pytest.fixture(scope="module")
def small_pipe():
    """The recipe of test_hires_init_gpu.py::small_pipe (width-5 model, width-4 VAE), the clip an argument."""
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    cond = S.conditioning(frames=16, seed=2)

    def run(use_graph, clip, seed=33, **kw):
        if "init_latents" in kw:
            kw.setdefault("init_retime", "linear")                           # (opt-in: without the keyword a short init is refused)
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
    """The first pass: 8 frames from pure noise."""
    return small_pipe(True, clips[8])


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_interpolation_pass_graph_equals_eager(small_pipe, clips, first_call):
    x0 = first_call[1]
    assert x0.shape == (1, 4, 8, 16, 32)
    graphed = small_pipe(True, clips[15], init_latents=x0, strength=STRENGTH, **WINDOWS)
    eager = small_pipe(False, clips[15], init_latents=x0, strength=STRENGTH, **WINDOWS)
    long = K.retime_pano_latent(x0, 15)
    errs = dict(graph_vs_eager_latent=rel(graphed[1], eager[1]), refined_vs_retimed_init=rel(graphed[1], long))
    _record("interpolation_pass", **errs)
    assert _same(graphed, eager), errs
    assert graphed[0].shape == (1, 3, 15, 128, 256) and graphed[1].shape == (1, 4, 15, 16, 32) and graphed[2].shape[3] == 15
    assert all(torch.isfinite(v.float()).all() for v in graphed)
    assert not torch.equal(graphed[1], long)                               # two steps were run on it
    by_hand = small_pipe(True, clips[15], init_latents=long, strength=STRENGTH, **WINDOWS)
    assert _same(graphed, by_hand)                                          # the RNG order: the run from the init retimed by hand
    cubic = small_pipe(True, clips[15], init_latents=x0, strength=STRENGTH, init_retime="cubic", **WINDOWS)
    assert not torch.equal(cubic[1], graphed[1]) and torch.isfinite(cubic[0]).all()


def test_interpolation_pass_keeps_the_source_frames_under_the_keyframe_mask(small_pipe, clips, first_call):
    """True frame interpolation: the even frames of the result are the 8 source frames bit for bit, graph replay as the eager loop."""
    x0 = first_call[1]
    m = context.keyframe_mask(8, 15)
    graphed = small_pipe(True, clips[15], init_latents=x0, strength=STRENGTH, regenerate_mask=m, **WINDOWS)
    eager = small_pipe(False, clips[15], init_latents=x0, strength=STRENGTH, regenerate_mask=m, **WINDOWS)
    long = K.retime_pano_latent(x0, 15)
    assert _same(graphed, eager)
    assert same_bits(graphed[1][:, :, 0::2].contiguous(), x0) and not torch.equal(graphed[1][:, :, 1::2], long[:, :, 1::2])
    assert all(torch.isfinite(v.float()).all() for v in graphed)


def test_looping_interpolation_pass_retimes_on_the_ring(small_pipe, clips, first_call):
    x0 = first_call[1]
    m = context.keyframe_mask(8, 16, loop=True)
    kw = dict(init_latents=x0, strength=STRENGTH, regenerate_mask=m, context_loop=True, **WINDOWS)
    graphed = small_pipe(True, clips[16], **kw)
    eager = small_pipe(False, clips[16], **kw)
    assert _same(graphed, eager)
    assert graphed[1].shape == (1, 4, 16, 16, 32) and all(torch.isfinite(v.float()).all() for v in graphed)
    assert same_bits(graphed[1][:, :, 0::2].contiguous(), x0)
    by_hand = small_pipe(True, clips[16], **dict(kw, init_latents=K.retime_pano_latent(x0, 16, "linear", True)))
    assert _same(graphed, by_hand)


def test_smaller_and_shorter_init_is_retimed_then_resized(small_pipe, clips, first_call):
    small = first_call[1][..., ::2, ::2].contiguous()                       # [1, 4, 8, 8, 16]
    got = small_pipe(True, clips[15], init_latents=small, strength=STRENGTH, **WINDOWS)
    by_hand = small_pipe(True, clips[15], init_latents=K.resize_pano_latent(K.retime_pano_latent(small, 15), 16, 32), strength=STRENGTH, **WINDOWS)
    assert _same(got, by_hand) and got[1].shape == (1, 4, 15, 16, 32) and all(torch.isfinite(v.float()).all() for v in got)


def test_a_call_without_an_init_afterwards_is_the_first_call(small_pipe, clips, first_call):
    """No state leaks from the interpolation passes (this file's order: after them) into a run from pure noise."""
    assert _same(small_pipe(True, clips[8]), first_call)
