"""The frame-interpolation pass (an init clip with fewer frames than the run, ``init_retime``) on CPU: the eager definition
``pano_geometry.retime_pano_latent`` against torch's ``align_corners=True`` interpolation along the frame axis, its ring form against the
open form on a padded clip, its keyframes (copies, bit for bit), its roll equivariance on a ring, ``context.keyframe_frames`` /
``keyframe_mask``, the stand-in's fp32 evaluation against the tolerance the GPU test holds the kernel to, and the pipeline's host logic
under emulated kernels: the one retime in front of the resize and of ``noise_latents``, ``loop`` following ``context_loop``, the unchanged
RNG order, ``init_video`` with fewer frames, ``regenerate_mask=keyframe_mask(...)`` keeping the source frames, zero calls at an equal
frame count, and the refusals."""
import contextlib
import random

import pytest
import torch
import torch.nn.functional as F

import _emu_ddim_step as ES
import _emu_keep_latents as EK
import _emu_kernels as E
import _emu_noise_latents as EN
import _emu_resize_latents as ER
import _emu_retime_latents as ET
import _emu_ring_step as EG
from imagine360_amd import configs, context, pano_geometry as G, synthetic as S
from imagine360_amd.scheduler import DDIMScheduler

torch.set_grad_enabled(False)

PAIRS = [(2, 3), (3, 5), (4, 7), (3, 8), (5, 6), (8, 15)]
INT_VIEW = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    return t.contiguous().view(INT_VIEW[t.element_size()])


# ------------------------------------------------------------------------------------------------ 1. the eager definition
@pytest.mark.parametrize("mode", ET.MODES)
@pytest.mark.parametrize("f,n", PAIRS)
def test_open_clip_is_torch_align_corners_interpolation_along_the_frame_axis(f, n, mode):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 3, f, 4, 5, generator=g, dtype=torch.float64)
    if mode == "linear":
        want = F.interpolate(x, size=(n, 4, 5), mode="trilinear", align_corners=True)
    else:
        rows = x.permute(0, 1, 3, 4, 2).reshape(1, 3 * 4 * 5, f, 1)                               # the frame axis as an image's rows
        want = F.interpolate(rows, size=(n, 1), mode="bicubic", align_corners=True).reshape(1, 3, 4, 5, n).permute(0, 1, 4, 2, 3)
    got = G.retime_pano_latent(x, n, mode)
    err = float((got - want).abs().max())
    print("retime definition vs torch", f, n, mode, err)
    assert got.shape == want.shape == (1, 3, n, 4, 5) and got.dtype == torch.float64 and err < 1e-12
    # ... which half-pixel centres do not give: they preserve no frame
    if f > 2:                                                               # (2 -> 3 is the one ratio at which the two agree)
        half = F.interpolate(x, size=(n, 4, 5), mode="trilinear", align_corners=False)
        assert float((half - want).abs().max()) > 1e-3


@pytest.mark.parametrize("f,n", PAIRS)
def test_ring_linear_is_the_open_clip_with_frame_0_appended(f, n):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, f, 4, 5, generator=g, dtype=torch.float64)
    closed = torch.cat([x, x[:, :, :1]], dim=2)
    assert torch.equal(G.retime_pano_latent(x, n, "linear", loop=True), G.retime_pano_latent(closed, n + 1, "linear")[:, :, :n])


@pytest.mark.parametrize("f,n", PAIRS + [(4, 8), (3, 9)])
def test_ring_cubic_is_the_open_form_on_a_circularly_padded_clip(f, n):
    """The clip padded circularly by one whole turn in front and one and a frame behind, 3 f + 1 -> 3 n + 1 frames: the open form has
    the ring's source time there, j' f / n, and output frame n + j reads the taps i0 - 1 .. i0 + 2 of ring frame j, one turn on, none
    of them clamped.  With an integer scale s a pad of 2 frames on either side is enough: f + 4 -> s (f + 3) + 1, read at 2 s + j."""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, 3, f, 4, 5, generator=g, dtype=torch.float64)
    ring = G.retime_pano_latent(x, n, "cubic", loop=True)
    turns = x[:, :, torch.arange(3 * f + 1) % f]
    assert torch.equal(ring, G.retime_pano_latent(turns, 3 * n + 1, "cubic")[:, :, n:2 * n])
    if n % f == 0:
        s = n // f
        padded = x[:, :, (torch.arange(f + 4) - 2) % f]
        got = G.retime_pano_latent(padded, s * (f + 3) + 1, "cubic")[:, :, 2 * s:2 * s + n]
        assert float((got - ring).abs().max()) < 1e-12


@pytest.mark.parametrize("dt", [torch.float64, torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", ET.MODES)
def test_keyframes_are_the_source_frames_bit_for_bit(mode, dt):
    """NaN and -0.0 planted in a source frame: a keyframe is a copy, no weighted sum (0 * NaN) is formed there -- and the identity."""
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 4, 4, 3, 5, generator=g).to(dt)
    x[0, 0, 1, 0, 0], x[0, 1, 1, 2, 4], x[0, 2, 2, 1, 1] = float("nan"), -0.0, float("nan")
    for n, loop in ((7, False), (8, True), (10, False), (12, True), (4, False), (4, True)):
        got = G.retime_pano_latent(x, n, mode, loop)
        keys = context.keyframe_frames(4, n, loop)
        src = [j * 4 // n if loop else j * 3 // (n - 1) for j in keys]
        assert got.dtype == dt and got.shape == (1, 4, n, 3, 5) and len(keys) == 4
        assert torch.equal(bits(got[:, :, keys]), bits(x[:, :, src])), (n, loop)
        # the NaNs stay where the taps reach: the frames next to the keyframe in time, nothing at the other end of the clip
        assert torch.isfinite(got[0, 3].float()).all()
    assert torch.equal(bits(G.retime_pano_latent(x, 4, mode)), bits(x))


def test_keyframe_frames_and_mask():
    assert context.keyframe_frames(4, 7) == [0, 2, 4, 6] and context.keyframe_frames(8, 15) == list(range(0, 15, 2))
    assert context.keyframe_frames(4, 8, loop=True) == [0, 2, 4, 6] and context.keyframe_frames(3, 9, loop=True) == [0, 3, 6]
    assert context.keyframe_frames(3, 8) == [0, 7] and context.keyframe_frames(5, 6) == [0, 5]       # ragged: the end frames alone
    assert context.keyframe_frames(3, 7, loop=True) == [0] and context.keyframe_frames(4, 8) == [0, 7]
    assert context.keyframe_frames(1, 4) == [0, 1, 2, 3] and context.keyframe_frames(5, 5) == list(range(5))
    assert context.keyframe_frames(1, 1) == [0]
    with pytest.raises(ValueError, match="1 <= f <= F"):
        context.keyframe_frames(5, 4)
    # the frames the definition copies are these frames
    for f, n, loop in ((4, 7, False), (4, 8, True), (3, 8, False), (3, 7, True), (6, 16, False), (6, 16, True)):
        _, _, key = G._retime_taps(f, n, "cubic", loop, torch.float32, "cpu")
        assert key.nonzero().flatten().tolist() == context.keyframe_frames(f, n, loop)
    m = context.keyframe_mask(4, 7)
    assert m.shape == (1, 7, 1, 1, 1) and m.dtype == torch.float32 and m.flatten().tolist() == [0, 1, 0, 1, 0, 1, 0]
    assert context.keyframe_mask(3, 6, loop=True).flatten().tolist() == [0, 1, 0, 1, 0, 1]


@pytest.mark.parametrize("mode", ET.MODES)
@pytest.mark.parametrize("s", [2, 3])
def test_rolling_a_ring_rolls_the_result_bit_for_bit(s, mode):
    """fp32, integer scales: t is periodic in the output frame, so a roll by k frames is a roll by s k frames of the same bits."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 4, 5, 3, 8, generator=g)
    base = G.retime_pano_latent(x, s * 5, mode, loop=True)
    for k in (1, 2, 4):
        assert torch.equal(G.retime_pano_latent(x.roll(k, dims=2), s * 5, mode, loop=True), base.roll(s * k, dims=2)), k


def test_definition_refusals():
    x = torch.zeros(1, 4, 4, 6, 9)
    with pytest.raises(ValueError, match="shrinks"):
        G.retime_pano_latent(x, 3)
    with pytest.raises(ValueError, match="mode must be one of"):
        G.retime_pano_latent(x, 7, "bicubic")
    for bad in (7.0, True, "7"):
        with pytest.raises(TypeError, match="F must be an int"):
            G.retime_pano_latent(x, bad)
    assert G.RETIME_MODES == ("linear", "cubic")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mode", ET.MODES)
def test_fp32_evaluation_is_inside_the_kernel_tolerance(mode, dt):
    """The stand-in (the definition in fp32, one rounding to T) against the fp64 definition on the shared cases: inside the bound the
    kernel is held to on the GPU; the identity case returns the input's bits."""
    worst = {}
    for name, (f, n, (h, w), loop) in ET.CASES.items():
        x = ET.case(name, dt)
        got = ET.retime_pano_latent(x, n, mode, loop)
        assert got.shape == (1, ET.C, n, h, w) and got.dtype == dt
        worst[name] = ET.worst_ratio(got, ET.reference(name, dt, mode), x, dt)
    print("retime fp32 evaluation / tolerance", mode, dt, worst)
    assert max(worst.values()) < 1.0, worst
    assert ET.same_bits(ET.retime_pano_latent(ET.case("identity", dt), 4, mode), ET.case("identity", dt))
    # the cases are on the sides of the launcher's choices they say they are
    hw = {k: v[2][0] * v[2][1] for k, v in ET.CASES.items()}
    assert all((hw[k] % 8 == 0) == (not k.startswith("scalar") and k != "ring_ragged") for k in hw)
    assert ET.TILE < hw["vector_two_tiles"] < 2 * ET.TILE and ET.TILE < hw["scalar_two_tiles"] < 2 * ET.TILE
    assert 256 * 8 < hw["vector_looped"] <= ET.TILE


# ------------------------------------------------------------------------------------------------ 2. the pipeline's host logic
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
def clip5():
    """The run: 5 frames (2 * 3 - 1) at 128 x 256 pixels, a 16 x 32 latent."""
    return S.video_batch(frames=5, pano_hw=(128, 256), seed=6), S.conditioning(frames=16, seed=6)


@pytest.fixture(scope="module")
def clip6():
    """A looping run: 6 frames (2 * 3)."""
    return S.video_batch(frames=6, pano_hw=(128, 256), seed=6), S.conditioning(frames=16, seed=6)


def pipe_kw(cond, vb, steps, **extra):
    extra.setdefault("init_retime", "linear")                               # (opt-in: without the keyword a short init is refused)
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
    """Every emulated kernel; yields (order, starts, retimes, resizes, keeps): the records of noise_latents, retime_pano_latent,
    resize_pano_latent and keep_latents, and ``order``, the names of the first three in the order they were called."""
    from imagine360_amd import kernels
    with contextlib.ExitStack() as st:
        for cm in (E.patched_kernels(), ES.patched_step_kernel(), EG.patched_ring_kernels()):          # (windows on a line and on a ring)
            st.enter_context(cm)
        starts, retimes = st.enter_context(EN.patched_noise_latents()), st.enter_context(ET.patched_retime_pano_latent())
        resizes, keeps = st.enter_context(ER.patched_resize_pano_latent()), st.enter_context(EK.patched_keep_latents())
        order = []

        def logged(name):
            fn = getattr(kernels, name)

            def call(*a, **k):
                order.append(name)
                return fn(*a, **k)
            setattr(kernels, name, call)
            st.callback(setattr, kernels, name, fn)
        for name in ("noise_latents", "retime_pano_latent", "resize_pano_latent"):
            logged(name)
        yield order, starts, retimes, resizes, keeps


@pytest.fixture(scope="module")
def short_init():
    """A clean latent of 3 frames at the run's size, [1, 4, 3, 16, 32]."""
    g = torch.Generator().manual_seed(12)
    return 0.5 * torch.randn(1, 4, 3, 16, 32, generator=g)


def test_short_init_is_retimed_once_in_front_of_noise_latents(cpu_pipe, clip5, short_init):
    """The start latents are ``noise_latents(retime(x0))`` bit for bit, on the panorama noise an init of the run's frame count draws from
    the same seed (the RNG order is unchanged); such an init makes no retime call and, given the retimed latent, the same run."""
    vb, cond = clip5
    with patches() as (order, starts, retimes, resizes, keeps):
        vid, lat = _run(cpu_pipe, **pipe_kw(cond, vb, 3, init_latents=short_init, strength=2 / 3))
        assert order == ["retime_pano_latent", "noise_latents"] and len(retimes) == 1 and resizes == [] and keeps == []
        x, n, mode, loop, long = retimes[0]
        assert (n, mode, loop) == (5, "linear", False) and torch.equal(x, short_init) and long.shape == (1, 4, 5, 16, 32)
        assert torch.equal(long, G.retime_pano_latent(short_init, 5, "linear"))
        assert torch.equal(long[:, :, [0, 2, 4]], short_init)
        torch.manual_seed(3)
        noise = torch.randn(1, 5, 1, 4, 16, 32).squeeze(2)                   # init_noise's draw, the first of the call
        host = cpu_pipe.scheduler._timesteps_host
        idx, ok = G.nearest_e2p_index(16, 32, vb["pers_size"] // 8, vb["pers_size"] // 8, vb["cameras"])
        want = EN.noise_latents(long, noise, idx.to(torch.int32), ok.to(torch.uint8), *cpu_pipe.scheduler.noise_coefficients(host[1]))
        assert torch.equal(starts[0][0], want[0]) and torch.equal(starts[0][1], want[1])
        assert vid.shape == (1, 3, 5, 128, 256) and torch.isfinite(vid).all() and lat[0].shape == (1, 4, 5, 16, 32)
        del order[:], starts[:], retimes[:]
        vid2, lat2 = _run(cpu_pipe, **pipe_kw(cond, vb, 3, init_latents=long, strength=2 / 3))
        assert retimes == [] and order == ["noise_latents"]                 # an equal frame count: the new code is not called at all
        assert torch.equal(starts[0][0], want[0]) and torch.equal(vid, vid2) and torch.equal(lat[0], lat2[0]) and torch.equal(lat[1], lat2[1])
        # cubic on request
        del retimes[:]
        _, lat3 = _run(cpu_pipe, **pipe_kw(cond, vb, 3, init_latents=short_init, strength=2 / 3, init_retime="cubic"))
        assert [c[1:4] for c in retimes] == [(5, "cubic", False)] and not torch.equal(lat3[0], lat[0])


def test_short_and_small_init_is_retimed_then_resized(cpu_pipe, clip5, short_init):
    vb, cond = clip5
    small = short_init[..., ::2, ::2].contiguous()                           # [1, 4, 3, 8, 16]
    with patches() as (order, starts, retimes, resizes, _):
        _run(cpu_pipe, **pipe_kw(cond, vb, 2, init_latents=small, strength=0.5, init_resize="bilinear"))
        assert order == ["retime_pano_latent", "resize_pano_latent", "noise_latents"] and len(retimes) == len(resizes) == len(starts) == 1
        assert torch.equal(retimes[0][0], small) and retimes[0][1:4] == (5, "linear", False) and retimes[0][4].shape == (1, 4, 5, 8, 16)
        assert torch.equal(resizes[0][0], retimes[0][4]) and resizes[0][1:4] == (16, 32, "bilinear")
        assert resizes[0][4].shape == (1, 4, 5, 16, 32)


def test_loop_follows_context_loop(cpu_pipe, clip6, short_init):
    """A looping run of 6 = 2 * 3 frames: the retime is the ring's, frame 5 a blend of source frames 2 and 0."""
    vb, cond = clip6
    with patches() as (order, starts, retimes, _, _):
        _, lat = _run(cpu_pipe, **pipe_kw(cond, vb, 2, init_latents=short_init, strength=0.5, context_frames=4, context_overlap=2,
                                          context_loop=True))
        assert order == ["retime_pano_latent", "noise_latents"] and retimes[0][1:4] == (6, "linear", True)
        ring = retimes[0][4]
        assert torch.equal(ring, G.retime_pano_latent(short_init, 6, "linear", loop=True))
        assert torch.equal(ring[:, :, 5], 0.5 * short_init[:, :, 2] + 0.5 * short_init[:, :, 0])
        assert lat[0].shape == (1, 4, 6, 16, 32) and torch.isfinite(lat[0]).all()
        del retimes[:]
        _run(cpu_pipe, **pipe_kw(cond, vb, 2, init_latents=short_init, strength=0.5, context_frames=4, context_overlap=2))
        assert retimes[0][1:4] == (6, "linear", False)                       # windows on a line: an open clip


def test_short_init_video_takes_the_same_path(cpu_pipe, clip5):
    """The clip is encoded at its own frame count (the posterior's mode, nothing drawn), then retimed: the call with ``init_latents`` =
    its encoding."""
    vb, cond = clip5
    video = S.video_batch(frames=3, pano_hw=(128, 256), seed=8)["pano_pixel_values"]            # [1, 3, 3, 128, 256]
    with patches() as (_, starts, retimes, resizes, _):
        x0 = cpu_pipe.encode_init_video(video)
        assert x0.shape == (1, 4, 3, 16, 32)
        _, a = _run(cpu_pipe, **pipe_kw(cond, vb, 2, init_video=video, strength=0.5))
        assert len(retimes) == 1 and torch.equal(retimes[0][0], x0) and retimes[0][1:4] == (5, "linear", False) and resizes == []
        _, b = _run(cpu_pipe, **pipe_kw(cond, vb, 2, init_latents=x0, strength=0.5))
        assert len(retimes) == 2 and torch.equal(starts[0][0], starts[1][0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("windows", [{}, dict(context_frames=3, context_overlap=1)], ids=["one_block", "windows"])
def test_keyframe_mask_keeps_the_source_frames(cpu_pipe, clip5, short_init, windows):
    """Frame interpolation: the source frames of ``last_latents[0]`` are the init's frames bit for bit, the in-betweens are denoised."""
    vb, cond = clip5
    mask = context.keyframe_mask(3, 5)
    with patches() as (_, _, retimes, _, keeps):
        _, got = _run(cpu_pipe, **pipe_kw(cond, vb, 3, init_latents=short_init, strength=2 / 3, regenerate_mask=mask, **windows))
        assert len(retimes) == 1 and len(keeps) == 2
        long = retimes[0][4]
    assert torch.equal(got[0][:, :, [0, 2, 4]], short_init)
    assert not torch.equal(got[0][:, :, 1], long[:, :, 1]) and not torch.equal(got[0][:, :, 3], long[:, :, 3])


def test_bad_inits_are_refused(cpu_pipe, clip5, short_init):
    from imagine360_amd.dist import FrameShard
    vb, cond = clip5
    kw = lambda **extra: pipe_kw(cond, vb, 3, strength=2 / 3, **extra)
    with patches() as (order, *_):
        with pytest.raises(ValueError, match="init_retime must be None or one of.*'nearest'"):
            cpu_pipe("synthetic", **kw(init_latents=short_init, init_retime="nearest"))
        with pytest.raises(ValueError, match=r"\[1, 4, 5, 16, 32\].*with fewer frames.*got \(1, 4, 6, 16, 32\)"):
            cpu_pipe("synthetic", **kw(init_latents=torch.zeros(1, 4, 6, 16, 32)))              # more frames than the run
        with pytest.raises(ValueError, match="with fewer frames"):
            cpu_pipe("synthetic", **kw(init_video=torch.zeros(1, 6, 3, 128, 256)))
        with pytest.raises(ValueError, match="with fewer frames"):
            cpu_pipe("synthetic", **kw(init_latents=short_init[:, :, :0]))                      # no frame at all
        bare = {k: v for k, v in kw(init_latents=short_init).items() if k != "init_retime"}
        for off in (bare, dict(bare, init_retime=None)):                    # without the keyword, the default, a short init is refused as ever
            with pytest.raises(ValueError, match=r"with init_retime=.*with fewer frames.*got \(1, 4, 3, 16, 32\)"):
                cpu_pipe("synthetic", **off)
        with pytest.raises(ValueError, match="cannot be combined with frame_shard.*not implemented"):
            cpu_pipe("synthetic", **kw(init_latents=short_init, frame_shard=FrameShard(5, rank=0, world=1)))
        assert order == []
