"""FreeInit passes on the MI355X: ``kernels.free_init_noise`` (csrc/free_init.hip) against the fp64 definition on the fp32-rounded
operators within the derived per-element bound of ``_emu_free_init`` on every shared case, aligned and one element off alignment (the
same bits), its exact properties (identity operators return n1's bits, a NaN reaches everything it is summed into), the cases between
guard bands, the refusals of the wrapper and of the C entry point, and the small pipeline: two passes graph replay against the eager loop,
one pass is the call without the keyword, windows on a line and on a ring, DPM-Solver++ 2M, guidance rescale, and a plain call after."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from _emu_free_init import C, CASES, SA, SB, case, same_bits, worst_ratio  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record as _record  # noqa: E402
from imagine360_amd import configs, kernels as K, synthetic as S  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402

torch.set_grad_enabled(False)


def off_alignment(t):
    """A contiguous copy of ``t`` that starts one element past a 256-byte aligned address: the launcher takes the scalar path."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size()
    return view


def check_case(name, dt, got):
    F, h, w = CASES[name][:3]
    assert got.shape == (1, F, C, h, w) and got.dtype == torch.float32
    assert torch.isfinite(got).all(), name
    ratio = worst_ratio(got, name, dt)
    print("free_init_noise", name, dt, "worst |error| / bound", ratio, flush=True)
    assert ratio < 1.0, (name, ratio)
    return ratio


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_free_init_noise_parity(dt):
    """Per element within (F + h + w + 16) 2^-24 T / sb + 2^-24 |ref| of the fp64 reference, every case: once on aligned inputs (the
    16-byte path where w % 4 == 0) and once with x0, n1 and n2 one element off their alignment (the scalar path) -- the same bits."""
    worst = {}
    for name in CASES:
        x0, n1, n2, Lf, Lh, Lw = (t.cuda() for t in case(name, dt))
        assert all(t.data_ptr() % 16 == 0 for t in (x0, n1, n2))
        got = K.free_init_noise(x0, n1, n2, Lf, Lh, Lw, SA, SB)
        worst[name] = check_case(name, dt, got)
        off = K.free_init_noise(off_alignment(x0), off_alignment(n1), off_alignment(n2), Lf, Lh, Lw, SA, SB)
        worst[name + "_off"] = check_case(name, dt, off)
        assert same_bits(got, off), name
    _record(f"free_init_noise_{str(dt).split('.')[-1]}", worst_ratio=max(worst.values()), **worst)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["vector", "odd_scalar", "frames_70", "cols_300"])
def test_identity_operators_return_n1_bit_for_bit(name, dt):
    """y == d exactly, so n1 + (y - d) / sb is n1: on the 16-byte path, on the scalar path, and past one trip of the tiled loops."""
    x0, n1, n2 = (t.cuda() for t in case(name, dt)[:3])
    F, h, w = CASES[name][:3]
    eye = [torch.eye(n, dtype=torch.float32, device="cuda") for n in (F, h, w)]
    assert same_bits(K.free_init_noise(x0, n1, n2, *eye, SA, SB), n1)
    assert same_bits(K.free_init_noise(off_alignment(x0), off_alignment(n1), off_alignment(n2), *eye, SA, SB), n1)


@pytest.mark.parametrize("name", ["vector", "odd_scalar"])
def test_a_nan_reaches_everything_it_is_summed_into(name):
    """A NaN in one element of n2 or of x0 is a term of every dot product along its row, then of its plane, then of its channel in every
    frame (dense operators; 0 * NaN is NaN too): that whole channel is NaN and the others are finite -- no element is skipped."""
    dt = torch.bfloat16
    x0, n1, n2, Lf, Lh, Lw = (t.cuda() for t in case(name, dt))
    F, h, w = CASES[name][:3]
    for which in ("n2", "x0"):
        a, b = x0.clone(), n2.clone()
        if which == "n2":
            b[0, F - 1, 2, h - 1, w - 1] = float("nan")
        else:
            a[0, 2, F - 1, h - 1, w - 1] = float("nan")
        got = K.free_init_noise(a, n1, b, Lf, Lh, Lw, SA, SB)
        assert torch.isnan(got[:, :, 2]).all(), which
        assert torch.isfinite(got[:, :, [0, 1, 3]]).all(), which


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("misalign", [0, 4])
@pytest.mark.parametrize("name", ["odd_scalar", "vector", "one_frame", "one_row", "frames_70", "rows_130", "cols_300", "odd_scalar_ring",
                                  "frames_16_ring"])
def test_free_init_noise_between_guard_bands(name, misalign, dt):
    """Every input, the result and the workspace between poisoned guards: no store outside the result or the workspace, no element of
    the result left unwritten, inputs and matrices untouched, no guard NaN in the result (``check_case``: finite, within the bound)."""
    host = case(name, dt)
    g = Guarded(K)
    x0, n1, n2 = (g.guard(t.cuda(), misalign=misalign if t.element_size() == 4 else misalign // 2) for t in host[:3])
    Lf, Lh, Lw = (g.guard(t.cuda()) for t in host[3:])
    with g:
        got = g.out(K.free_init_noise(x0, n1, n2, Lf, Lh, Lw, SA, SB))
    assert len(g.allocs) == 8                                               # the result and the workspace came from the proxy
    assert all(same_bits(a, b) for a, b in zip((x0, n1, n2, Lf, Lh, Lw), host))
    check_case(name, dt, got)


def test_free_init_noise_rejects_bad_arguments():
    dt = torch.bfloat16
    name = "vector"
    F, h, w = CASES[name][:3]
    x0, n1, n2, Lf, Lh, Lw = (t.cuda() for t in case(name, dt))
    ok = (x0, n1, n2, Lf, Lh, Lw)

    def call(**kw):
        a = dict(zip(("x0", "n1", "n2", "Lf", "Lh", "Lw"), ok), sa=SA, sb=SB)
        a.update(kw)
        return K.free_init_noise(a["x0"], a["n1"], a["n2"], a["Lf"], a["Lh"], a["Lw"], a["sa"], a["sb"])

    with pytest.raises(TypeError, match="bfloat16/float16"):
        call(x0=x0.float())
    with pytest.raises(RuntimeError, match="need tensors on the MI355X"):
        call(n2=n2.cpu())
    with pytest.raises(ValueError, match=r"x0 must be \[1, C, F, h, w\]"):
        call(x0=x0[0])
    with pytest.raises(ValueError, match="must not be empty"):
        call(x0=x0[:, :, :0])
    with pytest.raises(ValueError, match=r"n1 must be float32 \[1, 3, 4, 4, 8\]"):
        call(n1=n1.permute(0, 2, 1, 3, 4).contiguous())
    with pytest.raises(ValueError, match="n2 must be float32"):
        call(n2=n2.double())
    with pytest.raises(ValueError, match=r"Lh must be float32 \[4, 4\]"):
        call(Lh=Lw)
    with pytest.raises(ValueError, match="Lf must be float32"):
        call(Lf=Lf.double())
    with pytest.raises(ValueError, match="n1 must be contiguous"):
        call(n1=n1.transpose(3, 4).contiguous().transpose(3, 4))
    with pytest.raises(ValueError, match="Lw must be contiguous"):
        call(Lw=Lw.t())
    for bad in (0.0, -0.8, float("nan")):
        with pytest.raises(ValueError, match="sb=.* must be positive"):
            call(sb=bad)
    # the C entry point itself
    N = C * F * h * w
    out = torch.full((1, F, C, h, w), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.full((2 * N,), 7.0, dtype=torch.float32, device="cuda")
    before = out.clone()
    ptrs = [t.data_ptr() for t in ok] + [out.data_ptr(), ws.data_ptr()]
    sizes, coef = [C, F, h, w], [SA, SB, 1.0 / SB]
    fn, err = K.lib().im360_free_init_noise, K.lib().im360_last_error
    for i in range(8):
        bad = list(ptrs)
        bad[i] = None
        assert fn(*bad, 2 * N, *sizes, *coef, 0, None) != 0 and b"null pointer" in err(), i
    for i in range(4):
        for v in (0, -3):
            bad = list(sizes)
            bad[i] = v
            assert fn(*ptrs, 2 * N, *bad, *coef, 0, None) != 0 and b"must be positive" in err(), (i, v)
    assert fn(*ptrs, 1 << 40, 4, 1 << 10, 1 << 10, 1 << 9, *coef, 0, None) != 0 and b"2^31" in err()
    assert fn(*ptrs, 1 << 40, 1 << 31, 1, 1, 1, *coef, 0, None) != 0 and b"2^31" in err()
    assert fn(*ptrs, 2 * N - 1, *sizes, *coef, 0, None) != 0 and b"workspace holds" in err()
    for c in ([SA, 0.0, 1.0], [SA, -0.8, 1.25], [SA, SB, 0.0], [SA, float("nan"), 1.25]):
        assert fn(*ptrs, 2 * N, *sizes, *c, 0, None) != 0 and b"must be positive" in err(), c
    bad = list(ptrs)
    bad[0] += 1
    assert fn(*bad, 2 * N, *sizes, *coef, 0, None) != 0 and b"misaligned 16-bit tensor" in err()
    for i in range(1, 8):
        bad = list(ptrs)
        bad[i] += 2
        assert fn(*bad, 2 * N, *sizes, *coef, 0, None) != 0 and b"misaligned fp32 tensor" in err(), i
    for i in (0, 1, 2):                                                     # the result or the workspace on top of an input
        for j in (6, 7):
            bad = list(ptrs)
            bad[j] = ptrs[i]
            assert fn(*bad, 2 * N, *sizes, *coef, 0, None) != 0 and b"overlaps" in err(), (i, j)
    bad = list(ptrs)
    bad[6] = ptrs[7] + 4 * N
    assert fn(*bad, 2 * N, *sizes, *coef, 0, None) != 0 and b"out overlaps the workspace" in err()
    # the grid of the rows launch: 2^30 rows of one element are 2^24 workgroups of 64 rows, i.e. 2^32 threads
    assert fn(*ptrs, 1 << 40, 1, 1 << 15, 1 << 15, 1, *coef, 0, None) != 0 and b"2^24 (a launch holds fewer than 2^32 threads)" in err()
    assert fn(*ptrs, 2 * N, *sizes, *coef, 7, None) != 0 and b"dtype 7 unsupported" in err()
    torch.cuda.synchronize()
    assert same_bits(out, before) and float(ws.min()) == float(ws.max()) == 7.0                       # no refused call wrote anything
    assert all(same_bits(a, b) for a, b in zip(ok, case(name, dt)))
    stream = torch.cuda.current_stream().cuda_stream
    assert fn(*ptrs, 2 * N, *sizes, *coef, 0, stream) == 0                                            # the same arguments unbroken
    torch.cuda.synchronize()
    assert same_bits(out, K.free_init_noise(*ok, SA, SB))


# ------------------------------------------------------------------------------------------------ the small pipeline
STEPS = 3                                # a second-order step between two first-order ones under DPM-Solver++ 2M
WINDOWS = dict(context_frames=8, context_overlap=4)


@pytest.fixture(scope="module")
def clips():
    """8 frames, 15 (windows of 8 on a line) and 16 (on a ring), all at 128 x 256 pixels: a 16 x 32 latent."""
    return {n: S.video_batch(frames=n, pano_hw=(128, 256), seed=2) for n in (8, 15, 16)}


@pytest.fixture(scope="module")
def small_pipe():
    """The recipe of test_retime_init_gpu.py::small_pipe (width-5 model, width-4 VAE); returns (video, panorama latent, perspective
    latent, free_init_passes)."""
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    cond = S.conditioning(frames=16, seed=2)

    def run(use_graph, clip, seed=33, scheduler=DDIMScheduler, **kw):
        pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, scheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
        pipe._no_progress, pipe.use_graph = True, use_graph
        torch.manual_seed(seed)
        random.seed(seed)
        vid = pipe("synthetic", num_inference_steps=STEPS, guidance_scale_text=7.5, negative_prompt="", video_batch=clip,
                   use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video",
                   latents_dtype=dt, prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]),
                   **kw).videos
        return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone(), [p.clone() for p in pipe.free_init_passes]
    return run


@pytest.fixture(scope="module")
def plain_call(small_pipe, clips):
    return small_pipe(True, clips[8])


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and len(a[3]) == len(b[3]) and all(torch.equal(x, y) for x, y in zip(a[3], b[3]))


def _finite(run):
    return all(torch.isfinite(v.float()).all() for v in run[:3])


def test_one_pass_is_the_call_without_the_keyword(small_pipe, clips, plain_call):
    one = small_pipe(True, clips[8], free_init_iters=1, free_init_d_s=0.1, free_init_d_t=0.9)
    assert _same(one, plain_call) and len(one[3]) == 1 and torch.equal(one[3][0], one[1])


def test_two_passes_graph_equals_eager(small_pipe, clips, plain_call):
    graphed = small_pipe(True, clips[8], free_init_iters=2)
    eager = small_pipe(False, clips[8], free_init_iters=2)
    assert _same(graphed, eager) and _finite(graphed)
    assert len(graphed[3]) == 2 and torch.equal(graphed[3][0], plain_call[1]) and torch.equal(graphed[3][1], graphed[1])
    assert not torch.equal(graphed[1], plain_call[1]) and graphed[0].shape == plain_call[0].shape


@pytest.mark.parametrize("frames,loop", [(15, False), (16, True)], ids=["line_15", "ring_16"])
def test_two_passes_over_context_windows(small_pipe, clips, frames, loop):
    kw = dict(free_init_iters=2, context_loop=loop, **WINDOWS)
    graphed = small_pipe(True, clips[frames], **kw)
    eager = small_pipe(False, clips[frames], **kw)
    assert _same(graphed, eager) and _finite(graphed)
    assert graphed[1].shape == (1, 4, frames, 16, 32) and len(graphed[3]) == 2 and not torch.equal(graphed[3][0], graphed[3][1])
    first = small_pipe(True, clips[frames], context_loop=loop, **WINDOWS)
    assert torch.equal(graphed[3][0], first[1])


@pytest.mark.parametrize("kw", [dict(scheduler=DPMSolverMultistepScheduler), dict(guidance_rescale=0.7)], ids=["dpm_2m", "rescale"])
def test_two_passes_with_a_multistep_scheduler_and_with_guidance_rescale(small_pipe, clips, kw):
    graphed = small_pipe(True, clips[8], free_init_iters=2, **kw)
    eager = small_pipe(False, clips[8], free_init_iters=2, **kw)
    first = small_pipe(True, clips[8], **kw)
    assert _same(graphed, eager) and _finite(graphed)
    assert torch.equal(graphed[3][0], first[1]) and not torch.equal(graphed[1], first[1])


def test_a_plain_call_afterwards_is_unchanged(small_pipe, clips, plain_call):
    """``restart`` leaves no state behind (this file's order: after the passes)."""
    assert _same(small_pipe(True, clips[8]), plain_call)
