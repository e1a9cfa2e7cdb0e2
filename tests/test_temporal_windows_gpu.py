"""Window-fused temporal attention on the MI355X: ``kernels.temporal_attention_windows`` (csrc/temporal_attn.hip:
temporal_attn_windows_kernel) against the definition in fp64 on the same 16-bit inputs, its exact properties against itself, guarded
buffers at ragged shapes, the entry point's refusals, and the module / pipeline path of ``context_level="attention"`` (graph replay equals
the eager loop bit for bit under every loop variant).  The definition and the host logic on the CPU: tests/test_temporal_windows.py."""
import ctypes
import functools
import random

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _emu_temporal_windows as EW  # noqa: E402
import _release_pipe as RP  # noqa: E402
from _emu_keep_latents import half_mask  # noqa: E402
from _guarded import Guarded  # noqa: E402
from imagine360_amd import configs, context as CTX, kernels as K  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402
from imagine360_amd.unet3d import VersatileAttention  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
TOL = {torch.bfloat16: 1e-2, torch.float16: 3e-3}        # the project's table for attention kernels (tests/test_kernels_gpu.py)

# (B, F, P, heads, d, L, o, ring)
SHAPES = [(2, 32, 33, 8, 40, 16, 4, False),
          (1, 64, 9, 8, 160, 16, 4, False),              # the LDS limit: one head's rows of 64 frames
          (1, 24, 20, 8, 80, 16, 4, False),              # a partial frame tile
          (3, 20, 7, 8, 8, 8, 2, False),
          (1, 32, 17, 4, 24, 16, 10, False),             # three windows on some frames
          (2, 8, 50, 8, 40, 4, 2, True),
          (1, 32, 20, 8, 40, 16, 4, True),               # a window crossing the end of the clip
          (1, 11, 5, 8, 16, 5, 1, False)]                # L no multiple of 4: masked keys inside a lane's four scores
RAGGED = [SHAPES[2], SHAPES[3], SHAPES[5], SHAPES[7]]
sid = lambda s: "x".join(str(int(v)) for v in s)


def plan_of(shape, kind):
    B, Fr, P, heads, d, L, o, ring = shape
    return CTX.context_windows(Fr, L, o, loop=ring), CTX.context_weights(L, kind)


@functools.lru_cache(maxsize=None)
def reference(shape, dt, kind):
    B, Fr, P, heads, d, L, o, ring = shape
    qkv, pe = EW.inputs(B, Fr, P, heads, d, L, dt)
    starts, w = plan_of(shape, kind)
    return EW.brute_force(qkv, pe, B, Fr, P, heads, starts, w, ring=ring)


def launch(shape, dt, kind, starts=None, ring=None, out=None):
    B, Fr, P, heads, d, L, o, r = shape
    qkv, pe = EW.inputs(B, Fr, P, heads, d, L, dt)
    s, w = plan_of(shape, kind)
    s = s if starts is None else starts
    return K.temporal_attention_windows(qkv.cuda(), pe.cuda(), B, Fr, P, heads, torch.tensor(s, dtype=torch.int32, device="cuda"), w.cuda(),
                                        ring=r if ring is None else ring, out=out)


# ------------------------------------------------------------------------------------------------ 5. parity
@pytest.mark.parametrize("kind", CTX.WEIGHT_KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_windows_kernel_vs_fp64(shape, dt, kind):
    ref = reference(shape, dt, kind)
    out = launch(shape, dt, kind)
    err = EW.rel(out, ref)
    print(f"rel {err:.3e} (TOL {TOL[dt]:.0e})")
    assert out.dtype == dt and out.shape == ref.shape and bool(torch.isfinite(out.float()).all())
    assert err < TOL[dt]
    # out= with rows further apart than C: the gaps stay as they were
    C = shape[3] * shape[4]
    wide = torch.full((ref.shape[0], C + 8), 7.0, dtype=dt, device="cuda")
    got = launch(shape, dt, kind, out=wide[:, :C])
    assert got.data_ptr() == wide.data_ptr() and torch.equal(got, out) and bool((wide[:, C:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ 6. exact properties
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_exact_properties_of_the_kernel_against_itself(dt):
    line, ring = SHAPES[0], SHAPES[6]
    for shape in (line, ring):
        starts, _ = plan_of(shape, "pyramid")
        assert max(CTX.coverage(shape[1], shape[5], starts, loop=shape[7])) == 2
        a = launch(shape, dt, "pyramid")
        assert torch.equal(a, launch(shape, dt, "pyramid"))                                    # two calls: equal bits
        assert torch.equal(a, launch(shape, dt, "pyramid", starts=starts[::-1]))               # the order of the windows does not matter
        assert torch.equal(a, launch(shape, dt, "pyramid", starts=starts[1:] + starts[:1]))
    # a ring plan whose windows do not wrap: the bits of the line plan with the same starts
    assert torch.equal(launch(line, dt, "pyramid"), launch(line, dt, "pyramid", ring=True))


# ------------------------------------------------------------------------------------------------ 7. guarded buffers
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", RAGGED, ids=sid)
def test_windows_kernel_between_guard_bands(shape, dt):
    B, Fr, P, heads, d, L, o, ring = shape
    C = heads * d
    qkv, pe = EW.inputs(B, Fr, P, heads, d, L, dt)
    starts, w = plan_of(shape, "pyramid")
    ref = reference(shape, dt, "pyramid")
    g = Guarded(K)
    plain, wide = g.guard(qkv.cuda()), g.guard(qkv.cuda(), row_stride=3 * C + 8)      # the fused projection as a view of wider rows
    table = g.guard(pe.cuda())
    st, wt = torch.tensor(starts, dtype=torch.int32, device="cuda"), w.cuda()
    with g:
        o1 = g.out(K.temporal_attention_windows(plain, table, B, Fr, P, heads, st, wt, ring=ring))
        o2 = g.out(K.temporal_attention_windows(wide, table, B, Fr, P, heads, st, wt, ring=ring,
                                                out=g.empty((B * Fr * P, C), dt, "cuda", strides=(C + 8, 1))))
    assert EW.rel(o1, ref) < TOL[dt] and torch.equal(o1, o2)


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_entry_point_refusals_leave_the_output_untouched():
    dt = torch.bfloat16
    B, P, heads = 1, 3, 2

    def call(Fr=8, L=4, d=8, starts=(0, 2, 4), ring=False, shift=0, null=None):
        C = heads * d
        qkv = torch.randn(B * Fr * P, 3 * C + 8, device="cuda").to(dt)
        pe = torch.randn(L, 3 * C, device="cuda").to(dt)
        out = torch.full((B * Fr * P, C), 3.0, dtype=dt, device="cuda")
        st, w = (ctypes.c_int32 * len(starts))(*starts), (ctypes.c_float * L)(*([1.0] * L))
        ptr = {"q": qkv.data_ptr() + 2 * shift, "k": qkv.data_ptr() + 2 * C, "v": qkv.data_ptr() + 4 * C, "pe": pe.data_ptr(), "out": out.data_ptr(),
               "starts": ctypes.cast(st, ctypes.c_void_p), "weights": ctypes.cast(w, ctypes.c_void_p)}
        if null is not None:
            ptr[null] = None
        rs = 3 * C + 8
        rc = K.lib().im360_temporal_attn_windows_fwd(ptr["q"], ptr["k"], ptr["v"], ptr["pe"], ptr["out"], B, Fr, P, heads, d, P * rs, rs, Fr * P * rs,
                                                     P * C, C, Fr * P * C, ptr["starts"], len(starts), ptr["weights"], L, int(ring), d ** -0.5, 0,
                                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()) == (rc != 0)
        return rc, K.lib().im360_last_error().decode()

    assert call()[0] == 0 and call(starts=(0, 3, 6), ring=True)[0] == 0
    for kw, word in ((dict(Fr=65, L=16, starts=tuple(range(0, 50, 4))), "65 frames > 64"), (dict(Fr=32, L=17, starts=(0, 15)), "window length 17"),
                     (dict(d=12), "multiple of 8"), (dict(starts=(0, 4, 8)), "outside [0, 8)"), (dict(starts=(-1, 4)), "outside [0, 8)"),
                     (dict(starts=(0, 2, 6)), "past the end"), (dict(starts=(0, 5), ring=True), "frame 4 lies in no window"),
                     (dict(starts=(0,)), "lies in no window"), (dict(shift=4), "misaligned"), (dict(null="pe"), "null pointer"),
                     (dict(null="q"), "null pointer"), (dict(null="starts"), "null pointer")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    # the wrapper raises what the entry point refuses
    qkv, pe = torch.zeros(8 * 3, 48, dtype=dt, device="cuda"), torch.zeros(4, 48, dtype=dt, device="cuda")
    with pytest.raises(RuntimeError, match="lies in no window"):
        K.temporal_attention_windows(qkv, pe, 1, 8, 3, 2, [0], [1.0] * 4)


# ------------------------------------------------------------------------------------------------ 9. module and pipeline
@pytest.fixture(scope="module")
def clip():
    return RP.make_clip()


@pytest.fixture(scope="module")
def small_pipe(clip):
    return RP.make_runner(clip)


WINDOWS = dict(context_level="attention", context_frames=4, context_overlap=2)


@pytest.fixture(scope="module")
def plain_call(small_pipe):
    return small_pipe(True)


@pytest.fixture(scope="module")
def windowed_call(small_pipe):
    return small_pipe(True, **WINDOWS)


def test_motion_module_attention_with_windows_vs_the_definition():
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    torch.manual_seed(11)
    heads, d, B, Fr, P, L = 8, 40, 2, 8, 37, 4
    C = heads * d
    attn = VersatileAttention(C, heads, d, True, 24).to(dev, dt)
    norm = torch.nn.LayerNorm(C).to(dev, dt)
    x = torch.randn(B * Fr * P, C, device=dev).to(dt)
    plan = CTX.WindowPlan(Fr, L, 2, "pyramid", dev)
    with torch.no_grad():
        plain = attn(x, B, Fr, P, residual=x, norm=norm)
        attn.temporal_windows = plan
        got = attn(x, B, Fr, P, residual=x, norm=norm)
        attn.temporal_windows = None
        assert torch.equal(attn(x, B, Fr, P, residual=x, norm=norm), plain)
        w = torch.cat([attn.to_q.weight, attn.to_k.weight, attn.to_v.weight]).double()
        qkv = (F.layer_norm(x.double(), (C,), norm.weight.double(), norm.bias.double(), norm.eps) @ w.t())
        pe_qkv = attn.pos_encoder.pe[0, :L].to(dt).double() @ w.t()
        a = CTX.windowed_temporal_attention(qkv, pe_qkv, B, Fr, P, heads, plan.starts, plan.weights)
        want = F.linear(a, attn.to_out[0].weight.double(), attn.to_out[0].bias.double()) + x.double()
    err = EW.rel(got, want)
    print(f"rel {err:.3e}")
    assert err < TOL[dt] and EW.rel(plain, want) > 10 * err


VARIANTS = {
    "plain": dict(),
    "ring": dict(context_loop=True),
    "eta": dict(eta=0.5),
    "rescale": dict(guidance_rescale=0.7),
    "init_mask": dict(strength=RP.STRENGTH),
    "dpm_solver_2m": dict(),
    "interval": dict(guidance_interval=(0.2, 0.6)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_graph_replay_equals_the_eager_loop(small_pipe, plain_call, windowed_call, clip, variant):
    kw = dict(WINDOWS, **VARIANTS[variant])
    make = {}
    if variant == "eta":
        make["generator"] = lambda: torch.Generator(device="cuda").manual_seed(77)
    if variant == "dpm_solver_2m":
        make["scheduler"] = lambda: DPMSolverMultistepScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    if variant == "init_mask":
        kw.update(init_latents=plain_call[1], regenerate_mask=half_mask(RP.FRAMES, clip["pano_H"], clip["pano_W"]))
    graphed = windowed_call if variant == "plain" else small_pipe(True, **kw, **{k: f() for k, f in make.items()})
    eager = small_pipe(False, **kw, **{k: f() for k, f in make.items()})
    assert RP.same(graphed, eager), EW.rel(graphed[1], eager[1])
    assert all(bool(torch.isfinite(v.float()).all()) for v in graphed)
    if variant != "plain":
        assert not torch.equal(graphed[1], windowed_call[1])


def test_the_result_is_its_own(small_pipe, plain_call, windowed_call):
    """Neither the run without windows nor whole-model windows over the same plan."""
    model = small_pipe(True, context_frames=4, context_overlap=2)
    assert RP.same(model, small_pipe(True, context_frames=4, context_overlap=2, context_level="model"))
    assert not torch.equal(windowed_call[1], plain_call[1]) and not torch.equal(windowed_call[1], model[1])
    assert all(bool(torch.isfinite(v.float()).all()) for v in windowed_call)
    # without windows the level changes nothing
    assert RP.same(plain_call, small_pipe(True, context_level="attention", context_frames=8))


def test_nothing_is_left_set_on_the_pipeline(clip, plain_call):
    """A call without the keyword on the SAME pipeline object after a windowed one is a fresh pipeline's call."""
    from imagine360_amd import synthetic as S
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    cond = S.conditioning(frames=16, seed=2)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
    pipe._no_progress, pipe.use_graph = True, True

    def run(**kw):
        torch.manual_seed(33)
        random.seed(33)
        vid = pipe("synthetic", num_inference_steps=RP.STEPS, guidance_scale_text=7.5, negative_prompt="", video_batch=clip, use_outpaint=True,
                   use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video", latents_dtype=dt,
                   prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **kw).videos
        return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone()
    windowed = run(**WINDOWS)
    assert all(m.temporal_windows is None for m in mv.modules() if isinstance(m, VersatileAttention))
    assert not torch.equal(windowed[1], plain_call[1])
    assert RP.same(run(), plain_call)
