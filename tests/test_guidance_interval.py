"""``guidance_interval`` (guidance in a limited timestep interval, arXiv 2404.07724) on CPU: ``scheduler.guided_steps``, the torch
stand-ins of the unguided step entry points against the per-element bound of _ref_step.py, and the pipeline under emulated kernels --
the model runs at batch 1 outside the interval and at batch 2 inside, every traced latent is what the GUIDED stand-in gives on (c, c)
resp. (u, c) bit for bit, the guidance rescale launches no statistics on an unguided step, the kept region of ``regenerate_mask``
survives, ``frame_shard`` is refused."""
import contextlib
import random
import types

import pytest
import torch

import _emu_keep_latents as EK
import _emu_keep_release as EKR
import _emu_kernels as E
import _emu_multistep_step as EM
import _emu_noise_latents as EN
import _emu_rescale_step as ER
import _emu_ring_step as EG
import _emu_unguided_step as EU
import _interval_runs as IR
import _step_cases as C
import _unguided_cases as UC
from _emu_keep_latents import half_mask, kept
from imagine360_amd import configs, synthetic as S
from imagine360_amd.context import WindowPlan
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler

torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ 1. the scheduler
@pytest.mark.parametrize("cls", [DDIMScheduler, DPMSolverMultistepScheduler])
def test_guided_steps(cls):
    sch = cls(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(4)
    steps = sch._timesteps_host
    assert steps == [751, 501, 251, 1]                                                   # (750, 500, 250, 0 + steps_offset)
    assert sch.guided_steps(steps, (0.2, 0.6)) == [False, True, True, False] == IR.KINDS
    assert sch.guided_steps(steps, (0, 1)) == [True] * 4 and sch.guided_steps(steps, None) == [True] * 4
    assert sch.guided_steps(steps, (0.3, 0.3)) == [False] * 4
    assert sch.guided_steps(steps, (0.25, 0.75)) == [False, True, True, False]          # lo T <= t < hi T: 251 in, 751 out
    assert sch.guided_steps(steps, [0.0, 0.5]) == [False, False, True, True]
    _, short = sch.timesteps_for_strength(0.75)
    assert short == steps[1:] and sch.guided_steps(short, (0.2, 0.6)) == [True, True, False]
    assert cls.guided_steps is DDIMScheduler.guided_steps                                # the one definition
    for bad in ((0.6, 0.2), (-0.1, 0.5), (0.0, 1.5), (float("nan"), 0.5), (0.1, float("nan")), (0.5,), (0.1, 0.2, 0.3), 0.5, "ab", ("a", "b")):
        with pytest.raises(ValueError, match="guidance_interval"):
            sch.guided_steps(steps, bad)


# ------------------------------------------------------------------------------------------------ 2. the stand-ins
EMU = types.SimpleNamespace(**{n: getattr(EU, n) for n in EU.NAMES})
GUIDED_EMU = types.SimpleNamespace(cfg_ddim_update=E.cfg_ddim_update, cfg_ddim_step=ER.cfg_ddim_step, cfg_ddim_step_windows=EG.cfg_ddim_step_windows,
                                   cfg_multistep_step=EM.cfg_multistep_step, cfg_multistep_step_windows=EM.cfg_multistep_step_windows)


@pytest.mark.parametrize("family", UC.FAMILIES)
@pytest.mark.parametrize("dt", C.DTYPES, ids=C.dtname)
def test_unguided_stand_ins_within_rounding(dt, family):
    """Every non-rescale case of _step_cases.py with u := c through the stand-ins, scalar and tensor coefficients: within the bound of
    the fp64 restatement, and the guided stand-in's bits on (c, c) at guidance 7.5 and 1.0."""
    n, worst = 0, {}
    for case in UC.cases(dt, family):
        ref4 = UC.reference(case)
        for coef_dev in (False, True):
            out, hist = UC.call(EMU, case, coef_dev=coef_dev)
            C.check(case, out, hist, ref4, 0.0, worst)
            for g in (C.G, 1.0):
                want, want_hist = C.call(GUIDED_EMU, UC.with_guidance(case, g), coef_dev=coef_dev)
                assert torch.equal(out, want) and (hist is None or torch.equal(hist, want_hist)), (case.name, g)
        n += 1
    assert n >= 3 and 0.0 < worst["out"] <= 1.0


# ------------------------------------------------------------------------------------------------ 3. the pipeline's host logic
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
def clip4():
    return S.video_batch(frames=4, pano_hw=(128, 256), seed=8), S.conditioning(frames=16, seed=8)


def pipe_kw(cond, vb, **extra):
    return dict(num_inference_steps=4, guidance_scale_text=7.5, negative_prompt="", video_batch=vb, use_outpaint=True,
                use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video", latents_dtype=torch.float32,
                prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **extra)


def _run(pipe, seed=5, **kw):
    torch.manual_seed(seed)
    random.seed(seed)
    pipe("synthetic", **kw)
    return [v.clone() for v in pipe.last_latents]


@contextlib.contextmanager
def patches():
    """Every kernel the loops reach as its stand-in; yields (unguided stand-in calls, rescale statistics calls, keep blends)."""
    with contextlib.ExitStack() as st:
        for cm in (E.patched_kernels(), ER.patched_rescale_kernels(), EG.patched_ring_kernels(), EN.patched_noise_latents(),
                   EM.patched_multistep_kernels()):
            st.enter_context(cm)
        stats = []
        real = ER._factor
        st.callback(setattr, ER, "_factor", real)
        ER._factor = lambda *a, **k: (stats.append(1), real(*a, **k))[1]
        st.enter_context(EKR.patched_keep_release())
        yield st.enter_context(EU.patched_unguided_kernels()), stats, st.enter_context(EK.patched_keep_latents())


@pytest.mark.parametrize("variant", ["ddim", "ddim_eta", "dpm_solver_2m", "windows", "windows_ring_dpm"])
def test_every_step_is_the_guided_step_on_what_the_model_returned(cpu_pipe, clip4, variant, monkeypatch):
    """(0.2, 0.6) on 4 steps: the model runs at batch 1, 2, 2, 1 (per window), with the IP noise cut from the CFG batch's draw on the
    unguided steps, and the trace is the guided stand-in on (c, c) / (u, c) bit for bit.  Fails on a pipeline that ignores the keyword."""
    vb, cond = clip4
    eta = 0.5 if variant == "ddim_eta" else 0.0
    extra = dict(eta=eta) if eta else {}
    plan = None
    if variant.startswith("windows"):
        ring = "ring" in variant
        extra.update(context_frames=2, context_overlap=1, context_loop=ring)
        plan = WindowPlan(4, 2, 1, "pyramid", "cpu", loop=ring)
    saved = cpu_pipe.scheduler
    if "dpm" in variant:
        cpu_pipe.scheduler = DPMSolverMultistepScheduler.from_config(saved.config)
    try:
        with patches() as (calls, stats, _), IR.recording(cpu_pipe.mv_base_model, monkeypatch) as rec:
            trace = []
            got = _run(cpu_pipe, **pipe_kw(cond, vb, guidance_interval=IR.INTERVAL, trace=trace, **extra))
            nW = 1 if plan is None else len(plan)
            assert rec.batches() == [b for k in IR.KINDS for b in [2 if k else 1] * nW]
            assert len(calls) == 4 and len(set(calls)) == 1 and (("windows" in calls[0]) == (plan is not None)) \
                and (("multistep" in calls[0]) == ("dpm" in variant))
            assert cpu_pipe.mv_base_model._ip_noise_half is None
            want = IR.recompute_trace(cpu_pipe.scheduler, rec, cpu_pipe.scheduler._timesteps_host, IR.KINDS, eta=eta, plan=plan)
        assert len(trace) == 4 and all(torch.equal(a, b) for a, b in zip(trace, want)) and torch.equal(got[0], trace[-1])
        assert stats == [] and all(u.ip_cache_entries == 1 for u in (cpu_pipe.mv_base_model.unet, cpu_pipe.mv_base_model.pano_unet))
        assert not any(isinstance(k, tuple) for u in (cpu_pipe.mv_base_model.unet, cpu_pipe.mv_base_model.pano_unet) for k in u._ip_cache._store)
    finally:
        cpu_pipe.scheduler = saved


def test_none_and_a_covering_interval_are_the_call_without_the_keyword(cpu_pipe, clip4, monkeypatch):
    vb, cond = clip4
    with patches() as (calls, _, _), IR.recording(cpu_pipe.mv_base_model, monkeypatch) as rec:
        plain = _run(cpu_pipe, **pipe_kw(cond, vb))
        state = torch.get_rng_state(), random.getstate()
        for interval in (None, (0, 1), (0.0, 0.9)):                     # (timesteps 750 .. 0: all below 900)
            again = _run(cpu_pipe, **pipe_kw(cond, vb, guidance_interval=interval))
            assert all(torch.equal(a, b) for a, b in zip(plain, again))
        assert calls == [] and set(rec.batches()) == {2}
        # the RNG streams do not move: after a run with the interval every generator stands where it stands without
        other = _run(cpu_pipe, **pipe_kw(cond, vb, guidance_interval=IR.INTERVAL))
        assert torch.equal(torch.get_rng_state(), state[0]) and random.getstate() == state[1]
        assert not torch.equal(other[0], plain[0])
        none = _run(cpu_pipe, **pipe_kw(cond, vb, guidance_interval=(0.3, 0.3)))
        assert rec.batches()[-4:] == [1] * 4 and torch.equal(torch.get_rng_state(), state[0]) and not torch.equal(none[0], other[0])


def test_guidance_rescale_is_skipped_on_unguided_steps(cpu_pipe, clip4):
    vb, cond = clip4
    with patches() as (calls, stats, _):
        _run(cpu_pipe, **pipe_kw(cond, vb, guidance_rescale=0.7))
        assert len(stats) == 8 and calls == []                       # two branches x four steps
        del stats[:]
        _run(cpu_pipe, **pipe_kw(cond, vb, guidance_rescale=0.7, guidance_interval=IR.INTERVAL))
        assert len(stats) == 4 and calls == ["ddim_step"] * 4          # the two guided steps; the six-coefficient kernel on the others


@pytest.mark.parametrize("mode", ["blend", "release"])
def test_the_kept_region_is_still_the_init(cpu_pipe, clip4, mode):
    vb, cond = clip4
    half = half_mask(4, 128, 256)
    with patches() as (calls, _, blends):
        x0 = _run(cpu_pipe, **pipe_kw(cond, vb))[0]
        got = _run(cpu_pipe, **pipe_kw(cond, vb, init_latents=x0, strength=0.75, regenerate_mask=half, regenerate_mode=mode,
                                       guidance_interval=IR.INTERVAL))
        assert len(calls) == 2                                        # steps 500, 250, 0: guided, guided, unguided
    keep = kept(half, 16, 32).expand_as(x0)
    assert torch.equal(got[0][keep], x0[keep]) and not torch.equal(got[0][~keep], x0[~keep])


def test_refusals(cpu_pipe, clip4):
    from imagine360_amd.dist import FrameShard
    vb, cond = clip4
    with patches() as (calls, _, _):
        with pytest.raises(ValueError, match="guidance_interval cannot be combined with frame_shard.*not implemented"):
            cpu_pipe("synthetic", **pipe_kw(cond, vb, guidance_interval=IR.INTERVAL, frame_shard=FrameShard(4, rank=0, world=1)))
        for bad in ((0.6, 0.2), (0.1, 1.2), 0.5):
            with pytest.raises(ValueError, match="guidance_interval"):
                cpu_pipe("synthetic", **pipe_kw(cond, vb, guidance_interval=bad))
    assert calls == [] and cpu_pipe.mv_base_model._ip_noise_half is None
