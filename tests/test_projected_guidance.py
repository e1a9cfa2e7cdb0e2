"""Adaptive projected guidance (APG, arXiv 2410.02416) on CPU: ``scheduler.projected_guidance`` in fp64 against the paper's x0-space
algorithm written out, its defining properties (orthogonality at eta = 0, plain CFG at eta = 1, the clamped RMS), the routing of
``guidance_apg`` to the kernels, and the pipeline keywords ``apg_eta`` / ``apg_threshold`` under emulated kernels: off is the call
without them bit for bit, on is another clip, the refusals, no APG call on an unguided step, the RNG streams, the multistep history."""
import contextlib
import random

import pytest
import torch

import _emu_apg_step as EA
import _emu_kernels as E
import _emu_multistep_step as EM
import _emu_noise_latents as EN
import _emu_rescale_step as ER
import _emu_ring_step as EG
import _emu_unguided_step as EU
from imagine360_amd import configs, synthetic as S
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, projected_guidance

torch.set_grad_enabled(False)

TYPES = ("epsilon", "v_prediction", "sample")
G = 7.5


def kappa(pt, sa, sb):
    return {"epsilon": (1.0 / sa, -sb / sa), "v_prediction": (sa, -sb), "sample": (0.0, 1.0)}[pt]


def inputs(seed=3, shape=(1, 4, 5, 7, 24)):
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(shape, generator=gen, dtype=torch.float64) * 0.25
    c = torch.randn(shape, generator=gen, dtype=torch.float64) * 0.1 + 3.0
    x = torch.randn(shape, generator=gen, dtype=torch.float64)
    return u, c, x


def x0_space(u, c, x, g, sa, sb, pt, eta, r):
    """Algorithm 1 of the paper on the denoised predictions (no momentum), the result mapped back to the model's output; also the
    pieces the property tests look at: (m, D(c), D^, s Delta)."""
    kx, kp = kappa(pt, sa, sb)
    Du, Dc = kx * x + kp * u, kx * x + kp * c
    delta = Dc - Du
    s = 1.0 if r is None else min(1.0, r / float((delta ** 2).mean().sqrt()))
    delta = s * delta
    alpha = float((delta * Dc).sum() / (Dc * Dc).sum())
    par = alpha * Dc
    orth = delta - par
    Dhat = Dc + (g - 1.0) * (orth + eta * par)
    return (Dhat - kx * x) / kp, Dc, Dhat, delta


def max_rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


SA, SB = 0.6 ** 0.5, 0.4 ** 0.5


@pytest.mark.parametrize("pt", TYPES)
def test_projected_guidance_is_the_x0_space_algorithm(pt):
    u, c, x = inputs()
    rms = float((abs(kappa(pt, SA, SB)[1]) * (c - u)).pow(2).mean().sqrt())
    for eta in (0.0, 0.5, 1.0, -0.5):
        for r in (None, 0.5 * rms, 2.0 * rms):          # the clamp active, and inactive
            got = projected_guidance(u, c, x, G, SA, SB, pt, eta, r)
            want = x0_space(u, c, x, G, SA, SB, pt, eta, r)[0]
            assert got.dtype == torch.float64 and got.shape == u.shape
            assert max_rel(got, want) <= 1e-12, (pt, eta, r, max_rel(got, want))
    assert projected_guidance(u.float(), c.float(), x.float(), G, SA, SB, pt, 0.0).dtype == torch.float32
    with pytest.raises(ValueError, match="prediction_type"):
        projected_guidance(u, c, x, G, SA, SB, "velocity", 0.0)


@pytest.mark.parametrize("pt", TYPES)
def test_eta_zero_leaves_nothing_along_the_denoised_text_prediction(pt):
    u, c, x = inputs(4)
    kx, kp = kappa(pt, SA, SB)
    m = projected_guidance(u, c, x, G, SA, SB, pt, 0.0)
    Dc, Dhat = kx * x + kp * c, kx * x + kp * m
    dot = float(((Dhat - Dc) * Dc).sum())
    assert abs(dot) <= 1e-10 * float((Dhat - Dc).norm() * Dc.norm()), dot
    assert float((Dhat - Dc).norm()) > 1e-3 * float(Dc.norm())            # (a real update: not the zero vector)


@pytest.mark.parametrize("pt", TYPES)
def test_eta_one_without_a_threshold_is_plain_cfg(pt):
    u, c, x = inputs(5)
    m = projected_guidance(u, c, x, G, SA, SB, pt, 1.0)
    assert max_rel(m, u + G * (c - u)) <= 1e-12


@pytest.mark.parametrize("pt", TYPES)
def test_an_active_threshold_sets_the_rms_of_the_difference(pt):
    """eta = 1 keeps the whole clamped difference: D^ - D(c) = (g - 1) s Delta, and rms(s Delta) = r."""
    u, c, x = inputs(6)
    kx, kp = kappa(pt, SA, SB)
    full = float((kp * (c - u)).pow(2).mean().sqrt())
    for r in (0.25 * full, 0.9 * full):
        m = projected_guidance(u, c, x, G, SA, SB, pt, 1.0, r)
        s_delta = (kp * m - kp * c) / (G - 1.0)
        assert abs(float(s_delta.pow(2).mean().sqrt()) / r - 1.0) <= 1e-12
    m = projected_guidance(u, c, x, G, SA, SB, pt, 1.0, 3.0 * full)      # a radius the difference lies inside: no clamp
    assert max_rel(m, u + G * (c - u)) <= 1e-12


def test_edge_cases_are_what_the_formula_gives():
    u, c, x = inputs(7)
    for r in (None, 0.5):
        assert torch.equal(projected_guidance(c, c, x, G, SA, SB, "v_prediction", 0.0, r), c)       # u == c: m = c
    q0 = torch.zeros_like(c)
    assert torch.isnan(projected_guidance(u, q0, x, G, SA, SB, "sample", 0.0)).all()                 # sum q^2 = 0


# ------------------------------------------------------------------------------------------------ routing
def _sched(cls=DDIMScheduler):
    sch = cls(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    return sch, sch._timesteps_host[3]


def test_guidance_apg_routing():
    """None calls exactly what is called without the keyword; (eta, threshold) goes to the six-coefficient step kernel with apg=, for
    eta = 0 too; the unguided steps never pass it on but select the six-coefficient kernel with it."""
    from imagine360_amd import kernels
    calls = []
    names = ("cfg_ddim_update", "cfg_ddim_step", "cfg_ddim_step_windows", "ddim_update", "ddim_step", "cfg_multistep_step", "multistep_step")
    saved = {n: getattr(kernels, n) for n in names}
    for n in names:
        setattr(kernels, n, lambda *a, _n=n, **k: calls.append((_n, k)))
    try:
        x = torch.zeros(8)
        sch, t = _sched()
        assert sch.uses_step_kernel() is False and sch.uses_step_kernel(guidance_apg=None) is False
        assert sch.uses_step_kernel(guidance_apg=(0.0, None)) is True
        sch.fused_cfg_step(x, x, 7.5, t, x)
        sch.fused_cfg_step(x, x, 7.5, t, x, guidance_apg=None)
        sch.fused_cfg_step(x, x, 7.5, t, x, guidance_apg=(0.0, None))
        sch.fused_cfg_step(x, x, 7.5, t, x, eta=1.0, noise=x, guidance_apg=(0.5, 2.0))
        p, st, w = torch.zeros(1, 2, 4, 2, 1, 1), torch.zeros(1, dtype=torch.int32), torch.ones(2)
        lat = torch.zeros(1, 4, 2, 1, 1)
        sch.fused_cfg_step_windows(p, st, w, 7.5, t, lat)
        sch.fused_cfg_step_windows(p, st, w, 7.5, t, lat, guidance_apg=(0.0, 1.5), ring=True)
        sch.fused_step(x, t, x)
        sch.fused_step(x, t, x, guidance_apg=(0.0, None))
        dpm, td = _sched(DPMSolverMultistepScheduler)
        h = torch.zeros(8)
        dpm.fused_cfg_step(x, x, 7.5, td, x, history=h)
        dpm.fused_cfg_step(x, x, 7.5, td, x, history=h, guidance_apg=(0.0, None))
        dpm.fused_step(x, td, x, history=h, guidance_apg=(0.0, None))
    finally:
        for n, fn in saved.items():
            setattr(kernels, n, fn)
    assert calls[0] == calls[1] == ("cfg_ddim_update", {"coef_dev": None})
    assert calls[2] == ("cfg_ddim_step", {"coef_dev": None, "apg": (0.0, None)})
    assert calls[3] == ("cfg_ddim_step", {"coef_dev": None, "apg": (0.5, 2.0)})
    assert calls[4] == ("cfg_ddim_step_windows", {"coef_dev": None})
    assert calls[5] == ("cfg_ddim_step_windows", {"coef_dev": None, "ring": True, "apg": (0.0, 1.5)})
    assert calls[6] == ("ddim_update", {"coef_dev": None}) and calls[7] == ("ddim_step", {"coef_dev": None})
    assert calls[8] == ("cfg_multistep_step", {"coef_dev": None})
    assert calls[9] == ("cfg_multistep_step", {"coef_dev": None, "apg": (0.0, None)})
    assert calls[10] == ("multistep_step", {"coef_dev": None})


def test_wrappers_refuse_apg_beside_rescale_and_bad_values():
    """Host-side checks of kernels._apg_args, in front of any launch."""
    from imagine360_amd import kernels
    assert kernels._apg_args("t", (0, None)) == (0.0, float("inf")) and kernels._apg_args("t", (0.5, 2)) == (0.5, 2.0)
    for apg, rescale, pat in (((0.0, None), 0.7, "cannot be combined"), ((float("nan"), None), 0.0, "eta"), ((float("inf"), 1.0), 0.0, "eta"),
                              ((0.0, 0.0), 0.0, "threshold"), ((0.0, -1.0), 0.0, "threshold"), ((0.0, float("nan")), 0.0, "threshold")):
        with pytest.raises(ValueError, match=pat):
            kernels._apg_args("t", apg, rescale)


@pytest.mark.parametrize("pt", TYPES)
def test_stand_in_is_the_definition_then_the_step(pt):
    """The stand-in's scalars give the definition's m (the kernel's formula c + (g - 1) s d - lambda q), and one uniform window is the
    plain stand-in."""
    from imagine360_amd.context import context_weights
    u, c, x = (v.float() for v in inputs(8))
    mode = {"epsilon": 0, "v_prediction": 1, "sample": 2}[pt]
    coefs = (G, SA, SB, 0.9, 0.3, 0.0)
    rho = {"epsilon": -1.0 / SB, "v_prediction": -SA / SB, "sample": 0.0}[pt]
    for apg in ((0.0, None), (0.5, 0.05)):
        alpha, s, lam = (float(v) for v in EA.cfg_apg_scalars(u, c, x, mode, coefs, apg))
        m = c + (G - 1.0) * s * (c - u) - lam * (c + rho * x)
        want = projected_guidance(u.double(), c.double(), x.double(), G, SA, SB, pt, *apg)
        assert max_rel(m.double(), want) < 1e-5 and (apg[1] is None) == (s == 1.0)
        got = EA.cfg_ddim_step(u, c, x, None, mode, coefs, apg=apg)
        preds = torch.stack([torch.cat([u, c])])
        st, w = torch.zeros(1, dtype=torch.int32), context_weights(u.shape[2], "uniform")
        assert torch.equal(EA.cfg_ddim_step_windows(preds, x, None, st, w, mode, coefs, apg=apg), got)
        assert torch.equal(EA.cfg_apg_scalars_windows(preds, x, st, w, mode, coefs, apg), EA.cfg_apg_scalars(u, c, x, mode, coefs, apg))
    assert torch.equal(EA.cfg_ddim_step(u, c, x, None, mode, coefs), ER.cfg_ddim_step(u, c, x, None, mode, coefs))


# ------------------------------------------------------------------------------------------------ pipeline
@contextlib.contextmanager
def patches():
    """Every kernel the loops reach as its stand-in; yields (APG stand-in calls, unguided stand-in calls)."""
    with contextlib.ExitStack() as st:
        for cm in (E.patched_kernels(), ER.patched_rescale_kernels(), EG.patched_ring_kernels(), EN.patched_noise_latents(),
                   EM.patched_multistep_kernels()):
            st.enter_context(cm)
        unguided = st.enter_context(EU.patched_unguided_kernels())
        yield st.enter_context(EA.patched_apg_kernels()), unguided


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


def pipe_kw(cond, vb, steps=2, **extra):
    return dict(num_inference_steps=steps, guidance_scale_text=7.5, negative_prompt="", video_batch=vb, use_outpaint=True,
                use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video", latents_dtype=torch.float32,
                prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **extra)


def _run(pipe, seed=5, **kw):
    """-> (latents, the state of torch's and of Python's generator after the call)."""
    torch.manual_seed(seed)
    random.seed(seed)
    pipe("synthetic", **kw)
    return [v.clone() for v in pipe.last_latents], (torch.get_rng_state(), random.getstate())


VARIANTS = {"plain": {}, "windows": dict(context_frames=2, context_overlap=1), "ring": dict(context_frames=2, context_overlap=1, context_loop=True)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_pipeline_off_is_the_call_without_the_keywords_and_on_is_another_clip(cpu_pipe, clip4, variant):
    vb, cond = clip4
    extra = VARIANTS[variant]
    with patches() as (calls, _):
        base, base_rng = _run(cpu_pipe, **pipe_kw(cond, vb, **extra))
        off, off_rng = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=None, apg_threshold=None, **extra))
        assert not calls
        on, on_rng = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=0.0, **extra))
        n_on = len(calls)
        clamped, _ = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=0.0, apg_threshold=1e-3, **extra))
    assert all(torch.equal(a, b) for a, b in zip(off, base))
    assert n_on == 4 and set(calls) == {"cfg_ddim_step" if variant == "plain" else "cfg_ddim_step_windows"}       # 2 steps x 2 branches
    for a, b, k in zip(on, base, clamped):
        assert torch.isfinite(a).all() and torch.isfinite(k).all()
        assert float((a - b).norm() / b.norm()) > 1e-3 and float((k - a).norm() / a.norm()) > 1e-3
    # each generator ends where it ends without APG
    assert torch.equal(base_rng[0], off_rng[0]) and torch.equal(base_rng[0], on_rng[0]) and base_rng[1] == off_rng[1] == on_rng[1]


def test_generators_end_in_the_same_state_with_eta(cpu_pipe, clip4):
    vb, cond = clip4
    states = []
    with patches():
        for apg in ({}, dict(apg_eta=0.0, apg_threshold=0.5)):
            gen = torch.Generator().manual_seed(21)
            _, rng = _run(cpu_pipe, **pipe_kw(cond, vb, eta=0.8, generator=gen, **apg))
            states.append((gen.get_state(), *rng))
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1]) and states[0][2] == states[1][2]


def test_refusals(cpu_pipe, clip4):
    from imagine360_amd.dist import FrameShard
    vb, cond = clip4
    bad = ((dict(apg_threshold=1.0), "apg_threshold needs apg_eta"),
           (dict(apg_eta=float("nan")), "apg_eta must be finite"), (dict(apg_eta=float("inf")), "apg_eta must be finite"),
           (dict(apg_eta=0.0, apg_threshold=float("nan")), "apg_threshold must be"), (dict(apg_eta=0.0, apg_threshold=float("inf")), "apg_threshold must be"),
           (dict(apg_eta=0.0, apg_threshold=0.0), "apg_threshold must be"), (dict(apg_eta=0.0, apg_threshold=-1.0), "apg_threshold must be"),
           (dict(apg_eta=0.0, guidance_rescale=0.7), "apg_eta cannot be combined with guidance_rescale"),
           (dict(apg_eta=0.0, frame_shard=FrameShard(4, rank=0, world=1)), "apg_eta cannot be combined with frame_shard"))
    with patches() as (calls, _):
        for kw, pat in bad:
            with pytest.raises(ValueError, match=pat):
                _run(cpu_pipe, **pipe_kw(cond, vb, **kw))
        assert not calls


@pytest.mark.parametrize("variant", ["plain", "ring"])
def test_unguided_steps_make_no_apg_call(cpu_pipe, clip4, variant):
    """(0.2, 0.6) on 4 steps guides steps 1 and 2: two branches each form a projected guidance there and nowhere else; the unguided
    steps take the six-coefficient unguided kernel, as the guided steps of the run do."""
    vb, cond = clip4
    with patches() as (calls, unguided):
        _run(cpu_pipe, **pipe_kw(cond, vb, steps=4, guidance_interval=(0.2, 0.6), apg_eta=0.0, apg_threshold=0.5, **VARIANTS[variant]))
        assert len(calls) == 4, calls
        assert unguided == ["ddim_step" if variant == "plain" else "ddim_step_windows"] * 4, unguided


@pytest.mark.parametrize("variant", ["plain", "windows"])
def test_multistep_history_receives_the_x0_of_the_projected_guidance(cpu_pipe, clip4, variant, monkeypatch):
    vb, cond = clip4
    seen = []
    real = EM._step_on

    def spy(m, sample, hist, mode, coefs, coef_dev):
        out = real(m, sample, hist, mode, coefs, coef_dev)
        seen.append((m.clone(), sample.clone(), hist.clone(), mode, [float(v) for v in coefs]))
        return out
    monkeypatch.setattr(EM, "_step_on", spy)
    saved = cpu_pipe.scheduler
    cpu_pipe.scheduler = DPMSolverMultistepScheduler.from_config(saved.config)
    try:
        with patches() as (calls, _):
            on, _ = _run(cpu_pipe, **pipe_kw(cond, vb, steps=3, apg_eta=0.0, **VARIANTS[variant]))
            n = len(calls)
            base, _ = _run(cpu_pipe, **pipe_kw(cond, vb, steps=3, **VARIANTS[variant]))
    finally:
        cpu_pipe.scheduler = saved
    assert n == 6 and set(calls[:6]) == {"cfg_multistep_step" if variant == "plain" else "cfg_multistep_step_windows"}
    assert float((on[0] - base[0]).norm() / base[0].norm()) > 1e-3
    for m, x, hist, mode, coefs in seen[:6]:          # the APG run's six steps: hist is the x0 of the m the stand-in formed
        assert mode & 3 == 1
        x0 = coefs[1] * x.float() - coefs[2] * m
        if mode & 4:
            x0 = x0.clamp(-1.0, 1.0)
        assert torch.equal(hist.reshape(x0.shape), x0)


def test_scheduler_level_history_is_the_x0_of_m():
    sch, t = _sched(DPMSolverMultistepScheduler)
    u, c, x = (v.float() for v in inputs(9))
    h = sch.new_history(x)
    with patches():
        sch.fused_cfg_step(u, c, G, t, x, history=h, guidance_apg=(0.0, None))
    _, sa, sb = sch.step_coefficients(t, 0.0, G)[:3]
    m = projected_guidance(u.double(), c.double(), x.double(), G, sa, sb, sch.config.prediction_type, 0.0)
    kx, kp = kappa(sch.config.prediction_type, sa, sb)
    x0 = kx * x.double() + kp * m
    if sch.config.clip_sample:
        x0 = x0.clamp(-1.0, 1.0)
    assert max_rel(h.double(), x0) < 1e-5
