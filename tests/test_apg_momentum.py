"""The momentum of adaptive projected guidance (arXiv 2410.02416, algorithm 1 in full) on CPU: ``scheduler.projected_guidance(...,
momentum=)`` chained through ``apg_carry`` in fp64 against the paper's x0-space algorithm written out, ``apg_carry`` itself, the
wrappers' checks, and the pipeline keyword ``apg_momentum`` under emulated kernels: None is the call of before, 0.0 equals None bit for
bit, the carry sequence of a run, of a guidance interval, of FreeInit passes and of a shortened schedule, windows and the multistep
scheduler, the refusals."""
import contextlib
import random

import pytest
import torch

import _emu_apg_momentum as EP
import _emu_free_init as EF
import _emu_kernels as E
import _emu_multistep_step as EM
import _emu_noise_latents as EN
import _emu_rescale_step as ER
import _emu_ring_step as EG
import _emu_unguided_step as EU
from imagine360_amd import configs, synthetic as S
from imagine360_amd.scheduler import _APG_KAPPA, DDIMScheduler, DPMSolverMultistepScheduler, projected_guidance

torch.set_grad_enabled(False)

TYPES = ("epsilon", "v_prediction", "sample")
G = 7.5


def _sched(pt="v_prediction", cls=DDIMScheduler):
    sch = cls(**{**configs.NOISE_SCHEDULER_KWARGS, "prediction_type": pt})
    sch.set_timesteps(25)
    return sch


def inputs(seed, shape=(1, 4, 5, 7, 24)):
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(shape, generator=gen, dtype=torch.float64) * 0.25
    c = torch.randn(shape, generator=gen, dtype=torch.float64) * 0.1 + 3.0
    x = torch.randn(shape, generator=gen, dtype=torch.float64)
    return u, c, x


def max_rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _sab(sch, t):
    a = sch._alphas(t)[0]
    return a ** 0.5, (1.0 - a) ** 0.5


def x0_space_run(sch, pt, steps, data, beta, eta, r):
    """Algorithm 1 of the paper on the denoised predictions over consecutive steps: the running average Dbar in x0 units, clamped on
    Dbar, projected on D(c); each step's result mapped back to the model's output.  -> [m_t]"""
    out, dbar = [], 0.0
    for t, (u, c, x) in zip(steps, data):
        sa, sb = _sab(sch, t)
        kx, kp = _APG_KAPPA[pt](sa, sb)
        Du, Dc = kx * x + kp * u, kx * x + kp * c
        dbar = (Dc - Du) + beta * dbar                                  # the state keeps the UNclamped average
        s = 1.0 if r is None else min(1.0, r / float((dbar ** 2).mean().sqrt()))
        delta = s * dbar
        alpha = float((delta * Dc).sum() / (Dc * Dc).sum())
        Dhat = Dc + (G - 1.0) * (delta - (1.0 - eta) * alpha * Dc)
        out.append((Dhat - kx * x) / kp)
    return out


# ------------------------------------------------------------------------------------------------ 1. the definition
@pytest.mark.parametrize("pt", TYPES)
@pytest.mark.parametrize("beta", [-0.75, -0.5, 0.5])
def test_momentum_chain_is_the_x0_space_algorithm(pt, beta):
    sch = _sched(pt)
    steps = sch._timesteps_host[3:8]                 # five consecutive timesteps (sqrt_a > 0: epsilon's x0 is finite)
    data = [inputs(20 + i) for i in range(len(steps))]
    sa, sb = _sab(sch, steps[0])
    rms0 = float((abs(_APG_KAPPA[pt](sa, sb)[1]) * (data[0][1] - data[0][0])).pow(2).mean().sqrt())
    for eta in (0.0, 0.5):
        for r in (None, 0.5 * rms0, 1.2 * rms0):     # no clamp; active on every step; active on some steps
            want = x0_space_run(sch, pt, steps, data, beta, eta, r)
            e, t_prev = None, None
            for i, (t, (u, c, x)) in enumerate(zip(steps, data)):
                carry = sch.apg_carry(t_prev, t, beta)
                assert (carry == 0.0) == (i == 0)
                m, e = projected_guidance(u, c, x, G, *_sab(sch, t), pt, eta, r, momentum=(e, carry))
                t_prev = t
                assert m.dtype == torch.float64 and e.dtype == torch.float64 and e.shape == u.shape
                assert max_rel(m, want[i]) <= 1e-12, (pt, beta, eta, r, i, max_rel(m, want[i]))
            # the momentum matters: the last step differs from the momentum-less value
            plain = projected_guidance(*data[-1], G, *_sab(sch, steps[-1]), pt, eta, r)
            assert max_rel(m, plain) > 1e-4


@pytest.mark.parametrize("pt", TYPES)
def test_beta_zero_and_carry_zero_return_todays_bits(pt):
    sch = _sched(pt)
    t0, t1 = sch._timesteps_host[3:5]
    u, c, x = inputs(31)
    sa, sb = _sab(sch, t1)
    for r in (None, 0.05):
        today = projected_guidance(u, c, x, G, sa, sb, pt, 0.0, r)
        assert sch.apg_carry(t0, t1, 0.0) == 0.0
        nan = torch.full_like(u, float("nan"))
        for prev in (None, nan, torch.ones_like(u)):              # carry 0 does not read the state: NaN cannot leak
            m, e = projected_guidance(u, c, x, G, sa, sb, pt, 0.0, r, momentum=(prev, sch.apg_carry(t0, t1, 0.0)))
            assert torch.equal(m, today) and torch.equal(e, c - u)
        m, e = projected_guidance(u, c, x, G, sa, sb, pt, 0.0, r, momentum=(None, sch.apg_carry(None, t1, -0.5)))
        assert torch.equal(m, today) and torch.equal(e, c - u)
        assert torch.is_tensor(projected_guidance(u, c, x, G, sa, sb, pt, 0.0, r, momentum=None))


# ------------------------------------------------------------------------------------------------ 2. apg_carry
def test_apg_carry():
    for pt in TYPES:
        sch = _sched(pt)
        ts = sch._timesteps_host
        assert sch.apg_carry(None, ts[4], -0.5) == 0.0 and isinstance(sch.apg_carry(None, ts[4], -0.5), float)
        for t_prev, t in ((ts[3], ts[4]), (ts[2], ts[9]), (ts[20], ts[24])):         # consecutive, and across unguided steps
            got = sch.apg_carry(t_prev, t, -0.75)
            a_p, a_t = sch._alphas(t_prev)[0], sch._alphas(t)[0]
            if pt == "sample":
                assert got == -0.75
            elif pt == "epsilon":
                want = -0.75 * ((1 - a_p) ** 0.5 / a_p ** 0.5) / ((1 - a_t) ** 0.5 / a_t ** 0.5)
                assert abs(got / want - 1.0) <= 1e-14
            else:
                want = -0.75 * (1 - a_p) ** 0.5 / (1 - a_t) ** 0.5
                assert abs(got / want - 1.0) <= 1e-14
    dpm = _sched(cls=DPMSolverMultistepScheduler)
    ts = dpm._timesteps_host
    assert dpm.apg_carry(ts[3], ts[4], -0.5) == _sched().apg_carry(ts[3], ts[4], -0.5)


def test_new_apg_state_is_an_uninitialised_fp32_twin():
    sch = _sched()
    lat = torch.zeros(1, 4, 3, 2, 8, dtype=torch.bfloat16)
    st = sch.new_apg_state(lat)
    assert st.dtype == torch.float32 and st.shape == lat.shape and st.device == lat.device and st.is_contiguous()


# ------------------------------------------------------------------------------------------------ routing and checks
def test_scheduler_hands_the_state_on_only_when_set():
    from imagine360_amd import kernels
    calls = []
    names = ("cfg_ddim_step", "cfg_ddim_step_windows", "ddim_step", "ddim_step_windows", "cfg_multistep_step", "cfg_multistep_step_windows",
             "multistep_step")
    saved = {n: getattr(kernels, n) for n in names}
    for n in names:
        setattr(kernels, n, lambda *a, _n=n, **k: calls.append((_n, k)))
    try:
        x, st, cd = torch.zeros(8), torch.zeros(8), torch.zeros(1)
        sch = _sched()
        t = sch._timesteps_host[3]
        sch.fused_cfg_step(x, x, G, t, x, guidance_apg=(0.0, None))
        sch.fused_cfg_step(x, x, G, t, x, guidance_apg=(0.0, None), guidance_apg_momentum=None, carry_dev=None)
        sch.fused_cfg_step(x, x, G, t, x, guidance_apg=(0.0, None), guidance_apg_momentum=(st, -0.4))
        sch.fused_cfg_step(x, x, G, t, x, guidance_apg=(0.0, 2.0), guidance_apg_momentum=(st, 0.0), carry_dev=cd)
        p, s0, w = torch.zeros(1, 2, 4, 2, 1, 1), torch.zeros(1, dtype=torch.int32), torch.ones(2)
        lat, lst = torch.zeros(1, 4, 2, 1, 1), torch.zeros(1, 4, 2, 1, 1)
        sch.fused_cfg_step_windows(p, s0, w, G, t, lat, guidance_apg=(0.0, None), guidance_apg_momentum=(lst, 0.3), ring=True)
        sch.fused_step(x, t, x, guidance_apg=(0.0, None), guidance_apg_momentum=(st, -0.4), carry_dev=cd)       # unguided: ignored
        sch.fused_step_windows(p[:, :1], s0, w, t, lat, guidance_apg=(0.0, None), guidance_apg_momentum=(lst, 0.3))
        dpm = _sched(cls=DPMSolverMultistepScheduler)
        h = torch.zeros(8)
        dpm.fused_cfg_step(x, x, G, t, x, history=h, guidance_apg=(0.0, None), guidance_apg_momentum=(st, -0.4), carry_dev=cd)
        dpm.fused_cfg_step_windows(p, s0, w, G, t, lat, history=lst.clone(), guidance_apg=(0.0, None), guidance_apg_momentum=(lst, 0.3))
        dpm.fused_step(x, t, x, history=h, guidance_apg=(0.0, None), guidance_apg_momentum=(st, -0.4))
    finally:
        for n, fn in saved.items():
            setattr(kernels, n, fn)
    assert calls[0] == calls[1] == ("cfg_ddim_step", {"coef_dev": None, "apg": (0.0, None)})
    assert calls[2][0] == "cfg_ddim_step" and set(calls[2][1]) == {"coef_dev", "apg", "apg_momentum"}
    assert calls[2][1]["apg_momentum"][0] is st and calls[2][1]["apg_momentum"][1] == -0.4
    assert calls[3][1]["carry_dev"] is cd and calls[3][1]["apg"] == (0.0, 2.0) and calls[3][1]["apg_momentum"][1] == 0.0
    assert calls[4][0] == "cfg_ddim_step_windows" and calls[4][1]["apg_momentum"][0] is lst and calls[4][1]["ring"] is True
    assert calls[5] == ("ddim_step", {"coef_dev": None}) and calls[6] == ("ddim_step_windows", {"coef_dev": None})
    assert calls[7][0] == "cfg_multistep_step" and calls[7][1]["carry_dev"] is cd and calls[7][1]["apg_momentum"][0] is st
    assert calls[8][0] == "cfg_multistep_step_windows" and calls[8][1]["apg_momentum"][1] == 0.3
    assert calls[9] == ("multistep_step", {"coef_dev": None})


def test_wrapper_checks_in_front_of_any_launch():
    """kernels._apg_momentum_args; the device check comes first for CPU tensors, so the value checks are reached through it directly."""
    from imagine360_amd import kernels
    x = torch.zeros(16)
    with pytest.raises(ValueError, match="apg_momentum needs apg"):
        kernels._apg_momentum_args("t", None, (torch.zeros(16), 0.0), None, x)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="carry"):
            kernels._apg_momentum_args("t", (0.0, None), (torch.zeros(16), bad), None, x)
    # the apg tuple keeps its arity
    assert kernels._apg_args("t", (0.5, 2)) == (0.5, 2.0)
    for name in ("im360_cfg_apg_momentum_stats", "im360_cfg_apg_momentum_stats_windows", "im360_cfg_apg_momentum_stats_windows_ring",
                 "im360_cfg_ddim_step_apg_momentum", "im360_cfg_ddim_step_windows_apg_momentum", "im360_cfg_multistep_step_apg_momentum",
                 "im360_cfg_multistep_step_windows_apg_momentum"):
        assert name in kernels.exported_symbols()
    assert kernels.ABI_VERSION == 5


@pytest.mark.parametrize("pt", TYPES)
def test_stand_in_is_the_definition(pt):
    """The stand-in's scalars on e give the definition's m; carry 0 does not read the state and equals the momentum-less stand-in; the
    statistics pass leaves the state alone; one uniform window is the plain stand-in."""
    import _emu_apg_step as EA
    from imagine360_amd.context import context_weights
    u, c, x = (v.float() for v in inputs(8))
    gen = torch.Generator().manual_seed(5)
    prev = 0.3 * torch.randn(u.shape, generator=gen)
    mode = {"epsilon": 0, "v_prediction": 1, "sample": 2}[pt]
    sa, sb = 0.6 ** 0.5, 0.4 ** 0.5
    coefs = (G, sa, sb, 0.9, 0.3, 0.0)
    rho = {"epsilon": -1.0 / sb, "v_prediction": -sa / sb, "sample": 0.0}[pt]
    for apg in ((0.0, None), (0.5, 0.05)):
        state = prev.clone()
        alpha, s, lam = (float(v) for v in EP.cfg_apg_scalars(u, c, x, mode, coefs, apg, apg_momentum=(state, -0.5)))
        assert torch.equal(state, prev)
        e = (c - u) - 0.5 * prev
        m = c + (G - 1.0) * s * e - lam * (c + rho * x)
        want, e64 = projected_guidance(u.double(), c.double(), x.double(), G, sa, sb, pt, *apg, momentum=(prev.double(), -0.5))
        assert max_rel(m.double(), want) < 1e-5 and (apg[1] is None) == (s == 1.0)
        got = EP.cfg_ddim_step(u, c, x, None, mode, coefs, apg=apg, apg_momentum=(state, -0.5))
        assert max_rel(state.double(), e64) < 1e-6
        preds = torch.stack([torch.cat([u, c])])
        st, w = torch.zeros(1, dtype=torch.int32), context_weights(u.shape[2], "uniform")
        state_w = prev.clone()
        assert torch.equal(EP.cfg_ddim_step_windows(preds, x, None, st, w, mode, coefs, apg=apg, apg_momentum=(state_w, -0.5)), got)
        assert torch.equal(state_w, state)
        nan = torch.full_like(prev, float("nan"))
        assert torch.equal(EP.cfg_ddim_step(u, c, x, None, mode, coefs, apg=apg, apg_momentum=(nan, 0.0)),
                           EA.cfg_ddim_step(u, c, x, None, mode, coefs, apg=apg))
        assert torch.equal(nan, c - u)
    with pytest.raises(ValueError, match="needs apg"):
        EP.cfg_ddim_step(u, c, x, None, mode, coefs, apg_momentum=(prev.clone(), 0.0))


# ------------------------------------------------------------------------------------------------ 3. pipeline
@contextlib.contextmanager
def patches():
    """Every kernel the loops reach as its stand-in; yields (APG calls, momentum calls, unguided calls)."""
    with contextlib.ExitStack() as st:
        for cm in (E.patched_kernels(), ER.patched_rescale_kernels(), EG.patched_ring_kernels(), EN.patched_noise_latents(),
                   EM.patched_multistep_kernels(), EF.patched_free_init_noise()):
            st.enter_context(cm)
        unguided = st.enter_context(EU.patched_unguided_kernels())
        apg, mom = st.enter_context(EP.patched_apg_momentum_kernels())
        yield apg, mom, unguided


@contextlib.contextmanager
def logged_wrappers():
    """The six patched wrappers wrapped once more: every call's (name, sorted keywords) in order."""
    import _emu_apg_step as EA
    from imagine360_amd import kernels
    log = []
    saved = {n: getattr(kernels, n) for n in EA.NAMES}

    def wrap(n, fn):
        def call(*a, **k):
            log.append((n, tuple(sorted(k))))
            return fn(*a, **k)
        return call
    for n, fn in saved.items():
        setattr(kernels, n, wrap(n, fn))
    try:
        yield log
    finally:
        for n, fn in saved.items():
            setattr(kernels, n, fn)


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


def pipe_kw(cond, vb, steps=3, **extra):
    return dict(num_inference_steps=steps, guidance_scale_text=7.5, negative_prompt="", video_batch=vb, use_outpaint=True,
                use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video", latents_dtype=torch.float32,
                prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **extra)


def _run(pipe, seed=5, **kw):
    torch.manual_seed(seed)
    random.seed(seed)
    pipe("synthetic", **kw)
    return [v.clone() for v in pipe.last_latents]


VARIANTS = {"plain": {}, "windows": dict(context_frames=2, context_overlap=1), "ring": dict(context_frames=2, context_overlap=1, context_loop=True)}
BETA = -0.5


def _carries(mom):
    """The carry of every step of a run: the two branches of a step share it."""
    assert len(mom) % 2 == 0 and all(mom[i][1] == mom[i + 1][1] for i in range(0, len(mom), 2))
    assert all(mom[i][2] is mom[0][2] and mom[i + 1][2] is mom[1][2] for i in range(0, len(mom), 2)) and mom[0][2] is not mom[1][2]
    return [mom[i][1] for i in range(0, len(mom), 2)]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_none_is_the_call_of_before_and_zero_equals_none(cpu_pipe, clip4, variant, monkeypatch):
    vb, cond = clip4
    extra = VARIANTS[variant]
    made = []
    real = DDIMScheduler.new_apg_state
    monkeypatch.setattr(DDIMScheduler, "new_apg_state", lambda self, latent: made.append(1) or real(self, latent))
    with patches() as (apg, mom, _), logged_wrappers() as log:
        base = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=0.0, apg_threshold=0.5, **extra))
        base_log = list(log)
        del log[:]
        off = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=0.0, apg_threshold=0.5, apg_momentum=None, **extra))
        assert log == base_log and not mom and not made              # the calls of before, keyword for keyword; no state allocated
        assert all("apg_momentum" not in k and "carry_dev" not in k for _, k in log)
        zero = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=0.0, apg_threshold=0.5, apg_momentum=0.0, **extra))
        assert len(made) == 2 and _carries(mom) == [0.0, 0.0, 0.0]
        del mom[:]
        on = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=0.0, apg_threshold=0.5, apg_momentum=BETA, **extra))
        name = "cfg_ddim_step" if variant == "plain" else "cfg_ddim_step_windows"
        assert [m[0] for m in mom] == [name] * 6
        steps = cpu_pipe.scheduler._timesteps_host
        sch = cpu_pipe.scheduler
        assert _carries(mom) == [0.0, sch.apg_carry(steps[0], steps[1], BETA), sch.apg_carry(steps[1], steps[2], BETA)]
    assert all(torch.equal(a, b) for a, b in zip(off, base)) and all(torch.equal(a, b) for a, b in zip(zero, base))
    for a, b in zip(on, base):
        assert torch.isfinite(a).all() and float((a - b).norm() / b.norm()) > 1e-4


def test_unguided_steps_leave_state_and_predecessor_alone(cpu_pipe, clip4):
    """(0.2, 0.6) on 5 steps guides steps 1 and 2 (test_guidance_interval's rule); the guided steps alone make momentum calls, the first
    with carry 0, the second from the first guided timestep."""
    vb, cond = clip4
    sch = cpu_pipe.scheduler
    for variant in ("plain", "ring"):
        with patches() as (apg, mom, unguided):
            _run(cpu_pipe, **pipe_kw(cond, vb, steps=5, guidance_interval=(0.2, 0.6), apg_eta=0.0, apg_momentum=BETA, **VARIANTS[variant]))
            steps = sch._timesteps_host
            flags = sch.guided_steps(steps, (0.2, 0.6))
            gi = [i for i, f in enumerate(flags) if f]
            assert 0 < len(gi) < 5 and not flags[0]
            want = [0.0] + [sch.apg_carry(steps[a], steps[b], BETA) for a, b in zip(gi, gi[1:])]
            assert _carries(mom) == want and len(apg) == 2 * len(gi) and len(unguided) == 2 * (5 - len(gi))


def test_a_gap_in_the_guided_steps_uses_the_last_guided_timestep(monkeypatch, cpu_pipe, clip4):
    """Guided flags with a hole (steps 0 and 2 of 3): the carry of step 2 is apg_carry(t0, t2), not from the unguided t1."""
    vb, cond = clip4
    sch = cpu_pipe.scheduler
    monkeypatch.setattr(type(sch), "guided_steps", lambda self, steps, interval: [True, False, True])
    with patches() as (apg, mom, unguided):
        _run(cpu_pipe, **pipe_kw(cond, vb, steps=3, guidance_interval=(0.2, 0.6), apg_eta=0.0, apg_momentum=BETA))
        steps = sch._timesteps_host
        assert _carries(mom) == [0.0, sch.apg_carry(steps[0], steps[2], BETA)] and len(unguided) == 2


@pytest.mark.parametrize("variant", ["plain", "windows"])
def test_every_free_init_pass_starts_with_carry_zero(cpu_pipe, clip4, variant):
    vb, cond = clip4
    sch = cpu_pipe.scheduler
    with patches() as (apg, mom, _):
        _run(cpu_pipe, **pipe_kw(cond, vb, steps=2, free_init_iters=2, apg_eta=0.0, apg_momentum=BETA, **VARIANTS[variant]))
        steps = sch._timesteps_host
        c1 = sch.apg_carry(steps[0], steps[1], BETA)
        assert _carries(mom) == [0.0, c1, 0.0, c1]


def test_a_shortened_schedule_starts_with_carry_zero(cpu_pipe, clip4):
    vb, cond = clip4
    sch = cpu_pipe.scheduler
    x0 = 0.5 * torch.randn(1, 4, 4, 16, 32, generator=torch.Generator().manual_seed(2))
    with patches() as (apg, mom, _):
        _run(cpu_pipe, **pipe_kw(cond, vb, steps=4, init_latents=x0, strength=0.5, apg_eta=0.0, apg_momentum=BETA))
        steps = sch._timesteps_host
        assert _carries(mom) == [0.0, sch.apg_carry(steps[2], steps[3], BETA)]          # the run enters at step 2 of 4


@pytest.mark.parametrize("variant", ["plain", "ring"])
def test_multistep_scheduler_takes_it(cpu_pipe, clip4, variant):
    vb, cond = clip4
    saved = cpu_pipe.scheduler
    cpu_pipe.scheduler = sch = DPMSolverMultistepScheduler.from_config(saved.config)
    try:
        with patches() as (apg, mom, _):
            base = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=0.0, **VARIANTS[variant]))
            assert not mom
            zero = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=0.0, apg_momentum=0.0, **VARIANTS[variant]))
            del mom[:]
            on = _run(cpu_pipe, **pipe_kw(cond, vb, apg_eta=0.0, apg_momentum=BETA, **VARIANTS[variant]))
            steps = sch._timesteps_host
            assert [m[0] for m in mom] == ["cfg_multistep_step" if variant == "plain" else "cfg_multistep_step_windows"] * 6
            assert _carries(mom) == [0.0, sch.apg_carry(steps[0], steps[1], BETA), sch.apg_carry(steps[1], steps[2], BETA)]
    finally:
        cpu_pipe.scheduler = saved
    assert all(torch.equal(a, b) for a, b in zip(zero, base))
    assert float((on[0] - base[0]).norm() / base[0].norm()) > 1e-4


def test_refusals(cpu_pipe, clip4):
    from imagine360_amd.dist import FrameShard
    vb, cond = clip4
    bad = ((dict(apg_momentum=-0.5), "apg_momentum needs apg_eta"),
           (dict(apg_eta=0.0, apg_momentum=float("nan")), "apg_momentum must be finite"),
           (dict(apg_eta=0.0, apg_momentum=float("inf")), "apg_momentum must be finite"),
           (dict(apg_eta=0.0, apg_momentum=1.0), "apg_momentum must be finite"), (dict(apg_eta=0.0, apg_momentum=-1.0), "apg_momentum must be finite"),
           (dict(apg_eta=0.0, apg_momentum=-1.5), "apg_momentum must be finite"),
           (dict(apg_eta=0.0, apg_momentum=-0.5, guidance_rescale=0.7), "apg_eta cannot be combined with guidance_rescale"),
           (dict(apg_eta=0.0, apg_momentum=-0.5, frame_shard=FrameShard(4, rank=0, world=1)), "apg_eta cannot be combined with frame_shard"))
    with patches() as (apg, mom, _):
        for kw, pat in bad:
            with pytest.raises(ValueError, match=pat):
                _run(cpu_pipe, **pipe_kw(cond, vb, **kw))
        assert not apg and not mom
