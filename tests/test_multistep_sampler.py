"""DPM-Solver++ 2M (scheduler.DPMSolverMultistepScheduler, arXiv 2211.01095 algorithm 2) on CPU: order 1 against the project's DDIM,
order 2 against the closed-form probability-flow solution for Gaussian data, the coefficient vector (table, first / last step,
shortened runs, timesteps outside the run), one history per branch in the pipeline loop, the torch stand-in of the kernels against the
eager ``step``, and what is refused."""
import math
import random

import pytest
import torch

import _emu_kernels as E
import _emu_multistep_step as EM
import _emu_rescale_step as ER
from helpers import rel
from imagine360_amd import configs, synthetic as S
from imagine360_amd.context import context_weights
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, rescale_noise_cfg
from test_context_windows import TOL, pipe_kw, windows_case

torch.set_grad_enabled(False)
KW = configs.NOISE_SCHEDULER_KWARGS
G = 7.5


def _sched(n=None, cls=DPMSolverMultistepScheduler, **over):
    sch = cls(**{**KW, **over})
    if n is not None:
        sch.set_timesteps(n)
    return sch


# ------------------------------------------------------------------------------------------------ 1. order 1 is DDIM
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("pt", ["v_prediction", "epsilon", "sample"])
@pytest.mark.parametrize("n", [8, 20, 50])
def test_order_one_is_ddim(n, pt, clip):
    """First-order DPM-Solver++ is DDIM (eta = 0) in exact arithmetic: out = sigma'/sigma x + (alpha' - sigma' alpha / sigma) x0 =
    alpha' x0 + sigma' (x - alpha x0) / sigma.  The second form is ``DDIMScheduler.step`` with the noise estimate derived from the x0
    it uses -- its ``use_clipped_model_output=True``, which is the identity for unclipped v / epsilon and which clip_sample and
    prediction_type="sample" need (without it the reference's direction term multiplies the raw model output).  fp64, every step of
    the shipped grid, each from fresh inputs scaled so that the clamp bites; bound 1e-12 (the scalar recurrence measured 6e-16)."""
    dpm, ddim = _sched(n, solver_order=1, prediction_type=pt, clip_sample=clip), _sched(n, DDIMScheduler, prediction_type=pt, clip_sample=clip)
    gen = torch.Generator().manual_seed(3)
    worst = 0.0
    for t in dpm._timesteps_host:
        x, m = torch.randn(2, 4, 3, 5, generator=gen, dtype=torch.float64), torch.randn(2, 4, 3, 5, generator=gen, dtype=torch.float64)
        hist = torch.zeros_like(x)
        got = dpm.step(m, t, x, history=hist)
        want = ddim.step(m, t, x, eta=0.0, use_clipped_model_output=True)
        assert got.prev_sample.dtype == torch.float64 and torch.equal(hist, got.pred_original_sample)
        assert rel(got.pred_original_sample, want.pred_original_sample) <= 1e-14
        worst = max(worst, rel(got.prev_sample, want.prev_sample))
        assert torch.equal(dpm.step(m, t, x).prev_sample, got.prev_sample)           # first order needs no history
    assert worst <= 1e-12, worst


# ------------------------------------------------------------------------------------------------ 2. second order on a closed form
def _gaussian_error(sch, n, c):
    """Relative error at the end of an n-step run from x = 1 for data N(0, c^2): the exact x0 predictor alpha c^2 x / (alpha^2 c^2 +
    sigma^2) is handed to the scheduler as a "sample" prediction; the exact ODE solution scales x by sqrt(var_end / var_start)."""
    sch.set_timesteps(n)
    steps = sch._timesteps_host
    x = torch.ones(1, dtype=torch.float64)
    hist = torch.zeros(1, dtype=torch.float64)
    for t in steps:
        a = float(sch.alphas_cumprod[t])
        x0 = math.sqrt(a) * c * c * x / (a * c * c + 1.0 - a)
        x = sch.step(x0, t, x, history=hist).prev_sample if isinstance(sch, DPMSolverMultistepScheduler) else sch.step(x0, t, x, use_clipped_model_output=True).prev_sample
    a0, a1 = float(sch.alphas_cumprod[steps[0]]), float(sch.final_alpha_cumprod)
    exact = math.sqrt((a1 * c * c + 1 - a1) / (a0 * c * c + 1 - a0))
    return abs(float(x) / exact - 1.0)


def test_second_order_on_the_gaussian_closed_form():
    """fp64 on the shipped schedule, the project's DDIM as the yardstick.  Measured (DDIM / 2M), c = 1: N = 20 0.0784 / 0.0600,
    25 0.0636 / 0.0418, 40 0.0408 / 0.0187, 50 0.0331 / 0.0125, 100 0.0172 / 0.00310; c = 0.5: 50 0.0581 / 0.0339, 100 0.0317 /
    0.00909.  Nothing is asserted at N <= 10, where 2M loses (the first step from near-zero SNR is stiff)."""
    kw = dict(prediction_type="sample")
    dpm, ddim = _sched(**kw), _sched(cls=DDIMScheduler, **kw)
    err = {(c, n): (_gaussian_error(ddim, n, c), _gaussian_error(dpm, n, c)) for c, n in
           [(1.0, 20), (1.0, 25), (1.0, 40), (1.0, 50), (1.0, 100), (0.5, 50), (0.5, 100)]}
    for k, (d, m) in err.items():
        print(f"c = {k[0]}, N = {k[1]}: DDIM {d:.4g}, 2M {m:.4g}")
    for n in (20, 25, 40, 50):
        assert err[1.0, n][1] < err[1.0, n][0], (n, err[1.0, n])
    assert err[1.0, 20][1] < err[1.0, 25][0]                        # DDIM's 25-step error in 20 steps
    for c in (0.5, 1.0):
        ratio = err[c, 50][1] / err[c, 100][1]
        assert 3.0 <= ratio <= 5.0, (c, ratio)                       # second order: halving the step quarters the error (DDIM: 1.8 .. 1.9)
    for (c, n), (d, m) in err.items():                               # the figures above, as measured
        want = {(1.0, 20): (0.0784, 0.0600), (1.0, 25): (0.0636, 0.0418), (1.0, 40): (0.0408, 0.0187), (1.0, 50): (0.0331, 0.0125),
                (1.0, 100): (0.0172, 0.00310), (0.5, 50): (0.0581, 0.0339), (0.5, 100): (0.0317, 0.00909)}[c, n]
        assert abs(d / want[0] - 1) < 0.01 and abs(m / want[1] - 1) < 0.01, ((c, n), (d, m), want)


# ------------------------------------------------------------------------------------------------ 3. coefficients
TABLE = {(4, 751): (0.93319, 0.26829, 0.0), (4, 501): (0.72242, 0.66098, -0.18918), (4, 251): (0.06239, 2.40308, -1.45029),
         (4, 1): (0.0, 1.0, 0.0), (8, 126): (0.09685, 2.66285, -1.75110)}


def _fp64_coefficients(sch, steps, i):
    """The definition restated from the issue's formulas with math.* on the fp32 table (independent of the class's code path)."""
    n = sch.num_inference_steps
    ab = lambda t: float(sch.alphas_cumprod[t]) if t >= 0 else float(sch.final_alpha_cumprod)
    lam = lambda a: math.log(math.sqrt(a) / math.sqrt(1 - a))
    t = steps[i]
    a, ap = ab(t), ab(t - 1000 // n)
    if ap == 1.0:
        return 0.0, 1.0, 0.0
    h = lam(ap) - lam(a)
    A = -math.sqrt(ap) * math.expm1(-h)
    cx = math.sqrt(1 - ap) / math.sqrt(1 - a)
    if i == 0 or i == len(steps) - 1:
        return cx, A, 0.0
    r = (lam(a) - lam(ab(steps[i - 1]))) / h
    return cx, A * (1 + 1 / (2 * r)), -A / (2 * r)


def test_coefficients():
    sch = _sched()
    for n in (4, 8, 20, 50):
        sch.set_timesteps(n)
        steps = sch._timesteps_host
        top = [0.0, 0.0]
        for i, t in enumerate(steps):
            g, sa, sb, cx, c0, c1 = sch.multistep_coefficients(steps, i, G)
            assert g == G and (sa, sb) == sch.noise_coefficients(t)
            for got, want in zip((cx, c0, c1), _fp64_coefficients(sch, steps, i)):
                assert abs(got - want) <= 1e-9 * max(abs(want), 1e-300), (n, t, got, want)
            if (n, t) in TABLE:
                # the printed table.  Its five decimals are those of ONE build of the fp32 ``alphas_cumprod``: torch.cumprod over 1000
                # fp32 factors rounds in an order that depends on the CPU (up to 1000 x 2^-24 = 6e-5 relative in a_t), and near the
                # end of the schedule the second-order coefficients amplify that (seen: 2.66285 against 2.66289 at t = 126 on two
                # hosts).  So: 2e-4 against the print, 1e-9 against the formulas on this host's own table (above).
                assert all(abs(a - b) <= 2e-4 * max(1.0, abs(b)) for a, b in zip((cx, c0, c1), TABLE[n, t])), (n, t, cx, c0, c1)
            assert sch.step_coefficients(t, 0.0, G) == (g, sa, sb, cx, c0, c1)          # the run set_timesteps began
            top = [max(top[0], abs(c0)), max(top[1], abs(c1))]
            assert (c1 == 0.0) == (i in (0, n - 1)), (n, i, c1)
        assert sch.multistep_coefficients(steps, n - 1)[3:] == (0.0, 1.0, 0.0)          # final_alpha_cumprod = 1
        if n in (20, 50):
            assert all(abs(a - b) < 6e-3 for a, b in zip(top, {20: (2.42, 1.59), 50: (1.91, 1.19)}[n])), top
    # a shortened run: its first step is first order, its second step uses the lambda of ITS first step
    sch.set_timesteps(8)
    i0, steps = sch.timesteps_for_strength(0.5)
    assert i0 == 4 and steps == sch._timesteps_host[4:]
    full = sch._timesteps_host
    first, second = sch.multistep_coefficients(steps, 0), sch.multistep_coefficients(steps, 1)
    close = lambda a, b: all(abs(x - y) <= 1e-9 * abs(y) for x, y in zip(a, b))
    assert first[5] == 0.0 and close(first[3:5], _fp64_coefficients(sch, steps, 0)[:2]) and sch.multistep_coefficients(full, 4)[5] != 0.0
    assert second == sch.multistep_coefficients(full, 5) and second[5] != 0.0          # (the same predecessor in both lists)
    sch.begin_run(steps)
    assert sch.step_coefficients(steps[0]) == first and sch.step_coefficients(steps[1]) == second
    # a timestep outside the run (the graph warm-up at _timesteps_host[0]): the first-order vector of that timestep
    out = sch.step_coefficients(full[0], 0.0, G)
    assert out == sch.multistep_coefficients(full, 0, G) and out[5] == 0.0
    assert sch.step_coefficients(full[2])[5] == 0.0 and close(sch.step_coefficients(full[2])[3:5], _fp64_coefficients(sch, [full[2]], 0)[:2])
    # solver_order = 1: never a history term
    one = _sched(8, solver_order=1)
    assert all(one.multistep_coefficients(full, i)[5] == 0.0 for i in range(8))
    # zero terminal SNR entered at its last index: no finite lambda
    sch.set_timesteps(500)
    assert sch._timesteps_host[0] == 999 and float(sch.alphas_cumprod[999]) == 0.0
    with pytest.raises(ValueError, match="DDIM"):
        sch.multistep_coefficients(sch._timesteps_host, 0)
    with pytest.raises(ValueError, match="DDIM"):
        sch.step_coefficients(999)
    with pytest.raises(ValueError, match="eta"):
        sch.step_coefficients(501, eta=0.5)


def test_constructor_and_from_config():
    ddim = _sched(cls=DDIMScheduler)
    dpm = DPMSolverMultistepScheduler.from_config(ddim.config)
    assert torch.equal(dpm.alphas_cumprod, ddim.alphas_cumprod) and dpm.config.solver_order == 2 and len(dpm) == len(ddim)
    assert DPMSolverMultistepScheduler.from_config(ddim.config, solver_order=1).config.solver_order == 1
    assert dpm.uses_step_kernel() is True and dpm.kernel_mode() == ddim.kernel_mode()
    assert dpm.new_history(torch.zeros(1, 4, 2, 3, 5, dtype=torch.bfloat16)).dtype == torch.float32
    for bad in (dict(solver_order=3), dict(algorithm_type="sde-dpmsolver++"), dict(algorithm_type="dpmsolver")):
        with pytest.raises(ValueError):
            _sched(**bad)


# ------------------------------------------------------------------------------------------------ 5. stand-in against the eager step
def _blend64(preds, shape, starts, w, ring):
    """fp64 per-frame blends (guided, text) of the windows' predictions, on a line or a ring."""
    fd = len(shape) - 3
    F, L = shape[fd], preds.shape[fd + 1]
    m, cb, ws = (torch.zeros(shape, dtype=torch.float64) for _ in range(3))
    for k, s in enumerate(starts):
        u, c = preds[k, 0:1].double(), preds[k, 1:2].double()
        for j in range(L):
            f = (s + j) % F if ring else s + j
            m.select(fd, f).add_(float(w[j]) * (u + G * (c - u)).select(fd, j))
            cb.select(fd, f).add_(float(w[j]) * c.select(fd, j))
            ws.select(fd, f).add_(float(w[j]))
    return m / ws, cb / ws


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("pt,clip", [("v_prediction", False), ("epsilon", True), ("sample", True)])
def test_stand_in_against_eager_step(dt, pt, clip):
    """A 4-step recurrence (first / second / second / first order): the stand-ins carry the 16-bit latent and the fp32 history from
    step to step, the eager ``step`` runs the same recurrence in fp64 on the same 16-bit predictions with an fp64 history and never
    rounds.  Plain, windows on a line and on a ring, guidance rescale 0.7; bound after every step: TOL of the step kernels for the
    latent and for the history (the history is fp32, but its x0 inherits the rounding of the 16-bit latent it was computed from)."""
    sch = _sched(4, prediction_type=pt, clip_sample=clip)
    steps, mode = sch._timesteps_host, sch.kernel_mode()
    shape, L = (1, 4, 12, 4, 8), 8
    w = context_weights(L, "pyramid")
    worst = 0.0
    for kind, starts in (("plain", None), ("line", [0, 4]), ("ring", [0, 6])):
        for phi in (0.0, 0.7):
            x16 = windows_case(shape, L, [0], dt, seed=7)[1]
            x64, h64 = x16.double(), torch.zeros(shape, dtype=torch.float64)
            hist = torch.full(shape, float("nan"))                        # the first step must not read it
            for i, t in enumerate(steps):
                coefs = sch.step_coefficients(t, 0.0, G)
                if kind == "plain":
                    gen = torch.Generator().manual_seed(20 + i)
                    u, c = ((torch.randn(shape, generator=gen) * 0.25).to(dt) for _ in range(2))
                    m, cb = u.double() + G * (c.double() - u.double()), c.double()
                    x16 = EM.cfg_multistep_step(u, c, x16, hist, mode, coefs, rescale=phi)
                else:
                    preds = windows_case(shape, L, starts, dt, seed=30 + i)[0]
                    m, cb = _blend64(preds, shape, starts, w, kind == "ring")
                    x16 = EM.cfg_multistep_step_windows(preds, x16, hist, torch.tensor(starts, dtype=torch.int32), w, mode, coefs, rescale=phi,
                                                        ring=kind == "ring")
                x64 = sch.step(rescale_noise_cfg(m, cb, phi), t, x64, history=h64).prev_sample
                assert x16.dtype == dt and hist.dtype == torch.float32 and x64.dtype == torch.float64
                e, eh = rel(x16, x64), rel(hist, h64)
                worst = max(worst, e, eh)
                assert e < TOL[dt] and eh < TOL[dt], (kind, phi, i, e, eh)
    print(f"multistep stand-in vs eager step {dt} {pt}: worst rel over the recurrences {worst:.3g}")
    # device coefficients are the host ones; one uniform window is the plain stand-in
    u, c, x = ((torch.randn(shape, generator=torch.Generator().manual_seed(k)) * 0.5).to(dt) for k in (1, 2, 3))
    coefs = sch.step_coefficients(steps[1], 0.0, G)
    h1, h2, h3 = (torch.ones(shape) for _ in range(3))
    a = EM.cfg_multistep_step(u, c, x, h1, mode, coefs)
    assert torch.equal(EM.cfg_multistep_step(u, c, x, h2, mode, (0.0,) * 6, coef_dev=torch.tensor(coefs, dtype=torch.float64)), a)
    one = EM.cfg_multistep_step_windows(torch.stack([torch.cat([u, c])]), x, h3, torch.zeros(1, dtype=torch.int32),
                                        context_weights(shape[2], "uniform"), mode, coefs)
    assert torch.equal(one, a) and torch.equal(h1, h3) and torch.equal(h1, h2)


# ------------------------------------------------------------------------------------------------ 4. / 6. the pipeline
@pytest.fixture(scope="module")
def cpu_run():
    """The w/5 synthetic pipeline, 4 frames, 4 steps, host RNG, emulated kernels: run(scheduler, **keywords) -> the two latents."""
    from imagine360_amd.pipeline import AnimationPipeline
    mv = configs.build_mv_model(5, device="cpu", dtype=torch.float32, xformers=False)
    vae = configs.build_vae(4, device="cpu", dtype=torch.float32)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, None, None, "SAM")
    pipe.rng, pipe._no_progress = "host", True
    pipe.enable_vae_slicing()
    vb, cond = S.video_batch(frames=4, pano_hw=(128, 256), seed=4), S.conditioning(frames=16, seed=4)

    def run(scheduler, steps=4, **kw):
        pipe.scheduler = scheduler
        with E.patched_kernels(), ER.patched_rescale_kernels(), EM.patched_multistep_kernels():
            torch.manual_seed(13)
            random.seed(13)
            args = pipe_kw(cond, vb, latents_dtype=torch.float32, **kw)
            args["num_inference_steps"] = steps
            pipe("synthetic", **args)
        return [v.clone() for v in pipe.last_latents]
    run.pipe = pipe
    return run


def test_each_branch_has_its_own_history(cpu_run):
    """4 steps (first / second / second / first order) of the pipeline loop on the stand-ins, the scheduler's calls recorded.  Each
    branch is handed one history tensor over the whole run, not the other branch's; and the panorama of the run equals a run in which
    only the panorama history exists -- its four updates replayed alone on a fresh history from the recorded inputs -- and the same
    for the perspective branch.  A history kept inside the scheduler, written by the two calls of every step in turn, fails this."""
    sch = _sched()
    calls = []
    orig = sch.fused_cfg_step

    def spy(u, c, g, t, x, coef_dev=None, *, history=None, **kw):
        rec = dict(u=u.clone(), c=c.clone(), t=t, x=x.clone(), hist_id=id(history), hist_ptr=history.data_ptr(), kw=kw)
        out = orig(u, c, g, t, x, coef_dev, history=history, **kw)
        rec.update(out=out.clone(), hist_after=history.clone())
        calls.append(rec)
        return out
    sch.fused_cfg_step = spy
    got = cpu_run(sch)
    pano, pers = calls[0::2], calls[1::2]
    assert len(calls) == 8 and [r["t"] for r in pano] == [r["t"] for r in pers] == sch._timesteps_host
    assert len({r["hist_ptr"] for r in pano}) == 1 and len({r["hist_ptr"] for r in pers}) == 1 and pano[0]["hist_ptr"] != pers[0]["hist_ptr"]
    for branch, final in ((pano, got[0]), (pers, got[1])):
        # a run in which only this branch's history exists: replay its four updates alone on a fresh history
        hist = sch.new_history(branch[0]["x"])
        with EM.patched_multistep_kernels():
            for r in branch:
                assert r["hist_after"].shape == r["x"].shape
                out = orig(r["u"], r["c"], G, r["t"], r["x"], history=hist)
                assert torch.equal(out, r["out"]) and torch.equal(hist, r["hist_after"]), r["t"]
        assert torch.equal(branch[-1]["out"], final)
    # and the history is really used: order 1 is another clip
    one = cpu_run(_sched(solver_order=1))
    assert rel(one[0], got[0]) > 1e-3 and rel(one[1], got[1]) > 1e-3


def test_pipeline_equals_eager_step_loop(cpu_run):
    """The pipeline on the stand-ins == per branch u + g (c - u) -> ``scheduler.step(history=)`` in fp32 (bound of
    test_guidance_rescale.py for fp32 latents after a few steps), for the plain loop, with guidance_rescale, and under context windows it
    stays finite and differs from order 1."""
    for phi in (0.0, 0.7):
        kw = dict(guidance_rescale=phi) if phi else {}
        got = cpu_run(_sched(), **kw)
        sch = _sched()

        def step(u, c, g, t, x, coef_dev=None, *, history=None, **k):
            return sch.step(rescale_noise_cfg(u + g * (c - u), c, phi), t, x, history=history).prev_sample
        sch.fused_cfg_step = step
        want = cpu_run(sch, **kw)
        for a, b in zip(got, want):
            assert torch.isfinite(a).all() and rel(a, b) < 1e-4, (phi, rel(a, b))


def test_refusals_and_ddim_calls_unchanged(cpu_run):
    from imagine360_amd.dist import FrameShard
    with pytest.raises(ValueError, match="eta=0.5 cannot be combined with DPMSolverMultistepScheduler.*DDIMScheduler"):
        cpu_run(_sched(), eta=0.5)
    with pytest.raises(ValueError, match="frame_shard cannot be combined with DPMSolverMultistepScheduler.*history"):
        cpu_run(_sched(), frame_shard=FrameShard(4, rank=0, world=1))
    sch = _sched()
    x = torch.zeros(8)
    sch.set_timesteps(4)
    with pytest.raises(ValueError, match="history"):
        sch.fused_cfg_step(x, x, G, 751, x)
    with pytest.raises(ValueError, match="eta"):
        sch.fused_cfg_step(x, x, G, 751, x, history=x, eta=0.5, noise=x)
    with pytest.raises(ValueError, match="use_clipped_model_output"):
        sch.fused_cfg_step(x, x, G, 751, x, history=x, use_clipped_model_output=True)
    with pytest.raises(ValueError, match="needs the history"):
        sch.step(x, 501, x)
    # DDIM: the pipeline calls fused_cfg_step with exactly today's arguments -- positional (u, c, g, t, latent) and the one keyword
    ddim = _sched(cls=DDIMScheduler)
    seen = []
    orig = ddim.fused_cfg_step
    ddim.fused_cfg_step = lambda *a, **k: (seen.append((len(a), dict(k))), orig(*a, **k))[1]
    cpu_run(ddim, steps=2)
    assert seen == [(5, {"guidance_rescale": 0.0})] * 4
