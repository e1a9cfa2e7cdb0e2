"""DPM-Solver++ 2M on the MI355X: cfg_multistep_step_kernel / cfg_multistep_step_windows_kernel (csrc/sampler_step.hip) against fp64 for
every mode, first and second order, with and without the guidance rescale; the fp32 history (never rounded to 16 bits, not read when
c1 == 0, updated in place); one uniform window against the plain kernel bit for bit; both entry points between guard bands; their
refusals; and the pipeline with ``DPMSolverMultistepScheduler``: captured steps against eager ones for every loop variant, order 1
against DDIM, order 2 against order 1."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from _emu_keep_latents import half_mask, kept  # noqa: E402
from _emu_noise_latents import same_bits  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record as _record, rel  # noqa: E402
from imagine360_amd import configs, kernels as K, synthetic as S  # noqa: E402
from imagine360_amd.context import context_weights  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402
from test_context_windows import pipe_kw, windows_case  # noqa: E402
from test_context_windows_gpu import KERNEL_CASES  # noqa: E402
from test_ddim_stochastic_gpu import TOL  # noqa: E402

torch.set_grad_enabled(False)
G = 7.5
SHAPE = (1, 4, 5, 7, 24)   # 3360 elements: 420 lanes of 8, not a multiple of the 256-thread block
HIST_TOL = 1e-5            # the history is fp32 and never rounded to 16 bits: x0 from 16-bit inputs in fp32 arithmetic (2^-24 per operation)


def _coefs():
    """(first order, second order) vectors of the shipped grid: N = 8 at t = 876 (first step) and at t = 126, the step with the
    largest |c0|, |c1| of the issue's table (2.66, -1.75)."""
    sch = DPMSolverMultistepScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(8)
    st = sch._timesteps_host
    first, second = sch.multistep_coefficients(st, 0, G), sch.multistep_coefficients(st, 6, G)
    assert st[6] == 126 and first[5] == 0.0 and abs(second[4] - 2.66285) < 1e-3 and abs(second[5] + 1.75110) < 1e-3      # (the fp32 table differs from host to host in its last bits)
    return first, second


def _factor64(m, c, phi):
    return 1.0 if phi == 0.0 else float(phi * c.double().std() / m.double().std() + (1.0 - phi))


def _host_multistep(m, x, h, mode, coefs):
    """fp64: (out, x0) of the multistep update on the guided prediction m; h is used only when c1 != 0."""
    _, sa, sb, cx, c0, c1 = coefs
    m, x = m.double(), x.double()
    pred = mode & 3
    x0 = (x - sb * m) / sa if pred == 0 else sa * x - sb * m if pred == 1 else m
    if mode & 4:
        x0 = x0.clamp(-1, 1)
    out = cx * x + c0 * x0
    if c1 != 0.0:
        out = out + c1 * h.double()
    return out, x0


def _blend64(preds, x, starts, w, ring):
    """fp64 per-frame blends of u_k + G (c_k - u_k) and of c_k; frames (start + j) mod F on a ring."""
    fd = x.dim() - 3
    Fr, L = x.shape[fd], preds.shape[fd + 1]
    shape = [1] * x.dim()
    shape[fd] = L
    wv = w.double().reshape(shape)
    m, cb, ws = (torch.zeros(x.shape, dtype=torch.float64) for _ in range(3))
    for k, s in enumerate(starts):
        idx = (s + torch.arange(L)) % Fr
        assert ring or s + L <= Fr
        u, c = preds[k, 0:1].double(), preds[k, 1:2].double()
        m.index_add_(fd, idx, wv * (u + G * (c - u)))
        cb.index_add_(fd, idx, wv * c)
        ws.index_add_(fd, idx, wv.expand_as(u).contiguous())
    return m / ws, cb / ws


def _hist(shape, seed=5):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 0.7


# ------------------------------------------------------------------------------------------------ 1. kernels against fp64
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_multistep_step_kernel_all_modes(dt):
    gen = torch.Generator().manual_seed(52)
    u, c, x = (torch.randn(SHAPE, generator=gen).to(dt) for _ in range(3))
    u, c = u * 0.25, c * 0.25                # a guided x0 partly inside, partly outside [-1, 1]
    h = _hist(SHAPE)
    du, dc, dx = u.cuda(), c.cuda(), x.cuda()
    m = u.double() + G * (c.double() - u.double())
    errs, herrs = {}, {}
    for order, coefs in enumerate(_coefs(), 1):
        coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
        for mode in (0, 1, 2, 4, 5, 6):
            for phi in (0.0, 0.7):
                ref, x0 = _host_multistep(m * _factor64(m, c, phi), x, h, mode, coefs)
                dh = h.cuda()
                out = K.cfg_multistep_step(du, dc, dx, dh, mode, coefs, rescale=phi)
                assert out.dtype == dt and out.shape == SHAPE and dh.dtype == torch.float32
                key = f"order{order}_mode{mode}_phi{phi}"
                errs[key], herrs[key] = e, eh = rel(out, ref), rel(dh, x0)
                print(f"cfg_multistep_step {dt} {key}: out {e:.3g} hist {eh:.3g}")
                assert e < TOL[dt] and eh < HIST_TOL, (key, e, eh)
                dh2 = h.cuda()
                out2 = K.cfg_multistep_step(du, dc, dx, dh2, mode, (0.0,) * 6, coef_dev=coef_dev, rescale=phi)
                assert torch.equal(out2, out) and torch.equal(dh2, dh), key
        if order == 2:                        # the history term is used
            assert rel(out, _host_multistep(m * _factor64(m, c, 0.7), x, h * 0, 6, coefs)[0]) > 1e-1
    _record(f"cfg_multistep_step_{str(dt).split('.')[-1]}", max_rel=max(errs.values()), max_hist_rel=max(herrs.values()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_multistep_windows_kernel_all_modes_vs_fp64(dt):
    errs, herrs = {}, {}
    for ci, (shape, L, starts) in enumerate(KERNEL_CASES):
        F = shape[len(shape) - 3]
        ring_starts = [(s + F - 3) % F for s in starts] if len(starts) > 1 else None       # rolled by 3 frames: windows cross the end
        for ring, st_host in ((False, starts), (True, ring_starts)):
            if st_host is None:
                continue
            preds, x, _ = windows_case(shape, L, starts, dt, seed=60 + ci)
            h = _hist(shape, seed=9 + ci)
            dp, dx = preds.cuda(), x.cuda()
            st = torch.tensor(st_host, dtype=torch.int32, device="cuda")
            w = context_weights(L, "pyramid")
            dw = w.cuda()
            m, cb = _blend64(preds, x, st_host, w, ring)
            for order, coefs in enumerate(_coefs(), 1):
                coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
                for mode in (0, 1, 2, 4, 5, 6):
                    for phi in (0.0, 0.7):
                        ref, x0 = _host_multistep(m * _factor64(m, cb, phi), x, h, mode, coefs)
                        dh = h.cuda()
                        out = K.cfg_multistep_step_windows(dp, dx, dh, st, dw, mode, coefs, rescale=phi, ring=ring)
                        assert out.dtype == dt and out.shape == x.shape
                        key = f"case{ci}_ring{int(ring)}_order{order}_mode{mode}_phi{phi}"
                        errs[key], herrs[key] = e, eh = rel(out, ref), rel(dh, x0)
                        assert e < TOL[dt] and eh < HIST_TOL, (key, e, eh)
                        dh2 = h.cuda()
                        out2 = K.cfg_multistep_step_windows(dp, dx, dh2, st, dw, mode, (0.0,) * 6, coef_dev=coef_dev, rescale=phi, ring=ring)
                        assert torch.equal(out2, out) and torch.equal(dh2, dh), key
    print(f"cfg_multistep_step_windows {dt}: max rel out {max(errs.values()):.3g} hist {max(herrs.values()):.3g}")
    _record(f"cfg_multistep_step_windows_{str(dt).split('.')[-1]}", max_rel=max(errs.values()), max_hist_rel=max(herrs.values()))


# ------------------------------------------------------------------------------------------------ 2. / 3. the history
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_no_history_read_at_c1_zero_and_history_in_place(dt):
    """c1 == 0: a history full of NaN reaches neither ``out`` nor the new history (host and device coefficients, plain and windows,
    lanes and the scalar path).  Then a second-order call on the history the first call left: the fp64 two-step recurrence."""
    first, second = _coefs()
    gen = torch.Generator().manual_seed(77)
    u, c, x, u2, c2 = ((torch.randn(SHAPE, generator=gen) * s).to(dt) for s in (0.25, 0.25, 1.0, 0.25, 0.25))
    nan = torch.full(SHAPE, float("nan"), device="cuda")
    for coef_dev in (None, torch.tensor(first, dtype=torch.float32, device="cuda")):
        for phi in (0.0, 0.7):
            dh = nan.clone()
            out = K.cfg_multistep_step(u.cuda(), c.cuda(), x.cuda(), dh, 1, first if coef_dev is None else (0.0,) * 6, coef_dev=coef_dev, rescale=phi)
            assert torch.isfinite(out.float()).all() and torch.isfinite(dh).all(), (coef_dev is None, phi)
    for shape, L, starts in KERNEL_CASES[:2]:                      # 16-byte lanes / the scalar path
        preds, xs, _ = windows_case(shape, L, starts, dt, seed=3)
        dh = torch.full(shape, float("nan"), device="cuda")
        out = K.cfg_multistep_step_windows(preds.cuda(), xs.cuda(), dh, torch.tensor(starts, dtype=torch.int32, device="cuda"),
                                           context_weights(L, "pyramid").cuda(), 1, first)
        assert torch.isfinite(out.float()).all() and torch.isfinite(dh).all(), shape
    # two successive calls on the same history
    dh = nan.clone()
    ptr = dh.data_ptr()
    x1 = K.cfg_multistep_step(u.cuda(), c.cuda(), x.cuda(), dh, 1, first)
    h1 = dh.clone()
    x2 = K.cfg_multistep_step(u2.cuda(), c2.cuda(), x1, dh, 1, second)
    assert dh.data_ptr() == ptr
    m1, m2 = u.double() + G * (c.double() - u.double()), u2.double() + G * (c2.double() - u2.double())
    r1, x0_1 = _host_multistep(m1, x, None, 1, first)
    assert rel(x1, r1) < TOL[dt] and rel(h1, x0_1) < HIST_TOL
    r2, x0_2 = _host_multistep(m2, x1.cpu(), h1.cpu(), 1, second)          # the recurrence on the kernel's own first step ...
    e2, eh2 = rel(x2, r2), rel(dh, x0_2)
    r2f, _ = _host_multistep(m2, r1, x0_1, 1, second)                        # ... and never rounded in between
    e2f = rel(x2, r2f)
    print(f"two-step recurrence {dt}: step 2 on the kernel's step 1 {e2:.3g} (hist {eh2:.3g}); against the unrounded recurrence {e2f:.3g}")
    _record(f"cfg_multistep_two_steps_{str(dt).split('.')[-1]}", step2=e2, step2_hist=eh2, unrounded=e2f)
    assert e2 < TOL[dt] and eh2 < HIST_TOL and e2f < TOL[dt]


# ------------------------------------------------------------------------------------------------ 4. one uniform window
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_one_uniform_window_is_the_plain_kernel_bit_for_bit(dt):
    for shape in ((1, 4, 5, 7, 24), (1, 3, 4, 5, 4, 8), (1, 4, 8, 5, 7)):      # panorama / perspective lanes, the scalar path (inner 35)
        L = shape[-3]
        preds, x, _ = windows_case(shape, L, [0], dt, seed=80)
        preds[0, 0].view(-1)[:64] = 0.0                                 # exact zeros of both signs through the blend
        preds[0, 1].view(-1)[:64] = 0.0
        preds[0, 1].view(-1)[:32] = -0.0
        dp, dx = preds.cuda(), x.cuda()
        h = _hist(shape)
        w = context_weights(L, "uniform").cuda()
        for ring in (False, True):
            st = torch.zeros(1, dtype=torch.int32, device="cuda")
            for coefs in _coefs():
                for mode in (0, 1, 2, 4, 5, 6):
                    for phi in (0.0, 0.7):
                        ha, hb = h.cuda(), h.cuda()
                        a = K.cfg_multistep_step_windows(dp, dx, ha, st, w, mode, coefs, rescale=phi, ring=ring)
                        b = K.cfg_multistep_step(dp[0, 0:1].contiguous(), dp[0, 1:2].contiguous(), dx, hb, mode, coefs, rescale=phi)
                        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (shape, ring, coefs[5], mode, phi)
                        assert torch.equal(ha.view(torch.int32), hb.view(torch.int32)), (shape, ring, coefs[5], mode, phi)


# ------------------------------------------------------------------------------------------------ 5. guarded buffers
def _dn(g, t, **kw):
    return g.guard(t.cuda(), **kw)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_multistep_step_between_guard_bands(dt):
    """The plain entry point: inputs, the history (read and written in place) and the result between poisoned guards, first and
    second order, with and without the rescale workspace."""
    gen = torch.Generator().manual_seed(31)
    u, c, x = ((torch.randn(SHAPE, generator=gen) * s).to(dt) for s in (0.25, 0.25, 1.0))
    h = _hist(SHAPE)
    m = u.double() + G * (c.double() - u.double())
    for coefs in _coefs():
        for phi in (0.0, 0.7):
            ref, x0 = _host_multistep(m * _factor64(m, c, phi), x, h, 1 | 4, coefs)
            g = Guarded(K)
            du, dc, dx = (_dn(g, t) for t in (u, c, x))
            dh = g.empty(SHAPE, torch.float32, "cuda") if coefs[5] == 0.0 else _dn(g, h)     # first order: poisoned, must be written whole
            with g:
                out = g.out(K.cfg_multistep_step(du, dc, dx, dh, 1 | 4, coefs, rescale=phi))
                g.out(dh)
                wss = [a for a in g.allocs if a.dtype == torch.float32 and a.shape != SHAPE]
            assert rel(out, ref) < TOL[dt] and rel(dh, x0) < HIST_TOL, (coefs[5], phi)
            assert len(wss) == (1 if phi else 0)


def _windows_case(dt, inner_hw, ring, seed):
    Fr, L = 6, 4
    starts = [0, 3] if ring else [0, 2]                     # ring: frames 0-3 and 3, 4, 5, 0; line: 0-3 and 2-5
    shape = (1, 4, Fr) + inner_hw
    gen = torch.Generator().manual_seed(seed)
    preds = (torch.randn(2, 2, 4, L, *inner_hw, generator=gen) * 0.25).to(dt)
    x = torch.randn(shape, generator=gen).to(dt)
    return preds, x, _hist(shape, seed), starts, torch.tensor([1.0, 2.0, 2.0, 1.0])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("inner_hw", [(1, 8), (3, 8), (1, 7)])      # inner 8 and 24: 16-byte lanes; 7: the scalar path (V = 1 tail)
def test_multistep_step_windows_between_guard_bands(dt, ring, inner_hw):
    preds, x, h, starts, w = _windows_case(dt, inner_hw, ring, seed=160)
    m, cb = _blend64(preds, x, starts, w, ring)
    for coefs in _coefs():
        for phi in (0.0, 0.7):
            ref, x0 = _host_multistep(m * _factor64(m, cb, phi), x, h, 1 | 4, coefs)
            g = Guarded(K)
            dp, dx = _dn(g, preds), _dn(g, x)
            ds, dw = _dn(g, torch.tensor(starts, dtype=torch.int32)), _dn(g, w)
            dh = g.empty(x.shape, torch.float32, "cuda") if coefs[5] == 0.0 else _dn(g, h)
            with g:
                out = g.out(K.cfg_multistep_step_windows(dp, dx, dh, ds, dw, 1 | 4, coefs, rescale=phi, ring=ring))
                g.out(dh)
            assert rel(out, ref) < TOL[dt] and rel(dh, x0) < HIST_TOL, (coefs[5], phi)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("which", ["sample_out", "hist"])
def test_multistep_step_windows_misaligned_pair_falls_back_to_scalar(dt, which):
    """inner = 8 would take 16-byte lanes; a sample / out pair 2 bytes off its alignment, or a history 4 bytes off its, forces V = 1."""
    preds, x, h, starts, w = _windows_case(dt, (1, 8), False, seed=170)
    m, _ = _blend64(preds, x, starts, w, False)
    second = _coefs()[1]
    ref, x0 = _host_multistep(m, x, h, 1 | 4, second)
    g = Guarded(K)
    dp = _dn(g, preds)
    dx = _dn(g, x, misalign=2 if which == "sample_out" else 0)
    dh = _dn(g, h, misalign=4 if which == "hist" else 0)
    ds, dw = _dn(g, torch.tensor(starts, dtype=torch.int32)), _dn(g, w)
    with g:
        out = g.empty(x.shape, dt, "cuda", misalign=2 if which == "sample_out" else 0)
        assert (dx.data_ptr() | dh.data_ptr() | out.data_ptr()) % 16 != 0
        K._check(K.lib().im360_cfg_multistep_step_windows(dp.data_ptr(), dx.data_ptr(), dh.data_ptr(), out.data_ptr(), ds.data_ptr(), dw.data_ptr(),
                                                          2, 4, 6, 4, 8, 0, *second, 1 | 4, 0.0, None, 0, K._dt(dx), K._stream(), None), "multistep_step_windows")
        g.out(out, dh)
    assert rel(out, ref) < TOL[dt] and rel(dh, x0) < HIST_TOL


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_multistep_kernels_reject_bad_arguments():
    a = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    h = torch.zeros(24, dtype=torch.float32, device="cuda")
    coefs = (7.5, 0.5, 0.8, 0.6, 0.7, -0.3)
    for bad in (None, h[:12], h[:16].half(), h[:16].cpu(), h[::2][:8]):                      # null, short, not fp32, not on the device, strided
        with pytest.raises((ValueError, RuntimeError), match="history|cuda"):
            K.cfg_multistep_step(a, a, a, bad, 1, coefs)
    with pytest.raises(ValueError, match="bit 8"):
        K.cfg_multistep_step(a, a, a, h[:16], 1 | 8, coefs)
    with pytest.raises(RuntimeError, match="mode 3 unsupported"):
        K.cfg_multistep_step(a, a, a, h[:16], 3, coefs)
    with pytest.raises(RuntimeError, match="misaligned"):
        K.cfg_multistep_step(a, a, a, h[1:17], 1, coefs)                                     # 4 bytes off: the two float4 of a lane
    with pytest.raises(RuntimeError, match="multiple of 8"):
        K.cfg_multistep_step(a[:12], a[:12], a[:12], h[:12], 1, coefs)
    with pytest.raises(RuntimeError, match="must be finite"):
        K.cfg_multistep_step(a, a, a, h[:16], 1, coefs, rescale=float("nan"))
    with pytest.raises(TypeError):
        K.cfg_multistep_step(a.float(), a.float(), a.float(), h[:16], 1, coefs)
    lib, p, hp = K.lib(), a.data_ptr(), h.data_ptr()
    ws = torch.zeros(K.RESCALE_RECORD, dtype=torch.float32, device="cuda")
    tail = lambda phi, w, n: (phi, w, n, 0, None, None)
    rc = lib.im360_cfg_multistep_step(p, p, p, None, p, 16, *coefs, 1, *tail(0.0, None, 0))
    assert rc != 0 and b"null pointer" in lib.im360_last_error()
    rc = lib.im360_cfg_multistep_step(p, p, p, hp, p, 16, *coefs, 1 | 8, *tail(0.0, None, 0))
    assert rc != 0 and b"bit 8" in lib.im360_last_error()
    rc = lib.im360_cfg_multistep_step(p, p, p, hp, p, 16, *coefs, 1, *tail(0.7, None, 0))
    assert rc != 0 and b"needs the workspace" in lib.im360_last_error()                     # phi without a workspace
    rc = lib.im360_cfg_multistep_step(p, p, p, hp, p, 256 * 8 * 3, *coefs, 1, *tail(0.7, ws.data_ptr(), 8))
    assert rc != 0 and b"workspace of 8 floats, 24 needed" in lib.im360_last_error()
    rc = lib.im360_cfg_multistep_step(p, p, p, hp, p, 16, *coefs, 1, 0.0, None, 0, 7, None, None)
    assert rc != 0 and b"dtype 7 unsupported" in lib.im360_last_error()
    # windows
    x = torch.zeros(1, 4, 4, 2, 8, dtype=torch.bfloat16, device="cuda")
    pr = torch.zeros(2, 2, 4, 2, 2, 8, dtype=torch.bfloat16, device="cuda")
    hx = torch.zeros(x.numel() + 8, dtype=torch.float32, device="cuda")
    st, w = torch.tensor([0, 2], dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    with pytest.raises(ValueError, match="history"):
        K.cfg_multistep_step_windows(pr, x, hx[:100], st, w, 1, coefs)
    with pytest.raises(ValueError, match="bit 8"):
        K.cfg_multistep_step_windows(pr, x, hx[:x.numel()], st, w, 1 | 8, coefs)
    with pytest.raises(RuntimeError, match="mode 3 unsupported"):
        K.cfg_multistep_step_windows(pr, x, hx[:x.numel()], st, w, 3, coefs)
    q, geo = x.data_ptr(), (2, 4, 4, 2, 16)
    call = lambda hist, wrap, mode=1, phi=0.0, wsp=None, wsn=0, g=geo: lib.im360_cfg_multistep_step_windows(
        pr.data_ptr(), q, hist, q, st.data_ptr(), w.data_ptr(), *g, wrap, *coefs, mode, phi, wsp, wsn, 0, None, None)
    for wrap in (1, 2, 5, -4):
        assert call(hx.data_ptr(), wrap) != 0 and b"wrap=" in lib.im360_last_error()         # neither 0 nor F = 4
    assert call(None, 0) != 0 and b"null pointer" in lib.im360_last_error()
    assert call(hx.data_ptr() + 2, 0) != 0 and b"misaligned history" in lib.im360_last_error()
    assert call(hx.data_ptr(), 0, phi=0.7) != 0 and b"needs the workspace" in lib.im360_last_error()
    assert call(hx.data_ptr(), 0, mode=1 | 8) != 0 and b"bit 8" in lib.im360_last_error()
    assert call(hx.data_ptr(), 0, g=(2, 4, 4, 5, 16)) != 0 and b"out of range" in lib.im360_last_error()          # L > F
    assert call(hx.data_ptr(), 0) == 0 and call(hx.data_ptr(), 4) == 0 and call(hx.data_ptr() + 4, 4) == 0         # and unbroken they are accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. pipeline
@pytest.fixture(scope="module")
def gpu_run():
    """The w/5 synthetic pipeline of test_guidance_rescale_gpu.py::gpu_run (128 x 256, 8 frames, bf16) with a scheduler per call:
    run(scheduler, use_graph, frames, steps, **keywords) -> (video, panorama latent, perspective latent)."""
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, None, None, "SAM").to(dev)
    pipe._no_progress = True
    data = {}

    def run(scheduler, use_graph, frames=8, steps=4, seed=33, **kw):
        if frames not in data:
            data[frames] = S.video_batch(frames=frames, pano_hw=(128, 256), seed=12), S.conditioning(frames=max(frames, 16), seed=12)
        vb, cond = data[frames]
        pipe.scheduler, pipe.use_graph = scheduler, use_graph
        torch.manual_seed(seed)
        random.seed(seed)
        args = pipe_kw(cond, vb, latents_dtype=dt, **kw)
        args["num_inference_steps"] = steps
        vid = pipe("synthetic", **args).videos
        torch.cuda.synchronize()
        return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone()
    run.pipe = pipe
    return run


def _dpm(**kw):
    return DPMSolverMultistepScheduler(**configs.NOISE_SCHEDULER_KWARGS, **kw)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def init_clip(gpu_run):
    """A clean panorama latent to start from: the plain graphed 4-step run."""
    return gpu_run(_dpm(), True)


VARIANTS = {"plain": {}, "windows": dict(frames=24, context_frames=16, context_overlap=8),
            "context_loop": dict(frames=24, context_frames=16, context_overlap=8, context_loop=True),
            "guidance_rescale": dict(guidance_rescale=0.7)}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_graphed_multistep_steps_equal_eager_bit_for_bit(gpu_run, name, monkeypatch):
    """4 steps (first / second / second / first order): the captured step with its own histories replays the eager loop's numbers."""
    from imagine360_amd import graph_step
    kw = VARIANTS[name]
    cls = graph_step.GraphedWindowedStep if "context_frames" in kw else graph_step.GraphedDenoiseStep
    replays = []
    orig = cls.step
    monkeypatch.setattr(cls, "step", lambda self, t: (replays.append(self.sch.step_coefficients(t)[5] != 0.0), orig(self, t))[1])
    graphed, eager = gpu_run(_dpm(), True, **kw), gpu_run(_dpm(), False, **kw)
    assert replays == [False, True, True, False]
    errs = dict(pano=rel(graphed[1], eager[1]), pers=rel(graphed[2], eager[2]))
    _record(f"multistep_graphed_vs_eager_{name}", **errs)
    assert _same(graphed, eager), errs
    assert all(torch.isfinite(v.float()).all() for v in graphed)


def test_graphed_multistep_strength_and_keep_mask(gpu_run, init_clip):
    """strength = 0.5 of 8 steps: the run is the last four timesteps and the graph warm-up's timestep (the schedule's first) is outside
    it.  Then the same with a half ``regenerate_mask``: graphed equals eager, and the kept region is the init clip bit for bit."""
    x0 = init_clip[1]
    kw = dict(steps=8, init_latents=x0, strength=0.5)
    sch = _dpm()
    graphed, eager = gpu_run(sch, True, **kw), gpu_run(_dpm(), False, **kw)
    assert sch._run_steps == sch._timesteps_host[4:] and sch._timesteps_host[0] not in sch._run_steps
    errs = dict(pano=rel(graphed[1], eager[1]), pers=rel(graphed[2], eager[2]), vs_init=rel(graphed[1], x0))
    _record("multistep_graphed_vs_eager_strength", **errs)
    assert _same(graphed, eager), errs
    assert all(torch.isfinite(v.float()).all() for v in graphed) and not torch.equal(graphed[1], x0)
    m = half_mask(8, 128, 256)
    k = kept(m, 16, 32).expand(1, 4, -1, -1, -1).cuda()
    assert k.any() and not k.all()
    gm, em = gpu_run(_dpm(), True, regenerate_mask=m, **kw), gpu_run(_dpm(), False, regenerate_mask=m, **kw)
    errs = dict(pano=rel(gm[1], em[1]), pers=rel(gm[2], em[2]))
    _record("multistep_graphed_vs_eager_keep_mask", **errs)
    assert _same(gm, em), errs
    assert same_bits(gm[1][k], x0[k]) and not torch.equal(gm[1][~k], x0[~k]) and not torch.equal(gm[1], graphed[1])


def test_order_one_is_the_ddim_pipeline_and_order_two_is_not(gpu_run, init_clip):
    """solver_order = 1 against the DDIM pipeline on the latents after 1 step of the 4-step schedule (eager, ``trace``): the same
    update in exact arithmetic, two kernels' roundings apart.  solver_order = 2 after 4 steps differs from the DDIM pipeline (and from
    order 1) by more than 1e-3: the history is used."""
    tr_ddim, tr_one = [], []
    ddim = gpu_run(DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), False, trace=tr_ddim)
    one = gpu_run(_dpm(solver_order=1), False, trace=tr_one)
    e1 = rel(tr_one[0], tr_ddim[0])
    e4, e4_one = rel(init_clip[1], ddim[1]), rel(init_clip[1], one[1])
    print(f"order 1 vs DDIM after 1 step: {e1:.3g}; order 2 after 4 steps vs DDIM: {e4:.3g}, vs order 1: {e4_one:.3g}")
    _record("multistep_order1_vs_ddim", after_1_step=e1, order2_vs_ddim_after_4=e4, order2_vs_order1_after_4=e4_one)
    assert len(tr_ddim) == len(tr_one) == 4
    assert e1 < TOL[torch.bfloat16], e1
    assert e4 > 1e-3 and e4_one > 1e-3, (e4, e4_one)
