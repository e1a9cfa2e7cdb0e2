"""Adaptive projected guidance (APG, arXiv 2410.02416) on the MI355X: the scalars of the two-launch scheme (cfg_apg_stats_kernel ->
per-workgroup merge) against fp64, the four APG step kernels (plain and windows, DDIM and multistep) against the fp64 definition
``scheduler.projected_guidance`` for every mode, their bit-level guarantees (device coefficients, run-to-run, apg=None, one uniform
window), guarded buffers, the argument checks, and the pipeline keywords: captured steps against eager ones and one eager step against
the chain written out on the kernels."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from _guarded import Guarded, _SENTINEL  # noqa: E402
from helpers import record as _record, rel  # noqa: E402
from imagine360_amd import configs, kernels as K, synthetic as S  # noqa: E402
from imagine360_amd.context import context_weights  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, projected_guidance  # noqa: E402
from test_context_windows import pipe_kw, windows_case  # noqa: E402
from test_context_windows_gpu import KERNEL_CASES  # noqa: E402
from test_ddim_stochastic_gpu import TOL, _host_step  # noqa: E402
from test_guidance_rescale_gpu import FACTOR_TOL  # noqa: E402
from test_multistep_sampler_gpu import HIST_TOL, _coefs as _multistep_coefs, _hist, _host_multistep  # noqa: E402

torch.set_grad_enabled(False)
G = 7.5
SHAPE = (1, 4, 5, 7, 24)          # 3360 elements: 420 lanes of 8, not a multiple of the 256-thread block; 2 records
LARGE = 256 * 256 * 4 + 300       # lanes: 256 records, every workgroup of the capped statistics grid loops four or five times
PRED = {0: "epsilon", 1: "v_prediction", 2: "sample"}
# HIST_TOL (1e-5, test_multistep_sampler_gpu.py: x0 from 16-bit inputs in about ten fp32 operations of 2^-24 each) also covers the
# history of an APG step: on top of those roundings alpha's error, bounded by FACTOR_TOL (|d| / |q|), moves m by at most
# (g - 1) FACTOR_TOL |d|, i.e. 2e-6 of |m|.


def _sched():
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    return sch, sch._timesteps_host[8]


def _kp(pred, sa, sb):
    return (sb / sa, sb, 1.0)[pred]


def _rho(pred, sa, sb):
    return (-1.0 / sb, -sa / sb, 0.0)[pred]


def _scalars64(u, c, x, pred, g, sa, sb, eta, r):
    """fp64 (alpha, s, lambda, |d| / |q|, cos(d, q), kp rms(d))."""
    u, c, x = u.double(), c.double(), x.double()
    d, q = c - u, c + _rho(pred, sa, sb) * x
    alpha = float((d * q).sum() / (q * q).sum())
    rms = _kp(pred, sa, sb) * float((d * d).mean().sqrt())
    s = 1.0 if r is None else min(1.0, r / rms)
    return alpha, s, (g - 1.0) * s * (1.0 - eta) * alpha, float(d.norm() / q.norm()), float((d * q).sum() / (d.norm() * q.norm())), rms


def _m64(u, c, x, mode, coefs, apg):
    return projected_guidance(u.double(), c.double(), x.double(), coefs[0], coefs[1], coefs[2], PRED[mode & 3], apg[0], apg[1])


def _threshold(u, c, pred, sa, sb, share=0.5):
    """An active clamp: ``share`` of the RMS the guidance difference has in x0 units (fp64), so s = share."""
    return share * _kp(pred, sa, sb) * float((c.double() - u.double()).pow(2).mean().sqrt())


def _name(dt):
    return str(dt).split(".")[-1]


# ------------------------------------------------------------------------------------------------ 1. the scalars
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mean,std", [(0.0, 0.25), (3.0, 0.1)])
@pytest.mark.parametrize("lanes", [420, LARGE], ids=["small", "large"])
def test_cfg_apg_scalars_vs_fp64(dt, mean, std, lanes):
    """iid u, c ~ N(mean, std^2), x ~ N(0, 1).  Epsilon and v-prediction: there |cos(d, q)| lies in [0.02, 0.7] and alpha is well
    conditioned (asserted); for prediction type `sample` q = c and iid draws give cos = 1 / sqrt(2), just outside -- that type is
    covered by the step tests.  Errors: |alpha - alpha64| / (|d| / |q|) and |s / s64 - 1| with the clamp active."""
    sch, t = _sched()
    shape = SHAPE if lanes == 420 else (lanes * 8,)
    assert K.lib().im360_cfg_rescale_records(lanes * 8) == (2 if lanes == 420 else 256)
    gen = torch.Generator().manual_seed(91)
    u, c = ((torch.randn(shape, generator=gen) * std + mean).to(dt) for _ in range(2))
    x = torch.randn(shape, generator=gen).to(dt)
    du, dc, dx = u.cuda(), c.cuda(), x.cuda()
    coefs = sch.step_coefficients(t, 0.0, G)
    _, sa, sb = coefs[:3]
    coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
    for pred in (0, 1):
        r = _threshold(u, c, pred, sa, sb)
        alpha, s, lam, dq, cos, _ = _scalars64(u, c, x, pred, G, sa, sb, 0.25, r)
        assert 0.02 <= abs(cos) <= 0.7, (pred, cos)
        got = K.cfg_apg_scalars(du, dc, dx, pred, coefs, (0.25, r))
        assert got.dtype == torch.float32 and got.shape == (3,) and got.is_cuda
        ga, gs, gl = (float(v) for v in got)
        e_a, e_s = abs(ga - alpha) / dq, abs(gs / s - 1.0)
        e_l = abs(gl / ((G - 1.0) * gs * 0.75 * ga) - 1.0)          # lambda from the kernel's own alpha and s: three fp32 products
        print(f"cfg_apg_scalars {dt} N({mean}, {std}^2) {lanes} lanes pred {pred}: alpha {ga:.9g} (fp64 {alpha:.12g}) err {e_a:.3g}; "
              f"s {gs:.9g} (fp64 {s:.12g}) err {e_s:.3g}; lambda {gl:.9g} (fp64 {lam:.12g}) against its factors {e_l:.3g}; cos {cos:.3g}")
        _record(f"cfg_apg_scalars_{_name(dt)}_mean{mean}_{lanes}_pred{pred}", alpha_err=e_a, s_err=e_s, lambda_err=e_l, cos=cos)
        assert e_a <= FACTOR_TOL and e_s <= FACTOR_TOL, (e_a, e_s)
        assert e_l <= 4 * 2.0 ** -24, e_l          # (g - 1 and 1 - eta = 0.75 are exact; each product rounds by at most 2^-24)
        assert abs(s - 0.5) < 1e-12
        # the guidance (and sqrt_a, sqrt_b) read from coef_dev give the same bits as the scalars; twice the same bits
        assert torch.equal(K.cfg_apg_scalars(du, dc, dx, pred, (0.0,) * 6, (0.25, r), coef_dev=coef_dev), got)
        assert torch.equal(K.cfg_apg_scalars(du, dc, dx, pred, coefs, (0.25, r)), got)
        free = K.cfg_apg_scalars(du, dc, dx, pred, coefs, (0.25, None))
        assert float(free[1]) == 1.0 and float(free[0]) == ga              # no clamp: s = 1 exactly, the same alpha


# ------------------------------------------------------------------------------------------------ 2. the step kernels
def _inputs(dt, seed=52, shape=SHAPE):
    gen = torch.Generator().manual_seed(seed)
    u, c, x, z = (torch.randn(shape, generator=gen).to(dt) for _ in range(4))
    return u * 0.25, c * 0.25, x, z          # a guided x0 partly inside, partly outside [-1, 1]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_apg_ddim_step_kernel_all_modes(dt):
    sch, t = _sched()
    u, c, x, z = _inputs(dt)
    dev = [v.cuda() for v in (u, c, x, z)]
    errs = {}
    for eta in (0.0, 0.8):
        coefs = sch.step_coefficients(t, eta, G)
        coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
        noise = dev[3] if eta > 0 else None
        for pred in (0, 1, 2):
            thr = _threshold(u, c, pred, coefs[1], coefs[2])
            for extra in (0, 4, 8, 12):
                mode = pred | extra
                plain = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs)
                assert torch.equal(K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs, apg=None), plain), (eta, mode)
                for apg in ((0.0, None), (0.5, None), (0.0, thr), (0.5, thr)):
                    m = _m64(u, c, x, mode, coefs, apg)
                    ref = _host_step(m, m, x, z if eta > 0 else None, mode, coefs)          # (guidance on u = c = m is exact)
                    out = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs, apg=apg)
                    assert out.dtype == dt and out.shape == SHAPE
                    errs[f"eta{eta}_mode{mode}_apg{apg[0]}_{apg[1] is not None}"] = e = rel(out, ref)
                    assert e < TOL[dt], (eta, mode, apg, e)
                    out2 = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, (0.0,) * 6, coef_dev=coef_dev, apg=apg)
                    assert torch.equal(out2, out), (eta, mode, apg)
                    assert torch.equal(K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs, apg=apg), out), (eta, mode, apg)
                    if not (extra & 4):          # (a clamp of x0 to [-1, 1] hides a part of any change of m)
                        assert rel(out, plain.float().cpu()) > 1e-2, (eta, mode, apg)          # the scalars are used
    print(f"cfg_ddim_step apg {dt}: max rel {max(errs.values()):.3g}")
    _record(f"cfg_ddim_step_apg_{_name(dt)}", max_rel=max(errs.values()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_apg_multistep_step_kernel_all_modes(dt):
    u, c, x, _ = _inputs(dt)
    h = _hist(SHAPE)
    du, dc, dx = u.cuda(), c.cuda(), x.cuda()
    errs, herrs = {}, {}
    for order, coefs in enumerate(_multistep_coefs(), 1):
        coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
        for mode in (0, 1, 2, 4, 5, 6):
            thr = _threshold(u, c, mode & 3, coefs[1], coefs[2])
            dh0, dh1 = h.cuda(), h.cuda()
            plain = K.cfg_multistep_step(du, dc, dx, dh0, mode, coefs)
            assert torch.equal(K.cfg_multistep_step(du, dc, dx, dh1, mode, coefs, apg=None), plain) and torch.equal(dh0, dh1)
            for apg in ((0.0, None), (0.5, thr)):
                ref, x0 = _host_multistep(_m64(u, c, x, mode, coefs, apg), x, h, mode, coefs)
                dh = h.cuda()
                out = K.cfg_multistep_step(du, dc, dx, dh, mode, coefs, apg=apg)
                assert out.dtype == dt and out.shape == SHAPE and dh.dtype == torch.float32
                key = f"order{order}_mode{mode}_apg{apg[0]}"
                errs[key], herrs[key] = e, eh = rel(out, ref), rel(dh, x0)
                assert e < TOL[dt] and eh < HIST_TOL, (key, e, eh)
                dh2 = h.cuda()
                out2 = K.cfg_multistep_step(du, dc, dx, dh2, mode, (0.0,) * 6, coef_dev=coef_dev, apg=apg)
                assert torch.equal(out2, out) and torch.equal(dh2, dh), key
                if not (mode & 4):
                    assert rel(out, plain.float().cpu()) > 1e-2, key
    print(f"cfg_multistep_step apg {dt}: max rel out {max(errs.values()):.3g} hist {max(herrs.values()):.3g}")
    _record(f"cfg_multistep_step_apg_{_name(dt)}", max_rel=max(errs.values()), max_hist_rel=max(herrs.values()))
    with pytest.raises(ValueError, match="mode bit 8"):
        K.cfg_multistep_step(du, dc, dx, h.cuda(), 1 | 8, coefs, apg=(0.0, None))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_apg_grid_stride_and_all_records(dt):
    """The large size: every workgroup of the capped 256-workgroup statistics grid loops four or five times, the step's workgroups
    merge all 256 records and stride over the tensor; finite, within TOL, twice the same bits."""
    sch, t = _sched()
    n = LARGE * 8
    gen = torch.Generator().manual_seed(53)
    u, c, x, z = (torch.randn(n, generator=gen).to(dt) for _ in range(4))
    u, c = u * 0.25, c * 0.25
    dev = [v.cuda() for v in (u, c, x, z)]
    coefs = sch.step_coefficients(t, 1.0, G)
    apg = (0.0, _threshold(u, c, 1, coefs[1], coefs[2]))
    out = K.cfg_ddim_step(*dev, 1 | 4, coefs, apg=apg)
    m = _m64(u, c, x, 1, coefs, apg)
    e = rel(out, _host_step(m, m, x, z, 1 | 4, coefs))
    print(f"apg grid stride {dt}: step rel err {e:.3g}")
    _record(f"cfg_ddim_step_apg_grid_stride_{_name(dt)}", step_rel=e)
    assert torch.isfinite(out.float()).all() and e < TOL[dt], e
    assert torch.equal(K.cfg_ddim_step(*dev, 1 | 4, coefs, apg=apg), out)


# ------------------------------------------------------------------------------------------------ 3. windows
def _blend_uc64(preds, x, starts, w, ring):
    """fp64 per-frame blends of u_k and of c_k over the covering windows; frames (start + j) mod F on a ring."""
    fd = x.dim() - 3
    Fr, L = x.shape[fd], preds.shape[fd + 1]
    shape = [1] * x.dim()
    shape[fd] = L
    wv = w.double().reshape(shape)
    ub, cb, ws = (torch.zeros(x.shape, dtype=torch.float64) for _ in range(3))
    for k, s in enumerate(starts):
        idx = (s + torch.arange(L)) % Fr
        assert ring or s + L <= Fr
        u, c = preds[k, 0:1].double(), preds[k, 1:2].double()
        ub.index_add_(fd, idx, wv * u)
        cb.index_add_(fd, idx, wv * c)
        ws.index_add_(fd, idx, wv.expand_as(u).contiguous())
    return ub / ws, cb / ws


def _window_cases():
    """KERNEL_CASES of test_context_windows_gpu.py on a line (16-byte lanes, and inner 35 / 15: the scalar-lane instantiation), and
    those with more than one window again on a ring, their starts rolled by 3 frames so that windows cross the end of the clip."""
    for ci, (shape, L, starts) in enumerate(KERNEL_CASES):
        yield ci, shape, L, starts, starts, False
        if len(starts) > 1:
            F = shape[len(shape) - 3]
            yield ci, shape, L, starts, [(s + F - 3) % F for s in starts], True


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_apg_windows_kernels_vs_fp64(dt):
    """Both windowed forms against fp64 blends of the two halves, then the definition, then the step: the DDIM form for every mode
    and eta in {0, 0.8}, the multistep form first and second order with its history."""
    sch, t = _sched()
    errs, herrs, serrs = {}, {}, {}
    for ci, shape, L, starts, st_host, ring in _window_cases():
        preds, x, z = windows_case(shape, L, starts, dt, seed=170 + ci)
        dp, dx, dz = preds.cuda(), x.cuda(), z.cuda()
        st = torch.tensor(st_host, dtype=torch.int32, device="cuda")
        w = context_weights(L, "pyramid")
        dw = w.cuda()
        ub, cb = _blend_uc64(preds, x, st_host, w, ring)
        for eta in (0.0, 0.8):
            coefs = sch.step_coefficients(t, eta, G)
            coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
            noise, dnoise = (z, dz) if eta > 0 else (None, None)
            for pred in (0, 1, 2):
                apg = (0.5, _threshold(ub, cb, pred, coefs[1], coefs[2])) if pred == 1 else (0.0, None)
                m = _m64(ub, cb, x, pred, coefs, apg)
                if eta == 0.0:
                    alpha, s, lam, dq, _, _ = _scalars64(ub, cb, x, pred, G, coefs[1], coefs[2], *apg)
                    got = K.cfg_apg_scalars_windows(dp, dx, st, dw, pred, coefs, apg, ring=ring)
                    serrs[f"case{ci}_ring{int(ring)}_pred{pred}"] = max(abs(float(got[0]) - alpha) / dq, abs(float(got[1]) / s - 1.0))
                for extra in (0, 4, 8, 12):
                    mode = pred | extra
                    ref = _host_step(m, m, x, noise, mode, coefs)
                    out = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs, ring=ring, apg=apg)
                    assert out.dtype == dt and out.shape == x.shape
                    errs[f"case{ci}_ring{int(ring)}_eta{eta}_mode{mode}"] = e = rel(out, ref)
                    assert e < TOL[dt], (ci, ring, eta, mode, e)
                    out2 = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, (0.0,) * 6, coef_dev=coef_dev, ring=ring, apg=apg)
                    assert torch.equal(out2, out), (ci, ring, eta, mode)
        plain = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs, ring=ring)
        assert torch.equal(K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs, ring=ring, apg=None), plain)
        h = _hist(shape, seed=9 + ci)
        for order, coefs in enumerate(_multistep_coefs(), 1):
            for mode in (0, 1, 2, 5):
                apg = (0.0, _threshold(ub, cb, mode & 3, coefs[1], coefs[2])) if mode == 1 else (0.5, None)
                ref, x0 = _host_multistep(_m64(ub, cb, x, mode, coefs, apg), x, h, mode, coefs)
                dh = h.cuda()
                out = K.cfg_multistep_step_windows(dp, dx, dh, st, dw, mode, coefs, ring=ring, apg=apg)
                key = f"case{ci}_ring{int(ring)}_order{order}_mode{mode}"
                errs[key], herrs[key] = e, eh = rel(out, ref), rel(dh, x0)
                assert e < TOL[dt] and eh < HIST_TOL, (key, e, eh)
    print(f"apg windows {dt}: max rel out {max(errs.values()):.3g} hist {max(herrs.values()):.3g} scalars {max(serrs.values()):.3g}")
    _record(f"cfg_step_windows_apg_{_name(dt)}", max_rel=max(errs.values()), max_hist_rel=max(herrs.values()), max_scalar_err=max(serrs.values()))
    assert max(serrs.values()) <= FACTOR_TOL, serrs


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_one_uniform_window_is_the_plain_apg_step_bit_for_bit(dt):
    sch, t = _sched()
    # panorama / perspective on 16-byte lanes; inner 15: the scalar path, 480 elements in whole groups of 8; inner 35 (1120 elements)
    for shape in ((1, 4, 5, 7, 24), (1, 3, 4, 5, 4, 8), (1, 4, 8, 3, 5), (1, 4, 8, 5, 7)):
        L = shape[-3]
        preds, x, z = windows_case(shape, L, [0], dt, seed=81)
        preds[0, 0].view(-1)[:64] = 0.0
        preds[0, 1].view(-1)[:64] = 0.0
        preds[0, 1].view(-1)[:32] = -0.0
        dp, dx, dz = preds.cuda(), x.cuda(), z.cuda()
        du, dc = dp[0, 0:1].contiguous(), dp[0, 1:2].contiguous()
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        w = context_weights(L, "uniform").cuda()
        h = _hist(shape)
        for ring in (False, True):
            for apg in ((0.0, None), (0.5, 0.05)):
                for eta in (0.0, 0.8):
                    coefs = sch.step_coefficients(t, eta, G)
                    noise = dz if eta > 0 else None
                    for mode in (0, 1, 2, 1 | 4, 0 | 8, 1 | 12):
                        a = K.cfg_ddim_step_windows(dp, dx, noise, st, w, mode, coefs, ring=ring, apg=apg)
                        b = K.cfg_ddim_step(du, dc, dx, noise, mode, coefs, apg=apg)
                        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (shape, ring, apg, eta, mode)
                    sa = K.cfg_apg_scalars_windows(dp, dx, st, w, 1, coefs, apg, ring=ring)
                    assert torch.equal(sa.view(torch.int32), K.cfg_apg_scalars(du, dc, dx, 1, coefs, apg).view(torch.int32))
                for coefs in _multistep_coefs():
                    for mode in (0, 1, 2, 5):
                        ha, hb = h.cuda(), h.cuda()
                        a = K.cfg_multistep_step_windows(dp, dx, ha, st, w, mode, coefs, ring=ring, apg=apg)
                        b = K.cfg_multistep_step(du, dc, dx, hb, mode, coefs, apg=apg)
                        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (shape, ring, apg, coefs[5], mode)
                        assert torch.equal(ha.view(torch.int32), hb.view(torch.int32)), (shape, ring, apg, coefs[5], mode)


# ------------------------------------------------------------------------------------------------ 4. guarded buffers
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_apg_steps_and_workspace_between_guard_bands(dt):
    """One plain and one windows APG step (16-byte lanes and the scalar path) with every tensor between poisoned guards: no store
    outside, every result written whole.  Then the statistics pass into a workspace with room for four records more than it needs:
    records(n) records of four floats are written, nothing behind them."""
    sch, t = _sched()
    coefs = sch.step_coefficients(t, 0.8, G)
    u, c, x, z = _inputs(dt, seed=31)
    apg = (0.0, _threshold(u, c, 1, coefs[1], coefs[2]))
    m = _m64(u, c, x, 1, coefs, apg)
    g = Guarded(K)
    du, dc, dx, dz = (g.guard(v.cuda()) for v in (u, c, x, z))
    with g:
        out = g.out(K.cfg_ddim_step(du, dc, dx, dz, 1 | 4, coefs, apg=apg))
    assert rel(out, _host_step(m, m, x, z, 1 | 4, coefs)) < TOL[dt]
    first, second = _multistep_coefs()
    for shape, L, starts in (KERNEL_CASES[0], KERNEL_CASES[2]):
        preds, xs, zs = windows_case(shape, L, starts, dt, seed=33)
        w = context_weights(L, "pyramid")
        ub, cb = _blend_uc64(preds, xs, starts, w, False)
        mw = _m64(ub, cb, xs, 1, coefs, (0.5, None))
        h = _hist(shape)
        g = Guarded(K)
        dp, dxs, dzs, ds, dw = (g.guard(v.cuda()) for v in (preds, xs, zs, torch.tensor(starts, dtype=torch.int32), w))
        dh = g.guard(h.cuda())
        with g:
            out = g.out(K.cfg_ddim_step_windows(dp, dxs, dzs, ds, dw, 1 | 4, coefs, apg=(0.5, None)))
            out_m = g.out(K.cfg_multistep_step_windows(dp, dxs, dh, ds, dw, 1, second, apg=(0.5, None)))
            g.out(dh)
        assert rel(out, _host_step(mw, mw, xs, zs, 1 | 4, coefs)) < TOL[dt]
        ref, x0 = _host_multistep(_m64(ub, cb, xs, 1, second, (0.5, None)), xs, h, 1, second)
        assert rel(out_m, ref) < TOL[dt] and rel(dh, x0) < HIST_TOL
    # the workspace: records(n) = 2 for SHAPE
    recs = K.lib().im360_cfg_rescale_records(x.numel())
    assert recs == 2
    g = Guarded(K)
    du, dc, dx = (g.guard(v.cuda()) for v in (u, c, x))
    ws = g.empty(((recs + 4) * K.RESCALE_RECORD,), torch.float32, "cuda")
    rc = K.lib().im360_cfg_apg_stats(du.data_ptr(), dc.data_ptr(), dx.data_ptr(), x.numel(), coefs[1], coefs[2], 1, ws.data_ptr(), ws.numel(),
                                     K._dt(du), None, None)
    assert rc == 0, K.lib().im360_last_error()
    g.check()
    poisoned = (ws.view(torch.int32) == _SENTINEL[4]).cpu().view(recs + 4, K.RESCALE_RECORD)
    assert not poisoned[:recs, :4].any() and poisoned[recs:].all(), poisoned
    assert float(ws[0] + ws[K.RESCALE_RECORD]) == x.numel()          # the records' counts add up to n


# ------------------------------------------------------------------------------------------------ 5. the argument checks
def test_apg_entry_points_reject_bad_arguments():
    """Host-side checks only: nothing is launched."""
    a = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    hist = torch.zeros(16, dtype=torch.float32, device="cuda")
    coefs = (7.5, 0.5, 0.8, 0.6, 0.7, 0.0)
    with pytest.raises(ValueError, match="cannot be combined"):
        K.cfg_ddim_step(a, a, a, None, 1, coefs, rescale=0.7, apg=(0.0, None))
    with pytest.raises(ValueError, match="eta"):
        K.cfg_ddim_step(a, a, a, None, 1, coefs, apg=(float("nan"), None))
    with pytest.raises(ValueError, match="threshold"):
        K.cfg_multistep_step(a, a, a, hist, 1, coefs, apg=(0.0, 0.0))
    lib, p, hp = K.lib(), a.data_ptr(), hist.data_ptr()
    ws = torch.zeros(K.RESCALE_RECORD, dtype=torch.float32, device="cuda")
    out3 = torch.zeros(3, dtype=torch.float32, device="cuda")
    wp = ws.data_ptr()
    inf = float("inf")
    big = 256 * 8 * 3                        # three records needed

    def ddim(eta=0.0, thr=1.0, ws_ptr=wp, floats=8, n=16, mode=1, u=p, out=p):
        return lib.im360_cfg_ddim_step_apg(u, p, p, None, out, n, *coefs, mode, eta, thr, ws_ptr, floats, 0, None, None)

    def multi(eta=0.0, thr=1.0, ws_ptr=wp, floats=8, n=16, mode=1, h=hp):
        return lib.im360_cfg_multistep_step_apg(p, p, p, h, p, n, *coefs, mode, eta, thr, ws_ptr, floats, 0, None, None)

    def stats(ws_ptr=wp, floats=8, n=16, mode=1, u=p):
        return lib.im360_cfg_apg_stats(u, p, p, n, 0.5, 0.8, mode, ws_ptr, floats, 0, None, None)

    def scal(eta=0.0, thr=1.0, ws_ptr=wp, floats=8, n=16, out=out3.data_ptr()):
        return lib.im360_cfg_apg_scalars(ws_ptr, floats, n, 7.5, 0.5, 0.8, 1, eta, thr, out, None, None)

    for fn in (ddim, multi, scal):
        for eta in (float("nan"), inf, -inf):
            assert fn(eta=eta) != 0 and b"eta" in lib.im360_last_error() and b"must be finite" in lib.im360_last_error()
        for thr in (0.0, -1.0, float("nan"), -inf):
            assert fn(thr=thr) != 0 and b"must be > 0" in lib.im360_last_error(), thr
    for fn in (ddim, multi, stats, scal):
        assert fn(ws_ptr=None) != 0 and b"null or misaligned workspace" in lib.im360_last_error()
        assert fn(ws_ptr=wp + 2) != 0 and b"null or misaligned workspace" in lib.im360_last_error()
        assert fn(n=big) != 0 and b"workspace of 8 floats, 24 needed" in lib.im360_last_error()
    for fn in (ddim, stats):
        assert fn(u=None) != 0 and b"null pointer" in lib.im360_last_error()
        assert fn(u=p + 2) != 0 and b"misaligned pointer" in lib.im360_last_error()
        assert fn(n=12) != 0 and b"multiple of 8" in lib.im360_last_error()
        assert fn(mode=3) != 0 and b"mode 3 unsupported" in lib.im360_last_error()
    assert ddim(out=None) != 0 and b"null pointer" in lib.im360_last_error()
    assert multi(h=None) != 0 and b"null pointer" in lib.im360_last_error()
    assert multi(mode=1 | 8) != 0 and b"bit 8 (use_clipped_model_output) unsupported" in lib.im360_last_error()
    assert scal(out=None) != 0 and b"null or misaligned output" in lib.im360_last_error()
    # windows: the shape / table checks of the siblings, wrap, then the APG arguments
    x = torch.zeros(1, 4, 4, 2, 8, dtype=torch.bfloat16, device="cuda")
    pr = torch.zeros(2, 2, 4, 2, 2, 8, dtype=torch.bfloat16, device="cuda")
    hx = torch.zeros(x.shape, dtype=torch.float32, device="cuda")
    st, w = torch.tensor([0, 2], dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    q, geo = x.data_ptr(), (2, 4, 4, 2, 16)

    def wddim(eta=0.0, thr=1.0, ws_ptr=wp, wrap=0, mode=1, geo=geo, pred=pr.data_ptr()):
        return lib.im360_cfg_ddim_step_windows_apg(pred, q, None, q, st.data_ptr(), w.data_ptr(), *geo, wrap, *coefs, mode, eta, thr, ws_ptr, 8, 0,
                                                   None, None)

    def wmulti(eta=0.0, thr=1.0, ws_ptr=wp, wrap=0, mode=1, geo=geo, pred=pr.data_ptr()):
        return lib.im360_cfg_multistep_step_windows_apg(pred, q, hx.data_ptr(), q, st.data_ptr(), w.data_ptr(), *geo, wrap, *coefs, mode, eta, thr,
                                                        ws_ptr, 8, 0, None, None)

    def wstats(ring=False, ws_ptr=wp, mode=1, geo=geo, pred=pr.data_ptr()):
        fn = lib.im360_cfg_apg_stats_windows_ring if ring else lib.im360_cfg_apg_stats_windows
        return fn(pred, q, st.data_ptr(), w.data_ptr(), *geo, 0.5, 0.8, mode, ws_ptr, 8, 0, None, None)

    for fn in (wddim, wmulti):
        assert fn(eta=inf) != 0 and b"must be finite" in lib.im360_last_error()
        assert fn(thr=0.0) != 0 and b"must be > 0" in lib.im360_last_error()
        assert fn(wrap=3) != 0 and b"wrap=3 must be 0 (line) or F=4 (ring)" in lib.im360_last_error()
        assert fn(ws_ptr=None) != 0 and b"null or misaligned workspace" in lib.im360_last_error()
        assert fn(pred=None) != 0 and b"null pointer" in lib.im360_last_error()
        assert fn(geo=(2, 4, 4, 5, 16)) != 0 and b"out of range" in lib.im360_last_error()              # L > F
        assert fn(geo=(2, 4 * 256, 4, 2, 16)) != 0 and b"workspace of 8 floats" in lib.im360_last_error()
        assert fn(mode=3) != 0 and b"mode 3 unsupported" in lib.im360_last_error()
    assert wmulti(mode=1 | 8) != 0 and b"bit 8" in lib.im360_last_error()
    for ring in (False, True):
        assert wstats(ring, ws_ptr=None) != 0 and b"null or misaligned workspace" in lib.im360_last_error()
        assert wstats(ring, pred=None) != 0 and b"null pointer" in lib.im360_last_error()
        assert wstats(ring, geo=(2, 4, 4, 5, 16)) != 0 and b"out of range" in lib.im360_last_error()
        assert wstats(ring, mode=3) != 0 and b"mode 3 unsupported" in lib.im360_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. the pipeline
@pytest.fixture(scope="module")
def gpu_run():
    """The w/5 synthetic pipeline in bf16 on the real kernels: run(use_graph, frames, steps, **keywords) -> (video, panorama latent,
    perspective latent)."""
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
    pipe._no_progress = True
    data = {}

    def run(use_graph, frames=8, steps=3, seed=33, **kw):
        if frames not in data:
            data[frames] = S.video_batch(frames=frames, pano_hw=(128, 256), seed=12), S.conditioning(frames=max(frames, 16), seed=12)
        vb, cond = data[frames]
        pipe.use_graph = use_graph
        torch.manual_seed(seed)
        random.seed(seed)
        args = pipe_kw(cond, vb, latents_dtype=dt, **kw)
        args["num_inference_steps"] = steps
        vid = pipe("synthetic", **args).videos
        torch.cuda.synchronize()
        return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone()
    run.pipe = pipe
    return run


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


APG = dict(apg_eta=0.0, apg_threshold=0.5)
WINDOWS = dict(frames=24, context_frames=16, context_overlap=8)


def _graphed_vs_eager(gpu_run, monkeypatch, name, windows, expect, **kw):
    """Both runs; the graphed one must have replayed captured steps whose ``apg`` is ``expect``."""
    from imagine360_amd import graph_step
    cls = graph_step.GraphedWindowedStep if windows else graph_step.GraphedDenoiseStep
    replays = []
    orig = cls.step
    monkeypatch.setattr(cls, "step", lambda self, t: (replays.append(self.apg), orig(self, t))[1])
    out = {}
    for graph in (True, False):
        gen = dict(generator=torch.Generator(device="cuda").manual_seed(77)) if kw.get("eta", 0.0) > 0 else {}
        out[graph] = gpu_run(graph, **(WINDOWS if windows else {}), **kw, **gen)
    assert replays == [expect] * 3, replays
    errs = dict(pano=rel(out[True][1], out[False][1]), pers=rel(out[True][2], out[False][2]))
    _record(f"graphed_vs_eager_apg_{name}", **errs)
    assert _same(out[True], out[False]), errs
    assert all(torch.isfinite(v.float()).all() for v in out[True])
    return out[True]


@pytest.mark.parametrize("windows", [False, True], ids=["plain", "windows"])
@pytest.mark.parametrize("eta", [0.0, 0.8])
def test_graphed_apg_steps_equal_eager_bit_for_bit(gpu_run, windows, eta, monkeypatch):
    """apg_eta = 0 with a clamp, 3 steps: both launches of each branch are captured and replay the eager loop's numbers, for eta = 0
    and for eta = 0.8 with a seeded device generator."""
    kw = dict(eta=eta) if eta > 0 else {}
    on = _graphed_vs_eager(gpu_run, monkeypatch, f"{'windows' if windows else 'plain'}_eta{eta}", windows, (0.0, 0.5), **APG, **kw)
    if eta == 0.0:
        ctx = WINDOWS if windows else {}
        off = gpu_run(True, **ctx)
        assert _same(off, gpu_run(True, apg_eta=None, apg_threshold=None, **ctx))          # None: the call without the keywords
        assert rel(on[1], off[1]) > 1e-2                                                   # and APG is another clip


def test_graphed_apg_steps_equal_eager_with_dpm_solver(gpu_run, monkeypatch):
    pipe = gpu_run.pipe
    saved = pipe.scheduler
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(saved.config)
    try:
        _graphed_vs_eager(gpu_run, monkeypatch, "dpm_solver_2m", False, (0.0, 0.5), **APG)
    finally:
        pipe.scheduler = saved


def test_graphed_apg_steps_equal_eager_under_a_guidance_interval(gpu_run, monkeypatch):
    """3 steps at t = 667, 334, 1 under (0.2, 0.6): only the middle one is guided -- two captured graphs, the APG launches in one."""
    _graphed_vs_eager(gpu_run, monkeypatch, "guidance_interval", False, (0.0, 0.5), guidance_interval=(0.2, 0.6), **APG)


def test_eager_apg_step_equals_the_chain_written_out_on_the_kernels(gpu_run):
    """One eager step with APG against the chain written out per branch: ``projected_guidance`` in fp32, rounded to the latent dtype,
    then K.cfg_ddim_step with guidance 1.  The chain rounds m to 16 bits once more than the kernel does: inside TOL."""
    pipe = gpu_run.pipe
    got = gpu_run(False, steps=1, **APG)
    sch = pipe.scheduler

    def step(u, c, g, t, x, coef_dev=None, **kw):
        assert kw.pop("guidance_apg") == (0.0, 0.5)
        _, sa, sb = sch.step_coefficients(t, 0.0, g)[:3]
        m = projected_guidance(u.float(), c.float(), x.float(), g, sa, sb, sch.config.prediction_type, 0.0, 0.5).to(x.dtype).contiguous()
        return K.cfg_ddim_step(m, m, x.contiguous(), None, sch.kernel_mode(), sch.step_coefficients(t, 0.0, 1.0))
    sch.fused_cfg_step = step
    try:
        want = gpu_run(False, steps=1, **APG)
    finally:
        del sch.fused_cfg_step
    errs = dict(pano=rel(got[1], want[1]), pers=rel(got[2], want[2]))
    print(f"eager APG step vs the chain written out: {errs}")
    _record("apg_pipeline_vs_hand_loop", **errs)
    assert max(errs.values()) < TOL[torch.bfloat16], errs
