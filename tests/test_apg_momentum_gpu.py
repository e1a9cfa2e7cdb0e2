"""The momentum of adaptive projected guidance (arXiv 2410.02416, algorithm 1 in full) on the MI355X: the scalars of the momentum
statistics pass against fp64, the four momentum step kernels (plain and windows, DDIM and multistep) against the fp64 definition
``scheduler.projected_guidance(..., momentum=)`` for every mode with a per-element bound on the written state, their bit-level
guarantees (carry 0 with a NaN state, exact inputs, device carry, run-to-run, one uniform window, the statistics pass leaves the state
alone), guarded buffers, the argument checks, and the pipeline keyword ``apg_momentum``: captured steps against eager ones (plain,
windows, a guidance interval, FreeInit passes), one eager step against the chain written out on the wrappers, 0.0 against None."""
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
from test_ddim_stochastic_gpu import TOL, _host_step  # noqa: E402
from test_guidance_rescale_gpu import FACTOR_TOL  # noqa: E402
from test_multistep_sampler_gpu import HIST_TOL, _coefs as _multistep_coefs, _hist, _host_multistep  # noqa: E402
from test_projected_guidance_gpu import LARGE, PRED, SHAPE, _blend_uc64, _inputs, _kp, _name, _rho, _sched  # noqa: E402

torch.set_grad_enabled(False)
G = 7.5
CARRY = -0.5
# The smallest geometry of test_context_windows_gpu.KERNEL_CASES' kind: F = 5, L = 3, overlap 1 (two windows); inner 32 takes the
# 16-byte lanes (V = 8), inner 15 the scalar lanes (V = 1).  On a ring the starts are rolled so that a window crosses the end.
WINDOW_CASES = [((1, 4, 5, 4, 8), 3, [0, 2]), ((1, 4, 5, 3, 5), 3, [0, 2])]


def _f32(v):
    """``v`` as the float32 the entry points receive."""
    return float(torch.tensor(v, dtype=torch.float32))


def _state(shape, std, seed=7):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std


def _scalars64(u, c, x, prev, carry, pred, g, sa, sb, eta, r):
    """fp64 (alpha, s, lambda, |e| / |q|, cos(e, q)) with e = d + carry e_prev: the error measures of test_projected_guidance_gpu on e."""
    u, c, x = u.double(), c.double(), x.double()
    e, q = c - u + carry * prev.double(), c + _rho(pred, sa, sb) * x
    alpha = float((e * q).sum() / (q * q).sum())
    rms = _kp(pred, sa, sb) * float((e * e).mean().sqrt())
    s = 1.0 if r is None else min(1.0, r / rms)
    return alpha, s, (g - 1.0) * s * (1.0 - eta) * alpha, float(e.norm() / q.norm()), float((e * q).sum() / (e.norm() * q.norm())), rms


def _me64(u, c, x, prev, carry, mode, coefs, apg):
    return projected_guidance(u.double(), c.double(), x.double(), coefs[0], coefs[1], coefs[2], PRED[mode & 3], apg[0], apg[1],
                              momentum=(prev.double(), carry))


def _threshold(u, c, prev, carry, pred, sa, sb, share=0.5):
    """An active clamp: ``share`` of the RMS e has in x0 units (fp64), so s = share."""
    e = c.double() - u.double() + carry * prev.double()
    return share * _kp(pred, sa, sb) * float(e.pow(2).mean().sqrt())


def _state_excess(state, e64, u, c, prev, carry, blend=None):
    """max over the elements of |state - e64| / bound, bound = 2^-23 (|c| + |u| + |carry e_prev|): d = c - u and the fma round once
    each, by at most 2^-24 of values no larger than that sum.  ``blend`` (windows; = (K + 4) 2^-24 (sum w |u_k| + sum w |c_k|) / sum w
    per element): the fp32 blends of the K covering windows round K products, K - 1 additions and one division (reciprocal and product
    under fast-math) per half, each by at most 2^-24 of the blend of the absolute values."""
    bound = 2.0 ** -23 * (c.double().abs() + u.double().abs() + (carry * prev.double()).abs())
    if blend is not None:
        bound = bound + blend
    return float(((state.double().cpu() - e64).abs() / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ 4. the scalars
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mean,std", [(0.0, 0.25), (3.0, 0.1)])
@pytest.mark.parametrize("lanes", [420, LARGE], ids=["small", "large"])
def test_momentum_scalars_vs_fp64(dt, mean, std, lanes):
    """The inputs of test_cfg_apg_scalars_vs_fp64 with an iid state of the inputs' standard deviation (d has sqrt(2) of it) and carry
    -0.5: |cos(e, q)| stays in [0.02, 0.7] for epsilon and v-prediction (asserted; checked on the CPU for these seeds: 0.021 .. 0.48)."""
    sch, t = _sched()
    shape = SHAPE if lanes == 420 else (lanes * 8,)
    gen = torch.Generator().manual_seed(91)
    u, c = ((torch.randn(shape, generator=gen) * std + mean).to(dt) for _ in range(2))
    x = torch.randn(shape, generator=gen).to(dt)
    prev = _state(shape, std)
    du, dc, dx, dprev = u.cuda(), c.cuda(), x.cuda(), prev.cuda()
    coefs = sch.step_coefficients(t, 0.0, G)
    _, sa, sb = coefs[:3]
    coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
    carry_dev = torch.tensor([CARRY], dtype=torch.float32, device="cuda")
    for pred in (0, 1):
        r = _threshold(u, c, prev, CARRY, pred, sa, sb)
        alpha, s, lam, eq, cos, _ = _scalars64(u, c, x, prev, CARRY, pred, G, sa, sb, 0.25, r)
        assert 0.02 <= abs(cos) <= 0.7, (pred, cos)
        got = K.cfg_apg_scalars(du, dc, dx, pred, coefs, (0.25, r), apg_momentum=(dprev, CARRY))
        assert got.dtype == torch.float32 and got.shape == (3,) and got.is_cuda
        ga, gs, gl = (float(v) for v in got)
        e_a, e_s = abs(ga - alpha) / eq, abs(gs / s - 1.0)
        print(f"cfg_apg_scalars momentum {dt} N({mean}, {std}^2) {lanes} lanes pred {pred}: alpha {ga:.9g} (fp64 {alpha:.12g}) err {e_a:.3g}; "
              f"s {gs:.9g} (fp64 {s:.12g}) err {e_s:.3g}; cos {cos:.3g}")
        _record(f"cfg_apg_momentum_scalars_{_name(dt)}_mean{mean}_{lanes}_pred{pred}", alpha_err=e_a, s_err=e_s, cos=cos)
        assert e_a <= FACTOR_TOL and e_s <= FACTOR_TOL, (e_a, e_s)
        assert torch.equal(dprev.cpu(), prev)                                                   # (f) the pass leaves the state alone
        assert torch.equal(K.cfg_apg_scalars(du, dc, dx, pred, (0.0,) * 6, (0.25, r), coef_dev=coef_dev, apg_momentum=(dprev, 0.0),
                                             carry_dev=carry_dev), got)
        assert torch.equal(K.cfg_apg_scalars(du, dc, dx, pred, coefs, (0.25, r), apg_momentum=(dprev, CARRY)), got)
        # carry 0: the scalars without momentum, whatever the state holds
        nan = torch.full_like(dprev, float("nan"))
        assert torch.equal(K.cfg_apg_scalars(du, dc, dx, pred, coefs, (0.25, r), apg_momentum=(nan, 0.0)),
                           K.cfg_apg_scalars(du, dc, dx, pred, coefs, (0.25, r)))


# ------------------------------------------------------------------------------------------------ 5. the step kernels
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_momentum_ddim_step_kernel_all_modes(dt):
    sch, t = _sched()
    u, c, x, z = _inputs(dt)
    prev = _state(SHAPE, 0.35)
    dev = [v.cuda() for v in (u, c, x, z)]
    carry = sch.apg_carry(sch._timesteps_host[7], t, CARRY)             # the carry of a real pair of timesteps
    carry_dev = torch.tensor([carry], dtype=torch.float32, device="cuda")
    errs, serrs = {}, {}
    for eta in (0.0, 0.8):
        coefs = sch.step_coefficients(t, eta, G)
        coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
        noise = dev[3] if eta > 0 else None
        for pred in (0, 1, 2):
            thr = _threshold(u, c, prev, _f32(carry), pred, coefs[1], coefs[2])
            for extra in (0, 4, 8, 12):
                mode = pred | extra
                for apg in ((0.0, None), (0.5, thr)):
                    m, e64 = _me64(u, c, x, prev, _f32(carry), mode, coefs, apg)
                    ref = _host_step(m, m, x, z if eta > 0 else None, mode, coefs)
                    st = prev.cuda()
                    out = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs, apg=apg, apg_momentum=(st, carry))
                    assert out.dtype == dt and out.shape == SHAPE
                    key = f"eta{eta}_mode{mode}_apg{apg[0]}_{apg[1] is not None}"
                    errs[key], serrs[key] = e, es = rel(out, ref), _state_excess(st, e64, u, c, prev, _f32(carry))
                    assert e < TOL[dt] and es <= 1.0, (key, e, es)
                    st2 = prev.cuda()                                   # (c) the device carry and coefficients; (d) twice the same bits
                    out2 = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, (0.0,) * 6, coef_dev=coef_dev, apg=apg,
                                           apg_momentum=(st2, 0.0), carry_dev=carry_dev)
                    assert torch.equal(out2, out) and torch.equal(st2, st), key
                    st3 = prev.cuda()
                    assert torch.equal(K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs, apg=apg, apg_momentum=(st3, carry)), out)
                    assert torch.equal(st3, st), key
                    if not (extra & 4):                                 # the momentum is used: another result than without it
                        assert rel(out, K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs, apg=apg).float().cpu()) > 1e-2, key
    print(f"cfg_ddim_step apg momentum {dt}: max rel {max(errs.values()):.3g}, state error / bound {max(serrs.values()):.3g}")
    _record(f"cfg_ddim_step_apg_momentum_{_name(dt)}", max_rel=max(errs.values()), max_state_excess=max(serrs.values()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_momentum_multistep_step_kernel_all_modes(dt):
    u, c, x, _ = _inputs(dt)
    h = _hist(SHAPE)
    prev = _state(SHAPE, 0.35)
    du, dc, dx = u.cuda(), c.cuda(), x.cuda()
    carry_dev = torch.tensor([CARRY], dtype=torch.float32, device="cuda")
    errs, herrs, serrs = {}, {}, {}
    for order, coefs in enumerate(_multistep_coefs(), 1):
        coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
        for mode in (0, 1, 2, 4, 5, 6):
            thr = _threshold(u, c, prev, CARRY, mode & 3, coefs[1], coefs[2])
            for apg in ((0.0, None), (0.5, thr)):
                m, e64 = _me64(u, c, x, prev, CARRY, mode, coefs, apg)
                ref, x0 = _host_multistep(m, x, h, mode, coefs)
                dh, st = h.cuda(), prev.cuda()
                out = K.cfg_multistep_step(du, dc, dx, dh, mode, coefs, apg=apg, apg_momentum=(st, CARRY))
                assert out.dtype == dt and out.shape == SHAPE and dh.dtype == torch.float32
                key = f"order{order}_mode{mode}_apg{apg[0]}"
                errs[key], herrs[key], serrs[key] = e, eh, es = rel(out, ref), rel(dh, x0), _state_excess(st, e64, u, c, prev, CARRY)
                assert e < TOL[dt] and eh < HIST_TOL and es <= 1.0, (key, e, eh, es)
                dh2, st2 = h.cuda(), prev.cuda()
                out2 = K.cfg_multistep_step(du, dc, dx, dh2, mode, (0.0,) * 6, coef_dev=coef_dev, apg=apg, apg_momentum=(st2, 0.0),
                                            carry_dev=carry_dev)
                assert torch.equal(out2, out) and torch.equal(dh2, dh) and torch.equal(st2, st), key
    print(f"cfg_multistep_step apg momentum {dt}: max rel out {max(errs.values()):.3g} hist {max(herrs.values()):.3g}, "
          f"state error / bound {max(serrs.values()):.3g}")
    _record(f"cfg_multistep_step_apg_momentum_{_name(dt)}", max_rel=max(errs.values()), max_hist_rel=max(herrs.values()),
            max_state_excess=max(serrs.values()))
    with pytest.raises(ValueError, match="mode bit 8"):
        K.cfg_multistep_step(du, dc, dx, h.cuda(), 1 | 8, coefs, apg=(0.0, None), apg_momentum=(prev.cuda(), CARRY))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_momentum_grid_stride_and_all_records(dt):
    """The large size: 256 records, every workgroup of both launches loops; finite, within TOL and the state bound, twice the same bits."""
    sch, t = _sched()
    n = LARGE * 8
    gen = torch.Generator().manual_seed(53)
    u, c, x, z = (torch.randn(n, generator=gen).to(dt) for _ in range(4))
    u, c = u * 0.25, c * 0.25
    prev = _state((n,), 0.35)
    dev = [v.cuda() for v in (u, c, x, z)]
    coefs = sch.step_coefficients(t, 1.0, G)
    apg = (0.0, _threshold(u, c, prev, CARRY, 1, coefs[1], coefs[2]))
    st = prev.cuda()
    out = K.cfg_ddim_step(*dev, 1 | 4, coefs, apg=apg, apg_momentum=(st, CARRY))
    m, e64 = _me64(u, c, x, prev, CARRY, 1, coefs, apg)
    e, es = rel(out, _host_step(m, m, x, z, 1 | 4, coefs)), _state_excess(st, e64, u, c, prev, CARRY)
    print(f"apg momentum grid stride {dt}: step rel err {e:.3g}, state error / bound {es:.3g}")
    _record(f"cfg_ddim_step_apg_momentum_grid_stride_{_name(dt)}", step_rel=e, state_excess=es)
    assert torch.isfinite(out.float()).all() and e < TOL[dt] and es <= 1.0, (e, es)
    st2 = prev.cuda()
    assert torch.equal(K.cfg_ddim_step(*dev, 1 | 4, coefs, apg=apg, apg_momentum=(st2, CARRY)), out) and torch.equal(st2, st)


def _window_cases():
    for ci, (shape, L, starts) in enumerate(WINDOW_CASES):
        F = shape[len(shape) - 3]
        yield ci, shape, L, starts, False
        yield ci, shape, L, [(s + F - 3) % F for s in starts], True


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_momentum_windows_kernels_vs_fp64(dt):
    """Both windowed forms, V = 8 and V = 1, on a line and on a ring, against fp64 blends of the two halves, then the definition with
    the state on the clip of blends, then the step."""
    sch, t = _sched()
    errs, herrs, serrs, aerrs = {}, {}, {}, {}
    for ci, shape, L, starts, ring in _window_cases():
        preds, x, z = windows_case(shape, L, WINDOW_CASES[ci][2], dt, seed=170 + ci)
        prev = _state(shape, 0.35, seed=11 + ci)
        dp, dx, dz = preds.cuda(), x.cuda(), z.cuda()
        st_dev = torch.tensor(starts, dtype=torch.int32, device="cuda")
        w = context_weights(L, "pyramid")
        dw = w.cuda()
        ub, cb = _blend_uc64(preds, x, starts, w, ring)
        ua, ca = _blend_uc64(preds.abs(), x, starts, w, ring)
        blend = (len(starts) + 4) * 2.0 ** -24 * (ua + ca)
        for eta in (0.0, 0.8):
            coefs = sch.step_coefficients(t, eta, G)
            noise, dnoise = (z, dz) if eta > 0 else (None, None)
            for pred in (0, 1, 2):
                apg = (0.5, _threshold(ub, cb, prev, CARRY, pred, coefs[1], coefs[2])) if pred == 1 else (0.0, None)
                m, e64 = _me64(ub, cb, x, prev, CARRY, pred, coefs, apg)
                if eta == 0.0:
                    alpha, s, _, eq, _, _ = _scalars64(ub, cb, x, prev, CARRY, pred, G, coefs[1], coefs[2], *apg)
                    dprev = prev.cuda()
                    got = K.cfg_apg_scalars_windows(dp, dx, st_dev, dw, pred, coefs, apg, ring=ring, apg_momentum=(dprev, CARRY))
                    aerrs[f"case{ci}_ring{int(ring)}_pred{pred}"] = max(abs(float(got[0]) - alpha) / eq, abs(float(got[1]) / s - 1.0))
                    assert torch.equal(dprev.cpu(), prev)
                for extra in (0, 4, 8, 12):
                    mode = pred | extra
                    ref = _host_step(m, m, x, noise, mode, coefs)
                    st = prev.cuda()
                    out = K.cfg_ddim_step_windows(dp, dx, dnoise, st_dev, dw, mode, coefs, ring=ring, apg=apg, apg_momentum=(st, CARRY))
                    assert out.dtype == dt and out.shape == x.shape
                    key = f"case{ci}_ring{int(ring)}_eta{eta}_mode{mode}"
                    errs[key], serrs[key] = e, es = rel(out, ref), _state_excess(st, e64, ub, cb, prev, CARRY, blend)
                    assert e < TOL[dt] and es <= 1.0, (key, e, es)
        h = _hist(shape, seed=9 + ci)
        carry_dev = torch.tensor([CARRY], dtype=torch.float32, device="cuda")
        for order, coefs in enumerate(_multistep_coefs(), 1):
            for mode in (0, 1, 2, 5):
                apg = (0.0, _threshold(ub, cb, prev, CARRY, mode & 3, coefs[1], coefs[2])) if mode == 1 else (0.5, None)
                m, e64 = _me64(ub, cb, x, prev, CARRY, mode, coefs, apg)
                ref, x0 = _host_multistep(m, x, h, mode, coefs)
                dh, st = h.cuda(), prev.cuda()
                out = K.cfg_multistep_step_windows(dp, dx, dh, st_dev, dw, mode, coefs, ring=ring, apg=apg, apg_momentum=(st, CARRY))
                key = f"case{ci}_ring{int(ring)}_order{order}_mode{mode}"
                errs[key], herrs[key], serrs[key] = e, eh, es = rel(out, ref), rel(dh, x0), _state_excess(st, e64, ub, cb, prev, CARRY, blend)
                assert e < TOL[dt] and eh < HIST_TOL and es <= 1.0, (key, e, eh, es)
                dh2, st2 = h.cuda(), prev.cuda()
                out2 = K.cfg_multistep_step_windows(dp, dx, dh2, st_dev, dw, mode, coefs, ring=ring, apg=apg, apg_momentum=(st2, 0.0),
                                                    carry_dev=carry_dev)
                assert torch.equal(out2, out) and torch.equal(dh2, dh) and torch.equal(st2, st), key
    print(f"apg momentum windows {dt}: max rel out {max(errs.values()):.3g} hist {max(herrs.values()):.3g} scalars {max(aerrs.values()):.3g}, "
          f"state error / bound {max(serrs.values()):.3g}")
    _record(f"cfg_step_windows_apg_momentum_{_name(dt)}", max_rel=max(errs.values()), max_hist_rel=max(herrs.values()),
            max_scalar_err=max(aerrs.values()), max_state_excess=max(serrs.values()))
    assert max(aerrs.values()) <= FACTOR_TOL, aerrs


# ------------------------------------------------------------------------------------------------ 6. bit-level guarantees
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_carry_zero_with_a_nan_state_is_the_momentum_less_step(dt):
    """(a) carry = 0, the state pre-filled with NaN: the output of the ``apg=`` call on the same inputs, the state c - u in fp32 -- all
    four step forms, from the host carry and from the device carry."""
    sch, t = _sched()
    u, c, x, z = _inputs(dt, seed=61)
    du, dc, dx, dz = (v.cuda() for v in (u, c, x, z))
    d32 = dc.float() - du.float()
    zero_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
    nan = lambda like: torch.full(like.shape, float("nan"), dtype=torch.float32, device="cuda")
    first, second = _multistep_coefs()
    for apg in ((0.0, None), (0.5, 0.05)):
        for kw in (dict(), dict(carry_dev=zero_dev)):
            host = 0.0 if not kw else 0.25                            # (with a device carry the host value is not read)
            for eta in (0.0, 0.8):
                coefs = sch.step_coefficients(t, eta, G)
                for mode in (0, 1, 2, 1 | 4, 1 | 12):
                    st = nan(dx)
                    a = K.cfg_ddim_step(du, dc, dx, dz if eta > 0 else None, mode, coefs, apg=apg, apg_momentum=(st, host), **kw)
                    assert torch.equal(a, K.cfg_ddim_step(du, dc, dx, dz if eta > 0 else None, mode, coefs, apg=apg)), (apg, eta, mode)
                    assert torch.equal(st, d32)
            for coefs in (first, second):
                for mode in (0, 1, 2, 5):
                    st, ha, hb = nan(dx), _hist(SHAPE).cuda(), _hist(SHAPE).cuda()
                    a = K.cfg_multistep_step(du, dc, dx, ha, mode, coefs, apg=apg, apg_momentum=(st, host), **kw)
                    assert torch.equal(a, K.cfg_multistep_step(du, dc, dx, hb, mode, coefs, apg=apg)) and torch.equal(ha, hb)
                    assert torch.equal(st, d32)
    coefs = sch.step_coefficients(t, 0.0, G)
    for ci, shape, L, starts, ring in _window_cases():
        preds, xs, _ = windows_case(shape, L, WINDOW_CASES[ci][2], dt, seed=62 + ci)
        dp, dxs = preds.cuda(), xs.cuda()
        sd, dw = torch.tensor(starts, dtype=torch.int32, device="cuda"), context_weights(L, "pyramid").cuda()
        for apg in ((0.0, None), (0.5, 0.05)):
            st = nan(dxs)
            a = K.cfg_ddim_step_windows(dp, dxs, None, sd, dw, 1, coefs, ring=ring, apg=apg, apg_momentum=(st, 0.0))
            assert torch.equal(a, K.cfg_ddim_step_windows(dp, dxs, None, sd, dw, 1, coefs, ring=ring, apg=apg))
            assert torch.isfinite(st).all()
            st2, ha, hb = nan(dxs), _hist(shape).cuda(), _hist(shape).cuda()
            a = K.cfg_multistep_step_windows(dp, dxs, ha, sd, dw, 1, second, ring=ring, apg=apg, apg_momentum=(st2, 0.0))
            assert torch.equal(a, K.cfg_multistep_step_windows(dp, dxs, hb, sd, dw, 1, second, ring=ring, apg=apg)) and torch.equal(ha, hb)
            assert torch.equal(st2, st)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_exact_inputs_give_the_fp32_expression_after_two_chained_steps(dt):
    """(b) u, c small integers over 8 and carry -0.5: d, carry * e_prev and their sum are exact in fp32, so the state after two
    chained steps is the fp32 torch expression bit for bit, whatever the scalars are."""
    sch, t = _sched()
    gen = torch.Generator().manual_seed(71)
    u0, c0, u1, c1 = (torch.randint(-32, 33, SHAPE, generator=gen).to(torch.float32).div(8).to(dt).cuda() for _ in range(4))
    x = torch.randn(SHAPE, generator=gen).to(dt).cuda()
    coefs = sch.step_coefficients(t, 0.0, G)
    st = torch.full(SHAPE, float("nan"), dtype=torch.float32, device="cuda")
    x1 = K.cfg_ddim_step(u0, c0, x, None, 1, coefs, apg=(0.0, None), apg_momentum=(st, 0.0))
    assert torch.equal(st, c0.float() - u0.float())
    K.cfg_ddim_step(u1, c1, x1, None, 1, coefs, apg=(0.0, 0.05), apg_momentum=(st, -0.5))
    assert torch.equal(st, (c1.float() - u1.float()) + (-0.5) * (c0.float() - u0.float()))
    h = _hist(SHAPE).cuda()
    K.cfg_multistep_step(u0, c0, x, h, 1, _multistep_coefs()[1], apg=(0.0, None), apg_momentum=(st, 0.25))
    assert torch.equal(st, (c0.float() - u0.float()) + 0.25 * ((c1.float() - u1.float()) + (-0.5) * (c0.float() - u0.float())))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_one_uniform_window_is_the_plain_momentum_step_bit_for_bit(dt):
    """(e) one uniform window with L = F: the plain kernels' output, state (and history), and scalars, on 16-byte and scalar lanes."""
    sch, t = _sched()
    for shape in ((1, 4, 5, 7, 24), (1, 3, 4, 5, 4, 8), (1, 4, 8, 3, 5)):
        L = shape[-3]
        preds, x, z = windows_case(shape, L, [0], dt, seed=81)
        prev = _state(shape, 0.35)
        dp, dx, dz = preds.cuda(), x.cuda(), z.cuda()
        du, dc = dp[0, 0:1].contiguous(), dp[0, 1:2].contiguous()
        sd = torch.zeros(1, dtype=torch.int32, device="cuda")
        w = context_weights(L, "uniform").cuda()
        h = _hist(shape)
        for ring in (False, True):
            for apg in ((0.0, None), (0.5, 0.05)):
                for eta in (0.0, 0.8):
                    coefs = sch.step_coefficients(t, eta, G)
                    noise = dz if eta > 0 else None
                    for mode in (0, 1, 2, 1 | 4, 1 | 12):
                        sa_, sb_ = prev.cuda(), prev.cuda()
                        a = K.cfg_ddim_step_windows(dp, dx, noise, sd, w, mode, coefs, ring=ring, apg=apg, apg_momentum=(sa_, CARRY))
                        b = K.cfg_ddim_step(du, dc, dx, noise, mode, coefs, apg=apg, apg_momentum=(sb_, CARRY))
                        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (shape, ring, apg, eta, mode)
                        assert torch.equal(sa_.view(torch.int32), sb_.view(torch.int32)), (shape, ring, apg, eta, mode)
                    sw = K.cfg_apg_scalars_windows(dp, dx, sd, w, 1, coefs, apg, ring=ring, apg_momentum=(prev.cuda(), CARRY))
                    sp = K.cfg_apg_scalars(du, dc, dx, 1, coefs, apg, apg_momentum=(prev.cuda(), CARRY))
                    assert torch.equal(sw.view(torch.int32), sp.view(torch.int32))
                for coefs in _multistep_coefs():
                    for mode in (0, 1, 2, 5):
                        ha, hb, sa_, sb_ = h.cuda(), h.cuda(), prev.cuda(), prev.cuda()
                        a = K.cfg_multistep_step_windows(dp, dx, ha, sd, w, mode, coefs, ring=ring, apg=apg, apg_momentum=(sa_, CARRY))
                        b = K.cfg_multistep_step(du, dc, dx, hb, mode, coefs, apg=apg, apg_momentum=(sb_, CARRY))
                        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (shape, ring, apg, coefs[5], mode)
                        assert torch.equal(ha.view(torch.int32), hb.view(torch.int32)) and torch.equal(sa_.view(torch.int32), sb_.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 7. guarded buffers
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_momentum_steps_between_guard_bands(dt):
    """The plain steps at the ragged shape and the windows steps (16-byte and scalar lanes) with the state, the outputs, the history,
    the workspace and the carry buffer between poisoned guards: no store outside, every state and output element written.  The state
    starts as the poison pattern (a NaN) with carry 0, so an element the kernel skipped would still hold it."""
    sch, t = _sched()
    coefs = sch.step_coefficients(t, 0.8, G)
    first, second = _multistep_coefs()
    u, c, x, z = _inputs(dt, seed=31)
    prev = _state(SHAPE, 0.35)
    g = Guarded(K)
    du, dc, dx, dz = (g.guard(v.cuda()) for v in (u, c, x, z))
    st, sth, dh = g.guard(prev.cuda()), g.guard(prev.cuda()), g.guard(_hist(SHAPE).cuda())
    carry_dev = g.guard(torch.tensor([CARRY], dtype=torch.float32, device="cuda"))
    with g:                                                            # (the workspaces are torch.empty inside K: guarded too)
        out = g.out(K.cfg_ddim_step(du, dc, dx, dz, 1 | 4, coefs, apg=(0.5, None), apg_momentum=(st, 0.0), carry_dev=carry_dev))
        out_m = g.out(K.cfg_multistep_step(du, dc, dx, dh, 1, second, apg=(0.5, None), apg_momentum=(sth, CARRY)))
        g.out(st), g.out(sth), g.out(dh)
    m, e64 = _me64(u, c, x, prev, CARRY, 1, coefs, (0.5, None))
    assert rel(out, _host_step(m, m, x, z, 1 | 4, coefs)) < TOL[dt] and _state_excess(st, e64, u, c, prev, CARRY) <= 1.0
    m, e64 = _me64(u, c, x, prev, CARRY, 1, second, (0.5, None))
    assert rel(out_m, _host_multistep(m, x, _hist(SHAPE), 1, second)[0]) < TOL[dt] and _state_excess(sth, e64, u, c, prev, CARRY) <= 1.0
    for ci, shape, L, starts, ring in _window_cases():
        preds, xs, zs = windows_case(shape, L, WINDOW_CASES[ci][2], dt, seed=33)
        w = context_weights(L, "pyramid")
        g = Guarded(K)
        dp, dxs, dzs, ds, dw = (g.guard(v.cuda()) for v in (preds, xs, zs, torch.tensor(starts, dtype=torch.int32), w))
        dh = g.guard(_hist(shape).cuda())
        st = g.empty(tuple(xs.shape), torch.float32, "cuda")           # the poison pattern: NaN, never read with carry 0
        sth = g.empty(tuple(xs.shape), torch.float32, "cuda")
        with g:
            out = g.out(K.cfg_ddim_step_windows(dp, dxs, dzs, ds, dw, 1 | 4, coefs, ring=ring, apg=(0.5, None), apg_momentum=(st, 0.0)))
            out_m = g.out(K.cfg_multistep_step_windows(dp, dxs, dh, ds, dw, 1, second, ring=ring, apg=(0.5, None), apg_momentum=(sth, 0.0)))
            g.out(st), g.out(sth), g.out(dh)
        ub, cb = _blend_uc64(preds, xs, starts, w, ring)
        assert rel(st, cb - ub) < 1e-6 and torch.equal(st, sth)
        assert torch.isfinite(out.float()).all() and torch.isfinite(out_m.float()).all()
    # the statistics pass: records(n) records of four floats are written, nothing behind them, and the state is only read
    recs = K.lib().im360_cfg_rescale_records(x.numel())
    assert recs == 2
    g = Guarded(K)
    du, dc, dx, dst = (g.guard(v.cuda()) for v in (u, c, x, prev))
    ws = g.empty(((recs + 4) * K.RESCALE_RECORD,), torch.float32, "cuda")
    rc = K.lib().im360_cfg_apg_momentum_stats(du.data_ptr(), dc.data_ptr(), dx.data_ptr(), dst.data_ptr(), x.numel(), coefs[1], coefs[2], 1,
                                              CARRY, None, ws.data_ptr(), ws.numel(), K._dt(du), None, None)
    assert rc == 0, K.lib().im360_last_error()
    g.check()
    poisoned = (ws.view(torch.int32) == _SENTINEL[4]).cpu().view(recs + 4, K.RESCALE_RECORD)
    assert not poisoned[:recs, :4].any() and poisoned[recs:].all(), poisoned
    assert float(ws[0] + ws[K.RESCALE_RECORD]) == x.numel() and torch.equal(dst.cpu(), prev)


# ------------------------------------------------------------------------------------------------ the argument checks
def test_momentum_entry_points_reject_bad_arguments():
    """Host-side checks only: nothing is launched."""
    a = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(24, dtype=torch.float32, device="cuda")
    coefs = (7.5, 0.5, 0.8, 0.6, 0.7, 0.0)
    with pytest.raises(ValueError, match="apg_momentum needs apg"):
        K.cfg_ddim_step(a, a, a, None, 1, coefs, apg_momentum=(f[:16], 0.0))
    with pytest.raises(ValueError, match="carry"):
        K.cfg_ddim_step(a, a, a, None, 1, coefs, apg=(0.0, None), apg_momentum=(f[:16], float("nan")))
    with pytest.raises(AssertionError):
        K.cfg_ddim_step(a, a, a, None, 1, coefs, apg=(0.0, None), apg_momentum=(f[:8], 0.0))                    # element count
    with pytest.raises(AssertionError):
        K.cfg_ddim_step(a, a, a, None, 1, coefs, apg=(0.0, None), apg_momentum=(a.clone(), 0.0))                # dtype
    with pytest.raises(AssertionError):
        K.cfg_ddim_step(a, a, a, None, 1, coefs, apg=(0.0, None), apg_momentum=(f[:16], 0.0), carry_dev=f[:2])  # float32[1]
    with pytest.raises(RuntimeError, match="cuda"):
        K.cfg_ddim_step(a, a, a, None, 1, coefs, apg=(0.0, None), apg_momentum=(torch.zeros(16), 0.0))
    lib, p, sp = K.lib(), a.data_ptr(), f.data_ptr()
    hist = torch.zeros(16, dtype=torch.float32, device="cuda")
    ws = torch.zeros(K.RESCALE_RECORD, dtype=torch.float32, device="cuda")
    wp, hp = ws.data_ptr(), hist.data_ptr()

    def ddim(state=sp, carry=0.0, cdev=None, eta=0.0, ws_ptr=wp):
        return lib.im360_cfg_ddim_step_apg_momentum(p, p, p, None, state, p, 16, *coefs, 1, eta, 1.0, ws_ptr, 8, carry, cdev, 0, None, None)

    def multi(state=sp, carry=0.0, cdev=None, eta=0.0, ws_ptr=wp):
        return lib.im360_cfg_multistep_step_apg_momentum(p, p, p, hp, state, p, 16, *coefs, 1, eta, 1.0, ws_ptr, 8, carry, cdev, 0, None, None)

    def stats(state=sp, carry=0.0, cdev=None, ws_ptr=wp):
        return lib.im360_cfg_apg_momentum_stats(p, p, p, state, 16, 0.5, 0.8, 1, carry, cdev, ws_ptr, 8, 0, None, None)

    for fn in (ddim, multi, stats):
        assert fn(state=None) != 0 and b"null or misaligned momentum state" in lib.im360_last_error()
        assert fn(state=sp + 4) != 0 and b"null or misaligned momentum state" in lib.im360_last_error()
        for carry in (float("nan"), float("inf")):
            assert fn(carry=carry) != 0 and b"carry" in lib.im360_last_error() and b"must be finite" in lib.im360_last_error()
        assert fn(cdev=sp + 2) != 0 and b"misaligned device carry" in lib.im360_last_error()
        assert fn(ws_ptr=None) != 0 and b"null or misaligned workspace" in lib.im360_last_error()
    for fn in (ddim, multi):
        assert fn(eta=float("inf")) != 0 and b"must be finite" in lib.im360_last_error()
    assert multi(state=hp) != 0 and b"one buffer" in lib.im360_last_error()
    x = torch.zeros(1, 4, 4, 2, 8, dtype=torch.bfloat16, device="cuda")
    pr = torch.zeros(2, 2, 4, 2, 2, 8, dtype=torch.bfloat16, device="cuda")
    hx, sx = (torch.zeros(x.shape, dtype=torch.float32, device="cuda") for _ in range(2))
    st, w = torch.tensor([0, 2], dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    q, geo = x.data_ptr(), (2, 4, 4, 2, 16)

    def wddim(state=sx.data_ptr(), carry=0.0, wrap=0):
        return lib.im360_cfg_ddim_step_windows_apg_momentum(pr.data_ptr(), q, None, state, q, st.data_ptr(), w.data_ptr(), *geo, wrap, *coefs, 1,
                                                            0.0, 1.0, wp, 8, carry, None, 0, None, None)

    def wmulti(state=sx.data_ptr(), carry=0.0, wrap=0):
        return lib.im360_cfg_multistep_step_windows_apg_momentum(pr.data_ptr(), q, hx.data_ptr(), state, q, st.data_ptr(), w.data_ptr(), *geo,
                                                                 wrap, *coefs, 1, 0.0, 1.0, wp, 8, carry, None, 0, None, None)

    def wstats(ring, state=sx.data_ptr(), carry=0.0):
        fn = lib.im360_cfg_apg_momentum_stats_windows_ring if ring else lib.im360_cfg_apg_momentum_stats_windows
        return fn(pr.data_ptr(), q, state, st.data_ptr(), w.data_ptr(), *geo, 0.5, 0.8, 1, carry, None, wp, 8, 0, None, None)

    for fn in (wddim, wmulti, lambda **k: wstats(False, **k), lambda **k: wstats(True, **k)):
        assert fn(state=None) != 0 and b"null or misaligned momentum state" in lib.im360_last_error()
        assert fn(state=sx.data_ptr() + 2) != 0 and b"null or misaligned momentum state" in lib.im360_last_error()
        assert fn(carry=float("nan")) != 0 and b"must be finite" in lib.im360_last_error()
    for fn in (wddim, wmulti):
        assert fn(wrap=3) != 0 and b"wrap=3 must be 0 (line) or F=4 (ring)" in lib.im360_last_error()
    assert wmulti(state=hx.data_ptr()) != 0 and b"one buffer" in lib.im360_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 8. the pipeline
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
MOM = dict(apg_momentum=-0.5, **APG)
WINDOWS = dict(frames=24, context_frames=16, context_overlap=8)


def _graphed_vs_eager(gpu_run, monkeypatch, name, windows, replays_expected, **kw):
    """Both runs; the graphed one must have replayed captured steps that own momentum states and left ``_apg_prev_t`` at the last
    guided timestep."""
    from imagine360_amd import graph_step
    cls = graph_step.GraphedWindowedStep if windows else graph_step.GraphedDenoiseStep
    replays = []
    orig = cls.step
    monkeypatch.setattr(cls, "step", lambda self, t: (replays.append((self.apg_beta, self._apg_prev_t)), orig(self, t))[1])
    out = {}
    for graph in (True, False):
        out[graph] = gpu_run(graph, **(WINDOWS if windows else {}), **kw)
    assert len(replays) == replays_expected and all(b == -0.5 for b, _ in replays), replays
    errs = dict(pano=rel(out[True][1], out[False][1]), pers=rel(out[True][2], out[False][2]))
    _record(f"graphed_vs_eager_apg_momentum_{name}", **errs)
    assert _same(out[True], out[False]), errs
    assert all(torch.isfinite(v.float()).all() for v in out[True])
    return out[True], replays


@pytest.mark.parametrize("windows", [False, True], ids=["plain", "windows"])
def test_graphed_momentum_steps_equal_eager_bit_for_bit(gpu_run, windows, monkeypatch):
    """beta = -0.5, 3 steps: the statistics and step launches with the state are captured, the carry is uploaded per step, and the replay
    gives the eager loop's numbers.  The warm-up leaves the predecessor None: the first replayed step has carry 0."""
    on, replays = _graphed_vs_eager(gpu_run, monkeypatch, "windows" if windows else "plain", windows, 3, **MOM)
    steps = gpu_run.pipe.scheduler._timesteps_host
    assert [p for _, p in replays] == [None, steps[0], steps[1]]
    ctx = WINDOWS if windows else {}
    off = gpu_run(True, **ctx, **APG)
    assert _same(off, gpu_run(True, **ctx, apg_momentum=None, **APG))            # None: the call without the keyword
    assert _same(off, gpu_run(True, **ctx, apg_momentum=0.0, **APG))             # 0.0: the same bits through the kernels with the state
    assert rel(on[1], off[1]) > 1e-3                                             # and the momentum is another clip


def test_graphed_momentum_steps_equal_eager_under_a_guidance_interval(gpu_run, monkeypatch):
    """4 steps under (0.2, 0.6): the guided steps alone upload a carry and move the predecessor."""
    sch = gpu_run.pipe.scheduler
    _, replays = _graphed_vs_eager(gpu_run, monkeypatch, "guidance_interval", False, 4, steps=4, guidance_interval=(0.2, 0.6), **MOM)
    steps = sch._timesteps_host
    flags = sch.guided_steps(steps, (0.2, 0.6))
    assert 0 < sum(flags) < 4
    want, prev = [], None
    for t, f in zip(steps, flags):
        want.append(prev)
        prev = t if f else prev
    assert [p for _, p in replays] == want


def test_graphed_momentum_steps_equal_eager_over_free_init_passes(gpu_run, monkeypatch):
    """Two passes of 2 steps: ``restart`` clears the predecessor, so each pass begins with carry 0 on the state of the pass before."""
    _, replays = _graphed_vs_eager(gpu_run, monkeypatch, "free_init", False, 4, steps=2, free_init_iters=2, **MOM)
    steps = gpu_run.pipe.scheduler._timesteps_host
    assert [p for _, p in replays] == [None, steps[0], None, steps[0]]


def test_graphed_momentum_steps_equal_eager_with_dpm_solver(gpu_run, monkeypatch):
    pipe = gpu_run.pipe
    saved = pipe.scheduler
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(saved.config)
    try:
        _graphed_vs_eager(gpu_run, monkeypatch, "dpm_solver_2m", False, 3, **MOM)
    finally:
        pipe.scheduler = saved


def test_eager_momentum_steps_equal_the_chain_written_out_on_the_wrappers(gpu_run):
    """Two eager steps against the chain written out per branch on ``K.cfg_ddim_step(..., apg_momentum=)`` with a state and a
    predecessor of its own: the same bits."""
    pipe = gpu_run.pipe
    got = gpu_run(False, steps=2, **MOM)
    sch = pipe.scheduler
    chain = {}

    def step(u, c, g, t, x, coef_dev=None, **kw):
        assert kw.pop("guidance_apg") == (0.0, 0.5)
        kw.pop("guidance_apg_momentum")
        branch = x.dim()
        state, t_prev = chain.get(branch, (torch.full(x.shape, float("nan"), dtype=torch.float32, device=x.device), None))
        out = K.cfg_ddim_step(u.contiguous(), c.contiguous(), x.contiguous(), None, sch.kernel_mode(), sch.step_coefficients(t, 0.0, g),
                              apg=(0.0, 0.5), apg_momentum=(state, sch.apg_carry(t_prev, t, -0.5)))
        chain[branch] = (state, t)
        return out
    sch.fused_cfg_step = step
    try:
        want = gpu_run(False, steps=2, **MOM)
    finally:
        del sch.fused_cfg_step
    assert len(chain) == 2 and _same(got, want)
