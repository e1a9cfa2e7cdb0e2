"""Torch stand-ins of the momentum forms of the adaptive-projected-guidance kernels (csrc/sampler_step.hip: cfg_apg_momentum_stats_kernel
/ cfg_apg_momentum_stats_windows_kernel + the four cfg_*_step*_apg_momentum_kernel) for the CPU tier: the four guided step wrappers and
the two scalar wrappers of ``kernels`` with the ``apg_momentum`` / ``carry_dev`` keywords.  ``apg_momentum=None`` is the stand-in of
_emu_apg_step.py, called with exactly the arguments it had; otherwise ``scheduler.projected_guidance(..., momentum=)`` -- the definition
-- forms (m, e) in fp32 from u, c (for windows: the blends of the two halves), the fp32 sample and the state, e is stored to the state in
place, and m is stepped with the formulas of _emu_rescale_step.py / _emu_multistep_step.py.  With carry == 0 the state is not read.
Layered on _emu_apg_step.patched_apg_kernels()."""
import contextlib
import math

import torch

import _emu_apg_step as EA
import _emu_multistep_step as EM
import _emu_rescale_step as ER
from imagine360_amd.scheduler import projected_guidance

CALLS = []          # one entry per stand-in call with a state: (wrapper name, carry, the state tensor)


def _carry(who, apg, apg_momentum, carry_dev, sample):
    """The wrappers' checks (kernels._apg_momentum_args); -> (state, the carry the kernel would read)."""
    if apg is None:
        raise ValueError(f"{who}: apg_momentum needs apg")
    state, carry = apg_momentum
    carry = float(carry)
    if not math.isfinite(carry):
        raise ValueError(f"{who}: apg carry={carry} must be finite")
    assert state.dtype == torch.float32 and state.is_contiguous() and state.device == sample.device and state.numel() == sample.numel()
    if carry_dev is not None:
        assert carry_dev.dtype == torch.float32 and carry_dev.numel() == 1
        carry = float(carry_dev[0])
    return state, carry


def _me(who, u, c, sample, mode, coefs, coef_dev, apg, rescale, apg_momentum, carry_dev):
    state, carry = _carry(who, apg, apg_momentum, carry_dev, sample)
    eta, thr = EA._check(apg, rescale)
    g, sa, sb = EA._coefs(coefs, coef_dev)[:3]
    CALLS.append((who, carry, state))
    EA.CALLS.append(who)
    prev = state.reshape(sample.shape).clone() if carry != 0.0 else None          # carry 0: the state is not read
    m, e = projected_guidance(u.float(), c.float(), sample.float(), g, sa, sb, EA.PRED[mode & 3], eta, thr, momentum=(prev, carry))
    state.copy_(e.reshape(state.shape))
    return m, e


def _scalars(who, u, c, sample, mode, coefs, apg, coef_dev, apg_momentum, carry_dev):
    """EA.scalars on e: the statistics pass reads the state and leaves it alone."""
    state, carry = _carry(who, apg, apg_momentum, carry_dev, sample)
    e = c.float() - u.float()
    if carry != 0.0:
        e = e + carry * state.reshape(sample.shape)
    return _scalars_of(e, c, sample, mode, coefs, apg, coef_dev)


def _scalars_of(e, c, sample, mode, coefs, apg, coef_dev):
    eta, thr = EA._check(apg, 0.0)
    g, sa, sb = EA._coefs(coefs, coef_dev)[:3]
    rho, kp = ((-1.0 / sb, sb / sa), (-sa / sb, sb), (0.0, 1.0))[mode & 3]
    q = c.float() + rho * sample.float()
    alpha = (e * q).sum() / (q * q).sum()
    s = torch.tensor(1.0) if thr is None else torch.clamp(thr / (kp * (e * e).mean().sqrt()), max=1.0)
    return torch.stack([alpha, s, (g - 1.0) * s * (1.0 - eta) * alpha]).to(torch.float32)


def cfg_apg_scalars(uncond, cond, sample, mode, coefs, apg, coef_dev=None, apg_momentum=None, carry_dev=None):
    if apg_momentum is None:
        return EA.cfg_apg_scalars(uncond, cond, sample, mode, coefs, apg, coef_dev)
    return _scalars("cfg_apg_scalars", uncond, cond, sample, mode, coefs, apg, coef_dev, apg_momentum, carry_dev)


def cfg_apg_scalars_windows(preds, sample, starts, weights, mode, coefs, apg, coef_dev=None, ring=False, apg_momentum=None, carry_dev=None):
    if apg_momentum is None:
        return EA.cfg_apg_scalars_windows(preds, sample, starts, weights, mode, coefs, apg, coef_dev, ring)
    u, c = EA._blends(preds, sample, starts, weights, ring)
    return _scalars("cfg_apg_scalars_windows", u, c, sample, mode, coefs, apg, coef_dev, apg_momentum, carry_dev)


def cfg_ddim_step(uncond, cond, sample, noise, mode, coefs, coef_dev=None, rescale=0.0, apg=None, apg_momentum=None, carry_dev=None):
    if apg_momentum is None:
        return EA.cfg_ddim_step(uncond, cond, sample, noise, mode, coefs, coef_dev=coef_dev, rescale=rescale, apg=apg)
    m, _ = _me("cfg_ddim_step", uncond, cond, sample, mode, coefs, coef_dev, apg, rescale, apg_momentum, carry_dev)
    return ER._step_on(m, sample, noise, mode, coefs, coef_dev)


def cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=None, rescale=0.0, ring=False, apg=None,
                          apg_momentum=None, carry_dev=None):
    if apg_momentum is None:
        return EA.cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=coef_dev, rescale=rescale, ring=ring,
                                        apg=apg)
    if apg is None:
        raise ValueError("cfg_ddim_step_windows: apg_momentum needs apg")
    u, c = EA._blends(preds, sample, starts, weights, ring)
    m, _ = _me("cfg_ddim_step_windows", u, c, sample, mode, coefs, coef_dev, apg, rescale, apg_momentum, carry_dev)
    return ER._step_on(m, sample, noise, mode, coefs, coef_dev)


def cfg_multistep_step(uncond, cond, sample, hist, mode, coefs, coef_dev=None, rescale=0.0, apg=None, apg_momentum=None, carry_dev=None):
    if apg_momentum is None:
        return EA.cfg_multistep_step(uncond, cond, sample, hist, mode, coefs, coef_dev=coef_dev, rescale=rescale, apg=apg)
    m, _ = _me("cfg_multistep_step", uncond, cond, sample, mode, coefs, coef_dev, apg, rescale, apg_momentum, carry_dev)
    return EM._step_on(m, sample, hist, mode, coefs, coef_dev)


def cfg_multistep_step_windows(preds, sample, hist, starts, weights, mode, coefs, coef_dev=None, rescale=0.0, ring=False, apg=None,
                               apg_momentum=None, carry_dev=None):
    if apg_momentum is None:
        return EA.cfg_multistep_step_windows(preds, sample, hist, starts, weights, mode, coefs, coef_dev=coef_dev, rescale=rescale, ring=ring,
                                             apg=apg)
    if apg is None:
        raise ValueError("cfg_multistep_step_windows: apg_momentum needs apg")
    u, c = EA._blends(preds, sample, starts, weights, ring)
    m, _ = _me("cfg_multistep_step_windows", u, c, sample, mode, coefs, coef_dev, apg, rescale, apg_momentum, carry_dev)
    return EM._step_on(m, sample, hist, mode, coefs, coef_dev)


@contextlib.contextmanager
def patched_apg_momentum_kernels():
    """On top of ``EA.patched_apg_kernels()`` (entered here).  Yields (``EA.CALLS``, ``CALLS``), both emptied: the wrapper name of every
    projected guidance formed, and (name, carry, state) of every one formed with a momentum state, in order."""
    from imagine360_amd import kernels
    with EA.patched_apg_kernels() as apg_calls:
        saved = {n: getattr(kernels, n) for n in EA.NAMES}
        for n in EA.NAMES:
            setattr(kernels, n, globals()[n])
        del CALLS[:]
        try:
            yield apg_calls, CALLS
        finally:
            for n, fn in saved.items():
                setattr(kernels, n, fn)
