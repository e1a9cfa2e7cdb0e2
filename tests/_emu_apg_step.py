"""Torch stand-ins of the adaptive-projected-guidance kernels (csrc/sampler_step.hip: cfg_apg_stats_kernel / cfg_apg_stats_windows_kernel +
cfg_ddim_step_apg_kernel, cfg_ddim_step_windows_apg_kernel, cfg_multistep_step_apg_kernel, cfg_multistep_step_windows_apg_kernel) for
the CPU tier: ``kernels.cfg_ddim_step``, ``cfg_ddim_step_windows``, ``cfg_multistep_step`` and ``cfg_multistep_step_windows`` with the
``apg`` keyword, and ``kernels.cfg_apg_scalars`` / ``cfg_apg_scalars_windows``.  apg = None is the stand-in of _emu_ring_step.py /
_emu_multistep_step.py unchanged; otherwise u and c (for windows: the blends of the two halves, on a line or on a ring) are taken in
fp32, ``scheduler.projected_guidance`` -- the definition -- forms m from them and the fp32 sample, and m is stepped with those files'
formulas.  Used on top of _emu_kernels.patched_kernels()."""
import contextlib

import torch

import _emu_multistep_step as EM
import _emu_rescale_step as ER
import _emu_ring_step as EG
from imagine360_amd.scheduler import projected_guidance

PRED = {0: "epsilon", 1: "v_prediction", 2: "sample"}
CALLS = []          # one entry per stand-in call that formed a projected guidance: the wrapper's name


def _coefs(coefs, coef_dev):
    return [float(v) for v in coef_dev] if coef_dev is not None else [float(v) for v in coefs]


def _check(apg, rescale):
    if rescale != 0.0:
        raise ValueError("apg and rescale cannot be combined")
    eta, thr = apg
    if not torch.isfinite(torch.tensor(float(eta))) or (thr is not None and not float(thr) > 0.0):
        raise ValueError(f"apg={apg} out of range")
    return float(eta), None if thr is None else float(thr)


def _m(who, u, c, sample, mode, coefs, coef_dev, apg, rescale):
    eta, thr = _check(apg, rescale)
    g, sa, sb = _coefs(coefs, coef_dev)[:3]
    CALLS.append(who)
    return projected_guidance(u.float(), c.float(), sample.float(), g, sa, sb, PRED[mode & 3], eta, thr)


def _blends(preds, sample, starts, weights, ring):
    """(blend of u_k, blend of c_k) in fp32: guidance 0 makes the siblings' combined blend the blend of the unconditional halves."""
    return (EG.ring_blends if ring else ER.blends)(preds, sample, starts, weights, 0.0)


def scalars(u, c, sample, mode, coefs, apg, coef_dev=None):
    """(alpha, s, lambda) of the definition in fp32 tensors' own arithmetic: float32[3]."""
    eta, thr = _check(apg, 0.0)
    g, sa, sb = _coefs(coefs, coef_dev)[:3]
    pred = mode & 3
    rho, kp = ((-1.0 / sb, sb / sa), (-sa / sb, sb), (0.0, 1.0))[pred]
    d, q = c.float() - u.float(), c.float() + rho * sample.float()
    alpha = (d * q).sum() / (q * q).sum()
    s = torch.tensor(1.0) if thr is None else torch.clamp(thr / (kp * (d * d).mean().sqrt()), max=1.0)
    return torch.stack([alpha, s, (g - 1.0) * s * (1.0 - eta) * alpha]).to(torch.float32)


def cfg_apg_scalars(uncond, cond, sample, mode, coefs, apg, coef_dev=None):
    return scalars(uncond, cond, sample, mode, coefs, apg, coef_dev)


def cfg_apg_scalars_windows(preds, sample, starts, weights, mode, coefs, apg, coef_dev=None, ring=False):
    u, c = _blends(preds, sample, starts, weights, ring)
    return scalars(u, c, sample, mode, coefs, apg, coef_dev)


def cfg_ddim_step(uncond, cond, sample, noise, mode, coefs, coef_dev=None, rescale=0.0, apg=None):
    if apg is None:
        return ER.cfg_ddim_step(uncond, cond, sample, noise, mode, coefs, coef_dev=coef_dev, rescale=rescale)
    m = _m("cfg_ddim_step", uncond, cond, sample, mode, coefs, coef_dev, apg, rescale)
    return ER._step_on(m, sample, noise, mode, coefs, coef_dev)


def cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=None, rescale=0.0, ring=False, apg=None):
    if apg is None:
        return EG.cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=coef_dev, rescale=rescale, ring=ring)
    u, c = _blends(preds, sample, starts, weights, ring)
    m = _m("cfg_ddim_step_windows", u, c, sample, mode, coefs, coef_dev, apg, rescale)
    return ER._step_on(m, sample, noise, mode, coefs, coef_dev)


def cfg_multistep_step(uncond, cond, sample, hist, mode, coefs, coef_dev=None, rescale=0.0, apg=None):
    if apg is None:
        return EM.cfg_multistep_step(uncond, cond, sample, hist, mode, coefs, coef_dev=coef_dev, rescale=rescale)
    m = _m("cfg_multistep_step", uncond, cond, sample, mode, coefs, coef_dev, apg, rescale)
    return EM._step_on(m, sample, hist, mode, coefs, coef_dev)


def cfg_multistep_step_windows(preds, sample, hist, starts, weights, mode, coefs, coef_dev=None, rescale=0.0, ring=False, apg=None):
    if apg is None:
        return EM.cfg_multistep_step_windows(preds, sample, hist, starts, weights, mode, coefs, coef_dev=coef_dev, rescale=rescale, ring=ring)
    u, c = _blends(preds, sample, starts, weights, ring)
    m = _m("cfg_multistep_step_windows", u, c, sample, mode, coefs, coef_dev, apg, rescale)
    return EM._step_on(m, sample, hist, mode, coefs, coef_dev)


NAMES = ("cfg_ddim_step", "cfg_ddim_step_windows", "cfg_multistep_step", "cfg_multistep_step_windows", "cfg_apg_scalars",
         "cfg_apg_scalars_windows")


@contextlib.contextmanager
def patched_apg_kernels():
    """Yields ``CALLS``, emptied: the wrapper name of every projected guidance the stand-ins formed, in order."""
    from imagine360_amd import kernels
    saved = {n: getattr(kernels, n) for n in NAMES}
    for n in NAMES:
        setattr(kernels, n, globals()[n])
    del CALLS[:]
    try:
        yield CALLS
    finally:
        for n, fn in saved.items():
            setattr(kernels, n, fn)
