"""Torch stand-ins of the multistep step kernels (csrc/sampler_step.hip: cfg_multistep_step_kernel / cfg_multistep_step_windows_kernel)
for the CPU tier: ``kernels.cfg_multistep_step`` and ``kernels.cfg_multistep_step_windows``.  The guided prediction m (for windows: the
blend of _emu_rescale_step.py on a line, of _emu_ring_step.py on a ring; with ``rescale`` times r = rescale * std(c) / std(m) +
(1 - rescale)) is formed in fp32, x0 by the prediction-type formulas of _emu_ddim_step.py, then
    out = cx * x + c0 * x0 + c1 * hist        fp32, one rounding to the sample's dtype at the end
    hist <- x0                                fp32, in place
and, like the kernels, ``hist`` is not read when c1 == 0 (it may hold NaN).  Used on top of _emu_kernels.patched_kernels()."""
import contextlib

import torch

import _emu_rescale_step as ER
import _emu_ring_step as EG


def _step_on(m, sample, hist, mode, coefs, coef_dev):
    if coef_dev is not None:
        coefs = [float(v) for v in coef_dev]
    _, sa, sb, cx, c0, c1 = (float(v) for v in coefs)
    if hist is None or hist.dtype != torch.float32 or hist.numel() != sample.numel():
        raise ValueError("cfg_multistep_step: history must be a float32 tensor of the sample's element count")
    if mode & 8 or (mode & 3) == 3:
        raise ValueError(f"cfg_multistep_step: mode {mode} unsupported")
    x = sample.float()
    pred = mode & 3
    x0 = (x - sb * m) / sa if pred == 0 else sa * x - sb * m if pred == 1 else m
    if mode & 4:
        x0 = x0.clamp(-1.0, 1.0)
    out = cx * x + c0 * x0
    if c1 != 0.0:
        out = out + c1 * hist.reshape(x.shape)
    hist.copy_(x0.reshape(hist.shape))
    return out.to(sample.dtype)


def cfg_multistep_step(uncond, cond, sample, hist, mode, coefs, coef_dev=None, rescale=0.0):
    g = float(coef_dev[0]) if coef_dev is not None else coefs[0]
    u, c = uncond.float(), cond.float()
    m = u + g * (c - u)
    if rescale != 0.0:
        m = m * ER._factor(m, c, rescale)
    return _step_on(m, sample, hist, mode, coefs, coef_dev)


def cfg_multistep_step_windows(preds, sample, hist, starts, weights, mode, coefs, coef_dev=None, rescale=0.0, ring=False):
    g = float(coef_dev[0]) if coef_dev is not None else coefs[0]
    m, c = (EG.ring_blends if ring else ER.blends)(preds, sample, starts, weights, g)
    if rescale != 0.0:
        m = m * ER._factor(m, c, rescale)
    return _step_on(m, sample, hist, mode, coefs, coef_dev)


@contextlib.contextmanager
def patched_multistep_kernels():
    from imagine360_amd import kernels
    saved = kernels.cfg_multistep_step, kernels.cfg_multistep_step_windows
    kernels.cfg_multistep_step, kernels.cfg_multistep_step_windows = cfg_multistep_step, cfg_multistep_step_windows
    try:
        yield
    finally:
        kernels.cfg_multistep_step, kernels.cfg_multistep_step_windows = saved
