"""Torch stand-ins of the guidance-rescale kernels (csrc/sampler_step.hip: cfg_rescale_stats_kernel / cfg_rescale_stats_windows_kernel +
the rescaled cfg_ddim_step_kernel / cfg_ddim_step_windows_kernel) for the CPU tier: ``kernels.cfg_ddim_step`` and
``kernels.cfg_ddim_step_windows`` with the ``rescale`` keyword, and ``kernels.cfg_rescale_factor``.  rescale = 0 is the stand-in of
_emu_ddim_step.py / _emu_ctx_step.py unchanged; otherwise the guided prediction m (for windows: the blend) is formed in fp32, multiplied
by r = rescale * std(c) / std(m) + (1 - rescale) (torch.std, correction 1, over the whole tensor) and stepped with those files'
formulas.  Used on top of _emu_kernels.patched_kernels()."""
import contextlib

import torch

import _emu_ctx_step as EC
import _emu_ddim_step as ES


def _factor(m, c, rescale):
    return rescale * c.std() / m.std() + (1.0 - rescale)


def _step_on(m, sample, noise, mode, coefs, coef_dev):
    """The step on an already combined fp32 prediction m (guidance 1 on u = c = m is exact)."""
    if coef_dev is not None:
        coefs = [float(v) for v in coef_dev]
    if noise is None and coef_dev is None and coefs[5] != 0.0:
        raise ValueError("cfg_ddim_step: sigma > 0 needs a noise tensor")
    sigma = coefs[5] if noise is not None else 0.0
    return ES.cfg_ddim_step(m, m, sample.float(), None if noise is None else noise.float(), mode,
                            [1.0, *coefs[1:5], sigma]).to(sample.dtype)


def cfg_rescale_factor(uncond, cond, guidance, rescale, coef_dev=None):
    g = float(coef_dev[0]) if coef_dev is not None else guidance
    u, c = uncond.float(), cond.float()
    return _factor(u + g * (c - u), c, rescale).to(torch.float32)


def cfg_ddim_step(uncond, cond, sample, noise, mode, coefs, coef_dev=None, rescale=0.0):
    if rescale == 0.0:
        return ES.cfg_ddim_step(uncond, cond, sample, noise, mode, coefs, coef_dev=coef_dev)
    g = float(coef_dev[0]) if coef_dev is not None else coefs[0]
    u, c = uncond.float(), cond.float()
    m = u + g * (c - u)
    return _step_on(m * _factor(m, c, rescale), sample, noise, mode, coefs, coef_dev)


def blends(preds, sample, starts, weights, g):
    """(blend of u_k + g (c_k - u_k), blend of c_k) in fp32, accumulated over the windows in ascending order like _emu_ctx_step.py."""
    fd = sample.dim() - 3
    nW, L = preds.shape[0], preds.shape[fd + 1]
    assert preds.shape[1] == 2 and len(starts) == nW and len(weights) == L
    shape = [1] * sample.dim()
    shape[fd] = L
    w = weights.float().reshape(shape)
    acc_m = torch.zeros(sample.shape, dtype=torch.float32)
    acc_c = torch.zeros(sample.shape, dtype=torch.float32)
    wsum = torch.zeros([sample.shape[fd] if i == fd else 1 for i in range(sample.dim())], dtype=torch.float32)
    for k in range(nW):
        s = int(starts[k])
        u, c = preds[k, 0:1].float(), preds[k, 1:2].float()
        acc_m.narrow(fd, s, L).add_(w * (u + g * (c - u)))
        acc_c.narrow(fd, s, L).add_(w * c)
        wsum.narrow(fd, s, L).add_(w)
    return acc_m / wsum, acc_c / wsum


def cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=None, rescale=0.0):
    if rescale == 0.0:
        return EC.cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=coef_dev)
    g = float(coef_dev[0]) if coef_dev is not None else coefs[0]
    m, c = blends(preds, sample, starts, weights, g)
    return _step_on(m * _factor(m, c, rescale), sample, noise, mode, coefs, coef_dev)


@contextlib.contextmanager
def patched_rescale_kernels():
    from imagine360_amd import kernels
    saved = kernels.cfg_ddim_step, kernels.cfg_ddim_step_windows, kernels.cfg_rescale_factor
    kernels.cfg_ddim_step, kernels.cfg_ddim_step_windows, kernels.cfg_rescale_factor = cfg_ddim_step, cfg_ddim_step_windows, cfg_rescale_factor
    try:
        yield
    finally:
        kernels.cfg_ddim_step, kernels.cfg_ddim_step_windows, kernels.cfg_rescale_factor = saved
