"""Torch stand-in of ``kernels.cfg_ddim_step_windows`` (csrc/sampler_step.hip cfg_ddim_step_windows_kernel) for the CPU tier: the
per-frame weighted blend of the windows' CFG-combined predictions in fp32, accumulated over the windows in ascending order, then
the step formulas of _emu_ddim_step.py; one rounding to the sample's dtype at the end.  Used on top of
_emu_kernels.patched_kernels()."""
import contextlib

import torch

import _emu_ddim_step as ES


def cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=None):
    if coef_dev is not None:
        coefs = [float(v) for v in coef_dev]
    if noise is None and coef_dev is None and coefs[5] != 0.0:
        raise ValueError("cfg_ddim_step_windows: sigma > 0 needs a noise tensor")
    g = coefs[0]
    fd = sample.dim() - 3                       # frame axis of the sample and of preds [nW, 2, ...]
    nW, L = preds.shape[0], preds.shape[fd + 1]
    assert preds.shape[1] == 2 and len(starts) == nW and len(weights) == L
    shape = [1] * sample.dim()
    shape[fd] = L
    w = weights.float().reshape(shape)
    acc = torch.zeros(sample.shape, dtype=torch.float32)
    wsum = torch.zeros([sample.shape[fd] if i == fd else 1 for i in range(sample.dim())], dtype=torch.float32)
    for k in range(nW):
        s = int(starts[k])
        u, c = preds[k, 0:1].float(), preds[k, 1:2].float()
        acc.narrow(fd, s, L).add_(w * (u + g * (c - u)))
        wsum.narrow(fd, s, L).add_(w)
    m = (acc / wsum).to(sample.device)
    # the step on m: cfg_ddim_step's formulas with the combination already made (guidance 1 on u = c = m is exact)
    sigma = coefs[5] if noise is not None else 0.0          # (a null noise with device coefficients is zero noise, as in the kernel)
    return ES.cfg_ddim_step(m, m, sample.float(), None if noise is None else noise.float(), mode,
                            [1.0, *coefs[1:5], sigma]).to(sample.dtype)


@contextlib.contextmanager
def patched_windows_kernel():
    from imagine360_amd import kernels
    saved = kernels.cfg_ddim_step_windows
    kernels.cfg_ddim_step_windows = cfg_ddim_step_windows
    try:
        yield
    finally:
        kernels.cfg_ddim_step_windows = saved
