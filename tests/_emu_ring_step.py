"""Torch stand-ins of the ring entry points (csrc/sampler_step.hip: cfg_ddim_step_windows_kernel / cfg_rescale_stats_windows_kernel with
wrap = F) for the CPU tier: ``kernels.cfg_ddim_step_windows`` with the ``ring`` keyword and ``kernels.cfg_rescale_factor_windows``.
ring = False is the stand-in of _emu_rescale_step.py unchanged.  ring = True: window k adds its weighted predictions to the frames
(starts[k] + j) mod F in fp32, k ascending (no window covers a frame twice, so the order per frame is the kernel's), the sums are divided
by the per-frame weight sums, and the blend is stepped with the formulas of _emu_ddim_step.py; with ``rescale`` the blend is first
multiplied by r = rescale * std(c) / std(m) + (1 - rescale) over the whole clip.  Used on top of _emu_kernels.patched_kernels()."""
import contextlib

import torch

import _emu_rescale_step as ER


def ring_blends(preds, sample, starts, weights, g):
    """(blend of u_k + g (c_k - u_k), blend of c_k) in fp32 over the windows of a ring, slot k ascending."""
    fd = sample.dim() - 3
    F = sample.shape[fd]
    nW, L = preds.shape[0], preds.shape[fd + 1]
    assert preds.shape[1] == 2 and len(starts) == nW and len(weights) == L and L <= F
    shape = [1] * sample.dim()
    shape[fd] = L
    w = weights.float().reshape(shape)
    acc_m = torch.zeros(sample.shape, dtype=torch.float32)
    acc_c = torch.zeros(sample.shape, dtype=torch.float32)
    wsum = torch.zeros(F, dtype=torch.float32)
    for k in range(nW):
        s = int(starts[k])
        assert 0 <= s < F
        idx = (s + torch.arange(L)) % F
        u, c = preds[k, 0:1].float(), preds[k, 1:2].float()
        acc_m.index_add_(fd, idx, w * (u + g * (c - u)))
        acc_c.index_add_(fd, idx, w * c)
        wsum.index_add_(0, idx, weights.float())
    shape[fd] = F
    wsum = wsum.reshape(shape)
    return acc_m / wsum, acc_c / wsum


def cfg_rescale_factor_windows(preds, sample, starts, weights, guidance, rescale, coef_dev=None, ring=False):
    g = float(coef_dev[0]) if coef_dev is not None else guidance
    m, c = ring_blends(preds, sample, starts, weights, g) if ring else ER.blends(preds, sample, starts, weights, g)
    return ER._factor(m, c, rescale).to(torch.float32)


def cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=None, rescale=0.0, ring=False):
    if not ring:
        return ER.cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=coef_dev, rescale=rescale)
    if noise is None and coef_dev is None and coefs[5] != 0.0:
        raise ValueError("cfg_ddim_step_windows: sigma > 0 needs a noise tensor")
    g = float(coef_dev[0]) if coef_dev is not None else coefs[0]
    m, c = ring_blends(preds, sample, starts, weights, g)
    if rescale != 0.0:
        m = m * ER._factor(m, c, rescale)
    return ER._step_on(m, sample, noise, mode, coefs, coef_dev)


@contextlib.contextmanager
def patched_ring_kernels():
    from imagine360_amd import kernels
    saved = kernels.cfg_ddim_step_windows, kernels.cfg_rescale_factor_windows
    kernels.cfg_ddim_step_windows, kernels.cfg_rescale_factor_windows = cfg_ddim_step_windows, cfg_rescale_factor_windows
    try:
        yield
    finally:
        kernels.cfg_ddim_step_windows, kernels.cfg_rescale_factor_windows = saved
