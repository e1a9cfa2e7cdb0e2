"""Torch stand-in of ``kernels.keep_latents_release`` (csrc/keep_latents.hip, the RELEASE instantiation) for the CPU tier, to its
definition:

    known = T(fma(sa, x0, sb * noise))                                 ``_emu_keep_latents.known``: the expression of blend mode
    pano  = mask <= tau ? known : pano                                 the compare in fp32
    pers  = ok and mask at idx <= tau ? known at idx : pers

both latents updated in place; every element is a select, so the stand-in has the kernel's bits wherever ``known`` has them.
``patched_keep_release()`` yields the record of the calls made while the patch is active.  Also here: what the CPU and the GPU tests
of release mode share -- the strength map of a kernel case and the maps of the pipeline tests."""
import contextlib

import torch

from _emu_keep_latents import _at_views, keep_case, known


def keep_latents_release(pano, pers, x0, noise, mask, idx, ok, sqrt_a, sqrt_b, tau, coef_dev=None):
    _, C, F, h, w = pano.shape
    M, ph, pw = idx.shape
    assert x0.shape == pano.shape and x0.dtype == pano.dtype == pers.dtype and x0.data_ptr() != pano.data_ptr()
    assert tuple(noise.shape) == (1, F, C, h, w) and noise.dtype == torch.float32
    assert tuple(mask.shape) == (F, h, w) and mask.dtype == torch.float32
    assert idx.dtype == torch.int32 and ok.dtype == torch.uint8 and idx.shape == ok.shape
    assert tuple(pers.shape) == (1, M, C, F, ph, pw)
    if coef_dev is not None:
        assert coef_dev.numel() == 3 and coef_dev.dtype == torch.float32
        sqrt_a, sqrt_b, tau = (float(v) for v in coef_dev)
    k = known(x0, noise, sqrt_a, sqrt_b)
    tau32 = torch.tensor(tau, dtype=torch.float32)                                         # the kernel takes it as fp32
    kg = _at_views(k.reshape(C, F, h * w), idx).unsqueeze(0)                               # [1, M, C, F, ph, pw]
    pin = (mask <= tau32)
    pg = _at_views(pin.reshape(1, F, h * w), idx).unsqueeze(0) & ok.bool()[None, :, None, None]          # unseen: untouched
    pano.copy_(torch.where(pin[None, None], k, pano))
    pers.copy_(torch.where(pg, kg, pers))
    return pano, pers


@contextlib.contextmanager
def patched_keep_release():
    """``kernels.keep_latents_release`` is the stand-in; yields a list that gains (sqrt_a, sqrt_b, tau, pano.clone(), pers.clone()) of every
    call made inside.  On a tree without the wrapper the attribute is removed again on exit."""
    from imagine360_amd import kernels
    calls = []

    def recorded(pano, pers, x0, noise, mask, idx, ok, sqrt_a, sqrt_b, tau, coef_dev=None):
        out = keep_latents_release(pano, pers, x0, noise, mask, idx, ok, sqrt_a, sqrt_b, tau, coef_dev=coef_dev)
        calls.append((sqrt_a, sqrt_b, tau, pano.clone(), pers.clone()))
        return out

    saved = getattr(kernels, "keep_latents_release", None)
    kernels.keep_latents_release = recorded
    try:
        yield calls
    finally:
        if saved is None:
            del kernels.keep_latents_release
        else:
            kernels.keep_latents_release = saved


# ------------------------------------------------------------------------------------------------ shared by the CPU and the GPU tests
TAU = 0.4375                    # the threshold of the kernel cases: exactly representable, so is the value placed AT it


def release_case(F, C, h, w, M, ph, pw, dt, seed=7):
    """``keep_case`` with a strength map for the threshold ``TAU``: exact 0 and 1, values well below (<= TAU - 0.1), AT it (pinned: the
    compare is <=), and well above (>= TAU + 0.1) in every frame; pixels 0 and HW - 1, which idx is sure to hit, change their kind
    with the frame."""
    pano, pers, x0, noise, _, idx, ok = keep_case(F, C, h, w, M, ph, pw, dt, seed=seed)
    g = torch.Generator().manual_seed(seed + 2000)
    u, v = torch.rand(F, h * w, generator=g), torch.rand(F, h * w, generator=g)
    below, above = v * (TAU - 0.1), TAU + 0.1 + v * (1.0 - TAU - 0.1)
    s = torch.where(u < 0.2, torch.zeros(()), torch.where(u < 0.4, torch.ones(()), torch.where(u < 0.7, below, above)))
    kinds = (0.0, 1.0, TAU, TAU + 0.125)
    for f in range(F):
        s[f, 0], s[f, h * w - 1] = kinds[f % 4], kinds[(f + 1) % 4]
        s[f, 1], s[f, 2], s[f, 3], s[f, 4] = 0.0, 1.0, TAU, TAU - 0.125
    return pano, pers, x0, noise, s.reshape(F, h, w).contiguous(), idx, ok


def band_map(frames, H, W, n):
    """The strength map of the pipeline tests, [1, F, 1, H, W]: vertical bands of the values 0, 1 and ``(j + 1/2) / n`` for
    j = 0 .. n - 1 -- every value between two thresholds ``1 - (i + 1) / n`` and none on one; the bands are rolled by one from frame to
    frame, so the map differs between frames."""
    vals = [0.0, 1.0] + [(j + 0.5) / n for j in range(n)]
    bw = (W // 8) // len(vals) * 8                           # whole latent columns (stride 8); what is left over stays 1
    assert bw >= 8, (W, len(vals))
    m = torch.ones(1, frames, 1, H, W)
    for f in range(frames):
        for b, v in enumerate(vals):
            c0 = ((b + f) % len(vals)) * bw
            m[0, f, 0, :, c0:c0 + bw] = v
    return m
