"""Torch stand-in of ``kernels.keep_latents`` (csrc/keep_latents.hip) for the CPU tier, to its definition:

    known = T(fma(sa, x0, sb * noise))                                 sb * noise rounded to fp32, then one rounding of the sum
    pano  = blend(pano, known, mask)
    pers  = ok ? blend(pers, known at idx, mask at idx) : pers
    blend(x, k, w):  w >= 1 -> x;  w <= 0 -> k;  else T(fma(w, x - k, k))     x - k rounded to fp32, then one rounding of the sum

both latents updated in place.  torch has no fused multiply-add on the CPU, so an fma's exact product and sum are formed in fp64 (the
product of two fp32 numbers is exact there) and rounded to fp32: the fma's bits except where the fp64 sum lands within 2^-29 of an
fp32 tie -- never at the two exact ends of ``blend``, which are selects.  ``patched_keep_latents()`` yields the record of the calls made
while the patch is active.  Also here: what the CPU and the GPU tests of ``keep_latents`` share -- the inputs of a case, the fp64
composition built from ``scheduler.add_noise`` they are judged against, and the masks of the pipeline tests."""
import contextlib

import torch

from _emu_noise_latents import noise_case


def _fma(a, b, c):
    """fp32 fma(a, b, c) through fp64 (see the module's docstring)."""
    return (a.double() * b.double() + c.double()).float()


def _at_views(plane, idx):
    """[..., F, HW]-like ``plane`` [A, F, HW] gathered at the clamped table -> [M, A, F, ph, pw]."""
    A, F, HW = plane.shape
    g = plane[..., idx.reshape(-1).long().clamp(0, HW - 1)].reshape(A, F, *idx.shape)
    return g.permute(2, 0, 1, 3, 4)


def blend(x, k, w):
    """``blend`` of the definition on tensors that broadcast; x and k of one dtype, w fp32."""
    mixed = _fma(w, x.float() - k.float(), k.float()).to(x.dtype)
    return torch.where(w >= 1, x, torch.where(w <= 0, k, mixed))


def known(x0, noise, sqrt_a, sqrt_b):
    sa, sb = torch.tensor(sqrt_a, dtype=torch.float32), torch.tensor(sqrt_b, dtype=torch.float32)      # the kernel takes them as fp32
    return _fma(sa, x0.float(), sb * noise.permute(0, 2, 1, 3, 4)).to(x0.dtype)


def keep_latents(pano, pers, x0, noise, mask, idx, ok, sqrt_a, sqrt_b, coef_dev=None):
    _, C, F, h, w = pano.shape
    M, ph, pw = idx.shape
    assert x0.shape == pano.shape and x0.dtype == pano.dtype == pers.dtype and x0.data_ptr() != pano.data_ptr()
    assert tuple(noise.shape) == (1, F, C, h, w) and noise.dtype == torch.float32
    assert tuple(mask.shape) == (F, h, w) and mask.dtype == torch.float32
    assert idx.dtype == torch.int32 and ok.dtype == torch.uint8 and idx.shape == ok.shape
    assert tuple(pers.shape) == (1, M, C, F, ph, pw)
    if coef_dev is not None:
        sqrt_a, sqrt_b = (float(v) for v in coef_dev)
    k = known(x0, noise, sqrt_a, sqrt_b)
    kg = _at_views(k.reshape(C, F, h * w), idx).unsqueeze(0)                               # [1, M, C, F, ph, pw]
    wg = _at_views(mask.reshape(1, F, h * w), idx).unsqueeze(0)                            # [1, M, 1, F, ph, pw]
    wg = torch.where(ok.bool()[None, :, None, None], wg, torch.ones((), dtype=wg.dtype, device=wg.device))      # unseen: untouched
    pano.copy_(blend(pano, k, mask[None, None]))
    pers.copy_(blend(pers, kg, wg))
    return pano, pers


@contextlib.contextmanager
def patched_keep_latents():
    """``kernels.keep_latents`` is the stand-in; yields a list that gains (sqrt_a, sqrt_b, pano.clone()) of every call made inside."""
    from imagine360_amd import kernels
    calls = []

    def recorded(pano, pers, x0, noise, mask, idx, ok, sqrt_a, sqrt_b, coef_dev=None):
        out = keep_latents(pano, pers, x0, noise, mask, idx, ok, sqrt_a, sqrt_b, coef_dev=coef_dev)
        calls.append((sqrt_a, sqrt_b, pano.clone()))
        return out

    saved = getattr(kernels, "keep_latents", None)
    kernels.keep_latents = recorded
    try:
        yield calls
    finally:
        if saved is None:
            del kernels.keep_latents
        else:
            kernels.keep_latents = saved


# ------------------------------------------------------------------------------------------------ shared by the CPU and the GPU tests
def keep_case(F, C, h, w, M, ph, pw, dt, seed=7):
    """Inputs of ``keep_latents``: ``noise_case``'s x0 / noise / tables (idx holds 0, HW - 1 and repeats, ok holds zeros), two latents
    to blend into, and a mask that holds 0.0, 1.0 and fractional values in every frame and differs from frame to frame (pixels 0 and
    HW - 1, which idx is sure to hit, change their kind with the frame)."""
    x0, noise, idx, ok = noise_case(F, C, h, w, M, ph, pw, dt, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    pano = torch.randn(1, C, F, h, w, generator=g).to(dt)
    pers = torch.randn(1, M, C, F, ph, pw, generator=g).to(dt)
    u = torch.rand(F, h * w, generator=g)
    mask = torch.where(u < 0.3, torch.zeros(()), torch.where(u < 0.6, torch.ones(()), torch.rand(F, h * w, generator=g)))
    kinds = (0.0, 1.0, 0.375)
    for f in range(F):
        mask[f, 0], mask[f, h * w - 1] = kinds[f % 3], kinds[(f + 1) % 3]
        mask[f, 1], mask[f, 2], mask[f, 3] = 0.0, 1.0, 0.25 + 0.5 * f / F
    return pano, pers, x0, noise, mask.reshape(F, h, w).contiguous(), idx, ok


def mask_at_views(mask, idx, ok):
    """The mask value every perspective element is blended with, [1, M, 1, F, ph, pw]; 1 (untouched) where ``ok`` is 0."""
    F, h, w = mask.shape
    wg = _at_views(mask.reshape(1, F, h * w), idx).unsqueeze(0)
    return torch.where(ok.bool()[None, :, None, None], wg, torch.ones((), dtype=wg.dtype, device=wg.device))


def fp64_composition(sch, t, pano, pers, x0, noise, mask, idx, ok):
    """``scheduler.add_noise`` in fp64 at timestep ``t`` (None: the clean clip, coefficients (1, 0)), the gather, and the two linear
    blends ``known + w (x - known)`` in fp64; perspective elements no view of the panorama reaches stay."""
    _, C, F, h, w = x0.shape
    x0, noise, mask, idx, ok = x0.double().cpu(), noise.double().cpu(), mask.double().cpu(), idx.cpu(), ok.cpu()
    k = x0 if t is None else sch.add_noise(x0, noise.permute(0, 2, 1, 3, 4), torch.tensor([t]))
    kg = _at_views(k.reshape(C, F, h * w), idx).unsqueeze(0)
    wg = mask_at_views(mask, idx, ok)
    return k + mask[None, None] * (pano.double().cpu() - k), kg + wg * (pers.double().cpu() - kg)


def half_mask(frames, H, W):
    """The mask of the pipeline tests, [1, F, 1, H, W] (1: regenerate): on even frames the left half of the columns is kept, on odd
    frames a rectangle that crosses the seam (the middle rows, the last and the first eighth of the columns)."""
    m = torch.ones(1, frames, 1, H, W)
    m[:, 0::2, :, :, :W // 2] = 0.0
    m[:, 1::2, :, H // 4:3 * H // 4, 7 * W // 8:] = 0.0
    m[:, 1::2, :, H // 4:3 * H // 4, :W // 8] = 0.0
    return m


def kept(mask, h, w):
    """bool [1, 1, F, h, w]: the latent pixels ``half_mask`` keeps (nearest resize: the mask's blocks are multiples of the stride)."""
    m = torch.nn.functional.interpolate(mask.transpose(2, 1), size=(mask.shape[1], h, w))
    return m == 0
