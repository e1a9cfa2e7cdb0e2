"""Torch stand-in of ``kernels.resize_pano_latent`` (csrc/resize_latents.hip) for the CPU tier: the eager definition
``pano_geometry.resize_pano_latent`` evaluated in fp32 (fp64 for an fp64 latent) with one rounding to the latent's dtype, which is what the
kernel does.  ``patched_resize_pano_latent()`` yields the record of the calls made while the patch is active.  Also here: what the CPU and
the GPU tests of the kernel share -- the cases, their inputs, the fp64 reference and the per-element tolerance."""
import contextlib
import functools

import torch

from imagine360_amd import pano_geometry as G


def resize_pano_latent(x, H, W, mode="bicubic"):
    assert x.dim() == 5 and x.shape[0] == 1 and H >= x.shape[3] and W >= x.shape[4] and mode in G.RESIZE_MODES
    wide = x if x.dtype == torch.float64 else x.float()
    return G.resize_pano_latent(wide, H, W, mode).to(x.dtype)


@contextlib.contextmanager
def patched_resize_pano_latent():
    """``kernels.resize_pano_latent`` is the stand-in; yields a list that gains (x, H, W, mode, result) of every call made inside."""
    from imagine360_amd import kernels
    calls = []

    def recorded(x, H, W, mode="bicubic"):
        out = resize_pano_latent(x, H, W, mode)
        calls.append((x, H, W, mode, out))
        return out

    saved = getattr(kernels, "resize_pano_latent", None)
    kernels.resize_pano_latent = recorded
    try:
        yield calls
    finally:
        if saved is None:
            del kernels.resize_pano_latent
        else:
            kernels.resize_pano_latent = saved


# ------------------------------------------------------------------------------------------------ shared by the CPU and the GPU tests
C, F = 4, 2
ROWS_PER_WORKGROUP = 8        # kResizeRows of csrc/resize_latents.hip

# (h, w) -> (H, W): one case on each side of every choice the launcher and the kernel make
CASES = {
    "vector_x2": ((4, 8), (8, 16)),                   # 16-byte stores, scale 2
    "vector_ragged_scale": ((6, 10), (8, 16)),        # 16-byte stores, scales 4/3 and 8/5
    "scalar_ragged": ((3, 5), (7, 11)),               # W % 8 != 0: scalar stores, scales 7/3 and 11/5
    "identity": ((4, 8), (4, 8)),                     # equal sizes: the input's bits
    "vector_three_tiles": ((5, 8), (19, 24)),         # three row tiles per plane, the last one of 3 rows; scale 3 along the columns
    "scalar_two_tiles_looped": ((5, 12), (11, 35)),   # scalar, two row tiles, 8 * 35 = 280 units: a thread takes a second unit
    "vector_looped": ((2, 130), (9, 264)),            # 8 * 264 / 8 = 264 units of eight columns: a thread takes a second unit
    "one_pixel": ((1, 1), (2, 3)),                    # every wrapped and clamped tap is the one pixel
}
MODES = ("bilinear", "bicubic")

MANTISSA = {torch.bfloat16: 7, torch.float16: 10}
MIN_EXPONENT = {torch.bfloat16: -126, torch.float16: -14}


def ulp(ref, dt):
    """The spacing of ``dt`` at every element of the fp64 tensor ``ref`` (of the smallest normal binade at and below it)."""
    _, e = torch.frexp(ref.abs())                                       # |ref| = m 2^e, 0.5 <= m < 1
    e = torch.where(ref == 0, torch.full_like(e, MIN_EXPONENT[dt]), (e - 1).clamp_min(MIN_EXPONENT[dt]))
    return torch.ldexp(torch.ones_like(ref), e - MANTISSA[dt])


def tolerance(ref, x, dt):
    """Per element: half an ulp of ``dt`` at the reference for the one rounding at the store, plus 2^-17 max|x| for about 20 fp32
    operations on terms of at most (sum |w|)^2 max|x| ~ 1.9 max|x| (and t rounded to fp32), with margin."""
    return 0.5 * ulp(ref, dt) + 2.0 ** -17 * float(x.abs().max())


def worst_ratio(got, ref, x, dt):
    """max over the elements of |got - ref| / tolerance: below 1 passes."""
    return float(((got.double().cpu() - ref).abs() / tolerance(ref, x.double().cpu(), dt)).max())


@functools.lru_cache(maxsize=None)
def case(name, dt):
    """Host input ``1.5 randn`` rounded to ``dt``, [1, C, F, h, w], of one case (computed once, never written to)."""
    (h, w), _ = CASES[name]
    g = torch.Generator().manual_seed(101 + sorted(CASES).index(name))
    return (1.5 * torch.randn(1, C, F, h, w, generator=g)).to(dt)


@functools.lru_cache(maxsize=None)
def reference(name, dt, mode):
    """The eager definition in fp64 on the case's input."""
    _, (H, W) = CASES[name]
    return G.resize_pano_latent(case(name, dt).double(), H, W, mode)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
