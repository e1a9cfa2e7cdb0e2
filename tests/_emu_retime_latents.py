"""Torch stand-in of ``kernels.retime_pano_latent`` (csrc/retime_latents.hip) for the CPU tier: the eager definition
``pano_geometry.retime_pano_latent`` evaluated in fp32 (fp64 for an fp64 latent) with one rounding to the latent's dtype, which is what the
kernel does.  ``patched_retime_pano_latent()`` yields the record of the calls made while the patch is active.  Also here: what the CPU and
the GPU tests of the kernel share -- the cases, their inputs, the fp64 reference and (from ``_emu_resize_latents``, unchanged) the
per-element tolerance 0.5 ulp_T(ref) + 2^-17 max|x|: derived there for a two-pass sum of about 20 fp32 operations on terms of at most
1.9 max|x|; one four-tap pass (7 operations on terms of at most sum |w| max|x| = 1.25 max|x|) stays inside it a fortiori."""
import contextlib
import functools

import torch

from _emu_resize_latents import same_bits, worst_ratio  # noqa: F401  (shared with the tests that import this module)
from imagine360_amd import pano_geometry as G


def retime_pano_latent(x, F, mode="linear", loop=False):
    assert x.dim() == 5 and x.shape[0] == 1 and F >= x.shape[2] and mode in G.RETIME_MODES
    wide = x if x.dtype == torch.float64 else x.float()
    return G.retime_pano_latent(wide, F, mode, loop).to(x.dtype)


@contextlib.contextmanager
def patched_retime_pano_latent():
    """``kernels.retime_pano_latent`` is the stand-in; yields a list that gains (x, F, mode, loop, result) of every call made inside."""
    from imagine360_amd import kernels
    calls = []

    def recorded(x, F, mode="linear", loop=False):
        out = retime_pano_latent(x, F, mode, loop)
        calls.append((x, F, mode, loop, out))
        return out

    saved = getattr(kernels, "retime_pano_latent", None)
    kernels.retime_pano_latent = recorded
    try:
        yield calls
    finally:
        if saved is None:
            del kernels.retime_pano_latent
        else:
            kernels.retime_pano_latent = saved


# ------------------------------------------------------------------------------------------------ shared by the CPU and the GPU tests
C = 4
TILE = 4096                   # kRetimeTile of csrc/retime_latents.hip: plane elements per workgroup, 256 threads

# name -> (f, F, (h, w), loop): one case on each side of every choice the launcher and the kernel make
CASES = {
    "vector_keyframes": (2, 3, (4, 8), False),            # 16-byte path; frames 0 and 2 are keyframes, frame 1 a blend at t = 1/2
    "scalar_keyframes": (4, 7, (3, 5), False),            # hw = 15: scalar path; the even frames are keyframes
    "vector_ragged": (3, 8, (4, 8), False),               # 2 / 7: no interior keyframe
    "scalar_ragged": (5, 6, (3, 5), False),               # 4 / 5
    "ring_x2": (4, 8, (4, 8), True),                      # a ring, integer scale: frame 7 blends frames 3 and 0
    "ring_ragged": (3, 7, (3, 5), True),                  # a ring, 3 / 7: frame 0 the only keyframe
    "one_frame": (1, 4, (4, 8), False),                   # every clamped tap is the one frame
    "one_frame_ring": (1, 4, (4, 8), True),               # every wrapped tap is the one frame
    "identity": (4, 4, (4, 8), False),                    # equal frame counts: the input's bits
    "vector_two_tiles": (2, 3, (5, 1000), False),         # hw = 5000: two tiles, the second of 904 elements = 113 units
    "scalar_two_tiles": (2, 3, (3, 1399), False),         # hw = 4197, odd: two tiles, the second of 101 elements
    "vector_looped": (2, 4, (4, 640), True),              # hw = 2560: 320 units of eight in one tile, a thread takes a second unit
}
MODES = ("linear", "cubic")


@functools.lru_cache(maxsize=None)
def case(name, dt):
    """Host input ``1.5 randn`` rounded to ``dt``, [1, C, f, h, w], of one case (computed once, never written to)."""
    f, _, (h, w), _ = CASES[name]
    g = torch.Generator().manual_seed(211 + sorted(CASES).index(name))
    return (1.5 * torch.randn(1, C, f, h, w, generator=g)).to(dt)


@functools.lru_cache(maxsize=None)
def reference(name, dt, mode):
    """The eager definition in fp64 on the case's input."""
    _, F, _, loop = CASES[name]
    return G.retime_pano_latent(case(name, dt).double(), F, mode, loop)
