"""Torch stand-in of ``kernels.free_init_noise`` (csrc/free_init.hip) for the CPU tier: the eager definition
``pano_geometry.free_init_noise`` evaluated in fp32 on the fp32-rounded operators, three sequential passes, which is what the kernel does
up to the order of its roundings.  ``patched_free_init_noise()`` yields the record of the calls made while the patch is active.  Also
here: what the CPU and the GPU tests of the kernel share -- the cases, their inputs, the fp64 reference (on the SAME fp32-rounded
matrices the kernel receives, as three sequential contractions: one four-operand einsum asks for 128 GiB at the workload's size) and the
per-element bound.

The bound, derived, not measured (u = 2^-24, the unit roundoff of fp32; first order in u, the constant 16 leaves room for the rest):

    |out - ref| <= (F + h + w + 16) u T / sb + u |ref|,      T = (|Lf| (x) |Lh| (x) |Lw|) M + M,      M = |sa x0| + |sb n1| + |n2|

  in front (3):  sa and sb reach the kernel rounded to fp32 (u |sa x0| + u |sb n1|), s = fl(sb n1 - n2) (u |s| <= u M), d = fl(sa x0 + s)
                 (u |d| <= u M): |d^ - d| <= 3 u M, and |d| <= M.
  the passes:    a dot product of n terms as one fma chain has |fl(sum l_j x_j) - sum l_j x_j| <= n u sum |l_j| |x_j|; three of them chained,
                 lengths w, h and F, on |d| <= M:  |y^ - L d^| <= (w + h + F) u (|Lf| (x) |Lh| (x) |Lw|) M.
  behind (4):    r = fl(y^ - d^) (u |y - d| <= u T); the errors of y^ and d^ enter r as they are, the 3 u M of d^ through L - I, at most 3 u T;
                 1 / sb reaches the kernel rounded to fp32 (u |r| / sb); out = fl(r / sb + n1) (u |out|, the last term).
  together:      (F + h + w) u |L| M + 3 u T + u T + u T, all over sb, plus u |ref|  <=  (F + h + w + 5) u T / sb + u |ref|.
The division by sb is what makes the bound hold near the clean end of the schedule: the filter's error is one of the NOISED CLIP, and the
effective noise is that clip's deviation over sb.  An implementation that forgets the division misses the bound several thousandfold
(tests/test_free_init.py perturbs the stand-in that way)."""
import contextlib
import functools

import torch

from imagine360_amd import pano_geometry as G

U = 2.0 ** -24
C = 4
SA, SB = 0.6, 0.8                       # every term matters
D_S, D_T = 0.25, 0.4                    # d_s != d_t

# (F, h, w): why
SHAPES = {
    "odd_scalar": (2, 3, 5),            # odd sizes: the scalar path
    "vector": (3, 4, 8),                # the 16-byte path
    "one_frame": (1, 4, 8),             # a one-element axis
    "one_row": (4, 1, 8),
    "frames_16": (16, 2, 8),            # each axis at the workload's length
    "rows_64": (2, 64, 8),
    "cols_128": (2, 2, 128),
    "frames_70": (70, 2, 8),            # each axis past 64 / 128 / 256: a second trip of whatever loop tiles it
    "rows_130": (5, 130, 8),
    "cols_300": (2, 2, 300),
    "square": (3, 8, 8),                # h == w: Lh and Lw can be swapped
}
RINGS = ("odd_scalar", "vector", "frames_16", "frames_70", "square")
# name -> (F, h, w, loop, d_s, d_t): every shape mirrored in time, five also as a ring, and the two extremes of the cut-off on one
CASES = {name: (*s, False, D_S, D_T) for name, s in SHAPES.items()}
CASES.update({name + "_ring": (*SHAPES[name], True, D_S, D_T) for name in RINGS})
CASES["vector_ring_near_mean"] = (*SHAPES["vector"], True, 0.05, 0.05)
CASES["vector_near_identity"] = (*SHAPES["vector"], False, 4.0, 4.0)


def operators(F, h, w, loop, d_s, d_t, kinds=None):
    """The three fp32 operators the kernel receives, (Lf, Lh, Lw): frames periodic iff ``loop``, rows mirrored, columns periodic.
    ``kinds`` overrides the three ``periodic`` flags."""
    pf, ph, pw = (bool(loop), False, True) if kinds is None else kinds
    return tuple(G.free_init_operator(n, d, per).to(torch.float32) for n, d, per in ((F, d_t, pf), (h, d_s, ph), (w, d_s, pw)))


def free_init_noise(x0, n1, n2, Lf, Lh, Lw, sa, sb):
    """The stand-in: fp32 arithmetic on fp32 operators, the result fp32 [1, F, C, h, w]."""
    assert x0.dim() == 5 and n1.dtype == n2.dtype == torch.float32 and all(L.dtype == torch.float32 for L in (Lf, Lh, Lw))
    assert tuple(Lf.shape) == (x0.shape[2],) * 2 and tuple(Lh.shape) == (x0.shape[3],) * 2 and tuple(Lw.shape) == (x0.shape[4],) * 2
    return G.free_init_noise(x0, n1, n2, float(sa), float(sb), Lf, Lh, Lw)


@contextlib.contextmanager
def patched_free_init_noise():
    """``kernels.free_init_noise`` is the stand-in; yields a list that gains (x0, n1, n2, Lf, Lh, Lw, sa, sb, result) of every call."""
    from imagine360_amd import kernels
    calls = []

    def recorded(x0, n1, n2, Lf, Lh, Lw, sa, sb):
        out = free_init_noise(x0, n1, n2, Lf, Lh, Lw, sa, sb)
        calls.append((x0, n1, n2, Lf, Lh, Lw, sa, sb, out))
        return out

    saved = getattr(kernels, "free_init_noise", None)
    kernels.free_init_noise = recorded
    try:
        yield calls
    finally:
        if saved is None:
            del kernels.free_init_noise
        else:
            kernels.free_init_noise = saved


@functools.lru_cache(maxsize=None)
def case(name, dt):
    """Host inputs of one case, computed once and never written to: x0 = 1.5 randn rounded to ``dt`` [1, C, F, h, w]; n1, n2 = randn,
    fp32 [1, F, C, h, w]; the three fp32 operators."""
    F, h, w, loop, d_s, d_t = CASES[name]
    g = torch.Generator().manual_seed(977 + sorted(CASES).index(name))
    x0 = (1.5 * torch.randn(1, C, F, h, w, generator=g)).to(dt)
    n1, n2 = torch.randn(1, F, C, h, w, generator=g), torch.randn(1, F, C, h, w, generator=g)
    return (x0, n1, n2) + operators(F, h, w, loop, d_s, d_t)


def _apply(Lf, Lh, Lw, v):
    """(Lf (x) Lh (x) Lw) v on [1, F, C, h, w], three sequential contractions."""
    v = torch.matmul(v, Lw.t())
    v = torch.matmul(Lh, v)
    return torch.einsum("ij,bjchw->bichw", Lf, v)


@functools.lru_cache(maxsize=None)
def reference(name, dt):
    """(ref, bound): the definition in fp64 on the case's inputs and fp32-rounded operators, and the per-element bound above."""
    x0, n1, n2, Lf, Lh, Lw = case(name, dt)
    F, h, w = CASES[name][:3]
    ref = G.free_init_noise(x0.double(), n1.double(), n2.double(), SA, SB, Lf, Lh, Lw)
    M = (SA * x0.double().permute(0, 2, 1, 3, 4)).abs() + (SB * n1.double()).abs() + n2.double().abs()
    T = _apply(Lf.double().abs(), Lh.double().abs(), Lw.double().abs(), M) + M
    return ref, (F + h + w + 16) * U * T / SB + U * ref.abs()


def worst_ratio(got, name, dt):
    """max |got - ref| / bound over the elements of one case (inf for a NaN or a wrong shape)."""
    ref, bound = reference(name, dt)
    got = got.detach().cpu()
    if got.shape != ref.shape or got.dtype != torch.float32 or not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got.double() - ref).abs() / bound).max())


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(view), b.view(view))
