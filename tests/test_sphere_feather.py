"""The spherical feather of a ``regenerate_mask`` on CPU: ``pano_geometry.pixel_directions``, the eager ``sphere_distance2`` against a
direct fp64 great-circle computation, its behaviour at the +-180 degree seam and at a pole (where a distance counted in columns is
wrong), and ``feather_pano_mask``."""
import math

import pytest
import torch

from _emu_sphere_distance import BOUND, great_circle
from imagine360_amd import pano_geometry as G

torch.set_grad_enabled(False)


def angle(d2):
    return 2.0 * torch.asin((d2.double().sqrt() / 2.0).clamp(max=1.0))


def random_keep(F, h, w, seed, p=0.15):
    return (torch.rand(F, h, w, generator=torch.Generator().manual_seed(seed)) < p).to(torch.uint8)


@pytest.mark.parametrize("h,w", [(6, 12), (5, 13), (16, 32)])
def test_pixel_directions(h, w):
    n64, n32 = G.pixel_directions(h, w, torch.float64), G.pixel_directions(h, w)
    assert n64.shape == n32.shape == (h * w, 3) and n32.dtype == torch.float32 and n32.is_contiguous()
    assert (n64.norm(dim=1) - 1).abs().max() < 4e-16 and (n32.double().norm(dim=1) - 1).abs().max() < 2.0 ** -23
    assert torch.equal(n32, n64.float())                                               # fp64 on the host, rounded once
    # the stated angles: row 0 is half a row below the north pole, column 0 half a column east of -180 degrees; row-major order
    lat0, lon0 = math.pi / 2 - 0.5 / h * math.pi, 0.5 / w * 2 * math.pi - math.pi
    want = torch.tensor([math.cos(lat0) * math.cos(lon0), math.cos(lat0) * math.sin(lon0), math.sin(lat0)], dtype=torch.float64)
    assert (n64[0] - want).abs().max() < 1e-15
    assert torch.allclose(n64[w][2], torch.tensor(math.sin(math.pi / 2 - 1.5 / h * math.pi), dtype=torch.float64), atol=1e-15)
    assert torch.allclose(n64.reshape(h, w, 3)[:, :, 2], n64.reshape(h, w, 3)[:, :1, 2].expand(h, w))          # z is the row's alone


@pytest.mark.parametrize("F,h,w", [(2, 6, 12), (2, 5, 13), (3, 16, 32)])
def test_eager_distance_is_the_great_circle_distance(F, h, w):
    keep = random_keep(F, h, w, seed=h * w)
    ref = great_circle(h, w, keep)                                                     # from longitude and latitude, no vectors
    got64 = angle(G.sphere_distance2(keep, G.pixel_directions(h, w, torch.float64)))
    assert got64.shape == (F, h, w) and (got64 - ref).abs().max() < 1e-9               # (asin near 0 and near 1 loses digits)
    d32 = G.sphere_distance2(keep, G.pixel_directions(h, w))
    assert d32.dtype == torch.float32 and (angle(d32) - ref).abs().max() < 2e-6        # the fp32 table moves a vector by 2^-24
    assert (d32[keep.bool()] == 0).all() and (d32[~keep.bool()] > 0).all()
    # chunked: the same numbers however the pixels are cut
    assert torch.equal(G.sphere_distance2(keep, G.pixel_directions(h, w), chunk_elems=7), d32)
    with pytest.raises(ValueError, match="dirs must be"):
        G.sphere_distance2(keep, G.pixel_directions(h, w + 1))


def test_distance_crosses_the_seam():
    """A kept block at columns 0-1: column w - 1 lies as near to it (across the seam) as column 2 does; a distance in columns would
    put it w - 2 columns away."""
    h, w = 6, 12
    keep = torch.zeros(1, h, w, dtype=torch.uint8)
    keep[0, 2:4, 0:2] = 1
    d2 = G.sphere_distance2(keep, G.pixel_directions(h, w))[0]
    for y in range(h):
        a, b = float(d2[y, w - 1]), float(d2[y, 2])
        print(f"seam row {y}: d2[w - 1] = {a:.9g}, d2[2] = {b:.9g}, |a - b| / b / bound = {abs(a - b) / b / BOUND:.3f}")
        assert abs(a - b) <= BOUND * b, (y, a, b)
    theta = angle(d2)
    y = 2
    one_column = 2 * math.pi / w * math.cos(math.pi / 2 - (y + 0.5) / h * math.pi)      # the arc of one column along row y's parallel
    assert float(theta[y, w - 1]) <= one_column + 1e-6                                 # (the great circle is a little shorter than the parallel)
    planar = (w - 2) * one_column                                                      # what w - 2 columns would be
    assert float(theta[y, w - 1]) < 0.2 * planar
    ref = great_circle(h, w, keep)[0]
    assert abs(float(theta[y, w - 1]) - float(ref[y, w - 1])) < 2e-6


def test_distance_goes_over_the_pole():
    """A kept pixel in row 0: the opposite column of row 0 is 2 * (pi / 2h) away, over the pole -- not w / 2 columns."""
    h, w = 8, 16
    keep = torch.zeros(1, h, w, dtype=torch.uint8)
    keep[0, 0, 3] = 1
    theta = angle(G.sphere_distance2(keep, G.pixel_directions(h, w))[0])
    over_the_pole = 2 * (math.pi / (2 * h))
    assert abs(float(theta[0, 3 + w // 2]) - over_the_pole) < 2e-6
    along_the_row = (w // 2) * 2 * math.pi / w                                         # w / 2 columns are half a turn of longitude
    assert along_the_row > 7 * over_the_pole
    # every pixel of row 0 is within that arc of the kept one, whatever its column
    assert float(theta[0].max()) <= over_the_pole + 2e-6


def test_a_frame_without_kept_pixels_gives_an_all_ones_ramp():
    h, w = 6, 12
    keep = torch.zeros(2, h, w, dtype=torch.uint8)
    keep[1, 1, 1] = 1
    d2 = G.sphere_distance2(keep, G.pixel_directions(h, w))
    assert torch.isinf(d2[0]).all() and (d2[0] > 0).all() and torch.isfinite(d2[1]).all()
    for deg in (5.0, 90.0, 300.0):
        assert torch.equal(G.feather_ramp(d2, deg)[0], torch.ones(h, w))
    m = torch.ones(2, h, w)
    m[1, 1, 1] = 0
    assert torch.equal(G.feather_pano_mask(m, 30.0)[0], torch.ones(h, w))


@pytest.mark.parametrize("h,w,deg", [(16, 32, 40.0), (12, 24, 25.0)])
def test_feather_pano_mask(h, w, deg):
    m = torch.ones(2, h, w)
    m[0, h // 4:h // 2, :3] = 0                                                         # touches the seam
    m[0, h // 4:h // 2, -2:] = 0
    m[1, 0, 5] = 0                                                                     # at a pole
    out = G.feather_pano_mask(m, deg)
    assert out.shape == m.shape and out.dtype == m.dtype
    ref = great_circle(h, w, m <= 0)
    Theta = math.radians(deg)
    assert (out[m <= 0] == 0).all()                                                    # 0 on the kept set
    assert (out[ref > Theta + 1e-5] == 1).all() and (ref > Theta + 1e-5).any()         # 1 beyond Theta
    inside = (ref > 0) & (ref < Theta - 1e-5)
    assert inside.any() and ((out[inside] > 0) & (out[inside] < 1)).all()
    assert (out.double() - (ref / Theta).clamp(0, 1)).abs().max() < 1e-5               # the linear ramp in the angle
    for f in range(2):                                                                 # monotone in the angle
        order = ref[f].flatten().argsort()
        ramp = out[f].flatten()[order]
        assert (ramp[1:] - ramp[:-1]).min() > -1e-5
    # a fractional input is only ever lowered: min(m, ramp)
    frac = m.clone()
    frac[m > 0] = 0.3
    frac[1, h // 2:, :] = 0.8
    got = G.feather_pano_mask(frac, deg)
    assert torch.equal(got, torch.minimum(frac, out)) and (got == 0.3).any() and (got == 0.8).any() and ((got > 0) & (got < 0.3)).any()
    # 0 degrees is the mask; bad values are refused
    assert G.feather_pano_mask(frac, 0.0) is frac
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="degrees must be finite and >= 0"):
            G.feather_pano_mask(frac, bad)
    with pytest.raises(ValueError, match=r"mask must be \[F, h, w\]"):
        G.feather_pano_mask(frac[0], deg)
