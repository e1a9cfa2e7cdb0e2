"""Equirectangular <-> perspective geometry of the cross-view attention, computed once per
(resolution, camera rig) and cached on the device.

The reference rebuilds all of this on every WarpAttn call -- 7x per denoising step -- through dense
one-hot images of shape (views, pixels, H, W) pushed through kornia ``remap``
(src/utils/utils.py:12-164; src/utils/Perspective_and_Equirectangular/{e2p,p2e}.py).  A remapped
one-hot image is just the bilinear footprint of one sample point, so here the footprints are scattered
directly into the (views, equi-pixel, pers-pixel) correspondence matrix: same numbers, no 20 x N^2
intermediates, and the result is step-invariant so it is built once.  Only the reference's
``random.random() < 0.4`` coin (utils.py:15) stays per call.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------- reference API helpers
def pad_pano(pano, padding):
    """Circular pad of the last axis of a (b c h w) / (b m c h w) / (b c f h w) tensor (src/utils/pano.py:75-95)."""
    if padding <= 0:
        return pano
    return torch.cat([pano[..., -padding:], pano, pano[..., :padding]], dim=-1)


def unpad_pano(pano_pad, padding):
    """src/utils/pano.py:98-101."""
    return pano_pad if padding <= 0 else pano_pad[..., padding:-padding]


# ------------------------------------------------------------------------------- camera maps (host, fp64)
def _axis_angle(v):
    v = np.asarray(v, np.float64).reshape(3)
    th = float(np.linalg.norm(v))
    if th < 1e-15:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def _rotations(theta, phi):
    """Yaw about z then pitch about the rotated y axis (e2p.py:23-26, p2e.py:23-26)."""
    R1 = _axis_angle(np.array([0.0, 0.0, 1.0]) * np.radians(theta))
    R2 = _axis_angle((R1 @ np.array([0.0, 1.0, 0.0])) * np.radians(-phi))
    return R1, R2


def perspective_lonlat(fov, theta, phi, h, w):
    """(lon, lat) in radians of every pixel of a gnomonic view (e2p.py:9-40)."""
    hfov = float(h) / w * fov
    w_len, h_len = np.tan(np.radians(fov / 2.0)), np.tan(np.radians(hfov / 2.0))
    ys = np.tile(np.linspace(-w_len, w_len, w), [h, 1])
    zs = -np.tile(np.linspace(-h_len, h_len, h), [w, 1]).T
    xs = np.ones([h, w], np.float32)
    d = np.sqrt(xs ** 2 + ys ** 2 + zs ** 2)
    rays = (np.stack((xs, ys, zs), axis=2) / d[:, :, None]).reshape(h * w, 3).T
    R1, R2 = _rotations(theta, phi)
    rays = (R2 @ (R1 @ rays)).T
    return np.arctan2(rays[:, 1], rays[:, 0]).reshape(h, w), -np.arcsin(rays[:, 2]).reshape(h, w)


def perspective_sample_points(eh, ew, fov, theta, phi, h, w):
    """Equirect pixel coordinates (x, y) hit by every perspective pixel (e2p.py:43-56)."""
    lon, lat = perspective_lonlat(fov, theta, phi, h, w)
    cx, cy = (ew - 1) / 2.0, (eh - 1) / 2.0
    return np.degrees(lon) / 180 * cx + cx, np.degrees(lat) / 90 * cy + cy


def equirect_sample_points(ph, pw, fov, theta, phi, h, w):
    """Perspective pixel coordinates (x, y) hit by every equirect pixel, and their validity (p2e.py:9-53)."""
    hfov = float(ph) / pw * fov
    w_len, h_len = np.tan(np.radians(fov / 2.0)), np.tan(np.radians(hfov / 2.0))
    lon, lat = np.meshgrid(np.linspace(-180, 180, w), np.linspace(90, -90, h))
    rays = np.stack((np.cos(np.radians(lon)) * np.cos(np.radians(lat)), np.sin(np.radians(lon)) * np.cos(np.radians(lat)),
                     np.sin(np.radians(lat))), axis=2)
    R1, R2 = _rotations(theta, phi)
    rays = (np.linalg.inv(R1) @ (np.linalg.inv(R2) @ rays.reshape(h * w, 3).T)).T.reshape(h, w, 3)
    front = rays[:, :, 0] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rays = rays / rays[:, :, 0:1]
    inside = (-w_len < rays[:, :, 1]) & (rays[:, :, 1] < w_len) & (-h_len < rays[:, :, 2]) & (rays[:, :, 2] < h_len)
    x = np.where(inside, (rays[:, :, 1] + w_len) / 2 / w_len * pw, 0)
    y = np.where(inside, (-rays[:, :, 2] + h_len) / 2 / h_len * ph, 0)
    return x, y, inside & front


def camera_lists(cameras):
    """FoV/theta/phi of the rig as Python floats; accepts [m] or [1, m] tensors / arrays."""
    if "_lists" in cameras:
        return cameras["_lists"]
    out = []
    for k in ("FoV", "theta", "phi"):
        v = cameras[k]
        v = v.detach().cpu().reshape(-1).tolist() if torch.is_tensor(v) else np.asarray(v).reshape(-1).tolist()
        out.append([float(x) for x in v])
    m = min(len(v) for v in out)
    return [v[:m] for v in out]


# ------------------------------------------------------------------------------- bilinear footprints
def _footprint(points_x, points_y, H, W, valid=None):
    """Dense [P, H*W] matrix whose row p holds the bilinear weights of sample point p on an H x W grid with
    zero padding (== kornia remap(align_corners=True) / grid_sample of one-hot images)."""
    x = torch.as_tensor(points_x, dtype=torch.float32).reshape(-1)
    y = torch.as_tensor(points_y, dtype=torch.float32).reshape(-1)
    # grid_sample's normalise / unnormalise round trip in fp32
    x = ((2.0 * x / (W - 1) - 1.0) + 1.0) / 2.0 * (W - 1)
    y = ((2.0 * y / (H - 1) - 1.0) + 1.0) / 2.0 * (H - 1)
    x0, y0 = torch.floor(x), torch.floor(y)
    out = torch.zeros(x.numel(), H * W, dtype=torch.float32)
    rows = torch.arange(x.numel())
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wgt = (1 - (x - xi).abs()) * (1 - (y - yi).abs())
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            if valid is not None:
                ok = ok & torch.as_tensor(valid).reshape(-1)
            idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long()
            out.index_put_((rows[ok], idx[ok]), wgt[ok], accumulate=True)
    return out


def _gauss5(device):
    x = torch.arange(5, dtype=torch.float64) - 2.0
    g = torch.exp(-(x ** 2) / 2.0)
    return (g / g.sum()).float().to(device)


def _blur5(x, circular_w):
    """5x5 sigma=1 Gaussian; replicate borders, or circular along W (pad_pano(2) around the blur, utils.py:26-29)."""
    g = _gauss5(x.device)
    if circular_w:
        x = torch.cat([x[..., -2:], x, x[..., :2]], dim=-1)
        x = F.pad(x, (0, 0, 2, 2), mode="replicate")
    else:
        x = F.pad(x, (2, 2, 2, 2), mode="replicate")
    # separable 5-tap filter as shifted weighted sums (plain elementwise kernels; a conv2d call here would go
    # through MIOpen's im2col path once per (view, pixel) image)
    w = x.shape[-1] - 4
    x = sum(g[i] * x[..., i:i + w] for i in range(5))
    h = x.shape[-2] - 4
    return sum(g[i] * x[..., i:i + h, :] for i in range(5))


def _row_normalise(t):
    mx = torch.amax(t, dim=(1, 2, 3), keepdim=True)
    mx = torch.where(mx == 0, torch.ones_like(mx), mx)
    return t / mx * 2 - 1


def cross_view_bias(ph, pw, eh, ew, cameras, opposite, device="cpu", chunk=4):
    """Additive attention biases of one WarpAttn resolution (get_merged_masks, src/utils/utils.py:12-41).

    Returns fp32 ``bias_e2p`` [eh*ew, m*ph*pw] (equirect queries over the keys of all views, ordered
    (m, h, w)) and ``bias_p2e`` [m*ph*pw, eh*ew], values in [-1, 1].  ``opposite`` selects the antipodal
    variant (get_oppo_masks, utils.py:91-142: source columns shifted by W/2, cameras yawed 180 degrees)."""
    fov, theta, phi = camera_lists(cameras)
    m, ne, npx = len(fov), eh * ew, ph * pw
    A = torch.empty(m, ne, npx, device=device)            # e2p: weight of equi pixel e at the sample point of (m, p)
    B = torch.empty(m, npx, ne, device=device)            # p2e: weight of pers pixel p at the sample point of (m, e)
    shift = torch.arange(ne).reshape(eh, ew).roll(-(ew // 2), dims=1).reshape(-1) if opposite else None
    for i in range(m):
        px, py = perspective_sample_points(eh, ew, fov[i], theta[i], phi[i], ph, pw)
        fp = _footprint(px, py, eh, ew).t()                # [ne, npx] indexed by the pixel that is HIT
        if opposite:
            fp = fp[shift]                                 # source e lights the antipodal pixel opp(e)
        A[i] = fp.to(device)
        ex, ey, ok = equirect_sample_points(ph, pw, fov[i], theta[i] + (180 if opposite else 0), phi[i], eh, ew)
        B[i] = _footprint(ex, ey, ph, pw, valid=ok).t().to(device)
    # "fix missing pixels" symmetrisation (utils.py:79-87)
    pers_masks = torch.clamp(A + B.transpose(1, 2), 0, 1)                    # [m, ne, npx]
    equi_masks = torch.clamp(B + pers_masks.transpose(1, 2), 0, 1)           # [m, npx, ne]
    del A, B
    pm = torch.empty_like(pers_masks)
    em = torch.empty_like(equi_masks)
    for i in range(0, m, chunk):                                             # blur + per-source max-normalise
        pm[i:i + chunk] = _row_normalise(_blur5(pers_masks[i:i + chunk].reshape(-1, 1, ph, pw), False)).reshape(-1, ne, npx)
        em[i:i + chunk] = _row_normalise(_blur5(equi_masks[i:i + chunk].reshape(-1, 1, eh, ew), True)).reshape(-1, npx, ne)
    bias_e2p = pm.permute(1, 0, 2).reshape(ne, m * npx).contiguous()
    bias_p2e = em.reshape(m * npx, ne).contiguous()
    return bias_e2p, bias_p2e


def spherical_coords(ph, pw, eh, ew, cameras):
    """(lon, lat) of every pixel: pers [m, ph, pw, 2], equi [eh, ew, 2], fp32 (get_coords, utils.py:145-164)."""
    lon, lat = np.meshgrid(np.linspace(-np.pi, np.pi, ew), np.linspace(np.pi / 2, -np.pi / 2, eh))
    equi = torch.tensor(np.stack([lon, lat], axis=-1), dtype=torch.float32)
    fov, theta, phi = camera_lists(cameras)
    pers = [torch.tensor(np.stack(perspective_lonlat(f, t, p, ph, pw), axis=-1), dtype=torch.float32)
            for f, t, p in zip(fov, theta, phi)]
    return torch.stack(pers), equi


def nearest_e2p_index(eh, ew, ph, pw, cameras):
    """Per view, the flat equirect index each perspective pixel copies under nearest-neighbour E2P and a
    validity flag (init_noise, pipeline_animation_inference_dual.py:361-387).  Uses the same fp32
    normalise -> grid_sample(nearest) arithmetic as kornia.remap so ties resolve identically."""
    fov, theta, phi = camera_lists(cameras)
    idx_img = torch.arange(eh * ew, dtype=torch.float32).reshape(1, 1, eh, ew)
    one_img = torch.ones(1, 1, eh, ew)
    idx, ok = [], []
    for f, t, p in zip(fov, theta, phi):
        x, y = perspective_sample_points(eh, ew, f, t, p, ph, pw)
        gx = 2.0 * torch.as_tensor(x, dtype=torch.float32) / (ew - 1) - 1.0
        gy = 2.0 * torch.as_tensor(y, dtype=torch.float32) / (eh - 1) - 1.0
        grid = torch.stack([gx, gy], dim=-1)[None]
        idx.append(F.grid_sample(idx_img, grid, mode="nearest", padding_mode="zeros", align_corners=True)[0, 0].long())
        ok.append(F.grid_sample(one_img, grid, mode="nearest", padding_mode="zeros", align_corners=True)[0, 0] > 0.5)
    return torch.stack(idx), torch.stack(ok)


# ------------------------------------------------------------------------------- resampling a panorama latent
RESIZE_MODES = ("bilinear", "bicubic")


def _tap_weights(t, cubic):
    """Weights [taps, ...] of a sample at fraction ``t`` in [0, 1) behind tap i0: linear, taps i0, i0 + 1 with (1 - t, t); cubic, taps
    i0 - 1 .. i0 + 2 with the Keys kernel, A = -0.75.  Shared by the spatial resize and the retiming."""
    if not cubic:
        return torch.stack([1 - t, t])
    A = -0.75                                            # torch's upsample_bicubic2d: cubic_convolution1 / cubic_convolution2
    near = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    far = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return torch.stack([far(t + 1), near(t), near(1 - t), far(2 - t)])


def _resize_taps(n_in, n_out, mode, dtype, device):
    """Taps of the ``n_out`` samples of an axis of ``n_in``: (first tap [n_out] int64, unwrapped and unclamped; weights [taps, n_out]).
    Half-pixel centres from integers: sample ``o`` sits at ((2 o + 1) n_in - n_out) / (2 n_out) = i0 + t, 0 <= t < 1; no float
    coordinate accumulates, and t is periodic in ``o`` for every integer scale."""
    o = torch.arange(n_out, dtype=torch.int64, device=device)
    num = (2 * o + 1) * n_in - n_out
    i0 = torch.div(num, 2 * n_out, rounding_mode="floor")
    t = (num - i0 * 2 * n_out).to(dtype) / (2 * n_out)
    return (i0, _tap_weights(t, False)) if mode == "bilinear" else (i0 - 1, _tap_weights(t, True))


def resize_pano_latent(x, H, W, mode="bicubic"):
    """``x`` [..., h, w] -> [..., H, W], ``H >= h`` and ``W >= w``: a panorama latent upscaled as the equirectangular image it is.  The
    eager definition of ``kernels.resize_pano_latent``, in torch ops on any device, blending in ``x``'s dtype (the weights are
    formed in float32 for a 16-bit ``x``).  Half-pixel centres (``align_corners=False``) from integer coordinates; "bilinear": taps
    i0, i0 + 1 with weights (1 - t, t); "bicubic": taps i0 - 1 .. i0 + 2, Keys kernel with A = -0.75.  Longitude wraps (column taps
    mod w: no seam at +-180 degrees), latitude clamps (row taps in [0, h - 1]).  Horizontal pass, then vertical; a sum is
    w0 a0 + w1 a1 + ... in this order.  Equal sizes return the input's values: t = 0, weights exactly (0, 1, 0, 0)."""
    if mode not in RESIZE_MODES:
        raise ValueError(f"resize_pano_latent: mode must be one of {sorted(RESIZE_MODES)}, got {mode!r}")
    h, w = x.shape[-2:]
    if H < h or W < w:
        raise ValueError(f"resize_pano_latent: {h} x {w} -> {H} x {W} shrinks (there is no antialiasing filter; H >= h and W >= w)")
    wdt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32

    def blend(taps, weights):
        acc = weights[0] * taps[0]
        for wk, a in zip(weights[1:], taps[1:]):
            acc = acc + wk * a
        return acc

    c0, wx = _resize_taps(w, W, mode, wdt, x.device)
    wx = wx.to(x.dtype)
    x = blend([x[..., (c0 + j) % w] for j in range(wx.shape[0])], wx)                                     # [..., h, W]
    r0, wy = _resize_taps(h, H, mode, wdt, x.device)
    wy = wy.to(x.dtype)[:, :, None]
    return blend([x[..., (r0 + k).clamp(0, h - 1), :] for k in range(wy.shape[0])], wy)                    # [..., H, W]


# ------------------------------------------------------------------------------- retiming a panorama latent
RETIME_MODES = ("linear", "cubic")


def _retime_taps(f, F, mode, loop, dtype, device):
    """Taps of the ``F`` output frames of a clip of ``f``: (first tap [F] int64, unclamped and unwrapped; weights [taps, F]; keyframe flag
    [F], t == 0).  Output frame j samples source time num / den = i0 + t from integers: an open clip is endpoint-aligned (num =
    j (f - 1), den = max(F - 1, 1)), a ring is not (num = j f, den = F: frame F would be frame 0 again)."""
    j = torch.arange(F, dtype=torch.int64, device=device)
    num, den = (j * f, F) if loop else (j * (f - 1), max(F - 1, 1))
    i0 = torch.div(num, den, rounding_mode="floor")
    rem = num - i0 * den
    cubic = mode == "cubic"
    return (i0 - 1 if cubic else i0), _tap_weights(rem.to(dtype) / den, cubic), rem == 0


def retime_pano_latent(x, F, mode="linear", loop=False):
    """``x`` [..., f, h, w] -> [..., F, h, w], ``F >= f``: a clip resampled along its frame axis so that source frames land exactly on
    output frames.  The eager definition of ``kernels.retime_pano_latent``, in torch ops on any device, blending in ``x``'s dtype (the
    weights are formed in float32 for a 16-bit ``x``).  Output frame j samples source time i0 + t, from integers: an open clip
    (``loop=False``) is endpoint-aligned, num = j (f - 1) over den = max(F - 1, 1) -- frame 0 is frame 0 and frame F - 1 is frame f - 1,
    torch's ``align_corners=True``; a ring (``loop=True``) has num = j f over den = F, frame F being frame 0 again.  "linear": taps
    i0, i0 + 1 with weights (1 - t, t); "cubic": taps i0 - 1 .. i0 + 2, Keys kernel with A = -0.75 (the polynomials of
    ``resize_pano_latent``).  Tap frames clamp to [0, f - 1] on an open clip and wrap (mod f) on a ring.  A sum is w0 a0 + w1 a1 + ...
    in this order.  A frame with t == 0 is a COPY of source frame i0 -- NaNs and the sign of zero included -- and no weighted sum is
    formed there: with F = 2 f - 1 (open) or F = 2 f (ring) the even output frames are the source frames."""
    if mode not in RETIME_MODES:
        raise ValueError(f"retime_pano_latent: mode must be one of {sorted(RETIME_MODES)}, got {mode!r}")
    if not isinstance(F, int) or isinstance(F, bool):
        raise TypeError(f"retime_pano_latent: F must be an int, got {F!r}")
    if x.dim() < 3:
        raise ValueError(f"retime_pano_latent: x must be [..., f, h, w], got {list(x.shape)}")
    f = x.shape[-3]
    if F < f or f < 1:
        raise ValueError(f"retime_pano_latent: {f} -> {F} frames shrinks (there is no temporal antialiasing filter; F >= f >= 1)")
    wdt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    t0, wt, key = _retime_taps(f, F, mode, bool(loop), wdt, x.device)
    wt = wt.to(x.dtype)[:, :, None, None]
    frame = (lambda tap: tap % f) if loop else (lambda tap: tap.clamp(0, f - 1))
    acc = wt[0] * x[..., frame(t0), :, :]
    for k in range(1, wt.shape[0]):
        acc = acc + wt[k] * x[..., frame(t0 + k), :, :]
    i0 = t0 + 1 if mode == "cubic" else t0
    return torch.where(key[:, None, None], x[..., i0.clamp(0, f - 1), :, :], acc)


# ------------------------------------------------------------------------------- FreeInit: the low-pass of a panorama clip
def free_init_operator(n, d, periodic):
    """The Gaussian low-pass of FreeInit (arXiv 2312.07537; diffusers' ``free_init_utils``) along ONE axis of ``n`` samples, as a dense
    [n, n] float64 matrix (row i: the weights of output i), with the boundary that axis has.  FreeInit's gain is exp(-D^2 / (2 d_s^2))
    with D^2 = ((d_s / d_t) t)^2 + y^2 + x^2 in normalised frequency (fraction of Nyquist): a product of three 1-D gains, so the filter
    is three such operators -- ``d`` = d_s along h and w, d_t along the frames.  Only this Gaussian filter is offered: diffusers'
    Butterworth and ideal masks are not separable and would need a true 3-D transform.
    With g_N(k) = exp(-(2 k / N)^2 / (2 d^2)) over the signed integer frequencies k of ``torch.fft.fftfreq(N, 1 / N)``:
      ``periodic=True`` (longitude: the +-180 degree seam; the frames of a looping clip): the circular convolution
        L[i, j] = (1 / n) sum_k g_n(k) cos(2 pi k (i - j) / n);
      ``periodic=False`` (latitude: the poles; the frames of an open clip): the half-sample mirror extension to a ring of 2 n samples
        (x_0 .. x_{n-1}, x_{n-1} .. x_0), filtered there and cropped,
        L[i, j] = c(i - j) + c(i + j + 1),  c(m) = (1 / 2n) sum_k g_2n(k) cos(2 pi k m / 2n)
      -- ``fftn`` would wrap a pole into the other pole and the last frame into the first.
    ``n = 1`` gives [[1]].  Both kinds are symmetric and their rows sum to 1 (a constant clip passes unchanged), checked for n = 1 .. 64;
    d -> infinity gives the identity, d -> 0 the mean.  For even ``n`` on all three axes with ``periodic=True`` everywhere the operator
    equals diffusers' fftshift . Gaussian mask . ifftshift round trip (4e-16 at (16, 8, 16)); for odd ``n`` diffusers' mask is
    asymmetric in +-k and its result is not real: the symmetric gain above is the definition here."""
    if not isinstance(n, int) or isinstance(n, bool) or n < 1:
        raise ValueError(f"free_init_operator: n must be a positive int, got {n!r}")
    d = float(d)
    if not d > 0.0:
        raise ValueError(f"free_init_operator: d={d} must be positive (the cut-off as a fraction of Nyquist)")
    N = n if periodic else 2 * n
    k = torch.fft.fftfreq(N, 1.0 / N, dtype=torch.float64).round().to(torch.int64)
    g = torch.exp(-(2.0 * k.double() / N) ** 2 / (2.0 * d * d))

    def c(m):                                            # [..] int64 -> (1 / N) sum_k g(k) cos(2 pi k m / N), the angle reduced in integers
        ang = (k * m[..., None]) % N
        return (g * torch.cos(2.0 * math.pi * ang.double() / N)).sum(-1) / N

    i = torch.arange(n, dtype=torch.int64)
    diff, summ = i[:, None] - i[None, :], i[:, None] + i[None, :] + 1
    return c(diff) if periodic else c(diff) + c(summ)


def free_init_noise(x0, n1, n2, sa, sb, Lf, Lh, Lw):
    """FreeInit's EFFECTIVE NOISE, the eager definition of ``kernels.free_init_noise`` in torch ops on any device:

        d     = sa x0 + sb n1 - n2                  the noised clip minus the fresh noise
        y     = (Lf (x) Lh (x) Lw) d                along w, then h, then the frames
        n_eff = n1 + (y - d) / sb                   <=>  sa x0 + sb n_eff = n2 + L (sa x0 + sb n1 - n2) = LPF(noised clip) + HPF(n2)

    ``x0`` [1, 4, F, h, w] (the clean clip, 16-bit in the pipeline); ``n1`` (the noise the clip was generated from), ``n2`` (a fresh
    draw) and the result [1, F, 4, h, w], the layout ``pano_noise_and_index`` draws in, in ``n1``'s dtype (float32; float64 for the
    tests); the operators [F, F], [h, h], [w, w] from ``free_init_operator``, cast to that dtype.  A noise rather than a start latent
    is returned so that ``kernels.noise_latents``, the perspective gather and the graphed steps run unchanged on it and both branches
    begin from the same numbers.  ``sb <= 0`` is refused (pure signal has no noise to replace).  Only the Gaussian filter is offered:
    Butterworth and ideal masks are not separable."""
    if not float(sb) > 0.0:
        raise ValueError(f"free_init_noise: sb={float(sb)} must be positive (pure signal has no noise to replace)")
    if x0.dim() != 5 or n1.dim() != 5 or tuple(n1.shape) != (x0.shape[0], x0.shape[2], x0.shape[1], *x0.shape[3:]) or n2.shape != n1.shape:
        raise ValueError(f"free_init_noise: x0 [1, C, F, h, w] and n1, n2 [1, F, C, h, w] expected, got {list(x0.shape)}, {list(n1.shape)}, "
                         f"{list(n2.shape)}")
    wdt = n1.dtype
    Lf, Lh, Lw = (L.to(device=n1.device, dtype=wdt) for L in (Lf, Lh, Lw))
    d = sa * x0.permute(0, 2, 1, 3, 4).to(wdt) + sb * n1 - n2.to(wdt)
    y = torch.matmul(d, Lw.t())
    y = torch.matmul(Lh, y)
    y = torch.einsum("ij,bjchw->bichw", Lf, y)
    return n1 + (y - d) / sb


# ---------------------------------------------------------------------------------------------------------------------------------------
# The spherical feather of a regenerate_mask (pipeline ``regenerate_feather``): distances on the sphere, not on the pixel grid.

def pixel_directions(h, w, dtype=torch.float32):
    """Unit vectors of the pixel centres of an ``h x w`` equirectangular image, [h * w, 3] (row-major, the order of a flattened plane):
    longitude ``(x + 1/2) / w * 2 pi - pi``, latitude ``pi / 2 - (y + 1/2) / h * pi``, ``n = (cos lat cos lon, cos lat sin lon, sin lat)``.
    The trigonometry is fp64 on the host; the table is rounded once to ``dtype`` (float32: what ``kernels.sphere_distance2`` reads)."""
    lon = (torch.arange(w, dtype=torch.float64) + 0.5) / w * (2.0 * math.pi) - math.pi
    lat = math.pi / 2.0 - (torch.arange(h, dtype=torch.float64) + 0.5) / h * math.pi
    lat, lon = lat[:, None].expand(h, w), lon[None, :].expand(h, w)
    n = torch.stack((lat.cos() * lon.cos(), lat.cos() * lon.sin(), lat.sin()), dim=-1)
    return n.reshape(h * w, 3).to(dtype).contiguous()


def sphere_distance2(keep, dirs, chunk_elems=1 << 22):
    """The eager definition of ``kernels.sphere_distance2`` in torch ops on any device: ``keep`` bool / uint8 [F, h, w] (non-zero: a
    kept pixel), ``dirs`` [h * w, 3] (``pixel_directions``; float32, or float64 for the tests) -> [F, h, w] in ``dirs``'s dtype,

        d2[f, p] = min over the kept q of frame f of |dirs[p] - dirs[q]|^2 = dx^2 + dy^2 + dz^2 from the DIFFERENCES

    (``2 - 2 dot`` would lose the small distances), ``+inf`` for a frame that keeps nothing.  The kept vectors of a frame are gathered
    first and the pixels taken in chunks of at most ``chunk_elems`` pairs, so the ``HW x HW`` matrix never exists whole (4.3 GB per
    frame at 128 x 256 in fp32)."""
    F, h, w = keep.shape
    HW = h * w
    if tuple(dirs.shape) != (HW, 3):
        raise ValueError(f"sphere_distance2: dirs must be {[HW, 3]} for keep {list(keep.shape)}, got {list(dirs.shape)}")
    out = torch.full((F, HW), float("inf"), dtype=dirs.dtype, device=dirs.device)
    kept = keep.reshape(F, HW).to(dirs.device) != 0
    for f in range(F):
        cand = dirs[kept[f]]                                            # [K, 3]
        if cand.shape[0] == 0:
            continue
        step = max(1, int(chunk_elems) // cand.shape[0])
        for p0 in range(0, HW, step):
            d = dirs[p0:p0 + step, None, :] - cand[None, :, :]
            out[f, p0:p0 + step] = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).min(dim=1).values
    return out.reshape(F, h, w)


def feather_ramp(d2, degrees):
    """``clamp(theta / Theta, 0, 1)`` with ``theta = 2 asin(min(1, sqrt(d2) / 2))`` the great-circle angle of the squared chord ``d2``
    and ``Theta = degrees`` in radians; 1 where ``d2`` is ``+inf`` (a frame that keeps nothing has nothing to feather from)."""
    theta = 2.0 * torch.asin((d2.sqrt() / 2.0).clamp(max=1.0))
    ramp = (theta / math.radians(float(degrees))).clamp(0.0, 1.0)
    return torch.where(torch.isinf(d2), torch.ones((), dtype=ramp.dtype, device=ramp.device), ramp)


def feather_pano_mask(mask, degrees, distance2=None):
    """A ``regenerate_mask`` at latent resolution feathered on the sphere, the whole map: ``mask`` [F, h, w] in [0, 1] (1: regenerate,
    0: keep) -> ``min(mask, ramp)``, where ``ramp`` rises from 0 on the kept set ``{mask <= 0}`` of each frame to 1 over ``degrees`` of
    great-circle arc away from it (``feather_ramp`` of ``sphere_distance2``) -- across the +-180 degree seam, and by the same arc at a
    pole as at the equator.  A 0 / 1 mask becomes a strength map for ``regenerate_mode="release"``; fractional values are only ever
    lowered.  ``degrees == 0`` returns the mask.  ``distance2``: the function ``(keep, dirs) -> d2`` (None: the eager
    ``sphere_distance2``; the pipeline passes ``kernels.sphere_distance2``)."""
    degrees = float(degrees)
    if not (math.isfinite(degrees) and degrees >= 0.0):
        raise ValueError(f"feather_pano_mask: degrees must be finite and >= 0, got {degrees}")
    if mask.dim() != 3:
        raise ValueError(f"feather_pano_mask: mask must be [F, h, w], got {list(mask.shape)}")
    if degrees == 0.0:
        return mask
    dirs = pixel_directions(mask.shape[1], mask.shape[2]).to(mask.device)
    d2 = (distance2 or sphere_distance2)((mask <= 0).to(torch.uint8), dirs)
    return torch.minimum(mask, feather_ramp(d2, degrees).to(mask.dtype))
