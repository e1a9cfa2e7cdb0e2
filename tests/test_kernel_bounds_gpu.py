"""Guard-band tests (tests/_guarded.py): every kernel family at its ragged edges, with every input, result and workspace between
poisoned guards.  Each case checks the result against an fp64 CPU reference with the tolerances of test_kernels_gpu.py, and on
leaving the ``with`` block that (1) no guard byte changed, (2) no row gap of a strided buffer changed, (3) every result is fully
written, (4) every result lives in a guarded buffer.  The sentinel is a NaN: a tail read that leaks into a result fails the
comparison (``rel < tol`` is false for NaN).  Shapes are the smallest at which the edge exists."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _guarded import PATTERN, Guarded  # noqa: E402
from im360_oracle import geometry as OG  # noqa: E402
from imagine360_amd import kernels as K  # noqa: E402
from test_ddim_stochastic_gpu import _host_step  # noqa: E402
from test_kernels_gpu import DTYPES, TOL, blockrel, q16, rel, rnd  # noqa: E402

torch.set_grad_enabled(False)


def dn(g, t, dt=None, **kw):
    """A finite host tensor -> the device, between guards."""
    return g.guard((t if dt is None else t.to(dt)).cuda(), **kw)


def sdpa64(q, k, v, heads, scale=None, bias=None):
    B, Nq, C = q.shape
    d = C // heads
    sp = lambda t: t.double().reshape(t.shape[0], t.shape[1], heads, d).transpose(1, 2)
    s = sp(q) @ sp(k).transpose(2, 3) * (d ** -0.5 if scale is None else scale)
    if bias is not None:
        s = s + bias.double()
    return (torch.softmax(s, -1) @ sp(v)).transpose(1, 2).reshape(B, Nq, C)


def conv64(x, w, b, stride=1, up=False, wrap_pad=0, unpad=0):
    xr = x.double().permute(0, 3, 1, 2)
    if wrap_pad:
        xr = OG.pad_pano(xr, wrap_pad)
    if up:
        xr = F.interpolate(xr, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xr, w.double(), None if b is None else b.double(), stride=stride, padding=w.shape[-1] // 2)
    return OG.unpad_pano(y, unpad).permute(0, 2, 3, 1)


def close(out, ref, dt, rows=32, f=1.0):
    return rel(out, ref) < f * TOL[dt] and blockrel(out, ref, rows) < 2 * f * TOL[dt]


# ------------------------------------------------------------------------------------------ attention
ATTN_CASES = [  # D, B, H, Nq, Nk, kv_group, form
    (64, 2, 2, 33, 77, 1, "plain"), (32, 2, 3, 100, 130, 1, "plain"), (64, 1, 2, 5, 1, 1, "plain"), (32, 1, 2, 5, 77, 1, "plain"),
    (64, 4, 2, 100, 130, 2, "plain"), (32, 4, 2, 33, 77, 2, "plain"),
    (64, 2, 2, 33, 77, 1, "out"), (32, 2, 2, 100, 130, 1, "out"), (64, 2, 2, 33, 77, 1, "acc"), (32, 2, 2, 5, 130, 1, "acc"),
    (64, 2, 2, 33, 76, 1, "bias"), (32, 2, 2, 100, 76, 1, "bias"),                      # Nk % 4 == 0, 76 = 2 x 32 + 12
    (32, 2, 2, 40, 72, 1, "packed"),                                                      # the last 32 x 32 block is 8 x 8
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D,B,H,Nq,Nk,group,form", ATTN_CASES)
def test_attention_edges(dt, D, B, H, Nq, Nk, group, form):
    C = H * D
    q, k, v = (q16(rnd(b, n, C, seed=s), dt) for b, n, s in ((B, Nq, 1), (B // group, Nk, 2), (B // group, Nk, 3)))
    rep = lambda t: t.repeat_interleave(group, 0)
    g = Guarded(K)
    dq, dk, dv = (dn(g, t, dt) for t in (q, k, v))
    strides = ((Nq + 3) * (C + 8), C + 8, 1)                # row stride C + 8, batch stride three rows above Nq rows
    if form in ("plain", "out", "acc"):
        ref = sdpa64(q, rep(k), rep(v), H)
        with g:
            if form == "plain":
                out = K.attention(dq, dk, dv, H, kv_group=group)
            elif form == "out":
                out = K.attention(dq, dk, dv, H, out=g.empty((B, Nq, C), dt, "cuda", strides=strides))
            else:
                prev = q16(rnd(B, Nq, C, seed=4), dt)
                ref = prev.double() + 0.5 * ref
                out = K.attention(dq, dk, dv, H, out=dn(g, prev, dt, strides=strides), accumulate=True, out_scale=0.5)
            g.out(out)
        assert out.stride() == (strides if form != "plain" else (Nq * C, C, 1))
        assert close(out, ref, dt)
        return
    gen = torch.Generator().manual_seed(6)
    if form == "bias":
        bias = q16(torch.rand(Nq, Nk, generator=gen) * 2 - 1, dt)
        db = dn(g, bias, dt)
        with g:
            out = g.out(K.attention(dq, dk, dv, H, bias=db))
        assert close(out, sdpa64(q, k, v, H, bias=bias), dt)
        return
    # packed bias + block map: non-zero only in the top-left block and in the partial bottom-right one
    bias, alt = torch.zeros(Nq, Nk), torch.zeros(Nq, Nk)
    bias[:11, :21] = torch.rand(11, 21, generator=gen) * 2 - 1
    bias[33:, 65:] = torch.rand(Nq - 33, Nk - 65, generator=gen) * 2 - 1
    alt[33:, :40] = torch.rand(Nq - 33, 40, generator=gen) * 2 - 1
    bias, alt = q16(bias, dt), q16(alt, dt)
    db, da = dn(g, bias, dt), dn(g, alt, dt)
    sels = [dn(g, torch.tensor([f], dtype=torch.int32)) for f in (0, 1)]
    refs = sdpa64(q, k, v, H, bias=bias), sdpa64(q, k, v, H, bias=alt)
    try:
        for qb in (0, 2):                                    # 2: the two-query-block kernel, the one that reads the block map
            K.tuning_set("attn_qb", qb)
            with g:
                pb, pa = g.out(K.pack_attn_bias(db), K.pack_attn_bias(da))
                mb, ma = g.guard(K.attn_bias_blocks(pb)), g.guard(K.attn_bias_blocks(pa))
                outs = [g.out(K.attention(dq, dk, dv, H, bias=pb, bias_packed=True, bias_blocks=mb))]
                outs += [g.out(K.attention(dq, dk, dv, H, bias=pb, bias_alt=pa, bias_sel=s, bias_packed=True, bias_blocks=mb, bias_blocks_alt=ma))
                         for s in sels]
            assert rel(pb, bias * 1.4426950408889634) < 3e-3              # fp16 of bias * log2(e), both dtypes
            for o, r in zip(outs, (refs[0], refs[0], refs[1])):
                assert close(o, r, dt), qb
    finally:
        K.tuning_set("attn_qb", 0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("knob", [1, 66])                   # two schedules of test_attention_pipelined_kernel
@pytest.mark.parametrize("B,H,Nq,Nk", [(2, 2, 33, 77), (1, 2, 100, 130), (1, 1, 200, 128)])
def test_attention_pipelined_schedules_edges(dt, knob, B, H, Nq, Nk):
    """attn_pipe.hip ("past the end: the last tile again, never read") at ragged query / key counts; where the launcher keeps
    attn_fwd_kernel for a shape, the same bounds hold for that."""
    C = H * 64
    q, k, v = (q16(rnd(B, n, C, seed=s), dt) for n, s in ((Nq, 1), (Nk, 2), (Nk, 3)))
    g = Guarded(K)
    dq, dk, dv = (dn(g, t, dt) for t in (q, k, v))
    try:
        K.tuning_set("attn_pipe", knob)
        with g:
            out = g.out(K.attention(dq, dk, dv, H))
    finally:
        K.tuning_set("attn_pipe", K.ATTN_PIPE_DEFAULT)
    assert close(out, sdpa64(q, k, v, H), dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,Nq,n1,n2,group", [(2, 64, 65, 33, 1), (2, 64, 96, 64, 1), (4, 64, 65, 33, 2),       # resident route: Nq % 32 == 0
                                              (2, 40, 77, 64, 1), (2, 300, 77, 64, 1), (4, 40, 65, 33, 2)])     # generic route: Nq % 32 != 0
def test_attention_two_key_sets_edges(dt, B, Nq, n1, n2, group):
    H, D = 2, 64
    C = H * D
    q = q16(rnd(B, Nq, C, seed=70, scale=0.3), dt)
    k1, v1, k2, v2 = (q16(rnd(B // group, n, C, seed=s), dt) for n, s in ((n1, 71), (n1, 72), (n2, 73), (n2, 74)))
    rep = lambda t: t.repeat_interleave(group, 0)
    ref = sdpa64(q, rep(k1), rep(v1), H) + 0.7 * sdpa64(q, rep(k2), rep(v2), H)
    g = Guarded(K)
    args = [dn(g, t, dt) for t in (q, k1, v1, k2, v2)]
    with g:
        out = g.out(K.attention2(*args, H, out_scale2=0.7, kv_group=group))
    assert close(out, ref, dt, f=1.5)                        # (1.5: two attention results summed, as test_attention_two_kv_sets_one_launch)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("frame_major", [False, True])
@pytest.mark.parametrize("Fr", [1, 5, 16, 64])
def test_temporal_attention_edges(dt, frame_major, Fr):
    B, heads = 2, 2
    for P in (1, 7, 33):
        for d in (8, 40):
            C = heads * d
            qkv = q16(rnd(B * Fr * P, 3 * C, seed=15 + P + d), dt)
            x = qkv.reshape(Fr, B, P, 3 * C).permute(1, 0, 2, 3) if frame_major else qkv.reshape(B, Fr, P, 3 * C)
            t = x.permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
            ref = sdpa64(t[..., :C], t[..., C:2 * C], t[..., 2 * C:], heads).reshape(B, P, Fr, C)
            ref = (ref.permute(2, 0, 1, 3) if frame_major else ref.permute(0, 2, 1, 3)).reshape(B * Fr * P, C)
            g = Guarded(K)
            plain, wide = dn(g, qkv, dt), dn(g, qkv, dt, row_stride=3 * C + 8)       # the fused projection as a view of wider rows
            with g:
                o1 = g.out(K.temporal_attention(plain, B, Fr, P, heads, frame_major=frame_major))
                o2 = g.out(K.temporal_attention(wide, B, Fr, P, heads, frame_major=frame_major, out=g.empty((B * Fr * P, C), dt, "cuda")))
            assert rel(o1, ref) < TOL[dt] and rel(o2, ref) < TOL[dt], (P, d)


# ------------------------------------------------------------------------------------------ group norm
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("route", ["partials", "three", "fused"])
@pytest.mark.parametrize("H,W", [(4, 4), (6, 10), (8, 16)])
def test_group_norm_edges(dt, route, H, W):
    """Every route of kernels.group_norm; the partial-sum, scale / shift and counter workspaces come from the proxy, so their guards
    count.  The fused route's arrival counter: zeroed by the call, then one arrival per slab -- S on return."""
    N = 3
    saved = K.GN_MODE, K.GN_FUSED
    try:
        K.GN_MODE, K.GN_FUSED = ("three" if route == "three" else "partials"), route == "fused"
        for C1, C2 in ((32, 0), (320, 0), (64, 64), (320, 320)):
            C = C1 + C2
            xa = q16(rnd(N, H, W, C1, seed=16) + 0.5, dt)
            xb = q16(rnd(N, H, W, C2, seed=17) * 1.5, dt) if C2 else None
            gamma, beta = q16(1 + 0.1 * rnd(C, seed=18), dt), q16(0.1 * rnd(C, seed=19), dt)
            cat = (xa if xb is None else torch.cat([xa, xb], -1)).double().permute(0, 3, 1, 2)
            for pad in sorted({0, 2, W // 2}):
                base = F.group_norm(OG.pad_pano(cat, pad), 32, gamma.double(), beta.double(), 1e-5)
                for silu in (False, True):
                    ref = (F.silu(base) if silu else base).permute(0, 2, 3, 1)
                    g = Guarded(K)
                    da, dg, db = dn(g, xa, dt), dn(g, gamma, dt), dn(g, beta, dt)
                    x = da if xb is None else (da, dn(g, xb, dt))
                    with g:
                        out = g.out(K.group_norm(x, dg, db, 32, 1e-5, silu=silu, pad=pad))
                        ints = [a for a in g.allocs if a.dtype == torch.int32]
                    assert out.shape == ref.shape and rel(out, ref) < TOL[dt], (C1, C2, pad, silu)
                    if route == "fused":
                        assert len(ints) == 1 and ints[0].shape == (N,)
                        assert ints[0].view.tolist() == [K.lib().im360_gn_num_slabs(N, H, W)] * N
    finally:
        K.GN_MODE, K.GN_FUSED = saved


# ------------------------------------------------------------------------------------------ convolution
def _conv_inputs(dt, N, H, W, Cin, Cout, k, seed=19):
    x = q16(rnd(N, H, W, Cin, seed=seed), dt)
    w = q16(rnd(Cout, Cin, k, k, seed=seed + 1, scale=(k * k * Cin) ** -0.5), dt)
    b = q16(rnd(Cout, seed=seed + 2, scale=0.1), dt)
    return x, w, b


CONV_CASES = [  # N, H, W, Cin, Cout, k, kwargs, reference arguments
    (1, 5, 7, 32, 4, 3, dict(), dict()),                                         # the VAE's last layers
    (2, 3, 5, 32, 8, 1, dict(), dict()),
    (2, 6, 10, 64, 96, 3, dict(stride=2), dict(stride=2)),                       # Cout % 128 in (0, 64]
    (1, 5, 6, 64, 96, 3, dict(up=True, wrap=True), dict(up=True, wrap_pad=1, unpad=2)),
    (3, 9, 11, 64, 320, 3, dict(wrap=True), dict(wrap_pad=1, unpad=1)),          # M = 297: one full 256-row tile + 41 rows
    (3, 9, 11, 64, 320, 1, dict(), dict()),
    (2, 6, 10, 64, 96, 3, dict(stride=2, wrap=True), dict(stride=2, wrap_pad=2, unpad=1)),
]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,H,W,Cin,Cout,k,kw,rk", CONV_CASES)
def test_conv2d_edges(dt, N, H, W, Cin, Cout, k, kw, rk):
    x, w, b = _conv_inputs(dt, N, H, W, Cin, Cout, k)
    ref = conv64(x, w, b, **rk)
    g = Guarded(K)
    dx, dw, db = dn(g, x, dt), dn(g, w, dt), dn(g, b, dt)
    with g:
        wp = g.out(K.pack_conv_weight(dw))
        out = g.out(K.conv2d(dx, wp, Cout, bias=db, **kw))
    assert out.shape == ref.shape and close(out, ref, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_conv2d_offsets_temb_residual_edges(dt):
    """x_off on the W + 4 pre-padded tensor with an explicit wout; x_off = y_off = 1 (the VAE downsampler's (0, 1, 0, 1) padding);
    time embedding shared by two images + residual."""
    N, H, W, C, Co = 2, 6, 10, 64, 96
    x, w, b = _conv_inputs(dt, N, H, W, C, Co, 3, seed=22)
    xp = OG.pad_pano(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    temb, res = q16(rnd(N // 2, Co, seed=29), dt), q16(rnd(N, H, W, Co, seed=30), dt)
    ref_off = OG.unpad_pano(F.conv2d(xp.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1), 2).permute(0, 2, 3, 1)
    ref_vae = F.conv2d(F.pad(x.double().permute(0, 3, 1, 2), (0, 1, 0, 1)), w.double(), b.double(), stride=2).permute(0, 2, 3, 1)
    ref_epi = conv64(x, w, b) + temb.double().repeat_interleave(2, 0)[:, None, None, :] + res.double()
    g = Guarded(K)
    dx, dxp, dw, db, dte, dre = (dn(g, t, dt) for t in (x, xp, w, b, temb, res))
    with g:
        wp = K.pack_conv_weight(dw)
        o_off = g.out(K.conv2d(dxp, wp, Co, bias=db, x_off=2, wout=W))
        o_vae = g.out(K.conv2d(dx, wp, Co, bias=db, stride=2, x_off=1, y_off=1))
        o_epi = g.out(K.conv2d(dx, wp, Co, bias=db, temb=dte, imgs_per_temb=2, res=dre))
    assert close(o_off, ref_off, dt) and o_vae.shape == ref_vae.shape and close(o_vae, ref_vae, dt) and close(o_epi, ref_epi, dt)


def _unfold_conv64(x, w, b):
    cols = F.unfold(x.double().permute(0, 3, 1, 2), 3, padding=1)                           # [N, Cin * 9, H * W]
    y = torch.einsum("ok,nkp->npo", w.double().reshape(w.shape[0], -1), cols) + b.double()
    return y.reshape(x.shape[0], x.shape[1], x.shape[2], w.shape[0])


@pytest.mark.parametrize("dt", DTYPES)
def test_conv2d_256x320_tile_ragged_edges(dt):
    """The 256 x 320 tile: launch_conv (conv3x3.hip) takes it for Cout % 320 == 0, Cin % 64 == 0 and big_tile_count(M, Cout) =
    ceil(M / 256) * (Cout / 320) >= BIG_TILE_MIN = 512.  Cout 1280 gives 4 cout tiles, so 128 row tiles: the smallest ragged M is
    127 * 256 + 77 = 32589 = 27 * 17 * 71 pixels.  (The reference of this one case is 24 G fp64 multiply-adds: what the threshold costs.)"""
    N, H, W, Cin, Cout = 27, 17, 71, 64, 1280
    assert -(-N * H * W // 256) * (Cout // 320) == 512 and (N * H * W) % 256 == 77
    x, w, b = _conv_inputs(dt, N, H, W, Cin, Cout, 3, seed=40)
    ref = _unfold_conv64(x, w, b)
    g = Guarded(K)
    dx, dw, db = dn(g, x, dt), dn(g, w, dt), dn(g, b, dt)
    with g:
        out = g.out(K.conv2d(dx, K.pack_conv_weight(dw), Cout, bias=db))
    assert close(out, ref, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_conv2d_gn_statistics_edges(dt):
    """gn_stats=True where im360_conv_gn_slabs > 0 (whole 256-pixel tiles per image, 512 big tiles): 128 images of 16 x 16, 1 x 1
    taps, Cout 1280.  The partial sums [M / 256][2][Cout] are a result too: fully written, equal to sums over the stored output."""
    N, H, W, Cin, Cout = 128, 16, 16, 64, 1280
    assert K.lib().im360_conv_gn_slabs(N, H, W, Cin, Cout, 1) == 1
    x, w, b = _conv_inputs(dt, N, H, W, Cin, Cout, 1, seed=44)
    g = Guarded(K)
    dx, dw, db = dn(g, x, dt), dn(g, w, dt), dn(g, b, dt)
    with g:
        out = g.out(K.conv2d(dx, K.pack_conv_weight(dw), Cout, bias=db, gn_stats=True))
        part, slabs = K._gn_of(out)
        g.out(part)
    assert slabs == 1 and close(out, conv64(x, w, b), dt, rows=256)
    t = out.double().cpu().reshape(N, H * W, Cout)
    want = torch.stack([t.sum(1), (t * t).sum(1)], dim=1)
    assert rel(part.reshape(N, 2, Cout), want) < 1e-5


def _ksplit_case(dt):
    """conv_ksplit forced to 2 parts: ksplit_plan (conv3x3.hip) needs 3 x 3 taps, Cout % 320 == 0, Cin / 64 >= 2 chunks and at
    least 64 tiles; 7 images of 53 x 45 = 16695 pixels = 65 full row tiles + 55 rows."""
    N, H, W, Cin, Cout = 7, 53, 45, 128, 320
    x, w, b = _conv_inputs(dt, N, H, W, Cin, Cout, 3, seed=97)
    return (N, H, W, Cin, Cout), x, w, b, _unfold_conv64(x, w, b)


@pytest.mark.parametrize("dt", DTYPES)
def test_conv2d_k_split_edges(dt):
    (N, H, W, Cin, Cout), x, w, b, ref = _ksplit_case(dt)
    g = Guarded(K)
    dx, dw, db = dn(g, x, dt), dn(g, w, dt), dn(g, b, dt)
    lib = K.lib()
    tiles = -(-N * H * W // 256)
    try:
        K.tuning_set("conv_ksplit", 2)
        assert lib.im360_conv_ksplit_plan(N, H, W, Cin, Cout, 9, 0, 0, 0) == 2
        with g:
            wp = K.pack_conv_weight(dw)
            out = g.out(K.conv2d(dx, wp, Cout, bias=db))                   # the wrapper's own scratch and counters, guarded by the proxy
            cnts = [a for a in g.allocs if a.dtype == torch.int32]
            # the C entry point with caller-owned scratch: counters zero on entry, zero again on return; twice the same bits
            ws = g.empty((tiles * 160 * 512,), torch.float32, "cuda")
            cnt = g.guard(torch.zeros(tiles, dtype=torch.int32, device="cuda"))
            ys = [g.empty((N, H, W, Cout), dt, "cuda") for _ in range(2)]
            for y in ys:
                rc = lib.im360_conv_fwd_ksplit(dx.data_ptr(), wp.data_ptr(), db.data_ptr(), None, None, y.data_ptr(), N, H, W, Cin, H, W, Cout, 9, 1,
                                               0, 0, 0, 0, 1, K._dt(dx), K._stream(), None, ws.data_ptr(), ws.numel() * 4, cnt.data_ptr(), tiles)
                K._check(rc, "im360_conv_fwd_ksplit")
                torch.cuda.synchronize()
                assert int(cnt.abs().sum()) == 0
            g.out(*ys)
        assert len(cnts) == 1 and cnts[0].shape == (tiles,) and int(cnts[0].view.abs().sum()) == 0
    finally:
        K.tuning_set("conv_ksplit", 1)
    assert close(out, ref, dt) and torch.equal(ys[0], ys[1]) and torch.equal(ys[0], out)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wrap", [False, True])
def test_conv_up2_and_conv1x1_cat_edges(dt, wrap):
    N, H, W, Cin, Cout = 3, 5, 7, 64, 8                       # M = 105 low-resolution pixels: one ragged 128-row tile
    x, w, b = _conv_inputs(dt, N, H, W, Cin, Cout, 3, seed=92)
    up = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    if wrap:
        ref = F.conv2d(F.pad(torch.cat([up[..., -1:], up, up[..., :1]], dim=-1), (0, 0, 1, 1)), w.double(), b.double())
    else:
        ref = F.conv2d(up, w.double(), b.double(), padding=1)
    g = Guarded(K)
    dx, dw, db = dn(g, x, dt), dn(g, w, dt), dn(g, b, dt)
    with g:
        w4 = g.guard(K.pack_conv_up2_weight(dw))
        out = g.out(K.conv_up2(dx, w4, Cout, bias=db, wrap=wrap))
    assert out.shape == (N, 2 * H, 2 * W, Cout) and close(out, ref.permute(0, 2, 3, 1), dt)
    if wrap:
        return
    for Co in (320, 96):                                      # M = 297 rows: ragged against 128 and 256
        N, H, W, C1, C2 = 3, 9, 11, 64, 64
        xa, xb = q16(rnd(N, H, W, C1, seed=74), dt), q16(rnd(N, H, W, C2, seed=75), dt)
        w1 = q16(rnd(Co, C1 + C2, 1, 1, seed=76, scale=(C1 + C2) ** -0.5), dt)
        b1, r = q16(rnd(Co, seed=77, scale=0.1), dt), q16(rnd(N, H, W, Co, seed=78), dt)
        ref = F.linear(torch.cat([xa, xb], -1).double(), w1.double().reshape(Co, -1), b1.double()) + r.double()
        g = Guarded(K)
        da, dbb, dw1, db1, dr = (dn(g, t, dt) for t in (xa, xb, w1, b1, r))
        with g:
            out = g.out(K.conv1x1_cat(da, dbb, K.pack_conv_weight(dw1), Co, bias=db1, res=dr))
        assert close(out, ref, dt), Co


# ------------------------------------------------------------------------------------------ token-major linears
def _row_stats(x, sl=160):
    """(sum, sum of squares) per row and 160-column slice, the producer's layout."""
    M, Kd = x.shape
    xs = x.double().reshape(M, Kd // sl, sl) if Kd % sl == 0 else x.double().reshape(M, 1, Kd)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1).float().contiguous()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,Kd,N", [(1, 64, 320), (300, 64, 320), (257, 320, 640),
                                    (127 * 256 + 77, 64, 1280)])      # 128 x 4 tiles = BIG_TILE_MIN (conv3x3.hip), ragged remainder
def test_linear_row_statistics_edges(dt, M, Kd, N):
    x, w = q16(rnd(M, Kd, seed=80), dt), q16(rnd(N, Kd, seed=81, scale=Kd ** -0.5), dt)
    b, r = q16(rnd(N, seed=82, scale=0.2), dt), q16(rnd(M, N, seed=83) + 0.7, dt)
    ref = F.linear(x.double(), w.double(), b.double()) + r.double()
    g = Guarded(K)
    dx, dw, db, dr = dn(g, x, dt), dn(g, w.reshape(N, Kd, 1, 1), dt), dn(g, b, dt), dn(g, r, dt)
    with g:
        wp = K.pack_conv_weight(dw)
        y, st = g.out(*K.linear(dx, wp, N, bias=db, res=dr, row_stats=True))
        y0 = g.out(K.linear(dx, wp, N, bias=db, res=dr))
    assert close(y, ref, dt, rows=256) and torch.equal(y, y0)
    t = y.double().cpu().reshape(M, N // 160, 160)
    want = torch.stack([t.sum(-1), (t * t).sum(-1)], dim=-1)
    assert st.shape == (M, N // 160, 2) and float((st.double().cpu() - want).abs().max()) < 2e-5 * float(want.abs().max())


@pytest.mark.parametrize("dt", DTYPES)
def test_linear_gn_statistics_edges(dt):
    """linear(..., gn_hw=256): rows that are whole 256-row tiles also get GroupNorm partial sums [M / 256][2][n]."""
    M, Kd, N = 512, 64, 320
    x, w, b = q16(rnd(M, Kd, seed=84), dt), q16(rnd(N, Kd, seed=85, scale=Kd ** -0.5), dt), q16(rnd(N, seed=86, scale=0.2), dt)
    g = Guarded(K)
    dx, dw, db = dn(g, x, dt), dn(g, w.reshape(N, Kd, 1, 1), dt), dn(g, b, dt)
    with g:
        y = g.out(K.linear(dx, K.pack_conv_weight(dw), N, bias=db, gn_hw=256))
        part, slabs = K._gn_of(y)
        g.out(part)
    assert slabs == 1 and close(y, F.linear(x.double(), w.double(), b.double()), dt, rows=256)
    t = y.double().cpu().reshape(M // 256, 256, N)
    assert rel(part.reshape(M // 256, 2, N), torch.stack([t.sum(1), (t * t).sum(1)], dim=1)) < 1e-5


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M", [300, 513])
def test_linears_with_folded_layer_norm_and_geglu_edges(dt, M):
    Kd, N, I = 320, 320, 128
    x = q16(rnd(M, Kd, seed=60) + 0.3, dt)
    w, b = q16(rnd(N, Kd, seed=61, scale=Kd ** -0.5), dt), q16(rnd(N, seed=62, scale=0.1), dt)
    gam, bet = q16(1 + 0.1 * rnd(Kd, seed=63), dt), q16(0.1 * rnd(Kd, seed=64), dt)
    gw, gb = q16(rnd(2 * I, Kd, seed=65, scale=Kd ** -0.5), dt), q16(rnd(2 * I, seed=66, scale=0.1), dt)
    tab = rnd(3, N, seed=67)
    ln = F.layer_norm(x.double(), (Kd,), gam.double(), bet.double(), 1e-5)
    ref_ln = F.linear(ln, w.double(), b.double())
    ref_tab = ref_ln + tab.double()[(torch.arange(M) // 256) % 3]
    geglu = lambda h: h[:, :I] * F.gelu(h[:, I:])
    ref_g, ref_gln = geglu(F.linear(x.double(), gw.double(), gb.double())), geglu(F.linear(ln, gw.double(), gb.double()))
    # the folded operands are host-side algebra (kernels.fold_layer_norm / interleave_geglu): built first, then guarded
    wg, c1, c2 = K.fold_layer_norm(w.to(dt), b.to(dt), gam.to(dt), bet.to(dt))
    gwf, gc1, gc2 = K.fold_layer_norm(gw.to(dt), gb.to(dt), gam.to(dt), bet.to(dt))
    gwi, gc1i = K.interleave_geglu(gwf, gc1)
    gc2i = K.interleave_geglu(gwf, gc2)[1]
    gwp_, gbp_ = K.interleave_geglu(gw.to(dt), gb.to(dt))
    g = Guarded(K)
    dx, dst, dtab = dn(g, x, dt), dn(g, _row_stats(x)), dn(g, tab)
    dwg, dc1, dc2 = dn(g, wg.reshape(N, Kd, 1, 1)), dn(g, c1), dn(g, c2)
    dgw, dgb = dn(g, gwp_.reshape(2 * I, Kd, 1, 1).contiguous()), dn(g, gbp_)
    dgwf, dgc1, dgc2 = dn(g, gwi.reshape(2 * I, Kd, 1, 1).contiguous()), dn(g, gc1i.contiguous()), dn(g, gc2i.contiguous())
    with g:
        wgp, gwp, gwfp = K.pack_conv_weight(dwg), K.pack_conv_weight(dgw), K.pack_conv_weight(dgwf)
        o_ln = g.out(K.linear_ln(dx, wgp, dc1, dc2, dst, 1e-5, N))
        o_tab = g.out(K.linear_ln(dx, wgp, dc1, dc2, dst, 1e-5, N, tab=g.guard(dtab + dc2[None, :]), tab_div=256, tab_has_c2=True))
        o_g = g.out(K.linear_geglu(dx, gwp, dgb, I))
        o_gln = g.out(K.linear_geglu_ln(dx, gwfp, dgc1, dgc2, dst, 1e-5, I))
    for o, r in ((o_ln, ref_ln), (o_tab, ref_tab), (o_g, ref_g), (o_gln, ref_gln)):
        assert close(o, r, dt, rows=256)


@pytest.mark.parametrize("dt", DTYPES)
def test_linear_geglu_ring_route_edges(dt):
    """im360_linear_geglu takes the ring kernel from ceil(M / 256) * (2 I / 256) >= BIG_TILE_MIN = 512 (conv3x3.hip): I = 1280 gives
    10 column tiles, so 52 row tiles; M = 51 * 256 + 77 is ragged (no g4 tile: those need M % 256 == 0)."""
    M, Kd, I = 51 * 256 + 77, 64, 1280
    x, w, b = q16(rnd(M, Kd, seed=68), dt), q16(rnd(2 * I, Kd, seed=69, scale=Kd ** -0.5), dt), q16(rnd(2 * I, seed=70, scale=0.1), dt)
    h = F.linear(x.double(), w.double(), b.double())
    wi, bi = K.interleave_geglu(w.to(dt), b.to(dt))
    g = Guarded(K)
    dx, dw, db = dn(g, x, dt), dn(g, wi.reshape(2 * I, Kd, 1, 1).contiguous()), dn(g, bi)
    with g:
        out = g.out(K.linear_geglu(dx, K.pack_conv_weight(dw), db, I))
    assert close(out, h[:, :I] * F.gelu(h[:, I:]), dt, rows=256)


# ------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("C", [64, 320, 640, 2048])
def test_layer_norm_edges(dt, C):
    """ "tail rows re-read the last row, never stored" (elementwise.hip): row counts below, at and above a workgroup's share."""
    for rows in (1, 5, 1003):
        x = q16(rnd(rows, C, seed=40) * 1.3 + 0.2, dt)
        gam, bet = q16(1 + 0.1 * rnd(C, seed=41), dt), q16(0.1 * rnd(C, seed=42), dt)
        pre, post = q16(rnd(7, C, seed=43), dt), q16(rnd(5, C, seed=44), dt)
        r = torch.arange(rows)
        ln = lambda t: F.layer_norm(t.double(), (C,), gam.double(), bet.double(), 1e-5)
        g = Guarded(K)
        dx, dg, db, dpre, dpost = (dn(g, t, dt) for t in (x, gam, bet, pre, post))
        with g:
            o0 = g.out(K.layer_norm(dx, dg, db, 1e-5))
            o1 = g.out(K.layer_norm(dx, dg, db, 1e-5, pre=dpre))
            o2 = g.out(K.layer_norm(dx, dg, db, 1e-5, post=dpost, post_div=3))
        assert rel(o0, ln(x)) < TOL[dt] and rel(o1, ln(x + pre[r % 7])) < TOL[dt] and rel(o2, ln(x) + post.double()[(r // 3) % 5]) < TOL[dt], rows


@pytest.mark.parametrize("dt", DTYPES)
def test_geglu_softmax_and_single_head_attention_edges(dt):
    for rows in (3, 1001):
        h = q16(rnd(rows, 2 * 320, seed=45) * 2, dt)
        g = Guarded(K)
        dh = dn(g, h, dt)
        with g:
            out = g.out(K.geglu(dh))
        assert rel(out, h[:, :320].double() * F.gelu(h[:, 320:].double())) < TOL[dt]
    x = q16(rnd(37, 1000, seed=80) * 3, dt)
    ref = torch.softmax(x.double() * 0.37, -1)
    g = Guarded(K)
    dx, dwide, dinp = dn(g, x, dt), dn(g, x, dt, row_stride=1008), dn(g, x, dt, row_stride=1008)
    with g:
        o0 = g.out(K.softmax_rows(dx, 0.37))
        o1 = g.out(K.softmax_rows(dwide, 0.37, out=g.empty((37, 1000), dt, "cuda", strides=(1008, 1))))
        o2 = g.out(K.softmax_rows(dinp, 0.37, out=dinp))                           # in place, strided
    assert o1.stride() == (1008, 1) and all(rel(o, ref) < TOL[dt] for o in (o0, o1, o2))
    nq, nk, d = 37, 96, 64                                                         # Nk % 32 == 0 but not a 128-row weight tile
    q, k, v = (q16(rnd(n, d, seed=s), dt) for n, s in ((nq, 81), (nk, 82), (nk, 83)))
    s = q16((q.double() @ k.double().t() * d ** -0.5).float(), dt)                  # the scores are stored in 16 bits
    ref = q16(torch.softmax(s.double(), -1).float(), dt).double() @ v.double()
    g = Guarded(K)
    dq, dk, dv = dn(g, q, dt), dn(g, k, dt), dn(g, v, dt)
    with g:
        out = g.out(K.single_head_attention(dq, dk, dv, d ** -0.5))
    assert rel(out, ref) < TOL[dt]


# ------------------------------------------------------------------------------------------ copies
@pytest.mark.parametrize("dt", DTYPES)
def test_copy_kernels_edges(dt):
    x = q16(rnd(3, 5, 16, 8, seed=30), dt)
    g = Guarded(K)
    dx = dn(g, x, dt)
    with g:
        out = g.out(K.circular_pad_w(dx, 4))
    assert torch.equal(out.float().cpu(), OG.pad_pano(x.permute(0, 1, 3, 2), 4).permute(0, 1, 3, 2))
    # shard_pack, both directions, P % W != 0: the zero tail is the kernel's to write
    for Wr, B, Fl, P, C in ((2, 2, 3, 37, 64), (3, 1, 2, 5, 8)):
        PP = -(-P // Wr)
        tok = rnd(B, Fl, P, C, seed=270).to(dt)
        want = torch.zeros(Wr, Fl, B, PP, C, dtype=dt)
        for r in range(Wr):
            n = max(0, min(PP, P - r * PP))
            want[r, :, :, :n] = tok[:, :, r * PP:r * PP + n].permute(1, 0, 2, 3)
        g = Guarded(K)
        dtok = dn(g, tok)
        with g:
            buf = g.out(K.shard_pack(dtok, g.empty((Wr, Fl, B, PP, C), dt, "cuda"), B, Fl, P, Wr, PP))
            back = g.out(K.shard_pack(buf, g.empty((B, Fl, P, C), dt, "cuda"), B, Fl, P, Wr, PP, unpack=True))
        assert torch.equal(buf.cpu().view(torch.int16), want.view(torch.int16)) and torch.equal(back.cpu().view(torch.int16), tok.view(torch.int16))
    # pack_conv_weight: the padding of the packed tensor is zeros the kernel writes, not whatever the allocation held
    w = q16(rnd(4, 4, 3, 3, seed=20), dt)
    want = torch.zeros(128, 9, 32)
    want[:4, :, :4] = w.reshape(4, 4, 9).permute(0, 2, 1)
    g = Guarded(K)
    dw = dn(g, w, dt)
    with g:
        wp = g.out(K.pack_conv_weight(dw))
    assert wp.shape == (128, 9, 32) and torch.equal(wp.float().cpu(), want)
    bias = q16(torch.cat([rnd(5, 13, seed=21) * 3, torch.full((1, 13), -float("inf"))]), dt)
    g = Guarded(K)
    db = dn(g, bias, dt)
    with g:
        pb = g.out(K.pack_attn_bias(db))
    want = (bias.double() * 1.4426950408889634).clamp(-60000, 60000)
    assert pb.dtype == torch.float16 and rel(pb, want) < 1e-3 and bool((pb[-1] == -60000).all())       # -inf becomes a finite mask


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32, torch.uint8, torch.float64])
def test_circular_pad_hw_edges(dt):
    """Every unit width the launcher can pick (16 / 8 / 4 / 2 / 1 bytes), both axes, pads equal to the axis."""
    gen = torch.Generator().manual_seed(5)
    for shape, pad in [((2, 3, 4, 16, 64), (16, 16, 0, 0)), ((1, 3, 9, 31), (5, 2, 3, 1)), ((3, 7, 13), (13, 13, 7, 7)),
                       ((2, 2, 6, 24), (8, 0, 0, 6)), ((1, 1, 5, 33), (1, 0, 0, 0))]:
        x = torch.randint(0, 255, shape, generator=gen).to(dt) if dt == torch.uint8 else torch.randn(shape, generator=gen).to(dt)
        g = Guarded(K)
        dx = dn(g, x)
        with g:
            got = g.out(K.circular_pad_hw(dx, *pad))
        ref = OG.circular_pad(x, pad)
        assert got.shape == ref.shape and torch.equal(got.cpu().view(torch.uint8), ref.contiguous().view(torch.uint8)), (shape, pad)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_remap_cubic_wrap_edges(C):
    from im360_oracle import preprocess as OPP
    from imagine360_amd import preprocess as PP
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 37, 53, C), dtype=np.uint8)
    mx = (rng.random((3, 19, 31)) * 80 - 15).astype(np.float32)                    # odd h x w; coordinates outside the image wrap
    my = (rng.random((3, 19, 31)) * 60 - 12).astype(np.float32)
    mx[0, 0, :8] = [0.0, 0.5, 1.5, 52.0, 52.984375, -0.015625, 53.0, -1.0]
    my[0, 0, :8] = [0.0, 0.5, 2.5, 36.0, 36.5, -0.5, 37.0, -4.0]
    g = Guarded(K)
    di, dmx, dmy, dtab = (dn(g, torch.from_numpy(a)) for a in (img, mx, my, PP.cubic_weight_table()))
    with g:
        got = g.out(K.remap_cubic_wrap(di, dmx, dmy, dtab)).cpu().numpy()
    for n in range(2):
        for m in range(3):
            assert np.array_equal(got[n, m], OPP.remap_cubic_wrap_u8(img[n], mx[m], my[m])), (n, m)


# ------------------------------------------------------------------------------------------ the DDIM step family
COEFS = (7.5, 0.8, 0.6, 0.85, 0.5, 0.15)                   # (guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma): sqrt_a^2 + sqrt_b^2 = 1
SHAPE = (1, 4, 5, 7, 24)                                   # 3360 elements: a multiple of 8, not of a workgroup's 2048


def _factor64(m, c, phi):
    return 1.0 if phi == 0.0 else float(phi * c.double().std() / m.double().std() + (1.0 - phi))


@pytest.mark.parametrize("dt", DTYPES)
def test_cfg_ddim_update_and_step_edges(dt):
    u, c, x, z = (q16(rnd(*SHAPE, seed=s), dt) for s in (31, 32, 33, 34))
    u, c = q16(u * 0.25, dt), q16(c * 0.25, dt)
    g = Guarded(K)
    du, dc, dx, dz = (dn(g, t, dt) for t in (u, c, x, z))
    with g:
        out = g.out(K.cfg_ddim_update(du, dc, dx, 7.5, 0.83, -0.41))
    assert rel(out, 0.83 * x.double() + -0.41 * (u.double() + 7.5 * (c.double() - u.double()))) < TOL[dt]
    for noise in (False, True):
        coefs = COEFS if noise else COEFS[:5] + (0.0,)
        for phi in (0.0, 0.7):
            m = u.double() + coefs[0] * (c.double() - u.double())
            mr = m * _factor64(m, c, phi)
            ref = _host_step(mr, mr, x, z if noise else None, 1 | 4, coefs)
            g = Guarded(K)
            du, dc, dx, dz = (dn(g, t, dt) for t in (u, c, x, z))
            with g:
                out = g.out(K.cfg_ddim_step(du, dc, dx, dz if noise else None, 1 | 4, coefs, rescale=phi))
                wss = [a for a in g.allocs if a.dtype == torch.float32]
            assert rel(out, ref) < TOL[dt], (noise, phi)
            assert len(wss) == (1 if phi else 0)                                    # the rescale workspace came from the proxy


def _blend64(preds, x, starts, w, guid, ring):
    """fp64 per-frame blends of u_k + g (c_k - u_k) and of c_k; frames (start + j) mod F on a ring."""
    fd = x.dim() - 3
    Fr, L = x.shape[fd], preds.shape[fd + 1]
    shape = [1] * x.dim()
    shape[fd] = L
    wv = w.double().reshape(shape)
    m, cb, ws = (torch.zeros(x.shape, dtype=torch.float64) for _ in range(3))
    for k, s in enumerate(starts):
        idx = (s + torch.arange(L)) % Fr
        assert ring or s + L <= Fr
        u, c = preds[k, 0:1].double(), preds[k, 1:2].double()
        m.index_add_(fd, idx, wv * (u + guid * (c - u)))
        cb.index_add_(fd, idx, wv * c)
        ws.index_add_(fd, idx, wv.expand_as(u).contiguous())
    return m / ws, cb / ws


def _windows_case(dt, inner_hw, ring, seed):
    Fr, L = 6, 4
    starts = [0, 3] if ring else [0, 2]                     # ring: frames 0-3 and 3, 4, 5, 0; line: 0-3 and 2-5
    shape = (1, 4, Fr) + inner_hw
    preds = q16(rnd(2, 2, 4, L, *inner_hw, seed=seed) * 0.25, dt)
    x, z = q16(rnd(*shape, seed=seed + 1), dt), q16(rnd(*shape, seed=seed + 2), dt)
    w = torch.tensor([1.0, 2.0, 2.0, 1.0])
    return preds, x, z, starts, w


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("inner_hw", [(1, 8), (3, 8), (1, 7)])      # inner 8 and 24: 16-byte lanes; 7: the scalar path
def test_cfg_ddim_step_windows_edges(dt, ring, inner_hw):
    preds, x, z, starts, w = _windows_case(dt, inner_hw, ring, seed=160)
    for phi in (0.0, 0.7):
        m, cb = _blend64(preds, x, starts, w, COEFS[0], ring)
        mr = m * _factor64(m, cb, phi)
        ref = _host_step(mr, mr, x, z, 1 | 4, COEFS)
        g = Guarded(K)
        dp, dx, dz = (dn(g, t, dt) for t in (preds, x, z))
        ds, dw = dn(g, torch.tensor(starts, dtype=torch.int32)), dn(g, w)
        with g:
            out = g.out(K.cfg_ddim_step_windows(dp, dx, dz, ds, dw, 1 | 4, COEFS, rescale=phi, ring=ring))
        assert rel(out, ref) < TOL[dt], phi


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ring", [False, True])
def test_cfg_ddim_step_windows_misaligned_pair_and_workspace_tail(dt, ring):
    """The header: "16-byte lanes when inner % 8 == 0 and the tensors are 16-byte aligned, a scalar path otherwise" -- a sample / out
    pair 2 bytes off its alignment forces the scalar path at inner = 8.  And a rescale workspace larger than 8 floats per record:
    the floats past the records are not the kernels' to touch."""
    preds, x, z, starts, w = _windows_case(dt, (1, 8), ring, seed=170)
    lib = K.lib()
    n = x.numel()
    nrec = lib.im360_cfg_rescale_records(n)
    m, cb = _blend64(preds, x, starts, w, COEFS[0], ring)
    refs = [_host_step(mm, mm, x, z, 1 | 4, COEFS) for mm in (m, m * _factor64(m, cb, 0.7))]
    g = Guarded(K)
    dp, dz = dn(g, preds, dt), dn(g, z, dt)
    dx = dn(g, x, dt, misalign=2)
    ds, dw = dn(g, torch.tensor(starts, dtype=torch.int32)), dn(g, w)
    suffix = "_ring" if ring else ""
    geo = (2, 4, 6, 4, 8)
    with g:
        o0, o1 = (g.empty(x.shape, dt, "cuda", misalign=2) for _ in range(2))
        assert dx.data_ptr() % 16 == 2 and o0.data_ptr() % 16 == 2
        ws = g.empty((8 * nrec + 40,), torch.float32, "cuda")
        ptrs = (dp.data_ptr(), dx.data_ptr(), dz.data_ptr())
        K._check(getattr(lib, "im360_cfg_ddim_step_windows" + suffix)(*ptrs, o0.data_ptr(), ds.data_ptr(), dw.data_ptr(), *geo, *COEFS, 1 | 4,
                                                                      K._dt(dx), K._stream(), None), "step_windows")
        K._check(getattr(lib, "im360_cfg_rescale_stats_windows" + suffix)(dp.data_ptr(), ds.data_ptr(), dw.data_ptr(), *geo, COEFS[0], ws.data_ptr(),
                                                                          ws.numel(), K._dt(dx), K._stream(), None), "stats_windows")
        K._check(getattr(lib, "im360_cfg_ddim_step_windows" + suffix + "_rescale")(*ptrs, o1.data_ptr(), ds.data_ptr(), dw.data_ptr(), *geo, *COEFS, 1 | 4,
                                                                                   0.7, ws.data_ptr(), ws.numel(), K._dt(dx), K._stream(), None), "step_rescale")
        g.out(o0, o1)
    assert rel(o0, refs[0]) < TOL[dt] and rel(o1, refs[1]) < TOL[dt]
    tail = ws[8 * nrec:].view(torch.int32)
    assert tail.numel() == 40 and bool((tail == (PATTERN << 16 | PATTERN)).all())
    # the flat step: the same workspace contract through im360_cfg_rescale_stats
    u, c = preds[0, 0].contiguous(), preds[0, 1].contiguous()
    g = Guarded(K)
    du, dc = dn(g, u, dt), dn(g, c, dt)
    nrec = lib.im360_cfg_rescale_records(u.numel())
    with g:
        ws = g.empty((8 * nrec + 24,), torch.float32, "cuda")
        K._check(lib.im360_cfg_rescale_stats(du.data_ptr(), dc.data_ptr(), u.numel(), COEFS[0], ws.data_ptr(), ws.numel(), K._dt(du), K._stream(), None),
                 "im360_cfg_rescale_stats")
    assert bool((ws[8 * nrec:].view(torch.int32) == (PATTERN << 16 | PATTERN)).all())


# ------------------------------------------------------------------------------------------ the detector detects
# No broken kernel and no access outside the test's own buffers: a correct kernel is told a size one larger (or smaller) than the
# interior, so it legitimately steps one row or one key into the guard -- which is at least 256 rows wide.
def test_detector_flags_a_row_written_past_the_end():
    dt, rows, C = torch.bfloat16, 5, 64
    g = Guarded(K)
    # (x holds the extra row, so what lands in y's guard is a finite row and not a NaN that might carry the sentinel's payload)
    x, gam, bet = dn(g, rnd(rows + 1, C, seed=1), dt), dn(g, 1 + 0.1 * rnd(C, seed=2), dt), dn(g, rnd(C, seed=3), dt)
    with pytest.raises(AssertionError) as e:
        with g:
            y = g.empty((rows, C), dt, "cuda")
            K._check(K.lib().im360_layernorm(x.data_ptr(), gam.data_ptr(), bet.data_ptr(), None, None, y.data_ptr(), rows + 1, C, 1, 1, 1, 1e-5,
                                             K._dt(x), K._stream()), "im360_layernorm")
            g.out(y)
    msg = str(e.value)
    assert f"shape ({rows}, {C}) torch.bfloat16: back guard overwritten, bytes {rows * C * 2}..{(rows + 1) * C * 2 - 1} relative to the tensor" in msg, msg
    assert msg.count("overwritten") == 1 and "sentinel" not in msg, msg


def test_detector_flags_a_key_read_past_the_end():
    dt, B, H, D, Nq, Nk = torch.bfloat16, 1, 2, 64, 33, 77
    C = H * D
    g = Guarded(K)
    q, k, v = (dn(g, rnd(B, n, C, seed=s), dt) for n, s in ((Nq, 1), (Nk, 2), (Nk, 3)))
    with g:
        out = g.empty((B, Nq, C), dt, "cuda")
        rc = K.lib().im360_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), None, out.data_ptr(), B, H, Nq, Nk + 1, D, Nq * C, C, Nk * C, C, Nk * C, C,
                                    Nq * C, C, 0, 1, D ** -0.5, 1.0, 0, K._dt(q), K._stream(), None, None, None, None, 0)
        K._check(rc, "im360_attn_fwd")
    ref = sdpa64(q.float().cpu(), k.float().cpu(), v.float().cpu(), H)
    assert bool(out.float().isnan().any())                   # key row Nk is sentinel: a NaN score in every row
    assert not rel(out, ref) < TOL[dt]                       # ... which the comparison form of every test here turns into a failure


def test_detector_flags_a_row_left_unwritten():
    dt, rows, I = torch.bfloat16, 6, 320
    g = Guarded(K)
    h = dn(g, rnd(rows, 2 * I, seed=5), dt)
    with pytest.raises(AssertionError) as e:
        with g:
            out = g.empty((rows, I), dt, "cuda")
            K._check(K.lib().im360_geglu(h.data_ptr(), out.data_ptr(), rows - 1, I, K._dt(h), K._stream()), "im360_geglu")
            g.out(out)
    msg = str(e.value)
    assert f"shape ({rows}, {I}) torch.bfloat16: {I} element(s) still hold the sentinel" in msg, msg
    assert f"bytes {(rows - 1) * I * 2}..{rows * I * 2 - 1} relative to the tensor" in msg and "overwritten" not in msg, msg
