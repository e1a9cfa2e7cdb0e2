"""Parity of the kernel instantiations that only a tuning knob (kernels.KNOBS, each also seeded from an IM360_* environment variable)
or a shape rule of a host launcher selects, against an fp64 reference of the same operation AND against the default kernel on the
same inputs.  Shapes are read off the launchers' conditions (csrc/conv3x3.hip launch_conv / im360_linear_geglu(_ln), attn_fwd.hip
launch_attn_b, attn_pipe.hip, temporal_attn.hip launch_tattn, elementwise.hip launch_ln, groupnorm.hip): at least one that satisfies
the condition and, where the condition has a shape part, a ragged one that must fall back silently to the default kernel.

Conventions of tests/test_kernels_gpu.py (same helpers, same TOL).  Whether a variant must reproduce the default's BITS follows from
the code, not from a measurement: two kernels agree bit for bit when they feed the same products to the same fp32 accumulator in
the same order (tile shape, K-step size, load / store form and workgroup layout do not enter); they differ in the last bits when
the K order (taps innermost against tap-major) or the point where a 16-bit rounding / a softmax rescale happens differs.  Each test
states which of the two it expects and why."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from im360_oracle import unet as OU  # noqa: E402
from imagine360_amd import kernels as K  # noqa: E402
from test_kernels_gpu import DTYPES, TOL, blockrel, q16, rel  # noqa: E402

DEFAULTS = {"conv_big": 1, "conv_bk": 0, "conv_ring": 1, "conv_cm": 1, "conv_small": 2, "ln_packed": 1, "attn_one": 1, "attn_w3": 1,
            "attn_pipe": K.ATTN_PIPE_DEFAULT, "attn_qb": 0, "tattn_nt": 0, "nt": 1, "g4": 0, "gn_wgs": 0, "conv_dbg": 0}


ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}      # one unit in the last place of the storage format, relative to the value (its upper end)


class knobs:
    """``with knobs(g4=1): ...`` -- sets the knobs, restores the library defaults (abi.cpp) on exit."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            K.tuning_set(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            K.tuning_set(k, DEFAULTS[k])
        return False


def gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t, dt):
    return t.to(dt).cuda()


# ------------------------------------------------------------------------------------------ g4: four-wave 256 x 256 / 256 x 128 GEMM tiles
def _geglu_ref(h, inner):
    return h[:, :inner] * F.gelu(h[:, inner:])


def _row_stats(x):
    """Row statistics of x [M, K] (fp32 device tensor values) in the producer's layout: (sum, sum of squares) per 160-column slice."""
    M, Kd = x.shape
    sl = K.ROW_SLICE
    xs = x.float().reshape(M, Kd // sl, sl) if Kd % sl == 0 else x.float().reshape(M, 1, Kd)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1).contiguous()


# (M, K, I, takes the g4 tiles).  Call-site conditions: K % 64 == 0, K >= 128, M % 256 == 0, (M / 256) (2 I / 256) >= 256 for the
# 256 x 256 tile and (M / 256) (2 I / 128) >= 512 for the 256 x 128 one.
G4_SHAPES = [(16384, 128, 512, True),         # K = 128: two stages, the shortest loop (FIRST + LAST only); four cout tiles, 256 tiles exactly
             (32768, 320, 256, True),         # five stages (the odd-count instantiation), two cout tiles
             (8192, 1280, 1024, True),        # deep K: twenty stages, eight cout tiles
             (16384 + 77, 128, 512, False),   # M % 256 != 0: silent fallback to the default kernel
             (8192, 128, 512, False)]         # 128 tiles: below the minimum tile count, fallback


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,Kd,I,taken", G4_SHAPES)
def test_g4_tiles_geglu_projection(dt, M, Kd, I, taken):
    """Knob g4 bit 0 (256 x 256 tile on four waves, gemm_g4_kernel<T, 1>) and bit 2 (256 x 128, two workgroups per CU, gemm_g4b_kernel<T, 1>),
    and conv_ring 12 / 13 as the second way in, for the fused GEGLU projection: fp64 reference per 256-row tile, and the default loop's
    bits (every loop walks K in ascending 64-channel stages into the same 32 x 32 accumulators and shares tile_epilogue)."""
    g = gen(200)
    x = q16(torch.randn(M, Kd, generator=g), dt)
    w = q16(torch.randn(2 * I, Kd, generator=g) * Kd ** -0.5, dt)
    b = q16(torch.randn(2 * I, generator=g) * 0.5, dt)
    ref = _geglu_ref(F.linear(x.double(), w.double(), b.double()), I)
    dx = dev(x, dt)
    wp, bp = K.pack_geglu(dev(w, dt), dev(b, dt))
    base = K.linear_geglu(dx, wp, bp, I)
    e0 = rel(base, ref)
    assert e0 < TOL[dt] and blockrel(base, ref, 256) < 2 * TOL[dt]
    for kv in (dict(g4=1), dict(g4=4), dict(conv_ring=12), dict(conv_ring=13)):
        with knobs(**kv):
            out = K.linear_geglu(dx, wp, bp, I)
        e, be, same = rel(out, ref), blockrel(out, ref, 256), torch.equal(out, base)
        print(f"g4 geglu {dt} M={M} K={Kd} I={I} {kv}: rel {e:.3e} (default {e0:.3e}) blockrel256 {be:.3e} bits-equal-default {same}")
        assert e < TOL[dt] and be < 2 * TOL[dt], kv
        assert same, (kv, taken)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("M,Kd,I,taken", G4_SHAPES)
def test_g4_tiles_geglu_with_folded_layer_norm(dt, M, Kd, I, taken):
    """Knob g4 bit 1 / bit 3 (gemm_g4_kernel<T, 4> / gemm_g4b_kernel<T, 4>; conv_ring 12 / 13): GEGLU(LayerNorm(x)) with the normalisation folded
    into the GEMM, against LayerNorm -> Linear -> GEGLU in fp64 and against the default loop.

    NOT bit-identical to the default loop where the tiles are taken (measured on MI355X: every taken shape, both dtypes; error against fp64
    2.695e-03 / 2.683e-03 / 2.671e-03 in bf16 and 3.357e-04 / 3.376e-04 / 3.356e-04 in fp16 for BOTH kernels, equal to four digits).  The GEMM
    summation order is the same -- the plain GEGLU epilogue on the same two loops is bit-identical (test above).  What differs is the
    fp32 evaluation of `(acc - mu c1) rstd + c2` and of mu / rstd in tile_epilogue / epi_ln_row_stats: one source, compiled with -ffast-math
    into each kernel, and hipcc contracts / reassociates it differently in the two instantiations (same packed FMA / MUL / ADD counts per
    element, different scalar mixes: 13 v_mul + 4 v_fma + 4 v_add against 22 v_mul + 4 v_fmac + 6 v_fmamk).  A last-bit fp32 difference in
    front of the 16-bit rounding moves some outputs by one unit of the storage format, so the two kernels are held to one such unit in
    relative L2, whole tensor and per 256-row tile (2^-7 bf16, 2^-10 fp16: what every output being off by one unit would still meet -- a bound
    from the formats, not from the figures), next to the fp64 check at the usual tolerance."""
    g = gen(201)
    x = q16(torch.randn(M, Kd, generator=g) + 0.3, dt)
    w = q16(torch.randn(2 * I, Kd, generator=g) * Kd ** -0.5, dt)
    b = q16(torch.randn(2 * I, generator=g) * 0.5, dt)
    gam, bet = q16(1 + 0.1 * torch.randn(Kd, generator=g), dt), q16(0.1 * torch.randn(Kd, generator=g), dt)
    ref = _geglu_ref(F.linear(F.layer_norm(x.double(), (Kd,), gam.double(), bet.double(), 1e-5), w.double(), b.double()), I)
    dx = dev(x, dt)
    wf, c1, c2 = K.fold_layer_norm(dev(w, dt), dev(b, dt), dev(gam, dt), dev(bet, dt))
    wfp, c1p = K.pack_geglu(wf, c1)
    c2p = K.interleave_geglu(wf, c2)[1].contiguous()
    st = _row_stats(dx)
    run = lambda: K.linear_geglu_ln(dx, wfp, c1p.contiguous(), c2p, st, 1e-5, I)
    base = run()
    e0 = rel(base, ref)
    assert e0 < TOL[dt] and blockrel(base, ref, 256) < 2 * TOL[dt]
    for kv in (dict(g4=2), dict(g4=8), dict(conv_ring=12), dict(conv_ring=13)):
        with knobs(**kv):
            out = run()
        e, be, same = rel(out, ref), blockrel(out, ref, 256), torch.equal(out, base)
        d = rel(out, base.double().cpu())
        print(f"g4 geglu+LN {dt} M={M} K={Kd} I={I} {kv}: rel {e:.3e} (default {e0:.3e}) blockrel256 {be:.3e} bits-equal-default {same} rel-to-default {d:.3e}")
        assert e < TOL[dt] and be < 2 * TOL[dt], kv
        if taken:
            assert d < ULP[dt] and blockrel(out, base.double().cpu(), 256) < ULP[dt], kv
        else:
            assert same, kv                  # the default kernel itself


def test_g4_knob_bits_are_independent():
    """Every single bit of knob g4, and all four together, leaves the plain GEGLU projection right on a shape the tiles take (bits 1 / 3
    belong to the LayerNorm-folded entry point and must not disturb this one)."""
    dt = torch.bfloat16
    g = gen(202)
    M, Kd, I = 16384, 128, 512
    x, w, b = (q16(t, dt) for t in (torch.randn(M, Kd, generator=g), torch.randn(2 * I, Kd, generator=g) * Kd ** -0.5, torch.randn(2 * I, generator=g)))
    ref = _geglu_ref(F.linear(x.double(), w.double(), b.double()), I)
    wp, bp = K.pack_geglu(dev(w, dt), dev(b, dt))
    for bit in (1, 2, 4, 8, 15):
        with knobs(g4=bit):
            out = K.linear_geglu(dev(x, dt), wp, bp, I)
        assert rel(out, ref) < TOL[dt] and blockrel(out, ref, 256) < 2 * TOL[dt], bit


# ------------------------------------------------------------------------------------------ convolution tile policy
def _conv_case(dt, taps, N, H, W, Cin, Cout, stride, wrap, seed):
    g = gen(seed)
    x = q16(torch.randn(N, H, W, Cin, generator=g), dt)
    w = q16(torch.randn(Cout, Cin, 3 if taps == 9 else 1, 3 if taps == 9 else 1, generator=g) * (taps * Cin) ** -0.5, dt)
    b = q16(torch.randn(Cout, generator=g) * 0.1, dt)
    fr = 1
    for cand in (7, 5, 4, 3, 2):
        if N % cand == 0:
            fr = cand
            break
    temb = q16(torch.randn(N // fr, Cout, generator=g), dt)
    xr = x.double().permute(0, 3, 1, 2)
    pad = taps == 9
    if wrap and pad:        # circular along W: pad_pano(stride) -> conv -> unpad_pano, restated (columns wrap, rows zero-pad)
        if stride == 1:
            xr = torch.cat([xr[..., -1:], xr, xr[..., :1]], dim=-1)
            y = F.conv2d(F.pad(xr, (0, 0, 1, 1)), w.double(), b.double())
        else:
            xr = torch.cat([xr[..., -2:], xr, xr[..., :2]], dim=-1)
            y = F.conv2d(xr, w.double(), b.double(), stride=2, padding=1)[..., 1:-1]
    else:
        y = F.conv2d(xr, w.double(), b.double(), stride=stride, padding=1 if pad else 0)
    y = y.permute(0, 2, 3, 1)
    res = q16(torch.randn(y.shape, generator=g), dt)
    ref = y + temb.double().repeat_interleave(fr, 0)[:, None, None, :] + res.double()
    wp = K.pack_conv_weight(dev(w, dt))
    args = dict(bias=dev(b, dt), temb=dev(temb, dt), imgs_per_temb=fr, res=dev(res, dt), stride=stride, wrap=wrap)
    return dev(x, dt), wp, args, ref


# taps, N, H, W, Cin, Cout, stride, wrap.  Tile rule (launch_conv): 256 x 320 tiles when Cout % 320 == 0, Cin % 64 == 0 and
# ceil(M / 256) (Cout / 320) >= 512; below, Cout % 128 in (0, 64] takes knob conv_small's tile, everything else 128 x 128.
CONV_SHAPES = [(9, 133, 32, 31, 64, 320, 1, False),      # 516 large tiles, the last one ragged (131 936 pixels)
               (9, 131, 32, 31, 64, 320, 1, False),      # 508: just below the rule -> small tiles, Cout % 128 = 64
               (9, 66, 32, 64, 64, 320, 1, True),        # 528 large tiles, circular wrap (tap-major K order)
               (9, 20, 16, 36, 128, 192, 1, True),       # small grid, wrap, Cout % 128 = 64, ragged pixel tile (11 520 = 45 x 256)
               (9, 42, 30, 34, 64, 160, 2, False),       # stride 2, Cout % 128 = 32, ragged (42 x 15 x 17 = 10 710 pixels)
               (9, 21, 15, 17, 96, 320, 1, False),       # Cin % 64 != 0: 32-channel K steps by default
               (1, 130, 32, 32, 64, 320, 1, False),      # 1 x 1 on 520 large tiles
               (1, 35, 24, 23, 128, 320, 1, False),      # 1 x 1 below the rule, ragged (19 320 pixels)
               (1, 10, 24, 23, 64, 448, 1, False)]       # 1 x 1, Cout % 128 = 64 with four cout tiles


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("taps,N,H,W,Cin,Cout,stride,wrap", CONV_SHAPES)
def test_conv_tile_policy_knobs(dt, taps, N, H, W, Cin, Cout, stride, wrap):
    """Knobs conv_big (0: never the 256 x 320 tile; 2 / 3 / 4 name tiles of the ablation build and read as 1 in the shipped library),
    conv_bk 32 (32-channel K steps where the tile has them) and conv_small (0 / 1: 256 x 64 tiles with 32- / 64-channel steps, 2: 128 x 128)
    on 3 x 3 and 1 x 1 convolutions with bias + time embedding + residual: every setting against the fp64 reference per 32-pixel block.
    Bits: a setting keeps the default's bits when it keeps the default's K order.  The default order is taps-innermost for 3 x 3
    convolutions without wrap on whole 64-channel chunks (knob conv_cm) and tap-major otherwise; the 256 x 64 tile and the 32-channel
    kernels are tap-major only, so there they must reproduce the bits of the default kernel run with conv_cm = 0 instead."""
    x, wp, args, ref = _conv_case(dt, taps, N, H, W, Cin, Cout, stride, wrap, 210)
    run = lambda: K.conv2d(x, wp, Cout, **args)
    base = run()
    with knobs(conv_cm=0):
        base_tm = run()
    e0 = rel(base, ref)
    assert e0 < TOL[dt] and blockrel(base, ref, 32) < 2 * TOL[dt]
    assert rel(base_tm, ref) < TOL[dt] and blockrel(base_tm, ref, 32) < 2 * TOL[dt]
    cm_default = taps == 9 and not wrap and Cin % 64 == 0
    assert cm_default or torch.equal(base, base_tm)
    small_tile = 0 < Cout % 128 <= 64 and Cout > 64          # knob conv_small's tile once the 256 x 320 tile is out
    M = x.shape[0] * (H // stride) * (W // stride)
    big = Cout % 320 == 0 and Cin % 64 == 0 and -(-M // 256) * (Cout // 320) >= 512
    settings = [(dict(conv_big=0), True), (dict(conv_big=2), True), (dict(conv_big=3), True), (dict(conv_big=4), True),
                (dict(conv_bk=32), False), (dict(conv_big=0, conv_bk=32), False),
                (dict(conv_small=0), big or not small_tile), (dict(conv_small=1), big or not small_tile), (dict(conv_small=2), True),
                (dict(conv_big=0, conv_small=0), not small_tile), (dict(conv_big=0, conv_small=1), not small_tile)]
    for kv, keeps_cm in settings:
        if K.ablate_build() and kv.get("conv_big", 0) >= 2:
            keeps_cm = False                 # (make ablate: real 128 x 320 / 192 x 320 tiles, tap-major)
        with knobs(**kv):
            out = run()
        want = base if (keeps_cm or not cm_default) else base_tm
        e, be, same = rel(out, ref), blockrel(out, ref, 32), torch.equal(out, want)
        print(f"conv {dt} taps={taps} {N}x{H}x{W} {Cin}->{Cout} s{stride} wrap={wrap} {kv}: rel {e:.3e} (default {e0:.3e}) blockrel32 {be:.3e} "
              f"bits-equal-{'default' if want is base else 'tap-major default'} {same} (equal default: {torch.equal(out, base)})")
        assert e < TOL[dt] and be < 2 * TOL[dt], kv
        assert same, kv


# ------------------------------------------------------------------------------------------ LayerNorm, packed rows
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows", [1, 5, 1003])
def test_layer_norm_packed_rows_knob(dt, rows):
    """Knob ln_packed at C = 320: 1 (default) = layernorm_packed_kernel (eight lanes per row), 0 = the row-per-wave kernel; plain, with a
    ``pre`` table and with a ``post`` table, against fp64.  The two kernels reduce a row over different lane groups (another order of the
    fp32 partial sums), so they are compared through the reference and with each other at a quarter of the tolerance, not bit for bit."""
    C = 320
    g = gen(220)
    x = q16(torch.randn(rows, C, generator=g) * 1.3 + 0.2, dt)
    gam, bet = q16(1 + 0.1 * torch.randn(C, generator=g), dt), q16(0.1 * torch.randn(C, generator=g), dt)
    pre, post = q16(torch.randn(7, C, generator=g), dt), q16(torch.randn(5, C, generator=g), dt)
    r = torch.arange(rows)
    ln = lambda t: F.layer_norm(t.double(), (C,), gam.double(), bet.double(), 1e-5)
    cases = [(dict(), ln(x)), (dict(pre=dev(pre, dt)), ln(x.double() + pre.double()[r % 7])),
             (dict(post=dev(post, dt), post_div=3), ln(x) + post.double()[(r // 3) % 5])]
    dx, dg, db = dev(x, dt), dev(gam, dt), dev(bet, dt)
    for kw, ref in cases:
        outs = {}
        for v in (1, 0):
            with knobs(ln_packed=v):
                outs[v] = K.layer_norm(dx, dg, db, 1e-5, **kw)
            e, be = rel(outs[v], ref), blockrel(outs[v], ref, 1)
            print(f"ln_packed={v} {dt} rows={rows} {sorted(kw)}: rel {e:.3e} worst row {be:.3e}")
            assert e < TOL[dt] and be < 2 * TOL[dt], (v, sorted(kw))          # no single row may be off (the last, partly filled group of rows)
        print(f"   bits equal: {torch.equal(outs[0], outs[1])}")
        assert rel(outs[0], outs[1].float().cpu()) < TOL[dt] / 4


# ------------------------------------------------------------------------------------------ attention: one key tile, one block per wave
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Nq", [16, 48, 200])              # one-, two- and four-wave workgroups
@pytest.mark.parametrize("Nk", [63, 64, 65])               # one key short of a tile, exactly one tile, one past it (the default kernel again)
def test_attention_single_key_tile_knob(dt, Nq, Nk):
    """Knob attn_one: d = 64 without a bias and Nk <= 64 runs the single-buffer kernel (1, default) or the general one (0): same products,
    same online-softmax steps over the one tile -- the same bits; with 65 keys the knob must not matter."""
    B, H, D = 2, 3, 64
    g = gen(230)
    q, k, v = (q16(torch.randn(B, n, H * D, generator=g), dt) for n in (Nq, Nk, Nk))
    ref = OU.sdpa(q.double(), k.double(), v.double(), H)
    outs = {}
    for one in (1, 0):
        with knobs(attn_one=one):
            outs[one] = K.attention(dev(q, dt), dev(k, dt), dev(v, dt), H)
        e, be = rel(outs[one], ref), blockrel(outs[one], ref, 32)
        print(f"attn_one={one} {dt} Nq={Nq} Nk={Nk}: rel {e:.3e} blockrel32 {be:.3e}")
        assert e < TOL[dt] and be < 2 * TOL[dt], one
    same = torch.equal(outs[0], outs[1])
    print(f"   bits equal: {same}")
    assert same


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,H,Nq,Nk", [(2, 2, 300, 200),        # four-wave grid below the two-block rule: W3 kernel against the plain one-block kernel
                                       (8, 16, 2048, 136),      # B H ceil(Nq / 256) = 1024: attn_w3 0 takes two query blocks per wave here
                                       (2, 2, 64, 200)])        # two-wave workgroups: not a four-wave grid, the knob must not matter
def test_attention_one_block_per_wave_knob(dt, B, H, Nq, Nk):
    """Knob attn_w3 for d = 64 without a bias: 1 (default) one query block per wave at three waves per SIMD, 0 the round-2 rule.  Against
    the one-block kernel the arithmetic is the same (same bits); the two-block kernel of large grids rescales its running sums at other
    points (tests/test_kernels_gpu.py::test_attention_two_query_blocks_per_wave_variant), so there the two are compared through the
    reference and with each other at the tolerance."""
    D = 64
    g = gen(231)
    q, k, v = (q16(torch.randn(B, n, H * D, generator=g), dt) for n in (Nq, Nk, Nk))
    k[0, Nk - 7, :D] = q[0, 5, :D] * 5.0                  # head 0: the running max jumps in the last tile
    k = q16(k, dt)
    ref = OU.sdpa(q.double(), k.double(), v.double(), H)
    outs = {}
    for w3 in (1, 0):
        with knobs(attn_w3=w3):
            outs[w3] = K.attention(dev(q, dt), dev(k, dt), dev(v, dt), H)
        e, be = rel(outs[w3], ref), blockrel(outs[w3], ref, 32)
        print(f"attn_w3={w3} {dt} B={B} H={H} Nq={Nq} Nk={Nk}: rel {e:.3e} blockrel32 {be:.3e}")
        assert e < TOL[dt] and be < 2 * TOL[dt], w3
    same = torch.equal(outs[0], outs[1])
    print(f"   bits equal: {same}")
    two_blocks = Nq > 64 and B * H * ((Nq + 255) // 256) >= 1024
    if two_blocks:
        assert rel(outs[0], outs[1].float().cpu()) < TOL[dt]
    else:
        assert same


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("knob", [18, 11, 12, 26, 41])
def test_attention_pipelined_kernel_remaining_schedules(dt, knob):
    """The attn_pipe instantiations tests/test_kernels_gpu.py::test_attention_pipelined_kernel does not name: four waves with schedule 1 and
    read-ahead 3 (18), eight waves with schedules 2 / 3 (11 / 12), schedule 1 with read-ahead 3 (26) and read-ahead 4 (41).  Same checks."""
    B, H, Nq, Nk, D = 2, 3, 320, 448, 64
    g = gen(232)
    q, k, v = (q16(torch.randn(B, n, H * D, generator=g), dt) for n in (Nq, Nk, Nk))
    k[0, Nk - 70, :D] = q[0, 5, :D] * 5.0
    k[0, 9, :D] = q[0, 40, :D] * 7.0
    k = q16(k, dt)
    ref = OU.sdpa(q.double(), k.double(), v.double(), H)
    qd, kd, vd = dev(q, dt), dev(k, dt), dev(v, dt)
    with knobs(attn_pipe=0):
        base = K.attention(qd, kd, vd, H)
    with knobs(attn_pipe=knob):
        out = K.attention(qd, kd, vd, H)
    assert rel(out, ref) < TOL[dt] and blockrel(out, ref, 32) < 2 * TOL[dt]
    assert (out.double().cpu() - ref).abs().max() < 0.05
    assert rel(out, base) < 2e-3


# ------------------------------------------------------------------------------------------ temporal attention load / store forms
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("B,Fr,P,heads,d", [(2, 16, 96, 8, 40), (3, 8, 33, 8, 8), (1, 13, 20, 8, 16), (2, 16, 7, 8, 160),
                                            (1, 24, 20, 8, 40)])          # 24 frames: the long kernel, which has no such forms (fallback)
def test_temporal_attention_nontemporal_forms(dt, B, Fr, P, heads, d):
    """Knob tattn_nt (F <= 16, temporal_attn_mfma_kernel<T, 0 .. 3>): bit 0 = non-temporal output stores, bit 1 = non-temporal q | k | v loads.
    Only the cache policy of the memory instructions changes: fp64 reference and the default's bits."""
    C = heads * d
    g = gen(240)
    qkv = q16(torch.randn(B * Fr * P, 3 * C, generator=g), dt)
    t = qkv.double().reshape(B, Fr, P, 3 * C).permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    ref = OU.sdpa(t[..., :C], t[..., C:2 * C], t[..., 2 * C:], heads).reshape(B, P, Fr, C).permute(0, 2, 1, 3).reshape(B * Fr * P, C)
    dq = dev(qkv, dt)
    base = K.temporal_attention(dq, B, Fr, P, heads)
    assert rel(base, ref) < TOL[dt]
    for v in (1, 2, 3):
        with knobs(tattn_nt=v):
            out = K.temporal_attention(dq, B, Fr, P, heads)
        assert rel(out, ref) < TOL[dt] and blockrel(out, ref, 32) < 2 * TOL[dt], v
        assert torch.equal(out, base), v


# ------------------------------------------------------------------------------------------ epilogue store form
@pytest.mark.parametrize("dt", DTYPES)
def test_epilogue_nontemporal_store_knob(dt):
    """Knob nt (default 1): the conv / GEMM epilogues' output rows leave with non-temporal stores (both store sites of tile_epilogue: the
    plain one and the GEGLU one).  0 = plain stores: the same values, on a 3 x 3 convolution with residual (large and small tile), a
    token-major Linear and the GEGLU projection -- fp64 reference and identical bits."""
    g = gen(250)
    for (N, H, W) in ((133, 32, 31), (9, 15, 17)):
        x, wp, args, ref = _conv_case(dt, 9, N, H, W, 64, 320, 1, False, 251)
        base = K.conv2d(x, wp, 320, **args)
        with knobs(nt=0):
            out = K.conv2d(x, wp, 320, **args)
        assert rel(out, ref) < TOL[dt] and blockrel(out, ref, 32) < 2 * TOL[dt] and torch.equal(out, base), (N, H, W)
    M, Kd, I = 40000 + 77, 128, 256
    x = q16(torch.randn(M, Kd, generator=g), dt)
    w = q16(torch.randn(2 * I, Kd, generator=g) * Kd ** -0.5, dt)
    b = q16(torch.randn(2 * I, generator=g) * 0.1, dt)
    r = q16(torch.randn(M, 320, generator=g), dt)
    wp, bp = K.pack_geglu(dev(w, dt), dev(b, dt))
    lw = K.pack_conv_weight(dev(w[:320], dt).reshape(320, Kd, 1, 1).contiguous())
    ref_g = _geglu_ref(F.linear(x.double(), w.double(), b.double()), I)
    ref_l = F.linear(x.double(), w[:320].double(), b[:320].double()) + r.double()
    base = (K.linear_geglu(dev(x, dt), wp, bp, I), K.linear(dev(x, dt), lw, 320, bias=dev(b[:320], dt), res=dev(r, dt)))
    with knobs(nt=0):
        out = (K.linear_geglu(dev(x, dt), wp, bp, I), K.linear(dev(x, dt), lw, 320, bias=dev(b[:320], dt), res=dev(r, dt)))
    for o, bs, ref in zip(out, base, (ref_g, ref_l)):
        assert rel(o, ref) < TOL[dt] and blockrel(o, ref, 256) < 2 * TOL[dt] and torch.equal(o, bs)


# ------------------------------------------------------------------------------------------ GroupNorm apply: slabs per image
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,H,W,C1,C2,pad", [(3, 8, 16, 64, 0, 0), (2, 16, 32, 320, 0, 2), (2, 9, 7, 64, 96, 0), (1, 64, 128, 320, 0, 2)])
def test_group_norm_apply_workgroup_target_knob(dt, N, H, W, C1, C2, pad):
    """Knob gn_wgs (im360_groupnorm_apply_partials): the target number of workgroups, i.e. how many slabs an image is normalised in
    (1 = one slab per image, 7 = an odd split with a ragged last slab, 100000 = more than the default).  Every workgroup rebuilds the
    image's scale / shift from the same partial sums in the same order, so the split cannot change a bit; fp64 reference."""
    g = gen(260)
    C = C1 + C2
    xa = q16(torch.randn(N, H, W, C1, generator=g) + 0.5, dt)
    xb = q16(torch.randn(N, H, W, C2, generator=g) - 0.25, dt) if C2 else None
    gam, bet = q16(1 + 0.1 * torch.randn(C, generator=g), dt), q16(0.1 * torch.randn(C, generator=g), dt)
    xc = (xa if xb is None else torch.cat([xa, xb], dim=-1)).double().permute(0, 3, 1, 2)
    if pad:
        xc = torch.cat([xc[..., -pad:], xc, xc[..., :pad]], dim=-1)
    ref = F.silu(F.group_norm(xc, 32, gam.double(), bet.double(), 1e-5)).permute(0, 2, 3, 1)
    xin = dev(xa, dt) if xb is None else (dev(xa, dt), dev(xb, dt))
    run = lambda: K.group_norm(xin, dev(gam, dt), dev(bet, dt), 32, 1e-5, silu=True, pad=pad)
    assert K.GN_MODE == "partials" and not K.GN_FUSED
    base = run()
    assert base.shape == ref.shape and rel(base, ref) < TOL[dt]
    for tgt in (1, 7, 100000):
        with knobs(gn_wgs=tgt):
            out = run()
        assert rel(out, ref) < TOL[dt] and blockrel(out, ref, 32) < 2 * TOL[dt], tgt
        assert torch.equal(out, base), tgt


# ------------------------------------------------------------------------------------------ shard_pack in one process
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("Wr", [1, 2, 3])
@pytest.mark.parametrize("B,Fl,P,C", [(2, 3, 37, 64), (1, 4, 100, 320), (3, 1, 5, 8)])
def test_shard_pack_and_unpack_against_torch_indexing(dt, Wr, B, Fl, P, C):
    """im360_shard_pack: tokens [B, Fl, P, C] -> exchange buffer [W, Fl, B, PP, C] (rank r holds pixels r PP ..; the tail past P zero-filled)
    and back, against plain indexing, bit exact; P % W != 0 for W = 2, 3 on the first and last shape."""
    PP = -(-P // Wr)
    g = gen(270)
    tok = torch.randn(B, Fl, P, C, generator=g).to(dt)
    want = torch.zeros(Wr, Fl, B, PP, C, dtype=dt)
    for r in range(Wr):
        n = max(0, min(PP, P - r * PP))
        want[r, :, :, :n] = tok[:, :, r * PP:r * PP + n].permute(1, 0, 2, 3)
    buf = torch.full((Wr, Fl, B, PP, C), float("nan"), dtype=dt, device="cuda")       # the kernel must write the zero tail itself
    K.shard_pack(tok.cuda(), buf, B, Fl, P, Wr, PP)
    assert torch.equal(buf.cpu().view(torch.int16), want.view(torch.int16))
    back = torch.full((B, Fl, P, C), float("nan"), dtype=dt, device="cuda")
    K.shard_pack(buf, back, B, Fl, P, Wr, PP, unpack=True)
    assert torch.equal(back.cpu().view(torch.int16), tok.view(torch.int16))


# ------------------------------------------------------------------------------------------ closing the first launch ledger
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("Nq", [20, 48, 200])              # one-, two- and four-wave workgroups (launch_attn_b: Nq <= 32, <= 64, else)
def test_attention_bias_and_no_bias_at_every_workgroup_size(dt, D, Nq):
    """attn_fwd_kernel with the UNPACKED shared bias at both head dims and every workgroup size, the packed bias and no bias at d = 32 on
    one-wave workgroups, and two query blocks per wave forced (knob attn_qb 2) on the four-wave ones: the instantiations the first launch
    ledger showed no parity test reached.  fp64 reference per 32-query block; one against two blocks per wave through the reference
    (they rescale at different points)."""
    B, H, Nk = 2, 3, 136
    g = gen(280)
    q, k, v = (q16(torch.randn(B, n, H * D, generator=g), dt) for n in (Nq, Nk, Nk))
    bias = q16(torch.rand(Nq, Nk, generator=g) * 2 - 1, dt)
    dq, dk, dv, db = dev(q, dt), dev(k, dt), dev(v, dt), dev(bias, dt)
    cases = [("bias", dict(bias=db), bias), ("none", dict(), None)]
    if D == 32:
        cases.append(("packed", dict(bias=K.pack_attn_bias(db), bias_packed=True), bias))
    for name, kw, bref in cases:
        ref = OU.sdpa(q.double(), k.double(), v.double(), H, bias=None if bref is None else bref.double())
        for qb in ((1, 2) if Nq > 64 else (0,)):
            with knobs(attn_qb=qb):
                out = K.attention(dq, dk, dv, H, **kw)
            assert rel(out, ref) < TOL[dt] and blockrel(out, ref, 32) < 2 * TOL[dt], (name, qb)
            assert (out.double().cpu() - ref).abs().max() < 0.05, (name, qb)


@pytest.mark.parametrize("dt", DTYPES)
def test_attention_two_kv_sets_remaining_forms(dt):
    """im360_attn_fwd2: the generic two-pass kernel on one-wave workgroups (Nq = 20: not a whole query block, so not the resident kernel),
    and the resident kernel's general-key-count instance with 8-byte output stores (knob attn_x 2; same values as the 16-byte form)."""
    H, D, group = 4, 64, 2
    C = H * D
    g = gen(281)
    for B, Nq, n1, n2 in ((4, 20, 77, 64), (6, 320, 90, 48)):
        q = q16(torch.randn(B, Nq, C, generator=g) * 0.3, dt)
        k1, v1, k2, v2 = (q16(torch.randn(B // group, n, C, generator=g), dt) for n in (n1, n1, n2, n2))
        rep = lambda t: t.double().repeat_interleave(group, 0)
        ref = OU.sdpa(q.double(), rep(k1), rep(v1), H) + 0.5 * OU.sdpa(q.double(), rep(k2), rep(v2), H)
        outs = []
        for x in (1, 2):
            with knobs_attn_x(x):
                outs.append(K.attention2(dev(q, dt), dev(k1, dt), dev(v1, dt), dev(k2, dt), dev(v2, dt), H, out_scale2=0.5, kv_group=group))
            assert rel(outs[-1], ref) < 1.5 * TOL[dt] and blockrel(outs[-1], ref, 32) < 3 * TOL[dt], (Nq, x)      # (bounds of test_attention_two_kv_sets_one_launch)
        assert torch.equal(outs[0], outs[1]), Nq


class knobs_attn_x:
    def __init__(self, v):
        self.v = v

    def __enter__(self):
        K.tuning_set("attn_x", self.v)

    def __exit__(self, *exc):
        K.tuning_set("attn_x", 3)          # the library's default
        return False


@pytest.mark.parametrize("dt", DTYPES)
def test_cfg_ddim_update_both_dtypes(dt):
    """im360_cfg_ddim_update (x_prev = cx sample + cv (uncond + g (cond - uncond))) in bf16 and fp16, scalar and device-side coefficients,
    on an element count that is not a multiple of the vector width times the workgroup size."""
    g = gen(282)
    u, c, s = (q16(torch.randn(1, 4, 16, 9, 17, generator=g), dt) for _ in range(3))
    gd, cx, cv = 7.5, 0.83, -0.41
    ref = cx * s.double() + cv * (u.double() + gd * (c.double() - u.double()))
    out = K.cfg_ddim_update(dev(u, dt), dev(c, dt), dev(s, dt), gd, cx, cv)
    assert rel(out, ref) < TOL[dt] and blockrel(out.reshape(-1, 17), ref.reshape(-1, 17), 32) < 2 * TOL[dt]
    coef = torch.tensor([gd, cx, cv], dtype=torch.float32, device="cuda")
    assert torch.equal(K.cfg_ddim_update(dev(u, dt), dev(c, dt), dev(s, dt), 0.0, 0.0, 0.0, coef_dev=coef), out)


@pytest.mark.parametrize("dt", DTYPES)
def test_linear_epilogues_without_residual_and_with_both_statistics(dt):
    """im360_linear_fwd's epilogue combinations the first ledger showed unlaunched: no residual with GroupNorm partial sums, with LayerNorm
    row statistics, with both; and both statistics with a residual on round 3's ring loop (knob conv_ring 8).  Output against fp64 per
    256-row tile; row statistics against sums over the stored output; the partial sums through the GroupNorm they feed, against fp64
    GroupNorm of the stored output."""
    g = gen(283)
    Nimg, HW, Kd, N = 8, 1024, 320, 320
    M = Nimg * HW
    x = q16(torch.randn(M, Kd, generator=g), dt)
    w = q16(torch.randn(N, Kd, generator=g) * Kd ** -0.5, dt)
    b = q16(torch.randn(N, generator=g) * 0.5, dt)
    r = q16(torch.randn(M, N, generator=g) + 0.7, dt)
    gam, bet = q16(1 + 0.1 * torch.randn(N, generator=g), dt), q16(0.1 * torch.randn(N, generator=g), dt)
    dx, db, dr = dev(x, dt), dev(b, dt), dev(r, dt)
    wp = K.pack_conv_weight(dev(w, dt).reshape(N, Kd, 1, 1))
    ref0 = F.linear(x.double(), w.double(), b.double())

    def check(y, ref, st=None, gn=False):
        assert rel(y, ref) < TOL[dt] and blockrel(y, ref, 256) < 2 * TOL[dt]
        if st is not None:
            t = y.double().reshape(M, N // 160, 160)
            want = torch.stack([t.sum(-1), (t * t).sum(-1)], dim=-1)
            assert st.shape == (M, N // 160, 2) and (st.double() - want).abs().max() <= 2e-5 * want.abs().max()      # (bound of test_linear_row_statistics)
        if gn:
            assert K._gn_of(y) is not None
            img = K.carry_gn(y.reshape(Nimg, 32, 32, N), y)
            out = K.group_norm(img, dev(gam, dt), dev(bet, dt), 32, 1e-5)
            want = F.group_norm(y.double().cpu().reshape(Nimg, HW, N).permute(0, 2, 1), 32, gam.double(), bet.double(), 1e-5).permute(0, 2, 1)
            assert rel(out.reshape(Nimg, HW, N), want) < TOL[dt]

    plain = K.linear(dx, wp, N, bias=db)
    check(plain, ref0)
    y = K.linear(dx, wp, N, bias=db, gn_hw=HW)
    check(y, ref0, gn=True)
    assert torch.equal(y, plain)
    y, st = K.linear(dx, wp, N, bias=db, row_stats=True)
    check(y, ref0, st=st)
    assert torch.equal(y, plain)
    y, st = K.linear(dx, wp, N, bias=db, row_stats=True, gn_hw=HW)
    check(y, ref0, st=st, gn=True)
    assert torch.equal(y, plain)
    with knobs(conv_ring=8):
        y, st = K.linear(dx, wp, N, bias=db, res=dr, row_stats=True, gn_hw=HW)
    check(y, ref0 + r.double(), st=st, gn=True)
    assert torch.equal(y, K.linear(dx, wp, N, bias=db, res=dr))
