"""Bit-exact tests of the MFMA kernel families on inputs whose correct result is known exactly (tests/_exact_cases.py; its CPU
self-checks, including the proof that each case catches single-element defects, are in tests/test_exact_cases.py).

  * imagine360_amd/csrc/conv3x3.hip (K.conv2d, K.conv_up2, K.conv1x1_cat, K.linear): integer inputs; the expected bits are RNE(exact
    integer), with the epilogue's documented rounding points (residual added to the 16-bit value, imagine360_amd/csrc/conv3x3.hip:464-473).  "exact" cases: every
    output representable; "round" cases: a fifth of the outputs exact ties of the 16-bit type -- truncation, round-half-up or another
    rounding point fail.
  * attn_fwd.hip / attn_pipe.hip / temporal_attn.hip: queries and keys are signed two-hot codes, every non-selected weight underflows to
    exactly 0 in fp32, the expected output is a gather of V built by indexing.
  * groupnorm.hip: integer partial sums, wrapped columns counted twice; one structured tolerance test of the padded statistics.

Every comparison is ``torch.equal`` over all elements (the structured GroupNorm test apart).  A knob that does not apply to a shape must
not change a bit either, so every case runs under every knob setting of its family; all knobs are restored in a ``finally``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _exact_cases as E  # noqa: E402
from imagine360_amd import kernels as K  # noqa: E402

TOL = {E.BF16: 1e-2, E.FP16: 3e-3}          # tests/test_kernels_gpu.py
DEFAULTS = {"conv_big": 1, "conv_bk": 0, "conv_ring": 1, "conv_cm": 1, "conv_small": 2, "conv_halo": 0, "conv_ksplit": 1, "attn_one": 1, "attn_qb": 0,
            "attn_pipe": K.ATTN_PIPE_DEFAULT, "attn_x": 3, "tattn_scalar": 0}          # the library's defaults (csrc/abi.cpp)
ids = lambda d: str(d).split(".")[-1]
sid = lambda s: "x".join(str(v) if not isinstance(v, tuple) else "s" + "_".join(map(str, v)) for v in s)


class knobs:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            K.tuning_set(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            K.tuning_set(k, DEFAULTS[k])
        return False


def same(out, want, what=""):
    """torch.equal over ALL elements, with a message that says how many and where."""
    out = out.detach().cpu()
    assert out.dtype == want.dtype and out.shape == want.shape, (what, out.dtype, out.shape, want.dtype, want.shape)
    if not torch.equal(out, want):
        bad = (out != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {out.numel()} elements differ, first at {i}: got {out[i].item()}, want {want[i].item()}; "
                             f"last at {tuple(bad[-1].tolist())}")


def dev(t, dt):
    return None if t is None else t.to(dt).cuda()


# ================================================================================================ 1. integer convolution / GEMM
def conv_ref(name, dt, kind):
    c = E.conv_case(name, dt, kind)
    return c, c.expected()


def run_conv(c):
    x, wp, kw = E.conv_gpu_args(c, K)
    return K.conv2d(x, wp, c.Cout, **kw)


def conv_params(table, prefix):
    return pytest.mark.parametrize("name", [f"{prefix}/{n}" for n in table])


KIND = pytest.mark.parametrize("kind", E.KINDS)
DT = pytest.mark.parametrize("dt", E.DTYPES, ids=ids)


@KIND
@DT
@conv_params(E.CONV_FORMS, "forms")
def test_conv2d_addressing_forms(name, dt, kind):
    """K.conv2d on the default 128 x 128 tile at a fully ragged shape: plain, wrap, stride 2 (with and without wrap), nearest upsample (with and
    without wrap), the window of a pre-padded input, 1 x 1, and the temb / residual epilogue.  The residual is added AFTER the first 16-bit
    rounding (imagine360_amd/csrc/conv3x3.hip:464-473), which the reference models; "res_cout_not_8" takes the direct-store epilogue (conv3x3.hip:585-589), which
    rounds once."""
    c, want = conv_ref(name, dt, kind)
    same(run_conv(c), want, name)


def big_tile_count(c):
    ho, wo = c.out_hw()
    return -(-(c.N * ho * wo) // 256) * (c.Cout // 320) if c.Cout % 320 == 0 and c.Cin % 64 == 0 else 0


@KIND
@DT
@pytest.mark.parametrize("small", [2, 0, 1])
@conv_params(E.SMALL_TILE, "small")
def test_conv2d_256x64_tile(name, small, dt, kind):
    """Knob conv_small 0 / 1 (256 x 64 tiles with 32- / 64-channel K steps) for Cout % 128 in (0, 64] below the 256 x 320 tile's rule
    (launch_conv, imagine360_amd/csrc/conv3x3.hip:1909-1911), and 2 = the default 128 x 128 tile."""
    c, want = conv_ref(name, dt, kind)
    assert 0 < c.Cout % 128 <= 64 and c.Cout > 64 and big_tile_count(c) < 512
    with knobs(conv_small=small):
        same(run_conv(c), want, f"{name} conv_small={small}")


@KIND
@DT
@pytest.mark.parametrize("ksplit", [0, 2, 3, 4, 9])
@conv_params(E.KSPLIT, "ksplit")
def test_conv2d_forced_k_split(name, ksplit, dt, kind):
    """Knob conv_ksplit 2 / 3 / 4 on the 256 x 320 tile (Cin = 256: four 64-channel chunks, so three parts are uneven), 9 = the planner's rule with
    wrap-addressed launches included, 0 = unsplit (the 128 x 128 tile at this tile count).  The parts' fp32 partial sums are integers, so the
    split result equals the unsplit integer result bit for bit.  The plan must really split: asserted through im360_conv_ksplit_plan."""
    c, want = conv_ref(name, dt, kind)
    ho, wo = c.out_hw()
    assert 64 <= big_tile_count(c) <= 248 and c.Cin // 64 >= 4
    with knobs(conv_ksplit=ksplit):
        parts = K.lib().im360_conv_ksplit_plan(c.N, ho, wo, c.Cin, c.Cout, 9, 0, int(c.wrap), 0)
        assert parts == (1 if ksplit == 0 else ksplit if ksplit <= 4 else parts) and (ksplit == 0 or parts > 1), (ksplit, parts)
        same(run_conv(c), want, f"{name} conv_ksplit={ksplit} parts={parts}")


@KIND
@DT
@conv_params(E.BIG_TILE, "big")
def test_conv2d_256x320_tile_unsplit(name, dt, kind):
    """At least 512 tiles: the eight-wave 256 x 320 kernel, chunk-major (plain) and tap-major (wrap), with temb and residual."""
    c, want = conv_ref(name, dt, kind)
    assert big_tile_count(c) >= 512
    same(run_conv(c), want, name)


K_ORDER_KNOBS = [dict(), dict(conv_cm=0), dict(conv_bk=32)]


@KIND
@DT
@pytest.mark.parametrize("kv", K_ORDER_KNOBS, ids=lambda kv: "_".join(f"{k}{v}" for k, v in kv.items()) or "default")
@conv_params(E.K_ORDER, "korder")
def test_conv2d_k_orders(name, kv, dt, kind):
    """Knob conv_cm 1 (default: taps innermost for 3 x 3 convolutions without wrap on whole 64-channel chunks) / 0 (tap-major) and conv_bk 32
    (32-channel K steps), on the 128 x 128 tile: another fp32 summation order of the same integers -- the same bits."""
    c, want = conv_ref(name, dt, kind)
    assert c.Cin % 64 == 0 and not c.wrap and big_tile_count(c) < 512
    with knobs(**kv):
        same(run_conv(c), want, f"{name} {kv}")


@KIND
@DT
@conv_params(E.HALO, "halo")
def test_conv2d_halo_patch_kernel(name, dt, kind):
    """Knob conv_halo 1: the halo-patch kernel (conv_halo_kernel, imagine360_amd/csrc/conv3x3_ablate.hip:624).  It exists only in `make ablate`
    builds of the library and is asked only by launches that fill 256 x 320 tiles (launch_conv -> ablate_conv), so the shapes are the first and
    the pre-padded-window shape of tests/test_kernels_gpu.py::test_conv3x3_halo_patch_kernel.  The shipped library does not contain the
    kernel: there this test is skipped, like that one."""
    if not K.ablate_build():
        pytest.skip("the halo-patch kernel is compiled by `make ablate` only")
    c, want = conv_ref(name, dt, kind)
    # the shapes the kernel takes (halo_geometry, conv3x3_ablate.hip:519-530): whole 256-pixel tiles of R = 256 / W rows, patch of at most 528 pixels
    R = 256 // c.W
    seg = min(R, c.H)
    assert big_tile_count(c) >= 512 and c.taps == 9 and c.stride == 1 and not c.up and not c.wrap and 256 % c.W == 0 and (c.N * c.H * c.W) % 256 == 0
    assert (c.H % R == 0 or R % c.H == 0) and (R // seg) * (seg + 2) * (c.W + 2) <= 528
    with knobs(conv_halo=1):
        same(run_conv(c), want, f"{name} conv_halo=1")


@KIND
@DT
@conv_params(E.UP2, "up2")
def test_conv_up2_subpixel_kernels(name, dt, kind):
    """K.conv_up2: the four 2 x 2 sub-pixel convolutions with pre-summed taps (integers again) against nearest-x2 + conv3x3."""
    c, want = conv_ref(name, dt, kind)
    w4 = K.pack_conv_up2_weight(dev(c.w, dt))
    same(K.conv_up2(dev(c.x, dt), w4, c.Cout, bias=dev(c.bias, dt), wrap=c.wrap), want, name)


@KIND
@DT
@pytest.mark.parametrize("name", list(E.CAT))
def test_conv1x1_cat_pair(name, dt, kind):
    c, C1 = E.cat_case(name, dt, kind)
    assert K.can_conv1x1_cat(C1, c.Cin - C1) and C1 != c.Cin - C1
    xa, xb = dev(c.x[..., :C1].contiguous(), dt), dev(c.x[..., C1:].contiguous(), dt)
    out = K.conv1x1_cat(xa, xb, K.pack_conv_weight(dev(c.w, dt)), c.Cout, bias=dev(c.bias, dt), res=dev(c.res, dt))
    same(out, c.expected(), name)


@KIND
@DT
@pytest.mark.parametrize("ring", [1, 8], ids=["staggered", "ring"])
@pytest.mark.parametrize("M,Kd,n", E.LINEAR)
def test_linear_every_loop_and_row_statistics(M, Kd, n, ring, dt, kind):
    """K.linear with bias, with and without the residual (added after the first rounding, imagine360_amd/csrc/conv3x3.hip:464-473) and with row
    statistics, on the staggered loop (conv_ring 1, default) and the ring loop (8); M = 65536 + 77 ends 77 rows past a tile boundary.  In the
    "exact" cases the statistics -- sum and sum of squares of the stored integers per row and 160-column slice -- are exact in fp32 and
    compared bit for bit."""
    c = E.linear_case(M, Kd, n, dt, kind)
    p32 = c.pre(torch.float32)
    want, want_nores = c.finish(p32), E.rne(p32, dt)
    x, b, r = dev(c.x, dt), dev(c.bias, dt), dev(c.res, dt)
    wp = K.pack_conv_weight(dev(c.w, dt).reshape(n, Kd, 1, 1))
    with knobs(conv_ring=ring):
        same(K.linear(x, wp, n, bias=b, res=r), want, "residual")
        same(K.linear(x, wp, n, bias=b), want_nores, "no residual")
        y, st = K.linear(x, wp, n, bias=b, res=r, row_stats=True)
        same(y, want, "residual + row statistics")
        if kind == "exact":
            same(st, E.row_stats(want).float(), "row statistics")
        y, st = K.linear(x, wp, n, bias=b, row_stats=True)
        same(y, want_nores, "row statistics, no residual")
        if kind == "exact":
            same(st, E.row_stats(want_nores).float(), "row statistics of the output without residual")


# ================================================================================================ 2. attention as exact selection
ATTN_KNOBS = [dict(), dict(attn_qb=1), dict(attn_qb=2), dict(attn_one=0), dict(attn_pipe=0)]
kvid = lambda kv: "_".join(f"{k}{v}" for k, v in kv.items()) or "default"


def fused_rows(t, dt, slot, g):
    """``t`` [B, N, C] as the view [..., slot C : (slot + 1) C] of fused-projection rows [B, N, 3 C] (row stride 3 C); the other two thirds hold
    other integers."""
    B, N, C = t.shape
    wide = E.ints((B, N, 3 * C), -64, 64, g)
    wide[..., slot * C:(slot + 1) * C] = t
    return wide.to(dt).cuda()[..., slot * C:(slot + 1) * C]


@DT
@pytest.mark.parametrize("kv", ATTN_KNOBS, ids=kvid)
@pytest.mark.parametrize("shape", E.ATTN_SHAPES, ids=sid)
def test_attention_selects_exact_rows(shape, kv, dt):
    """K.attention (attn_fwd_kernel) at d = 64 / 32 on one-, two- and four-wave workgroups, key counts around the 64-key tile and 1288 (20 tiles +
    8 keys), kv_group 2, q / k / v as strided views of fused QKV rows; one and two query blocks per wave (attn_qb; it applies to the four-wave
    workgroups, Nq > 64), the single-key-tile kernel off (attn_one 0; it applies to d = 64, Nk <= 64), attn_pipe off.  A knob that does not
    apply to a shape must not change a bit.  Expected: V[sel] (a mean of 2 or 4 rows where keys share a code), by indexing."""
    B, H, Nq, Nk, d, group = shape
    c = E.attn_case(shape)
    g = E.gen(5)
    q, k, v = fused_rows(c.q, dt, 0, g), fused_rows(c.k, dt, 1, g), fused_rows(c.v, dt, 2, g)
    with knobs(**kv):
        same(K.attention(q, k, v, H, kv_group=group), c.expected(dt), str(kv))


@DT
@pytest.mark.parametrize("knob", [18, 11, 12, 26, 41, 1, 2, 3, 4])
@pytest.mark.parametrize("shape", E.ATTN_PIPE_SHAPES, ids=sid)
def test_attention_pipelined_kernel_selects_exact_rows(shape, knob, dt):
    """attn_pipe.hip under the schedules tests/test_kernel_variants_gpu.py names (18, 11, 12, 26, 41) and the first four of
    tests/test_kernels_gpu.py.  launch_attn_pipe (imagine360_amd/csrc/attn_pipe.hip:461-465) takes d = 64 without a bias, Nq >= 128 and whole
    64-key tiles, at least two -- asserted here from the shape, so that every case runs the pipelined kernel: 448 keys (7 tiles) with a ragged
    last query block of 320 queries, and 1344 keys (21 tiles) with 200 queries (ragged in every workgroup size).  The library's default rule (knob -1) turns
    the kernel on only from 2048 x 2048 up and is not exercised here; ragged key counts never reach it (test_attention_selects_exact_rows
    covers them on attn_fwd_kernel)."""
    B, H, Nq, Nk, d, group = shape
    assert d == 64 and Nk % 64 == 0 and Nk >= 128 and Nq >= 128 and knob > 0 and (knob & 7) != 0
    c = E.attn_case(shape)
    with knobs(attn_pipe=knob):
        out = K.attention(dev(c.q, dt), dev(c.k, dt), dev(c.v, dt), H, kv_group=group)
    same(out, c.expected(dt), f"attn_pipe={knob}")


@DT
@pytest.mark.parametrize("kv", [dict(), dict(attn_qb=1), dict(attn_qb=2)], ids=kvid)
@pytest.mark.parametrize("shape", E.ATTN_BIAS_SHAPES, ids=sid)
def test_attention_bias_selects_between_twin_keys(shape, kv, dt):
    """Every key has a twin with the same code; the shared bias [Nq, Nk] is 0 except -256 at (i, twin of sel[i]), so row sel[i] alone comes out:
    one wrong bias row or column returns the pair's mean or the twin.  Unpacked bias; at d = 32 also packed (K.pack_attn_bias), packed with
    block maps (K.attn_bias_blocks; the background is exactly zero), and the device-side switch to a second matrix that suppresses the
    selected key instead (the twin's row comes out)."""
    B, H, Nq, Nk, d, group = shape
    c = E.attn_case(shape, suppress=True)
    want, want_alt = c.expected(dt), c.expected(dt, alt=True)
    q, k, v = dev(c.q, dt), dev(c.k, dt), dev(c.v, dt)
    b, a = dev(c.bias, dt), dev(c.bias_alt, dt)
    flags = [torch.tensor([f], dtype=torch.int32, device="cuda") for f in (0, 1)]
    with knobs(**kv):
        same(K.attention(q, k, v, H, bias=b, kv_group=group), want, f"unpacked {kv}")
        same(K.attention(q, k, v, H, bias=b, bias_alt=a, bias_sel=flags[0], kv_group=group), want, f"unpacked, switch 0 {kv}")
        same(K.attention(q, k, v, H, bias=b, bias_alt=a, bias_sel=flags[1], kv_group=group), want_alt, f"unpacked, switch 1 {kv}")
        if not K.can_pack_attn_bias(d, Nk):
            return
        pb, pa = K.pack_attn_bias(b), K.pack_attn_bias(a)
        mb, ma = K.attn_bias_blocks(pb), K.attn_bias_blocks(pa)
        same(K.attention(q, k, v, H, bias=pb, bias_packed=True, kv_group=group), want, f"packed {kv}")
        same(K.attention(q, k, v, H, bias=pb, bias_packed=True, bias_blocks=mb, kv_group=group), want, f"packed + block map {kv}")
        for f, w in ((0, want), (1, want_alt)):
            same(K.attention(q, k, v, H, bias=pb, bias_alt=pa, bias_sel=flags[f], bias_packed=True, kv_group=group), w, f"packed, switch {f} {kv}")
            same(K.attention(q, k, v, H, bias=pb, bias_alt=pa, bias_sel=flags[f], bias_packed=True, bias_blocks=mb, bias_blocks_alt=ma,
                             kv_group=group), w, f"packed + block maps, switch {f} {kv}")


ATTN2_RING_SHAPE = (64, 1024, 77, 64, 16)


def attn2_kernel(shape, x, H=4):
    """Which kernel im360_attn_fwd2 runs (launch_xattn_resident, imagine360_amd/csrc/attn_fwd.hip:975-987): "generic" two-pass, "resident" K / V
    (attn_x 1; 2 = the same with 8-byte stores), or the twelve-wave "ring" variant (attn_x 3 on the model's key counts from 3072 query blocks up)."""
    B, Nq, n1, n2, group = shape
    if not (x and 64 < n1 <= 96 and 32 < n2 <= 64 and Nq % 32 == 0):
        return "generic"
    blocks = (B // group) * H * group * (Nq // 32)
    return "ring" if x == 3 and n1 <= 80 and n2 == 64 and blocks >= 12 * 256 else "resident"


@DT
@pytest.mark.parametrize("x", [3, 0, 1, 2])
@pytest.mark.parametrize("shape", E.ATTN2_SHAPES, ids=sid)
def test_attention2_selects_one_row_of_each_set(shape, x, dt):
    """K.attention2: the same query selects key sel1 of the first set and key sel2 of the second (the second set's keys carry codes of first-set
    keys); out_scale2 = 1/2, V in [-64, 64]: V1[sel1] + V2[sel2] / 2 is exact.  attn_x 0 = the generic two-pass kernel, 1 / 2 = resident K / V
    (Nq % 32 == 0), 3 = the twelve-wave ring variant, which only the largest shape reaches (8192 query blocks); the other shapes run the
    resident or generic kernel under knob 3.  The kernel each case must run is asserted from the launcher's rule."""
    B, Nq, n1, n2, group = shape
    want_kernel = "generic" if x == 0 or Nq % 32 else ("ring" if x == 3 and shape == ATTN2_RING_SHAPE else "resident")
    assert attn2_kernel(shape, x) == want_kernel
    c = E.Attn2Case(B, 4, Nq, n1, n2, 64, group, seed=Nq + n1)
    with knobs(attn_x=x):
        out = K.attention2(dev(c.q, dt), dev(c.k1, dt), dev(c.v1, dt), dev(c.k2, dt), dev(c.v2, dt), 4, out_scale2=0.5, kv_group=group)
    same(out, c.expected(dt, 0.5), f"attn_x={x} ({want_kernel})")


@DT
def test_single_head_attention_selects_exact_rows(dt):
    """K.single_head_attention (d = 512: GEMM -> row softmax of the 16-bit scores -> GEMM) at the smallest key count it accepts, ragged queries."""
    d, Nk, Nq = 512, 32, 40
    assert K.can_single_head_attention(d, Nk) and not K.can_single_head_attention(d, Nk - 1)
    c = E.AttnCase(1, 1, Nq, Nk, d, seed=3)
    out = K.single_head_attention(dev(c.q[0], dt), dev(c.k[0], dt), dev(c.v[0], dt), d ** -0.5)
    same(out, c.expected(dt)[0], "single head")


@DT
@pytest.mark.parametrize("scalar", [0, 1], ids=["mfma", "scalar"])
@pytest.mark.parametrize("frame_major", [False, True], ids=["token_major", "frame_major"])
@pytest.mark.parametrize("shape", E.TEMPORAL_SHAPES, ids=sid)
def test_temporal_attention_selects_exact_frames(shape, frame_major, scalar, dt):
    """K.temporal_attention: frame f takes the row of frame sel[f] != f (a cyclic permutation per (batch, pixel, head)); the MFMA kernels and the
    scalar fallback (knob tattn_scalar), both row orders."""
    B, Fr, P, heads, d = shape
    c = E.TemporalCase(B, Fr, P, heads, d, frame_major=frame_major, seed=Fr + d)
    with knobs(tattn_scalar=scalar):
        same(K.temporal_attention(dev(c.qkv, dt), B, Fr, P, heads, frame_major=frame_major), c.out.to(dt), f"tattn_scalar={scalar}")


@DT
@pytest.mark.parametrize("kind", ["uniform", "pyramid"])
@pytest.mark.parametrize("shape", E.WINDOW_SHAPES, ids=sid)
def test_temporal_windows_without_pe_return_v(shape, kind, dt):
    """(a) pe_qkv = 0 and every frame selects itself: every covering window returns the same row, so the fusion returns V under any plan and weights."""
    from imagine360_amd import context as CTX
    B, Fr, P, heads, d, L, starts, ring = shape
    c = E.TemporalCase(B, Fr, P, heads, d, seed=L, identity=True)
    C = heads * d
    pe = torch.zeros(L, 3 * C, dtype=dt, device="cuda")
    out = K.temporal_attention_windows(dev(c.qkv, dt), pe, B, Fr, P, heads, list(starts), CTX.context_weights(L, kind), ring=ring)
    same(out, c.qkv[:, 2 * C:].to(dt), "no PE")


@DT
@pytest.mark.parametrize("shape", E.WINDOW_SHAPES, ids=sid)
def test_temporal_windows_select_through_the_pe_rows(shape, dt):
    """(b) the selector lives in the PE rows only: position p of EVERY window takes position pi(p) of that window, frames (starts[k] + pi(p)) % F;
    uniform weights and coverage 1 / 2 / 4 make the fusion a dyadic mean.  Pins that positions restart per window and that the ring wraps."""
    B, Fr, P, heads, d, L, starts, ring = shape
    c = E.WindowsPECase(B, Fr, P, heads, d, L, starts, ring, seed=Fr)
    out = K.temporal_attention_windows(dev(c.qkv, dt), dev(c.pe, dt), B, Fr, P, heads, list(starts), c.weights, ring=ring)
    same(out, c.expected().float().to(dt), "PE selector")


# ================================================================================================ 3. GroupNorm statistics
def partial_sums(buf, S, N, C):
    return buf.view(N, S, 2, C).double().sum(1).cpu()


@DT
@pytest.mark.parametrize("N,H,W,C,pad", E.GN_PARTIAL_SHAPES)
def test_group_norm_partial_sums_are_the_integer_sums(N, H, W, C, pad, dt):
    """K.group_norm_partials on integers in [-8, 8]: the slabs' fp32 partial sums are exact; summed over slabs they are the integer sum and sum of
    squares of the circularly padded tensor, wrapped columns counted twice."""
    x = E.ints((N, H, W, C), -8, 8, E.gen(W + C))
    buf, S = K.group_norm_partials(dev(x, dt), pad)
    same(partial_sums(buf, S, N, C), E.gn_sums(x, pad), f"pad={pad}")


@DT
def test_group_norm_partial_sums_from_the_conv_epilogue(dt):
    """conv2d(..., gn_stats=True) at its smallest qualifying shape (512 tiles of 256 x 320): the epilogue's partial sums are those of the STORED
    integers (|y| <= 128 keeps a 256-pixel slab's sum of squares below 2^24)."""
    c = E.ConvCase(dt, "exact", 128, 32, 32, 64, 320, temb_fr=1, res=True, seed=11, limit=128)
    want = c.expected()
    x, wp, kw = E.conv_gpu_args(c, K)
    y = K.conv2d(x, wp, c.Cout, gn_stats=True, **kw)
    g = K._gn_of(y)
    assert g is not None and g[1] == 4 and 256 * 128 ** 2 < E.FP32_EXACT
    same(y, want, "conv output")
    same(partial_sums(g[0], g[1], c.N, c.Cout), E.gn_sums(want.float(), 0), "partial sums")


@DT
def test_group_norm_partial_sums_from_the_linear_epilogue(dt):
    """linear(..., gn_hw=256): one slab per 256-row tile, statistics of the stored integers."""
    Nimg, HW, Kd, n = 5, 256, 64, 320
    c = E.LinearCase(dt, "exact", Nimg * HW, Kd, n, seed=12, limit=128)
    want = c.expected()
    y = K.linear(dev(c.x, dt), K.pack_conv_weight(dev(c.w, dt).reshape(n, Kd, 1, 1)), n, bias=dev(c.bias, dt), res=dev(c.res, dt), gn_hw=HW)
    g = K._gn_of(y)
    assert g is not None and g[1] == 1
    same(y, want, "linear output")
    same(partial_sums(g[0], g[1], Nimg, n), E.gn_sums(want.float().reshape(Nimg, 16, 16, n), 0), "partial sums")


@DT
@pytest.mark.parametrize("mode", ["partials", "three"])
@pytest.mark.parametrize("N,H,W,C1,C2", E.GN_STRUCTURED)
def test_group_norm_padded_statistics_on_structured_columns(N, H, W, C1, C2, mode, dt):
    """K.group_norm with pad = 2 (single tensor and the (xa, xb) pair form) where the wrapped columns sit 8 standard deviations from the rest of
    the image: statistics that weight them once miss TOL by more than ten times (tests/test_exact_cases.py).  fp64 F.group_norm of the padded tensor."""
    C = C1 + C2
    x = E.gn_structured_input(N, H, W, C, dt, seed=W + C)
    g = E.gen(C)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(dt).float(), (0.1 * torch.randn(C, generator=g)).to(dt).float()
    ref = E.gn_reference(x, gamma, beta, 32, 1e-5, 2)
    xin = dev(x, dt) if C2 == 0 else (dev(x[..., :C1].contiguous(), dt), dev(x[..., C1:].contiguous(), dt))
    old = K.GN_MODE
    try:
        K.GN_MODE = mode
        out = K.group_norm(xin, dev(gamma, dt), dev(beta, dt), 32, 1e-5, pad=2)
    finally:
        K.GN_MODE = old
    err = E.rel(out, ref)
    print(f"rel {err:.3e} (TOL {TOL[dt]:.0e})")
    assert out.shape == ref.shape and err < TOL[dt]
