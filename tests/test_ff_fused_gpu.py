"""The fused feed-forward launch (csrc/ff_fused.hip: kernels.ff_fused / ff_fused_ln, K = 320, inner 1280, N = 320) against today's pair
of launches -- kernels.linear_geglu[_ln], then kernels.conv2d of the [M, 1, 1, 1280] view with bias and residual, which is what
layers.gemm_linear issues -- and against an fp64 reference of LayerNorm -> Linear -> GEGLU -> Linear + bias + residual.

What must hold, and why:
  * plain-bias form: the pair's BITS.  Same MFMA shape, same ascending K order in both GEMMs, same 16-bit rounding of the intermediate,
    same epilogue arithmetic (bias add, rounding, residual add, rounding).
  * LayerNorm-folded form: the pair's bits, or -- the library is built with -ffast-math and hipcc has contracted `(acc - mu c1) rstd + c2`
    differently between instantiations before (test_kernel_variants_gpu.test_g4_tiles_geglu_with_folded_layer_norm) -- one unit of the
    storage format in relative L2 (ULP[dt]: 2^-7 bf16, 2^-10 fp16; whole tensor and per 256-row block: a bound from the formats).
  * against fp64: within the pair's own error + ULP (triangle inequality), and within TOL: the chain rounds three times to the storage
    format (intermediate, output, output + residual: 3 x 2^-9 = 5.9e-3 in bf16, 3 x 2^-12 = 7.3e-4 in fp16, as relative L2 bounds).
Inputs: rows with a non-zero mean (+ 0.3, as the g4 test), gate rows scaled by 2 so that gates reach the polynomial's +- 4.2 clamp, a
residual scaled by 0.1 so that the feed-forward term dominates the norm.  Shapes: one tile, a ragged single tile, several tiles with a
ragged tail, and 65 721 rows = 514 tiles: on 256 CUs some workgroups of the persistent walk take three tiles, others two."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from _guarded import Guarded  # noqa: E402
from helpers import record  # noqa: E402
from imagine360_amd import kernels as K, layers  # noqa: E402
from test_kernel_variants_gpu import ULP, _row_stats  # noqa: E402
from test_kernels_gpu import DTYPES, TOL, blockrel, rel  # noqa: E402

C, INNER = K.FF_FUSED_SHAPE
M_MAX = 2 * 256 * 128 + 128 + 57
SHAPES = [128, 200, 128 * 3 + 57, M_MAX]
EPS = 1e-5
_CASES = {}


def _case(dt, ln):
    """Operands of one (dtype, form) on the device, for M_MAX rows (smaller cases take the first rows: the operation is row-wise), with the
    pair's output and the fp64 reference -- computed once, shared by the tests, never modified."""
    key = (dt, ln)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(300 + 2 * DTYPES.index(dt) + int(ln))
    rn = lambda *s: torch.randn(*s, generator=g)
    x = (rn(M_MAX, C) + 0.3).to(dt).cuda()
    res = (0.1 * rn(M_MAX, C)).to(dt).cuda()
    w1 = rn(2 * INNER, C) * C ** -0.5
    w1[INNER:] *= 2.0                                             # gates of std ~ 2: a few per cent of them beyond the +- 4.2 clamp
    w1, b1 = w1.to(dt).cuda(), (0.5 * rn(2 * INNER)).to(dt).cuda()
    w2, b2 = (rn(C, INNER) * INNER ** -0.5).to(dt).cuda(), (0.1 * rn(C)).to(dt).cuda()
    gam, bet = (1 + 0.1 * rn(C)).to(dt).cuda(), (0.1 * rn(C)).to(dt).cuda()
    w2p = K.pack_conv_weight(w2.reshape(C, INNER, 1, 1))
    c = dict(x=x, res=res, w2p=w2p, b2=b2)
    xd = x.double()
    if ln:
        wf, c1, c2 = K.fold_layer_norm(w1, b1, gam, bet)
        wp, c1p = K.pack_geglu(wf, c1)
        c.update(wp=wp, c1p=c1p.contiguous(), c2p=K.interleave_geglu(wf, c2)[1].contiguous(), stats=_row_stats(x))
        xd = F.layer_norm(xd, (C,), gam.double(), bet.double(), EPS)
    else:
        wp, bp = K.pack_geglu(w1, b1)
        c.update(wp=wp, bp=bp)
    h = F.linear(xd, w1.double(), b1.double())
    h = h[:, :INNER] * F.gelu(h[:, INNER:])
    c["clamped"] = float((F.linear(xd, w1.double()[INNER:], b1.double()[INNER:]).abs() > 4.2).double().mean())
    c["ff64"] = F.linear(h, w2.double(), b2.double())              # + the residual of the case at hand
    del h, xd
    _CASES[key] = c
    return c


def _pair(c, M, ln, res):
    x = c["x"][:M]
    h = K.linear_geglu_ln(x, c["wp"], c["c1p"], c["c2p"], c["stats"][:M].contiguous(), EPS, INNER) if ln else K.linear_geglu(x, c["wp"], c["bp"], INNER)
    return K.conv2d(h.reshape(M, 1, 1, INNER), c["w2p"], C, bias=c["b2"], res=res.reshape(M, 1, 1, C)).reshape(M, C)


def _fused(c, M, ln, res, x=None):
    x = c["x"][:M] if x is None else x
    if ln:
        return K.ff_fused_ln(x, c["wp"], c["c1p"], c["c2p"], c["stats"][:M].contiguous(), EPS, c["w2p"], c["b2"], res)
    return K.ff_fused(x, c["wp"], c["bp"], c["w2p"], c["b2"], res)


def _compare(tag, dt, ln, fused, pair, ref):
    same = torch.equal(fused, pair)
    d, db = rel(fused, pair), blockrel(fused, pair, 256)
    e_f, e_p = rel(fused, ref), rel(pair, ref)
    b_f = blockrel(fused, ref, 256)
    print(f"ff_fused {tag}: bits-equal-pair {same} rel-to-pair {d:.3e} blockrel256-to-pair {db:.3e}  vs fp64: fused {e_f:.3e} pair {e_p:.3e} blockrel256 {b_f:.3e}")
    record("ff_fused_" + tag, bits_equal_pair=same, rel_to_pair=d, fused_vs_fp64=e_f, pair_vs_fp64=e_p)
    if ln:
        assert same or (d < ULP[dt] and db < ULP[dt]), (d, db)
    else:
        assert same, (d, db)
    assert e_f <= e_p + ULP[dt] and e_f < TOL[dt] and b_f < 2 * TOL[dt], (e_f, e_p, b_f)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ln", [False, True], ids=["bias", "ln"])
@pytest.mark.parametrize("M", SHAPES)
def test_ff_fused_matches_the_pair_of_launches(dt, ln, M):
    c = _case(dt, ln)
    assert 0.005 < c["clamped"] < 0.2, c["clamped"]              # the inputs do reach the clamp
    res = c["res"][:M].contiguous()
    fused, pair = _fused(c, M, ln, res), _pair(c, M, ln, res)
    assert fused.shape == (M, C) and fused.dtype == dt
    ref = c["ff64"][:M] + res.double()
    _compare(f"{'ln' if ln else 'bias'}_{str(dt).split('.')[-1]}_M{M}", dt, ln, fused, pair, ref)


@pytest.mark.parametrize("dt", DTYPES)
def test_ff_fused_residual_may_alias_the_input(dt):
    """The production call: layers.FeedForward is called with residual = its input."""
    M, ln = 128 * 3 + 57, True
    c = _case(dt, ln)
    x = c["x"][:M].contiguous()
    fused, pair = _fused(c, M, ln, x, x=x), _pair(c, M, ln, x)
    _compare(f"alias_{str(dt).split('.')[-1]}", dt, ln, fused, pair, c["ff64"][:M] + x.double())
    assert torch.equal(x, c["x"][:M])                             # the input is read only


@pytest.mark.parametrize("ln", [False, True], ids=["bias", "ln"])
def test_ff_fused_writes_every_row_and_nothing_else(ln):
    """Guard bands (tests/_guarded.py) around every operand and the output at a ragged tail: nothing outside the output is written, no
    row of it is skipped, and the rows past M that the last tile covers are not read into the result (the guards are NaNs)."""
    dt, M = torch.bfloat16, 128 * 3 + 57
    c = _case(dt, ln)
    g = Guarded(K)
    x, res = g.guard(c["x"][:M].contiguous()), g.guard(c["res"][:M].contiguous())
    ops = {k: g.guard(v) for k, v in c.items() if k in ("wp", "bp", "c1p", "c2p", "w2p", "b2")}
    with g:
        if ln:
            y = K.ff_fused_ln(x, ops["wp"], ops["c1p"], ops["c2p"], g.guard(c["stats"][:M].contiguous()), EPS, ops["w2p"], ops["b2"], res)
        else:
            y = K.ff_fused(x, ops["wp"], ops["bp"], ops["w2p"], ops["b2"], res)
        g.out(y)
    assert torch.equal(y, _fused(c, M, ln, c["res"][:M].contiguous()))


def test_ff_fused_rejects_other_widths():
    dt = torch.bfloat16
    c = _case(dt, False)
    x = torch.zeros(256, 640, dtype=dt, device="cuda")
    rc = K.lib().im360_ff_fused(x.data_ptr(), c["wp"].data_ptr(), None, None, None, None, 0, 0.0, c["w2p"].data_ptr(), None, x.data_ptr(),
                                x.data_ptr(), 256, 640, 2560, 640, 0, None)
    assert rc == -2 and b"unsupported" in K.lib().im360_last_error()


@pytest.mark.parametrize("dt", DTYPES)
def test_feed_forward_route_and_knob(dt):
    """layers.FeedForward at M >= ROUTE_MIN_TOKENS (lowered, as the routed tests of test_kernels_gpu lower it): knob ff_fused = 0 gives
    today's pair of launches and its bits exactly; the default takes the fused launch (one gemm-class launch instead of two) and equals the
    direct call of the wrapper."""
    M = 128 * 3 + 57
    g = torch.Generator().manual_seed(311)
    ff = layers.FeedForward(C).to(dt).cuda()
    norm = torch.nn.LayerNorm(C).to(dt).cuda()
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * torch.randn(C, generator=g))
        norm.bias.copy_(0.1 * torch.randn(C, generator=g))
    x = (torch.randn(M, C, generator=g) + 0.3).to(dt).cuda()
    st = _row_stats(x)
    saved, default = layers.ROUTE_MIN_TOKENS, K.tuning_get("ff_fused")
    layers.ROUTE_MIN_TOKENS = 0
    counts = {}
    try:
        with torch.no_grad():
            for knob in (0, 1):
                K.tuning_set("ff_fused", knob)
                K.STATS = {}
                y = ff(x, residual=x, ln=norm, stats=st)
                counts[knob] = (y, K.STATS["gemm"][2])
            K.tuning_set("ff_fused", 0)
            no_res = ff(x, ln=norm, stats=st)                     # no residual: the route is not taken
    finally:
        K.STATS = None
        layers.ROUTE_MIN_TOKENS = saved
        K.tuning_set("ff_fused", default)
    assert default == 1 and counts[0][1] == 2 and counts[1][1] == 1, (default, counts[0][1], counts[1][1])
    # today's pair, issued by hand
    wf, c1, c2 = K.fold_layer_norm(ff.net[0].proj.weight, ff.net[0].proj.bias.detach(), norm.weight, norm.bias)
    wp, c1p = K.pack_geglu(wf, c1)
    c2p = K.interleave_geglu(wf, c2)[1].contiguous()
    w2p = K.pack_conv_weight(ff.net[2].weight.detach().reshape(C, INNER, 1, 1))
    h = K.linear_geglu_ln(x, wp, c1p.contiguous(), c2p, st, norm.eps, INNER)
    pair = K.conv2d(h.reshape(M, 1, 1, INNER), w2p, C, bias=ff.net[2].bias, res=x.reshape(M, 1, 1, C)).reshape(M, C)
    assert torch.equal(counts[0][0], pair)
    assert torch.equal(no_res, K.conv2d(h.reshape(M, 1, 1, INNER), w2p, C, bias=ff.net[2].bias).reshape(M, C))
    direct = K.ff_fused_ln(x, wp, c1p.contiguous(), c2p, st, norm.eps, w2p, ff.net[2].bias.detach(), x)
    assert torch.equal(counts[1][0], direct)
    d = rel(direct, pair)
    assert torch.equal(direct, pair) or d < ULP[dt], d
