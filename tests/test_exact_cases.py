"""CPU self-checks of tests/_exact_cases.py: the exact references are right (two independent computations agree; the fp32 path is exact
by a bound on the magnitudes), the cases have the properties the GPU tests rely on (tie shares, underflow gaps, edge selections), and
the cases BITE: deliberately wrong host emulations of each operation -- a dropped key, a wrong wrapped neighbour, a shifted tap, a
skipped K chunk, a split-K part added twice, truncation, another rounding point, single-weighted wrapped columns -- all give a result
that differs from the reference.  Host code only: nothing here launches or perturbs a kernel."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import _exact_cases as E
from imagine360_amd import context as CTX

TOL = {E.BF16: 1e-2, E.FP16: 3e-3}          # tests/test_kernels_gpu.py
ids = lambda d: str(d).split(".")[-1]


# ------------------------------------------------------------------------------------------------ integer convolution / GEMM
def _check_int_case(c, dt, kind):
    assert c.bound < E.FP32_EXACT                                      # every fp32 partial sum is an exact integer, in any order
    p64, p32 = c.pre(torch.float64), c.pre(torch.float32)
    assert p32.dtype == torch.float32 and torch.equal(p32.double(), p64)
    assert torch.equal(p64, p64.round()) and float(p64.abs().max()) <= c.bound
    y64, y32 = c.finish(p64), c.expected()
    assert y32.dtype == dt and torch.equal(y32, y64)
    ties, odd = E.shares(p64, dt)
    if kind == "exact":
        total = p64 if c.res is None else p64 + c.res.double()
        assert float(total.abs().max()) <= c.limit <= E.EXACT_MAX[dt] and ties == 0 and odd == 0
        assert torch.equal(y64.double(), total)                         # nothing is rounded at all
    else:
        assert ties >= 0.01 and odd >= 0.10, (ties, odd)
        lo = E.EXACT_MAX[dt]
        band = (p64.abs() > lo) & (p64.abs() < 2 * lo) & (p64.abs() % 2 == 1)          # the odd integers of the first binade with spacing 2
        assert float(band.double().mean()) >= 0.01
        # a truncating epilogue and round-half-up differ from RNE on this case
        assert not torch.equal(c.finish(p64, E.truncate), y64)
        half_up = lambda t, d: (torch.floor(t.double() / E.spacing(t, d) + 0.5) * E.spacing(t, d)).float().to(d)
        assert not torch.equal(c.finish(p64, half_up), y64)
        if c.res is not None:                                          # the other rounding point (module docstring of _exact_cases)
            once = E.rne(p64 + c.res.double(), dt)
            twice = E.rne(E.rne(p64, dt).double() + c.res.double(), dt)
            assert not torch.equal(once, twice)
            assert torch.equal(y64, twice if c.rounds_before_residual() else once)
    return p64, y64


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("dt", E.DTYPES, ids=ids)
@pytest.mark.parametrize("name", list(E.ALL_CONV))
def test_conv_cases_are_exact_and_two_references_agree(name, dt, kind):
    c = E.conv_case(name, dt, kind)
    if kind == "exact":
        assert c.acc_bound == 2 * c.nnz and float(c.w.abs().sum((1, 2, 3)).max()) == c.nnz and float(c.x.abs().max()) <= 2
    else:
        assert float(c.x.abs().max()) <= c.xmax and float(c.w.abs().max()) <= c.wmax and c.acc_bound == c.taps * c.Cin * c.xmax * c.wmax
    for t in (c.x, c.w, c.bias, c.temb, c.res):
        assert t is None or torch.equal(t.to(dt).float(), t)                                   # representable in the 16-bit type
    assert not torch.equal(c.x, c.x.flip(2)) and not torch.equal(c.x, c.x.roll(1, 2))          # no mirror or translation symmetry along W
    _check_int_case(c, dt, kind)


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("dt", E.DTYPES, ids=ids)
@pytest.mark.parametrize("name", ["forms/wrap", "forms/stride2_wrap", "forms/up_wrap", "forms/plain", "forms/temb_res", "korder/ragged_3_chunks", "ksplit/ragged_tile"])
def test_conv_cases_catch_wrong_addressing(name, dt, kind):
    """Wrong host emulations: the wrapped neighbour (column W - 1 instead of column 0 at the right edge, and the reverse), one tap shifted by
    a column, one 64-channel K chunk skipped, a split-K part added twice, the last pixel's row of x dropped."""
    c = E.conv_case(name, dt, kind)
    ref = c.expected(torch.float64)
    wrongs = {}
    if c.wrap:
        # through the padded tensor: the right wrap column (a copy of column 0) replaced by column W - 1, the left one by column 0
        nowrap = copy.copy(c)
        nowrap.wrap = False
        p = 2 if c.stride == 2 else 1
        xr = c.x.double().permute(0, 3, 1, 2)
        clamp = torch.cat([xr[..., :1].expand(-1, -1, -1, p), xr, xr[..., -1:].expand(-1, -1, -1, p)], dim=-1)     # replicate instead of wrap
        if not c.up and c.stride == 1:
            y = F.conv2d(F.pad(clamp, (0, 0, 1, 1)), c.w.double()).permute(0, 2, 3, 1)
            y = y + c.bias.double() + (c.temb.double().repeat_interleave(c.temb_fr, 0)[:, None, None, :] if c.temb is not None else 0)
            wrongs["clamp_instead_of_wrap"] = c.finish(y)
        wrongs["no_wrap_at_all"] = nowrap.finish(nowrap.pre())
    if c.taps == 9:
        w = c.w.clone()
        w[:, :, 1, 2] = c.w[:, :, 1, 1]                  # tap (1, 2) reads what tap (1, 1) reads: one tap shifted by a column
        w[:, :, 1, 1] = c.w[:, :, 1, 2]
        wrongs["tap_shifted"] = c.finish(c.pre(w=w))
    if c.Cin >= 128:
        x = c.x.clone()
        x[..., 64:128] = 0
        skipped = c.pre(x=x)
        wrongs["k_chunk_skipped"] = c.finish(skipped)
        wrongs["k_part_twice"] = c.finish(2 * c.pre() - skipped)          # conv + bias + chunk 1's products once more
    x = c.x.clone()
    x[-1, -1, -1] = 0
    wrongs["last_pixel_dropped"] = c.finish(c.pre(x=x))
    assert wrongs
    for what, y in wrongs.items():
        assert y.shape == ref.shape and not torch.equal(y, ref), what


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("dt", E.DTYPES, ids=ids)
@pytest.mark.parametrize("name", list(E.CAT))
def test_cat_cases(name, dt, kind):
    c, C1 = E.cat_case(name, dt, kind)
    assert C1 != c.Cin - C1
    _check_int_case(c, dt, kind)
    swapped = torch.cat([c.x[..., C1:], c.x[..., :C1]], dim=-1)                      # the two sources in the wrong order
    assert not torch.equal(c.finish(c.pre(x=swapped)), c.expected())


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("dt", E.DTYPES, ids=ids)
@pytest.mark.parametrize("M,Kd,n", [s for s in E.LINEAR if s[0] == 300] + [(65536 + 77, 320, 320)])
def test_linear_cases(M, Kd, n, dt, kind):
    c = E.linear_case(M, Kd, n, dt, kind)
    p64, y = _check_int_case(c, dt, kind)
    if kind == "exact":          # the row statistics of the stored integers are exact in fp32: a slice's sum of squares stays below 2^24
        assert E.ROW_SLICE * c.limit ** 2 < E.FP32_EXACT
        st = E.row_stats(y)
        assert torch.equal(st, st.round()) and float(st.abs().max()) < E.FP32_EXACT and torch.equal(st.float().double(), st)
        gone = y.clone()
        gone[M - 1, n - 1] += 1                      # one element of one row's last slice
        assert not torch.equal(E.row_stats(gone), st)
    assert not torch.equal(c.finish(c.pre(skip_chunk=0)), y)
    if Kd > 64:
        assert not torch.equal(c.finish(c.pre(skip_chunk=Kd // 64 - 1)), y)


# ------------------------------------------------------------------------------------------------ attention as selection
def test_amplitudes_meet_the_underflow_gap():
    for d, want in ((8, 32), (24, 32), (32, 32), (40, 32), (64, 32), (80, 32), (160, 64), (512, 64)):
        amp = E.amplitude(d)
        assert amp == want and amp * amp * d ** -0.5 * E.LOG2E >= E.UNDERFLOW_GAP
        assert (amp // 2) ** 2 * d ** -0.5 * E.LOG2E < E.UNDERFLOW_GAP          # the smallest power of two that does
    assert 2.0 ** -E.UNDERFLOW_GAP < 2.0 ** -149 and torch.exp2(torch.tensor(-E.UNDERFLOW_GAP)).item() == 0.0


def test_codes_are_distinct_two_hot_rows():
    for d in (8, 32):
        rows = E.code_rows(torch.arange(E.n_codes(d)), d, 32)
        assert rows.shape == (4 * math.comb(d, 2), d) and len({tuple(r.tolist()) for r in rows}) == rows.shape[0]
        assert bool(((rows != 0).sum(1) == 2).all()) and set(rows.unique().tolist()) == {-32.0, 0.0, 32.0}
        s = rows @ rows.t()
        assert bool((s.diagonal() == 2 * 32 * 32).all()) and float((s - torch.diag(s.diagonal())).max()) == 32 * 32


@pytest.mark.parametrize("shape", E.ATTN_SHAPES + E.ATTN_PIPE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_cases(shape):
    B, H, Nq, Nk, d, group = shape
    c = E.attn_case(shape)
    assert c.gap_log2() >= E.UNDERFLOW_GAP and c.amp == E.amplitude(d)
    props = E.sel_properties(c.sel, Nq, Nk)
    assert all(props.values()), props
    sizes = torch.zeros(B // group, H, Nk).scatter_add_(2, c.grp, torch.ones(B // group, H, Nk))
    assert set(sizes.unique().tolist()) <= {0.0, 1.0, 2.0, 4.0} and (Nk < 16 or {2.0, 4.0} <= set(sizes.unique().tolist()))
    w = c.weights()
    assert set(w.unique().tolist()) <= {0.0, 0.25, 0.5, 1.0} and bool((w.sum(-1) == 1).all())
    if Nk >= 16:
        assert bool((w == 0.5).any()) and bool((w == 0.25).any())                # some queries average 2 and some 4 rows (the row sum)
    for dt in E.DTYPES:
        want = c.expected(dt)
        for t in (c.q, c.k, c.v):
            assert torch.equal(t.to(dt).float(), t)
        # the fp32 softmax is exactly the selection; so is its result after the one rounding
        got = E.softmax_attention(c.q, c.k, c.v, H, c.scale, group)
        assert torch.equal(got.to(dt), want)
    assert not torch.equal(E.softmax_attention(c.q, c.k, c.v, H, c.scale, group, drop_last_key=True).to(E.BF16), c.expected(E.BF16))
    swapped = [E.softmax_attention(c.q, c.k, c.v, H, c.scale, group, swap_keys=(j, j + 1)).to(E.BF16) for j in (0, Nk - 2, 31) if j + 1 < Nk]
    assert all(not torch.equal(s, c.expected(E.BF16)) for s in swapped)


@pytest.mark.parametrize("shape", E.ATTN_BIAS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention_bias_cases(shape):
    B, H, Nq, Nk, d, group = shape
    c = E.attn_case(shape, suppress=True)
    assert c.gap_log2() >= E.UNDERFLOW_GAP and c.bias_mag * E.LOG2E >= E.UNDERFLOW_GAP
    props = E.sel_properties(c.sel, Nq, Nk, full=Nq // 2 - 2 >= len(E.edge_keys(Nk)))
    assert all(props.values()), props
    for dt in E.DTYPES:
        assert torch.equal(c.bias.to(dt).float(), c.bias)
        want = c.expected(dt)
        # without the bias the query averages the pair; with the wrong row or column of the bias too
        plain = E.softmax_attention(c.q, c.k, c.v, H, c.scale, group).to(dt)
        assert not torch.equal(plain, want)
    assert not torch.equal(c.expected(E.BF16, alt=True), c.expected(E.BF16))
    assert int((c.bias != 0).sum()) == Nq                                           # background exactly zero: most 32 x 32 blocks are empty
    blocks = F.pad(c.bias != 0, (0, -Nk % 32, 0, -Nq % 32)).reshape(-(-Nq // 32), 32, -(-Nk // 32), 32).any(3).any(1)
    assert 0 < float(blocks.float().mean()) and (Nk < 1024 or float(blocks.float().mean()) < 0.8)          # blocks to skip and blocks to add


@pytest.mark.parametrize("shape", E.ATTN2_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attention2_cases(shape):
    B, Nq, n1, n2, group = shape
    H, d = 4, 64
    c = E.Attn2Case(B, H, Nq, n1, n2, d, group, seed=Nq + n1)
    assert all(E.sel_properties(c.sel2, Nq, n2).values()) and all(E.sel_properties(c.sel1, Nq, n1).values())
    assert bool((c.map.sort(-1).values.diff(dim=-1) > 0).all())                       # injective
    one = E.softmax_attention(c.q, c.k1, c.v1, H, d ** -0.5, group)
    two = E.softmax_attention(c.q, c.k2, c.v2, H, d ** -0.5, group)
    for dt in E.DTYPES:
        assert torch.equal((one + 0.5 * two).to(dt), c.expected(dt, 0.5))
    wrong = E.softmax_attention(c.q, c.k2, c.v2, H, d ** -0.5, group, drop_last_key=True)
    assert not torch.equal((one + 0.5 * wrong).to(E.BF16), c.expected(E.BF16, 0.5))
    assert not torch.equal((one + two).to(E.BF16), c.expected(E.BF16, 0.5))          # the second set's scale


def test_single_head_case():
    d, Nk, Nq = 512, 32, 40
    c = E.AttnCase(1, 1, Nq, Nk, d, seed=3)
    assert c.amp == 64 and c.gap_log2() >= E.UNDERFLOW_GAP
    for dt in E.DTYPES:          # the kernel's own op order: 16-bit scaled queries, 16-bit scores, fp32 row softmax, 16-bit probabilities
        s = ((c.q[0].to(dt) * d ** -0.5).float() @ c.k[0].t()).to(dt).float()
        assert float(s.max()) < 65504 and float((s.amax(-1, keepdim=True) - s)[s < s.amax(-1, keepdim=True)].min()) > 104          # e^-104 < 2^-149
        out = (torch.softmax(s, -1).to(dt).float() @ c.v[0]).to(dt)
        assert torch.equal(out, c.expected(dt)[0])


@pytest.mark.parametrize("shape", E.TEMPORAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_cases(shape):
    B, Fr, P, heads, d = shape
    c = E.TemporalCase(B, Fr, P, heads, d, seed=Fr + d)
    assert c.gap_log2() >= E.UNDERFLOW_GAP
    assert not bool((c.sel == torch.arange(Fr)).any()) and bool((c.sel.sort(1).values == torch.arange(Fr)).all())          # a permutation without fixed points
    C = heads * d
    t = c.qkv.reshape(B, Fr, P, 3 * C).permute(0, 2, 1, 3).reshape(B * P, Fr, 3 * C)
    got = E.softmax_attention(t[..., :C], t[..., C:2 * C], t[..., 2 * C:], heads, d ** -0.5)
    got = got.reshape(B, P, Fr, C).permute(0, 2, 1, 3).reshape(B * Fr * P, C)
    assert torch.equal(got, c.out)
    fm = E.TemporalCase(B, Fr, P, heads, d, frame_major=True, seed=Fr + d)
    assert torch.equal(fm.qkv.reshape(Fr, B, P, -1).permute(1, 0, 2, 3).reshape(c.qkv.shape), c.qkv)
    assert torch.equal(fm.out.reshape(Fr, B, P, -1).permute(1, 0, 2, 3).reshape(c.out.shape), c.out) and (B == 1 or not torch.equal(fm.out, c.out))
    drop = E.softmax_attention(t[..., :C], t[:, :-1, C:2 * C], t[:, :-1, 2 * C:], heads, d ** -0.5)
    assert not torch.equal(drop.reshape(B, P, Fr, C).permute(0, 2, 1, 3).reshape(B * Fr * P, C), c.out)


@pytest.mark.parametrize("shape", E.WINDOW_SHAPES, ids=lambda s: "x".join(str(v) if not isinstance(v, tuple) else "s" + "_".join(map(str, v)) for v in s))
def test_window_cases(shape):
    B, Fr, P, heads, d, L, starts, ring = shape
    # (a) no PE: every frame selects itself; any plan and weights return V
    a = E.TemporalCase(B, Fr, P, heads, d, seed=L, identity=True)
    C = heads * d
    pe0 = torch.zeros(L, 3 * C, dtype=torch.float64)
    w = CTX.context_weights(L, "pyramid")
    got = CTX.windowed_temporal_attention(a.qkv.double(), pe0, B, Fr, P, heads, list(starts), w, ring=ring)
    assert float((got - a.qkv[:, 2 * C:].double()).abs().max()) <= 1e-12 * 128 and torch.equal(a.out, a.qkv[:, 2 * C:])
    # (b) the selector in the PE rows
    c = E.WindowsPECase(B, Fr, P, heads, d, L, starts, ring, seed=Fr)
    assert set(c.cover) <= {1, 2, 4} and len(set(c.cover)) >= 1 and not bool((c.pi == torch.arange(L)).any())
    assert c.amp ** 2 * d ** -0.5 * E.LOG2E >= E.UNDERFLOW_GAP
    want = c.expected()
    got = CTX.windowed_temporal_attention(c.qkv.double(), c.pe.double(), B, Fr, P, heads, list(starts), c.weights, ring=ring)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    for dt in E.DTYPES:
        assert torch.equal(want.float().to(dt).double(), want)                 # dyadic means of small integers: representable
        assert torch.equal(c.qkv.to(dt).float(), c.qkv) and torch.equal(c.pe.to(dt).float(), c.pe)
    # positions that do not restart per window (PE[f] instead of PE[p]) and a ring that does not wrap give something else
    if len(starts) > 1:
        glob = torch.zeros_like(want)
        acc = glob.reshape(B, Fr, P, C)
        for s in starts:
            for p in range(L):
                f = (s + p) % Fr
                src = (s + int(c.pi[(s + p) % L])) % Fr
                acc[:, f] += c.v[:, src].double()
        acc /= torch.tensor(c.cover, dtype=torch.float64)[None, :, None, None]
        if any(s % L for s in starts):          # (with every start a multiple of L, PE[f % L] is PE[p])
            assert not torch.equal(glob, want)
    if ring and any(s + L > Fr for s in starts):
        assert not torch.equal(c.expected(wrap=False), want)


# ------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("N,H,W,C,pad", E.GN_PARTIAL_SHAPES)
def test_group_norm_sums_weight_the_wrapped_columns_twice(N, H, W, C, pad):
    x = E.ints((N, H, W, C), -8, 8, E.gen(W + C))
    s = E.gn_sums(x, pad)
    assert s.shape == (N, 2, C) and torch.equal(s, s.round()) and H * (W + 2 * pad) * 64 < E.FP32_EXACT
    xi = x.long()
    cols = torch.ones(W, dtype=torch.long)
    if pad:
        cols[:pad] += 1
        cols[-pad:] += 1
    assert torch.equal(s[:, 0].long(), (xi * cols[None, None, :, None]).sum((1, 2))) and torch.equal(s[:, 1].long(), (xi * xi * cols[None, None, :, None]).sum((1, 2)))
    if pad:
        assert not torch.equal(s, E.gn_sums(x, 0))


@pytest.mark.parametrize("dt", E.DTYPES, ids=ids)
@pytest.mark.parametrize("N,H,W,C1,C2", E.GN_STRUCTURED)
def test_structured_group_norm_case_separates_the_two_weightings(N, H, W, C1, C2, dt):
    C = C1 + C2
    x = E.gn_structured_input(N, H, W, C, dt, seed=W + C)
    g = E.gen(C)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(dt).float(), (0.1 * torch.randn(C, generator=g)).to(dt).float()
    ref = E.gn_reference(x, gamma, beta, 32, 1e-5, 2)
    single = E.gn_reference(x, gamma, beta, 32, 1e-5, 2, single_weight=True)
    assert E.rel(single, ref) >= 10 * TOL[dt], E.rel(single, ref)
    same = E.gn_reference(x, gamma, beta, 32, 1e-5, 0)
    assert E.rel(E.gn_reference(x, gamma, beta, 32, 1e-5, 0, single_weight=True), same) < 1e-12          # the emulation itself is a GroupNorm
