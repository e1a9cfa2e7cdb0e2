"""CPU tier of the pairwise parity sweep: the covering arrays cover, the fp64 references agree with the plain-torch stand-ins, every
optional operand is large enough to be seen, and stand-ins with a defect that fires under ONE PAIR of factor values are flagged.
The same tables run against the HIP kernels in tests/test_kernel_pairs_gpu.py."""
import functools

import pytest
import torch

import _emu_kernels as EMU
import _pair_cases as PC
from _pairwise import cover, legal_from, legal_pairs, uncovered

torch.set_grad_enabled(False)

FAMS = list(PC.FAMILIES.values())
ALL = [pytest.param(f, c, id=f"{f.name}-{f.case_id(c)}") for f in FAMS for c in f.cases]
MAX_CASES = 80

# the generated lists must not shrink (or move) silently: a change of a table shows up here and is reviewed with it
DIGESTS = {
    "conv": "1698a5203c12793f", "conv_up2": "255905ef1baa0963", "conv1x1_cat": "b10dae8157a87420", "attention": "5dca1de77360b319", "attention2": "35582b9502bfe070",
    "group_norm": "01e5d9206d8afab9", "linear": "3befd3c2999ee7d8",
}


# ------------------------------------------------------------------------------------------------ the generator
def test_cover_is_deterministic_and_covers_a_toy_table():
    factors = {"a": [0, 1, 2], "b": ["x", "y"], "c": [False, True], "d": [10, 20, 30]}
    legal = legal_from([("no_a2_with_y", lambda c: not (c["a"] == 2 and c["b"] == "y"), "toy.py:1")])
    seeds = [dict(site="toy.py:2", a=2, b="x", c=True, d=30)]
    cases = cover(factors, legal, seeds, rng_seed=3)
    assert cases == cover(factors, legal, seeds, rng_seed=3) and cases[0] == seeds[0]
    assert uncovered(cases, factors, legal) == [] and all(legal({k: c[k] for k in factors}) for c in cases)
    assert (("a", 2), ("b", "y")) not in legal_pairs(factors, legal) and len(legal_pairs(factors, legal)) == 6 + 6 + 9 + 4 + 6 + 6 - 1
    assert uncovered(cases[:1], factors, legal) != [] and legal.why(dict(a=2, b="y", c=False, d=10)) == ["no_a2_with_y"]
    assert len(cases) <= 12          # 9 is the least (3 x 3 values); greedy stays close


@pytest.mark.parametrize("fam", FAMS, ids=lambda f: f.name)
def test_tables_cover_every_legal_pair(fam):
    cases = fam.cases
    assert uncovered(cases, fam.factors, fam.legal) == []
    for n, vals in fam.factors.items():
        assert {c[n] for c in cases} == set(vals), f"{n}: a value is constrained away"
    for s, c in zip(fam.seeds, cases):
        assert c == s and ":" in s["site"]
    assert all(fam.legal(fam.core(c)) for c in cases) and len(cases) <= MAX_CASES
    for name, _, reason in fam.constraints:
        assert ".py:" in reason or ".hip:" in reason, f"{name}: the reason cites no line"
    assert fam.digest() == DIGESTS[fam.name], (fam.name, fam.digest(), len(cases), len(legal_pairs(fam.factors, fam.legal)))


# ------------------------------------------------------------------------------------------------ references against the stand-ins
@functools.lru_cache(maxsize=None)
def _clean(fam_name, idx):
    """One fp32 stand-in run per case, shared by the tests below: (failures under TOL[fp16], observed, ops, refs)."""
    fam = PC.FAMILIES[fam_name]
    case = fam.cases[idx]
    ops = PC.build(fam, case, torch.bfloat16, PC.emu())
    bad, obs, _, refs = PC.run_case(fam, case, PC.emu(), ops=ops, tol_dt=torch.float16)
    if refs["out"].numel() > KEEP:          # (the few large cases are rebuilt where they are needed again, not kept for the session)
        ops = refs = None
    return bad, obs, ops, refs


KEEP = 1 << 22


def _ops_refs(fam_name, idx):
    _, _, ops, refs = _clean(fam_name, idx)
    if ops is None:
        fam = PC.FAMILIES[fam_name]
        ops = PC.build(fam, fam.cases[idx], torch.bfloat16, PC.emu())
        refs = PC.run_case(fam, fam.cases[idx], PC.emu(), ops=ops, tol_dt=torch.float16)[3]
    return ops, refs


def _index(fam, case):
    return next(i for i, c in enumerate(fam.cases) if c is case)


@pytest.mark.parametrize("fam,case", ALL)
def test_stand_in_agrees_with_the_reference(fam, case):
    bad, obs, _, _ = _clean(fam.name, _index(fam, case))
    assert not bad, (bad, obs)


@pytest.mark.parametrize("fam,case", [p for p in ALL if p.values[0].optional(p.values[1])])
def test_every_optional_operand_is_seen(fam, case):
    """Dropping it moves blockrel by at least 10 x TOL[bf16] on the case's own reference: its pairs are not vacuous."""
    ops, refs = _ops_refs(fam.name, _index(fam, case))
    for name in fam.optional(case):
        moved = PC.blockrel(fam.ref(case, PC.without(ops, name), None)["out"], refs["out"], fam.rows)
        assert moved >= 10 * PC.TOL[torch.bfloat16], (name, moved)


# ------------------------------------------------------------------------------------------------ mutants
def _m_temb_dropped_at_stride_2():
    def conv2d(x, wp, cout, stride=1, temb=None, **k):
        return EMU.conv2d(x, wp, cout, stride=stride, temb=None if stride == 2 else temb, **k)
    return PC.emu(conv2d=conv2d)


def _m_partials_over_the_unwindowed_width():
    def gn_partials_of(y, slabs, mod, x, wp, case, kw, **_):
        if kw.get("x_off", 0) > 0 and kw.get("stride", 1) == 1:
            y = mod.conv2d(x, wp, case["cout"], **dict(kw, x_off=0, wout=x.shape[2], res=None))
            return PC.emu_gn_partials(y, 1).reshape(y.shape[0], 1, 2, -1).expand(-1, slabs, -1, -1).div(slabs).reshape(-1)
        return PC.emu_gn_partials(y, slabs)
    return PC.emu(gn_partials_of=gn_partials_of)


def _m_residual_dropped_under_wrap():
    def conv2d(x, wp, cout, wrap=False, res=None, **k):
        return EMU.conv2d(x, wp, cout, wrap=wrap, res=None if wrap else res, **k)
    return PC.emu(conv2d=conv2d)


def _m_bias_alt_ignored_with_kv_group():
    def attention(q, k, v, heads, kv_group=1, bias_sel=None, **k2):
        return EMU.attention(q, k, v, heads, kv_group=kv_group, bias_sel=None if kv_group > 1 else bias_sel, **k2)
    return PC.emu(attention=attention)


def _m_scale_ignored_when_accumulating():
    def attention(q, k, v, heads, scale=None, accumulate=False, **k2):
        return EMU.attention(q, k, v, heads, scale=None if accumulate else scale, accumulate=accumulate, **k2)
    return PC.emu(attention=attention)


def _m_strided_views_read_at_the_packed_pitch():
    def attention(q, k, v, heads, kv_group=1, **k2):          # the key batch index taken without the group division when k is a strided view
        if kv_group > 1 and k.stride(1) != k.shape[2]:
            k = k.flip(0)
        return EMU.attention(q, k, v, heads, kv_group=kv_group, **k2)
    return PC.emu(attention=attention)


def _m_out_scale2_ignored_at_ragged_queries():
    def attention2(q, k, v, k2, v2, heads, out_scale2=1.0, **kw):
        return EMU.attention2(q, k, v, k2, v2, heads, out_scale2=1.0 if q.shape[1] % 32 else out_scale2, **kw)
    return PC.emu(attention2=attention2)


def _m_pair_counts_wrapped_columns_once():
    def group_norm(x, gamma, beta, groups, eps, silu=False, pad=0):
        if isinstance(x, (tuple, list)) and pad:
            scale, shift = EMU.group_norm_stats(x, gamma, beta, groups, eps, 0)
            return EMU.group_norm_apply(x, scale, shift, silu, pad)
        return EMU.group_norm(x, gamma, beta, groups, eps, silu=silu, pad=pad)
    return PC.emu(group_norm=group_norm)


def _m_residual_skipped_with_row_stats():
    def linear(x, wp, n, res=None, row_stats=False, **k):
        return EMU.linear(x, wp, n, res=None if row_stats else res, row_stats=row_stats, **k)
    return PC.emu(linear=linear)


def _m_cat_bias_dropped_with_residual():
    def conv1x1_cat(xa, xb, wp, cout, bias=None, res=None):
        return EMU.conv1x1_cat(xa, xb, wp, cout, bias=None if res is not None else bias, res=res)
    return PC.emu(conv1x1_cat=conv1x1_cat)


MUTANTS = [          # (family, the pair of factor values under which the defect fires, the defective stand-ins)
    ("conv", lambda c: c["geom"] in ("s2", "vae") and c["temb"] != "none", _m_temb_dropped_at_stride_2),
    ("conv", lambda c: c["geom"] == "pre" and c["gn"], _m_partials_over_the_unwindowed_width),
    ("conv", lambda c: c["wrap"] and c["res"], _m_residual_dropped_under_wrap),
    ("attention", lambda c: c["bias"] == "alt1" and c["group"] > 1, _m_bias_alt_ignored_with_kv_group),
    ("attention", lambda c: c["scale"] == "one" and c["out"] == "acc", _m_scale_ignored_when_accumulating),
    ("attention", lambda c: c["views"] and c["group"] > 1, _m_strided_views_read_at_the_packed_pitch),
    ("attention2", lambda c: c["scale2"] != 1.0 and c["nq"] % 32 != 0, _m_out_scale2_ignored_at_ragged_queries),
    ("group_norm", lambda c: c["form"] == "pair" and c["pad"] > 0, _m_pair_counts_wrapped_columns_once),
    ("conv1x1_cat", lambda c: c["bias"] and c["res"], _m_cat_bias_dropped_with_residual),
    ("linear", lambda c: c["res"] != "none" and c["row_stats"], _m_residual_skipped_with_row_stats),
]


@pytest.mark.parametrize("fam_name,fires,make", [m for m in MUTANTS if m[0] in PC.FAMILIES], ids=lambda v: getattr(v, "__name__", None) if callable(v) else v)
def test_a_defect_under_one_pair_is_flagged(fam_name, fires, make):
    """Judged at the loosest tolerance of the GPU tier (bf16's): what is flagged here is flagged in both dtypes.  The cases where the
    pair is absent must stay clean -- the defect is the pair's, not a factor's."""
    fam = PC.FAMILIES[fam_name]
    hit = [c for c in fam.cases if fires(fam.core(c))]
    assert hit, "no case carries the pair"
    P = make()
    flagged = 0
    # (not every carrier can show every defect: a single key makes the logits irrelevant, two wrapped columns in 36 move a variance by
    #  less than the tolerance -- one flag per defect is what the sweep promises; the cheapest carriers are tried first)
    price = fam.cost or (lambda c: 0)
    for i in sorted((i for i, c in enumerate(fam.cases) if fires(fam.core(c))), key=lambda i: price(fam.core(fam.cases[i]))):
        assert not _clean(fam_name, i)[0]
        bad, _, _, _ = PC.run_case(fam, fam.cases[i], P, ops=_ops_refs(fam_name, i)[0], tol_dt=torch.bfloat16)
        flagged += bool(bad)
        if flagged:
            break
    assert flagged >= 1, (flagged, len(hit))
    quiet = next(i for i, c in enumerate(fam.cases) if not fires(fam.core(c)))
    assert not PC.run_case(fam, fam.cases[quiet], P, ops=_ops_refs(fam_name, quiet)[0], tol_dt=torch.bfloat16)[0]
