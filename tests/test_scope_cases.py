"""CPU tier of the scope-heterogeneous cases (tests/_scope_cases.py): the builders are deterministic and heterogeneous in the STORED
tensors, the fp64 references rounded once keep 3 x room under every threshold, the plain-torch stand-ins pass every case under both
criteria (which validates the references) and are isolated bit for bit, and stand-ins with ONE defect in how statistics are gathered
miss a threshold by at least 3 x in both 16-bit dtypes -- while three of them pass ``close`` on the iid inputs of ``test_group_norm``.
The same cases run against the HIP kernels in tests/test_scope_kernels_gpu.py."""
import functools

import pytest
import torch

import _scope_cases as SC
from test_kernels_gpu import TOL, q16, rnd

torch.set_grad_enabled(False)

ALL = [pytest.param(f, c, id=f"{f.name}-{c['id']}") for f in SC.FAMILIES.values() for c in f.cases]
ids = lambda d: str(d).split(".")[-1]


KEEP = 1 << 22          # (the one large case is rebuilt where it is needed again, not kept for the session)


@functools.lru_cache(maxsize=None)
def _kept(fam_name, idx, dt):
    fam = SC.FAMILIES[fam_name]
    got = SC.run_case(fam, fam.cases[idx], SC.emu(), dt)
    return got if max(r.numel() for r in got[2].values()) <= KEEP else None


def _clean(fam_name, idx, dt):
    """One stand-in run per case and dtype, shared by the tests below and never modified: (ops, results, refs)."""
    fam = SC.FAMILIES[fam_name]
    return _kept(fam_name, idx, dt) or SC.run_case(fam, fam.cases[idx], SC.emu(), dt)


def _index(fam, case):
    return next(i for i, c in enumerate(fam.cases) if c is case)


# ------------------------------------------------------------------------------------------------ the builders
@pytest.mark.parametrize("fam,case", ALL)
def test_builders_are_deterministic(fam, case):
    a, b = fam.build(case, SC.BF16, SC.emu()), fam.build(case, SC.BF16, SC.emu())
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
    assert all(torch.equal(v, q16(v, SC.BF16)) for k, v in a.items() if torch.is_tensor(v) and k in ("x_a", "x_b", "src_a", "w_a", "x", "hres", "src"))


@pytest.mark.parametrize("dt", SC.DTYPES, ids=ids)
@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in SC.GN_CASES if c["kind"] == "hetero"])
def test_group_norm_inputs_are_heterogeneous_as_stored(case, dt):
    """Of the STORED members -- a tagged one is what its producer wrote.  spread: the scope means spread (standard deviation) at least
    4 x the median within-scope std; ratio: |mean| / std <= 8 in every scope (fp32 partial sums enter var = E[x^2] - mean^2 amplified by
    1 + ratio^2: with GN_SUM_BOUND below 1e-3); the outer columns' and the last slab's mean at least 0.5 std off the scope's mean."""
    _, results, _ = _clean("group_norm", _index(SC.GN, case), dt)
    rep = SC.hetero_report(SC.gn_stored(results))
    print("HETERO", case["id"], ids(dt), {k: (None if v is None else round(v, 3)) for k, v in rep.items()})
    assert rep["spread"] >= 4.0 and rep["ratio"] <= 8.0 and rep["scale_span"] >= 8.0, rep
    assert (1 + rep["ratio"] ** 2) * SC.PC.GN_SUM_BOUND < 1e-3
    assert rep["pad_dev"] is None or rep["pad_dev"] >= 0.5, rep
    assert rep["slab_dev"] is None or rep["slab_dev"] >= 0.5, rep
    H, W = (int(s) for s in case["hw"].split("x"))
    assert (rep["pad_dev"] is None) == (W <= 2 * SC.PAD_COLS) and (rep["slab_dev"] is None) == (SC.pick_slabs(SC.gn_shape(case)[0], H * W) == 1)


def test_group_norm_cases_reach_the_slab_partitions_they_name():
    assert SC.pick_slabs(3, 16 * 32) == 8 and SC.pick_slabs(3, 16 * 36) == 9 and SC.pick_slabs(2, 130) == 2 and SC.pick_slabs(2, 128) == 2
    assert SC.pick_slabs(1, 63) == 1 and SC.pick_slabs(3, 256) == 4 and SC.pick_slabs(2, 64) == 1 and SC.pick_slabs(3, 4) == 1
    for c in SC.GN_CASES:          # the straddling groups
        if len(c["chans"]) == 2:
            cpg = sum(c["chans"]) // SC.GROUPS
            assert (c["chans"][0] % cpg != 0) == (c["id"] != "pair-320+320-6x10-pad2")
    assert SC.gn_probe_group(SC.GN_CASES[6]) == 21 and SC.gn_probe_group(SC.GN_CASES[7]) == 21


@pytest.mark.parametrize("dt", SC.DTYPES, ids=ids)
def test_dedicated_group_norm_scopes(dt):
    """8 samples per scope; scopes of std 2^-8 / 2^-6 around 0; the exactly constant group, whose reference is act(beta)."""
    small = next(c for c in SC.GN_CASES if c["kind"] == "small")
    x = SC.gn_stored(_clean("group_norm", _index(SC.GN, small), dt)[1])
    assert x.shape[1] * x.shape[2] * (x.shape[3] // SC.GROUPS) == 8
    for case in (c for c in SC.GN_CASES if c["kind"] == "flat"):
        ops, results, refs = _clean("group_norm", _index(SC.GN, case), dt)
        x = SC.gn_stored(results)
        N, H, W, C = x.shape
        t = x.double().reshape(N, H * W, SC.GROUPS, C // SC.GROUPS)
        mean, std = t.mean(dim=(1, 3)), t.std(dim=(1, 3), unbiased=False)
        n, g, v = SC.FLAT_CONST
        assert float(std[n, g]) == 0.0 and float(mean[n, g]) == v
        keep = torch.ones_like(std, dtype=torch.bool)
        keep[n, g] = False
        assert float((mean.abs() / std)[keep].max()) < 0.5                      # around 0
        lows, highs = (std[keep] < 2.0 ** -7), (std[keep] >= 2.0 ** -7)
        assert int(lows.sum()) >= 20 and int(highs.sum()) >= 20
        assert float((std[keep][lows] / 2.0 ** -8 - 1).abs().max()) < 0.2 and float((std[keep][highs] / 2.0 ** -6 - 1).abs().max()) < 0.2
        lo, hi = SC.gn_group_channels(case, g)
        beta = ops["beta"].double()[lo:hi]
        want = (torch.nn.functional.silu(beta) if case["silu"] else beta).expand(H, W, hi - lo)
        # (F.group_norm evaluates x scale + shift: beta up to the rounding of 0.375 rstd gamma in fp64)
        assert float((refs["out"][n, :, :, lo:hi] - want).abs().max()) < 1e-9 and torch.isfinite(results["out"]).all()


@pytest.mark.parametrize("dt", SC.DTYPES, ids=ids)
def test_row_inputs_are_heterogeneous_as_stored(dt):
    for fam, name in ((SC.LN, "x"), (SC.FOLD, "h")):
        for i, case in enumerate(fam.cases):
            ops, results, _ = _clean(fam.name, i, dt)
            x = (ops[name] if name in ops else results[name]).double()
            M = x.shape[0]
            low, const = SC.special_rows(M)
            mean, std = x.mean(1), x.std(1, unbiased=False)
            assert float(std[const]) == 0.0 and float(mean[const]) == SC.ROW_CONST
            assert float((std[low] / SC.LOW_STD - 1).abs().max()) < 0.25 and float((mean[low].abs() / std[low]).max()) < 0.5
            rest = torch.ones(M, dtype=torch.bool)
            rest[low + [const]] = False
            assert float((mean[rest].abs() / std[rest]).max()) <= 8.0
            if M >= 64:          # (the 5-row cases are there for the ragged last wave)
                assert float(std[rest].max() / std[rest].min()) >= 16.0 and float(mean[rest].std() / std[rest].median()) >= 1.0
            if fam is SC.FOLD:          # the slices of a row differ: their means spread at least half the row's std
                sl = x.reshape(M, -1, 160).mean(-1)
                assert float(((sl.max(1).values - sl.min(1).values) / std)[rest].median()) >= 0.5
    x = SC.sm_build(SC.SM_CASES[0], dt)["x"]
    assert float(x.max()) * SC.SM_CASES[0]["scale"] > 89 and float(x.min()) * SC.SM_CASES[0]["scale"] < -89          # exp overflows in fp32 without the maximum
    assert float(x[SC.SM_EQUAL].std()) == 0.0


# ------------------------------------------------------------------------------------------------ references and stand-ins
@pytest.mark.parametrize("dt", SC.DTYPES, ids=ids)
@pytest.mark.parametrize("fam,case", ALL)
def test_reference_rounded_once_keeps_room_and_stand_in_passes(fam, case, dt):
    _, results, refs = _clean(fam.name, _index(fam, case), dt)
    for name, ref in refs.items():
        m = SC.measures(q16(ref.float(), dt), ref, fam.scopes)
        assert SC.factor(m, dt) * SC.ROOM <= 1.0, ("the reference rounded once", name, m)
        assert SC.passes(results[name], ref, torch.float16, fam.scopes), ("stand-in, fp32", name, SC.measures(results[name], ref, fam.scopes))
        assert SC.passes(q16(results[name], dt), ref, dt, fam.scopes), ("stand-in, rounded", name)


@pytest.mark.parametrize("fam,case", ALL)
def test_stand_ins_are_isolated(fam, case):
    ops, results, _ = _clean(fam.name, _index(fam, case), SC.BF16)
    assert SC.isolation(fam, case, ops, results, SC.emu(), SC.BF16) == []
    labels = [p[0] for p in fam.perturb(case, ops, SC.BF16)]
    assert labels == (["row"] if fam is not SC.GN else ["image"] * (SC.gn_shape(case)[0] > 1) + ["image-group"] * (case["tag"] in ("none", "first")))


@pytest.mark.parametrize("d", [64, 32])
def test_attention_stand_ins_are_isolated(d):
    for two in ([False, True] if d == 64 else [False]):
        ops = SC.attn_build(d, SC.BF16, two)
        a = SC.attn_run(ops, SC.emu(), SC.Host(), d)
        for label, ops2, m in SC.attn_perturb(ops, d, SC.BF16):
            assert SC.outside_same_inside_differs(a, SC.attn_run(ops2, SC.emu(), SC.Host(), d), m) == [], label
    for fm in (False, True):
        ops = SC.tattn_build(SC.BF16)
        a = SC.tattn_run(ops, SC.emu(), SC.Host(), fm)
        for label, ops2, m in SC.tattn_perturb(ops, SC.BF16, fm):
            assert SC.outside_same_inside_differs(a, SC.tattn_run(ops2, SC.emu(), SC.Host(), fm), m) == [], (label, fm)


# ------------------------------------------------------------------------------------------------ mutants
def _trip(name, dt):
    """(the largest factor by which the mutant misses a threshold over the family's cases, the case) -- stops at the first >= ROOM."""
    fam, make = SC.MUTANTS[name]
    P = make()
    best = (0.0, None)
    for i, case in enumerate(fam.cases):
        ops, _, refs = _clean(fam.name, i, dt)
        for variant in fam.variants[:1]:
            _, results, refs2 = SC.run_case(fam, case, P, dt, ops=ops, **variant)
            f = SC.judge(fam, results, refs2, dt, round_to=dt)[1]
            if f > best[0]:
                best = (f, case["id"])
        if best[0] >= 4 * SC.ROOM:
            break
    return best


@pytest.mark.parametrize("name", list(SC.MUTANTS))
def test_a_defect_in_the_statistics_trips_a_threshold_by_3x_in_both_dtypes(name):
    for dt in SC.DTYPES:
        f, where = _trip(name, dt)
        print("MUTANT", name, ids(dt), f"{f:.1f} x at {where}")
        assert f >= SC.ROOM, (name, ids(dt), f, where)


def test_three_defects_pass_on_iid_inputs_and_fail_here():
    """The motivation, kept honest: on the iid inputs of ``test_group_norm`` (2 x 16 x 32 x 320, pad 2, bf16) a GroupNorm that drops the
    last slab, weights the wrapped columns once or draws the group boundaries one channel late passes ``close`` (fp64 + SiLU, rounded
    once); on the heterogeneous case of the same shape class each misses it."""
    dt = SC.BF16
    x = q16(rnd(2, 16, 32, 320, seed=16) + 0.5, dt)
    gamma, beta = q16(1 + 0.1 * rnd(320, seed=17), dt), q16(0.1 * rnd(320, seed=18), dt)
    ref = SC.gn64(x, gamma, beta, 1e-5, 2, True)
    case = next(c for c in SC.GN_CASES if c["id"] == "320-16x32-pad2")
    ops, _, refs = _clean("group_norm", _index(SC.GN, case), dt)
    for mut in ("last_slab", "pad_once", "late"):
        out = q16(SC.gn64_mutant(x, gamma, beta, 1e-5, 2, True, mut).float(), dt)
        m = SC.measures(out, ref, SC.gn_scopes)
        print("IID", mut, {k: f"{v:.2e}" for k, v in m.items()})
        assert SC.close(out, ref, dt), (mut, m)
        bad = q16(SC.gn64_mutant(ops["x_a"], ops["gamma"], ops["beta"], 1e-5, 2, True, mut).float(), dt)
        assert not SC.close(bad, refs["out"], dt) and SC.factor(SC.measures(bad, refs["out"], SC.gn_scopes), dt) >= SC.ROOM, mut
    assert SC.close(q16(ref.float(), dt), ref, dt) and TOL[dt] == 1e-2
