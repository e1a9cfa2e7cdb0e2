"""GPU tier of the pairwise parity sweep: every case of the covering arrays of tests/_pair_cases.py through the HIP kernels, in both
16-bit dtypes, every operand, result and workspace between guard bands (tests/_guarded.py), against the case's fp64 CPU reference
under the project's own criterion -- ``close`` of test_kernel_bounds_gpu.py: rel < TOL[dt] and blockrel(32 rows) < 2 TOL[dt]
(f = 1.5 for the two summed attention results of attention2, as the existing tests).  Extra checks where the case asks for them
(_pair_cases.failures): GroupNorm partial sums from an epilogue against the any-order fp32 summation bound over the STORED output,
bit equality with the same call without them, the slab count, group_norm of the tagged tensor; row statistics against the same bound
at n = 160; a strided ``out=`` keeps its gaps (the guard check on leaving the block).  The tables hold only combinations the wrappers
accept: nothing here exercises a refusal, loops or retries.  tests/test_pair_cases.py is the CPU tier: coverage, references, mutants."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _pair_cases as PC  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record  # noqa: E402
from imagine360_amd import kernels as K  # noqa: E402
from test_kernels_gpu import DTYPES  # noqa: E402

torch.set_grad_enabled(False)

WORST = {}


class Dev:
    """Places a case's host operands on the device between guard bands: fp32 host tensors as the 16-bit dtype, others as they are."""

    def __init__(self, g, dt):
        self.g, self.dt = g, dt

    def to(self, t, strides=None):
        return self.g.guard((t.to(self.dt) if t.dtype == torch.float32 else t).cuda(), strides=strides)

    def to32(self, t):
        return self.g.guard(t.cuda())

    def empty(self, shape, strides=None):
        return self.g.empty(shape, self.dt, "cuda", strides=strides)


def _run(fam, case, dt):
    switches = K.GN_MODE, K.GN_FUSED, K.GN_FROM_PRODUCER
    ops = PC.build(fam, case, dt, K)
    g = Guarded(K)
    mk = Dev(g, dt)
    d = PC.place(fam, case, ops, mk)
    try:
        with g:
            results = fam.call(case, d, K, mk)
            g.out(*[t for t in results.values() if torch.is_tensor(t)])
    finally:
        K.GN_MODE, K.GN_FUSED, K.GN_FROM_PRODUCER = switches
    assert results["out"].dtype == dt
    if case.get("out") in ("strided", "acc"):
        assert results["out"].stride() == PC.attn_out_strides(case)
    refs = fam.ref(case, ops, results)
    refs.update({k: ops[k] for k in ("gamma", "beta") if k in ops})
    bad, obs = PC.failures(fam, case, results, refs, dt)
    key = f"pairs_{fam.name}_{str(dt).split('.')[-1]}"
    w = WORST.setdefault(key, dict(rel=0.0, blockrel=0.0, cases=0))
    w.update(rel=max(w["rel"], obs[0]), blockrel=max(w["blockrel"], obs[1]), cases=w["cases"] + 1)
    print("PAIR", fam.name, fam.case_id(case), f"rel {obs[0]:.3e} blockrel {obs[1]:.3e}", flush=True)
    record(key, **w)
    assert not bad, (fam.case_id(case), case.get("site"), bad)


def _params(fam):
    return [pytest.param(c, id=fam.case_id(c)) for c in fam.cases]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", _params(PC.CONV))
def test_conv2d_pairs(dt, case):
    N, H, W, _, _ = PC.conv_geometry(case)
    if case["taps"] == 9:          # the launch class is the one the table names: a knob change cannot silently move a case off its path
        plan = K.lib().im360_conv_ksplit_plan(N, H, W, case["cin"], case["cout"], 9, int(case["geom"] == "up"), int(case["wrap"]), int(case["gn"]))
        assert plan == (PC.KSPLIT_PARTS if case["launch"] == "ksplit" else 1), plan
    tiles = -(-N * H * W // 256) * (case["cout"] // 320)
    assert (tiles >= 512) == (case["launch"] == "big") or case["cout"] % 320, tiles
    _run(PC.CONV, case, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", _params(PC.UP2))
def test_conv_up2_pairs(dt, case):
    _run(PC.UP2, case, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", _params(PC.CAT))
def test_conv1x1_cat_pairs(dt, case):
    _run(PC.CAT, case, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", _params(PC.LIN))
def test_linear_family_pairs(dt, case):
    _run(PC.LIN, case, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", _params(PC.ATTN))
def test_attention_pairs(dt, case):
    _run(PC.ATTN, case, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", _params(PC.ATTN2))
def test_attention2_pairs(dt, case):
    _run(PC.ATTN2, case, dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", _params(PC.GN))
def test_group_norm_pairs(dt, case):
    _run(PC.GN, case, dt)
