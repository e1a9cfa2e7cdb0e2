"""GPU tier of the scope-heterogeneous cases (tests/_scope_cases.py): the reducing HIP kernels on inputs whose reduction scopes differ
-- every (image, group) of a GroupNorm, every row of a LayerNorm / LayerNorm-folded linear / ``softmax_rows`` has its own mean and
scale, and a GroupNorm scope carries profiles along H, W and its channels -- in both 16-bit dtypes, against the fp64 reference of the
STORED inputs under ``close`` (test_kernel_bounds_gpu.py, unchanged) plus ``scoperel`` < 2 TOL, the relative L2 error per scope.
Then ISOLATION, bit for bit: the same call on inputs that differ inside one scope only (8 x larger, shifted) must return identical
bits everywhere outside that scope and different bits inside it -- for GroupNorm (image; image and group, pairs, pad, a producer's
partial sums), the row kernels (the change goes into the producer's residual row, so the row statistics change too), ``attention`` /
``attention2`` (one (batch, head)'s keys and values; one query row) and ``temporal_attention`` (one (batch, pixel, head), both row
orders).  The kernels reduce in a fixed order without float atomics: a difference is a leak between scopes or a data-dependent order.
GN_FUSED is not run: off by default, it waits between workgroups, and test_kernels_gpu.py pins its bits to the three-kernel path.
tests/test_scope_cases.py is the CPU tier: builders, references, stand-ins, mutants."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _scope_cases as SC  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record  # noqa: E402
from imagine360_amd import kernels as K  # noqa: E402
from imagine360_amd import layers  # noqa: E402
from test_kernel_pairs_gpu import Dev  # noqa: E402
from test_kernels_gpu import DTYPES  # noqa: E402

torch.set_grad_enabled(False)

WORST = {}
ids = lambda d: str(d).split(".")[-1]


class Plain:
    """Places a perturbed run's operands on the device without guard bands (the guarded run is the first one)."""

    def __init__(self, dt):
        self.dt = dt

    def to(self, t, strides=None):
        return (t.to(self.dt) if t.dtype == torch.float32 else t).cuda()

    def to32(self, t):
        return t.cuda()


def _note(key, dt, ms):
    w = WORST.setdefault(f"scope_{key}_{ids(dt)}", dict(rel=0.0, blockrel=0.0, scoperel=0.0, cases=0))
    for m in ms.values():
        w.update({k: max(w[k], m[k]) for k in m})
    w["cases"] += 1
    record(f"scope_{key}_{ids(dt)}", **w)


def _run(fam, case, dt, **variant):
    switches = K.GN_MODE, K.GN_FUSED, K.GN_FROM_PRODUCER, layers.ROUTE_MIN_TOKENS
    try:
        ops = fam.build(case, dt, K)
        g = Guarded(K)
        mk = Dev(g, dt)
        d = fam.place(ops, mk)
        with g:
            results = fam.run(case, d, K, mk, **variant)
            g.out(*[t for t in results.values() if torch.is_tensor(t)])
        refs = fam.ref(case, ops, results)
        ms, worst = SC.judge(fam, results, refs, dt)
        print("SCOPE", fam.name, case["id"], variant, {n: {k: f"{v:.3e}" for k, v in m.items()} for n, m in ms.items()}, flush=True)
        _note(fam.name, dt, ms)
        bad = [(n, ms[n]) for n, ref in refs.items() if not SC.passes(results[n], ref, dt, fam.scopes)]
        assert all(results[n].dtype == dt and torch.isfinite(results[n]).all() for n in refs)
        assert not bad, (fam.name, case["id"], variant, bad)
        leaks = SC.isolation(fam, case, ops, results, K, dt, mk_of=lambda: Plain(dt), **variant)
        print("ISOLATION", fam.name, case["id"], variant, [p[0] for p in fam.perturb(case, ops, dt)], "ok" if not leaks else leaks, flush=True)
        assert not leaks, (fam.name, case["id"], variant, leaks)
    finally:
        K.GN_MODE, K.GN_FUSED, K.GN_FROM_PRODUCER, layers.ROUTE_MIN_TOKENS = switches


def _params(fam):
    return [pytest.param(c, id=c["id"]) for c in fam.cases]


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("mode", SC.GN_MODES)
@pytest.mark.parametrize("case", _params(SC.GN))
def test_group_norm_scopes(case, mode, dt):
    N, H, W = SC.gn_shape(case)
    assert K.lib().im360_gn_num_slabs(N, H, W) == SC.pick_slabs(N, H * W)          # the host restatement the CPU tier's properties use
    _run(SC.GN, case, dt, mode=mode)


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("case", _params(SC.LN))
def test_layer_norm_scopes(case, dt):
    _run(SC.LN, case, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("case", _params(SC.FOLD))
def test_folded_layer_norm_scopes(case, dt):
    _run(SC.FOLD, case, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("case", _params(SC.SM))
def test_softmax_rows_scopes(case, dt):
    _run(SC.SM, case, dt)


def _isolated(name, run, ops, perturbed, dt):
    a = run(ops)
    assert a.dtype == dt and torch.isfinite(a).all()
    for label, ops2, m in perturbed:
        bad = SC.outside_same_inside_differs(a, run(ops2), m)
        print("ISOLATION", name, label, "ok" if not bad else bad, flush=True)
        assert not bad, (name, label, bad)


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("d,two", [(64, False), (32, False), (64, True)], ids=["d64", "d32", "two-key-sets"])
def test_attention_scopes_are_isolated(d, two, dt):
    ops = SC.attn_build(d, dt, two)
    _isolated(f"attention d={d} two={two}", lambda o: SC.attn_run(o, K, Plain(dt), d), ops, SC.attn_perturb(ops, d, dt), dt)


@pytest.mark.parametrize("dt", DTYPES, ids=ids)
@pytest.mark.parametrize("frame_major", [False, True], ids=["pixel-major", "frame-major"])
def test_temporal_attention_scopes_are_isolated(frame_major, dt):
    ops = SC.tattn_build(dt)
    _isolated(f"temporal_attention frame_major={frame_major}", lambda o: SC.tattn_run(o, K, Plain(dt), frame_major), ops,
              SC.tattn_perturb(ops, dt, frame_major), dt)
