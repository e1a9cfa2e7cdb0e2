"""``guidance_interval`` on the MI355X: the unguided step kernels (csrc/sampler_step.hip, GUIDED = false) against their guided siblings
fed (c, c) -- the same bits, for any guidance -- and against the per-element bound of _ref_step.py; their refusals and guard bands; and
the pipeline on the small pipe of _release_pipe.py with the interval (0.2, 0.6) on 4 steps: batch 1, 2, 2, 1, every eager step the
guided kernel on what the model returned, the RNG streams where they stand without the keyword, graph replay (two graphs) equal to
eager in every loop variant."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import _interval_runs as IR  # noqa: E402
import _ref_step as R  # noqa: E402
import _release_pipe as RP  # noqa: E402
import _step_cases as C  # noqa: E402
import _unguided_cases as UC  # noqa: E402
import test_kernel_bounds_gpu as B  # noqa: E402
from _emu_keep_latents import half_mask, kept  # noqa: E402
from _guarded import Guarded  # noqa: E402
from helpers import record as _record  # noqa: E402
from imagine360_amd import configs, kernels as K  # noqa: E402
from imagine360_amd.context import WindowPlan  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402

torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("family", UC.FAMILIES)
@pytest.mark.parametrize("dt", C.DTYPES, ids=C.dtname)
def test_unguided_step_kernels_parity(dt, family):
    """Every non-rescale case of _step_cases.py with u := c (update, ddim, multistep; ddim_windows and multistep_windows on a line and
    on a ring; first and second order; with and without noise; 16-byte lanes and the scalar path), scalar and device coefficients:
    (a) torch.equal with the guided sibling on (c, c) at guidance 7.5 and at 1.0 -- out and fp32 history; (b) within the bound of
    _ref_step.py of the fp64 restatement of the unguided step."""
    worst, failures, cache, n = {}, [], {}, 0
    for case in UC.cases(dt, family):
        ref4 = UC.reference(case)
        for coef_dev in (False, True):
            out, hist = UC.call(K, case, device="cuda", coef_dev=coef_dev, cache=cache)
            assert out.dtype == case.dt and out.shape == case.x.shape
            for g in (C.G, 1.0):
                want, want_hist = C.call(K, UC.with_guidance(case, g), device="cuda", coef_dev=coef_dev, cache=cache)
                if not (torch.equal(out, want) and (hist is None or torch.equal(hist, want_hist))):
                    failures.append(f"{case.name} coef_dev={coef_dev}: not the bits of the guided sibling on (c, c) at guidance {g}")
            try:
                C.check(case, out, hist, ref4, 0.0, worst)
            except R.Outside as e:
                worst["out"] = max(worst.get("out", 0.0), e.worst)
                failures.append(f"{'coef_dev ' if coef_dev else ''}{e}")
            if hist is not None and case.coefs[5] == 0.0:           # first order: the NaN history is not read
                assert torch.isfinite(out.float()).all() and torch.isfinite(hist).all(), case.name
        n += 1
    _record(f"unguided_step_{family}_{C.dtname(dt)}", cases=n, worst_err_over_bound=worst.get("out", 0.0),
            **({"worst_hist_err_over_bound": worst["hist"]} if "hist" in worst else {}))
    assert n > 0 and not failures, f"{len(failures)} failures, the first ones:\n" + "\n".join(failures[:12])


def test_unguided_entry_points_reject_what_their_siblings_reject():
    a = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    h = torch.zeros(24, dtype=torch.float32, device="cuda")
    lib, p, hp = K.lib(), a.data_ptr(), h.data_ptr()
    ddim, ms = (7.5, 0.5, 0.8, 0.6, 0.7, 0.0), (7.5, 0.5, 0.8, 0.6, 0.7, -0.3)
    tail = (0, None, None)                                            # dtype, stream, coef_dev

    def both(new, old, text):
        """The same non-zero code and the same complaint from the new entry point and from its sibling."""
        rc_new, err_new = new(), lib.im360_last_error()
        rc_old, err_old = old(), lib.im360_last_error()
        assert rc_new == rc_old != 0 and text in err_new and text in err_old, (rc_new, rc_old, err_new, err_old)
    both(lambda: lib.im360_ddim_update(None, p, p, 16, 0.5, 0.5, *tail), lambda: lib.im360_cfg_ddim_update(None, p, p, p, 16, 7.5, 0.5, 0.5, *tail), b"null pointer")
    both(lambda: lib.im360_ddim_update(p, p, p, 12, 0.5, 0.5, *tail), lambda: lib.im360_cfg_ddim_update(p, p, p, p, 12, 7.5, 0.5, 0.5, *tail), b"multiple of 8")
    both(lambda: lib.im360_ddim_update(p + 2, p, p, 8, 0.5, 0.5, *tail), lambda: lib.im360_cfg_ddim_update(p, p + 2, p, p, 8, 7.5, 0.5, 0.5, *tail), b"misaligned")
    both(lambda: lib.im360_ddim_update(p, p, p, 16, 0.5, 0.5, 7, None, None), lambda: lib.im360_cfg_ddim_update(p, p, p, p, 16, 7.5, 0.5, 0.5, 7, None, None),
         b"dtype 7 unsupported")
    both(lambda: lib.im360_ddim_step(p, None, None, p, 16, *ddim[1:], 1, *tail), lambda: lib.im360_cfg_ddim_step(p, p, None, None, p, 16, *ddim, 1, *tail), b"null pointer")
    both(lambda: lib.im360_ddim_step(p, p, None, p, 16, *ddim[1:], 3, *tail), lambda: lib.im360_cfg_ddim_step(p, p, p, None, p, 16, *ddim, 3, *tail), b"mode 3 unsupported")
    both(lambda: lib.im360_ddim_step(p, p, None, p, 16, *ddim[1:5], 0.2, 1, *tail), lambda: lib.im360_cfg_ddim_step(p, p, p, None, p, 16, *ddim[:5], 0.2, 1, *tail),
         b"needs a noise tensor")
    both(lambda: lib.im360_multistep_step(p, p, None, p, 16, *ms[1:], 1, *tail),
         lambda: lib.im360_cfg_multistep_step(p, p, p, None, p, 16, *ms, 1, 0.0, None, 0, *tail), b"null pointer")
    both(lambda: lib.im360_multistep_step(p, p, hp, p, 16, *ms[1:], 1 | 8, *tail),
         lambda: lib.im360_cfg_multistep_step(p, p, p, hp, p, 16, *ms, 1 | 8, 0.0, None, 0, *tail), b"bit 8")
    both(lambda: lib.im360_multistep_step(p, p, hp + 4, p, 16, *ms[1:], 1, *tail),
         lambda: lib.im360_cfg_multistep_step(p, p, p, hp + 4, p, 16, *ms, 1, 0.0, None, 0, *tail), b"misaligned")
    st = torch.zeros(2, dtype=torch.int32, device="cuda").data_ptr()
    w = torch.ones(4, dtype=torch.float32, device="cuda").data_ptr()
    geo = lambda L: (2, 1, 6, L, 8)                                   # nW, outer, F, L, inner
    for suffix in ("", "_ring"):
        new, old = getattr(lib, "im360_ddim_step_windows" + suffix), getattr(lib, "im360_cfg_ddim_step_windows" + suffix)
        both(lambda: new(p, p, None, p, None, w, *geo(4), *ddim[1:], 1, *tail), lambda: old(p, p, None, p, None, w, *geo(4), *ddim, 1, *tail), b"null pointer")
        both(lambda: new(p, p, None, p, st, w, *geo(7), *ddim[1:], 1, *tail), lambda: old(p, p, None, p, st, w, *geo(7), *ddim, 1, *tail), b"out of range")
        both(lambda: new(p, p, None, p, st, w, *geo(4), *ddim[1:], 7, *tail), lambda: old(p, p, None, p, st, w, *geo(4), *ddim, 7, *tail), b"mode 7 unsupported")
        both(lambda: new(p, p, None, p, st + 2, w, *geo(4), *ddim[1:], 1, *tail), lambda: old(p, p, None, p, st + 2, w, *geo(4), *ddim, 1, *tail), b"misaligned table")
    new, old = lib.im360_multistep_step_windows, lib.im360_cfg_multistep_step_windows
    both(lambda: new(p, p, hp, p, st, w, *geo(4), 3, *ms[1:], 1, *tail), lambda: old(p, p, hp, p, st, w, *geo(4), 3, *ms, 1, 0.0, None, 0, *tail), b"wrap=3")
    both(lambda: new(p, p, None, p, st, w, *geo(4), 0, *ms[1:], 1, *tail), lambda: old(p, p, None, p, st, w, *geo(4), 0, *ms, 1, 0.0, None, 0, *tail), b"null pointer")
    both(lambda: new(p, p, hp, p, st, w, *geo(4), 6, *ms[1:], 1 | 8, *tail), lambda: old(p, p, hp, p, st, w, *geo(4), 6, *ms, 1 | 8, 0.0, None, 0, *tail), b"bit 8")
    # the wrappers: the layout of the one-half buffer, the history, the noise
    x = torch.zeros(1, 4, 6, 1, 8, dtype=torch.bfloat16, device="cuda")
    two = torch.zeros(2, 2, 4, 4, 1, 8, dtype=torch.bfloat16, device="cuda")
    sd, wd = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.ones(4, dtype=torch.float32, device="cuda")
    with pytest.raises(AssertionError):
        K.ddim_step_windows(two, x, None, sd, wd, 1, ddim)                  # a CFG-batched buffer is not what the unguided step takes
    with pytest.raises(ValueError, match="history"):
        K.multistep_step(a, a, None, 1, ms)
    with pytest.raises(ValueError, match="sigma > 0 needs a noise tensor"):
        K.ddim_step(a, a, None, 1, ddim[:5] + (0.3,))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", B.DTYPES)
def test_unguided_plain_kernels_guard_bands(dt):
    """The ragged edge of the plain launches (420 lanes of 8: one full workgroup and a partial one) between guards: nothing stored outside
    ``out`` / ``hist``, nothing left unwritten, and the guided sibling's bits on (c, c)."""
    c, x, z = (B.q16(B.rnd(*B.SHAPE, seed=s), dt) for s in (32, 33, 34))
    c = B.q16(c * 0.25, dt)
    hist = B.rnd(*B.SHAPE, seed=35)
    ms = (7.5, 0.8, 0.6, 0.9, 1.4, -0.5)
    g = Guarded(K)
    dc, dx, dz = (B.dn(g, t, dt) for t in (c, x, z))
    h0, h1 = B.dn(g, hist), B.dn(g, hist)
    with g:
        outs = [g.out(K.ddim_update(dc, dx, 0.83, -0.41)), g.out(K.ddim_step(dc, dx, dz, 1 | 4, B.COEFS)),
                g.out(K.ddim_step(dc, dx, None, 0 | 8, B.COEFS[:5] + (0.0,))), g.out(K.multistep_step(dc, dx, h0, 1 | 4, ms))]
        g.out(h0)
    want = [K.cfg_ddim_update(dc, dc, dx, 7.5, 0.83, -0.41), K.cfg_ddim_step(dc, dc, dx, dz, 1 | 4, B.COEFS),
            K.cfg_ddim_step(dc, dc, dx, None, 0 | 8, B.COEFS[:5] + (0.0,)), K.cfg_multistep_step(dc, dc, dx, h1, 1 | 4, ms)]
    assert all(torch.equal(a, b) for a, b in zip(outs, want)) and torch.equal(h0, h1)


@pytest.mark.parametrize("dt", B.DTYPES)
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("inner_hw", [(1, 8), (3, 8), (1, 7)])      # inner 8 and 24: 16-byte lanes; 7: the scalar path
def test_unguided_windows_kernels_guard_bands(dt, ring, inner_hw):
    """The [nW, 1, ...] buffer sits directly against its back guard (NaN bits): a read of a second prediction half, a store outside
    ``out`` / ``hist`` or a lane left unwritten fails; the result is the guided sibling's on a buffer with both halves equal."""
    preds, x, z, starts, w = B._windows_case(dt, inner_hw, ring, seed=170)
    one = preds[:, 1:2].contiguous()
    hist = B.rnd(*x.shape, seed=173)
    ms = (7.5, 0.8, 0.6, 0.9, 1.4, -0.5)
    g = Guarded(K)
    dp, dx, dz = (B.dn(g, t, dt) for t in (one, x, z))
    ds, dw = B.dn(g, torch.tensor(starts, dtype=torch.int32)), B.dn(g, w)
    h0 = B.dn(g, hist)
    with g:
        out = g.out(K.ddim_step_windows(dp, dx, dz, ds, dw, 1 | 4, B.COEFS, ring=ring))
        out_ms = g.out(K.multistep_step_windows(dp, dx, h0, ds, dw, 1 | 4, ms, ring=ring))
        g.out(h0)
    both = one.expand(-1, 2, *one.shape[2:]).contiguous().to(dt).cuda()
    h1 = hist.cuda()
    assert torch.equal(out, K.cfg_ddim_step_windows(both, dx, dz, ds, dw, 1 | 4, B.COEFS, ring=ring))
    assert torch.equal(out_ms, K.cfg_multistep_step_windows(both, dx, h1, ds, dw, 1 | 4, ms, ring=ring)) and torch.equal(h0, h1)


# ------------------------------------------------------------------------------------------------ 2. the pipeline
@pytest.fixture(scope="module")
def run():
    return RP.make_runner(RP.make_clip())


def _model(run):
    """The model of the shared runner (it builds one and keeps it in its closure)."""
    return dict(zip(run.__code__.co_freevars, (c.cell_contents for c in run.__closure__)))["mv"]


def _ddim():
    return DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)


def _dpm():
    return DPMSolverMultistepScheduler(**configs.NOISE_SCHEDULER_KWARGS)


RING = dict(context_frames=4, context_overlap=2, context_loop=True)


@pytest.fixture(scope="module")
def eager(run):
    """{(scheduler, windows): the eager run with the interval}, computed once and left unchanged."""
    return {(s, w): run(False, scheduler=(_dpm if s == "dpm" else _ddim)(), guidance_interval=IR.INTERVAL, **(RING if w else {}))
            for s in ("ddim", "dpm") for w in (False, True)}


class _CountedGraphs:
    """Counts the captured graphs through their constructor."""

    def __init__(self, monkeypatch):
        self.n = 0
        real = torch.cuda.CUDAGraph

        def counted(*a, **k):
            self.n += 1
            return real(*a, **k)
        monkeypatch.setattr(torch.cuda, "CUDAGraph", counted)


@pytest.mark.parametrize("windows", [False, True], ids=["one_block", "ring_windows"])
def test_eager_steps_are_the_guided_kernels_on_what_the_model_returned(run, monkeypatch, windows):
    """Batch sizes 1, 2, 2, 1 (per window), and every traced latent recomputed with the real GUIDED kernels -- (c, c) on the unguided
    steps -- bit for bit.  Then the shared-RNG claim, directly: after an eager run with the interval and one without, from the same
    seeds, the device generator and Python's stand where they stood."""
    mv, sch, extra = _model(run), _ddim(), (RING if windows else {})
    plan = WindowPlan(RP.FRAMES, 4, 2, "pyramid", "cuda", loop=True) if windows else None
    with IR.recording(mv, monkeypatch) as rec:
        trace = []
        got = run(False, scheduler=sch, guidance_interval=IR.INTERVAL, trace=trace, **extra)
        state = torch.cuda.get_rng_state(), random.getstate()
        nW = 1 if plan is None else len(plan)
        assert rec.batches() == [b for k in IR.KINDS for b in [2 if k else 1] * nW]
        want = IR.recompute_trace(sch, rec, sch._timesteps_host, IR.KINDS, plan=plan)
    assert len(trace) == 4 and all(torch.equal(a, b) for a, b in zip(trace, want)) and torch.equal(got[1], trace[-1])
    plain = run(False, scheduler=_ddim(), trace=[], **extra)
    assert torch.equal(torch.cuda.get_rng_state(), state[0]) and random.getstate() == state[1]
    assert not torch.equal(plain[1], got[1]) and mv._ip_noise_half is None
    assert all(u.ip_cache_entries == 1 and not any(isinstance(k, tuple) for k in u._ip_cache._store) for u in (mv.unet, mv.pano_unet))


@pytest.mark.parametrize("windows", [False, True], ids=["one_block", "ring_windows"])
@pytest.mark.parametrize("sampler", ["ddim", "dpm"])
def test_graph_replay_is_the_eager_run(run, eager, monkeypatch, sampler, windows):
    graphs = _CountedGraphs(monkeypatch)
    got = run(True, scheduler=(_dpm if sampler == "dpm" else _ddim)(), guidance_interval=IR.INTERVAL, **(RING if windows else {}))
    assert graphs.n == 2 and RP.same(got, eager[(sampler, windows)])


def test_graphed_regenerate_mask_keeps_the_init(run, eager):
    x0 = eager[("ddim", False)][1]
    half = half_mask(RP.FRAMES, *RP.PANO_HW)
    got = run(True, init_latents=x0, strength=RP.STRENGTH, regenerate_mask=half, guidance_interval=IR.INTERVAL)
    keep = kept(half, *RP.LAT_HW).to(x0.device).expand_as(x0)
    assert torch.equal(got[1][keep], x0[keep]) and not torch.equal(got[1][~keep], x0[~keep])


def test_free_init_passes_replay_both_graphs(run, monkeypatch):
    want = run(False, guidance_interval=IR.INTERVAL, free_init_iters=2)
    graphs = _CountedGraphs(monkeypatch)
    got = run(True, guidance_interval=IR.INTERVAL, free_init_iters=2)
    assert graphs.n == 2 and RP.same(got, want)                      # both graphs captured once, restarted for the second pass


def test_a_covering_interval_is_none_and_one_graph(run, monkeypatch):
    graphs = _CountedGraphs(monkeypatch)
    plain = run(True)
    assert graphs.n == 1
    for interval in (None, (0, 1)):
        assert RP.same(run(True, guidance_interval=interval), plain)
    assert graphs.n == 3


def test_an_empty_interval_never_runs_the_cfg_batch(run, monkeypatch):
    mv = _model(run)
    with IR.recording(mv, monkeypatch) as rec:
        want = run(False, guidance_interval=(0.3, 0.3), trace=[])
        assert rec.batches() == [1] * 4
        graphs = _CountedGraphs(monkeypatch)
        got = run(True, guidance_interval=(0.3, 0.3))
        assert graphs.n == 1 and set(rec.batches()) == {1}           # warm-up and capture included
    assert RP.same(got, want)
