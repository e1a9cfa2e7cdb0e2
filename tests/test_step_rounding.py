"""The per-element rounding bound of the sampler-step family on CPU (_ref_step.py): its fp64 restatement agrees with the restatements
the suite already has, every torch stand-in of the family meets the bound on all cases the kernels are run on
(test_step_rounding_gpu.py), and perturbed copies of the stand-ins -- a coefficient a few parts in a thousand off, a dropped clamp,
a shifted weight table, a history not written -- do not, although the whole-tensor ``rel < TOL`` of the older tests accepts most."""
import types

import pytest
import torch

import _emu_ctx_step as EC
import _emu_ddim_step as ES
import _emu_kernels as E
import _emu_multistep_step as EM
import _emu_rescale_step as ER
import _emu_ring_step as EG
import _ref_step as R
import _step_cases as C
from helpers import rel
from imagine360_amd.context import context_weights
from test_context_windows import TOL, VIEW_SHAPES, host_windows_step, windows_case

torch.set_grad_enabled(False)
FACTOR_TOL = 2e-6          # test_guidance_rescale_gpu.py (the agreement test below checks that it still says so)

# the newest stand-in of every entry point; rescale = 0 / ring = False delegate down to _emu_ddim_step.py / _emu_ctx_step.py
STAND_INS = types.SimpleNamespace(cfg_ddim_update=E.cfg_ddim_update, cfg_ddim_step=ER.cfg_ddim_step, cfg_ddim_step_windows=EG.cfg_ddim_step_windows,
                                  cfg_multistep_step=EM.cfg_multistep_step, cfg_multistep_step_windows=EM.cfg_multistep_step_windows)
OLDEST = types.SimpleNamespace(cfg_ddim_step=ES.cfg_ddim_step, cfg_ddim_step_windows=EC.cfg_ddim_step_windows)


# ------------------------------------------------------------------------------------------------ 1. one definition, not a third
def test_agrees_with_the_existing_restatements():
    import test_context_loop as TL
    import test_ddim_stochastic_gpu as TD
    import test_guidance_rescale_gpu as TR
    import test_multistep_sampler_gpu as TM
    assert TR.FACTOR_TOL == FACTOR_TOL and TD.TOL == TOL
    tol = 1e-14
    coefs = C.ddim_coefficients()
    for dt in C.DTYPES:
        # _host_step / _host_rescaled_step on the inputs of test_cfg_ddim_step_kernel_all_modes (seed 51)
        gen = torch.Generator().manual_seed(51)
        u, c, x, z = (torch.randn(C.SHAPE, generator=gen).to(dt) for _ in range(4))
        u, c = u * 0.25, c * 0.25
        for eta in (0.0, 0.8):
            cf, noise = coefs[(8, eta)], z if eta > 0 else None
            for mode in C.DDIM_MODES:
                assert rel(R.cfg_ddim_step(u, c, x, noise, mode, cf)[0], TD._host_step(u, c, x, noise, mode, cf)) < tol
                assert rel(R.cfg_ddim_step(u, c, x, noise, mode, cf, 0.7)[0], TR._host_rescaled_step(u, c, x, noise, mode, cf, 0.7)) < tol
        m, _ = R.guided(u, c, C.G)
        assert abs(R.factor(m, c, 0.7) / TR._host_factor(m, c, 0.7) - 1.0) < tol
        # host_windows_step, _host_blends (line) on VIEW_SHAPES; host_ring_step / host_ring_blends on RING_SHAPES
        cf = coefs[(8, 0.8)]
        for kind in ("uniform", "pyramid"):
            for shape, L, starts in VIEW_SHAPES:
                preds, x, z = windows_case(shape, L, starts, dt)
                w = context_weights(L, kind)
                for mode in C.DDIM_MODES:
                    assert rel(R.cfg_ddim_step_windows(preds, x, z, starts, w, mode, cf)[0], host_windows_step(preds, x, z, starts, w, mode, cf)) < tol
                m, _, cb = R.blends(preds, x, starts, w, C.G)
                hm, hc = TR._host_blends(preds, x, starts, w, C.G)
                assert rel(m, hm) < tol and rel(cb, hc) < tol
            for shape, L, starts in TL.RING_SHAPES:
                preds, x, z = windows_case(shape, L, starts, dt, seed=52)
                w = context_weights(L, kind)
                m, _, cb = R.blends(preds, x, starts, w, C.G, ring=True)
                hm, hc = TL.host_ring_blends(preds, x, starts, w, C.G)
                assert rel(m, hm) < tol and rel(cb, hc) < tol
                for mode in (0, 1 | 4, 2 | 8, 0 | 12):
                    for phi in C.RESCALES:
                        assert rel(R.cfg_ddim_step_windows(preds, x, z, starts, w, mode, cf, phi, ring=True)[0],
                                   TL.host_ring_step(preds, x, z, starts, w, mode, cf, rescale=phi)) < tol
        # _host_multistep / _blend64 / _factor64 on the inputs of test_multistep_step_kernel_all_modes (seed 52)
        gen = torch.Generator().manual_seed(52)
        u, c, x = (torch.randn(C.SHAPE, generator=gen).to(dt) for _ in range(3))
        u, c = u * 0.25, c * 0.25
        h = TM._hist(C.SHAPE)
        m, _ = R.guided(u, c, C.G)
        for cf in TM._coefs():
            for mode in C.MULTISTEP_MODES:
                for phi in C.RESCALES:
                    ref, _, x0, _ = R.cfg_multistep_step(u, c, x, h, mode, cf, phi)
                    want, want0 = TM._host_multistep(m * TM._factor64(m, c, phi), x, h, mode, cf)
                    assert rel(ref, want) < tol and rel(x0, want0) < tol
        shape, L, starts = VIEW_SHAPES[1]
        preds, x, _ = windows_case(shape, L, starts, dt, seed=60)
        w = context_weights(L, "pyramid")
        for ring, st in ((False, starts), (True, C.ring_starts(starts, shape[-3]))):
            m, _, cb = R.blends(preds, x, st, w, C.G, ring)
            hm, hc = TM._blend64(preds, x, st, w, ring)
            assert rel(m, hm) < tol and rel(cb, hc) < tol


def test_ulp_and_bound_helpers():
    for dt, p in ((torch.bfloat16, 8), (torch.float16, 11)):
        v = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, -3.0, 0.0, 1e-30], dtype=torch.float64)
        got = R.ulp(v, dt)
        floor = 2.0 ** (R.MIN_EXP[dt] - p + 1)
        want = [2.0 ** (1 - p), 2.0 ** (1 - p), 2.0 ** (1 - p), 2.0 ** (2 - p), 2.0 ** (-p), 2.0 ** (2 - p), floor, max(floor, 2.0 ** (-100 - p + 1))]
        assert got.tolist() == want, (dt, got.tolist(), want)
        # the spacing is the type's own: the neighbour of a representable value is one ulp away
        x = torch.tensor([0.3, 1.0, 5.5, 100.0]).to(dt)
        nxt = (x.view(torch.int16) + 1).view(dt)
        assert torch.equal((nxt.double() - x.double()), R.ulp(x.double(), dt))
    assert float(R.ulp(torch.tensor([6e-8], dtype=torch.float64), torch.float16)) == 2.0 ** -24        # fp16 subnormals
    ref = torch.tensor([1.0, 2.0, -0.5], dtype=torch.float64)
    T = ref.abs()
    ok = ref.to(torch.bfloat16)
    assert R.within_rounding(ok, ref, T, torch.bfloat16) == 0.0
    off = ok.clone()
    off[1] = 2.0 + 2.0 ** -6                                     # one bf16 ulp at 2
    with pytest.raises(R.Outside, match=r"worst \|err\| / bound 1\.99.* at \(1,\), 33\.3 % of 3 elements"):
        R.within_rounding(off, ref, T, torch.bfloat16, what="x")
    with pytest.raises(R.Outside):
        R.within_rounding(torch.tensor([1.0, float("nan"), -0.5]).to(torch.bfloat16), ref, T, torch.bfloat16)
    with pytest.raises(AssertionError, match="not sharp"):
        R.within_rounding(ok, ref, T * 1e4, torch.bfloat16)
    h = torch.tensor([1.0, 2.0, -0.5])
    assert R.history_within(h, ref, T) == 0.0
    with pytest.raises(R.Outside, match="history"):
        R.history_within(h * (1 + 2.0 ** -19), ref, T)
    with pytest.raises(R.Outside):
        R.history_within(torch.tensor([1.0, float("nan"), -0.5]), ref, T)


# ------------------------------------------------------------------------------------------------ 2. the stand-ins meet the bound
@pytest.fixture(scope="module")
def refs():
    """{case name: (ref, T, x0, X0)}: each reference is computed once."""
    store = {}

    def get(case):
        if case.name not in store:
            store[case.name] = C.reference(case)
        return store[case.name]
    return get


def _stand_ins_pass(cases, refs, tag):
    worst, n = {}, 0
    for case in cases:
        ref4 = refs(case)
        for coef_dev in (False, True):
            out, hist = C.call(STAND_INS, case, coef_dev=coef_dev)
            C.check(case, out, hist, ref4, FACTOR_TOL, worst)
            if hist is not None and case.coefs[5] == 0.0:
                assert torch.isfinite(out.float()).all() and torch.isfinite(hist).all(), case.name       # the NaN history is not read
        if case.entry in ("ddim", "ddim_windows") and case.rescale == 0.0 and not case.ring:
            assert torch.equal(C.call(OLDEST, case)[0], C.call(STAND_INS, case)[0]), case.name
        n += 1
    print(f"stand-ins {tag}: {n} cases, worst |err| / bound {worst}")
    assert n > 0 and worst["out"] <= 1.0


@pytest.mark.parametrize("dt", C.DTYPES, ids=C.dtname)
def test_plain_stand_ins_within_rounding(dt, refs):
    _stand_ins_pass(C.update_cases(dt), refs, f"update {dt}")
    _stand_ins_pass(C.ddim_cases(dt), refs, f"ddim {dt}")
    _stand_ins_pass(C.multistep_cases(dt), refs, f"multistep {dt}")


@pytest.mark.parametrize("ring", [False, True], ids=["line", "ring"])
@pytest.mark.parametrize("dt", C.DTYPES, ids=C.dtname)
def test_windows_stand_ins_within_rounding(dt, ring, refs):
    _stand_ins_pass(C.ddim_windows_cases(dt, ring), refs, f"ddim windows ring={ring} {dt}")
    _stand_ins_pass(C.multistep_windows_cases(dt, ring), refs, f"multistep windows ring={ring} {dt}")


def test_grid_stride_tail_stand_in_within_rounding(refs):
    _stand_ins_pass([C.tail_case()], refs, "grid-stride tail")


# ------------------------------------------------------------------------------------------------ 3. mutants
def _blend32(k, g, mut):
    """Copy of _emu_rescale_step.blends (line) / _emu_ring_step.ring_blends (ring) with the mutants of the blend."""
    preds, sample, starts = k.preds, k.x, k.starts
    fd = sample.dim() - 3
    F = sample.shape[fd]
    nW, L = preds.shape[0], preds.shape[fd + 1]
    weights = torch.roll(k.weights, 1) if mut == "weight index shifted by one" else k.weights
    shape = [1] * sample.dim()
    shape[fd] = L
    w = weights.float().reshape(shape)
    wadd = torch.ones_like(weights) if mut == "blend divided by the window count" else weights.float()
    acc_m = torch.zeros(sample.shape, dtype=torch.float32)
    acc_c = torch.zeros(sample.shape, dtype=torch.float32)
    if k.ring:
        wsum = torch.zeros(F, dtype=torch.float32)
    else:
        wsum = torch.zeros([F if i == fd else 1 for i in range(sample.dim())], dtype=torch.float32)
    for i in range(nW):
        s = int(starts[i])
        u, c = preds[i, 0:1].float(), preds[i, 1:2].float()
        stat = u if mut == "rescale from std(u)" else c
        if k.ring:
            idx = s + torch.arange(L)
            idx = idx.clamp(max=F - 1) if mut == "ring wrap replaced by a clamp" else idx % F
            acc_m.index_add_(fd, idx, w * (u + g * (c - u)))
            acc_c.index_add_(fd, idx, w * stat)
            wsum.index_add_(0, idx, wadd)
        else:
            acc_m.narrow(fd, s, L).add_(w * (u + g * (c - u)))
            acc_c.narrow(fd, s, L).add_(w * stat)
            wsum.narrow(fd, s, L).add_(wadd.reshape(shape))
    if k.ring:
        shape[fd] = F
        wsum = wsum.reshape(shape)
    return acc_m / wsum, acc_c / wsum


def eval32(k, mut=None):
    """A copy of the stand-ins' fp32 evaluation (scalar coefficients) with one perturbation ``mut`` -> (out, history or None); None:
    the stand-ins themselves, bit for bit (test_the_copy_is_the_stand_ins)."""
    if k.entry == "update":
        g, cx, cv = k.coefs
        return (cx * k.x.float() + cv * (k.u.float() + g * (k.c.float() - k.u.float()))).to(k.dt), None
    g = k.coefs[0] * (1.005 if mut == "guidance x 1.005" else 1.0)
    phi = k.rescale * (1.02 if mut == "phi x 1.02" else 1.0)
    if k.entry.endswith("windows"):
        m, stat = _blend32(k, g, mut)
    else:
        u, c = k.u.float(), k.c.float()
        m, stat = u + g * (c - u), (u if mut == "rescale from std(u)" else c)
    if k.rescale != 0.0:
        m = m * (phi * stat.std() / m.std() + (1.0 - phi))
    x = k.x.float()
    _, sa, sb = k.coefs[:3]
    pred = k.mode & 3
    x0 = (x - sb * m) / sa if pred == 0 else sa * x - sb * m if pred == 1 else m
    raw = x0
    if k.mode & 4 and mut != "clamp dropped":
        x0 = x0.clamp(-1.0, 1.0)
    if k.entry.startswith("multistep"):
        cx, c0, c1 = k.coefs[3:]
        hist = k.hist.clone()
        out = cx * x + c0 * x0
        if c1 != 0.0:
            out = out + c1 * (x0 if mut == "c1 term reading the new x0" else hist.reshape(x.shape))
        if not (mut == "history not written when c1 == 0" and c1 == 0.0):
            hist.copy_(x0.reshape(hist.shape))
        return out.to(k.dt), hist
    sap, direction, sigma = k.coefs[3:]
    sap = sap * (1.003 if mut == "sa_prev x 1.003" else 1.0)
    direction = direction * (0.99 if mut == "direction x 0.99" else 1.0)
    sigma = sigma * (1.05 if mut == "sigma x 1.05" else 1.0)
    eps = sa * m + sb * x if pred == 1 else m
    if k.mode & 8:
        eps = (x - sa * (raw if mut == "e re-derived from the unclamped x0" else x0)) / sb
    out = sap * x0 + direction * eps
    if k.z is not None:
        out = out + sigma * k.z.float()
    return out.to(k.dt), None


def _pool(name):
    both = lambda f, *a: [k for dt in C.DTYPES for k in f(dt, *a)]
    if name == "ddim":
        return [k for k in both(C.ddim_cases) if k.rescale == 0.0]
    if name == "rescale":
        return [k for k in both(C.ddim_cases) if k.rescale != 0.0] + [k for k in both(C.ddim_windows_cases, False) if k.rescale != 0.0 and "_t8_" in k.name]
    if name == "line":
        return [k for k in both(C.ddim_windows_cases, False) if k.rescale == 0.0 and "_t8_" in k.name]
    if name == "ring":
        return [k for k in both(C.ddim_windows_cases, True) if k.rescale == 0.0 and "_t8_" in k.name]
    assert name == "multistep"
    return [k for k in both(C.multistep_cases) if k.rescale == 0.0]


MUTANTS = [("guidance x 1.005", "ddim"), ("sa_prev x 1.003", "ddim"), ("direction x 0.99", "ddim"), ("sigma x 1.05", "ddim"),
           ("clamp dropped", "ddim"), ("e re-derived from the unclamped x0", "ddim"), ("weight index shifted by one", "line"),
           ("blend divided by the window count", "line"), ("ring wrap replaced by a clamp", "ring"),
           ("c1 term reading the new x0", "multistep"), ("history not written when c1 == 0", "multistep"),
           ("rescale from std(u)", "rescale"), ("phi x 1.02", "rescale")]


def test_the_copy_is_the_stand_ins(refs):
    seen = set()
    for pool in ("ddim", "rescale", "line", "ring", "multistep"):
        for k in _pool(pool):
            out, hist = eval32(k)
            want, want_h = C.call(STAND_INS, k)
            assert torch.equal(out, want) and (hist is None or torch.equal(hist, want_h)), k.name
            seen.add(k.entry)
    k = next(C.update_cases(torch.bfloat16))
    assert torch.equal(eval32(k)[0], C.call(STAND_INS, k)[0])
    assert seen == {"ddim", "ddim_windows", "multistep"}


def _passes(k, out, hist, ref4):
    try:
        C.check(k, out, hist, ref4, FACTOR_TOL)
        return True
    except R.Outside:
        return False


def _old_check_passes(k, out, hist, ref4):
    """The whole-tensor check of the older tests: rel < TOL on the result, rel < 1e-5 (HIST_TOL) on the history."""
    ref, _, x0, _ = ref4
    return bool(rel(out, ref) < TOL[k.dt]) and (x0 is None or bool(rel(hist, x0) < 1e-5))


@pytest.mark.parametrize("mut,pool", MUTANTS, ids=[m.replace(" ", "_") for m, _ in MUTANTS])
def test_mutants_are_rejected(mut, pool, refs):
    """Every mutant changes some case, and every case it changes by more than rounding is outside the bound; the record says how many
    of those the older whole-tensor check accepts."""
    changed = rejected = old_accepts = 0
    worst_rel = 0.0
    for k in _pool(pool):
        out, hist = eval32(k, mut)
        base, base_h = eval32(k)
        if torch.equal(out.view(torch.int16), base.view(torch.int16)) and (hist is None or torch.equal(hist.view(torch.int32), base_h.view(torch.int32))):
            continue                                        # the mutation is not on this case's path (no clamp bit, eta = 0, uniform weights ...)
        changed += 1
        ref4 = refs(k)
        if not _passes(k, out, hist, ref4):
            rejected += 1
            if _old_check_passes(k, out, hist, ref4):
                old_accepts += 1
                worst_rel = max(worst_rel, rel(out, ref4[0]))
    print(f"MUTANT {mut!r}: changes {changed} cases of pool {pool!r}; the bound rejects {rejected}; "
          f"rel < TOL accepts {old_accepts} of the rejected ones (largest accepted rel {worst_rel:.3g})")
    assert changed > 0 and rejected >= 1
    assert rejected == changed, f"{mut}: {changed - rejected} changed cases pass the bound"
