"""The cases of the per-element rounding tests of the sampler-step family (test_step_rounding.py on the stand-ins, test_step_rounding_gpu.py
on the kernels): seeded 16-bit inputs at the smallest shapes the suite runs, the coefficient vectors of the shipped schedulers, and one
dispatcher that calls a module with the signatures of ``imagine360_amd.kernels`` (the kernels themselves or a stand-in namespace) or
the fp64 restatement of _ref_step.py on a case."""
import types

import torch

import _ref_step as R
from imagine360_amd import configs
from imagine360_amd.context import context_weights
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
from test_context_windows import VIEW_SHAPES, windows_case

G = 7.5
SHAPE = (1, 4, 5, 7, 24)                  # 3360 elements: 420 lanes of 8, not a multiple of a 256-thread block
TAIL_LANES = 4096 * 256 + 300             # more lanes than the capped grid covers in one pass
STEPS = (1, 8, 23)                        # timestep indices of a 25-step schedule: early, middle, late
DDIM_MODES = [pred | extra for pred in (0, 1, 2) for extra in (0, 4, 8, 12)]
MULTISTEP_MODES = [0, 1, 2, 4, 5, 6]
RESCALES = (0.0, 0.7)
DTYPES = [torch.bfloat16, torch.float16]


def dtname(dt):
    return str(dt).split(".")[-1]


def ddim_coefficients():
    """{(step index, eta): coefficient vector} at guidance 7.5."""
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    return {(i, eta): sch.step_coefficients(sch._timesteps_host[i], eta, G) for i in STEPS for eta in (0.0, 0.8)}


def update_coefficients():
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    return {i: sch.coefficients(sch._timesteps_host[i]) for i in STEPS}


def multistep_coefficients():
    """{name: vector}: first order (c1 == 0) at the first step of the 25- and of the 8-step grid; second order at steps 1, 8, 23 of 25 and
    at step 6 of 8, the largest |c0|, |c1| of the shipped grids (2.66, -1.75)."""
    s25, s8 = (DPMSolverMultistepScheduler(**configs.NOISE_SCHEDULER_KWARGS) for _ in range(2))
    s25.set_timesteps(25)
    s8.set_timesteps(8)
    out = {"first25": s25.multistep_coefficients(s25._timesteps_host, 0, G), "first8": s8.multistep_coefficients(s8._timesteps_host, 0, G)}
    out.update({f"second25_{i}": s25.multistep_coefficients(s25._timesteps_host, i, G) for i in STEPS})
    out["second8_6"] = s8.multistep_coefficients(s8._timesteps_host, 6, G)
    assert all((v[5] == 0.0) == k.startswith("first") for k, v in out.items())
    assert abs(out["second8_6"][4] - 2.66285) < 1e-3 and abs(out["second8_6"][5] + 1.75110) < 1e-3
    return out


class Case(types.SimpleNamespace):
    """entry: update | ddim | ddim_windows | multistep | multistep_windows; the tensors on the host; mode, coefs, rescale, ring."""
    rescale, ring, mode, z, hist = 0.0, False, 0, None, None


def _plain_inputs(dt, seed, n=None):
    gen = torch.Generator().manual_seed(seed)
    shape = SHAPE if n is None else (n,)
    u, c, x, z = (torch.randn(shape, generator=gen).to(dt) for _ in range(4))
    return u * 0.25, c * 0.25, x, z          # predictions scaled: the guided x0 straddles +-1


def _hist(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 0.7


def update_cases(dt):
    u, c, x, _ = _plain_inputs(dt, 50)
    for i, (cx, cv) in update_coefficients().items():
        yield Case(entry="update", name=f"update_{dtname(dt)}_t{i}", dt=dt, u=u, c=c, x=x, coefs=(G, cx, cv))


def ddim_cases(dt):
    u, c, x, z = _plain_inputs(dt, 51)
    for (i, eta), coefs in ddim_coefficients().items():
        for mode in DDIM_MODES:
            for phi in RESCALES:
                yield Case(entry="ddim", name=f"ddim_{dtname(dt)}_t{i}_eta{eta}_mode{mode}_phi{phi}", dt=dt, u=u, c=c, x=x,
                           z=z if eta > 0 else None, mode=mode, coefs=coefs, rescale=phi)


def tail_case():
    """The grid-stride tail, bf16: (4096 * 256 + 300) lanes of 8, v-prediction with the clamp, eta = 0.8."""
    u, c, x, z = _plain_inputs(torch.bfloat16, 53, TAIL_LANES * 8)
    return Case(entry="ddim", name="ddim_bfloat16_grid_stride_tail", dt=torch.bfloat16, u=u, c=c, x=x, z=z, mode=1 | 4,
                coefs=ddim_coefficients()[(8, 0.8)])


def ring_starts(starts, F):
    """The line's table rolled back by three frames: windows cross the end of the clip, frames stay covered by 1, 2 and 3 windows."""
    return [(s + F - 3) % F for s in starts]


def _window_sets(dt, ring, seed):
    for si, (shape, L, starts) in enumerate(VIEW_SHAPES):
        F = shape[len(shape) - 3]
        st = ring_starts(starts, F) if ring else starts
        assert not ring or any(s + L > F for s in st)
        preds, x, z = windows_case(shape, L, starts, dt, seed=seed + si)
        for kind in ("uniform", "pyramid"):
            yield f"view{si}_{kind}", preds, x, z, torch.tensor(st, dtype=torch.int32), context_weights(L, kind), _hist(shape, seed + 10 + si)


def ddim_windows_cases(dt, ring):
    for tag, preds, x, z, st, w, _ in _window_sets(dt, ring, 60):
        for (i, eta), coefs in ddim_coefficients().items():
            for mode in DDIM_MODES:
                for phi in RESCALES:
                    yield Case(entry="ddim_windows", name=f"ddim_{'ring' if ring else 'line'}_{dtname(dt)}_{tag}_t{i}_eta{eta}_mode{mode}_phi{phi}",
                               dt=dt, preds=preds, x=x, z=z if eta > 0 else None, starts=st, weights=w, mode=mode, coefs=coefs, rescale=phi,
                               ring=ring)


def _nan_like(h):
    return torch.full(h.shape, float("nan"))


def multistep_cases(dt):
    u, c, x, _ = _plain_inputs(dt, 52)
    h = _hist(SHAPE, 5)
    for cname, coefs in multistep_coefficients().items():
        for mode in MULTISTEP_MODES:
            for phi in RESCALES:
                yield Case(entry="multistep", name=f"multistep_{dtname(dt)}_{cname}_mode{mode}_phi{phi}", dt=dt, u=u, c=c, x=x,
                           hist=_nan_like(h) if coefs[5] == 0.0 else h, mode=mode, coefs=coefs, rescale=phi)


def multistep_windows_cases(dt, ring):
    for tag, preds, x, _, st, w, h in _window_sets(dt, ring, 80):
        for cname, coefs in multistep_coefficients().items():
            for mode in MULTISTEP_MODES:
                for phi in RESCALES:
                    yield Case(entry="multistep_windows", name=f"multistep_{'ring' if ring else 'line'}_{dtname(dt)}_{tag}_{cname}_mode{mode}_phi{phi}",
                               dt=dt, preds=preds, x=x, starts=st, weights=w, hist=_nan_like(h) if coefs[5] == 0.0 else h, mode=mode,
                               coefs=coefs, rescale=phi, ring=ring)


# ------------------------------------------------------------------------------------------------ dispatch
def reference(case):
    """(ref, T, x0, X0) in fp64; x0 = X0 = None for the entry points without a history."""
    k = case
    if k.entry == "update":
        return R.cfg_ddim_update(k.u, k.c, k.x, *k.coefs) + (None, None)
    if k.entry == "ddim":
        return R.cfg_ddim_step(k.u, k.c, k.x, k.z, k.mode, k.coefs, k.rescale) + (None, None)
    if k.entry == "ddim_windows":
        return R.cfg_ddim_step_windows(k.preds, k.x, k.z, k.starts, k.weights, k.mode, k.coefs, k.rescale, k.ring) + (None, None)
    if k.entry == "multistep":
        return R.cfg_multistep_step(k.u, k.c, k.x, k.hist, k.mode, k.coefs, k.rescale)
    assert k.entry == "multistep_windows"
    return R.cfg_multistep_step_windows(k.preds, k.x, k.hist, k.starts, k.weights, k.mode, k.coefs, k.rescale, k.ring)


def call(mod, case, device="cpu", coef_dev=False, cache=None):
    """Run ``case`` through ``mod`` (functions with the signatures of ``imagine360_amd.kernels``) -> (out, history or None).  The keywords
    ``rescale`` / ``ring`` are passed only when set (the oldest stand-ins do not take them); ``coef_dev``: the coefficients travel
    as a float32 tensor on ``device`` and the scalar arguments are zeros.  ``cache``: {id(host tensor): device tensor}."""
    k = case

    def dev(t):
        if t is None or device == "cpu":
            return t
        if cache is None:
            return t.to(device)
        if id(t) not in cache:
            cache[id(t)] = (t, t.to(device))           # (keeps the host tensor alive: its id stays its own)
        return cache[id(t)][1]
    kw = {}
    coefs = k.coefs
    if coef_dev:
        kw["coef_dev"] = torch.tensor(k.coefs, dtype=torch.float32, device=device)
        coefs = (0.0,) * len(k.coefs)
    if k.rescale != 0.0:
        kw["rescale"] = k.rescale
    if k.ring:
        kw["ring"] = True
    if k.entry == "update":
        return mod.cfg_ddim_update(dev(k.u), dev(k.c), dev(k.x), *coefs, **kw), None
    if k.entry == "ddim":
        return mod.cfg_ddim_step(dev(k.u), dev(k.c), dev(k.x), dev(k.z), k.mode, coefs, **kw), None
    if k.entry == "ddim_windows":
        return mod.cfg_ddim_step_windows(dev(k.preds), dev(k.x), dev(k.z), dev(k.starts), dev(k.weights), k.mode, coefs, **kw), None
    h = k.hist.to(device).clone()                       # written in place: a fresh copy per call
    if k.entry == "multistep":
        return mod.cfg_multistep_step(dev(k.u), dev(k.c), dev(k.x), h, k.mode, coefs, **kw), h
    assert k.entry == "multistep_windows"
    return mod.cfg_multistep_step_windows(dev(k.preds), dev(k.x), h, dev(k.starts), dev(k.weights), k.mode, coefs, **kw), h


def check(case, out, hist, ref4, extra_for_rescale, worst=None):
    """``within_rounding`` on the result and ``history_within`` on the history of one case; ``worst``: {key: ratio} kept at its maximum."""
    ref, T, x0, X0 = ref4
    extra = extra_for_rescale if case.rescale != 0.0 else 0.0
    r = R.within_rounding(out, ref, T, case.dt, extra=extra, what=case.name)
    rh = None if x0 is None else R.history_within(hist, x0, X0, what=case.name)
    if worst is not None:
        worst["out"] = max(worst.get("out", 0.0), r)
        if rh is not None:
            worst["hist"] = max(worst.get("hist", 0.0), rh)
    return r, rh
