"""The cases of the unguided step entry points (test_guidance_interval.py on the stand-ins of _emu_unguided_step.py,
test_guidance_interval_gpu.py on the kernels): every non-rescale case of _step_cases.py with the unconditional prediction replaced by the
text prediction (for windows: both halves of ``preds`` the text half), and one dispatcher with the signatures of ``imagine360_amd.kernels``.
``_step_cases.call`` of such a case runs the guided sibling on (c, c).  ``reference`` is the fp64 restatement of the UNGUIDED step from
the pieces of _ref_step.py with the majorant of what it computes, M = |c| (the guided restatement on (c, c) gives the same ``ref`` but
carries M = |u| + g (|c| + |u|) = 16 |c|, a bound 16 times looser in its prediction terms than the step is entitled to)."""
import copy

import torch

import _ref_step as R
import _step_cases as C

FAMILIES = ("plain", "windows_line", "windows_ring")
_HALVES = {}


def unguided(case):
    """``case`` with u := c; ``pred`` / ``preds1`` ([nW, 1, ...], contiguous) is what the unguided entry point is given."""
    assert case.rescale == 0.0
    k = copy.copy(case)
    if hasattr(case, "preds"):
        if id(case.preds) not in _HALVES:       # (one pair per window set: the cases of a set share their tensors, and so do the uploads)
            p1 = case.preds[:, 1:2].contiguous()
            _HALVES[id(case.preds)] = (case.preds, p1, p1.expand(-1, 2, *p1.shape[2:]).contiguous())
        _, k.preds1, k.preds = _HALVES[id(case.preds)]
    else:
        k.u = k.pred = case.c
    return k


def cases(dt, family):
    """update + ddim + multistep ("plain"), ddim_windows + multistep_windows on a line / on a ring; rescale == 0 only."""
    if family == "plain":
        gens = (C.update_cases(dt), C.ddim_cases(dt), C.multistep_cases(dt))
    else:
        ring = family == "windows_ring"
        gens = (C.ddim_windows_cases(dt, ring), C.multistep_windows_cases(dt, ring))
    for gen in gens:
        for case in gen:
            if case.rescale == 0.0:
                yield unguided(case)


def reference(case):
    """(ref, T, x0, X0) in fp64 of the unguided entry point of ``case`` (x0 = X0 = None without a history)."""
    k = case
    if hasattr(k, "preds1"):
        two = lambda p: p.expand(-1, 2, *p.shape[2:])
        m = R.blends(two(k.preds1), k.x, k.starts, k.weights, 1.0, k.ring)[2]               # the blend of the text halves ...
        M = R.blends(two(k.preds1.abs()), k.x, k.starts, k.weights, 1.0, k.ring)[2]         # ... and of their absolute values
    else:
        m, M = k.pred.double(), k.pred.double().abs()
    if k.entry == "update":
        _, cx, cv = k.coefs
        x = k.x.double()
        return cx * x + cv * m, abs(cx) * x.abs() + abs(cv) * M, None, None
    if k.entry in ("ddim", "ddim_windows"):
        return R.ddim_on(m, M, k.x, k.z, k.mode, k.coefs) + (None, None)
    return R.multistep_on(m, M, k.x, k.hist, k.mode, k.coefs)


def with_guidance(case, g):
    """The same case at another guidance value (element 0 of the coefficient vector)."""
    k = copy.copy(case)
    k.coefs = (float(g),) + tuple(case.coefs[1:])
    return k


def call(mod, case, device="cpu", coef_dev=False, cache=None):
    """``_step_cases.call`` for the unguided entry point of ``case``: (out, history or None).  ``coef_dev``: the SIBLING's vector on the
    device (guidance in element 0), zeros as scalars."""
    k = case

    def dev(t):
        if t is None or device == "cpu":
            return t
        if cache is None:
            return t.to(device)
        if id(t) not in cache:
            cache[id(t)] = (t, t.to(device))
        return cache[id(t)][1]
    kw = {}
    coefs = k.coefs
    if coef_dev:
        kw["coef_dev"] = torch.tensor(k.coefs, dtype=torch.float32, device=device)
        coefs = (0.0,) * len(k.coefs)
    if k.ring:
        kw["ring"] = True
    if k.entry == "update":
        return mod.ddim_update(dev(k.pred), dev(k.x), *coefs[1:], **kw), None
    if k.entry == "ddim":
        return mod.ddim_step(dev(k.pred), dev(k.x), dev(k.z), k.mode, coefs, **kw), None
    if k.entry == "ddim_windows":
        return mod.ddim_step_windows(dev(k.preds1), dev(k.x), dev(k.z), dev(k.starts), dev(k.weights), k.mode, coefs, **kw), None
    h = k.hist.to(device).clone()
    if k.entry == "multistep":
        return mod.multistep_step(dev(k.pred), dev(k.x), h, k.mode, coefs, **kw), h
    assert k.entry == "multistep_windows"
    return mod.multistep_step_windows(dev(k.preds1), dev(k.x), h, dev(k.starts), dev(k.weights), k.mode, coefs, **kw), h
