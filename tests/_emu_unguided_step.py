"""Torch stand-ins of the unguided step entry points (csrc/sampler_step.hip, the GUIDED = false instantiations) for the CPU tier:
``kernels.ddim_update``, ``ddim_step``, ``ddim_step_windows`` (``ring=``), ``multistep_step`` and ``multistep_step_windows`` (``ring=``).
Each is its guided sibling's stand-in on the one prediction in both places -- u + g (c - u) with u == c is c in fp32 for any finite g --
so the formulas, the blend (the line's of _emu_rescale_step.py, the ring's of _emu_ring_step.py), the x0 history and the one rounding
at the end are stated once.  Used on top of _emu_kernels.patched_kernels() and the siblings' patches."""
import contextlib

import _emu_kernels as E
import _emu_multistep_step as EM
import _emu_rescale_step as ER
import _emu_ring_step as EG

NAMES = ("ddim_update", "ddim_step", "ddim_step_windows", "multistep_step", "multistep_step_windows")


def _two(preds):
    """[nW, 1, ...] -> [nW, 2, ...] with both halves the text half (a view)."""
    assert preds.shape[1] == 1, tuple(preds.shape)
    return preds.expand(-1, 2, *preds.shape[2:])


def ddim_update(pred, sample, cx, cv, coef_dev=None):
    return E.cfg_ddim_update(pred, pred, sample, 1.0, cx, cv, coef_dev=coef_dev)


def ddim_step(pred, sample, noise, mode, coefs, coef_dev=None):
    return ER.cfg_ddim_step(pred, pred, sample, noise, mode, coefs, coef_dev=coef_dev)


def ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=None, ring=False):
    return EG.cfg_ddim_step_windows(_two(preds), sample, noise, starts, weights, mode, coefs, coef_dev=coef_dev, ring=ring)


def multistep_step(pred, sample, hist, mode, coefs, coef_dev=None):
    return EM.cfg_multistep_step(pred, pred, sample, hist, mode, coefs, coef_dev=coef_dev)


def multistep_step_windows(preds, sample, hist, starts, weights, mode, coefs, coef_dev=None, ring=False):
    return EM.cfg_multistep_step_windows(_two(preds), sample, hist, starts, weights, mode, coefs, coef_dev=coef_dev, ring=ring)


@contextlib.contextmanager
def patched_unguided_kernels():
    """``calls``: the name of every unguided stand-in called, in order."""
    from imagine360_amd import kernels
    saved = {n: getattr(kernels, n) for n in NAMES}
    calls = []

    def counted(name):
        fn = globals()[name]

        def wrapper(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapper
    for n in NAMES:
        setattr(kernels, n, counted(n))
    try:
        yield calls
    finally:
        for n, fn in saved.items():
            setattr(kernels, n, fn)
