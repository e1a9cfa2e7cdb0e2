"""The sampler-step kernels (csrc/sampler_step.hip) on the MI355X against the per-element rounding bound of _ref_step.py: every element
of cfg_ddim_update, cfg_ddim_step, cfg_ddim_step_windows (line and ring), cfg_multistep_step and cfg_multistep_step_windows (line and
ring), each with and without the guidance rescale, with scalar and with device coefficients, within half an ulp of the 16-bit type plus
32 fp32 roundings of the fp64 restatement; the fp32 history within 16 roundings.  The cases are those of test_step_rounding.py, which
holds the torch stand-ins to the same bound and shows that coefficient errors of a few parts in a thousand do not meet it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _ref_step as R  # noqa: E402
import _step_cases as C  # noqa: E402
from helpers import record as _record  # noqa: E402
from imagine360_amd import kernels as K  # noqa: E402
from test_guidance_rescale_gpu import FACTOR_TOL  # noqa: E402

torch.set_grad_enabled(False)


def _entry_point(case):
    name = {"update": "cfg_ddim_update", "ddim": "cfg_ddim_step", "ddim_windows": "cfg_ddim_step_windows", "multistep": "cfg_multistep_step",
            "multistep_windows": "cfg_multistep_step_windows"}[case.entry]
    return name + ("_ring" if case.ring else "") + ("_rescale" if case.rescale != 0.0 else "")


def _kernels_within_rounding(cases, tag):
    """Every case through the real entry point, with scalar and with device coefficients.  All cases are run before the verdict, so
    that one run names every case outside the bound; the worst ratios per entry point are recorded either way."""
    worst, failures, cache, n = {}, [], {}, 0
    for case in cases:
        ref4 = C.reference(case)
        w = worst.setdefault(_entry_point(case), {"out": 0.0, "cases": 0})
        w["cases"] += 1
        for coef_dev in (False, True):
            out, hist = C.call(K, case, device="cuda", coef_dev=coef_dev, cache=cache)
            assert out.dtype == case.dt and out.shape == case.x.shape
            try:
                C.check(case, out, hist, ref4, FACTOR_TOL, w)
            except R.Outside as e:
                key = "hist" if "history" in str(e) else "out"
                w[key] = max(w.get(key, 0.0), e.worst)
                failures.append(f"{'coef_dev ' if coef_dev else ''}{e}")
            if hist is not None and case.coefs[5] == 0.0:           # first order: the NaN history is not read
                assert torch.isfinite(out.float()).all() and torch.isfinite(hist).all(), case.name
        n += 1
    for name, w in worst.items():
        vals = {"worst_err_over_bound": w["out"]}
        if "hist" in w:
            vals["worst_hist_err_over_bound"] = w["hist"]
        _record(f"step_rounding_{name}_{tag}", cases=w["cases"], **vals)
    assert n > 0 and not failures, f"{len(failures)} results outside the bound, the first ones:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("dt", C.DTYPES, ids=C.dtname)
def test_cfg_ddim_update_within_rounding(dt):
    _kernels_within_rounding(C.update_cases(dt), C.dtname(dt))


@pytest.mark.parametrize("dt", C.DTYPES, ids=C.dtname)
def test_cfg_ddim_step_within_rounding(dt):
    """3 timesteps x eta 0 / 0.8 x 12 modes x rescale 0 / 0.7 on 420 lanes of 8."""
    _kernels_within_rounding(C.ddim_cases(dt), C.dtname(dt))


def test_cfg_ddim_step_grid_stride_tail_within_rounding():
    """(4096 * 256 + 300) lanes: the capped grid strides, the last pass is partial."""
    case = C.tail_case()
    assert case.x.numel() // 8 > 4096 * 256 and (case.x.numel() // 8) % 256 != 0
    _kernels_within_rounding([case], "bfloat16_grid_stride_tail")


@pytest.mark.parametrize("ring", [False, True], ids=["line", "ring"])
@pytest.mark.parametrize("dt", C.DTYPES, ids=C.dtname)
def test_cfg_ddim_step_windows_within_rounding(dt, ring):
    """Panorama (16-byte lanes) and perspective (scalar path) latents, frames covered by 1, 2 and 3 windows, uniform and pyramid
    weights; on the ring the tables are rolled so that windows cross the end of the clip."""
    _kernels_within_rounding(C.ddim_windows_cases(dt, ring), C.dtname(dt))


@pytest.mark.parametrize("dt", C.DTYPES, ids=C.dtname)
def test_cfg_multistep_step_within_rounding(dt):
    """6 modes x first order (c1 == 0, the history holds NaN) and second order (steps 1, 8, 23 of 25 and the largest |c0|, |c1| of the
    8-step grid) x rescale 0 / 0.7; the history against x0."""
    _kernels_within_rounding(C.multistep_cases(dt), C.dtname(dt))


@pytest.mark.parametrize("ring", [False, True], ids=["line", "ring"])
@pytest.mark.parametrize("dt", C.DTYPES, ids=C.dtname)
def test_cfg_multistep_step_windows_within_rounding(dt, ring):
    _kernels_within_rounding(C.multistep_windows_cases(dt, ring), C.dtname(dt))
