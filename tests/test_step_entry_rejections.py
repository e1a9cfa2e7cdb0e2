"""The argument checks of the sampler-step and latent-plane entry points (csrc/sampler_step.hip, csrc/noise_latents.hip,
csrc/keep_latents.hip) refuse what they refused before their host code was rewritten: tests/golden/step_entry_rejections.json
holds calls recorded through ``kernels.lib()`` on the commit before the rewrite, each breaking exactly one rule of one entry point
(a null pointer, ``n % 8``, mode 3 or 16, sigma > 0 without noise, L > F, a misaligned table, a short workspace, a non-finite
rescale, x0 == pano, a size that reaches 2^31, an unsupported dtype, ...), with the return code and the ``im360_last_error()``
text each call gave.  The test replays them and compares both.

The pointers in the fixture are made-up aligned integers: a refused call never dereferences them.  Hence two guards: every recorded
return code must be nonzero (asserted over the whole fixture before the first call), and the test does not run where a GPU is
present -- there a check that had lapsed would launch a kernel on a made-up address."""
import json
import os

import pytest
import torch

from imagine360_amd import kernels as K

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_entry_rejections.json")
ENTRY_POINTS = {"im360_cfg_ddim_step", "im360_cfg_ddim_step_rescale", "im360_cfg_ddim_step_windows", "im360_cfg_ddim_step_windows_rescale",
                "im360_cfg_ddim_step_windows_ring", "im360_cfg_ddim_step_windows_ring_rescale", "im360_cfg_rescale_stats",
                "im360_cfg_rescale_stats_windows", "im360_cfg_rescale_stats_windows_ring", "im360_cfg_rescale_factor",
                "im360_cfg_ddim_update", "im360_noise_latents", "im360_keep_latents"}


def _arg(v):
    return float(v) if isinstance(v, str) else v          # "inf" / "-inf" / "nan": not JSON numbers


@pytest.mark.skipif(torch.cuda.is_available(), reason="replays refused calls with made-up pointers: only where nothing could launch")
def test_recorded_rejections_replay():
    with open(FIXTURE) as f:
        fixture = json.load(f)
    cases = fixture["cases"]
    assert fixture["abi_version"] == K.ABI_VERSION
    assert len(cases) >= 36 and {c["entry"] for c in cases} == ENTRY_POINTS
    assert all(c["rc"] in (-1, -2) and c["error"] for c in cases), "every recorded call must be a refusal in front of the launch"
    for c in cases:
        assert len(c["args"]) == len(fixture["arguments"][c["entry"]]) == len(K._SIGNATURES[c["entry"]][1]), c
    lib = K.lib()
    wrong = []
    for c in cases:
        rc = getattr(lib, c["entry"])(*(_arg(v) for v in c["args"]))
        got = (rc, lib.im360_last_error().decode())
        if got != (c["rc"], c["error"]):
            wrong.append((c["entry"], c["rule"], got, (c["rc"], c["error"])))
    assert not wrong, wrong
