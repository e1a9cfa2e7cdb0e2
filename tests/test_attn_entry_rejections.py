"""The argument checks of the attention entry points (csrc/attn_fwd.hip: ``im360_attn_fwd``, ``im360_attn_fwd2``; csrc/temporal_attn.hip:
``im360_temporal_attn_fwd``) refuse what they refused before their host code was rewritten: tests/golden/attn_entry_rejections.json holds
calls recorded through ``kernels.lib()`` on the commit before the rewrite, each breaking exactly one rule of one entry point (a null
pointer, an empty problem, ``kv_group`` 0, an unsupported head dim, ``B*H`` too large, one misaligned stride or base per operand, each
bias / packed-bias / ``bias_sel`` / block-map rule, the packed flag without a bias, F > 64, a head dim that is no multiple of 8, K|V over
the LDS budget, an unsupported dtype, ...), with the return code and the ``im360_last_error()`` text each call gave.  The test replays
them and compares both.

Every ``IM360_CHECK_ARG`` of the three entry points is broken by at least one call.  Three refusals of the launchers behind them are
recorded too: a packed bias at head dim 64, and the grid limit of ``attn_fwd_kernel`` and of the resident two-set kernel.  Two refusals
cannot be reached by a call: "attn_fwd2: two key/value sets need head dim 64" (``im360_attn_fwd2`` has refused every other head dim by
then) and attn_pipe.hip's "attn_pipe: ... workgroups exceed the grid limit" (with the knobs at their defaults its eight-wave workgroups
take twice the query rows of those whose grid ``launch_attn_b`` has checked in front of it).

The pointers in the fixture are made-up aligned integers: a refused call never dereferences them.  Hence two guards: every recorded
return code must be nonzero (asserted over the whole fixture before the first call), and the test does not run where a GPU is
present -- there a check that had lapsed would launch a kernel on a made-up address."""
import json
import os

import pytest
import torch

from imagine360_amd import kernels as K

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_entry_rejections.json")
ENTRY_POINTS = {"im360_attn_fwd", "im360_attn_fwd2", "im360_temporal_attn_fwd"}


@pytest.mark.skipif(torch.cuda.is_available(), reason="replays refused calls with made-up pointers: only where nothing could launch")
def test_recorded_rejections_replay():
    with open(FIXTURE) as f:
        fixture = json.load(f)
    cases = fixture["cases"]
    assert fixture["abi_version"] == K.ABI_VERSION
    assert len(cases) >= 100 and {c["entry"] for c in cases} == ENTRY_POINTS
    assert all(c["rc"] in (-1, -2) and c["error"] for c in cases), "every recorded call must be a refusal in front of the launch"
    for c in cases:
        assert len(c["args"]) == len(fixture["arguments"][c["entry"]]) == len(K._SIGNATURES[c["entry"]][1]), c
    lib = K.lib()
    wrong = []
    for c in cases:
        rc = getattr(lib, c["entry"])(*c["args"])
        got = (rc, lib.im360_last_error().decode())
        if got != (c["rc"], c["error"]):
            wrong.append((c["entry"], c["rule"], got, (c["rc"], c["error"])))
    assert not wrong, wrong
