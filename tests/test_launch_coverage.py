"""Every gfx950 kernel inside the shipped libim360_kernels.so is launched by a kernel-level parity test (CPU check, no GPU).

tests/golden/kernel_launch_coverage.json is the ledger tools/kernel_launch_coverage.py writes from rocprofv3 kernel traces of the parity
tests (tests/test_kernels_gpu.py, tests/test_kernel_variants_gpu.py, the step-kernel and preprocessing kernel tests): launches per
kernel and traced file.  A kernel the host launchers can select but no reference-checked test launches can be arbitrarily wrong with a
green suite; this file makes "launched under a reference check" a property of the library that is tested."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_launch_coverage as cov  # noqa: E402

# Kernels a single-process kernel-level test must not or cannot launch on a shared machine: {mangled name: reason citing the launcher}.
# At most 5.  A kernel that no entry point of the default build can launch does not belong here: its instantiation moves under
# IM360_ABLATE instead.
WAIVED = {}

REGENERATE = ("add a parity test that launches them, then regenerate the ledger on the MI355X: "
              "python tools/kernel_launch_coverage.py --emit-script build/cov > job.sh; bash job.sh; "
              "python tools/kernel_launch_coverage.py --collect build/cov")


@pytest.fixture(scope="module")
def library():
    have = cov.library_kernels()
    if have is None:
        pytest.skip("ROCm LLVM binutils not installed")
    assert len(have) >= 100, len(have)
    return have


@pytest.fixture(scope="module")
def ledger():
    with open(cov.LEDGER) as fh:
        led = json.load(fh)
    assert led["commit"] and led["runs"] and all(r["command"].startswith("rocprofv3 --kernel-trace") and "--pmc" not in r["command"] for r in led["runs"])
    return led


def launched(ledger):
    return {k for k, per_file in ledger["kernels"].items() if sum(per_file.values()) > 0}


def test_every_library_kernel_is_launched_by_a_parity_test(library, ledger):
    missing = [k for k in library if k not in launched(ledger) and k not in WAIVED]
    assert not missing, f"{len(missing)} kernels of the library are launched by no kernel-level parity test: {missing}; {REGENERATE}"


def test_ledger_and_waivers_name_kernels_of_the_library(library, ledger):
    """A stale ledger (taken before a kernel's template arguments changed) or a stale waiver fails."""
    have = set(library)
    stale = sorted(k for k in ledger["kernels"] if k not in have)
    assert not stale, f"the ledger names kernels the library does not contain: {stale}; {REGENERATE}"
    gone = sorted(k for k in WAIVED if k not in have)
    assert not gone, f"WAIVED names kernels the library does not contain: {gone}"
    both = sorted(k for k in WAIVED if k in launched(ledger))
    assert not both, f"WAIVED kernels that the ledger shows launched (drop the waiver): {both}"


def test_both_dtypes_of_every_templated_kernel_are_launched(library, ledger):
    have, hit = set(library), launched(ledger)
    pairs = [(k, cov.dtype_partner(k)) for k in library if "DF16b" in k]
    assert len(pairs) >= 50 and all(p in have for _, p in pairs), [k for k, p in pairs if p not in have]
    half = sorted(k for a, b in pairs for k in (a, b) if k not in hit and k not in WAIVED and (a in hit or b in hit))
    assert not half, f"kernels whose other 16-bit instantiation is launched but which are not: {half}; {REGENERATE}"


def test_waivers_are_few_and_reasoned():
    assert len(WAIVED) <= 5, len(WAIVED)
    for name, reason in WAIVED.items():
        assert name.startswith(cov.PREFIX) and isinstance(reason, str) and "\n" not in reason.strip() and ".hip:" in reason, (name, reason)
