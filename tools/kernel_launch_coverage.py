#!/usr/bin/env python
"""Launch-coverage ledger of libim360_kernels.so: which compiled gfx950 kernels the kernel-level parity tests launch, and how often.

tests/test_launch_coverage.py (CPU) checks the ledger against the kernel names inside the shipped library: a kernel that no
reference-checked test launches -- a new instantiation, a re-templated one -- fails there until a test reaches it and the ledger is
regenerated here.

The traced commands are a fixed list, kernel-level parity tests only (a kernel reached only through a whole forward at a whole-model
tolerance does not count as checked; multi-process tests are not traced):

    python -m pytest -q -m gpu tests/test_kernels_gpu.py
    python -m pytest -q -m gpu tests/test_kernel_variants_gpu.py
    python -m pytest -q -m gpu tests/test_ddim_stochastic_gpu.py::test_cfg_ddim_step_kernel_all_modes
    python -m pytest -q -m gpu tests/test_context_windows_gpu.py::test_windows_kernel_all_modes_vs_fp64 tests/test_context_windows_gpu.py::test_one_uniform_window_is_cfg_ddim_step_bit_for_bit
    python -m pytest -q -m gpu tests/test_guidance_rescale_gpu.py::test_cfg_rescale_factor_vs_fp64 tests/test_guidance_rescale_gpu.py::test_rescaled_step_kernel_all_modes tests/test_guidance_rescale_gpu.py::test_rescaled_windows_kernel_all_modes_vs_fp64
    python -m pytest -q -m gpu tests/test_context_loop_gpu.py::test_ring_kernel_all_modes_vs_fp64 tests/test_context_loop_gpu.py::test_non_wrapping_tables_are_the_linear_entry_points_bit_for_bit tests/test_context_loop_gpu.py::test_rolling_the_clip_rolls_the_result_bit_for_bit tests/test_context_loop_gpu.py::test_ring_statistics_and_rescaled_step_vs_fp64
    python -m pytest -q -m gpu tests/test_model_gpu.py::test_preprocessing_warps_vs_oracle
    python -m pytest -q -m gpu tests/test_init_strength_gpu.py::test_noise_latents_parity
    python -m pytest -q -m gpu tests/test_keep_mask_gpu.py::test_keep_latents_parity
    python -m pytest -q -m gpu tests/test_hires_init_gpu.py::test_resize_pano_latent_parity tests/test_hires_init_gpu.py::test_vector_and_scalar_paths_give_the_same_bits
    python -m pytest -q -m gpu tests/test_multistep_sampler_gpu.py::test_multistep_step_kernel_all_modes tests/test_multistep_sampler_gpu.py::test_multistep_windows_kernel_all_modes_vs_fp64
    python -m pytest -q -m gpu tests/test_retime_init_gpu.py::test_retime_pano_latent_parity
    python -m pytest -q -m gpu tests/test_free_init_gpu.py::test_free_init_noise_parity
    python -m pytest -q -m gpu tests/test_release_mask_gpu.py::test_keep_latents_release_parity
    python -m pytest -q -m gpu tests/test_sphere_feather_gpu.py::test_sphere_distance2_parity
    python -m pytest -q -m gpu tests/test_guidance_interval_gpu.py::test_unguided_step_kernels_parity
    python -m pytest -q -m gpu tests/test_temporal_windows_gpu.py::test_windows_kernel_vs_fp64
    python -m pytest -q -m gpu tests/test_ff_fused_gpu.py
    python -m pytest -q -m gpu tests/test_projected_guidance_gpu.py::test_cfg_apg_scalars_vs_fp64 tests/test_projected_guidance_gpu.py::test_apg_ddim_step_kernel_all_modes tests/test_projected_guidance_gpu.py::test_apg_multistep_step_kernel_all_modes tests/test_projected_guidance_gpu.py::test_apg_windows_kernels_vs_fp64
    python -m pytest -q -m gpu tests/test_apg_momentum_gpu.py::test_momentum_scalars_vs_fp64 tests/test_apg_momentum_gpu.py::test_momentum_ddim_step_kernel_all_modes tests/test_apg_momentum_gpu.py::test_momentum_multistep_step_kernel_all_modes tests/test_apg_momentum_gpu.py::test_momentum_windows_kernels_vs_fp64

each as   rocprofv3 --kernel-trace --stats -M --output-format csv -d <dir>/<label> -o trace -- <command>   (mangled names; kernel trace only,
no counters), one rocprofv3 invocation per command, each under its own `timeout -k 10`; the job stops at the first step that fails.

    python tools/kernel_launch_coverage.py --emit-script <dir> > job.sh      # the MI355X job: per command an untraced run (its wall time x 3 is
                                                                            # the traced run's time limit), then the traced run; writes <dir>/<label>/
    python tools/kernel_launch_coverage.py --collect <dir> --commit <hash>   # <dir>/<label>/*kernel_stats.csv + meta.json -> tests/golden/kernel_launch_ledger_apg_momentum.json
    python tools/kernel_launch_coverage.py --collect <dir> --label <label>   # only these runs were traced again: the other runs' launches are taken
                                                                            # over from --base (default: the previous ledger) for the kernels the library still has
    python tools/kernel_launch_coverage.py --report                          # library kernels against the ledger: unlaunched, stale, unpaired dtypes
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (tests/golden/kernel_launch_coverage.json is the ledger of the library before the guidance-rescale kernels, kernel_launch_ledger.json the
# one before the windows kernels took their `wrap` argument, kernel_launch_ledger_ring.json the one before noise_latents_kernel,
# kernel_launch_ledger_init.json the one before keep_latents_kernel, kernel_launch_ledger_keep.json the one before
# resize_pano_latent_kernel, kernel_launch_ledger_resize.json the one before the multistep step kernels,
# kernel_launch_ledger_multistep.json the one before retime_pano_latent_kernel, kernel_launch_ledger_retime.json the one before the
# free_init kernels, kernel_launch_ledger_freeinit.json the one before keep_latents_kernel took its RELEASE argument and
# sphere_distance2_kernel, kernel_launch_ledger_release.json the one before the step kernels took their GUIDED argument and ddim_kernel,
# kernel_launch_ledger_interval.json the one before temporal_attn_windows_kernel, kernel_launch_ledger_tattn_windows.json the one before
# ff_fused_kernel, kernel_launch_ledger_ff_fused.json the one before the adaptive-projected-guidance kernels,
# kernel_launch_ledger_apg.json the one before their momentum forms: all fourteen kept as they were; the last one is read only as the
# default --base of a partial --collect)
LEDGER = os.path.join(ROOT, "tests", "golden", "kernel_launch_ledger_apg_momentum.json")
PREVIOUS_LEDGER = os.path.join(ROOT, "tests", "golden", "kernel_launch_ledger_apg.json")
LIB = os.path.join(ROOT, "imagine360_amd", "libim360_kernels.so")
LLVM = "/opt/rocm/lib/llvm/bin"
PREFIX = "_ZN5im360"

RUNS = [("test_kernels_gpu", ["tests/test_kernels_gpu.py"]),
        ("test_kernel_variants_gpu", ["tests/test_kernel_variants_gpu.py"]),
        ("test_ddim_stochastic_gpu", ["tests/test_ddim_stochastic_gpu.py::test_cfg_ddim_step_kernel_all_modes"]),
        ("test_context_windows_gpu", ["tests/test_context_windows_gpu.py::test_windows_kernel_all_modes_vs_fp64",
                                      "tests/test_context_windows_gpu.py::test_one_uniform_window_is_cfg_ddim_step_bit_for_bit"]),
        ("test_guidance_rescale_gpu", ["tests/test_guidance_rescale_gpu.py::test_cfg_rescale_factor_vs_fp64",
                                       "tests/test_guidance_rescale_gpu.py::test_rescaled_step_kernel_all_modes",
                                       "tests/test_guidance_rescale_gpu.py::test_rescaled_windows_kernel_all_modes_vs_fp64"]),
        ("test_context_loop_gpu", ["tests/test_context_loop_gpu.py::test_ring_kernel_all_modes_vs_fp64",
                                   "tests/test_context_loop_gpu.py::test_non_wrapping_tables_are_the_linear_entry_points_bit_for_bit",
                                   "tests/test_context_loop_gpu.py::test_rolling_the_clip_rolls_the_result_bit_for_bit",
                                   "tests/test_context_loop_gpu.py::test_ring_statistics_and_rescaled_step_vs_fp64"]),
        ("test_model_gpu", ["tests/test_model_gpu.py::test_preprocessing_warps_vs_oracle"]),
        ("test_init_strength_gpu", ["tests/test_init_strength_gpu.py::test_noise_latents_parity"]),
        ("test_keep_mask_gpu", ["tests/test_keep_mask_gpu.py::test_keep_latents_parity"]),
        ("test_hires_init_gpu", ["tests/test_hires_init_gpu.py::test_resize_pano_latent_parity",
                                 "tests/test_hires_init_gpu.py::test_vector_and_scalar_paths_give_the_same_bits"]),
        ("test_multistep_sampler_gpu", ["tests/test_multistep_sampler_gpu.py::test_multistep_step_kernel_all_modes",
                                        "tests/test_multistep_sampler_gpu.py::test_multistep_windows_kernel_all_modes_vs_fp64"]),
        ("test_retime_init_gpu", ["tests/test_retime_init_gpu.py::test_retime_pano_latent_parity"]),
        ("test_free_init_gpu", ["tests/test_free_init_gpu.py::test_free_init_noise_parity"]),
        ("test_release_mask_gpu", ["tests/test_release_mask_gpu.py::test_keep_latents_release_parity"]),
        ("test_sphere_feather_gpu", ["tests/test_sphere_feather_gpu.py::test_sphere_distance2_parity"]),
        ("test_guidance_interval_gpu", ["tests/test_guidance_interval_gpu.py::test_unguided_step_kernels_parity"]),
        ("test_temporal_windows_gpu", ["tests/test_temporal_windows_gpu.py::test_windows_kernel_vs_fp64"]),
        ("test_ff_fused_gpu", ["tests/test_ff_fused_gpu.py"]),
        ("test_projected_guidance_gpu", ["tests/test_projected_guidance_gpu.py::test_cfg_apg_scalars_vs_fp64",
                                         "tests/test_projected_guidance_gpu.py::test_apg_ddim_step_kernel_all_modes",
                                         "tests/test_projected_guidance_gpu.py::test_apg_multistep_step_kernel_all_modes",
                                         "tests/test_projected_guidance_gpu.py::test_apg_windows_kernels_vs_fp64"]),
        ("test_apg_momentum_gpu", ["tests/test_apg_momentum_gpu.py::test_momentum_scalars_vs_fp64",
                                   "tests/test_apg_momentum_gpu.py::test_momentum_ddim_step_kernel_all_modes",
                                   "tests/test_apg_momentum_gpu.py::test_momentum_multistep_step_kernel_all_modes",
                                   "tests/test_apg_momentum_gpu.py::test_momentum_windows_kernels_vs_fp64"])]


def command(args):
    return "python -m pytest -q -m gpu -p no:cacheprovider " + " ".join(args)


def library_kernels(lib=LIB):
    """Kernel names (the .name entries of the code objects' metadata notes: kernels only, not device functions) of every gfx950 code
    object inside the library, or None when the LLVM binutils are missing."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        return None
    tmp = tempfile.mkdtemp()
    try:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", so], capture_output=True, cwd=tmp, check=True)
        names = set()
        for f in sorted(glob.glob(so + ".*gfx950")):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f], capture_output=True, text=True, check=True).stdout
            names.update(re.findall(r"\.name:\s+(\S+)", notes))
        return sorted(n for n in names if n.startswith(PREFIX))
    finally:
        shutil.rmtree(tmp)


def dtype_partner(name):
    """The other 16-bit instantiation of a dtype-templated kernel (bf16 <-> fp16 in the mangled name), or None."""
    if "DF16b" in name:
        return name.replace("DF16b", "DF16_")
    if "DF16_" in name:
        return name.replace("DF16_", "DF16b")
    return None


def read_counts(path):
    """{kernel name: launches} of one rocprofv3 CSV: a *_kernel_stats.csv (Name, Calls) or a *_kernel_trace.csv (Kernel_Name per launch)."""
    counts = {}
    with open(path, newline="") as fh:
        rows = csv.DictReader(l for l in fh if not l.startswith("#"))
        for r in rows:
            if "Kernel_Name" in r:
                name, n = r["Kernel_Name"], 1
            else:
                name, n = r["Name"], int(r["Calls"])
            name = name.split(".kd")[0].strip()
            if name.startswith(PREFIX):
                counts[name] = counts.get(name, 0) + n
    return counts


def collect(directory, commit, labels=(), base=None):
    runs, kernels = [], {}
    old = None
    if labels:
        # a partial regeneration: the runs that were not traced again keep the launches the base ledger recorded for them
        with open(base or (LEDGER if os.path.exists(LEDGER) else PREVIOUS_LEDGER)) as fh:
            old = json.load(fh)
        have_now = library_kernels()
        for name, per in old["kernels"].items():
            kept = {lab: n for lab, n in per.items() if lab not in labels}
            if kept and (have_now is None or name in have_now):
                kernels[name] = kept
    for label, args in RUNS:
        if labels and label not in labels:
            runs += [r for r in old["runs"] if r["label"] == label]
            continue
        d = os.path.join(directory, label)
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)) or \
            sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
        if not files:
            sys.exit(f"no *kernel_stats.csv / *kernel_trace.csv under {d}: run the job of --emit-script first")
        meta = json.load(open(os.path.join(d, "meta.json")))
        if meta.get("traced_rc") != 0 or meta.get("untraced_rc") != 0:
            sys.exit(f"{label}: the traced command did not pass ({meta}); a ledger is taken from passing tests only")
        for f in files:
            for name, n in read_counts(f).items():
                kernels.setdefault(name, {})
                kernels[name][label] = kernels[name].get(label, 0) + n
        runs.append({"label": label, "command": "rocprofv3 --kernel-trace --stats -M --output-format csv -- " + command(args),
                     "untraced_wall_s": meta["untraced_s"], "traced_wall_s": meta["traced_s"], "pytest_summary": meta.get("summary", "")})
    have = library_kernels()
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "imagine360_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if os.path.isfile(os.path.join(csrc, f)):
            h.update(f.encode() + b"\0" + open(os.path.join(csrc, f), "rb").read())
    ledger = {"commit": commit,
              "csrc_sha256": h.hexdigest(),
              "note": "launches per traced test file of every im360 kernel; regenerate with tools/kernel_launch_coverage.py after adding or re-templating a kernel"
                      + (f"; runs {', '.join(labels)} traced at this commit, the others taken over from the ledger of commit {old['commit']}" if labels else ""),
              "library_kernels": None if have is None else len(have),
              "runs": runs,
              "kernels": {k: kernels[k] for k in sorted(kernels)}}
    with open(LEDGER, "w") as fh:
        json.dump(ledger, fh, indent=1, sort_keys=False)
        fh.write("\n")
    print(f"wrote {os.path.relpath(LEDGER, ROOT)}: {len(kernels)} kernels launched")
    return ledger


def report(without=()):
    ledger = json.load(open(LEDGER))
    have = library_kernels()
    if have is None:
        sys.exit("ROCm LLVM binutils not installed")
    launched = {k for k, v in ledger["kernels"].items() if sum(n for lab, n in v.items() if lab not in without) > 0}
    missing = [k for k in have if k not in launched]
    stale = sorted(k for k in ledger["kernels"] if k not in have)
    unpaired = sorted(k for k in launched if dtype_partner(k) in have and dtype_partner(k) not in launched)
    print(f"library: {len(have)} im360 kernels; launched under a reference check: {len(launched & set(have))}" + (f" (without {', '.join(without)})" if without else ""))
    for title, names in (("NOT LAUNCHED", missing), ("IN THE LEDGER BUT NOT IN THE LIBRARY", stale), ("LAUNCHED WITHOUT THE OTHER DTYPE", unpaired)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("   ", n)
    return missing, stale, unpaired


def emit_script(directory, labels=()):
    out = ["#!/bin/bash", "# generated by tools/kernel_launch_coverage.py --emit-script: untraced + traced run of every ledger command", "set -u",
           "R=$PWD", f"OUT=$R/{directory}", "mkdir -p $OUT", "export TMPDIR=/tmp"]
    for label, args in RUNS:
        if labels and label not in labels:
            continue
        cmd = command(args)
        out += [f"# ---- {label}",
                f"D=$OUT/{label}; mkdir -p $D",
                "t0=$(date +%s)",
                f"timeout -k 10 ${{UNTRACED_LIMIT:-900}} {cmd} ${{PYTEST_EXTRA:-}} > $D/untraced.log 2>&1; rc0=$?",
                "t1=$(date +%s)",
                "u=$((t1 - t0 + 1))",
                "tail -3 $D/untraced.log",
                "if [ $rc0 -ne 0 ]; then echo \"" + label + ": untraced run failed rc=$rc0 -- stopping\"; "
                "echo \"{\\\"untraced_rc\\\": $rc0, \\\"untraced_s\\\": $u, \\\"traced_rc\\\": null, \\\"traced_s\\\": null}\" > $D/meta.json; exit 1; fi",
                "lim=$((3 * u))       # three times the untraced wall time",
                "t0=$(date +%s)",
                f"timeout -k 10 $lim rocprofv3 --kernel-trace --stats -M --output-format csv -d $D -o trace -- {cmd} > $D/traced.log 2>&1; rc1=$?",
                "t1=$(date +%s)",
                "t=$((t1 - t0 + 1))",
                "find $D -name '*kernel_trace.csv' -delete; find $D -name '*.db' -delete",
                "s=$(grep -E '(passed|failed|error)' $D/traced.log | tail -1 | tr -d '\"')",
                "echo \"{\\\"untraced_rc\\\": $rc0, \\\"untraced_s\\\": $u, \\\"traced_rc\\\": $rc1, \\\"traced_s\\\": $t, \\\"limit_s\\\": $lim, \\\"summary\\\": \\\"$s\\\"}\" > $D/meta.json",
                "cat $D/meta.json",
                "if [ $rc1 -ne 0 ]; then echo \"" + label + ": traced run failed rc=$rc1 -- stopping\"; tail -20 $D/traced.log; exit 1; fi"]
    out.append("echo ALL_TRACED_OK")
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--emit-script", metavar="DIR", help="print the MI355X job that writes DIR/<label>/ (DIR relative to the repository root)")
    ap.add_argument("--label", action="append", default=[], help="--emit-script / --collect: only this run (repeatable; a job has a time limit of its own)")
    ap.add_argument("--base", default=None, help="--collect --label: the ledger whose other runs are taken over (default: the current ledger, else the previous one)")
    ap.add_argument("--collect", metavar="DIR", help="build the ledger from DIR/<label>/")
    ap.add_argument("--commit", default=None, help="commit the traced tree was built from (default: git rev-parse HEAD)")
    ap.add_argument("--report", action="store_true", help="compare the ledger with the kernels inside the built library")
    ap.add_argument("--without", action="append", default=[], help="--report: ignore the launches of this run label (repeatable)")
    a = ap.parse_args()
    if a.emit_script:
        emit_script(a.emit_script, tuple(a.label))
    if a.collect:
        commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=ROOT, check=True).stdout.strip()
        collect(a.collect, commit, tuple(a.label), a.base)
    if a.report:
        missing, stale, unpaired = report(tuple(a.without))
        sys.exit(1 if (missing or stale or unpaired) else 0)


if __name__ == "__main__":
    main()
