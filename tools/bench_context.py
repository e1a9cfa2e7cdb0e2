#!/usr/bin/env python
"""Sliding temporal context windows at BASELINE cfg4 size (48 frames, full width, CFG batch 2): one windowed denoising step
(L = 16, overlap 4 -> 4 windows, one captured hipGraph: graph_step.GraphedWindowedStep) next to the 48-frame full-attention step
(graph_step.GraphedDenoiseStep), replays alternated round by round, timed with a host clock around work that ends in a device
synchronise; and the blend + CFG + DDIM kernel alone next to cfg_ddim_step_kernel on the same perspective latent, timed with
device events, with the bytes each has to move computed from the shapes.  Prints one line of JSON (and writes it to --out).
    python tools/bench_context.py [--steps 3] [--rounds 3] [--kernel-iters 200] [--out profiles/context_windows.json]
    python tools/bench_context.py --kernel-only       # skip the two whole steps
    python tools/bench_context.py --sampler dpmpp2m   # any of the modes with scheduler.DPMSolverMultistepScheduler (DPM-Solver++ 2M) instead of
                                                      # DDIM: the captured steps own their x0 histories, and the two kernels timed alone are
                                                      # cfg_multistep_step_windows / cfg_multistep_step at a second-order timestep
    python tools/bench_context.py --loop [--passes 2] # the looping clip: the ring plan's captured step next to the linear plan's (same F, L,
                                                      # overlap; ms per step and per window), and the ring entry point of the blend kernel next to
                                                      # the linear one on the SAME non-wrapping tables and on the ring's own; every measurement is
                                                      # made --passes times over, so the spread between identical passes stands next to the numbers
    python tools/bench_context.py --frames 32 --context-frames 16 --context-overlap 4 --context-level model|attention|both [--loop]
                                                      # WHERE the windows apply: the captured step of whole-model windows (model) and of windows
                                                      # inside the motion modules' attention (attention: one forward of all <= 64 frames,
                                                      # kernels.temporal_attention_windows), alternated round by round for `both`
    python tools/bench_context.py --strength 0.5 [--frames 48] [--num-steps 6] [--loop]
                                                      # the refinement pass: whole pipeline calls (encode, loop, decode; host clock around a call that
                                                      # ends in a device synchronise) from pure noise and, with init_latents taken from a first call,
                                                      # at this strength, alternated --rounds times; over context windows when --frames > 16 (--loop:
                                                      # on a ring); and kernels.noise_latents at the size of that clip next to the torch-op composition
                                                      # it replaces (device events, alternated), with the bytes the launch has to move
    python tools/bench_context.py --strength 0.5 --regenerate-mask half|feather [--frames 16]
                                                      # part of the clip kept (pipeline regenerate_mask; even frames: the left half, odd frames: a
                                                      # rectangle across the seam): the refinement call with the mask next to the same call without it,
                                                      # alternated --rounds times, and kernels.keep_latents next to the torch ops it replaces;
                                                      # feather: that mask with regenerate_feather=20 in regenerate_mode="release"
    python tools/bench_context.py --init-scale 2 --strength 0.5 [--pano-hw 128 256] [--frames 16] [--num-steps 20]
                                                      # the hi-res pass: a first pipeline call from pure noise at 1/N of the size plus a second call
                                                      # at the full size from its latent (init_latents smaller than the run: kernels.resize_pano_latent)
                                                      # at this strength, next to ONE call from pure noise at the full size, alternated --rounds times
                                                      # after one warm-up of every shape; and kernels.resize_pano_latent at these sizes, both modes, next
                                                      # to the eager definition pano_geometry.resize_pano_latent on the GPU.  --pano-hw: the latent size
                                                      # of the full-size run (default 128 256: BASELINE cfg5, 1024 x 2048 pixels)
    python tools/bench_context.py --init-frames 16 --frames 31 --strength 0.5 [--loop] [--num-steps 20]
                                                      # the frame-interpolation pass: a first pipeline call from pure noise with --init-frames frames
                                                      # plus a second call with --frames frames from its latent (init_latents with fewer frames than
                                                      # the run: kernels.retime_pano_latent; context windows of 16, --loop: on a ring) at this strength,
                                                      # next to ONE call from pure noise with --frames frames, alternated --rounds times after one
                                                      # warm-up of every shape; and kernels.retime_pano_latent at the cfg2 latent size, both modes,
                                                      # next to the eager definition pano_geometry.retime_pano_latent on the GPU
    python tools/bench_context.py --free-init 3 [--frames 16] [--num-steps 25] [--loop]
                                                      # FreeInit passes: whole pipeline calls with free_init_iters = N next to the call without it,
                                                      # alternated --rounds times after one warm-up of each (context windows of 16 when --frames > 16,
                                                      # --loop: on a ring, the frame axis of the filter periodic); and kernels.free_init_noise at the
                                                      # size of that clip next to the eager definition pano_geometry.free_init_noise on the GPU"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagine360_amd import configs, kernels, synthetic  # noqa: E402
from imagine360_amd.context import WindowPlan, coverage, ip_cache_slots  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler  # noqa: E402

FRAMES, LENGTH, OVERLAP = 48, 16, 4
PANO_HW, PERS_HW, PERS_PX = (64, 128), (32, 32), 256


def kernel_bytes(sample, plan):
    """Bytes the two kernels have to move for ``sample`` (no variance noise): the windowed one reads both CFG halves of every
    window once (2 x sum of coverage) + the sample and writes one latent; the plain one reads uncond, cond, sample and writes one."""
    per_frame = sample.numel() // plan.frames * sample.element_size()
    cov = sum(coverage(plan.frames, plan.length, plan.starts, loop=plan.loop))
    return dict(windows=(2 * cov + 2 * plan.frames) * per_frame, plain=4 * plan.frames * per_frame)


def time_kernels(sch, plan, sample, iters, rounds=5, ring_plan=None):
    """Device-event time of the two kernels on ``sample`` (alternated round by round, ``iters`` back-to-back launches each).
    ``ring_plan``: instead the linear entry point, the ring entry point on the same (non-wrapping) tables, and the ring entry point on
    the ring plan's tables."""
    t = sch._timesteps_host[8]
    coefs = sch.step_coefficients(t, 0.0, 7.5)
    mode = sch.kernel_mode()
    fd = sample.dim() - 3
    shape = list(sample.shape)
    shape[fd] = plan.length
    preds = torch.randn(len(plan), 2, *shape[1:], device=sample.device).to(sample.dtype)
    u, c = (torch.randn(sample.shape, device=sample.device).to(sample.dtype) for _ in range(2))
    fns = dict(windows=lambda: kernels.cfg_ddim_step_windows(preds, sample, None, plan.starts_dev, plan.weights, mode, coefs),
               plain=lambda: kernels.cfg_ddim_step(u, c, sample, None, mode, coefs))
    if hasattr(sch, "new_history"):               # --sampler dpmpp2m: a second-order step (history read and written)
        assert ring_plan is None, "--sampler dpmpp2m times the linear and the plain kernel"
        hist = sch.new_history(sample)
        fns = dict(windows=lambda: kernels.cfg_multistep_step_windows(preds, sample, hist, plan.starts_dev, plan.weights, mode, coefs),
                   plain=lambda: kernels.cfg_multistep_step(u, c, sample, hist, mode, coefs))
    if ring_plan is not None:
        assert len(ring_plan) == len(plan) and ring_plan.length == plan.length        # the same prediction buffer serves all three
        fns = dict(linear=fns["windows"],
                   ring_entry_linear_tables=lambda: kernels.cfg_ddim_step_windows(preds, sample, None, plan.starts_dev, plan.weights, mode, coefs,
                                                                                  ring=True),
                   ring=lambda: kernels.cfg_ddim_step_windows(preds, sample, None, ring_plan.starts_dev, ring_plan.weights, mode, coefs, ring=True))
    times = {k: [] for k in fns}
    for r in range(rounds + 1):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:                                   # round 0 warms both up
                times[name].append(a.elapsed_time(b) / iters * 1e3)
    return {k: dict(us_min=min(v), us_median=statistics.median(v)) for k, v in times.items()}


def time_steps(graphs, ts_host, steps, rounds, per_name=None):
    """Host-clock ms per step of captured steps, replays alternated round by round; round 0 warms every graph up.  ``per_name``:
    {name: its own timestep list} instead of ``ts_host`` (--guidance-interval: the timestep selects the graph)."""
    times = {k: [] for k in graphs}
    for r in range(rounds + 1):
        for name, gs in graphs.items():
            ts = ts_host if per_name is None else per_name[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                gs.step(ts[i % len(ts)])
            torch.cuda.synchronize()
            if r:
                times[name].append((time.perf_counter() - t0) / steps * 1e3)
    return {k: dict(ms_min=min(v), ms_median=statistics.median(v), rounds=len(v), steps_per_round=steps) for k, v in times.items()}


def spread(passes, key):
    """Largest relative difference of ``key`` between identical passes."""
    v = [p[key] for p in passes]
    return (max(v) - min(v)) / min(v)


def loop_bench(args, sch, dev, dt, ts_host):
    """--loop: the ring plan against the linear plan of the same frames / length / overlap."""
    line = WindowPlan(FRAMES, LENGTH, OVERLAP, "pyramid", dev)
    ring = WindowPlan(FRAMES, LENGTH, OVERLAP, "pyramid", dev, loop=True)
    res = dict(tool="bench_context --loop", frames=FRAMES, context_frames=LENGTH, context_overlap=OVERLAP, linear_windows=line.starts,
               ring_windows=ring.starts, pano_hw=PANO_HW, pers_hw=PERS_HW, dtype="bfloat16", device=torch.cuda.get_device_name(0),
               passes=args.passes)
    pers = torch.randn(1, 20, 4, FRAMES, *PERS_HW, device=dev).to(dt)
    kp = [time_kernels(sch, line, pers, args.kernel_iters, ring_plan=ring) for _ in range(args.passes)]
    res["blend_kernel"] = {k: dict(us_min=[p[k]["us_min"] for p in kp], us_median=[p[k]["us_median"] for p in kp],
                                   spread_between_passes=spread([p[k] for p in kp], "us_min")) for k in kp[0]}
    best = {k: min(v["us_min"]) for k, v in res["blend_kernel"].items()}
    res["blend_kernel"]["ring_entry_over_linear_same_tables"] = best["ring_entry_linear_tables"] / best["linear"]
    res["blend_kernel"]["ring_over_linear"] = best["ring"] / best["linear"]
    res["blend_kernel"]["tensor"] = list(pers.shape)
    res["blend_kernel"]["bytes"] = dict(linear=kernel_bytes(pers, line)["windows"], ring=kernel_bytes(pers, ring)["windows"])
    if not args.kernel_only:
        mv = configs.build_mv_model(1, device=dev, dtype=dt, xformers=True)
        mv.dual_stream, mv.warp_streams = True, True
        inp = synthetic.mv_inputs(frames=FRAMES, pano_hw=PANO_HW, pers_hw=PERS_HW, seed=1, dtype=dt, device=dev)
        inp.pop("timestep")
        cams = synthetic.icosahedron_cameras(90, PERS_PX, device=dev)
        pano_lat, pers_lat = inp["pano_latent"][:1, :4].contiguous(), inp["latents"][:1, :, :4].contiguous()
        from imagine360_amd.graph_step import GraphedWindowedStep
        graphs = {}
        for name, plan in (("linear_step", line), ("ring_step", ring)):
            with ip_cache_slots(mv, len(plan)):
                graphs[name] = GraphedWindowedStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, plan, warmup=1)
            torch.cuda.synchronize()
            print(f"captured: {name}", file=sys.stderr, flush=True)
        sp = [time_steps(graphs, ts_host, args.steps, args.rounds) for _ in range(args.passes)]
        for name, plan in (("linear_step", line), ("ring_step", ring)):
            ms = min(p[name]["ms_min"] for p in sp)
            res[name] = dict(ms_min=[p[name]["ms_min"] for p in sp], ms_median=[p[name]["ms_median"] for p in sp], windows=len(plan),
                             ms_per_window=ms / len(plan), spread_between_passes=spread([p[name] for p in sp], "ms_min"),
                             rounds=args.rounds, steps_per_round=args.steps)
        res["ring_over_linear_step"] = min(res["ring_step"]["ms_min"]) / min(res["linear_step"]["ms_min"])
        res["ring_over_linear_per_window"] = res["ring_step"]["ms_per_window"] / res["linear_step"]["ms_per_window"]
        res["finite"] = bool(all(torch.isfinite(g.pano_lat.float()).all() and torch.isfinite(g.pers_lat.float()).all() for g in graphs.values()))
    return res


def torch_noise_latents(x0, noise, idx, ok, sqrt_a, sqrt_b):
    """What ``kernels.noise_latents`` replaces, in torch ops: the noised panorama start in fp32, rounded, and its gather by the
    tables of ``init_noise``, masked, in the perspective latent's layout (``idx`` int64, ``ok`` bool, as ``init_noise`` holds them)."""
    _, C, F, h, w = x0.shape
    pano = (sqrt_a * x0.float() + sqrt_b * noise.permute(0, 2, 1, 3, 4)).to(x0.dtype)
    flat = pano.permute(0, 2, 1, 3, 4).reshape(1, F, C, h * w)
    pers = flat[..., idx.reshape(-1)].reshape(1, F, C, *idx.shape) * ok
    return pano.contiguous(), pers.permute(0, 3, 2, 1, 4, 5).contiguous()


def time_noise_latents(sch, frames, dev, dt, iters, rounds=5):
    """Device-event time of ``kernels.noise_latents`` and of the torch-op composition on one clip (alternated round by round, ``iters``
    back-to-back calls each, allocation of the results included), and the bytes of noise, x0 and the two results."""
    from imagine360_amd import pano_geometry as G
    cams = synthetic.icosahedron_cameras(90, PERS_PX)
    idx64, okb = (t.to(dev) for t in G.nearest_e2p_index(*PANO_HW, *PERS_HW, cams))
    idx32, ok8 = idx64.to(torch.int32), okb.to(torch.uint8)
    x0 = torch.randn(1, 4, frames, *PANO_HW, device=dev).to(dt)
    noise = torch.randn(1, frames, 4, *PANO_HW, device=dev)
    sa, sb = sch.noise_coefficients(sch.timesteps_for_strength(0.5)[1][0])
    fns = dict(kernel=lambda: kernels.noise_latents(x0, noise, idx32, ok8, sa, sb), torch_ops=lambda: torch_noise_latents(x0, noise, idx64, okb, sa, sb))
    a, b = fns["kernel"](), fns["torch_ops"]()
    # the two are not the same bits: torch rounds sqrt_a * x0 to fp32 before the add, the kernel fuses the product into one fma
    differ = float((a[0] != b[0]).float().mean())
    max_diff = float((a[0].float() - b[0].float()).abs().max())
    times = {k: [] for k in fns}
    for r in range(rounds + 1):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:                                   # round 0 warms both up
                times[name].append(e0.elapsed_time(e1) / iters * 1e3)
    nbytes = noise.numel() * 4 + 2 * x0.numel() * 2 + a[1].numel() * 2
    res = {k: dict(us_min=min(v), us_median=statistics.median(v)) for k, v in times.items()}
    res.update(bytes=nbytes, tables_bytes=idx32.numel() * 5, gb_per_s_kernel=nbytes / (res["kernel"]["us_min"] * 1e-6) / 1e9,
               x0=list(x0.shape), pers=list(a[1].shape), pano_fraction_differing_from_torch_ops=differ, pano_max_abs_diff=max_diff,
               note="event time over back-to-back calls; the working set fits the Infinity Cache, so GB/s is an effective rate")
    return res


def half_mask(frames, H, W):
    """[1, F, 1, H, W], 1 = regenerate: even frames keep the left half of the columns, odd frames a rectangle across the seam."""
    m = torch.ones(1, frames, 1, H, W)
    m[:, 0::2, :, :, :W // 2] = 0.0
    m[:, 1::2, :, H // 4:3 * H // 4, 7 * W // 8:] = 0.0
    m[:, 1::2, :, H // 4:3 * H // 4, :W // 8] = 0.0
    return m


def torch_keep_latents(pano, pers, x0, noise, mask, idx, ok, sqrt_a, sqrt_b):
    """What ``kernels.keep_latents`` replaces, in torch ops: add_noise in fp32 and its rounding, the gather of it and of the mask by
    the tables, and one lerp per branch (``idx`` int64, ``ok`` bool, ``mask`` [F, h, w]); results in fresh tensors."""
    _, C, F, h, w = x0.shape
    known = (sqrt_a * x0.float() + sqrt_b * noise.permute(0, 2, 1, 3, 4)).to(x0.dtype)
    flat = idx.reshape(-1)
    kg = known.reshape(C, F, h * w)[..., flat].reshape(C, F, *idx.shape).permute(2, 0, 1, 3, 4).unsqueeze(0)
    wg = mask.reshape(F, h * w)[:, flat].reshape(F, *idx.shape).permute(1, 0, 2, 3)[None, :, None]
    wg = torch.where(ok[None, :, None, None], wg, 1.0)
    return torch.lerp(known, pano, mask[None, None].to(pano.dtype)), torch.lerp(kg, pers, wg.to(pers.dtype))


def time_keep_latents(sch, frames, dev, dt, iters, rounds=5):
    """Device-event time of ``kernels.keep_latents`` (in place) and of the torch-op composition on one clip under the half mask
    (alternated round by round, ``iters`` back-to-back calls each), and the bytes the launch has to move: x0, noise and mask read, the
    parts of the two latents the mask changes read (fractional values only) and written."""
    from imagine360_amd import pano_geometry as G
    cams = synthetic.icosahedron_cameras(90, PERS_PX)
    idx64, okb = (t.to(dev) for t in G.nearest_e2p_index(*PANO_HW, *PERS_HW, cams))
    idx32, ok8 = idx64.to(torch.int32), okb.to(torch.uint8)
    x0, pano = (torch.randn(1, 4, frames, *PANO_HW, device=dev).to(dt) for _ in range(2))
    pers = torch.randn(1, idx32.shape[0], 4, frames, *PERS_HW, device=dev).to(dt)
    noise = torch.randn(1, frames, 4, *PANO_HW, device=dev)
    mask = torch.nn.functional.interpolate(half_mask(frames, PANO_HW[0] * 8, PANO_HW[1] * 8).transpose(2, 1),
                                           size=(frames, *PANO_HW))[0, 0].contiguous().to(dev)
    sa, sb = sch.noise_coefficients(sch.timesteps_for_strength(0.5)[1][1])
    fns = dict(kernel=lambda: kernels.keep_latents(pano, pers, x0, noise, mask, idx32, ok8, sa, sb),
               torch_ops=lambda: torch_keep_latents(pano, pers, x0, noise, mask, idx64, okb, sa, sb))
    b = fns["torch_ops"]()                                    # before the kernel blends in place
    a = fns["kernel"]()
    max_diff = max(float((a[0].float() - b[0].float()).abs().max()), float((a[1].float() - b[1].float()).abs().max()))
    times = {k: [] for k in fns}
    for r in range(rounds + 1):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:                                   # round 0 warms both up
                times[name].append(e0.elapsed_time(e1) / iters * 1e3)
    kept_pano = float((mask < 1).float().mean())
    kept_pers = float(((mask.reshape(frames, -1)[:, idx64.reshape(-1)] < 1) & okb.reshape(-1)).float().mean())
    nbytes = int(noise.numel() * 4 + x0.numel() * 2 + mask.numel() * 4 + kept_pano * pano.numel() * 2 + kept_pers * pers.numel() * 2)
    res = {k: dict(us_min=min(v), us_median=statistics.median(v)) for k, v in times.items()}
    res.update(bytes=nbytes, tables_bytes=idx32.numel() * 5, gb_per_s_kernel=nbytes / (res["kernel"]["us_min"] * 1e-6) / 1e9,
               x0=list(x0.shape), pers=list(pers.shape), kept_fraction_pano=kept_pano, kept_fraction_pers=kept_pers,
               max_abs_diff_from_torch_ops=max_diff,
               note="event time over back-to-back calls on the same tensors (after the first call the kept region already holds the "
                    "noised clip: the same loads and stores, the same values); the working set fits the Infinity Cache")
    return res


def time_resize(small_hw, big_hw, frames, dev, dt, iters, rounds=5):
    """Device-event time of ``kernels.resize_pano_latent`` and of the eager definition ``pano_geometry.resize_pano_latent`` on the GPU,
    both modes (alternated round by round, ``iters`` back-to-back calls each, allocation of the result included), the spread over the
    rounds, and the bytes the launch has to move."""
    from imagine360_amd import pano_geometry as G
    x = (1.5 * torch.randn(1, 4, frames, *small_hw, device=dev)).to(dt)
    res = dict(x=list(x.shape), out=[1, 4, frames, *big_hw], bytes=x.numel() * 2 + 4 * frames * big_hw[0] * big_hw[1] * 2, iters=iters, rounds=rounds)
    for mode in G.RESIZE_MODES:
        fns = dict(kernel=lambda: kernels.resize_pano_latent(x, *big_hw, mode), eager=lambda: G.resize_pano_latent(x, *big_hw, mode))
        ref = G.resize_pano_latent(x.double(), *big_hw, mode)
        diff = {k: float((fn().double() - ref).abs().max()) for k, fn in fns.items()}
        times = {k: [] for k in fns}
        for r in range(rounds + 1):
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r:                                   # round 0 warms both up
                    times[name].append(e0.elapsed_time(e1) / iters * 1e3)
        res[mode] = {k: dict(us_min=min(v), us_median=statistics.median(v), us_max=max(v), max_abs_diff_from_fp64=diff[k]) for k, v in times.items()}
        res[mode]["eager_over_kernel"] = res[mode]["eager"]["us_min"] / res[mode]["kernel"]["us_min"]
    res["note"] = ("event time over back-to-back calls; the eager definition blends in bf16 (several roundings), the kernel in fp32 (one); "
                   "the working set fits the Infinity Cache")
    return res


def time_retime(f, frames, hw, loop, dev, dt, iters, rounds=5):
    """Device-event time of ``kernels.retime_pano_latent`` and of the eager definition ``pano_geometry.retime_pano_latent`` on the GPU,
    both modes (alternated round by round, ``iters`` back-to-back calls each, allocation of the result included), the spread over the
    rounds, and the bytes the launch has to move (a keyframe reads one frame, a linear in-between two, a cubic one four)."""
    from imagine360_amd import pano_geometry as G
    from imagine360_amd.context import keyframe_frames
    x = (1.5 * torch.randn(1, 4, f, *hw, device=dev)).to(dt)
    keys = len(keyframe_frames(f, frames, loop))
    plane = 4 * hw[0] * hw[1] * 2
    res = dict(x=list(x.shape), out=[1, 4, frames, *hw], loop=bool(loop), keyframes=keys, iters=iters, rounds=rounds)
    for mode, taps in zip(G.RETIME_MODES, (2, 4)):
        fns = dict(kernel=lambda: kernels.retime_pano_latent(x, frames, mode, loop), eager=lambda: G.retime_pano_latent(x, frames, mode, loop))
        ref = G.retime_pano_latent(x.double(), frames, mode, loop)
        diff = {k: float((fn().double() - ref).abs().max()) for k, fn in fns.items()}
        times = {k: [] for k in fns}
        for r in range(rounds + 1):
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if r:                                   # round 0 warms both up
                    times[name].append(e0.elapsed_time(e1) / iters * 1e3)
        res[mode] = {k: dict(us_min=min(v), us_median=statistics.median(v), us_max=max(v), max_abs_diff_from_fp64=diff[k]) for k, v in times.items()}
        res[mode]["eager_over_kernel"] = res[mode]["eager"]["us_min"] / res[mode]["kernel"]["us_min"]
        res[mode]["bytes"] = plane * (frames + keys + taps * (frames - keys))
        res[mode]["gb_per_s_kernel"] = res[mode]["bytes"] / (res[mode]["kernel"]["us_min"] * 1e-6) / 1e9
    res["note"] = ("event time over back-to-back calls; the eager definition blends in bf16 (several roundings), the kernel in fp32 (one); "
                   "the working set fits the Infinity Cache, and at this size the launch is latency-bound")
    return res


def retime_bench(args, sch, dev, dt):
    """--init-frames f: the two-pass run (f frames from pure noise, then --frames frames from its latent at --strength, in windows of 16
    when --frames > 16) next to one run from pure noise with --frames frames; whole pipeline calls (encode, loop, decode), host clock
    around a call that ends in a device synchronise."""
    import random

    from imagine360_amd.pipeline import AnimationPipeline
    f, frames = args.init_frames, args.frames
    assert 1 <= f <= frames, f"--init-frames {f} must be at most --frames {frames}"
    res = dict(tool="bench_context --init-frames", init_frames=f, strength=args.strength, frames=frames, num_inference_steps=args.num_steps,
               pano_hw=PANO_HW, dtype="bfloat16", device=torch.cuda.get_device_name(0))
    res["retime_pano_latent"] = time_retime(f, frames, PANO_HW, args.loop, dev, dt, args.kernel_iters)
    if args.kernel_only:
        return res
    mv = configs.build_mv_model(1, device=dev, dtype=dt, xformers=True)
    mv.dual_stream, mv.warp_streams = True, True
    vae = configs.build_vae(1, device=dev, dtype=dt)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, type(sch)(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
    pipe._no_progress = True
    vbs = {n: synthetic.video_batch(frames=n, pano_hw=(PANO_HW[0] * 8, PANO_HW[1] * 8), seed=1) for n in (f, frames)}
    cond = synthetic.conditioning(frames=max(frames, 16), seed=1)
    windows = {n: (dict(context_frames=LENGTH, context_overlap=OVERLAP, context_loop=args.loop) if n > LENGTH else {}) for n in (f, frames)}
    res["windows"] = windows[frames]

    def call(n, **kw):
        torch.manual_seed(21)
        random.seed(21)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vid = pipe("synthetic", num_inference_steps=args.num_steps, guidance_scale_text=7.5, negative_prompt="", latents_dtype=dt,
                   video_batch=vbs[n], use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video",
                   prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **windows[n], **kw).videos
        torch.cuda.synchronize()
        assert vid.shape[2] == n
        return (time.perf_counter() - t0) * 1e3, bool(torch.isfinite(vid).all())

    def two_pass():
        a, ok_a = call(f)
        b, ok_b = call(frames, init_latents=pipe.last_latents[0], strength=args.strength, init_retime="linear")
        return dict(first_pass_ms=a, second_pass_ms=b, total_ms=a + b), ok_a and ok_b

    sch.set_timesteps(args.num_steps)
    res["steps"] = dict(first_pass=args.num_steps, second_pass=len(sch.timesteps_for_strength(args.strength)[1]), direct=args.num_steps)
    warm, fin = two_pass()                                  # warms every shape of both frame counts up
    res["warm_up"] = dict(two_pass=warm, direct_ms=call(frames)[0])
    print("warm-up done", file=sys.stderr, flush=True)
    runs = dict(two_pass=[], direct=[])
    for _ in range(args.rounds):
        t, ok = two_pass()
        runs["two_pass"].append(t)
        ms, ok2 = call(frames)
        runs["direct"].append(ms)
        fin = fin and ok and ok2
    res["two_pass"] = dict(calls=runs["two_pass"], total_ms_min=min(r["total_ms"] for r in runs["two_pass"]),
                           total_ms_max=max(r["total_ms"] for r in runs["two_pass"]))
    res["direct"] = dict(call_ms=runs["direct"], call_ms_min=min(runs["direct"]), call_ms_max=max(runs["direct"]))
    res["two_pass_over_direct"] = res["two_pass"]["total_ms_min"] / res["direct"]["call_ms_min"]
    res["finite"] = fin
    return res


def time_free_init(frames, hw, loop, sch, dev, dt, iters, rounds=5):
    """Device-event time of ``kernels.free_init_noise`` (three launches; its result and workspace allocated per call) next to the eager
    definition on the GPU, alternated round by round after a warm-up round; min / median / max."""
    from imagine360_amd import pano_geometry as G
    x0 = torch.randn(1, 4, frames, *hw, device=dev).to(dt)
    n1, n2 = (torch.randn(1, frames, 4, *hw, device=dev) for _ in range(2))
    ops = [G.free_init_operator(n, 0.25, per).to(torch.float32).to(dev) for n, per in ((frames, bool(loop)), (hw[0], False), (hw[1], True))]
    sa, sb = sch.noise_coefficients(sch._timesteps_host[0])
    fns = dict(kernel=lambda: kernels.free_init_noise(x0, n1, n2, *ops, sa, sb), eager=lambda: G.free_init_noise(x0, n1, n2, sa, sb, *ops))
    times = {k: [] for k in fns}
    for r in range(rounds + 1):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(a.elapsed_time(b) / iters * 1e3)
    n = n1.numel()
    out = {k: dict(us_min=min(v), us_median=statistics.median(v), us_max=max(v)) for k, v in times.items()}
    out.update(tensor=list(n1.shape), ring=bool(loop), sa=sa, sb=sb, fma_per_call=n * (frames + hw[0] + hw[1]),
               max_abs_diff_vs_eager=float((fns["kernel"]() - fns["eager"]()).abs().max()),
               note="three launches; the working set (2 MB per fp32 tensor at cfg2) is cache-resident")
    return out


def free_init_bench(args, sch, dev, dt):
    """--free-init N: whole pipeline calls (encode, capture, N passes of the loop, decode of the last) next to the plain call; host clock
    around a call that ends in a device synchronise."""
    import random

    from imagine360_amd.pipeline import AnimationPipeline
    frames, n = args.frames, args.free_init
    assert n >= 2, "--free-init N counts the passes in total: N >= 2"
    res = dict(tool="bench_context --free-init", free_init_iters=n, frames=frames, num_inference_steps=args.num_steps, pano_hw=PANO_HW,
               dtype="bfloat16", device=torch.cuda.get_device_name(0), sampler=args.sampler)
    sch.set_timesteps(args.num_steps)
    res["free_init_noise"] = time_free_init(frames, PANO_HW, args.loop, sch, dev, dt, args.kernel_iters)
    if args.kernel_only:
        return res
    mv = configs.build_mv_model(1, device=dev, dtype=dt, xformers=True)
    mv.dual_stream, mv.warp_streams = True, True
    vae = configs.build_vae(1, device=dev, dtype=dt)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, type(sch)(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
    pipe._no_progress = True
    vb = synthetic.video_batch(frames=frames, pano_hw=(PANO_HW[0] * 8, PANO_HW[1] * 8), seed=1)
    cond = synthetic.conditioning(frames=max(frames, 16), seed=1)
    windows = dict(context_frames=LENGTH, context_overlap=OVERLAP, context_loop=args.loop) if frames > LENGTH else {}
    res["windows"] = windows

    def call(**kw):
        torch.manual_seed(21)
        random.seed(21)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vid = pipe("synthetic", num_inference_steps=args.num_steps, guidance_scale_text=7.5, negative_prompt="", latents_dtype=dt,
                   video_batch=vb, use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video",
                   prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **windows, **kw).videos
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, bool(torch.isfinite(vid).all())

    res["warm_up"] = dict(plain_ms=call()[0], free_init_ms=call(free_init_iters=n)[0])
    print("warm-up done", file=sys.stderr, flush=True)
    runs, fin = dict(plain=[], free_init=[]), True
    for _ in range(args.rounds):
        for k, kw in (("plain", {}), ("free_init", dict(free_init_iters=n))):
            ms, ok = call(**kw)
            runs[k].append(ms)
            fin = fin and ok
    res["plain"] = dict(call_ms=runs["plain"], call_ms_min=min(runs["plain"]))
    res["free_init"] = dict(call_ms=runs["free_init"], call_ms_min=min(runs["free_init"]))
    res["ms_per_extra_pass"] = (res["free_init"]["call_ms_min"] - res["plain"]["call_ms_min"]) / (n - 1)
    res["finite"] = fin
    return res


def interval_bench(args, sch, dev, dt, ts_host):
    """--guidance-interval LO HI at cfg2 size (16 frames, 512 x 1024, bf16): one captured step object whose run of 25 steps holds both
    kinds of step (two graphs over the same static buffers), next to one without the interval (one graph).  ms per guided and per
    unguided step (replays of the two graphs interleaved round by round in this one process), ms per step of the 25-step run with and
    without the interval, and the peak device memory behind one graph and behind two."""
    from imagine360_amd.graph_step import GraphedDenoiseStep
    frames = 16
    interval = tuple(args.guidance_interval)
    flags = sch.guided_steps(ts_host, interval)
    assert True in flags and False in flags, f"--guidance-interval {interval}: the 25-step run must hold both kinds of step to compare them"
    res = dict(tool="bench_context --guidance-interval", guidance_interval=list(interval), frames=frames, pano_hw=PANO_HW, pers_hw=PERS_HW,
               dtype="bfloat16", device=torch.cuda.get_device_name(0), sampler=args.sampler, steps_of_25=dict(guided=sum(flags), unguided=len(flags) - sum(flags)))
    mv = configs.build_mv_model(1, device=dev, dtype=dt, xformers=True)
    mv.dual_stream, mv.warp_streams = True, True
    inp = synthetic.mv_inputs(frames=frames, pano_hw=PANO_HW, pers_hw=PERS_HW, seed=1, dtype=dt, device=dev)
    inp.pop("timestep")
    cams = synthetic.icosahedron_cameras(90, PERS_PX, device=dev)
    pano_lat, pers_lat = inp["pano_latent"][:1, :4].contiguous(), inp["latents"][:1, :, :4].contiguous()
    mib = lambda: torch.cuda.max_memory_allocated() / 2 ** 20
    torch.cuda.reset_peak_memory_stats()
    one = GraphedDenoiseStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, warmup=1)
    torch.cuda.synchronize()
    res["peak_mib_one_graph"] = mib()
    with ip_cache_slots(mv, 2):
        two = GraphedDenoiseStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, warmup=1, guidance_interval=interval, steps=ts_host)
        torch.cuda.synchronize()
        res["peak_mib_two_graphs"] = mib()                  # (the one-graph object is still alive: the peak behind all three graphs)
        assert len(two.graphs) == 2
        t_guided, t_unguided = ts_host[flags.index(True)], ts_host[flags.index(False)]
        kinds = dict(guided_step=[t_guided], unguided_step=[t_unguided])
        res.update(time_steps({k: two for k in kinds}, None, args.steps, args.rounds, per_name=kinds))
        res.update(time_steps(dict(run_without_interval=one, run_with_interval=two), ts_host, len(ts_host), args.rounds))
        res["finite"] = bool(torch.isfinite(two.pano_lat.float()).all() and torch.isfinite(two.pers_lat.float()).all())
    res["unguided_over_guided"] = res["unguided_step"]["ms_min"] / res["guided_step"]["ms_min"]
    res["note"] = ("randomly initialised weights: what the interval does to a clip's quality can only be judged with trained weights; "
                   "host-clock ms around replays that end in a device synchronise")
    return res


def apg_bench(args, sch, dev, dt, ts_host):
    """--apg ETA [R] at cfg2 size (16 frames, 512 x 1024, bf16): the captured step with adaptive projected guidance (a statistics launch
    and a step launch per branch), next to the plain captured step and the one with guidance_rescale = 0.7 (the same two-launch scheme),
    replays alternated round by round.  The six-coefficient step kernel serves all three (eta = 0 without either option runs
    ``cfg_ddim_update``: the shipped default, timed as `plain_step`).  ``--apg-momentum BETA`` adds the captured step with the momentum
    of the projected guidance (an fp32 state per branch and an uploaded carry) to the same alternated rounds."""
    from imagine360_amd.graph_step import GraphedDenoiseStep
    frames = 16
    apg = (float(args.apg[0]), float(args.apg[1]) if len(args.apg) > 1 else None)
    assert len(args.apg) <= 2, "--apg ETA [R]"
    res = dict(tool="bench_context --apg", apg_eta=apg[0], apg_threshold=apg[1], frames=frames, pano_hw=PANO_HW, pers_hw=PERS_HW, dtype="bfloat16",
               device=torch.cuda.get_device_name(0), sampler=args.sampler)
    mv = configs.build_mv_model(1, device=dev, dtype=dt, xformers=True)
    mv.dual_stream, mv.warp_streams = True, True
    inp = synthetic.mv_inputs(frames=frames, pano_hw=PANO_HW, pers_hw=PERS_HW, seed=1, dtype=dt, device=dev)
    inp.pop("timestep")
    cams = synthetic.icosahedron_cameras(90, PERS_PX, device=dev)
    pano_lat, pers_lat = inp["pano_latent"][:1, :4].contiguous(), inp["latents"][:1, :, :4].contiguous()
    graphs = dict(plain_step=GraphedDenoiseStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, warmup=1),
                  rescale_step=GraphedDenoiseStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, warmup=1, guidance_rescale=0.7),
                  apg_step=GraphedDenoiseStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, warmup=1, guidance_apg=apg))
    if args.apg_momentum is not None:
        graphs["apg_momentum_step"] = GraphedDenoiseStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, warmup=1, guidance_apg=apg,
                                                         guidance_apg_momentum=args.apg_momentum)
        res["apg_momentum"] = args.apg_momentum
    torch.cuda.synchronize()
    res.update(time_steps(graphs, ts_host, args.steps, args.rounds))
    res["finite"] = all(bool(torch.isfinite(g.pano_lat.float()).all() and torch.isfinite(g.pers_lat.float()).all()) for g in graphs.values())
    res["apg_over_plain"] = res["apg_step"]["ms_median"] / res["plain_step"]["ms_median"]
    res["apg_over_rescale"] = res["apg_step"]["ms_median"] / res["rescale_step"]["ms_median"]
    if args.apg_momentum is not None:
        res["apg_momentum_over_apg"] = res["apg_momentum_step"]["ms_median"] / res["apg_step"]["ms_median"]
        res["apg_momentum_over_apg_min"] = res["apg_momentum_step"]["ms_min"] / res["apg_step"]["ms_min"]
    res["note"] = ("randomly initialised weights: what APG does to a clip's look can only be judged with trained weights; host-clock ms around "
                   "replays that end in a device synchronise")
    return res


def hires_bench(args, sch, dev, dt):
    """--init-scale N: the two-pass run (1 / N of the size from pure noise, then the full size from its latent at --strength) next to one
    run from pure noise at the full size; whole pipeline calls (encode, loop, decode), host clock around a call that ends in a device
    synchronise."""
    import random

    from imagine360_amd.pipeline import AnimationPipeline
    n, frames, big = args.init_scale, args.frames, tuple(args.pano_hw)
    assert big[0] % n == 0 and big[1] % n == 0, f"--pano-hw {big} is not a multiple of --init-scale {n}"
    small = (big[0] // n, big[1] // n)
    res = dict(tool="bench_context --init-scale", init_scale=n, strength=args.strength, frames=frames, num_inference_steps=args.num_steps,
               pano_hw=list(big), first_pass_pano_hw=list(small), dtype="bfloat16", device=torch.cuda.get_device_name(0))
    res["resize_pano_latent"] = time_resize(small, big, frames, dev, dt, args.kernel_iters)
    if args.kernel_only:
        return res
    mv = configs.build_mv_model(1, device=dev, dtype=dt, xformers=True)
    mv.dual_stream, mv.warp_streams = True, True
    vae = configs.build_vae(1, device=dev, dtype=dt)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, type(sch)(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
    pipe._no_progress = True
    vbs = {hw: synthetic.video_batch(frames=frames, pano_hw=(hw[0] * 8, hw[1] * 8), seed=1) for hw in (small, big)}
    cond = synthetic.conditioning(frames=max(frames, 16), seed=1)
    windows = dict(context_frames=LENGTH, context_overlap=OVERLAP, context_loop=args.loop) if frames > LENGTH else {}
    res["windows"] = windows

    def call(hw, **kw):
        torch.manual_seed(21)
        random.seed(21)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vid = pipe("synthetic", num_inference_steps=args.num_steps, guidance_scale_text=7.5, negative_prompt="", latents_dtype=dt,
                   video_batch=vbs[hw], use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video",
                   prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **windows, **kw).videos
        torch.cuda.synchronize()
        assert tuple(vid.shape[-2:]) == (hw[0] * 8, hw[1] * 8)
        return (time.perf_counter() - t0) * 1e3, bool(torch.isfinite(vid).all())

    def two_pass():
        a, ok_a = call(small)
        b, ok_b = call(big, init_latents=pipe.last_latents[0], strength=args.strength)
        return dict(first_pass_ms=a, second_pass_ms=b, total_ms=a + b), ok_a and ok_b

    sch.set_timesteps(args.num_steps)
    res["steps"] = dict(first_pass=args.num_steps, second_pass=len(sch.timesteps_for_strength(args.strength)[1]), direct=args.num_steps)
    warm, fin = two_pass()                                  # warms every shape of both sizes up
    res["warm_up"] = dict(two_pass=warm, direct_ms=call(big)[0])
    print("warm-up done", file=sys.stderr, flush=True)
    runs = dict(two_pass=[], direct=[])
    for _ in range(args.rounds):
        t, ok = two_pass()
        runs["two_pass"].append(t)
        ms, ok2 = call(big)
        runs["direct"].append(ms)
        fin = fin and ok and ok2
    res["two_pass"] = dict(calls=runs["two_pass"], total_ms_min=min(r["total_ms"] for r in runs["two_pass"]),
                           total_ms_max=max(r["total_ms"] for r in runs["two_pass"]))
    res["direct"] = dict(call_ms=runs["direct"], call_ms_min=min(runs["direct"]), call_ms_max=max(runs["direct"]))
    res["two_pass_over_direct"] = res["two_pass"]["total_ms_min"] / res["direct"]["call_ms_min"]
    res["finite"] = fin
    return res


def strength_bench(args, sch, dev, dt):
    """--strength S: whole pipeline calls from pure noise and from the first call's latent at strength S."""
    import random

    from imagine360_amd.pipeline import AnimationPipeline
    frames = args.frames
    res = dict(tool="bench_context --strength", strength=args.strength, frames=frames, num_inference_steps=args.num_steps,
               pano_hw=PANO_HW, pers_hw=PERS_HW, dtype="bfloat16", device=torch.cuda.get_device_name(0))
    res["noise_latents"] = time_noise_latents(sch, frames, dev, dt, args.kernel_iters)
    if args.regenerate_mask:
        res["regenerate_mask"] = args.regenerate_mask
        res["keep_latents"] = time_keep_latents(sch, frames, dev, dt, args.kernel_iters)
    if args.kernel_only:
        return res
    mv = configs.build_mv_model(1, device=dev, dtype=dt, xformers=True)
    mv.dual_stream, mv.warp_streams = True, True
    vae = configs.build_vae(1, device=dev, dtype=dt)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, type(sch)(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
    pipe._no_progress = True
    vb = synthetic.video_batch(frames=frames, pano_hw=(PANO_HW[0] * 8, PANO_HW[1] * 8), seed=1)
    cond = synthetic.conditioning(frames=max(frames, 16), seed=1)
    windows = dict(context_frames=LENGTH, context_overlap=OVERLAP, context_loop=args.loop) if frames > LENGTH else {}
    res["windows"] = windows

    def call(**kw):
        torch.manual_seed(21)
        random.seed(21)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vid = pipe("synthetic", num_inference_steps=args.num_steps, guidance_scale_text=7.5, negative_prompt="", latents_dtype=dt,
                   video_batch=vb, use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video",
                   prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]), **windows, **kw).videos
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, bool(torch.isfinite(vid).all())

    res["first_call_ms"], fin = call()                       # warms every shape up; its latent is the init of the refinement passes
    x0 = pipe.last_latents[0].clone()
    print("first call done", file=sys.stderr, flush=True)
    sch.set_timesteps(args.num_steps)
    steps = dict(from_noise=args.num_steps, refine=len(sch.timesteps_for_strength(args.strength)[1]))
    if args.regenerate_mask:
        return masked_refinement(args, res, call, x0, steps["refine"], half_mask(frames, PANO_HW[0] * 8, PANO_HW[1] * 8), fin)
    times = dict(from_noise=[], refine=[])
    for _ in range(args.rounds):
        for name, kw in (("from_noise", {}), ("refine", dict(init_latents=x0, strength=args.strength))):
            ms, ok = call(**kw)
            times[name].append(ms)
            fin = fin and ok
    for k, v in times.items():
        res[k] = dict(call_ms=v, call_ms_min=min(v), steps=steps[k])
    res["ms_per_skipped_step"] = (res["from_noise"]["call_ms_min"] - res["refine"]["call_ms_min"]) / max(steps["from_noise"] - steps["refine"], 1)
    res["refine_over_from_noise"] = res["refine"]["call_ms_min"] / res["from_noise"]["call_ms_min"]
    res["finite"] = fin
    return res


def masked_refinement(args, res, call, x0, steps, mask, fin):
    """--regenerate-mask: the refinement call with the mask next to the same call without it, alternated.  "feather": the half mask
    feathered by 20 degrees on the sphere (``regenerate_feather``: one ``sphere_distance2`` launch per call) and run in release mode."""
    times = dict(refine=[], refine_masked=[])
    init = dict(init_latents=x0, strength=args.strength)
    soft = dict(regenerate_feather=20.0, regenerate_mode="release") if args.regenerate_mask == "feather" else {}
    res["regenerate_keywords"] = soft
    for _ in range(args.rounds + 1):                       # (round 0 warms the masked call's shapes up)
        for name, kw in (("refine", init), ("refine_masked", dict(regenerate_mask=mask, **soft, **init))):
            ms, ok = call(**kw)
            times[name].append(ms)
            fin = fin and ok
    for k, v in times.items():
        res[k] = dict(call_ms=v[1:], call_ms_min=min(v[1:]), call_ms_median=statistics.median(v[1:]), steps=steps)
    res["masked_minus_plain_ms_per_step"] = (res["refine_masked"]["call_ms_min"] - res["refine"]["call_ms_min"]) / steps
    res["masked_over_plain"] = res["refine_masked"]["call_ms_min"] / res["refine"]["call_ms_min"]
    # (an upper bound of the share of a step: the call time per step also holds the encode, the graph capture and the decode)
    res["keep_latents_share_of_call_time_per_step"] = res["keep_latents"]["kernel"]["us_min"] * 1e-3 / (res["refine"]["call_ms_min"] / steps)
    res["finite"] = fin
    return res


def level_bench(args, sch, dev, dt, ts_host):
    """--context-level: the captured step of one clip under the same window plan at the two levels -- whole-model windows
    (GraphedWindowedStep: one forward per window, the predictions blended in the step kernel) and windows inside the motion modules'
    attention (``mv.set_temporal_windows`` + the plain GraphedDenoiseStep: one forward of all frames) -- replays alternated round by
    round, host clock around work that ends in a device synchronise.  The frame evaluations per step stand next to the times."""
    from imagine360_amd.graph_step import GraphedDenoiseStep, GraphedWindowedStep
    frames = args.frames
    assert args.context_frames < frames <= 64, "--context-level: a clip of at most 64 frames, longer than its windows"
    plan = WindowPlan(frames, args.context_frames, args.context_overlap, "pyramid", dev, loop=args.loop)
    levels = ["model", "attention"] if args.context_level == "both" else [args.context_level]
    res = dict(tool="bench_context --context-level", level=args.context_level, frames=frames, context_frames=plan.length,
               context_overlap=args.context_overlap, loop=bool(args.loop), windows=plan.starts, pano_hw=PANO_HW, pers_hw=PERS_HW, dtype="bfloat16",
               device=torch.cuda.get_device_name(0), sampler=args.sampler,
               frame_evaluations_per_step=dict(model=len(plan) * plan.length, attention=frames))
    mv = configs.build_mv_model(1, device=dev, dtype=dt, xformers=True)
    mv.dual_stream, mv.warp_streams = True, True
    inp = synthetic.mv_inputs(frames=frames, pano_hw=PANO_HW, pers_hw=PERS_HW, seed=1, dtype=dt, device=dev)
    inp.pop("timestep")
    cams = synthetic.icosahedron_cameras(90, PERS_PX, device=dev)
    pano_lat, pers_lat = inp["pano_latent"][:1, :4].contiguous(), inp["latents"][:1, :, :4].contiguous()
    graphs = {}
    if "model" in levels:
        with ip_cache_slots(mv, len(plan)):
            graphs["model_level_step"] = GraphedWindowedStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, plan, warmup=1)
        torch.cuda.synchronize()
        print("captured: whole-model windows", file=sys.stderr, flush=True)
    if "attention" in levels:
        mv.set_temporal_windows(plan)
        try:
            graphs["attention_level_step"] = GraphedDenoiseStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, warmup=1)
        finally:
            mv.set_temporal_windows(None)            # (the captured launches keep the tables they were made with)
        torch.cuda.synchronize()
        print("captured: windows inside the temporal attention", file=sys.stderr, flush=True)
    res.update(time_steps(graphs, ts_host, args.steps, args.rounds))
    res["finite"] = all(bool(torch.isfinite(g.pano_lat.float()).all() and torch.isfinite(g.pers_lat.float()).all()) for g in graphs.values())
    if len(graphs) == 2:
        res["attention_over_model"] = res["attention_level_step"]["ms_median"] / res["model_level_step"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--loop", action="store_true", help="the ring plan of a looping clip against the linear plan")
    ap.add_argument("--passes", type=int, default=2, help="--loop: identical passes of every measurement")
    ap.add_argument("--strength", type=float, default=None, help="the refinement pass: pipeline calls with init_latents at this strength next to calls from pure noise")
    ap.add_argument("--frames", type=int, default=FRAMES, help="--strength: frames of the clip (context windows above 16)")
    ap.add_argument("--num-steps", type=int, default=6, help="--strength: num_inference_steps of every call")
    ap.add_argument("--regenerate-mask", choices=["half", "feather"], default=None,
                    help="--strength: keep part of the clip (pipeline regenerate_mask) and time that call next to the call without the mask; "
                         "feather: the half mask with regenerate_feather=20 in regenerate_mode='release'")
    ap.add_argument("--init-scale", type=int, default=None,
                    help="with --strength: the hi-res pass -- a first call at 1/N of --pano-hw, a second call at --pano-hw from its latent -- next to one call from pure noise at --pano-hw")
    ap.add_argument("--init-frames", type=int, default=None,
                    help="with --strength: the frame-interpolation pass -- a first call with this many frames, a second call with --frames frames from its latent -- next to one call from pure noise with --frames frames")
    ap.add_argument("--free-init", type=int, default=None,
                    help="FreeInit: pipeline calls with free_init_iters = N next to the plain call (--frames, --num-steps, --loop), and the filter kernel against its eager definition")
    ap.add_argument("--guidance-interval", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="guided and unguided captured steps of one 25-step run at cfg2 size, interleaved (--steps replays per round, --rounds)")
    ap.add_argument("--apg", type=float, nargs="+", default=None, metavar="ETA [R]",
                    help="the captured cfg2 step with adaptive projected guidance (apg_eta ETA, apg_threshold R; no R: no clamp) next to the plain "
                         "and the guidance-rescale step, interleaved (--steps replays per round, --rounds)")
    ap.add_argument("--apg-momentum", type=float, default=None, metavar="BETA",
                    help="with --apg: the captured step with the momentum of the projected guidance (apg_momentum BETA) in the same rounds")
    ap.add_argument("--pano-hw", type=int, nargs=2, default=[128, 256], metavar=("H", "W"), help="--init-scale: latent size of the full-size run (default: cfg5)")
    ap.add_argument("--sampler", choices=["ddim", "dpmpp2m"], default="ddim", help="the scheduler of every step and call (dpmpp2m: DPM-Solver++ 2M)")
    ap.add_argument("--context-level", choices=["model", "attention", "both"], default=None,
                    help="one captured step of a clip of --frames frames (<= 64) under windows of --context-frames with --context-overlap: whole-model "
                         "windows (model), windows inside the motion modules' attention (attention), or both alternated round by round")
    ap.add_argument("--context-frames", type=int, default=LENGTH, help="--context-level: frames per window")
    ap.add_argument("--context-overlap", type=int, default=OVERLAP, help="--context-level: frames two neighbouring windows share")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_context.py measures on the MI355X; there is nothing to time without one"
    torch.set_grad_enabled(False)
    kernels.lib()
    dev, dt = torch.device("cuda", 0), torch.bfloat16
    sch = (DPMSolverMultistepScheduler if args.sampler == "dpmpp2m" else DDIMScheduler)(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    ts_host = [int(t) for t in sch._timesteps_host]
    if args.context_level is not None:
        return emit(level_bench(args, sch, dev, dt, ts_host), args.out)
    if args.apg is not None:
        return emit(apg_bench(args, sch, dev, dt, ts_host), args.out)
    if args.guidance_interval is not None:
        return emit(interval_bench(args, sch, dev, dt, ts_host), args.out)
    if args.free_init is not None:
        assert args.strength is None and args.init_scale is None and args.init_frames is None, "--free-init N goes alone (FreeInit starts from pure noise)"
        return emit(free_init_bench(args, sch, dev, dt), args.out)
    if args.init_frames is not None:
        assert args.strength is not None and args.init_scale is None, "--init-frames f goes with --strength (and not with --init-scale)"
        return emit(retime_bench(args, sch, dev, dt), args.out)
    if args.init_scale is not None:
        assert args.strength is not None and args.init_scale >= 1, "--init-scale N (>= 1) goes with --strength"
        return emit(hires_bench(args, sch, dev, dt), args.out)
    if args.strength is not None:
        return emit(strength_bench(args, sch, dev, dt), args.out)
    if args.loop:
        return emit(loop_bench(args, sch, dev, dt, ts_host), args.out)
    plan = WindowPlan(FRAMES, LENGTH, OVERLAP, "pyramid", dev)
    res = dict(tool="bench_context", frames=FRAMES, context_frames=LENGTH, context_overlap=OVERLAP, windows=plan.starts,
               pano_hw=PANO_HW, pers_hw=PERS_HW, dtype="bfloat16", device=torch.cuda.get_device_name(0), sampler=args.sampler)

    pers = torch.randn(1, 20, 4, FRAMES, *PERS_HW, device=dev).to(dt)
    nbytes = kernel_bytes(pers, plan)
    kt = time_kernels(sch, plan, pers, args.kernel_iters)
    res["blend_kernel"] = {k: dict(**kt[k], bytes=nbytes[k], gb_per_s=nbytes[k] / (kt[k]["us_min"] * 1e-6) / 1e9) for k in kt}
    res["blend_kernel"]["tensor"] = list(pers.shape)
    res["blend_kernel"]["note"] = "event time over back-to-back launches; the working set fits the 256 MB Infinity Cache, so GB/s is an effective rate"

    if not args.kernel_only:
        mv = configs.build_mv_model(1, device=dev, dtype=dt, xformers=True)
        mv.dual_stream, mv.warp_streams = True, True
        inp = synthetic.mv_inputs(frames=FRAMES, pano_hw=PANO_HW, pers_hw=PERS_HW, seed=1, dtype=dt, device=dev)
        inp.pop("timestep")
        cams = synthetic.icosahedron_cameras(90, PERS_PX, device=dev)
        pano_lat, pers_lat = inp["pano_latent"][:1, :4].contiguous(), inp["latents"][:1, :, :4].contiguous()
        from imagine360_amd.graph_step import GraphedDenoiseStep, GraphedWindowedStep
        with ip_cache_slots(mv, len(plan)):
            windowed = GraphedWindowedStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, plan, warmup=1)
        torch.cuda.synchronize()
        print("captured: windowed step", file=sys.stderr, flush=True)
        full = GraphedDenoiseStep(mv, sch, inp, cams, pano_lat, pers_lat, 7.5, warmup=1)
        torch.cuda.synchronize()
        print("captured: 48-frame full-attention step", file=sys.stderr, flush=True)
        graphs = dict(windowed_step=windowed, full_attention_step=full)
        res.update(time_steps(graphs, ts_host, args.steps, args.rounds))
        res["finite"] = bool(torch.isfinite(windowed.pano_lat.float()).all() and torch.isfinite(windowed.pers_lat.float()).all())
    emit(res, args.out)


def emit(res, out):
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
