"""Looping clips on the MI355X: the ring entry points of the windows kernels (wrap = F) against the fp64 restatement, their bit-level
guarantees (non-wrapping tables are the linear entry points; rolling the clip rolls the result), the ring statistics pass + rescaled
step, the argument checks; then the pipeline's ``context_loop`` keyword against a hand-written loop on the kernels, captured steps
against eager ones, and one looping windowed step against the fp32 oracle."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import record as _record, rel  # noqa: E402
from imagine360_amd import configs, kernels as K, synthetic as S  # noqa: E402
from imagine360_amd.context import WindowPlan, context_weights, context_windows, ip_cache_slots  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler  # noqa: E402
from test_context_loop import hand_written_ring_loop, host_factor, host_ring_blends, host_step_on, ring_cut  # noqa: E402
from test_context_windows import TOL, capture_loop_inputs, windows_case  # noqa: E402
from test_context_windows_gpu import _run, gpu_pipe  # noqa: E402,F401
from test_guidance_rescale_gpu import FACTOR_TOL  # noqa: E402

torch.set_grad_enabled(False)
G = 7.5

# (sample shape, L, starts)
RING_CASES = [((1, 4, 12, 4, 8), 8, [0, 6]),                        # 16-byte lanes; window 1 wraps
              ((1, 3, 4, 12, 3, 5), 8, [0, 4, 8]),                  # scalar path, inner 15
              ((1, 4, 20, 6, 4), 8, [0, 3, 6, 9, 12, 15, 18]),      # context_windows(20, 8, 5, loop=True): two wrapping windows
              ((1, 4, 9, 5, 7), 8, [0, 7])]                         # inner 35; 1260 elements: the statistics pass ends in a short group
MODES = [pred | extra for pred in (0, 1, 2) for extra in (0, 4, 8, 12)]


def _sched():
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    return sch, sch._timesteps_host[8]


def _bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _dev_starts(starts):
    return torch.tensor(starts, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_ring_kernel_all_modes_vs_fp64(dt):
    sch, t = _sched()
    assert context_windows(20, 8, 5, loop=True) == RING_CASES[2][2]
    errs = {}
    for ci, (shape, L, starts) in enumerate(RING_CASES):
        preds, x, z = windows_case(shape, L, starts, dt, seed=260 + ci)
        dp, dx, dz, st = preds.cuda(), x.cuda(), z.cuda(), _dev_starts(starts)
        for kind in ("uniform", "pyramid"):
            w = context_weights(L, kind)
            dw = w.cuda()
            m, _ = host_ring_blends(preds, x, starts, w, G)
            for eta in (0.0, 1.0):
                coefs = sch.step_coefficients(t, eta, G)
                coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
                noise, dnoise = (z, dz) if eta > 0 else (None, None)
                for mode in MODES:
                    ref = host_step_on(m, x, noise, mode, coefs)
                    out = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs, ring=True)
                    assert out.dtype == dt and out.shape == x.shape
                    errs[f"case{ci}_{kind}_eta{eta}_mode{mode}"] = e = rel(out, ref)
                    print(f"ring step {dt} case{ci} {kind} eta{eta} mode{mode}: rel {e:.3g}")
                    assert e < TOL[dt], (ci, kind, eta, mode, e)
                    out2 = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, (0.0,) * 6, coef_dev=coef_dev, ring=True)
                    assert _bits(out2, out), (ci, kind, eta, mode)
    _record(f"cfg_ddim_step_windows_ring_{str(dt).split('.')[-1]}", max_rel=max(errs.values()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_non_wrapping_tables_are_the_linear_entry_points_bit_for_bit(dt):
    """Starts [0, 4] on the first shape: j = f - start[k] is never lifted by F into [0, L), so the ring entry points are the
    linear ones -- step, rescaled step and the factor."""
    sch, t = _sched()
    shape, L, _ = RING_CASES[0]
    starts = [0, 4]
    preds, x, z = windows_case(shape, L, starts, dt, seed=270)
    dp, dx, dz, st = preds.cuda(), x.cuda(), z.cuda(), _dev_starts(starts)
    for kind in ("uniform", "pyramid"):
        dw = context_weights(L, kind).cuda()
        assert torch.equal(K.cfg_rescale_factor_windows(dp, dx, st, dw, G, 0.7, ring=True), K.cfg_rescale_factor_windows(dp, dx, st, dw, G, 0.7))
        for eta in (0.0, 1.0):
            coefs = sch.step_coefficients(t, eta, G)
            coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
            noise = dz if eta > 0 else None
            for mode in MODES:
                for kw in ({}, dict(rescale=0.7), dict(coef_dev=coef_dev), dict(coef_dev=coef_dev, rescale=0.7)):
                    a = K.cfg_ddim_step_windows(dp, dx, noise, st, dw, mode, coefs, ring=True, **kw)
                    b = K.cfg_ddim_step_windows(dp, dx, noise, st, dw, mode, coefs, **kw)
                    assert _bits(a, b), (kind, eta, mode, kw.keys())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("r", [1, 5, 11])
def test_rolling_the_clip_rolls_the_result_bit_for_bit(dt, r):
    """x and the noise rolled by r frames, the starts replaced by (s + r) mod F, slots unchanged: every frame sees the same windows at
    the same positions in the same order, so the output is the rolled output."""
    sch, t = _sched()
    shape, L, starts = RING_CASES[0]
    F, fd = shape[2], 2
    preds, x, z = windows_case(shape, L, starts, dt, seed=280)
    dp, dx, dz = preds.cuda(), x.cuda(), z.cuda()
    rolled = [(s + r) % F for s in starts]
    for kind in ("uniform", "pyramid"):
        dw = context_weights(L, kind).cuda()
        for eta in (0.0, 1.0):
            coefs = sch.step_coefficients(t, eta, G)
            for mode in MODES:
                base = K.cfg_ddim_step_windows(dp, dx, dz if eta > 0 else None, _dev_starts(starts), dw, mode, coefs, ring=True)
                out = K.cfg_ddim_step_windows(dp, dx.roll(r, fd).contiguous(), dz.roll(r, fd).contiguous() if eta > 0 else None,
                                              _dev_starts(rolled), dw, mode, coefs, ring=True)
                assert _bits(out, base.roll(r, fd).contiguous()), (kind, eta, mode, rolled)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_ring_statistics_and_rescaled_step_vs_fp64(dt):
    sch, t = _sched()
    errs, ferrs = {}, {}
    for ci, (shape, L, starts) in enumerate(RING_CASES):
        preds, x, z = windows_case(shape, L, starts, dt, seed=290 + ci)
        dp, dx, dz, st = preds.cuda(), x.cuda(), z.cuda(), _dev_starts(starts)
        for kind in ("uniform", "pyramid"):
            w = context_weights(L, kind)
            dw = w.cuda()
            m, cb = host_ring_blends(preds, x, starts, w, G)
            want = host_factor(m, cb, 0.7)
            r = K.cfg_rescale_factor_windows(dp, dx, st, dw, G, 0.7, ring=True)
            assert r.dtype == torch.float32 and r.shape == () and r.is_cuda
            ferrs[f"case{ci}_{kind}"] = fe = abs(float(r) / want - 1.0)
            print(f"ring factor {dt} case{ci} {kind}: r = {float(r):.9g}, fp64 {want:.12g}, rel err {fe:.3g}")
            assert fe <= FACTOR_TOL, (ci, kind, fe)
            coef_g = torch.tensor([G, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
            assert torch.equal(K.cfg_rescale_factor_windows(dp, dx, st, dw, 0.0, 0.7, coef_dev=coef_g, ring=True), r)
            mr = m * want
            for eta in (0.0, 1.0):
                coefs = sch.step_coefficients(t, eta, G)
                coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
                noise, dnoise = (z, dz) if eta > 0 else (None, None)
                for mode in MODES:
                    ref = host_step_on(mr, x, noise, mode, coefs)
                    out = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs, rescale=0.7, ring=True)
                    assert out.dtype == dt and out.shape == x.shape
                    errs[f"case{ci}_{kind}_eta{eta}_mode{mode}"] = e = rel(out, ref)
                    print(f"ring rescaled step {dt} case{ci} {kind} eta{eta} mode{mode}: rel {e:.3g}")
                    assert e < TOL[dt], (ci, kind, eta, mode, e)
                    out2 = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, (0.0,) * 6, coef_dev=coef_dev, rescale=0.7, ring=True)
                    assert _bits(out2, out), (ci, kind, eta, mode)
            plain = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs, ring=True)
            assert _bits(K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs, rescale=0.0, ring=True), plain)
            assert rel(out, plain.float().cpu()) > 1e-3                         # the factor is used
    _record(f"cfg_ddim_step_windows_ring_rescale_{str(dt).split('.')[-1]}", max_rel=max(errs.values()), factor_rel_err=max(ferrs.values()))


def test_ring_entry_points_reject_bad_arguments():
    x = torch.zeros(1, 4, 4, 2, 8, dtype=torch.bfloat16, device="cuda")
    pr = torch.zeros(2, 2, 4, 2, 2, 8, dtype=torch.bfloat16, device="cuda")
    st, w = torch.tensor([0, 2], dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    ws = torch.zeros(K.RESCALE_RECORD, dtype=torch.float32, device="cuda")
    coefs = (7.5, 0.5, 0.8, 0.6, 0.7, 0.1)
    with pytest.raises(ValueError, match="noise"):
        K.cfg_ddim_step_windows(pr, x, None, st, w, 1, coefs, ring=True)
    with pytest.raises(RuntimeError, match="cfg_ddim_step_windows_ring: mode 3 unsupported"):
        K.cfg_ddim_step_windows(pr, x, x, st, w, 3, coefs, ring=True)
    with pytest.raises(RuntimeError, match="cfg_ddim_step_windows_ring_rescale: rescale=.* must be finite"):
        K.cfg_ddim_step_windows(pr, x, x, st, w, 1, coefs, rescale=float("nan"), ring=True)
    with pytest.raises(AssertionError):
        K.cfg_ddim_step_windows(pr, x, x, st.long(), w, 1, coefs, ring=True)
    lib, p, q, s_, w_, v = K.lib(), pr.data_ptr(), x.data_ptr(), st.data_ptr(), w.data_ptr(), ws.data_ptr()
    err = lambda: lib.im360_last_error()
    step = lambda *a: lib.im360_cfg_ddim_step_windows_ring(*a, None, None)
    resc = lambda *a, phi=0.7, wsp=v: lib.im360_cfg_ddim_step_windows_ring_rescale(*a[:-1], phi, wsp, 8, a[-1], None, None)
    for fn, name in ((step, b"cfg_ddim_step_windows_ring: "), (resc, b"cfg_ddim_step_windows_ring_rescale: ")):
        for null in range(6):
            if null == 2:
                continue                                                      # (a null noise is the zero noise; refused below with sigma > 0)
            ptrs = [p, q, q, q, s_, w_]
            ptrs[null] = None
            assert fn(*ptrs, 2, 4, 4, 2, 16, *coefs, 1, 0) != 0 and err() == name + b"null pointer", (name, null, err())
        assert fn(p, q, q, q, s_, w_, 2, 4, 4, 5, 16, *coefs, 1, 0) != 0 and err().startswith(name) and b"out of range" in err()        # L > F
        assert fn(p, q, q, q, s_, w_, 2, 4, 4, 2, 16, *coefs, 3, 0) != 0 and err() == name + b"mode 3 unsupported"
        assert fn(p, q, q, q, s_, w_, 2, 4, 4, 2, 16, *coefs, 16, 0) != 0 and err() == name + b"mode 16 unsupported"
        assert fn(p, q, None, q, s_, w_, 2, 4, 4, 2, 16, *coefs, 1, 0) != 0 and err().startswith(name) and b"needs a noise tensor" in err()
        assert fn(p, q, q, q, s_, w_, 2, 4, 4, 2, 16, *coefs, 1, 7) != 0 and err() == name + b"dtype 7 unsupported"
    assert resc(p, q, q, q, s_, w_, 2, 4, 4, 2, 16, *coefs, 1, 0, wsp=None) != 0 and b"ring_rescale: null or misaligned workspace" in err()
    assert resc(p, q, q, q, s_, w_, 2, 4 * 256, 4, 2, 16, *coefs, 1, 0) != 0 and b"ring_rescale: workspace of 8 floats" in err()
    assert resc(p, q, q, q, s_, w_, 2, 4, 4, 2, 16, *coefs, 1, 0, phi=float("inf")) != 0 and b"must be finite" in err()
    stats = lambda pp, ss, ww, L=2, wsp=v, dtype=0: lib.im360_cfg_rescale_stats_windows_ring(pp, ss, ww, 2, 4, 4, L, 16, 7.5, wsp, 8, dtype, None, None)
    name = b"cfg_rescale_stats_windows_ring: "
    for ptrs in ((None, s_, w_), (p, None, w_), (p, s_, None)):
        assert stats(*ptrs) != 0 and err() == name + b"null pointer"
    assert stats(p, s_, w_, L=5) != 0 and err().startswith(name) and b"out of range" in err()
    assert stats(p, s_, w_, wsp=None) != 0 and err() == name + b"null or misaligned workspace"
    assert stats(p, s_, w_, dtype=7) != 0 and err() == name + b"dtype 7 unsupported"
    torch.cuda.synchronize()
    assert float(ws.abs().sum()) == 0.0                                        # no statistics pass wrote a record


# ------------------------------------------------------------------------------------------------ pipeline
LOOP = dict(context_frames=16, context_overlap=4, context_loop=True)         # F = 24: windows at 0 and 12, the second one wraps


def test_looping_pipeline_equals_hand_written_loop_on_the_kernels(gpu_pipe):
    """F = 24, L = 16, overlap 4 on a ring, eager, device RNG: bit-identical to cutting the ring by hand (slices, the wrapping window
    as tail + head), calling the model per window in slot order and blending with the ring kernel."""
    pipe = gpu_pipe
    vb = S.video_batch(frames=24, pano_hw=(128, 256), seed=7)
    cond = S.conditioning(frames=24, seed=7)
    st = {}
    capture_loop_inputs(pipe, st)
    try:
        vid, pano, pers = _run(pipe, vb, cond, False, **LOOP)
    finally:
        del pipe._windowed_loop
    assert vid.shape == (1, 3, 24, 128, 256) and torch.isfinite(vid).all()
    assert context_windows(24, 16, 4, loop=True) == [0, 12]
    random.setstate(st["py_rng"])
    torch.cuda.set_rng_state(st["cuda_rng"])
    h_pano, h_pers = hand_written_ring_loop(pipe.mv_base_model, pipe.scheduler, st, [0, 12], 16, context_weights(16, "pyramid"),
                                            K.cfg_ddim_step_windows)
    errs = dict(pano=rel(pano, h_pano), pers=rel(pers, h_pers))
    _record("looping_pipeline_vs_hand_loop", **errs)
    assert torch.equal(pano, h_pano) and torch.equal(pers, h_pers), errs
    # the ring matters: the linear plan of the same arguments from the same seeds is a different clip
    _, line_pano, _ = _run(pipe, vb, cond, False, context_frames=16, context_overlap=4)
    assert rel(pano, line_pano) > 1e-2


@pytest.mark.parametrize("eta,rescale", [(0.0, 0.0), (1.0, 0.0), (0.0, 0.7)], ids=["eta0", "eta1", "rescale"])
def test_graphed_looping_steps_equal_eager_bit_for_bit(gpu_pipe, eta, rescale, monkeypatch):
    from imagine360_amd import graph_step
    replays = []
    orig = graph_step.GraphedWindowedStep.step
    monkeypatch.setattr(graph_step.GraphedWindowedStep, "step", lambda self, t: (replays.append(self.plan.loop), orig(self, t))[1])
    pipe = gpu_pipe
    vb = S.video_batch(frames=24, pano_hw=(128, 256), seed=8)
    cond = S.conditioning(frames=24, seed=8)
    out, states = {}, {}
    for graph in (True, False):
        gen = torch.Generator(device="cuda").manual_seed(77) if eta > 0 else None
        kw = dict(eta=eta, generator=gen) if eta > 0 else {}
        if rescale:
            kw["guidance_rescale"] = rescale
        out[graph] = _run(pipe, vb, cond, graph, steps=2, **LOOP, **kw)
        states[graph] = (random.getstate(), torch.cuda.get_rng_state(), gen.get_state() if gen is not None else None)
    assert replays == [True, True]
    errs = dict(pano=rel(out[True][1], out[False][1]), pers=rel(out[True][2], out[False][2]))
    _record(f"graphed_vs_eager_loop_eta{int(eta)}_rescale{rescale}", **errs)
    assert all(torch.equal(a, b) for a, b in zip(out[True], out[False])), errs
    assert all(torch.isfinite(v.float()).all() for v in out[True])
    assert states[True][0] == states[False][0], "Python RNG (WarpAttn coins)"
    assert torch.equal(states[True][1], states[False][1]), "device RNG (IP-adapter noise)"
    if eta > 0:
        assert torch.equal(states[True][2], states[False][2]), "user generator (variance noise)"


@pytest.mark.parametrize("dt,tol", [(torch.bfloat16, 3e-2), (torch.float16, 4e-3)])
def test_looping_windowed_step_vs_oracle(dt, tol):
    """One looping windowed step (F = 24, L = 16, overlap 4: windows at 0 and 12, the second one frames 12 .. 23, 0 .. 3) of the
    reduced-width model: expected = the fp32 oracle's forward per ring-gathered window, blended and stepped in fp64 here.  The bound
    of test_context_windows_gpu.py::test_windowed_step_vs_oracle: same model, same size."""
    from im360_oracle import mv as OMV
    from im360_oracle.cfg import sd21_unet_cfg
    dev = torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    mv.noise_on_host = True
    F, L = 24, 16
    inp = S.mv_inputs(frames=F, pano_hw=(32, 64), pers_hw=(16, 16), seed=0, sam_frames=F)
    cams = S.icosahedron_cameras(90, 128)
    dinp = S.cast_mv_inputs(inp, dev, dt)
    sch, t = _sched()
    dinp["timestep"] = inp["timestep"] = torch.tensor([t], dtype=torch.int64)
    plan = WindowPlan(F, L, 4, "pyramid", dev, loop=True)
    assert plan.starts == [0, 12] and plan.wraps(1)
    pano_lat, pers_lat = dinp["pano_latent"][:1, :4].contiguous(), dinp["latents"][:1, :, :4].contiguous()
    preds_pers, preds_pano = plan.pred_buffers(pano_lat, pers_lat)
    torch.manual_seed(7)
    random.seed(7)
    with ip_cache_slots(mv, len(plan)):
        plan.forward(mv, dinp, plan.static_inputs(dinp), cams, dinp["timestep"].to(dev), True, preds_pers, preds_pano)
    new_pano = sch.fused_cfg_step_windows(preds_pano, plan.starts_dev, plan.weights, G, t, pano_lat, ring=True)
    new_pers = sch.fused_cfg_step_windows(preds_pers, plan.starts_dev, plan.weights, G, t, pers_lat, ring=True)
    torch.cuda.synchronize()

    cfg = sd21_unet_cfg(5)
    cfg.xformers = True
    sd = {k: v.float().cpu() for k, v in mv.state_dict().items()}
    q = lambda v: v.to(dt).float() if torch.is_floating_point(v) else v
    torch.manual_seed(7)
    random.seed(7)
    masks, o_pers, o_pano = {}, [], []
    for s in plan.starts:
        op, on = OMV.mv_forward(sd, cfg, q(ring_cut(inp["latents"], 3, s, L)), q(ring_cut(inp["pano_latent"], 2, s, L)), inp["timestep"],
                                q(inp["prompt_embd"]), q(inp["pano_prompt_embd"]), cams, inp["fps_tensor_pano"],
                                inp["fps_tensor_pers"], q(ring_cut(inp["reference_images_clip_feat_pano"], 1, s, L)),
                                q(ring_cut(inp["reference_images_clip_feat_pers"], 2, s, L)), ring_cut(inp["relative_position_tensor"], 1, s, L),
                                ring_cut(inp["pitchs_tensor"], 1, s, L), mask_cache=masks)
        o_pers.append(op)
        o_pano.append(on)
    coefs = sch.step_coefficients(t, 0.0, G)
    w = context_weights(L, "pyramid")
    x_pano, x_pers = q(inp["pano_latent"])[:1, :4], q(inp["latents"])[:1, :, :4]
    e_pano = host_step_on(host_ring_blends(torch.stack(o_pano), x_pano, plan.starts, w, G)[0], x_pano, None, sch.kernel_mode(), coefs)
    e_pers = host_step_on(host_ring_blends(torch.stack(o_pers), x_pers, plan.starts, w, G)[0], x_pers, None, sch.kernel_mode(), coefs)
    errs = dict(pano_latent=rel(new_pano, e_pano), pers_latent=rel(new_pers, e_pers),
                pano_pred_w0=rel(preds_pano[0], o_pano[0]), pano_pred_w1=rel(preds_pano[1], o_pano[1]),
                pers_pred_w0=rel(preds_pers[0], o_pers[0]), pers_pred_w1=rel(preds_pers[1], o_pers[1]))
    _record(f"looping_windowed_step_vs_oracle_{str(dt).split('.')[-1]}", **errs)
    assert max(errs.values()) < tol, errs
