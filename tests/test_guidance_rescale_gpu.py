"""Guidance rescale on the MI355X: the factor of the two-launch scheme (cfg_rescale_stats_kernel -> per-workgroup Chan merge) against
fp64, the rescaled step kernels (plain and windows) against an fp64 restatement for every mode, their bit-level guarantees
(rescale = 0, device coefficients, one uniform window, run-to-run), the argument checks, and the pipeline keyword: captured steps
against eager ones and the eager loop against a hand-written one."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import record as _record, rel  # noqa: E402
from imagine360_amd import configs, kernels as K, synthetic as S  # noqa: E402
from imagine360_amd.context import context_weights  # noqa: E402
from imagine360_amd.scheduler import DDIMScheduler, rescale_noise_cfg  # noqa: E402
from test_context_windows import pipe_kw, windows_case  # noqa: E402
from test_context_windows_gpu import KERNEL_CASES  # noqa: E402
from test_ddim_stochastic_gpu import TOL, _host_step  # noqa: E402

torch.set_grad_enabled(False)
G = 7.5
FACTOR_TOL = 2e-6          # 40x what a 256-record Chan merge in fp32 gives on these inputs (1e-8 .. 5e-8); naive fp32 sum x, sum x^2
#                            on the N(3, 0.1^2) case gives 1e-5 .. 2e-5
SHAPE = (1, 4, 5, 7, 24)   # 3360 elements: 420 lanes of 8, not a multiple of the 256-thread block


def _sched():
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(25)
    return sch, sch._timesteps_host[8]


def _host_factor(m, c, phi):
    """fp64: phi std(c) / std(m) + 1 - phi, correction 1, over everything."""
    m, c = m.double(), c.double()
    return float(phi * c.std() / m.std() + (1.0 - phi))


def _host_rescaled_step(u, c, x, z, mode, coefs, phi):
    u, c = u.double(), c.double()
    m = u + coefs[0] * (c - u)
    mr = m * _host_factor(m, c, phi)
    return _host_step(mr, mr, x, z, mode, coefs)           # (guidance on u = c = mr is exact)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mean,std", [(0.0, 0.25), (1.0, 0.25), (3.0, 0.1)])
def test_cfg_rescale_factor_vs_fp64(dt, mean, std):
    """The far-mean case N(3, 0.1^2) is the one a plain fp32 sum x, sum x^2 fails (1e-5 .. 2e-5)."""
    gen = torch.Generator().manual_seed(91)
    u, c = ((torch.randn(SHAPE, generator=gen) * std + mean).to(dt) for _ in range(2))
    r = K.cfg_rescale_factor(u.cuda(), c.cuda(), G, 0.7)
    assert r.dtype == torch.float32 and r.shape == () and r.is_cuda
    want = _host_factor(u.double() + G * (c.double() - u.double()), c, 0.7)
    e = abs(float(r) / want - 1.0)
    print(f"cfg_rescale_factor {dt} N({mean}, {std}^2): r = {float(r):.9g}, fp64 {want:.12g}, rel err {e:.3g}")
    _record(f"cfg_rescale_factor_{str(dt).split('.')[-1]}_mean{mean}", rel_err=e)
    assert e <= FACTOR_TOL, (mean, std, e)
    coef_dev = torch.tensor([G, 0, 0, 0, 0, 0], dtype=torch.float32, device="cuda")
    assert torch.equal(K.cfg_rescale_factor(u.cuda(), c.cuda(), 0.0, 0.7, coef_dev=coef_dev), r)      # guidance from coef_dev[0]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_rescaled_step_kernel_all_modes(dt):
    sch, t = _sched()
    gen = torch.Generator().manual_seed(52)
    u, c, x, z = (torch.randn(SHAPE, generator=gen).to(dt) for _ in range(4))
    u, c = u * 0.25, c * 0.25                # a guided x0 partly inside, partly outside [-1, 1]
    dev = [v.cuda() for v in (u, c, x, z)]
    errs = {}
    for eta in (0.0, 0.8):
        coefs = sch.step_coefficients(t, eta, G)
        coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
        noise = dev[3] if eta > 0 else None
        for pred in (0, 1, 2):
            for extra in (0, 4, 8, 12):
                mode = pred | extra
                for phi in (0.7, 1.0):
                    ref = _host_rescaled_step(u, c, x, z if eta > 0 else None, mode, coefs, phi)
                    out = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs, rescale=phi)
                    assert out.dtype == dt and out.shape == SHAPE
                    errs[f"eta{eta}_mode{mode}_phi{phi}"] = e = rel(out, ref)
                    assert e < TOL[dt], (eta, mode, phi, e)
                    out2 = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, (0.0,) * 6, coef_dev=coef_dev, rescale=phi)
                    assert torch.equal(out2, out), (eta, mode, phi)
                # rescale = 0.0 takes the wrapper's shipped branch (one launch of im360_cfg_ddim_step, no statistics pass)
                plain = K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs)
                assert torch.equal(K.cfg_ddim_step(dev[0], dev[1], dev[2], noise, mode, coefs, rescale=0.0), plain), (eta, mode)
                assert rel(out, plain.float().cpu()) > 1e-2          # (phi = 1.0) the factor is used
    print(f"cfg_ddim_step rescale {dt}: max rel {max(errs.values()):.3g}")
    _record(f"cfg_ddim_step_rescale_{str(dt).split('.')[-1]}", max_rel=max(errs.values()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_grid_stride_and_all_records(dt):
    """256 * 256 * 4 + 300 lanes: every workgroup of the capped 256-workgroup statistics grid loops four or five times, the consumers
    merge all 256 records; twice the same bits."""
    sch, t = _sched()
    n8 = 256 * 256 * 4 + 300
    assert K.lib().im360_cfg_rescale_records(n8 * 8) == 256 and K.lib().im360_cfg_rescale_records(SHAPE[1] * 5 * 7 * 24) == 2
    gen = torch.Generator().manual_seed(53)
    u, c, x, z = (torch.randn(n8 * 8, generator=gen).to(dt) for _ in range(4))
    u, c = u * 0.25 + 1.0, c * 0.25 + 1.0
    dev = [v.cuda() for v in (u, c, x, z)]
    coefs = sch.step_coefficients(t, 1.0, G)
    r = K.cfg_rescale_factor(dev[0], dev[1], G, 0.7)
    want = _host_factor(u.double() + G * (c.double() - u.double()), c, 0.7)
    e_r = abs(float(r) / want - 1.0)
    out = K.cfg_ddim_step(*dev, 1 | 4, coefs, rescale=0.7)
    e = rel(out, _host_rescaled_step(u, c, x, z, 1 | 4, coefs, 0.7))
    print(f"grid stride {dt}: factor rel err {e_r:.3g}, step rel err {e:.3g}")
    _record(f"cfg_ddim_step_rescale_grid_stride_{str(dt).split('.')[-1]}", factor_rel_err=e_r, step_rel=e)
    assert torch.isfinite(out.float()).all() and e < TOL[dt], e
    assert e_r <= FACTOR_TOL, e_r
    assert torch.equal(K.cfg_ddim_step(*dev, 1 | 4, coefs, rescale=0.7), out)
    assert torch.equal(K.cfg_rescale_factor(dev[0], dev[1], G, 0.7), r)


def _host_blends(preds, x, starts, w, g):
    """fp64 per-frame blends of u_k + g (c_k - u_k) and of c_k over the covering windows."""
    fd = x.dim() - 3
    L = preds.shape[fd + 1]
    shape = [1] * x.dim()
    shape[fd] = L
    wv = w.double().reshape(shape)
    m, cb, ws = (torch.zeros(x.shape, dtype=torch.float64) for _ in range(3))
    for k, s in enumerate(starts):
        u, c = preds[k, 0:1].double(), preds[k, 1:2].double()
        m.narrow(fd, s, L).add_(wv * (u + g * (c - u)))
        cb.narrow(fd, s, L).add_(wv * c)
        ws.narrow(fd, s, L).add_(wv.expand_as(u))
    return m / ws, cb / ws


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_rescaled_windows_kernel_all_modes_vs_fp64(dt):
    sch, t = _sched()
    errs = {}
    for ci, (shape, L, starts) in enumerate(KERNEL_CASES):
        preds, x, z = windows_case(shape, L, starts, dt, seed=160 + ci)
        dp, dx, dz = preds.cuda(), x.cuda(), z.cuda()
        st = torch.tensor(starts, dtype=torch.int32, device="cuda")
        for kind in ("uniform", "pyramid"):
            w = context_weights(L, kind)
            dw = w.cuda()
            m, cb = _host_blends(preds, x, starts, w, G)
            mr = m * _host_factor(m, cb, 0.7)
            for eta in (0.0, 0.8):
                coefs = sch.step_coefficients(t, eta, G)
                coef_dev = torch.tensor(coefs, dtype=torch.float32, device="cuda")
                noise, dnoise = (z, dz) if eta > 0 else (None, None)
                for pred in (0, 1, 2):
                    for extra in (0, 4, 8, 12):
                        mode = pred | extra
                        ref = _host_step(mr, mr, x, noise, mode, coefs)
                        out = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs, rescale=0.7)
                        assert out.dtype == dt and out.shape == x.shape
                        errs[f"case{ci}_{kind}_eta{eta}_mode{mode}"] = e = rel(out, ref)
                        assert e < TOL[dt], (ci, kind, eta, mode, e)
                        out2 = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, (0.0,) * 6, coef_dev=coef_dev, rescale=0.7)
                        assert torch.equal(out2, out), (ci, kind, eta, mode)
            plain = K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs)
            assert torch.equal(K.cfg_ddim_step_windows(dp, dx, dnoise, st, dw, mode, coefs, rescale=0.0), plain)
    print(f"cfg_ddim_step_windows rescale {dt}: max rel {max(errs.values()):.3g}")
    _record(f"cfg_ddim_step_windows_rescale_{str(dt).split('.')[-1]}", max_rel=max(errs.values()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_one_uniform_window_is_the_rescaled_step_bit_for_bit(dt):
    sch, t = _sched()
    # panorama / perspective on 16-byte lanes; inner 15 and 9: the scalar path, 480 elements in whole groups of 8 / 108 with a short last one
    for shape in ((1, 4, 5, 7, 24), (1, 3, 4, 5, 4, 8), (1, 4, 8, 3, 5)):
        L = shape[-3]
        preds, x, z = windows_case(shape, L, [0], dt, seed=81)
        preds[0, 0].view(-1)[:64] = 0.0
        preds[0, 1].view(-1)[:64] = 0.0
        preds[0, 1].view(-1)[:32] = -0.0
        dp, dx, dz = preds.cuda(), x.cuda(), z.cuda()
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        w = context_weights(L, "uniform").cuda()
        for eta in (0.0, 0.8):
            coefs = sch.step_coefficients(t, eta, G)
            noise = dz if eta > 0 else None
            for mode in (0, 1, 2, 1 | 4, 0 | 8, 1 | 12):
                a = K.cfg_ddim_step_windows(dp, dx, noise, st, w, mode, coefs, rescale=0.7)
                b = K.cfg_ddim_step(dp[0, 0:1].contiguous(), dp[0, 1:2].contiguous(), dx, noise, mode, coefs, rescale=0.7)
                assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (shape, eta, mode)


def test_rescale_kernels_reject_bad_arguments():
    a = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    coefs = (7.5, 0.5, 0.8, 0.6, 0.7, 0.1)
    with pytest.raises(ValueError, match="noise"):
        K.cfg_ddim_step(a, a, a, None, 1, coefs, rescale=0.7)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        K.cfg_ddim_step(a[:12], a[:12], a[:12], a[:12], 1, coefs, rescale=0.7)
    with pytest.raises(RuntimeError, match="misaligned"):
        K.cfg_ddim_step(a[1:9], a[1:9], a[1:9], a[1:9], 1, coefs, rescale=0.7)
    with pytest.raises(RuntimeError, match="mode 3 unsupported"):
        K.cfg_ddim_step(a, a, a, a, 3, coefs, rescale=0.7)
    with pytest.raises(RuntimeError, match="must be finite"):
        K.cfg_ddim_step(a, a, a, a, 1, coefs, rescale=float("nan"))
    with pytest.raises(RuntimeError, match="must be finite"):
        K.cfg_rescale_factor(a, a, 7.5, float("inf"))
    with pytest.raises(TypeError):
        K.cfg_ddim_step(a.float(), a.float(), a.float(), a.float(), 1, coefs, rescale=0.7)
    lib, p = K.lib(), a.data_ptr()
    ws = torch.zeros(K.RESCALE_RECORD, dtype=torch.float32, device="cuda")
    big = 256 * 8 * 3                        # three records needed
    for rc in (lib.im360_cfg_rescale_stats(p, p, 16, 7.5, None, 8, 0, None, None),
               lib.im360_cfg_ddim_step_rescale(p, p, p, p, p, 16, *coefs, 1, 0.7, None, 8, 0, None, None),
               lib.im360_cfg_rescale_factor(None, 8, 16, 0.7, ws.data_ptr(), None)):
        assert rc != 0 and b"null or misaligned workspace" in lib.im360_last_error()
    for rc in (lib.im360_cfg_rescale_stats(p, p, big, 7.5, ws.data_ptr(), 8, 0, None, None),
               lib.im360_cfg_ddim_step_rescale(p, p, p, p, p, big, *coefs, 1, 0.7, ws.data_ptr(), 8, 0, None, None),
               lib.im360_cfg_rescale_factor(ws.data_ptr(), 8, big, 0.7, ws.data_ptr(), None)):
        assert rc != 0 and b"workspace of 8 floats, 24 needed" in lib.im360_last_error()
    rc = lib.im360_cfg_ddim_step_rescale(p, p, p, p, p, 16, *coefs, 1, float("inf"), ws.data_ptr(), 8, 0, None, None)
    assert rc != 0 and b"must be finite" in lib.im360_last_error()
    rc = lib.im360_cfg_ddim_step_rescale(p, p, p, None, p, 16, *coefs, 1, 0.7, ws.data_ptr(), 8, 0, None, None)
    assert rc != 0 and b"needs a noise tensor" in lib.im360_last_error()
    rc = lib.im360_cfg_rescale_stats(p, p, 16, 7.5, ws.data_ptr(), 8, 7, None, None)
    assert rc != 0 and b"dtype 7 unsupported" in lib.im360_last_error()
    # windows: the same workspace / phi checks, the shape checks of im360_cfg_ddim_step_windows
    x = torch.zeros(1, 4, 4, 2, 8, dtype=torch.bfloat16, device="cuda")
    pr = torch.zeros(2, 2, 4, 2, 2, 8, dtype=torch.bfloat16, device="cuda")
    st, w = torch.tensor([0, 2], dtype=torch.int32, device="cuda"), torch.ones(2, device="cuda")
    with pytest.raises(ValueError, match="noise"):
        K.cfg_ddim_step_windows(pr, x, None, st, w, 1, coefs, rescale=0.7)
    with pytest.raises(RuntimeError, match="must be finite"):
        K.cfg_ddim_step_windows(pr, x, x, st, w, 1, coefs, rescale=float("nan"))
    q = x.data_ptr()
    rc = lib.im360_cfg_rescale_stats_windows(pr.data_ptr(), st.data_ptr(), w.data_ptr(), 2, 4, 4, 2, 16, 7.5, None, 8, 0, None, None)
    assert rc != 0 and b"null or misaligned workspace" in lib.im360_last_error()
    rc = lib.im360_cfg_rescale_stats_windows(pr.data_ptr(), st.data_ptr(), w.data_ptr(), 2, 4, 4, 5, 16, 7.5, ws.data_ptr(), 8, 0, None, None)
    assert rc != 0 and b"out of range" in lib.im360_last_error()                                           # L > F
    rc = lib.im360_cfg_ddim_step_windows_rescale(pr.data_ptr(), q, q, q, st.data_ptr(), w.data_ptr(), 2, 4 * 256, 4, 2, 16, *coefs, 1, 0.7,
                                                 ws.data_ptr(), 8, 0, None, None)
    assert rc != 0 and b"workspace of 8 floats" in lib.im360_last_error()
    rc = lib.im360_cfg_ddim_step_windows_rescale(pr.data_ptr(), q, q, q, st.data_ptr(), w.data_ptr(), 2, 4, 4, 2, 16, *coefs, 3, 0.7,
                                                 ws.data_ptr(), 8, 0, None, None)
    assert rc != 0 and b"mode 3 unsupported" in lib.im360_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def gpu_run():
    """The w/5 synthetic pipeline in bf16 on the real kernels: run(use_graph, frames, steps, **keywords) -> (video, panorama latent,
    perspective latent)."""
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM").to(dev)
    pipe._no_progress = True
    data = {}

    def run(use_graph, frames=8, steps=3, seed=33, **kw):
        if frames not in data:
            data[frames] = S.video_batch(frames=frames, pano_hw=(128, 256), seed=12), S.conditioning(frames=max(frames, 16), seed=12)
        vb, cond = data[frames]
        pipe.use_graph = use_graph
        torch.manual_seed(seed)
        random.seed(seed)
        args = pipe_kw(cond, vb, latents_dtype=dt, **kw)
        args["num_inference_steps"] = steps
        vid = pipe("synthetic", **args).videos
        torch.cuda.synchronize()
        return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone()
    run.pipe = pipe
    return run


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("ctx", [{}, dict(frames=24, context_frames=16, context_overlap=8)], ids=["plain", "windows"])
@pytest.mark.parametrize("eta", [0.0, 0.8])
def test_graphed_rescaled_steps_equal_eager_bit_for_bit(gpu_run, ctx, eta, monkeypatch):
    """guidance_rescale = 0.7, 3 steps: both launches of each branch are captured and replay the eager loop's numbers, for eta = 0
    and for eta = 0.8 with a seeded device generator."""
    from imagine360_amd import graph_step
    cls = graph_step.GraphedWindowedStep if ctx else graph_step.GraphedDenoiseStep
    replays = []
    orig = cls.step
    monkeypatch.setattr(cls, "step", lambda self, t: (replays.append(self.rescale), orig(self, t))[1])
    out = {}
    for graph in (True, False):
        kw = dict(eta=eta, generator=torch.Generator(device="cuda").manual_seed(77)) if eta > 0 else {}
        out[graph] = gpu_run(graph, guidance_rescale=0.7, **ctx, **kw)
    assert replays == [0.7] * 3
    errs = dict(pano=rel(out[True][1], out[False][1]), pers=rel(out[True][2], out[False][2]))
    _record(f"graphed_vs_eager_rescale_{'windows' if ctx else 'plain'}_eta{eta}", **errs)
    assert _same(out[True], out[False]), errs
    assert all(torch.isfinite(v.float()).all() for v in out[True])
    if eta == 0.0:
        off = gpu_run(True, **ctx)
        assert _same(off, gpu_run(True, guidance_rescale=0.0, **ctx))          # phi = 0: the call without the keyword
        assert rel(out[True][1], off[1]) > 1e-2                                 # and phi = 0.7 is another clip


def test_eager_rescaled_step_equals_hand_written_loop_on_the_kernels(gpu_run):
    """One eager step with guidance_rescale = 0.7 against the chain written out per branch: the combination in fp32,
    rescale_noise_cfg in fp32, rounded to the latent dtype, then K.cfg_ddim_step with guidance 1.  The hand-written chain rounds the
    rescaled prediction to 16 bits once more than the kernel does: inside TOL."""
    pipe = gpu_run.pipe
    got = gpu_run(False, steps=1, guidance_rescale=0.7)
    sch = pipe.scheduler

    def step(u, c, g, t, x, coef_dev=None, **kw):
        m = u.float() + g * (c.float() - u.float())
        mr = rescale_noise_cfg(m, c.float(), 0.7).to(x.dtype).contiguous()
        return K.cfg_ddim_step(mr, mr, x.contiguous(), None, sch.kernel_mode(), sch.step_coefficients(t, 0.0, 1.0))
    sch.fused_cfg_step = step
    try:
        want = gpu_run(False, steps=1)
    finally:
        del sch.fused_cfg_step
    errs = dict(pano=rel(got[1], want[1]), pers=rel(got[2], want[2]))
    print(f"eager rescaled step vs hand-written: {errs}")
    _record("rescale_pipeline_vs_hand_loop", **errs)
    assert max(errs.values()) < TOL[torch.bfloat16], errs
