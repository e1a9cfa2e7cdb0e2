#!/usr/bin/env python
"""Fixtures of stochastic DDIM sampling (eta > 0), recorded from the REAL reference (imported read-only through
oracle/tools/ref_shims.py and ref_build.py, like oracle/tools/gen_golden.py).  Authoring container only.

    python tools/gen_ddim_goldens.py [ddim pipeline]

  ddim      -> tests/golden/ddim_full.npz: DDIMScheduler.step (prev_sample, pred_original_sample) over five scheduler
               configurations, eta in {0, 0.5, 1}, with and without use_clipped_model_output, first / middle / last step of
               a 25-step schedule, noise given as variance_noise or drawn from a seeded CPU generator.
  pipeline  -> tests/golden/pipeline_eta_w5.npz: the reference AnimationPipeline exactly as pipeline_w5.npz (width / 5,
               16 frames, 256 x 512, 2 steps, seeds 21, CFG 7.5, fp32, CPU) but with eta = 1.0.
"""
import functools
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
import ref_build as RB  # noqa: E402
import ref_shims  # noqa: E402
from im360_oracle.cfg import sd21_unet_cfg, sd21_vae_cfg  # noqa: E402
from imagine360_amd import configs, synthetic as S  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)

# scheduler configurations of ddim_full.npz (name -> constructor keywords)
DDIM_CONFIGS = {
    "yaml": dict(configs.NOISE_SCHEDULER_KWARGS),
    "default": {},
    "sample": dict(prediction_type="sample"),
    "scaled": dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012, set_alpha_to_one=False,
                   steps_offset=1, clip_sample=False),
    "cos": dict(beta_schedule="squaredcos_cap_v2"),
}
DDIM_STEPS, DDIM_IDX, DDIM_SHAPE = 25, (0, 12, 24), (1, 4, 2, 8, 16)
# (eta, use_clipped_model_output, noise source); eta = 0 draws no noise
DDIM_CASES = [(0.0, False, "vn"), (0.0, True, "vn"), (0.5, False, "vn"), (0.5, True, "vn"), (1.0, False, "vn"),
              (1.0, True, "vn"), (1.0, False, "gen")]
GEN_SEED = 1234


def ddim_inputs():
    """x_t, model output and variance noise of every case (re-derived by the tests, also stored in the fixture)."""
    g = torch.Generator().manual_seed(7)
    return tuple(torch.randn(DDIM_SHAPE, generator=g) for _ in range(3))


def case_key(cfg, idx, eta, clipped, src):
    return f"{cfg}_i{idx}_e{int(eta * 10)}_c{int(clipped)}_{src}"


def save(name, **arrs):
    path = os.path.join(GOLD, name)
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in arrs.items()})
    print("  wrote", path, f"{os.path.getsize(path) / 1e3:.0f} kB")


def round_mantissa(t, bits=15):
    """fp32 rounded to ``bits`` explicit mantissa bits (relative error <= 2^-(bits+1)), the low byte zeroed: the two fp32
    latent trajectories of pipeline_eta_w5.npz then compress below 1 MiB (pipeline_w5.npz holds them unrounded).
    2^-16 = 1.5e-5 at most per element, against the 1e-4 bound of the tests."""
    drop = 23 - bits
    i = t.contiguous().view(torch.int32)
    i = (i + (1 << (drop - 1))) & ~((1 << drop) - 1)
    return i.view(torch.float32)


def gen_ddim():
    print("[ddim_full]")
    R = ref_shims.ref_modules()
    x, v, noise = ddim_inputs()
    out = {"x": x, "model_output": v, "noise": noise}
    for cfg, kw in DDIM_CONFIGS.items():
        sch = R["DDIMScheduler"](**kw)
        sch.set_timesteps(DDIM_STEPS)
        out[f"{cfg}_alphas_cumprod"] = sch.alphas_cumprod
        out[f"{cfg}_timesteps"] = sch.timesteps
        for idx in DDIM_IDX:
            t = sch.timesteps[idx]
            for eta, clipped, src in DDIM_CASES:
                extra = dict(variance_noise=noise) if src == "vn" else dict(generator=torch.Generator().manual_seed(GEN_SEED))
                o = sch.step(v, t, x, eta=eta, use_clipped_model_output=clipped, **extra)
                out[case_key(cfg, idx, eta, clipped, src) + "_prev"] = o.prev_sample
                x0 = o.pred_original_sample
                if f"{cfg}_i{idx}_x0" in out:         # the x0 estimate depends on neither eta, noise nor clipped output
                    assert torch.equal(out[f"{cfg}_i{idx}_x0"], x0)
                out[f"{cfg}_i{idx}_x0"] = x0
        try:
            sch.step(v, sch.timesteps[0], x, eta=1.0, generator=torch.Generator(), variance_noise=noise)
            raise AssertionError("the reference accepted both generator and variance_noise")
        except ValueError:
            pass
    save("ddim_full.npz", **out)


def gen_pipeline():
    """Same run as oracle/tools/gen_golden.py gen_pipeline (pipeline_w5.npz), with eta = 1.0 (no oracle pass: the oracle
    restates the eta = 0 pipeline only)."""
    print("[pipeline_eta_w5]")
    R = ref_shims.ref_modules()
    import animatediff.pipelines.pipeline_animation_inference_dual  # noqa: F401
    frames, steps = 16, 2
    ucfg, vcfg = sd21_unet_cfg(5), sd21_vae_cfg(4)
    mv = RB.ref_mv(ucfg)
    vae = RB.ref_vae(vcfg)
    vb = S.video_batch(frames=frames, pano_hw=(256, 512), seed=0)
    cond = S.conditioning(frames=frames, seed=0)
    pipe = R["AnimationPipeline"](vae=vae, text_encoder=None, tokenizer=None, pers_unet=mv.unet, pano_unet=mv.pano_unet,
                                  mv_base_model=mv, scheduler=RB.ref_scheduler(), image_encoder=None,
                                  image_encoder_name="SAM")
    pipe.enable_vae_slicing()
    pipe._encode_prompt = lambda prompt, *a, **k: cond["text_pano"] if len(prompt) == 1 else cond["text_pers"]
    to_chw = lambda t: t[0].reshape(frames, 64, 64, 256).permute(0, 3, 1, 2)
    ref_shims._SamStub.preset = torch.cat([to_chw(cond["sam_pano"]), to_chw(cond["sam_pers"])])
    pipe.SAMpredictor = ref_shims._SamStub()
    pipe.SAMProcessor = pipe.SAMpredictor.transform
    trace = []
    orig_step = pipe.scheduler.step
    calls = [0]

    @functools.wraps(orig_step)             # the pipeline passes eta / generator only to a step whose signature names them
    def step(*a, **k):
        assert k.get("eta") == 1.0, k
        o = orig_step(*a, **k)
        if calls[0] % 2 == 0:
            trace.append(o.prev_sample.clone())
        calls[0] += 1
        return o
    pipe.scheduler.step = step
    torch.manual_seed(21)
    random.seed(21)
    np.random.seed(21)
    t0 = time.time()
    vid = pipe("a synthetic prompt", num_inference_steps=steps, guidance_scale_text=7.5, negative_prompt="", eta=1.0,
               latents_dtype=torch.float32, video_batch=vb, use_outpaint=True, use_ip_plus_cross_attention=True,
               use_fps_condition=True, ip_plus_condition="video").videos
    print(f"  reference pipeline {time.time() - t0:.1f}s", vid.shape)
    out = {f"pano_latent_{i}": round_mantissa(t) for i, t in enumerate(trace)}
    out["video_sub"] = vid[:, :, ::3, ::4, ::4].half()
    out["video_frame_stats"] = torch.stack([vid.mean(dim=(0, 1, 3, 4)), vid.std(dim=(0, 1, 3, 4))])
    save("pipeline_eta_w5.npz", **out)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["ddim", "pipeline"]:
        globals()["gen_" + w]()
