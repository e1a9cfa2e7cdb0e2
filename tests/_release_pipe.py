"""The small pipeline the GPU tests of release mode and of the spherical feather share (the recipe of
test_keep_mask_gpu.py::small_pipe): 8 frames -- the ring windows of 4 frames need them; on the GPU the temporal attention refuses a
window of 2 -- 256 x 512, width-5 model, bf16, 4 inference steps of which ``strength`` 0.75 runs the last 3."""
import random

import torch

from imagine360_amd import configs, synthetic as S
from imagine360_amd.scheduler import DDIMScheduler

FRAMES, PANO_HW, STEPS, STRENGTH = 8, (256, 512), 4, 0.75
LAT_HW = (PANO_HW[0] // 8, PANO_HW[1] // 8)


def make_clip():
    return S.video_batch(frames=FRAMES, pano_hw=PANO_HW, seed=2)


def make_runner(clip):
    """run(use_graph, seed=33, scheduler=None, **keywords) -> (video, panorama latent, perspective latent), a fresh pipeline per call."""
    from imagine360_amd.pipeline import AnimationPipeline
    dt, dev = torch.bfloat16, torch.device("cuda", 0)
    mv = configs.build_mv_model(5, device=dev, dtype=dt, xformers=True)
    vae = configs.build_vae(4, device=dev, dtype=dt)
    cond = S.conditioning(frames=16, seed=2)

    def run(use_graph, seed=33, scheduler=None, **kw):
        sch = scheduler or DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
        pipe = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, sch, None, "SAM").to(dev)
        pipe._no_progress, pipe.use_graph = True, use_graph
        torch.manual_seed(seed)
        random.seed(seed)
        vid = pipe("synthetic", num_inference_steps=STEPS, guidance_scale_text=7.5, negative_prompt="", video_batch=clip,
                   use_outpaint=True, use_ip_plus_cross_attention=True, use_fps_condition=True, ip_plus_condition="video",
                   latents_dtype=dt, prompt_embeds=(cond["text_pano"], cond["text_pers"]), sam_features=(cond["sam_pano"], cond["sam_pers"]),
                   **kw).videos
        return vid, pipe.last_latents[0].clone(), pipe.last_latents[1].clone()
    prep = AnimationPipeline(vae, None, None, mv.unet, mv.pano_unet, mv, DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS), None, "SAM")
    run.prepare_mask = lambda mask, feather=0.0: prep.prepare_regenerate_mask(mask, FRAMES, *LAT_HW, dev, feather=feather)
    return run


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def run_thresholds():
    """(steps, [tau_i]) of the run: the timesteps that are run and the release thresholds after each."""
    sch = DDIMScheduler(**configs.NOISE_SCHEDULER_KWARGS)
    sch.set_timesteps(STEPS)
    steps = sch.timesteps_for_strength(STRENGTH)[1]
    return sch, steps, [sch.release_threshold(steps, i) for i in range(len(steps))]
