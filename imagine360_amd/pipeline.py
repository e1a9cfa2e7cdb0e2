"""AnimationPipeline: the DDIM loop that drives the dual-branch model
(animatediff/pipelines/pipeline_animation_inference_dual.py:60-824), same constructor and ``__call__``
surface, rebuilt for the MI355X:

  * the loop body is MultiViewBaseModel.forward (HIP kernels) + ONE fused CFG+DDIM kernel per branch;
    no per-step empty_cache()/flush() syncs, no host round trips (timesteps are host ints);
  * conditioning that the reference recomputes is built once: text embeddings, SAM features, masked
    latents, the nearest-E2P index maps of init_noise, the pad-4 latent for the decode;
  * RNG: ``rng="host"`` draws every Gaussian (init noise, VAE posterior samples, per-step IP noise) from
    the CPU generator in the reference's order, so results are comparable to the reference's CPU path
    on the same seeds; ``rng="device"`` (default) draws on the GPU like the reference's GPU path;
  * stochastic DDIM (``eta > 0``): per step, after the model's IP-adapter noise, the panorama then the perspective variance
    noise is drawn (from ``generator`` when given), exactly where the reference's ``scheduler.step`` draws it;
  * guidance rescale (``guidance_rescale=phi``, arXiv 2305.08891 section 3.4): the guided prediction of each branch scaled towards
    the text prediction's standard deviation inside the CFG + DDIM kernels (a statistics launch in front of the step launch);
  * adaptive projected guidance (``apg_eta=eta``, ``apg_threshold=r``, arXiv 2410.02416): the guidance difference of each branch split
    along the text branch's denoised prediction, its parallel part scaled by eta, its RMS clamped to r, in place of the CFG
    combination inside the fused step kernels (a statistics launch in front of the step launch); ``apg_momentum=beta`` adds the
    paper's momentum, a running average of the guidance difference over the guided steps held in an fp32 state per branch that the
    same kernels read and update in place;
  * long clips (``context_frames=L``): sliding temporal context windows -- one forward of the unmodified model per window
    of L frames, the windows' predictions blended per frame inside the CFG + DDIM kernel (imagine360_amd/context.py).
  * a start from a clip that exists (``init_latents`` / ``init_video`` with ``strength``): the clean latent noised to the timestep at
    which the shortened schedule is entered and resampled to the views in ONE kernel (``kernels.noise_latents``); only the
    remaining steps run.
  * regenerating part of such a clip (``regenerate_mask``): after the two step kernels of every step ONE more kernel
    (``kernels.keep_latents``) blends both latents with the clean clip noised to the level they now have, so the kept region ends as
    the input, bit for bit.  ``regenerate_mode="release"`` reads the mask as a per-pixel strength instead (Differential Diffusion,
    arXiv 2306.00950): the same launch pins a pixel to the noised clip until the run passes the pixel's own entry point and leaves it
    alone from then on (``kernels.keep_latents_release``), so nothing is averaged; ``regenerate_feather`` feathers the mask on the
    sphere, in great-circle angle, with the distances from ONE kernel (``kernels.sphere_distance2``).
  * a hi-res pass (``init_latents`` / ``init_video`` SMALLER than the run, ``init_resize``): the clean latent of a clip generated at the
    trained size is upscaled once, as the equirectangular image it is (longitude wraps, latitude clamps), in ONE kernel
    (``kernels.resize_pano_latent``) in front of everything above, which then sees a clean latent of the run's size.
  * a frame-interpolation pass (``init_latents`` / ``init_video`` with FEWER FRAMES than the run, ``init_retime``): the clean latent of
    a clip generated at a coarse frame stride is retimed once along its frame axis -- source frames land exactly on output frames; a
    looping clip is a ring -- in ONE kernel (``kernels.retime_pano_latent``) in front of the upscale.
  * FreeInit passes (``free_init_iters`` > 1, arXiv 2312.07537): the whole schedule is run again from the previous pass's clean clip,
    noised back to the first timestep with an EFFECTIVE noise that keeps the low spatio-temporal frequencies of the noised clip and takes
    the high ones from a fresh draw (``kernels.free_init_noise``: three launches, each axis filtered with its own boundary -- longitude
    periodic, latitude mirrored, frames periodic only on a looping clip); the captured step graph is replayed across the passes.
  * a guidance interval (``guidance_interval=(lo, hi)``, arXiv 2404.07724): the steps whose timestep lies outside the interval run the
    model on the text half alone -- batch 1 instead of the CFG batch of two -- and the unguided form of the same step kernel
    (``scheduler.fused_step``); a graphed run replays one of two captured graphs per step.

CLIP text encoding and SAM feature extraction are outside the hot path: the
pipeline uses ``text_encoder``/``tokenizer``/``image_encoder`` when given, and also accepts precomputed
``prompt_embeds`` / ``sam_features`` keyword arguments.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from . import kernels
from . import pano_geometry as G

VAE_SCALE = 0.18215        # hard-coded in the reference pipeline (:303, :440, :465)


def variance_noise(scheduler, latent, model_dtype, generator, rng, shard=None, frame_dim=2, use_clipped_model_output=False):
    """The variance noise DDIMScheduler.step draws for ``latent`` (scheduling_ddim.py:354-366), in the latent's dtype.
    ``rng="device"``: torch.randn on the latent's device from ``generator`` (None: the global device generator) in the dtype
    the reference draws in; ``"host"``: float32 from the CPU ``generator`` (or the global CPU generator), then moved.
    ``shard`` (dist.FrameShard): drawn for the whole clip along ``frame_dim`` and cut to the local frames."""
    shape = list(latent.shape)
    if shard is not None:
        shape[frame_dim] = shard.total
    if rng == "host":
        gen = generator if generator is not None and generator.device.type == "cpu" else None
        z = torch.randn(shape, generator=gen, dtype=torch.float32)
    else:
        dt = scheduler.noise_dtype(model_dtype, latent.dtype, use_clipped_model_output)
        z = torch.randn(shape, generator=generator, device=latent.device, dtype=dt)
    if shard is not None:
        z = shard.take(z, frame_dim)
    return z.to(device=latent.device, dtype=latent.dtype).contiguous()


REGENERATE_MODES = ("blend", "release")
CONTEXT_LEVELS = ("model", "attention")          # where the context windows apply: whole-model forwards, or inside the motion modules' attention


class KeepRegion:
    """What ``regenerate_mask`` pins while the rest of a given clip is regenerated: the clean panorama latent ``x0`` [1, 4, F, h, w],
    the fp32 panorama noise [1, F, 4, h, w] the start latents were noised with, the mask [F, h, w] (float32; 1: regenerate, 0: keep),
    the nearest-E2P tables of the views and the timesteps that are run.  ``apply`` is the launch after the two step launches of step
    ``i``; the graphed steps call ``blend`` themselves with ``coefficients_at`` uploaded to the device (``n_coef`` floats).
    ``mode``: "blend" (``kernels.keep_latents``, two coefficients) or "release" (``kernels.keep_latents_release``: the mask is a
    per-pixel strength, the third coefficient ``scheduler.release_threshold`` of the step)."""

    def __init__(self, scheduler, steps, x0, noise, mask, idx, ok, mode="blend"):
        if mode not in REGENERATE_MODES:
            raise ValueError(f"regenerate_mode must be one of {list(REGENERATE_MODES)}, got {mode!r}")
        self.scheduler, self.steps, self.mode = scheduler, list(steps), mode
        self.x0, self.noise, self.mask, self.idx, self.ok = x0, noise, mask, idx, ok
        self.n_coef = 3 if mode == "release" else 2

    def coefficients(self, i):
        """The coefficients of the launch after step ``i``: ``scheduler.keep_coefficients``, in release mode followed by
        ``scheduler.release_threshold``."""
        c = self.scheduler.keep_coefficients(self.steps, i)
        return c + (self.scheduler.release_threshold(self.steps, i),) if self.mode == "release" else c

    def coefficients_at(self, t_host):
        """``coefficients`` for the step at timestep ``t_host``; (1.0, 0.0) for a timestep the run does not hold (the warm-up of a
        graphed step, whose numbers are dropped), in release mode with a threshold of -1.0, which pins nothing."""
        t = int(t_host)
        if t in self.steps:
            return self.coefficients(self.steps.index(t))
        return (1.0, 0.0, -1.0) if self.mode == "release" else (1.0, 0.0)

    def blend(self, pano_latent, pers_latent, sqrt_a=1.0, sqrt_b=0.0, tau=-1.0, coef_dev=None):
        """The launch itself (``tau``: release mode only)."""
        if self.mode == "release":
            return kernels.keep_latents_release(pano_latent, pers_latent, self.x0, self.noise, self.mask, self.idx, self.ok, sqrt_a, sqrt_b,
                                                tau, coef_dev=coef_dev)
        return kernels.keep_latents(pano_latent, pers_latent, self.x0, self.noise, self.mask, self.idx, self.ok, sqrt_a, sqrt_b,
                                    coef_dev=coef_dev)

    def apply(self, pano_latent, pers_latent, i):
        return self.blend(pano_latent, pers_latent, *self.coefficients(i))


@dataclass
class AnimationPipelineOutput:
    videos: torch.Tensor


class AnimationPipeline:
    def __init__(self, vae, text_encoder, tokenizer, pers_unet, pano_unet, mv_base_model, scheduler,
                 image_encoder=None, image_encoder_name="CLIP"):
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.pers_unet, self.pano_unet, self.mv_base_model, self.scheduler = pers_unet, pano_unet, mv_base_model, scheduler
        self.image_encoder, self.image_encoder_name = image_encoder, image_encoder_name
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1)
        self.SAMpredictor = self.SAMProcessor = None
        if image_encoder_name == "SAM" and image_encoder is not None:
            from segment_anything import SamPredictor
            self.SAMpredictor = SamPredictor(image_encoder)
            self.SAMProcessor = self.SAMpredictor.transform
        self.rng = "device"
        self.use_graph = True       # replay one captured hipGraph per step (device RNG only; see graph_step.py)
        self._device = None

    # ---- reference surface ------------------------------------------------------------------------
    def to(self, device):
        self._device = torch.device(device)
        for m in (self.vae, self.text_encoder, self.mv_base_model, self.image_encoder):
            if isinstance(m, torch.nn.Module):
                m.to(device)
        return self

    @property
    def device(self):
        return self._device or self.vae.device

    _execution_device = device

    def enable_vae_slicing(self):
        self.vae.enable_slicing()

    def disable_vae_slicing(self):
        self.vae.disable_slicing()

    def progress_bar(self, iterable=None, total=None):
        from tqdm.auto import tqdm
        return tqdm(iterable, total=total, disable=getattr(self, "_no_progress", False))

    # ---- conditioning producers (outside the hot path) ----------------------------------------------
    def _encode_prompt(self, prompt, device, num_videos_per_prompt, do_classifier_free_guidance, negative_prompt):
        """CLIP text embeddings, uncond first (pipeline...dual.py:210-297)."""
        if self.text_encoder is None or self.tokenizer is None:
            raise RuntimeError("no text_encoder/tokenizer: pass prompt_embeds=(pano [2,77,d], pers [2m,77,d])")
        tok = lambda s: self.tokenizer(s, padding="max_length", max_length=self.tokenizer.model_max_length,
                                       truncation=True, return_tensors="pt").input_ids.to(device)
        emb = self.text_encoder(tok(prompt))[0]
        emb = emb.repeat_interleave(num_videos_per_prompt, dim=0)
        if do_classifier_free_guidance:
            neg = negative_prompt if negative_prompt is not None else [""] * len(prompt)
            neg = [neg] * len(prompt) if isinstance(neg, str) else ["" if n is None else n for n in neg]   # None -> "" like the reference
            un = self.text_encoder(tok(neg))[0].repeat_interleave(num_videos_per_prompt, dim=0)
            emb = torch.cat([un, emb])
        return emb

    def _sam_features(self, anchor):
        """anchor [1, F, 3, h, w] in [-1, 1] -> [1, F, 4096, 256] (pipeline...dual.py:671-718)."""
        if self.SAMpredictor is None:
            raise RuntimeError("no SAM image_encoder: pass sam_features=(pano [1,F,4096,256], pers [1,F,4096,256])")
        imgs = np.uint8(((anchor.float() + 1.0) / 2.0 * 255).squeeze(0).cpu().numpy().transpose(0, 2, 3, 1))
        ts = torch.stack([torch.as_tensor(self.SAMProcessor.apply_image(im), device=anchor.device).permute(2, 0, 1).contiguous()
                          for im in imgs])
        assert ts.shape[0] % 8 == 0
        feats = []
        for i in range(0, ts.shape[0], 8):
            self.SAMpredictor.set_torch_image(ts[i:i + 8], ts[0].shape[:2])
            feats.append(self.SAMpredictor.get_image_embedding().flatten(2).transpose(1, 2))
        return torch.cat(feats).unsqueeze(0)

    # ---- pieces of the hot path -------------------------------------------------------------------
    def _randn(self, shape, device, dtype=torch.float32):
        if self.rng == "host":
            return torch.randn(shape, dtype=torch.float32).to(device=device, dtype=dtype)
        return torch.randn(shape, device=device, dtype=dtype)

    def pano_noise_and_index(self, bs, video_length, equi_h, equi_w, pers_h, pers_w, cameras, device):
        """The first half of ``init_noise``: the ONE panorama noise draw, float32 [bs, F, 1, 4, h, w], and the frame-invariant
        nearest-neighbour E2P tables (index, validity flag; [m, ph, pw]) on ``device``.  A run that starts from a given clip
        (``init_latents`` / ``init_video``) takes these and leaves the second half to ``kernels.noise_latents``."""
        pano = self._randn((bs, video_length, 1, 4, equi_h, equi_w), device)
        idx, ok = G.nearest_e2p_index(equi_h, equi_w, pers_h, pers_w, cameras)            # [m, ph, pw]
        return pano, idx.to(device), ok.to(device)

    def init_noise(self, bs, video_length, equi_h, equi_w, pers_h, pers_w, cameras, device, latents_dtype=torch.float16):
        """One panorama noise; the perspective noise is its nearest-neighbour E2P resampling, so both branches
        start from consistent noise (pipeline...dual.py:361-387).  The index maps are frame-invariant and
        built once instead of 16 x 20 host-side map builds."""
        pano, idx, ok = self.pano_noise_and_index(bs, video_length, equi_h, equi_w, pers_h, pers_w, cameras, device)
        return self.latents_from_noise(pano, idx, ok, latents_dtype)

    def latents_from_noise(self, pano, idx, ok, latents_dtype=torch.float16):
        """The second half of ``init_noise``: both start latents from the panorama noise and the tables of ``pano_noise_and_index``."""
        bs, video_length, _, _, equi_h, equi_w = pano.shape
        flat = pano.squeeze(2).reshape(bs, video_length, 4, equi_h * equi_w)
        pers = flat[..., idx.reshape(-1)].reshape(bs, video_length, 4, *idx.shape) * ok   # b f c m h w
        return (pano.squeeze(2).permute(0, 2, 1, 3, 4).contiguous().to(latents_dtype),
                pers.permute(0, 3, 2, 1, 4, 5).contiguous().to(latents_dtype))

    def encode_init_video(self, video, chunk=8):
        """A clip [1, F, 3, H, W] in [-1, 1] -> its clean panorama latent [1, 4, F, H/8, W/8], scaled by ``VAE_SCALE``: the VAE
        encoder in chunks of ``chunk`` frames, the posterior's mode -- no draw from any RNG, so every other draw of the call keeps
        its place."""
        b, f = video.shape[:2]
        x = video.reshape(b * f, *video.shape[2:])
        lat = torch.cat([self.vae.encode(x[i:i + chunk], min(chunk, b * f - i)).latent_dist.mode() for i in range(0, b * f, chunk)])
        return lat.reshape(b, f, *lat.shape[1:]).permute(0, 2, 1, 3, 4) * VAE_SCALE

    def resize_init(self, x0, video_length, equi_h, equi_w, device, latents_dtype=torch.float16, init_resize="bicubic", init_retime=None,
                    loop=False):
        """The clean init latent ``x0`` [1, 4, f, h, w] at the frame count and size of the run: itself when ``(f, h, w) == (video_length,
        equi_h, equi_w)`` -- no launch, no copy.  Otherwise, in ``latents_dtype`` on ``device``: with ``f < video_length`` and
        ``init_retime`` given ("linear" or "cubic"; None, the default: another frame count is refused as ever) retimed once at its
        own (small) size (``kernels.retime_pano_latent``: source frames land on output frames;
        ``loop``: the frames are a ring), then, with another size, upscaled once (``kernels.resize_pano_latent``: half-pixel centres,
        ``init_resize`` "bicubic" or "bilinear", columns wrap, rows clamp).  An init that differs in both is rounded to
        ``latents_dtype`` twice, once by each kernel.  ``ValueError``: more frames than the run (there is no temporal antialiasing
        filter), fewer without ``init_retime``, or an init that is larger than the run in either dimension (there is no spatial
        filter either)."""
        frames_ok = x0.dim() == 5 and (x0.shape[2] == video_length or (init_retime is not None and 1 <= x0.shape[2] < video_length))
        if not frames_ok or tuple(x0.shape[:2]) != (1, 4) or x0.shape[3] > equi_h or x0.shape[4] > equi_w:
            raise ValueError(f"the init latent must be [1, 4, {video_length}, {equi_h}, {equi_w}] or smaller in its last two dimensions "
                             f"(a clean panorama latent, multiplied by VAE_SCALE, such as pipe.last_latents[0]; a smaller one is "
                             f"upscaled, init_resize) or, with init_retime='linear' or 'cubic', with fewer frames (retimed to the run's frame count), got "
                             f"{tuple(x0.shape)}")
        if x0.shape[2] != video_length:
            x0 = kernels.retime_pano_latent(x0.to(device=device, dtype=latents_dtype).contiguous(), video_length, init_retime, bool(loop))
        if tuple(x0.shape[3:]) == (equi_h, equi_w):
            return x0
        return kernels.resize_pano_latent(x0.to(device=device, dtype=latents_dtype).contiguous(), equi_h, equi_w, init_resize)

    def init_from_clip(self, x0, strength, video_length, equi_h, equi_w, pers_h, pers_w, cameras, device, latents_dtype=torch.float16,
                       regenerate_mask=None, regenerate_mode="blend"):
        """The start of a run from a given clean panorama latent ``x0`` [1, 4, F, h, w] (SDEdit): ``init_noise``'s panorama noise
        draw at its place in the RNG order, the schedule entered at ``scheduler.timesteps_for_strength(strength)``, and ``x0`` noised
        to the first timestep that is run, the perspective start being the nearest-neighbour E2P resampling of the panorama start
        (``kernels.noise_latents``, one launch).  Returns (pano_latent, pers_latent, steps); with ``regenerate_mask`` (float32
        [F, h, w] on ``device``) a fourth value, the ``KeepRegion`` (of ``regenerate_mode``) that holds on to the clean latent, this noise and
        the tables."""
        if tuple(x0.shape) != (1, 4, video_length, equi_h, equi_w):
            raise ValueError(f"the init latent must be [1, 4, {video_length}, {equi_h}, {equi_w}] (a clean panorama latent, multiplied by "
                             f"VAE_SCALE, such as pipe.last_latents[0]), got {tuple(x0.shape)}")
        noise, idx, ok = self.pano_noise_and_index(1, video_length, equi_h, equi_w, pers_h, pers_w, cameras, device)
        _, steps = self.scheduler.timesteps_for_strength(strength)
        sqrt_a, sqrt_b = self.scheduler.noise_coefficients(steps[0])
        x0, noise, idx, ok = x0.to(device=device, dtype=latents_dtype).contiguous(), noise.squeeze(2), idx.to(torch.int32), ok.to(torch.uint8)
        pano, pers = kernels.noise_latents(x0, noise, idx, ok, sqrt_a, sqrt_b)
        if regenerate_mask is not None:
            return pano, pers, steps, KeepRegion(self.scheduler, steps, x0, noise, regenerate_mask, idx, ok, mode=regenerate_mode)
        return pano, pers, steps

    def prepare_regenerate_mask(self, mask, video_length, equi_h, equi_w, device, feather=0.0):
        """``regenerate_mask`` [1, F, 1, H', W'] (the layout and polarity of ``video_batch["pano_mask"]``: 1 regenerate, 0 keep) ->
        float32 [F, h, w] on ``device``: nearest-resized to the panorama latent with the call of ``prepare_masked_latents_pano``,
        clamped to [0, 1].  ``feather`` > 0 (degrees of great-circle arc): the map is then feathered on the sphere,
        ``pano_geometry.feather_pano_mask`` with the distances from ``kernels.sphere_distance2`` (one launch)."""
        if mask.dim() != 5 or mask.shape[0] != 1 or mask.shape[2] != 1:
            raise ValueError(f"regenerate_mask must be [1, F, 1, H, W] like video_batch['pano_mask'], got {tuple(mask.shape)}")
        if mask.shape[1] != video_length:
            raise ValueError(f"regenerate_mask has {mask.shape[1]} frames, the clip has video_length = {video_length}")
        m = mask.to(device=device, dtype=torch.float32).transpose(2, 1)
        m = F.interpolate(m, size=(m.shape[2], equi_h, equi_w))
        m = m.clamp(0.0, 1.0).reshape(video_length, equi_h, equi_w).contiguous()
        if float(feather) > 0.0:
            m = G.feather_pano_mask(m, feather, distance2=kernels.sphere_distance2).contiguous()
        return m

    def _encode_chunks(self, x, chunk=8, keep_rows=None):
        """VAE-encode images [n, 3, H, W] in chunks of ``chunk`` and sample the posteriors (one randn per chunk, in order).
        ``keep_rows`` (lo, hi): only the rows in [lo, hi) are needed (frame-sharded runs): chunks outside that range are
        not encoded -- their posterior noise is still DRAWN (same shapes, same order) and dropped, so the kept rows get
        exactly the samples of the unsharded run.  Returns the latents of all rows (keep_rows None) or of [lo, hi)."""
        self.vae.sample_on_host = self.rng == "host"
        out = []
        for i in range(0, x.shape[0], chunk):
            xs = x[i:i + chunk]
            n = xs.shape[0]
            if keep_rows is not None and (i + n <= keep_rows[0] or i >= keep_rows[1]):
                shape = (n, 4, xs.shape[-2] // 8, xs.shape[-1] // 8)
                if self.vae.sample_on_host:
                    torch.randn(shape, dtype=torch.float32)
                else:
                    torch.randn(shape, device=x.device)
                continue
            lat = self.vae.encode(xs, n).latent_dist.sample()
            if keep_rows is not None:
                lat = lat[max(keep_rows[0] - i, 0):max(min(keep_rows[1] - i, n), 0)]
            out.append(lat)
        return torch.cat(out)

    def prepare_masked_latents_pano(self, video_length, pix_masked, pano_mask, keep=None):
        """(:427-448) pix [b f c h w] -> latents [b c f h w]; mask nearest-resized to latent resolution.
        ``keep`` (first frame, count): encode only these frames (b == 1); the mask is returned for all frames."""
        b = pix_masked.shape[0]
        rows = None if keep is None else (keep[0], keep[0] + keep[1])
        fl = video_length if keep is None else keep[1]
        assert keep is None or b == 1
        lat = self._encode_chunks(pix_masked.reshape(b * video_length, *pix_masked.shape[2:]), keep_rows=rows)
        lat = lat.reshape(b, fl, *lat.shape[1:]).permute(0, 2, 1, 3, 4) * VAE_SCALE
        mask = pano_mask.transpose(2, 1)
        mask = F.interpolate(mask, size=(mask.shape[2], lat.shape[-2], lat.shape[-1]))
        return lat, mask.to(lat.device)

    def prepare_masked_latents_pers(self, video_length, pix_masked, pers_masks, keep=None):
        """(:451-473) pix [b f m c h w] -> latents [b m c f h w]; ``keep`` as in ``prepare_masked_latents_pano``."""
        b, _, m = pix_masked.shape[:3]
        rows = None if keep is None else (keep[0] * m, (keep[0] + keep[1]) * m)
        fl = video_length if keep is None else keep[1]
        assert keep is None or b == 1
        lat = self._encode_chunks(pix_masked.reshape(b * video_length * m, *pix_masked.shape[3:]), keep_rows=rows)
        lat = lat.reshape(b, fl, m, *lat.shape[1:]).permute(0, 2, 3, 1, 4, 5) * VAE_SCALE
        mk = pers_masks.permute(0, 3, 1, 2, 4, 5).squeeze(0)
        mk = F.interpolate(mk, size=(m, lat.shape[-2], lat.shape[-1])).unsqueeze(3)
        return lat, mk.permute(0, 2, 3, 1, 4, 5).to(lat.device)

    def decode_latents(self, latents, frames_per_call=8):
        """(:301-313) VAE decode -> float32 numpy in [0, 1], [b, 3, f, H, W].  The reference decodes frame by frame; every
        VAE op is per image (GroupNorm, conv, the mid-block attention), so decoding ``frames_per_call`` frames per call
        gives the same numbers with 1/8 of the launches."""
        b, c, f, h, w = latents.shape
        z = (latents / VAE_SCALE).permute(0, 2, 1, 3, 4).reshape(b * f, c, h, w)
        import inspect
        kw = {"batched": True} if "batched" in inspect.signature(self.vae.decode).parameters else {}     # (a user-supplied diffusers VAE has no such keyword)
        frames = [self.vae.decode(z[i:i + frames_per_call].to(self.vae.dtype), **kw).sample
                  for i in range(0, z.shape[0], frames_per_call)]
        video = torch.cat(frames).reshape(b, f, 3, h * 8, w * 8).permute(0, 2, 1, 3, 4)
        return (video / 2 + 0.5).clamp(0, 1).cpu().float().numpy()

    def padding_pano(self, pano, padding=4, latent=False):
        return G.pad_pano(pano, padding if latent else padding * 8)

    def unpadding_pano(self, pano_pad, padding=4, latent=False):
        return G.unpad_pano(pano_pad, padding if latent else padding * 8)

    # ---- the loop ------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, prompt, num_inference_steps=50, guidance_scale_text=7.5, guidance_scale_adapter=7.5,
                 negative_prompt=None, num_videos_per_prompt=1, eta=0.0, generator=None, latents=None,
                 output_type="tensor", return_dict=True, callback=None, callback_steps=1, latents_dtype=torch.float16,
                 video_batch=None, use_outpaint=False, use_ip_plus_cross_attention=False, use_fps_condition=False,
                 ip_plus_condition="image", prompt_embeds=None, sam_features=None, trace=None, frame_shard=None,
                 context_frames=None, context_overlap=4, context_weights="pyramid", guidance_rescale=0.0, context_loop=False,
                 init_latents=None, init_video=None, strength=1.0, regenerate_mask=None, init_resize="bicubic", init_retime=None,
                 free_init_iters=1, free_init_d_s=0.25, free_init_d_t=0.25, regenerate_mode="blend", regenerate_feather=0.0,
                 guidance_interval=None, context_level="model", apg_eta=None, apg_threshold=None, apg_momentum=None, **kwargs):
        """``frame_shard`` (imagine360_amd.dist.FrameShard): this rank denoises a contiguous chunk of the frames (BASELINE
        configs 4 / 5); all ranks must be called with the same seeds and inputs.  Noise is drawn for the whole clip and
        cut, the VAE encodes / the loop runs / the VAE decodes only the local frames, the motion modules exchange tokens
        with one all-to-all each way, and the decoded frames are all-gathered at the end (the only other collective).
        ``context_frames`` (None: off): sliding temporal context windows (imagine360_amd.context) -- per step the model runs on
        overlapping windows of ``context_frames`` frames (the motion modules' trained length; frame positions 0 .. L-1 inside
        every window, which lifts the temporal_position_encoding_max_len ceiling), ``context_overlap`` frames shared between
        neighbours, and the windows' predictions are blended per frame with ``context_weights`` ("pyramid" / "uniform") inside
        the CFG + DDIM kernel.  ``context_frames >= video_length`` is the call without it.
        ``context_loop`` (False: off): the clip is played as a loop -- the windows lie on a ring of ``video_length`` frames
        (context_windows(loop=True)), so a window that crosses the end of the clip shows the motion modules ... F-2, F-1, 0, 1 ...
        as consecutive frames and the loop point is denoised like every other pair of neighbours.  Needs ``context_frames <
        video_length`` (one window cannot wrap); not with ``frame_shard``.
        ``context_level`` ("model": the above, the default; "attention"): WHERE the windows apply.  "attention" runs the model ONCE per
        step on all frames and applies the same plan and weight tables inside the motion modules' temporal self-attention -- the only
        place that looks across frames: every window is attended with frame positions 0 .. L-1 and the windows' attention outputs are
        fused per frame (FreeNoise's window-based attention fusion, arXiv 2310.15169 section 3.2; one launch of
        ``kernels.temporal_attention_windows`` per attention, ``context.windowed_temporal_attention`` is its definition).  No frame of
        an overlap is evaluated twice, and the plain loop runs, so every loop variant works unchanged (graph replay, ``eta``,
        ``guidance_rescale``, ``init_latents`` / ``strength``, ``regenerate_mask`` in both modes, DPM-Solver++ 2M, ``free_init_iters``,
        ``guidance_interval``); the IP tokens come from the whole clip.  At most 64 frames (longer clips: "model"), ``context_frames <=
        16``, not with ``frame_shard``; ``context_frames >= video_length`` is the call without windows.  The result differs from the
        "model" form (there the windows' noise predictions are blended, here the attention outputs inside every motion module); what
        either does to a clip's quality can only be judged with trained weights.
        ``guidance_rescale`` (0.0: off; the paper uses 0.7): ``scheduler.rescale_noise_cfg`` on each branch's guided prediction
        before the update (arXiv 2305.08891, section 3.4: with zero-terminal-SNR betas a guidance of 7.5 over-exposes without it),
        the standard deviations over the whole panorama latent / over all views of the perspective latent (with context windows:
        over the whole clip of blends), computed inside the fused CFG + DDIM kernels.
        ``init_latents`` / ``init_video`` (at most one; None: start from pure noise) with ``strength`` in (0, 1]: start from a clip
        that exists (SDEdit, the video-to-video call of diffusers' pipelines).  ``init_latents``: a clean panorama latent
        [1, 4, F, H/8, W/8], already multiplied by ``VAE_SCALE`` -- ``pipe.last_latents[0]`` of an earlier call is one; ``init_video``:
        [1, F, 3, H, W] in [-1, 1], encoded here (``encode_init_video``: the posterior's mode, no RNG draw).  The clip is noised to the
        timestep at which the schedule is entered and only the last ``int(num_inference_steps * strength)`` steps are run
        (``scheduler.timesteps_for_strength``); ``callback`` and ``trace`` count these steps from 0.  The panorama noise is the draw
        ``init_noise`` makes, at the same place in the RNG order; both start latents come from one launch (``kernels.noise_latents``).
        Every loop variant runs the shortened schedule (graph replay, context windows, ``context_loop``, ``eta``,
        ``guidance_rescale``); not with ``frame_shard``.  Without an init, ``strength`` must be 1.0 and the call is the one without
        these keywords.
        ``regenerate_mask`` (None: off; needs an init): [1, F, 1, H', W'] with values in [0, 1], the layout and polarity of
        ``video_batch["pano_mask"]`` -- 1: regenerate, 0: keep the init clip, between: a blend.  Nearest-resized to the panorama latent
        and clamped (``prepare_regenerate_mask``).  After the two step kernels of every step one launch (``kernels.keep_latents``)
        blends both latents with the clean clip noised to the level the latents now have (``scheduler.keep_coefficients``: the next
        timestep's, the clean clip after the last step), the perspective latent through the nearest-E2P tables of the start, so the
        kept region of ``last_latents[0]`` is the init latent bit for bit; ``trace`` and ``callback`` see the blended latent.
        ``regenerate_mask=video_batch["pano_mask"]`` pins the footage an outpainted panorama came from.  Independent of the model's
        own mask channels; every loop variant; not with ``frame_shard``.  Without the keyword nothing of this runs.
        ``regenerate_mode`` ("blend": the above, the default; "release": Differential Diffusion, arXiv 2306.00950, diffusers' differential
        img2img): ``regenerate_mask`` is a per-pixel STRENGTH ``s`` in [0, 1] and nothing is ever averaged -- a blend of the running latent
        with the noised clip at every step ends as a cross-fade of two clean clips.  After step ``i`` of the ``n`` steps that are run a pixel
        with ``s <= scheduler.release_threshold(steps, i) = 1 - (i + 1) / n`` is PINNED to the noised clip (the bits of mask 0 in blend
        mode) and every other pixel is left as the step wrote it: a pixel is released once and then denoised freely with its neighbours, for
        about the last ``s n`` steps -- the map scales ``strength`` per pixel.  ``s = 1`` is never pinned; ``s = 0`` is pinned after every
        step including the last, so the kept region of ``last_latents[0]`` is the init latent bit for bit as in blend mode, and a 0 / 1 mask
        gives the bits of blend mode at every step.  Still the one launch per step (``kernels.keep_latents_release``; the threshold is the
        third uploaded coefficient of a graphed step); every loop variant ``regenerate_mask`` supports.  "release" without a mask and any
        other name raise ``ValueError``.  ``regenerate_mask=context.keyframe_strength(f, video_length, loop)`` lets the in-betweens of a
        frame-interpolation pass change the less the nearer they are to a source frame; a latitude ramp keeps the poles of a hi-res pass.
        ``regenerate_feather`` (0.0: off; degrees of great-circle arc; needs a mask): the resized mask is feathered ON THE SPHERE once,
        before the loop -- ``min(mask, ramp)`` where ``ramp`` rises from 0 on the kept set ``{mask <= 0}`` of each frame to 1 over that many
        degrees of arc away from it (``pano_geometry.feather_pano_mask``; the distances from ``kernels.sphere_distance2``, one launch, no
        ``HW x HW`` matrix).  It crosses the +-180 degree seam and measures the same arc at a pole as at the equator, which a feather on
        the pixel grid does not.  Independent of ``regenerate_mode``, but a feathered map is MEANT FOR "release" (in blend mode it is a
        ghosted band): ``regenerate_mask=video_batch["pano_mask"], regenerate_feather=20, regenerate_mode="release"`` is the refinement
        pass after an outpaint.  Negative or non-finite values raise ``ValueError``.  Whether release mode and the feather improve a clip
        can only be judged with trained weights.
        ``init_resize`` ("bicubic", or "bilinear"): the hi-res pass.  ``init_latents`` may be [1, 4, F, h, w] with ``h <= H/8`` and
        ``w <= W/8`` and ``init_video`` [1, F, 3, 8h, 8w] (encoded at its own size, no RNG draw): a smaller clean latent is upscaled once
        to the run's size before anything else sees it (``kernels.resize_pano_latent``, one launch: half-pixel centres, columns wrap
        around the +-180 degree seam, rows clamp at the poles), so the noising, ``regenerate_mask`` (the kept region of
        ``last_latents[0]`` is the UPSCALED clean latent bit for bit), both graphed steps, context windows, ``context_loop``, ``eta`` and
        ``guidance_rescale`` run as for an init of the run's size and the RNG order is unchanged.  Generate at the trained size, then
        call again with a ``video_batch`` of twice the size, ``init_latents=pipe.last_latents[0]`` and ``strength`` around 0.5.  An init
        of the run's size never reaches the new code; a larger one raises ``ValueError``.
        ``init_retime`` (None: off, an init with another frame count raises as it always did; "linear", or "cubic"): the
        frame-interpolation pass.  With it ``init_latents`` may be [1, 4, f, h, w] with ``f <= video_length`` and ``init_video`` [1, f, 3, 8h, 8w] (encoded at its own frame count and size, no RNG draw): a clip of fewer
        frames is retimed once to the run's frame count before anything else sees it (``kernels.retime_pano_latent``, one launch, at
        the init's own size and in front of the upscale when both apply -- two roundings to ``latents_dtype`` then).  Output frame j
        samples source time j (f - 1) / (F - 1): endpoint-aligned, so source frames land exactly on output frames (the even ones for
        ``video_length = 2 f - 1``) and are copied there bit for bit; with ``context_loop`` the frames are a ring, j f / F, and the
        in-betweens after the last source frame blend towards the first (the even frames for ``video_length = 2 f``).  Generate 16
        frames at a coarse frame stride, then call again with a ``video_batch`` of the finer stride, ``context_frames=16``,
        ``init_latents=pipe.last_latents[0]``, ``init_retime="linear"`` and ``strength`` around 0.5: the windows inherit the coarse clip's global motion.
        ``regenerate_mask=context.keyframe_mask(f, video_length, loop)`` pins the source frames and denoises only the in-betweens.
        The conditioning ``video_batch`` is the caller's, at the run's frame count.  Everything after the retime runs as for an init
        of the run's frame count, the RNG order is unchanged, and such an init never reaches the new code; an init with MORE
        frames than the run raises ``ValueError`` (there is no temporal antialiasing filter).
        ``free_init_iters`` (1: off, the call without the keyword bit for bit), ``free_init_d_s`` / ``free_init_d_t``: FreeInit (arXiv
        2312.07537; diffusers' ``enable_free_init``, Gaussian filter).  The count is of passes IN TOTAL.  Pass 0 is the call from pure
        noise; its fp32 panorama noise n1 is kept as drawn.  Pass k >= 1 clones the clean panorama latent of pass k - 1, draws a fresh
        panorama noise n2 (one ``_randn((1, F, 1, 4, h, w))`` at the head of the pass, then the per-step draws of any run), forms the
        effective noise ``kernels.free_init_noise(x0, n1, n2, Lf, Lh, Lw, sa, sb)`` with ``(sa, sb) =
        scheduler.noise_coefficients(steps[0])`` -- ``sa x0 + sb n_eff`` is the low-pass of the clip noised with n1 plus the high-pass of
        n2 -- makes both start latents from it with ``kernels.noise_latents`` on the tables of pass 0, and runs the whole schedule
        again.  The clip is noised to the FIRST TIMESTEP OF THE RUN, not to ``num_train_timesteps - 1`` as in diffusers: with the shipped
        zero-terminal-SNR betas t = 999 is pure noise and would erase the clip.  The low-pass is three dense operators
        (``pano_geometry.free_init_operator``), cut-off ``free_init_d_s`` along h and w and ``free_init_d_t`` along the frames (fractions
        of Nyquist): w periodic (the +-180 degree seam), h mirrored (the poles), the frames periodic with ``context_loop`` and mirrored
        otherwise.  The conditioning (masked latents and their posterior draws, text, SAM, masks) is built once and shared; a captured
        step graph is restarted (``GraphedDenoiseStep.restart``), not captured again; ``trace`` / ``callback`` see every pass, step
        indices restart per pass; context windows, ``context_loop``, ``eta``, ``guidance_rescale``, a multistep scheduler and
        ``rng="host"`` work across passes.  ``pipe.free_init_passes``: the clean panorama latent of every pass (one clone each; with
        ``free_init_iters=1`` the one of ``last_latents``); only the last pass is decoded.  Refused (``ValueError``): ``init_latents`` /
        ``init_video`` / ``strength != 1`` / ``regenerate_mask`` (FreeInit re-noises its own result from pure noise), ``frame_shard``,
        ``free_init_iters < 1``.  Whether the passes improve a clip can only be judged with trained weights.
        ``guidance_interval`` (None: off, the call without the keyword bit for bit -- nothing new runs and no second graph is built;
        ``(lo, hi)`` with ``0 <= lo <= hi <= 1``, fractions of ``num_train_timesteps``): "Applying Guidance in a Limited Interval" (arXiv
        2404.07724; ComfyUI's timestep ranges, A1111's CFG interval).  The step at timestep t is GUIDED iff ``lo T <= t < hi T``
        (``scheduler.guided_steps``, the one definition); guidance hurts at high noise levels and is superfluous at low ones, and with
        the shipped zero-terminal-SNR betas at guidance 7.5 that is a quality control of its own.  On an UNGUIDED step the model is
        evaluated on the text half alone (rows [1:2] / [m:2m] of every CFG-batched input; batch 1 instead of 2) and each branch's latent
        is updated by the unguided form of the step kernel the run uses (``scheduler.fused_step`` / ``fused_step_windows``: one prediction
        stream, no guidance read).  RNG: the IP-adapter noise is drawn for the whole CFG batch and cut (``mv._ip_noise_half``, restored
        also when the loop raises), the WarpAttn coins and the ``eta`` variance noise are drawn as on a guided step -- every stream
        stands after the call where it stands after the call without the keyword.  ``guidance_rescale`` is SKIPPED on an unguided step
        (no statistics launch, no factor): the rescale of a prediction towards its own standard deviation is the identity.  Everything
        behind the step is unchanged: ``regenerate_mask``, ``trace`` / ``callback``, the multistep x0 history (its six coefficients do not
        depend on guidance), FreeInit's passes (every pass uses the same flags).  ``lo == hi`` guides no step: a conditional-only
        sampler.  An interval that covers every timestep of the run takes the path of ``None``.  Every loop variant (eager, graph replay,
        context windows on a line and on a ring, ``eta``, ``init_latents`` / ``strength``, DPM-Solver++ 2M, ``free_init_iters``); a graphed run
        with both kinds of step owns two captured graphs over the same static buffers and ``step`` replays the one the flags select.
        The IP tokens of both forms of the SAM features are cached side by side for the run (``context.ip_cache_slots``) and dropped on
        exit.  Malformed intervals and ``frame_shard`` raise ``ValueError``.  What the interval does to a clip's quality can only be
        judged with trained weights.
        ``apg_eta`` (None: off; the paper's value is 0.0) / ``apg_threshold`` (None: no clamp): adaptive projected guidance (APG, arXiv
        2410.02416, algorithm 1; ``scheduler.projected_guidance`` is the definition) in place of the plain CFG
        combination on every guided step.  In x0 space the guidance difference is split into the part parallel to the text branch's
        denoised prediction -- the part that saturates under the shipped zero-terminal-SNR, guidance-7.5 configuration -- and the part
        orthogonal to it; the parallel part is scaled by ``apg_eta`` (0 removes it, 1 keeps it) and the difference is first clamped to
        ``apg_threshold``.  The threshold is an RMS in x0 units, not the paper's norm (which would tie the setting to clip length and
        resolution): the paper's radius equals ``apg_threshold * sqrt(C * H * W)``; it must be > 0.  The three sums run over the domain
        of ``guidance_rescale`` (the whole panorama latent, all views of the perspective latent, with context windows the whole clip of
        blends) inside the fused step kernels: a statistics launch in front of each branch's step launch, nothing read back, captured
        with the step under graph replay.  ``apg_eta=1`` without a threshold is plain CFG up to rounding, not bit for bit; equal
        unconditional and text predictions give the text prediction; a zero denoised text prediction gives NaN.  Everything behind the
        combination is unchanged (the clamp, ``use_clipped_model_output``, ``eta`` > 0, the multistep update and its history, which
        receives the x0 of the projected guidance), and so is the RNG order.  Every loop variant (graph replay, ``eta``, context windows
        on a line and on a ring, ``context_level="attention"``, ``init_latents`` / ``strength``, ``regenerate_mask`` in both modes,
        DPM-Solver++ 2M, ``free_init_iters``, ``guidance_interval``: an unguided step has no guidance difference and makes no APG
        launch).  ``ValueError``: ``apg_threshold`` without ``apg_eta``, non-finite values, ``apg_threshold <= 0``, ``apg_eta`` with
        ``guidance_rescale != 0`` (the two address the same defect; the product of the kernel variants is not built) and with
        ``frame_shard`` (the sums span the frames of all ranks).  What APG does to a clip's look can only be judged with trained
        weights.
        ``apg_momentum`` (None: off, the call without the keyword bit for bit -- no state is allocated and the entry points of before
        run; the paper's values are -0.5 ... -0.75): the paper's momentum beta.  The difference that is projected and clamped becomes
        the running average ``Dbar_t = Delta_t + beta * Dbar_prev`` (x0 units) over the GUIDED steps of a run; a negative beta keeps the
        differences of consecutive steps from piling up in one direction.  Each branch owns an fp32 state like its latent, next to the
        multistep history, read by the statistics launch and read and rewritten in place by the step launch
        (``kernels.cfg_ddim_step(..., apg_momentum=)``); the factor on it, ``scheduler.apg_carry(t_prev, t, beta)``, is computed on
        the host per step (under graph replay: one float uploaded beside the coefficients).  Update order: the first step that is run
        has carry 0 -- it writes the state without reading it -- in a full run, in a ``strength`` < 1 run that enters the schedule
        later, and in every FreeInit pass (the state of the previous pass is dropped); the unguided steps of ``guidance_interval``
        leave the state and the predecessor alone, so the next guided step continues from the last guided one; ``regenerate_mask``
        does not touch the state (it blends latents, not guidance); ``context_level="attention"`` is the plain loop; with whole-model
        context windows (line or ring) the state lives on the clip of blends; both schedulers.  ``apg_momentum=0.0`` equals None bit
        for bit (on the kernels with the state).  ``ValueError``: ``apg_momentum`` without ``apg_eta``, a non-finite value, ``|beta|
        >= 1`` (the running sum diverges); ``frame_shard`` and ``guidance_rescale`` stay refused through ``apg_eta``.  What the
        momentum does to a clip's look can only be judged with trained weights."""
        device = self.device
        vb = video_batch
        plan = None
        guidance_rescale = float(guidance_rescale)
        if hasattr(self.scheduler, "new_history"):
            if eta > 0:
                raise ValueError(f"eta={eta} cannot be combined with {type(self.scheduler).__name__} (DPM-Solver++ 2M is the ODE solver; its "
                                 "SDE variant is not implemented): use DDIMScheduler for stochastic sampling")
            if frame_shard is not None:
                raise ValueError(f"frame_shard cannot be combined with {type(self.scheduler).__name__} (the cut of the x0 history to a rank's "
                                 "frames is not implemented): use DDIMScheduler")
        if guidance_interval is not None:
            self.scheduler.guided_steps((), guidance_interval)            # (ValueError for a malformed interval, before any work)
            if frame_shard is not None:
                raise ValueError("guidance_interval cannot be combined with frame_shard (the text-half step of a frame-sharded model and "
                                 "its second captured graph are not implemented)")
        if guidance_rescale != 0.0 and frame_shard is not None:
            raise ValueError("guidance_rescale cannot be combined with frame_shard (the standard deviations span the frames of all "
                             "ranks and would need an all-reduce inside the step, which is not implemented)")
        apg_kw = {}
        if apg_eta is None:
            if apg_threshold is not None:
                raise ValueError("apg_threshold needs apg_eta (adaptive projected guidance is off without it)")
        else:
            apg_eta = float(apg_eta)
            apg_threshold = None if apg_threshold is None else float(apg_threshold)
            if not math.isfinite(apg_eta):
                raise ValueError(f"apg_eta must be finite, got {apg_eta}")
            if apg_threshold is not None and not (math.isfinite(apg_threshold) and apg_threshold > 0.0):
                raise ValueError(f"apg_threshold must be None (no clamp) or a finite RMS radius > 0, got {apg_threshold}")
            if guidance_rescale != 0.0:
                raise ValueError("apg_eta cannot be combined with guidance_rescale != 0 (both address the over-exposure of a "
                                 "zero-terminal-SNR schedule under strong guidance; the product of the kernel variants is not built)")
            if frame_shard is not None:
                raise ValueError("apg_eta cannot be combined with frame_shard (its sums span the frames of all ranks and would need an "
                                 "all-reduce inside the step, which is not implemented)")
            apg_kw = dict(guidance_apg=(apg_eta, apg_threshold))
        apg_beta = None
        if apg_momentum is not None:
            if apg_eta is None:
                raise ValueError("apg_momentum needs apg_eta (adaptive projected guidance is off without it)")
            apg_beta = float(apg_momentum)
            if not (math.isfinite(apg_beta) and abs(apg_beta) < 1.0):
                raise ValueError(f"apg_momentum must be finite with |beta| < 1 (the running sum diverges otherwise; the paper's values "
                                 f"are -0.5 ... -0.75), got {apg_beta}")
        if context_loop and frame_shard is not None:
            raise ValueError("context_loop cannot be combined with frame_shard (windows under frame sharding are not implemented)")
        if init_latents is not None and init_video is not None:
            raise ValueError("give at most one of init_latents and init_video")
        if init_resize not in G.RESIZE_MODES:
            raise ValueError(f"init_resize must be one of {sorted(G.RESIZE_MODES)}, got {init_resize!r}")
        if init_retime is not None and init_retime not in G.RETIME_MODES:
            raise ValueError(f"init_retime must be None or one of {sorted(G.RETIME_MODES)}, got {init_retime!r}")
        has_init = init_latents is not None or init_video is not None
        if not isinstance(free_init_iters, int) or isinstance(free_init_iters, bool) or free_init_iters < 1:
            raise ValueError(f"free_init_iters counts the passes in total and must be an int >= 1, got {free_init_iters!r}")
        if free_init_iters > 1:
            if has_init or regenerate_mask is not None or float(strength) != 1.0:
                raise ValueError("free_init_iters > 1 cannot be combined with init_latents / init_video / strength != 1 / regenerate_mask "
                                 "(FreeInit re-noises the result of its own first pass, which starts from pure noise and runs the whole "
                                 "schedule)")
            if frame_shard is not None:
                raise ValueError("free_init_iters > 1 cannot be combined with frame_shard (the filter along the frames spans the frames of "
                                 "all ranks and would need a gather between the passes, which is not implemented)")
            if not (float(free_init_d_s) > 0.0 and float(free_init_d_t) > 0.0):
                raise ValueError(f"free_init_d_s={free_init_d_s} and free_init_d_t={free_init_d_t} must be positive (cut-offs as fractions of "
                                 "Nyquist)")
        if regenerate_mode not in REGENERATE_MODES:
            raise ValueError(f"regenerate_mode must be one of {list(REGENERATE_MODES)}, got {regenerate_mode!r}")
        if regenerate_mode == "release" and regenerate_mask is None:
            raise ValueError('regenerate_mode="release" needs regenerate_mask (the per-pixel strength map)')
        regenerate_feather = float(regenerate_feather)
        if not (math.isfinite(regenerate_feather) and regenerate_feather >= 0.0):
            raise ValueError(f"regenerate_feather must be finite and >= 0 (degrees of arc), got {regenerate_feather}")
        if regenerate_feather > 0.0 and regenerate_mask is None:
            raise ValueError("regenerate_feather needs regenerate_mask (the mask that is feathered)")
        if regenerate_mask is not None and not has_init:
            raise ValueError("regenerate_mask needs init_latents or init_video (the clip whose unmasked part is kept)")
        if regenerate_mask is not None and frame_shard is not None:
            raise ValueError("regenerate_mask cannot be combined with frame_shard (the cut of the kept clip, its noise and the mask to a "
                             "rank's frames is not implemented)")
        strength = float(strength)
        if not has_init and strength != 1.0:
            raise ValueError(f"strength={strength} needs init_latents or init_video (a run from pure noise always runs the whole schedule)")
        if has_init and frame_shard is not None:
            raise ValueError("init_latents / init_video cannot be combined with frame_shard (the cut of the noised start latents to a "
                             "rank's frames and the sharded encode of an init clip are not implemented)")
        if context_loop and (context_frames is None or int(context_frames) >= vb["video_length"]):
            raise ValueError(f"context_loop needs context_frames < video_length = {vb['video_length']} (one window cannot wrap around), "
                             f"got context_frames={context_frames}")
        if context_level not in CONTEXT_LEVELS:
            raise ValueError(f"context_level must be one of {list(CONTEXT_LEVELS)}, got {context_level!r}")
        attn_plan = None
        if context_level == "attention":
            if frame_shard is not None:
                raise ValueError('context_level="attention" cannot be combined with frame_shard (windows under frame sharding are not '
                                 "implemented)")
            if vb["video_length"] > 64:
                raise ValueError(f'context_level="attention" runs the model once on the whole clip and takes at most 64 frames, got '
                                 f'video_length={vb["video_length"]}: use context_level="model" (whole-model windows) for longer clips')
            if context_frames is not None and int(context_frames) > 16:
                raise ValueError(f'context_level="attention" takes windows of at most 16 frames (the kernel\'s window tile), got '
                                 f"context_frames={context_frames}")
        if context_frames is not None and int(context_frames) < vb["video_length"]:
            if frame_shard is not None:
                raise ValueError("context_frames cannot be combined with frame_shard (windows under frame sharding are not implemented)")
            from .context import WindowPlan
            plan = WindowPlan(vb["video_length"], context_frames, context_overlap, context_weights, device, loop=bool(context_loop))
            if context_level == "attention":
                # the same plan and tables, applied inside the motion modules' attention: the plain loop runs (``plan`` stays None)
                attn_plan, plan = plan, None
        assert use_outpaint and use_ip_plus_cross_attention, "the dual pipeline runs with use_outpaint and the IP adapter"
        cfg = guidance_scale_text > 1.0
        assert cfg, "the reference only binds its model inputs under classifier-free guidance (:744-751)"
        pano_pix, pano_mask = vb["pano_pixel_values"], vb["pano_mask"]
        pers_pix, pers_masks = vb["pers_pixel_values"], vb["pers_masks"]
        cameras, f = vb["cameras"], vb["video_length"]
        m = pers_pix.shape[2]
        H, W, ps = vb["pano_H"], vb["pano_W"], vb["pers_size"]
        self.mv_base_model.noise_on_host = self.rng == "host"

        pano_pix_masked = (pano_pix * (pano_mask < 0.5)).to(device)
        pers_pix_masked = (pers_pix * (pers_masks < 0.5)).to(device)
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        steps_host = self.scheduler._timesteps_host
        if has_init:
            # the encode draws nothing, so it may come first: the panorama noise is then drawn where init_noise draws it
            x0 = init_latents if init_latents is not None else self.encode_init_video(init_video.to(device))
            x0 = self.resize_init(x0, f, H // 8, W // 8, device, latents_dtype, init_resize, init_retime,
                                  loop=bool(context_loop))                                       # (itself at the run's frame count and size)
            keep_mask = None if regenerate_mask is None else self.prepare_regenerate_mask(regenerate_mask, f, H // 8, W // 8, device,
                                                                                                   feather=regenerate_feather)
            pano_latent, pers_latent, steps_host, *region = self.init_from_clip(x0, strength, f, H // 8, W // 8, ps // 8, ps // 8, cameras,
                                                                                device, latents_dtype, regenerate_mask=keep_mask,
                                                                                regenerate_mode=regenerate_mode)
            region = region[0] if region else None             # (KeepRegion)
        elif free_init_iters > 1:
            # pass 0 is init_noise, its two halves called here so that the panorama noise is kept in fp32 as drawn
            noise1, fi_idx, fi_ok = self.pano_noise_and_index(1, f, H // 8, W // 8, ps // 8, ps // 8, cameras, device)
            pano_latent, pers_latent = self.latents_from_noise(noise1, fi_idx, fi_ok, latents_dtype)
            region = None
        else:
            pano_latent, pers_latent = self.init_noise(1, f, H // 8, W // 8, ps // 8, ps // 8, cameras, device, latents_dtype)
            region = None
        next_pass, passes = None, []
        if free_init_iters > 1:
            noise1, fi_idx, fi_ok = noise1.squeeze(2), fi_idx.to(torch.int32), fi_ok.to(torch.uint8)
            fi_ops = [G.free_init_operator(n, d, per).to(torch.float32).to(device)
                      for n, d, per in ((f, free_init_d_t, bool(context_loop)), (H // 8, free_init_d_s, False), (W // 8, free_init_d_s, True))]

            def next_pass(pano_now, pers_now):
                """Behind the last step of a pass: its clean panorama latent is kept; None after the last pass, else the two start
                latents of the next one."""
                x0 = pano_now.clone()                      # (a graphed step returns its static buffers)
                passes.append(x0)
                if len(passes) >= free_init_iters:
                    return None
                noise2 = self._randn((1, f, 1, 4, H // 8, W // 8), device).squeeze(2)
                sqrt_a, sqrt_b = self.scheduler.noise_coefficients(steps_host[0])
                n_eff = kernels.free_init_noise(x0, noise1, noise2, *fi_ops, sqrt_a, sqrt_b)
                return kernels.noise_latents(x0, n_eff, fi_idx, fi_ok, sqrt_a, sqrt_b)
        hist = None
        if hasattr(self.scheduler, "new_history"):
            # a multistep scheduler: the run's timestep list fixes its coefficients, and each branch's latent owns its x0 history
            self.scheduler.begin_run(steps_host)
            hist = (self.scheduler.new_history(pano_latent), self.scheduler.new_history(pers_latent))
        apg_mom_kw = {} if apg_beta is None else dict(guidance_apg_momentum=apg_beta)
        # (guidance_interval) the flags of the run's steps; None: every step is guided, the call without the keyword
        guided = None if guidance_interval is None else self.scheduler.guided_steps(steps_host, guidance_interval)
        if guided is not None and all(guided):
            guided, guidance_interval = None, None
        sh = frame_shard
        if sh is not None:
            # every rank drew the whole clip's noise from the same seed: cut to the local frames
            pano_latent, pers_latent = sh.take(pano_latent, 2).contiguous(), sh.take(pers_latent, 3).contiguous()
        # frame-sharded: only this rank's frames go through the VAE encoder; the posterior noise of the other frames is still
        # drawn (and dropped), so the samples are those of the unsharded run
        keep = None if sh is None else (sh.f0, sh.local)
        pano_ml, pano_mask_l = self.prepare_masked_latents_pano(f, pano_pix_masked, pano_mask.to(device), keep)
        pers_ml, pers_mask_l = self.prepare_masked_latents_pers(f, pers_pix_masked, pers_masks.to(device), keep)
        if sh is not None:
            pano_mask_l, pers_mask_l = sh.take(pano_mask_l, 2), sh.take(pers_mask_l, 3)
            self.mv_base_model.set_frame_shard(sh)
        ip_slots = None
        try:
            if attn_plan is not None:
                self.mv_base_model.set_temporal_windows(attn_plan)      # before any capture; cleared in the `finally` below
            if prompt_embeds is not None:
                text_pano, text_pers = prompt_embeds
            else:
                text_pano = self._encode_prompt([prompt], device, num_videos_per_prompt, cfg, [negative_prompt])
                text_pers = text_pano.repeat_interleave(m, dim=0)     # the reference encodes the same prompt m times (:628, :655)
            text_pano, text_pers = text_pano.to(device, latents_dtype), text_pers.to(device, latents_dtype)
            if sam_features is not None:
                sam_pano, sam_pers = sam_features
            else:
                sam_pano = self._sam_features(vb["anchor_pixels_values"].to(device))
                sam_pers = self._sam_features(vb["anchor_pixels_values_pers"].to(device))
            feat_pano = torch.cat([sam_pano, sam_pano]).to(device, latents_dtype)
            feat_pers = torch.cat([sam_pers, sam_pers]).to(device, latents_dtype).unsqueeze(1).expand(-1, m, -1, -1, -1)
            fps = torch.tensor(vb["fps"], device=device).unsqueeze(0)
            fps_pano = torch.cat([fps] * 2) if use_fps_condition else None
            fps_pers = torch.cat([fps.unsqueeze(-1).repeat(1, m)] * 2) if use_fps_condition else None
            rel = torch.cat([vb["relative_position"].to(device).unsqueeze(0)] * 2)
            pitch = torch.cat([vb["pitchs"].to(device).unsqueeze(0)] * 2)
            ts_dev = [torch.tensor([t], dtype=torch.int64, device=device) for t in steps_host]
            dt = latents_dtype
            # static halves of the model input: mask + masked latent (channels 4..8), duplicated for CFG
            in_pano = torch.cat([torch.cat((pano_latent, pano_mask_l.to(dt), pano_ml.to(dt)), dim=1)] * 2)
            in_pers = torch.cat([torch.cat((pers_latent, pers_mask_l.to(dt), pers_ml.to(dt)), dim=2)] * 2)

            if plan is not None:
                inputs = dict(latents=in_pers, pano_latent=in_pano, prompt_embd=text_pers, pano_prompt_embd=text_pano,
                              fps_tensor_pano=fps_pano, fps_tensor_pers=fps_pers, reference_images_clip_feat_pano=feat_pano,
                              reference_images_clip_feat_pers=feat_pers, relative_position_tensor=rel, pitchs_tensor=pitch)
                pano_latent, pers_latent = self._windowed_loop(plan, inputs, cameras, pano_latent, pers_latent, steps_host, ts_dev,
                                                               guidance_scale_text, use_fps_condition, eta, generator, trace,
                                                               callback, callback_steps, guidance_rescale, region, hist, next_pass,
                                                               **({} if guided is None else dict(guidance_interval=guidance_interval)), **apg_kw,
                                                               **apg_mom_kw)
            graphed = None
            if guided is not None and plan is None:
                # the text-half views of the model inputs, made once and kept (the IP-token cache keys on the feature tensors' identity),
                # and room in that cache for both forms of the SAM features; closed in the `finally` below
                from .context import ip_cache_slots
                from .dist import cfg_half_inputs
                text_half = cfg_half_inputs(dict(latents=in_pers, pano_latent=in_pano, prompt_embd=text_pers, pano_prompt_embd=text_pano,
                                                 fps_tensor_pano=fps_pano, fps_tensor_pers=fps_pers, reference_images_clip_feat_pano=feat_pano,
                                                 reference_images_clip_feat_pers=feat_pers, relative_position_tensor=rel,
                                                 pitchs_tensor=pitch), 1)
                ip_slots = ip_cache_slots(self.mv_base_model, 2)
                ip_slots.__enter__()
            import torch.distributed as tdist
            capturable = sh is None or (tdist.is_initialized() and tdist.get_backend(sh.group) == "nccl")     # RCCL all-to-alls are stream ops
            if (plan is None and self.use_graph and self.rng == "device" and pano_latent.is_cuda and trace is None and callback is None
                    and capturable):
                from .graph_step import GraphedDenoiseStep
                inputs = dict(latents=in_pers, pano_latent=in_pano, prompt_embd=text_pers, pano_prompt_embd=text_pano,
                              fps_tensor_pano=fps_pano, fps_tensor_pers=fps_pers, reference_images_clip_feat_pano=feat_pano,
                              reference_images_clip_feat_pers=feat_pers, relative_position_tensor=rel, pitchs_tensor=pitch)
                stoch = dict(eta=eta, generator=generator, frame_shard=sh) if eta > 0 else {}
                if region is not None:
                    stoch["keep"] = region
                if guided is not None:
                    stoch.update(guidance_interval=guidance_interval, steps=steps_host)
                stoch.update(apg_kw)
                stoch.update(apg_mom_kw)
                graphed = GraphedDenoiseStep(self.mv_base_model, self.scheduler, inputs, cameras, pano_latent, pers_latent,
                                             guidance_scale_text, use_fps=use_fps_condition, warmup=1, guidance_rescale=guidance_rescale, **stoch)       # one eager step fills every cache
            # (apg_momentum, eager loop) one momentum state per branch next to `hist`, never initialised: the first guided step of
            # every pass has carry 0 and only writes it
            apg_state = None
            if apg_beta is not None and plan is None and graphed is None:
                apg_state = (self.scheduler.new_apg_state(pano_latent), self.scheduler.new_apg_state(pers_latent))
            while plan is None:                 # one round per pass: once without free_init_iters
                apg_prev_t = None               # the previous guided timestep of this pass
                for i, t in enumerate(self.progress_bar(steps_host)):
                    if graphed is not None:
                        pano_latent, pers_latent = graphed.step(t)
                        continue
                    if guided is not None and not guided[i]:
                        pano_latent, pers_latent = self._unguided_step(text_half, pano_latent, pers_latent, ts_dev[i], t, cameras,
                                                                       use_fps_condition, eta, generator, guidance_rescale, hist, **apg_kw)
                    else:
                        in_pano[:, :4] = pano_latent
                        in_pers[:, :, :4] = pers_latent
                        pred_pers, pred_pano = self.mv_base_model(
                            latents=in_pers, pano_latent=in_pano, timestep=ts_dev[i], prompt_embd=text_pers,
                            pano_prompt_embd=text_pano, cameras=cameras, use_fps_condition=use_fps_condition,
                            use_ip_plus_cross_attention=use_ip_plus_cross_attention, fps_tensor_pano=fps_pano, fps_tensor_pers=fps_pers,
                            reference_images_clip_feat_pano=feat_pano, reference_images_clip_feat_pers=feat_pers,
                            relative_position_tensor=rel, pitchs_tensor=pitch)
                        mom = ({}, {})
                        if apg_state is not None:
                            carry = self.scheduler.apg_carry(apg_prev_t, t, apg_beta)
                            mom = tuple(dict(guidance_apg_momentum=(state, carry)) for state in apg_state)
                            apg_prev_t = t
                        pano_latent = self._cfg_step(pred_pano, guidance_scale_text, t, pano_latent, eta, generator, sh, 2, guidance_rescale,
                                                     **({} if hist is None else dict(history=hist[0])), **apg_kw, **mom[0])
                        pers_latent = self._cfg_step(pred_pers, guidance_scale_text, t, pers_latent, eta, generator, sh, 3, guidance_rescale,
                                                     **({} if hist is None else dict(history=hist[1])), **apg_kw, **mom[1])
                    if region is not None:
                        region.apply(pano_latent, pers_latent, i)
                    if trace is not None:
                        trace.append(pano_latent.clone())
                    if callback is not None and i % callback_steps == 0:
                        callback(i, t, pano_latent)
                # (FreeInit) the start latents of the next pass; a captured step is restarted, a multistep history needs no reset (the
                # first step of a run is first order and only writes it)
                start = None if next_pass is None else next_pass(pano_latent, pers_latent)
                if start is None:
                    break
                if graphed is not None:
                    graphed.restart(*start)
                pano_latent, pers_latent = start

            video = self.decode_latents(self.padding_pano(pano_latent, latent=True))
            video = self.unpadding_pano(video)
            if sh is not None:                  # latent / video boundary: the only collective besides the motion-module exchanges
                self.mv_base_model.set_frame_shard(None)
                video = sh.gather_frames(torch.from_numpy(np.ascontiguousarray(video)).to(device), 2).cpu().numpy()
                pano_latent = sh.gather_frames(pano_latent, 2)
                pers_latent = sh.gather_frames(pers_latent, 3)
            if output_type == "tensor":
                video = torch.from_numpy(np.ascontiguousarray(video))
            self.last_latents = (pano_latent, pers_latent)
            self.free_init_passes = passes if free_init_iters > 1 else [pano_latent]
            return AnimationPipelineOutput(videos=video) if return_dict else video
        finally:
            if sh is not None:
                self.mv_base_model.set_frame_shard(None)      # also when the loop raises: the model must not stay sharded
            if attn_plan is not None:
                self.mv_base_model.set_temporal_windows(None)  # ... nor windowed
            if ip_slots is not None:
                ip_slots.__exit__(None, None, None)           # (guidance_interval) back to the single-entry IP-token cache

    def _cfg_step(self, pred, g, t, latent, eta=0.0, generator=None, shard=None, frame_dim=2, guidance_rescale=0.0, guidance_apg=None,
                  guidance_apg_momentum=None, **history):
        """``history`` (``history=``, a multistep scheduler only): the x0 history of this latent, handed on to the scheduler.
        ``guidance_apg`` / ``guidance_apg_momentum`` = (state, carry): handed on when set (``apg_eta`` / ``apg_momentum``)."""
        u, c = pred.to(latent.dtype).chunk(2)          # latents_dtype may differ from the model dtype (the reference promotes)
        apg = {} if guidance_apg is None else dict(guidance_apg=guidance_apg)
        if guidance_apg_momentum is not None:
            apg["guidance_apg_momentum"] = guidance_apg_momentum
        if eta > 0:
            z = variance_noise(self.scheduler, latent, pred.dtype, generator, self.rng, shard, frame_dim)
            return self.scheduler.fused_cfg_step(u, c, g, t, latent, eta=eta, noise=z, guidance_rescale=guidance_rescale, **apg)
        return self.scheduler.fused_cfg_step(u, c, g, t, latent, guidance_rescale=guidance_rescale, **apg, **history)

    def _text_half_step(self, forward, step, pano_latent, pers_latent, eta, generator, hist, model_dtype=None):
        """One unguided step (``guidance_interval``): ``forward()`` runs the model on the text half with ``mv._ip_noise_half = (1, 2)`` --
        the IP-adapter noise is drawn for the whole CFG batch and cut, so the stream advances as on a guided step -- restored also when
        it raises; then ``step(prediction, latent, noise, frame_dim, history)`` per branch, panorama first, the variance noise drawn
        where a guided step draws it (in the dtype it draws it in: ``model_dtype``, default the prediction's)."""
        mv = self.mv_base_model
        was = mv._ip_noise_half
        mv._ip_noise_half = (1, 2)
        try:
            pred_pers, pred_pano = forward()
        finally:
            mv._ip_noise_half = was
        mdt = pred_pano.dtype if model_dtype is None else model_dtype
        out = []
        for branch, (pred, latent, frame_dim) in enumerate(((pred_pano, pano_latent, 2), (pred_pers, pers_latent, 3))):
            z = variance_noise(self.scheduler, latent, mdt, generator, self.rng, None, frame_dim) if eta > 0 else None
            out.append(step(pred, latent, z, {} if hist is None else dict(history=hist[branch])))
        return out

    def _unguided_step(self, text_half, pano_latent, pers_latent, t_dev, t, cameras, use_fps, eta, generator, guidance_rescale, hist,
                       **apg_kw):
        """The one-block loop's unguided step: the model on ``text_half`` (``dist.cfg_half_inputs(inputs, 1)``, made once per run), then
        ``scheduler.fused_step`` per branch."""
        def forward():
            text_half["pano_latent"][:, :4] = pano_latent
            text_half["latents"][:, :, :4] = pers_latent
            return self.mv_base_model(timestep=t_dev, cameras=cameras, use_fps_condition=use_fps, use_ip_plus_cross_attention=True, **text_half)

        def step(pred, latent, z, history):
            return self.scheduler.fused_step(pred.to(latent.dtype), t, latent, **(dict(eta=eta, noise=z) if eta > 0 else {}),
                                             guidance_rescale=guidance_rescale, **apg_kw, **history)
        return self._text_half_step(forward, step, pano_latent, pers_latent, eta, generator, hist)

    def _unguided_windows_step(self, plan, text_half, text_static, text_preds, pano_latent, pers_latent, t_dev, t, cameras, use_fps, eta,
                               generator, guidance_rescale, hist, **apg_kw):
        """The windowed loop's unguided step: every window on its text half (``text_half`` / ``text_static``: views made once per run)
        into the [nW, 1, ...] buffers ``text_preds`` (perspective, panorama), then ``scheduler.fused_step_windows`` per branch."""
        mv, sch = self.mv_base_model, self.scheduler

        def forward():
            text_half["pano_latent"][:, :4] = pano_latent
            text_half["latents"][:, :, :4] = pers_latent
            plan.forward(mv, text_half, text_static, cameras, t_dev, use_fps, *text_preds)
            return text_preds

        def step(preds, latent, z, history):
            return sch.fused_step_windows(preds, plan.starts_dev, plan.weights, t, latent, noise=z, eta=eta,
                                          guidance_rescale=guidance_rescale, ring=plan.loop, **apg_kw, **history)
        return self._text_half_step(forward, step, pano_latent, pers_latent, eta, generator, hist, model_dtype=mv.unet.dtype)

    def _windowed_loop(self, plan, inputs, cameras, pano_latent, pers_latent, steps_host, ts_dev, g, use_fps, eta, generator,
                       trace, callback, callback_steps, guidance_rescale=0.0, keep=None, hist=None, next_pass=None, guidance_interval=None,
                       guidance_apg=None, guidance_apg_momentum=None):
        """The denoising loop over sliding temporal context windows: per step one forward per window (slot order), then ONE
        blend + CFG + DDIM kernel per branch, panorama first.  RNG: as len(plan) successive calls of the model, then (eta > 0)
        the whole clip's panorama and perspective variance noise.  Captured in one hipGraph under the conditions of the
        one-block loop (graph_step.GraphedWindowedStep), issued eagerly otherwise.  ``keep`` (KeepRegion): its blend of the whole
        clip after the two windows kernels of every step.  ``hist``: the (panorama, perspective) x0 histories of a multistep scheduler for the
        eager loop (the graphed step owns its own).  ``next_pass`` (FreeInit): called with the two latents behind the last step; None ends the
        loop, else it returns the start latents of another run of the whole schedule (the captured step is restarted, not captured again).
        ``guidance_interval`` (None: every step guided): the unguided steps run every window on its text half (views made once, [nW, 1, ...]
        prediction buffers, ``scheduler.fused_step_windows``), and the IP-token cache holds both forms of every window's features.
        ``guidance_apg`` (``apg_eta``): handed on to the scheduler's step functions and the graphed step when it is set.
        ``guidance_apg_momentum`` (``apg_momentum``, beta): the graphed step owns the momentum states; the eager loop makes one per branch
        on the clip of blends and tracks the previous guided timestep of each pass itself."""
        from .context import ip_cache_slots
        mv, sch = self.mv_base_model, self.scheduler
        apg_kw = {} if guidance_apg is None else dict(guidance_apg=guidance_apg)
        apg_beta = guidance_apg_momentum
        guided = None if guidance_interval is None else sch.guided_steps(steps_host, guidance_interval)
        with ip_cache_slots(mv, len(plan) * (1 if guided is None else 2)):
            if self.use_graph and self.rng == "device" and pano_latent.is_cuda and trace is None and callback is None:
                from .graph_step import GraphedWindowedStep
                graphed = GraphedWindowedStep(mv, sch, inputs, cameras, pano_latent, pers_latent, g, plan, use_fps=use_fps, warmup=1,
                                              eta=eta, generator=generator, guidance_rescale=guidance_rescale,
                                              **({} if keep is None else dict(keep=keep)),
                                              **({} if guided is None else dict(guidance_interval=guidance_interval, steps=steps_host)), **apg_kw,
                                              **({} if apg_beta is None else dict(guidance_apg_momentum=apg_beta)))
                while True:
                    for t in self.progress_bar(steps_host):
                        pano_latent, pers_latent = graphed.step(t)
                    start = None if next_pass is None else next_pass(pano_latent, pers_latent)
                    if start is None:
                        return pano_latent, pers_latent
                    graphed.restart(*start)
            static = plan.static_inputs(inputs)
            preds_pers, preds_pano = plan.pred_buffers(pano_latent, pers_latent)
            if guided is not None:
                from .dist import cfg_half_inputs
                text_half, text_static = cfg_half_inputs(inputs, 1), plan.text_half(static)
                text_preds = plan.pred_buffers(pano_latent, pers_latent, halves=1)           # (perspective, panorama)
            apg_state = None if apg_beta is None else (sch.new_apg_state(pano_latent), sch.new_apg_state(pers_latent))
            while True:
                apg_prev_t = None               # the previous guided timestep of this pass: its first guided step has carry 0
                for i, t in enumerate(self.progress_bar(steps_host)):
                    if guided is not None and not guided[i]:
                        pano_latent, pers_latent = self._unguided_windows_step(plan, text_half, text_static, text_preds, pano_latent,
                                                                               pers_latent, ts_dev[i], t, cameras, use_fps, eta, generator,
                                                                               guidance_rescale, hist, **apg_kw)
                    else:
                        inputs["pano_latent"][:, :4] = pano_latent
                        inputs["latents"][:, :, :4] = pers_latent
                        plan.forward(mv, inputs, static, cameras, ts_dev[i], use_fps, preds_pers, preds_pano)
                        mdt = mv.unet.dtype
                        kw = dict(eta=eta, guidance_rescale=guidance_rescale, ring=plan.loop, **apg_kw)
                        mom = ({}, {})
                        if apg_state is not None:
                            carry = sch.apg_carry(apg_prev_t, t, apg_beta)
                            mom = tuple(dict(guidance_apg_momentum=(state, carry)) for state in apg_state)
                            apg_prev_t = t
                        z = variance_noise(sch, pano_latent, mdt, generator, self.rng) if eta > 0 else None
                        pano_latent = sch.fused_cfg_step_windows(preds_pano, plan.starts_dev, plan.weights, g, t, pano_latent, noise=z, **kw,
                                                                 **({} if hist is None else dict(history=hist[0])), **mom[0])
                        z = variance_noise(sch, pers_latent, mdt, generator, self.rng, frame_dim=3) if eta > 0 else None
                        pers_latent = sch.fused_cfg_step_windows(preds_pers, plan.starts_dev, plan.weights, g, t, pers_latent, noise=z, **kw,
                                                                 **({} if hist is None else dict(history=hist[1])), **mom[1])
                    if keep is not None:
                        keep.apply(pano_latent, pers_latent, i)
                    if trace is not None:
                        trace.append(pano_latent.clone())
                    if callback is not None and i % callback_steps == 0:
                        callback(i, t, pano_latent)
                start = None if next_pass is None else next_pass(pano_latent, pers_latent)
                if start is None:
                    return pano_latent, pers_latent
                pano_latent, pers_latent = start
