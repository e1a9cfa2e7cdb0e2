"""Sliding temporal context windows: the plan (window start frames) and the per-position blend weights.

A clip of ``frames`` frames is denoised as overlapping windows of ``length`` frames (the length the motion modules were
trained on); per step every window is one forward of the unmodified model with frame positions 0 .. length-1, and the
windows' predictions are blended per frame -- weighted by ``context_weights`` and divided by the per-frame sum of the weights of
the windows that cover the frame -- inside the CFG + DDIM kernel (``kernels.cfg_ddim_step_windows``).  No wrap-around in time.
"""
import torch

WEIGHT_KINDS = ("uniform", "pyramid")


def context_windows(frames, length, overlap):
    """Start frames of the windows, ascending: k (length - overlap) while the window ends before the last frame, then one
    last window shifted back so that it ends on the last frame.  ``length >= frames``: the single window [0] (of ``frames``
    frames).  Every frame lies in at least one window and in at most ceil(length / (length - overlap)) + 1."""
    frames, length, overlap = int(frames), int(length), int(overlap)
    if frames < 1 or length < 1:
        raise ValueError(f"context_windows: frames={frames} and length={length} must be positive")
    if not 0 <= overlap < length:
        raise ValueError(f"context_windows: overlap={overlap} must satisfy 0 <= overlap < length={length}")
    if length >= frames:
        return [0]
    stride = length - overlap
    starts = []
    s = 0
    while s + length < frames:
        starts.append(s)
        s += stride
    starts.append(frames - length)
    return starts


def window_length(frames, length):
    """Frames per window: ``length`` clipped to the clip."""
    return min(int(frames), int(length))


def context_weights(length, kind="pyramid"):
    """float32 [length] blend weight of each position inside a window: "uniform" all 1, "pyramid" min(j + 1, length - j)
    (window centres count more than window edges).  Only ratios matter: the blend normalises per frame."""
    length = int(length)
    if length < 1:
        raise ValueError(f"context_weights: length={length} must be positive")
    if kind == "uniform":
        return torch.ones(length, dtype=torch.float32)
    if kind == "pyramid":
        j = torch.arange(length)
        return torch.minimum(j + 1, length - j).to(torch.float32)
    raise ValueError(f"context_weights: kind {kind!r} must be one of {WEIGHT_KINDS}")


def coverage(frames, length, starts):
    """Number of windows covering each frame (list of ``frames`` ints)."""
    cov = [0] * frames
    for s in starts:
        for f in range(s, s + length):
            cov[f] += 1
    return cov


class WindowPlan:
    """The windows of one clip: ``starts`` (host ints), ``length``, the device tables the blend kernel reads, and the per-window
    model inputs.  ``inputs``: the keyword tensors of MultiViewBaseModel.forward for the WHOLE clip."""

    def __init__(self, frames, length, overlap=4, kind="pyramid", device="cpu"):
        self.frames, self.length = int(frames), window_length(frames, length)
        self.starts = context_windows(frames, length, overlap)
        self.kind = kind
        self.weights = context_weights(self.length, kind).to(device)
        self.starts_dev = torch.tensor(self.starts, dtype=torch.int32, device=device)

    def __len__(self):
        return len(self.starts)

    def static_inputs(self, inputs):
        """Per window, the step-invariant frame-indexed conditioning cut to the window's frames: the SAM features as one
        contiguous tensor per window (the model caches the IP tokens it derives from them on the tensor's identity; the
        perspective one keeps its stride-0 view axis), crop rectangles and pitches as views."""
        out = []
        for s in self.starts:
            e = s + self.length
            fp = inputs["reference_images_clip_feat_pers"]
            shared = fp.stride(1) == 0
            fp_w = (fp[:, 0, s:e].contiguous().unsqueeze(1).expand(-1, fp.shape[1], -1, -1, -1) if shared
                    else fp[:, :, s:e].contiguous())
            rel, pitch = inputs["relative_position_tensor"], inputs["pitchs_tensor"]
            out.append(dict(reference_images_clip_feat_pano=inputs["reference_images_clip_feat_pano"][:, s:e].contiguous(),
                            reference_images_clip_feat_pers=fp_w,
                            relative_position_tensor=None if rel is None else rel[:, s:e],
                            pitchs_tensor=None if pitch is None else pitch[:, s:e]))
        return out

    def forward(self, mv, inputs, static, cameras, timestep, use_fps, preds_pers, preds_pano, coins=None):
        """One forward of the unmodified model per window, ascending: window k sees frames s_k .. s_k + L - 1 of both model
        inputs (``inputs["latents"]`` [2,m,9,F,h,w], ``inputs["pano_latent"]`` [2,9,F,H,W]) and ``static[k]``; text embeddings,
        fps and cameras are shared.  Its CFG-batched predictions go to slot k of ``preds_pers`` [nW,2,m,4,L,h,w] / ``preds_pano``
        [nW,2,4,L,H,W] (cast to their dtype by the copy).  Each call draws its IP-adapter noise (panorama, perspective) and its
        seven WarpAttn coins, like nW successive calls of the model; ``coins`` [nW, 8] device int32: preloaded coins, row k for
        window k (captured steps)."""
        L = self.length
        saved = mv._coins_dev, mv.coins_preloaded
        try:
            for k, s in enumerate(self.starts):
                if coins is not None:
                    mv._coins_dev, mv.coins_preloaded = coins[k], True
                pred_pers, pred_pano = mv(
                    latents=inputs["latents"][:, :, :, s:s + L], pano_latent=inputs["pano_latent"][:, :, s:s + L],
                    timestep=timestep, prompt_embd=inputs["prompt_embd"], pano_prompt_embd=inputs["pano_prompt_embd"],
                    cameras=cameras, use_fps_condition=use_fps, use_ip_plus_cross_attention=True,
                    fps_tensor_pano=inputs["fps_tensor_pano"], fps_tensor_pers=inputs["fps_tensor_pers"], **static[k])
                preds_pano[k].copy_(pred_pano)
                preds_pers[k].copy_(pred_pers)
        finally:
            if coins is not None:
                mv._coins_dev, mv.coins_preloaded = saved

    def pred_buffers(self, pano_latent, pers_latent):
        """Empty [nW, 2, ...] prediction buffers in the latents' dtype and layout with L frames."""
        nW, L = len(self), self.length
        ps, qs = list(pano_latent.shape), list(pers_latent.shape)
        ps[2], qs[3] = L, L
        return (pers_latent.new_empty((nW, 2, *qs[1:])), pano_latent.new_empty((nW, 2, *ps[1:])))


class ip_cache_slots:
    """Context manager: both UNets of ``mv`` keep the IP tokens of ``n`` feature tensors (one per window) instead of one; on
    exit the single-entry behaviour and memory footprint are restored."""

    def __init__(self, mv, n):
        self.unets, self.n = (mv.unet, mv.pano_unet), int(n)

    def __enter__(self):
        for u in self.unets:
            u.ip_cache_entries = self.n
        return self

    def __exit__(self, *exc):
        for u in self.unets:
            u.ip_cache_entries = 1
            store = u._ip_cache._store
            for k in [k for k in store if isinstance(k, tuple) and k[0] == "ip"]:
                del store[k]
        return False
