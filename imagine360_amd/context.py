"""Sliding temporal context windows: the plan (window start frames) and the per-position blend weights.

A clip of ``frames`` frames is denoised as overlapping windows of ``length`` frames (the length the motion modules were
trained on); per step every window is one forward of the unmodified model with frame positions 0 .. length-1, and the
windows' predictions are blended per frame -- weighted by ``context_weights`` and divided by the per-frame sum of the weights of
the windows that cover the frame -- inside the CFG + DDIM kernel (``kernels.cfg_ddim_step_windows``).

A clip that is played as a loop takes its windows on a ring (``loop=True``): window k covers the frames (s_k + j) mod frames, so the
windows that cross the end of the clip show the model ... F-2, F-1, 0, 1 ... as consecutive frames, and the last and the first frame
are blended like any other pair of neighbours.  The default is the line: no wrap-around in time.
"""
import torch

WEIGHT_KINDS = ("uniform", "pyramid")


def context_windows(frames, length, overlap, loop=False):
    """Start frames of the windows, ascending: k (length - overlap) while the window ends before the last frame, then one
    last window shifted back so that it ends on the last frame.  ``length >= frames``: the single window [0] (of ``frames``
    frames).  Every frame lies in at least one window and in at most ceil(length / (length - overlap)) + 1.
    ``loop``: the windows of a ring of ``frames`` frames -- k (length - overlap) for k = 0 .. ceil(frames / (length - overlap)) - 1,
    all below ``frames``, no shifted last window; window k covers the frames (start + j) mod frames.  Needs length < frames."""
    frames, length, overlap = int(frames), int(length), int(overlap)
    if frames < 1 or length < 1:
        raise ValueError(f"context_windows: frames={frames} and length={length} must be positive")
    if not 0 <= overlap < length:
        raise ValueError(f"context_windows: overlap={overlap} must satisfy 0 <= overlap < length={length}")
    if loop:
        if length >= frames:
            raise ValueError(f"context_windows: a looping clip needs context_frames < video_length (one window cannot wrap around), "
                             f"got length={length}, frames={frames}")
        stride = length - overlap
        return [k * stride for k in range(-(-frames // stride))]
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


def coverage(frames, length, starts, loop=False):
    """Number of windows covering each frame (list of ``frames`` ints).  ``loop``: the windows wrap around the end of the clip."""
    cov = [0] * frames
    for s in starts:
        for f in range(s, s + length):
            cov[f % frames if loop else f] += 1
    return cov


def windowed_temporal_attention(qkv, pe_qkv, B, F, P, heads, starts, weights, ring=False):
    """Eager definition of window-fused temporal attention (``context_level="attention"``; FreeNoise's window-based attention fusion,
    arXiv 2310.15169 section 3.2) -- what ``kernels.temporal_attention_windows`` computes in one launch.
    qkv [B*F*P, 3*C] in the activation dtype T, rows (batch, frame, pixel): the fused projection of LayerNorm(x) WITHOUT the frame PE;
    pe_qkv [L, 3*C] in T: PE rows 0 .. L-1 through the same projection; ``starts`` [nW] ints, ``weights`` [L].  Window k holds the
    frames f = starts[k] + p (modulo F on a ``ring``) at positions p = 0 .. L-1:
      rows       r[k, p] = round_T(float(qkv[f]) + float(pe_qkv[p]))       -- the position restarts in every window: PE[p], never PE[f]
      attention  o[k, p] = softmax(scale q k^T) v over the window's L rows, per (batch, pixel, head)
      fusion     out[f]  = sum over the windows holding f of w[p] / (sum of their w[p']) * o[k, p], rounded to T once.
    The arithmetic runs in float32 for 16-bit inputs and in the inputs' own dtype otherwise (float64 in: the reference of the tests).
    Returns [B*F*P, C] in qkv's dtype."""
    starts = [int(s) for s in (starts.tolist() if torch.is_tensor(starts) else starts)]
    T = qkv.dtype
    wide = torch.float32 if T in (torch.bfloat16, torch.float16) else T
    C = qkv.shape[1] // 3
    L, d = pe_qkv.shape[0], C // heads
    assert qkv.shape == (B * F * P, 3 * C) and pe_qkv.shape == (L, 3 * C) and len(weights) == L and len(starts) >= 1
    w = torch.as_tensor(weights).to(device=qkv.device, dtype=wide)
    x = qkv.reshape(B, F, P, 3 * C)
    pos = torch.arange(L, device=qkv.device)
    acc = torch.zeros(B, F, P, C, dtype=wide, device=qkv.device)
    wsum = torch.zeros(F, dtype=wide, device=qkv.device)
    for s in starts:
        if not (0 <= s < F and L <= F and (ring or s + L <= F)):
            raise ValueError(f"windowed_temporal_attention: window at {s} of {L} frames does not fit {F} frames (ring={bool(ring)})")
        wsum.index_add_(0, (s + pos) % F, w)
    if not bool((wsum > 0).all()):
        raise ValueError(f"windowed_temporal_attention: frames {(wsum <= 0).nonzero().flatten().tolist()} lie in no window")
    for s in starts:
        f = (s + pos) % F
        r =(x[:, f].to(wide) + pe_qkv.to(wide)[None, :, None, :]).to(T).to(wide)                 # [B, L, P, 3C]
        q, k, v = (t.reshape(B, L, P, heads, d).permute(0, 2, 3, 1, 4) for t in r.split(C, dim=-1))        # [B, P, heads, L, d]
        o = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1) @ v
        acc.index_add_(1, f, o.permute(0, 3, 1, 2, 4).reshape(B, L, P, C) * (w / wsum[f])[None, :, None, None])
    return acc.to(T).reshape(B * F * P, C)


def keyframe_frames(f, F, loop=False):
    """The frames of a clip retimed from ``f`` to ``F`` frames (``pano_geometry.retime_pano_latent``) that ARE source frames (t == 0),
    ascending: the j with j (f - 1) divisible by max(F - 1, 1) on an open clip, with j f divisible by F on a ring (``loop``).  The
    even frames for F = 2 f - 1 (open) and F = 2 f (ring); the first and the last frame alone when f - 1 and F - 1 share no factor."""
    f, F = int(f), int(F)
    if not 1 <= f <= F:
        raise ValueError(f"keyframe_frames: needs 1 <= f <= F, got f={f}, F={F}")
    num, den = (f, F) if loop else (f - 1, max(F - 1, 1))
    return [j for j in range(F) if (j * num) % den == 0]


def keyframe_mask(f, F, loop=False):
    """A ``regenerate_mask`` [1, F, 1, 1, 1] (float32; ``prepare_regenerate_mask`` resizes it to the latent) for a frame-interpolation
    pass: 0 (keep) at ``keyframe_frames(f, F, loop)``, 1 (regenerate) at the frames in between."""
    m = torch.ones(1, int(F), 1, 1, 1, dtype=torch.float32)
    m[0, keyframe_frames(f, F, loop)] = 0.0
    return m


def keyframe_strength(f, F, loop=False, floor=0.0):
    """The soft sibling of ``keyframe_mask`` for ``regenerate_mode="release"``: a strength map [1, F, 1, 1, 1] (float32) that is 0
    (pinned to the end) at ``keyframe_frames(f, F, loop)`` and rises linearly with the distance in frames to the nearest source
    frame, reaching 1 midway between two neighbouring source frames -- an in-between next to a keyframe is released late and
    changes little, the one in the middle of a gap is free for the whole run.  On a ring (``loop``) the distance wraps: the gap
    behind the last source frame closes at frame 0.  ``floor`` in [0, 1]: the lowest value a frame that is NOT a source frame may get
    (every in-between is then free for at least the last ``floor`` of the steps)."""
    floor = float(floor)
    if not 0.0 <= floor <= 1.0:
        raise ValueError(f"keyframe_strength: floor must be in [0, 1], got {floor}")
    F = int(F)
    keys = keyframe_frames(f, F, loop)
    m = torch.zeros(1, F, 1, 1, 1, dtype=torch.float32)
    ends = keys + [keys[0] + F] if loop else keys
    for a, b in zip(ends[:-1], ends[1:]):                       # the frames strictly between two neighbouring source frames
        for j in range(a + 1, b):
            m[0, j % F] = max(floor, min(2.0 * min(j - a, b - j) / (b - a), 1.0))
    if not loop:
        # (an open clip starts and ends on a source frame, keyframe_frames: nothing lies outside the gaps)
        assert keys[0] == 0 and keys[-1] == F - 1
    return m


class WindowPlan:
    """The windows of one clip: ``starts`` (host ints), ``length``, the device tables the blend kernel reads, and the per-window
    model inputs.  ``inputs``: the keyword tensors of MultiViewBaseModel.forward for the WHOLE clip.  ``loop``: the windows of a
    ring (context_windows(loop=True)); ``frame_index[k]`` is then the device int64 vector (s_k + arange(L)) % F of window k's frames,
    and a window that crosses the end of the clip is cut with one ``index_select`` per tensor instead of a slice view."""

    def __init__(self, frames, length, overlap=4, kind="pyramid", device="cpu", loop=False):
        self.frames, self.length = int(frames), window_length(frames, length)
        self.loop = bool(loop)
        self.starts = context_windows(frames, length, overlap, loop=True) if self.loop else context_windows(frames, length, overlap)
        self.kind = kind
        self.weights = context_weights(self.length, kind).to(device)
        self.starts_dev = torch.tensor(self.starts, dtype=torch.int32, device=device)
        self.frame_index = None
        if self.loop:
            self.frame_index = [(s + torch.arange(self.length, dtype=torch.int64, device=device)) % self.frames for s in self.starts]

    def __len__(self):
        return len(self.starts)

    def wraps(self, k):
        """True when window k crosses the end of the clip (looping plans only)."""
        return self.starts[k] + self.length > self.frames

    def _cut(self, x, dim, k):
        """Window k's frames of ``x`` along ``dim``: the slice view, or -- the window wraps -- one gather."""
        if self.wraps(k):
            return x.index_select(dim, self.frame_index[k])
        return x.narrow(dim, self.starts[k], self.length)

    def static_inputs(self, inputs):
        """Per window, the step-invariant frame-indexed conditioning cut to the window's frames: the SAM features as one
        contiguous tensor per window (the model caches the IP tokens it derives from them on the tensor's identity; the
        perspective one keeps its stride-0 view axis), crop rectangles and pitches as views.  A window that wraps gathers all
        four here, once."""
        out = []
        for k, s in enumerate(self.starts):
            e = s + self.length
            fp = inputs["reference_images_clip_feat_pers"]
            shared = fp.stride(1) == 0
            rel, pitch = inputs["relative_position_tensor"], inputs["pitchs_tensor"]
            if self.wraps(k):
                fp_w = (self._cut(fp[:, 0], 1, k).unsqueeze(1).expand(-1, fp.shape[1], -1, -1, -1) if shared else self._cut(fp, 2, k))
                out.append(dict(reference_images_clip_feat_pano=self._cut(inputs["reference_images_clip_feat_pano"], 1, k),
                                reference_images_clip_feat_pers=fp_w,
                                relative_position_tensor=None if rel is None else self._cut(rel, 1, k),
                                pitchs_tensor=None if pitch is None else self._cut(pitch, 1, k)))
                continue
            fp_w = (fp[:, 0, s:e].contiguous().unsqueeze(1).expand(-1, fp.shape[1], -1, -1, -1) if shared
                    else fp[:, :, s:e].contiguous())
            out.append(dict(reference_images_clip_feat_pano=inputs["reference_images_clip_feat_pano"][:, s:e].contiguous(),
                            reference_images_clip_feat_pers=fp_w,
                            relative_position_tensor=None if rel is None else rel[:, s:e],
                            pitchs_tensor=None if pitch is None else pitch[:, s:e]))
        return out

    def forward(self, mv, inputs, static, cameras, timestep, use_fps, preds_pers, preds_pano, coins=None):
        """One forward of the unmodified model per window, ascending: window k sees frames s_k .. s_k + L - 1 (on a ring: modulo
        F; a window that wraps gathers them with one index_select per input, every call -- their first four channels change) of both
        model inputs (``inputs["latents"]`` [2,m,9,F,h,w], ``inputs["pano_latent"]`` [2,9,F,H,W]) and ``static[k]``; text embeddings,
        fps and cameras are shared.  Its CFG-batched predictions go to slot k of ``preds_pers`` [nW,2,m,4,L,h,w] / ``preds_pano``
        [nW,2,4,L,H,W] (cast to their dtype by the copy).  Each call draws its IP-adapter noise (panorama, perspective) and its
        seven WarpAttn coins, like nW successive calls of the model; ``coins`` [nW, 8] device int32: preloaded coins, row k for
        window k (captured steps)."""
        saved = mv._coins_dev, mv.coins_preloaded
        try:
            for k in range(len(self.starts)):
                if coins is not None:
                    mv._coins_dev, mv.coins_preloaded = coins[k], True
                pred_pers, pred_pano = mv(
                    latents=self._cut(inputs["latents"], 3, k), pano_latent=self._cut(inputs["pano_latent"], 2, k),
                    timestep=timestep, prompt_embd=inputs["prompt_embd"], pano_prompt_embd=inputs["pano_prompt_embd"],
                    cameras=cameras, use_fps_condition=use_fps, use_ip_plus_cross_attention=True,
                    fps_tensor_pano=inputs["fps_tensor_pano"], fps_tensor_pers=inputs["fps_tensor_pers"], **static[k])
                preds_pano[k].copy_(pred_pano)
                preds_pers[k].copy_(pred_pers)
        finally:
            if coins is not None:
                mv._coins_dev, mv.coins_preloaded = saved

    def pred_buffers(self, pano_latent, pers_latent, halves=2):
        """Empty [nW, 2, ...] prediction buffers in the latents' dtype and layout with L frames; ``halves=1``: [nW, 1, ...], for the
        steps that run the text half alone (pipeline ``guidance_interval``)."""
        nW, L = len(self), self.length
        ps, qs = list(pano_latent.shape), list(pers_latent.shape)
        ps[2], qs[3] = L, L
        return (pers_latent.new_empty((nW, halves, *qs[1:])), pano_latent.new_empty((nW, halves, *ps[1:])))

    @staticmethod
    def text_half(static):
        """``static_inputs`` for a forward of the text half alone (pipeline ``guidance_interval``): per window the second CFG row of
        every tensor, as views.  Made ONCE per run and kept: the model caches the IP tokens on the feature tensors' identity, and
        ``ip_cache_slots(mv, 2 * len(plan))`` holds both forms of every window at once."""
        return [{k: (None if v is None else v[1:2]) for k, v in st.items()} for st in static]


class ip_cache_slots:
    """Context manager: both UNets of ``mv`` keep the IP tokens of ``n`` feature tensors (one per window; with a guidance interval
    two per window, the CFG batch and its text half, and two without windows) instead of one; on exit the single-entry behaviour
    and memory footprint are restored."""

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
