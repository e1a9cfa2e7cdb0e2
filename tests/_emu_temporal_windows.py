"""Torch stand-in of ``kernels.temporal_attention_windows`` (csrc/temporal_attn.hip: temporal_attn_windows_kernel) for the CPU tier: the
eager definition ``context.windowed_temporal_attention`` behind the wrapper's argument checks.  ``patched_temporal_windows()`` yields
the record of the calls made while the patch is active.  Also here: what the CPU and the GPU tests share -- the plans, the brute-force
fp64 reference (one Python loop per window, frame, pixel group: gather, add PE[p], plain softmax attention, weighted mean) and the
inputs."""
import contextlib
import functools

import torch

from imagine360_amd import context as CTX

# (F, L, o): the (32, 16, 10) line has three windows on some frames; the last window of the (20, 8, 3) ring wraps by 3 frames
LINE_PLANS = [(32, 16, 4), (24, 16, 4), (20, 8, 2), (32, 16, 10), (8, 4, 2), (11, 5, 1)]
RING_PLANS = [(32, 16, 4), (8, 4, 2), (20, 8, 3)]


def check_plan(F, L, starts, weights, ring):
    """What the entry point refuses, as ValueError."""
    starts = [int(s) for s in (starts.tolist() if torch.is_tensor(starts) else starts)]
    if not (1 <= F <= 64 and 1 <= L <= 16 and L <= F and 1 <= len(starts) <= 64 and len(weights) == L):
        raise ValueError(f"temporal_attention_windows: F={F}, L={L}, nW={len(starts)} outside the kernel's limits")
    for s in starts:
        if not (0 <= s < F and (ring or s + L <= F)):
            raise ValueError(f"temporal_attention_windows: window at {s} does not fit")
    if min(CTX.coverage(F, L, starts, loop=True)) < 1:
        raise ValueError("temporal_attention_windows: a frame lies in no window")


def temporal_attention_windows(qkv, pe_qkv, B, F, P, heads, starts, weights, ring=False, out=None):
    C = qkv.shape[1] // 3
    assert qkv.shape[0] == B * F * P and pe_qkv.shape == (len(weights), 3 * C) and pe_qkv.dtype == qkv.dtype
    check_plan(F, pe_qkv.shape[0], starts, weights, ring)
    o = CTX.windowed_temporal_attention(qkv, pe_qkv, B, F, P, heads, starts, weights, ring=ring)
    if out is not None:
        out.copy_(o)
        return out
    return o


@contextlib.contextmanager
def patched_temporal_windows():
    """``kernels.temporal_attention_windows`` is the stand-in; yields a list that gains (B, F, P, heads, starts, weights, ring) per call."""
    from imagine360_amd import kernels
    calls = []

    def recorded(qkv, pe_qkv, B, F, P, heads, starts, weights, ring=False, out=None):
        calls.append((B, F, P, heads, [int(s) for s in starts.tolist()], [float(w) for w in weights.tolist()], bool(ring)))
        return temporal_attention_windows(qkv, pe_qkv, B, F, P, heads, starts, weights, ring=ring, out=out)

    saved = getattr(kernels, "temporal_attention_windows", None)
    kernels.temporal_attention_windows = recorded
    try:
        yield calls
    finally:
        if saved is None:
            del kernels.temporal_attention_windows
        else:
            kernels.temporal_attention_windows = saved


def brute_force(qkv, pe_qkv, B, F, P, heads, starts, weights, ring=False):
    """The definition spelled out in fp64 with Python loops: per window the gathered rows + PE[p] rounded to the INPUT dtype, plain softmax
    attention per (batch, pixel, head), then per frame the weighted mean over the windows that hold it.  fp64 [B*F*P, C]."""
    T = qkv.dtype
    C = qkv.shape[1] // 3
    L, d = pe_qkv.shape[0], C // heads
    x = qkv.reshape(B, F, P, 3 * C)
    num = torch.zeros(B, F, P, C, dtype=torch.float64)
    den = [0.0] * F
    for s in starts:
        frames = [(s + p) % F if ring else s + p for p in range(L)]
        rows = torch.stack([(x[:, f].double() + pe_qkv[p].double()).to(T).double() for p, f in enumerate(frames)], dim=1)       # [B, L, P, 3C]
        for h in range(heads):
            q, k, v = (rows[..., i * C + h * d:i * C + (h + 1) * d].permute(0, 2, 1, 3) for i in range(3))                   # [B, P, L, d]
            o = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5, dim=-1) @ v
            for p, f in enumerate(frames):
                num[:, f, :, h * d:(h + 1) * d] += float(weights[p]) * o[:, :, p]
        for p, f in enumerate(frames):
            den[f] += float(weights[p])
    return (num / torch.tensor(den, dtype=torch.float64)[None, :, None, None]).reshape(B * F * P, C)


@functools.lru_cache(maxsize=None)
def inputs(B, F, P, heads, d, L, dt, seed=0):
    """(qkv [B*F*P, 3C], pe_qkv [L, 3C]) in ``dt`` on the host, computed once and never written to."""
    g = torch.Generator().manual_seed(4100 + seed)
    C = heads * d
    return torch.randn(B * F * P, 3 * C, generator=g).to(dt), (0.5 * torch.randn(L, 3 * C, generator=g)).to(dt)


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30))
