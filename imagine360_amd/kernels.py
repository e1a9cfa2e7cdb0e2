"""torch-tensor front end of libim360_kernels.so (C ABI in include/im360_kernels.h).

Every function here launches a hand-written gfx950 kernel on ``torch.cuda.current_stream()``.
There is NO fallback: a missing library or a non-GPU tensor raises.  Model code calls these
through the module (``kernels.attention(...)``).
"""
import ctypes
import math
import os

import torch

# IM360_KERNELS_LIB: another build of the SAME library for the A/B tools (`make -C csrc ablate-lib` -> libim360_kernels_ablate.so:
# the shipped kernels plus the measured-and-rejected variants); never a different implementation
_LIB_PATH = os.environ.get("IM360_KERNELS_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libim360_kernels.so")
_lib = None

_I64, _F32, _INT, _PTR = ctypes.c_int64, ctypes.c_float, ctypes.c_int, ctypes.c_void_p

_SIGNATURES = {
    "im360_abi_version": (_INT, []),
    "im360_build_flags": (_INT, []),
    "im360_last_error": (ctypes.c_char_p, []),
    "im360_attn_fwd": (_INT, [_PTR] * 5 + [_I64] * 15 + [_F32, _F32, _INT, _INT, _PTR, _PTR, _PTR, _PTR, _PTR, _I64]),
    "im360_attn_fwd2": (_INT, [_PTR] * 6 + [_I64] * 19 + [_F32, _F32, _F32, _INT, _PTR]),
    "im360_temporal_attn_fwd": (_INT, [_PTR] * 4 + [_I64] * 11 + [_F32, _INT, _PTR]),
    "im360_temporal_attn_windows_fwd": (_INT, [_PTR] * 5 + [_I64] * 11 + [_PTR, _I64, _PTR, _I64, _INT, _F32, _INT, _PTR]),
    "im360_shard_pack": (_INT, [_PTR] * 2 + [_I64] * 6 + [_INT, _PTR]),
    "im360_gn_num_slabs": (_I64, [_I64] * 3),
    "im360_groupnorm_stats": (_INT, [_PTR] * 6 + [_I64] * 6 + [_F32, _INT, _PTR]),
    "im360_groupnorm_apply": (_INT, [_PTR] * 4 + [_I64] * 5 + [_INT, _INT, _PTR]),
    "im360_groupnorm_stats_cat": (_INT, [_PTR] * 7 + [_I64] * 7 + [_F32, _INT, _PTR]),
    "im360_groupnorm_fused": (_INT, [_PTR] * 7 + [_I64] * 7 + [_F32, _INT, _INT, _PTR]),
    "im360_groupnorm_apply_cat": (_INT, [_PTR] * 5 + [_I64] * 6 + [_INT, _INT, _PTR]),
    "im360_conv1x1_cat_fwd": (_INT, [_PTR] * 6 + [_I64] * 6 + [_INT, _PTR]),
    "im360_linear_fwd": (_INT, [_PTR] * 6 + [_I64] * 3 + [_INT, _PTR, _PTR]),
    "im360_linear_ln_fwd": (_INT, [_PTR] * 5 + [_I64, _F32, _PTR, _I64, _I64, _PTR] + [_I64] * 3 + [_INT, _PTR]),
    "im360_linear_geglu_ln": (_INT, [_PTR] * 5 + [_I64, _F32, _PTR] + [_I64] * 3 + [_INT, _PTR]),
    "im360_conv_fwd": (_INT, [_PTR] * 6 + [_I64] * 14 + [_INT, _PTR, _PTR]),
    "im360_conv_gn_slabs": (_I64, [_I64] * 6),
    "im360_conv_ksplit_plan": (_I64, [_I64] * 9),
    "im360_conv_fwd_ksplit": (_INT, [_PTR] * 6 + [_I64] * 14 + [_INT, _PTR, _PTR] + [_PTR, _I64, _PTR, _I64]),
    "im360_groupnorm_partial": (_INT, [_PTR] * 2 + [_I64] * 4 + [_INT, _PTR]),
    "im360_groupnorm_finalize": (_INT, [_PTR, _I64, _I64, _PTR, _I64, _I64] + [_PTR] * 4 + [_I64] * 3 + [_F32, _INT, _PTR]),
    "im360_groupnorm_partial_pad": (_INT, [_PTR] * 2 + [_I64] * 5 + [_INT, _PTR]),
    "im360_groupnorm_apply_partials": (_INT, [_PTR, _PTR, _PTR, _I64, _PTR, _I64, _PTR, _PTR, _PTR] + [_I64] * 7 + [_F32, _INT, _INT, _PTR]),
    "im360_pack_conv_weight": (_INT, [_PTR] * 2 + [_I64] * 5 + [_INT, _PTR]),
    "im360_attn_pack_bias": (_INT, [_PTR] * 2 + [_I64, _INT, _PTR]),
    "im360_conv_up2_fwd": (_INT, [_PTR] * 4 + [_I64] * 6 + [_INT, _PTR]),
    "im360_remap_cubic_wrap_u8": (_INT, [_PTR] * 5 + [_I64] * 7 + [_PTR]),
    "im360_max_rect": (_INT, [_PTR, _I64, _I64, _PTR]),
    "im360_circular_pad_w": (_INT, [_PTR] * 2 + [_I64] * 4 + [_INT, _PTR]),
    "im360_circular_pad_hw": (_INT, [_PTR] * 2 + [_I64] * 8 + [_PTR]),
    "im360_cfg_ddim_update": (_INT, [_PTR] * 4 + [_I64] + [_F32] * 3 + [_INT, _PTR, _PTR]),
    "im360_cfg_ddim_step": (_INT, [_PTR] * 5 + [_I64] + [_F32] * 6 + [_INT, _INT, _PTR, _PTR]),
    "im360_cfg_ddim_step_windows": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 4 + [_F32] * 6 + [_INT, _INT, _PTR, _PTR]),
    "im360_cfg_rescale_records": (_I64, [_I64]),
    "im360_cfg_rescale_stats": (_INT, [_PTR] * 2 + [_I64, _F32, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_rescale_stats_windows": (_INT, [_PTR] * 3 + [_INT] + [_I64] * 4 + [_F32, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_rescale_factor": (_INT, [_PTR, _I64, _I64, _F32, _PTR, _PTR]),
    "im360_cfg_ddim_step_rescale": (_INT, [_PTR] * 5 + [_I64] + [_F32] * 6 + [_INT, _F32, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_ddim_step_windows_rescale": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 4 + [_F32] * 6 + [_INT, _F32, _PTR, _I64, _INT, _PTR,
                                                                                                  _PTR]),
    "im360_cfg_ddim_step_windows_ring": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 4 + [_F32] * 6 + [_INT, _INT, _PTR, _PTR]),
    "im360_cfg_rescale_stats_windows_ring": (_INT, [_PTR] * 3 + [_INT] + [_I64] * 4 + [_F32, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_ddim_step_windows_ring_rescale": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 4 + [_F32] * 6 + [_INT, _F32, _PTR, _I64, _INT,
                                                                                                       _PTR, _PTR]),
    "im360_cfg_multistep_step": (_INT, [_PTR] * 5 + [_I64] + [_F32] * 6 + [_INT, _F32, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_multistep_step_windows": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 5 + [_F32] * 6 + [_INT, _F32, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_ddim_update": (_INT, [_PTR] * 3 + [_I64] + [_F32] * 2 + [_INT, _PTR, _PTR]),
    "im360_ddim_step": (_INT, [_PTR] * 4 + [_I64] + [_F32] * 5 + [_INT, _INT, _PTR, _PTR]),
    "im360_ddim_step_windows": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 4 + [_F32] * 5 + [_INT, _INT, _PTR, _PTR]),
    "im360_ddim_step_windows_ring": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 4 + [_F32] * 5 + [_INT, _INT, _PTR, _PTR]),
    "im360_multistep_step": (_INT, [_PTR] * 4 + [_I64] + [_F32] * 5 + [_INT, _INT, _PTR, _PTR]),
    "im360_multistep_step_windows": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 5 + [_F32] * 5 + [_INT, _INT, _PTR, _PTR]),
    "im360_cfg_apg_stats": (_INT, [_PTR] * 3 + [_I64, _F32, _F32, _INT, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_apg_stats_windows": (_INT, [_PTR] * 4 + [_INT] + [_I64] * 4 + [_F32, _F32, _INT, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_apg_stats_windows_ring": (_INT, [_PTR] * 4 + [_INT] + [_I64] * 4 + [_F32, _F32, _INT, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_apg_scalars": (_INT, [_PTR, _I64, _I64] + [_F32] * 3 + [_INT, _F32, _F32, _PTR, _PTR, _PTR]),
    "im360_cfg_ddim_step_apg": (_INT, [_PTR] * 5 + [_I64] + [_F32] * 6 + [_INT, _F32, _F32, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_ddim_step_windows_apg": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 5 + [_F32] * 6 + [_INT, _F32, _F32, _PTR, _I64, _INT, _PTR,
                                                                                              _PTR]),
    "im360_cfg_multistep_step_apg": (_INT, [_PTR] * 5 + [_I64] + [_F32] * 6 + [_INT, _F32, _F32, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_multistep_step_windows_apg": (_INT, [_PTR] * 6 + [_INT] + [_I64] * 5 + [_F32] * 6 + [_INT, _F32, _F32, _PTR, _I64, _INT,
                                                                                                   _PTR, _PTR]),
    "im360_cfg_apg_momentum_stats": (_INT, [_PTR] * 4 + [_I64, _F32, _F32, _INT, _F32, _PTR, _PTR, _I64, _INT, _PTR, _PTR]),
    "im360_cfg_apg_momentum_stats_windows": (_INT, [_PTR] * 5 + [_INT] + [_I64] * 4 + [_F32, _F32, _INT, _F32, _PTR, _PTR, _I64, _INT, _PTR,
                                                                                        _PTR]),
    "im360_cfg_apg_momentum_stats_windows_ring": (_INT, [_PTR] * 5 + [_INT] + [_I64] * 4 + [_F32, _F32, _INT, _F32, _PTR, _PTR, _I64, _INT,
                                                                                             _PTR, _PTR]),
    "im360_cfg_ddim_step_apg_momentum": (_INT, [_PTR] * 6 + [_I64] + [_F32] * 6 + [_INT, _F32, _F32, _PTR, _I64, _F32, _PTR, _INT, _PTR,
                                                                                   _PTR]),
    "im360_cfg_ddim_step_windows_apg_momentum": (_INT, [_PTR] * 7 + [_INT] + [_I64] * 5 + [_F32] * 6 + [_INT, _F32, _F32, _PTR, _I64, _F32,
                                                                                                        _PTR, _INT, _PTR, _PTR]),
    "im360_cfg_multistep_step_apg_momentum": (_INT, [_PTR] * 6 + [_I64] + [_F32] * 6 + [_INT, _F32, _F32, _PTR, _I64, _F32, _PTR, _INT,
                                                                                        _PTR, _PTR]),
    "im360_cfg_multistep_step_windows_apg_momentum": (_INT, [_PTR] * 7 + [_INT] + [_I64] * 5 + [_F32] * 6 + [_INT, _F32, _F32, _PTR, _I64,
                                                                                                             _F32, _PTR, _INT, _PTR, _PTR]),
    "im360_noise_latents": (_INT, [_PTR] * 6 + [_I64] * 5 + [_F32, _F32, _INT, _PTR]),
    "im360_keep_latents": (_INT, [_PTR] * 7 + [_I64] * 5 + [_F32, _F32, _INT, _PTR, _PTR]),
    "im360_keep_latents_release": (_INT, [_PTR] * 7 + [_I64] * 5 + [_F32, _F32, _F32, _INT, _PTR, _PTR]),
    "im360_sphere_distance2": (_INT, [_PTR] * 3 + [_I64] * 2 + [_PTR]),
    "im360_resize_pano_latent": (_INT, [_PTR] * 2 + [_I64] * 6 + [_INT, _INT, _PTR]),
    "im360_retime_pano_latent": (_INT, [_PTR] * 2 + [_I64] * 4 + [_INT, _INT, _INT, _PTR]),
    "im360_free_init_noise": (_INT, [_PTR] * 8 + [_I64] * 5 + [_F32] * 3 + [_INT, _PTR]),
    "im360_layernorm": (_INT, [_PTR] * 6 + [_I64] * 5 + [_F32, _INT, _PTR]),
    "im360_geglu": (_INT, [_PTR] * 2 + [_I64] * 2 + [_INT, _PTR]),
    "im360_linear_geglu": (_INT, [_PTR] * 4 + [_I64] * 3 + [_INT, _PTR]),
    "im360_ff_fused": (_INT, [_PTR] * 6 + [_I64, _F32] + [_PTR] * 4 + [_I64] * 4 + [_INT, _PTR]),
    "im360_softmax_rows": (_INT, [_PTR] * 2 + [_I64] * 4 + [_F32, _INT, _PTR]),
    "im360_tuning_set": (_INT, [_INT, _INT]),
    "im360_tuning_get": (_INT, [_INT]),
    "im360_prof_enable": (None, [ctypes.c_uint]),
    "im360_prof_collect": (_INT, [_INT, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]),
}

ABI_VERSION = 5          # include/im360_kernels.h: what im360_abi_version() of a matching library returns

PROF_KINDS = {"attn": 0, "temporal": 1, "conv": 2, "gn_stats": 3, "gn_apply": 4, "misc": 5, "gemm": 6, "attn_warp": 7, "attn_x2": 8}


# Algorithmic work of the launches, by class (bench.py's roofline legs): None = off, else {class: [flops, bytes, launches]}
STATS = None


# Launch mix by shape (bench.py weights the measured HBM traffic of tools/hbm_traffic.py with it): None = off, else
# {(class, shape key): [launches, algorithmic bytes]}
SHAPES = None


def _count(kind, flops, nbytes, executed=None, shape=None):
    """``flops``: the reference algorithm's flops of the launch; ``executed``: what the kernel actually multiplies when it
    differs (the sub-pixel upsample convolutions run 4 / 9 of them) -- hardware utilisation is priced on executed flops.
    ``shape``: a key naming the launch's shape class (token count excluded), for the launch-mix statistics."""
    if STATS is not None:
        s = STATS.setdefault(kind, [0.0, 0.0, 0, 0.0])
        s[0] += flops
        s[1] += nbytes
        s[2] += 1
        s[3] += flops if executed is None else executed
    if SHAPES is not None and shape is not None:
        h = SHAPES.setdefault((kind, shape), [0, 0.0])
        h[0] += 1
        h[1] += nbytes


def exported_symbols():
    return sorted(_SIGNATURES)


def lib():
    """Load libim360_kernels.so (built by ``__graft_entry__.build()`` / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} is missing: build it with `make -C imagine360_amd/csrc` "
                               "(hipcc --offload-arch=gfx950); imagine360_amd has no CPU fallback")
        L = ctypes.CDLL(_LIB_PATH)
        # the version first: a stale library that lacks a newer symbol must fail with the rebuild message, not with an
        # AttributeError from the loop below
        try:
            ver = L.im360_abi_version
        except AttributeError:
            raise RuntimeError(f"{_LIB_PATH} exports no im360_abi_version: rebuild it with `make -C imagine360_amd/csrc`") from None
        ver.restype, ver.argtypes = _SIGNATURES["im360_abi_version"]
        have = ver()
        if have != ABI_VERSION:
            # (version 1 -> 2 added a trailing pointer to two entry points; a stale library would read garbage for it)
            raise RuntimeError(f"{_LIB_PATH} reports C-ABI version {have}, this binding is written for version {ABI_VERSION}: "
                               "rebuild it with `make -C imagine360_amd/csrc`")
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {lib().im360_last_error().decode()}")


def _dt(t):
    if t.dtype == torch.bfloat16:
        return 0
    if t.dtype == torch.float16:
        return 1
    raise TypeError(f"imagine360_amd kernels take bfloat16/float16 tensors, got {t.dtype}")


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("imagine360_amd kernels need tensors on the MI355X (cuda) device; no CPU fallback")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------ attention
def pack_attn_bias(bias):
    """bias (16-bit, any shape) -> fp16 ``bias * log2(e)`` clamped to +-60000 (finite: -inf masks become an exact zero
    weight instead of poisoning the identity-slice MFMA that adds them): the form ``attention(..., bias_packed=True)``
    feeds to the matrix pipe (head dim 32, Nk % 8 == 0).  Once per cached mask."""
    _dev(bias)
    b = bias.contiguous()
    out = torch.empty(b.shape, dtype=torch.float16, device=b.device)
    _check(lib().im360_attn_pack_bias(_p(b), _p(out), b.numel(), _dt(b), _stream()), "im360_attn_pack_bias")
    return out


def attn_bias_blocks(packed):
    """Block map of a packed bias matrix [Nq, Nk] (fp16, ``pack_attn_bias``): int32 [ceil(Nq / 32), ceil(Nk / 1024)], bit h % 32 of
    word h // 32 of row r is set when the 32 x 32 block (query rows 32 r .., keys 32 h ..) holds a non-zero entry.  The attention
    kernel skips the bias of blocks whose bit is clear; WarpAttn shifts its masks so that the background is exactly zero
    (softmax is invariant under a per-row constant)."""
    nq, nk = packed.shape
    rq, rk = -(-nq // 32), -(-nk // 32)
    nz = torch.zeros((rq * 32, rk * 32), dtype=torch.bool, device=packed.device)
    nz[:nq, :nk] = packed != 0
    blocks = nz.view(rq, 32, rk, 32).any(dim=3).any(dim=1)                      # [rq, rk]
    words = -(-rk // 32)
    bits = torch.zeros((rq, words * 32), dtype=torch.int64, device=packed.device)
    bits[:, :rk] = blocks.to(torch.int64)
    w = (bits.view(rq, words, 32) << torch.arange(32, device=packed.device, dtype=torch.int64)).sum(dim=2)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).contiguous()


def can_pack_attn_bias(d, nk):
    return d == 32 and nk % 8 == 0


def attention(q, k, v, heads, scale=None, bias=None, out=None, accumulate=False, out_scale=1.0, kv_group=1,
              bias_alt=None, bias_sel=None, bias_packed=False, bias_blocks=None, bias_blocks_alt=None):
    """q [B, Nq, heads*d], k/v [B / kv_group, Nk, heads*d] (last dim contiguous, any row/batch stride),
    bias [Nq, Nk] shared by every (batch, head); with ``bias_sel`` (device int32 scalar) the kernel picks
    ``bias_alt`` when it is non-zero.  ``bias_packed``: bias / bias_alt come from ``pack_attn_bias``; ``bias_blocks`` /
    ``bias_blocks_alt``: their block maps (``attn_bias_blocks``) -- 32 x 32 blocks of zeros are skipped.
    Returns out [B, Nq, heads*d]."""
    _dev(q, k, v, bias, out)
    B, Nq, C = q.shape
    Nk = k.shape[1]
    d = C // heads
    assert k.shape[0] * kv_group == B and v.shape[0] == k.shape[0] and v.shape[1] == Nk and k.shape[2] == C and v.shape[2] == C
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    if out is None:
        assert not accumulate
        out = torch.empty((B, Nq, C), dtype=q.dtype, device=q.device)
    else:
        _written(out)
    assert out.stride(2) == 1
    if bias is not None:
        assert bias.shape == (Nq, Nk) and bias.stride(1) == 1 and bias.dtype == (torch.float16 if bias_packed else q.dtype)
        assert bias_alt is None or bias_alt.dtype == bias.dtype
    if scale is None:
        scale = d ** -0.5
    rc = lib().im360_attn_fwd(_p(q), _p(k), _p(v), _p(bias), _p(out), B, heads, Nq, Nk, d,
                              q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                              out.stride(0), out.stride(1), bias.stride(0) if bias is not None else 0, kv_group,
                              float(scale), float(out_scale), int(accumulate), _dt(q) + (256 if bias_packed else 0), _stream(), _p(bias_alt), _p(bias_sel),
                              _p(bias_blocks), _p(bias_blocks_alt), bias_blocks.shape[1] if bias_blocks is not None else 0)
    _check(rc, "im360_attn_fwd")
    _count("attn" if bias is None else "attn_warp", 4.0 * B * heads * Nq * Nk * d, q.element_size() * (2 * B * Nq * C + 2 * k.shape[0] * Nk * C)
           + (0 if bias is None else bias.element_size() * Nq * Nk))
    return out


def attention2(q, k, v, k2, v2, heads, scale=None, out_scale=1.0, out_scale2=1.0, kv_group=1):
    """out_scale * attn(q, k, v) + out_scale2 * attn(q, k2, v2) in ONE launch (two independent softmaxes over two
    key / value sets: the text and the IP-adapter tokens of IPCrossAttention, animatediff/models/attention.py:113-148).
    Shapes as in ``attention``; head dim 64."""
    _dev(q, k, v, k2, v2)
    B, Nq, C = q.shape
    d = C // heads
    for t in (k, v, k2, v2):
        assert t.shape[0] * kv_group == B and t.shape[2] == C and t.stride(2) == 1
    assert v.shape[1] == k.shape[1] and v2.shape[1] == k2.shape[1] and q.stride(2) == 1
    out = torch.empty((B, Nq, C), dtype=q.dtype, device=q.device)
    if scale is None:
        scale = d ** -0.5
    rc = lib().im360_attn_fwd2(_p(q), _p(k), _p(v), _p(k2), _p(v2), _p(out), B, heads, Nq, k.shape[1], k2.shape[1], d,
                               q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1),
                               k2.stride(0), k2.stride(1), v2.stride(0), v2.stride(1), out.stride(0), out.stride(1),
                               kv_group, float(scale), float(out_scale), float(out_scale2), _dt(q), _stream())
    _check(rc, "im360_attn_fwd2")
    _count("attn_x2", 4.0 * B * heads * Nq * (k.shape[1] + k2.shape[1]) * d,
           q.element_size() * (2 * B * Nq * C + 2 * k.shape[0] * (k.shape[1] + k2.shape[1]) * C))
    return out


def temporal_attention(qkv, B, F, P, heads, frame_major=False, out=None):
    """qkv [B*F*P, 3*C] = fused (q | k | v) projection of token-major activations [B, F, P, C].
    Attention over the F axis per (batch, pixel, head).  Returns [B*F*P, C].
    ``frame_major``: rows (and the result's) are ordered [F, B, P] instead -- the receive layout of the frame <-> pixel
    all-to-all (``shard_pack``), read in place through the kernel's strides.  ``out``: preallocated result."""
    _dev(qkv, out)
    C = qkv.shape[1] // 3
    assert qkv.shape[0] == B * F * P and qkv.stride(1) == 1
    rs = qkv.stride(0)
    if out is None:
        out = torch.empty((B * F * P, C), dtype=qkv.dtype, device=qkv.device)
    else:
        _written(out)
    assert out.shape == (B * F * P, C) and out.is_contiguous() and out.dtype == qkv.dtype
    d = C // heads
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    fs, bs = (B * P, P) if frame_major else (P, F * P)          # frame / batch strides in rows
    rc = lib().im360_temporal_attn_fwd(_p(q), _p(k), _p(v), _p(out), B, F, P, heads, d,
                                       fs * rs, rs, bs * rs, fs * C, C, bs * C,
                                       float(d ** -0.5), _dt(qkv), _stream())
    _check(rc, "im360_temporal_attn_fwd")
    _count("temporal", 4.0 * B * P * heads * F * F * d, qkv.element_size() * 4 * B * F * P * C)
    return out


def _host_table(t, ctype):
    """Host copy of a small plan table (``starts`` / ``weights``: a tensor on any device, or a sequence) as a ctypes array.  A tensor
    keeps its copy on the tensor OBJECT (with the version it was taken at): the one device-to-host read happens on the first call --
    the eager warm-up of a captured step -- and never inside a capture."""
    if not torch.is_tensor(t):
        vals = list(t)
        return (ctype * len(vals))(*vals), len(vals)
    hit = getattr(t, "_im360_host", None)
    if hit is None or hit[0] != t._version:
        vals = t.detach().reshape(-1).tolist()
        hit = (t._version, (ctype * len(vals))(*vals), len(vals))
        t._im360_host = hit
    return hit[1], hit[2]


def temporal_attention_windows(qkv, pe_qkv, B, F, P, heads, starts, weights, ring=False, out=None):
    """Window-fused temporal attention (``context.windowed_temporal_attention`` is the definition; FreeNoise, arXiv 2310.15169 3.2).
    qkv [B*F*P, 3*C]: the fused projection WITHOUT the frame PE, rows (batch, frame, pixel); pe_qkv [L, 3*C]: PE rows 0 .. L-1 through
    the same projection; ``starts`` [nW] (int32) / ``weights`` [L] (float32): the plan's tables (``context.context_windows`` /
    ``context.context_weights``; tensors or sequences -- the launch takes host copies, see ``_host_table``); ``ring``: window k
    holds the frames (starts[k] + p) % F.  One launch; returns [B*F*P, C].  ``out``: preallocated result, rows at any stride that is a
    multiple of 8 elements."""
    _dev(qkv, pe_qkv, out)
    C = qkv.shape[1] // 3
    assert qkv.shape[0] == B * F * P and qkv.stride(1) == 1
    assert pe_qkv.dim() == 2 and pe_qkv.shape[1] == 3 * C and pe_qkv.is_contiguous() and pe_qkv.dtype == qkv.dtype
    rs = qkv.stride(0)
    if out is None:
        out = torch.empty((B * F * P, C), dtype=qkv.dtype, device=qkv.device)
    else:
        _written(out)
    assert out.shape == (B * F * P, C) and out.stride(1) == 1 and out.dtype == qkv.dtype
    os_ = out.stride(0)
    d = C // heads
    st, nW = _host_table(starts, ctypes.c_int32)
    wt, L = _host_table(weights, ctypes.c_float)
    assert pe_qkv.shape[0] == L, (pe_qkv.shape, L)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    rc = lib().im360_temporal_attn_windows_fwd(_p(q), _p(k), _p(v), _p(pe_qkv), _p(out), B, F, P, heads, d,
                                               P * rs, rs, F * P * rs, P * os_, os_, F * P * os_,
                                               ctypes.cast(st, _PTR), nW, ctypes.cast(wt, _PTR), L, int(bool(ring)),
                                               float(d ** -0.5), _dt(qkv), _stream())
    _check(rc, "im360_temporal_attn_windows_fwd")
    _count("temporal", 4.0 * B * P * heads * nW * L * L * d, qkv.element_size() * (4 * B * F * P * C + 3 * L * C))
    return out


def shard_pack(src, dst, B, Fl, P, W, PP, unpack=False):
    """Frame-sharded tokens [B, Fl, P, C] <-> the all-to-all buffer [W, Fl, B, PP, C] (``im360_shard_pack``); both tensors are
    caller-owned (pre-sized, so the exchange can be graph-captured).  ``unpack``: buffer (src) -> tokens (dst)."""
    _dev(src, dst)
    C = src.shape[-1]
    assert src.is_contiguous() and dst.is_contiguous() and dst.shape[-1] == C and src.dtype == dst.dtype and src.element_size() == 2
    _written(dst)
    tok, buf = (dst, src) if unpack else (src, dst)
    assert tok.numel() == B * Fl * P * C and buf.numel() == W * Fl * B * PP * C, (tok.shape, buf.shape)
    rc = lib().im360_shard_pack(_p(src), _p(dst), B, Fl, P, C, W, PP, int(bool(unpack)), _stream())
    _check(rc, "im360_shard_pack")
    _count("misc", 0.0, 2 * tok.element_size() * tok.numel())
    return dst


# ------------------------------------------------------------------------------------------ group norm
# GroupNorm statistics from the producer's epilogue: conv2d(..., gn_stats=True) / linear(..., gn_hw=pixels)
# attach `(partial sums, slabs per image)` to the tensor they return when the launch can write them (im360_conv_gn_slabs);
# group_norm_stats() then skips its own pass over that tensor.  The tag belongs to the tensor OBJECT and dies with a view /
# reshape (carry_gn moves it onto a reshaped view of the same rows) or an in-place write (checked through _version).
GN_FROM_PRODUCER = True


def _gn_of(t):
    g = getattr(t, "_im360_gn", None)
    if g is None or g[2] != t._version:
        return None
    return g[0], g[1]


def _tag_gn(t, partial, slabs):
    t._im360_gn = (partial, slabs, t._version)
    return t


def _written(t):
    """The ctypes kernels write through raw pointers and do not bump ``t._version`` (the tag's invalidation rule): every wrapper
    that writes into a CALLER-SUPPLIED tensor (``out=`` / ``accumulate`` / a destination buffer) drops a producer tag it may carry."""
    if t is not None and getattr(t, "_im360_gn", None) is not None:
        del t._im360_gn
    return t


def carry_gn(view, src):
    """``view`` is a reshape of ``src`` with the same rows (tokens [n, hw, c] <-> images [n, h, w, c]): keep the producer's partial sums."""
    g = getattr(src, "_im360_gn", None)
    if g is not None and g[2] == src._version and view.numel() == src.numel():
        view._im360_gn = (g[0], g[1], view._version)
    return view


def group_norm_stats(x, gamma, beta, groups, eps, pad=0):
    """x [N, H, W, C] channels-last, or a pair (xa [N, H, W, C1], xb [N, H, W, C2]) standing for their channel
    concatenation (never materialised).  Returns fp32 (scale, shift) [N, C] with GN(x) = x*scale + shift;
    pad > 0 = statistics of the circularly W-padded tensor."""
    xa, xb = x if isinstance(x, (tuple, list)) else (x, None)
    _dev(xa, xb, gamma, beta)
    N, H, W, C1 = xa.shape
    C = C1 + (xb.shape[-1] if xb is not None else 0)
    assert xa.is_contiguous() and gamma.dtype == xa.dtype and beta.dtype == xa.dtype and gamma.numel() == C
    scale = torch.empty((N, C), dtype=torch.float32, device=xa.device)
    shift = torch.empty((N, C), dtype=torch.float32, device=xa.device)
    srcs = [xa] if xb is None else [xa, xb]
    if pad == 0 and GN_FROM_PRODUCER and any(_gn_of(t) is not None for t in srcs):
        # at least one source carries partial sums from the epilogue of the kernel that produced it (conv2d / linear with
        # gn_stats): only the others get a statistics pass, then one finalize over both sets of partial sums
        parts, read = [], 0
        for t in srcs:
            g = _gn_of(t)
            if g is None:
                St = lib().im360_gn_num_slabs(N, H, W)
                buf = torch.empty((N * St * 2 * t.shape[-1],), dtype=torch.float32, device=t.device)
                assert t.is_contiguous() and t.shape[:3] == xa.shape[:3] and t.dtype == xa.dtype
                _check(lib().im360_groupnorm_partial(_p(t), _p(buf), N, H, W, t.shape[-1], _dt(t), _stream()), "im360_groupnorm_partial")
                g = (buf, St)
                read += t.element_size() * t.numel()
            parts.append(g)
        (pa, Sa), (pb, Sb) = parts[0], (parts[1] if len(parts) > 1 else (None, 0))
        rc = lib().im360_groupnorm_finalize(_p(pa), Sa, C1, _p(pb), Sb, C - C1, _p(gamma), _p(beta), _p(scale), _p(shift), N, groups,
                                            H * W, float(eps), _dt(xa), _stream())
        _check(rc, "im360_groupnorm_finalize")
        _count("gn_stats", 0.0, read + 4 * sum(p_.numel() for p_, _ in parts))
        return scale, shift
    S = lib().im360_gn_num_slabs(N, H, W)
    partial = torch.empty((N * S * 2 * C,), dtype=torch.float32, device=xa.device)
    if xb is None:
        rc = lib().im360_groupnorm_stats(_p(xa), _p(gamma), _p(beta), _p(partial), _p(scale), _p(shift),
                                         N, H, W, C, groups, pad, float(eps), _dt(xa), _stream())
        _check(rc, "im360_groupnorm_stats")
    else:
        assert xb.is_contiguous() and xb.shape[:3] == xa.shape[:3] and xb.dtype == xa.dtype
        rc = lib().im360_groupnorm_stats_cat(_p(xa), _p(xb), _p(gamma), _p(beta), _p(partial), _p(scale), _p(shift),
                                             N, H, W, C1, C - C1, groups, pad, float(eps), _dt(xa), _stream())
        _check(rc, "im360_groupnorm_stats_cat")
    _count("gn_stats", 0.0, xa.element_size() * N * H * W * C)
    return scale, shift


def group_norm_apply(x, scale, shift, silu, pad=0):
    """y [N, H, W + 2 pad, C] = act(x * scale + shift), circular along W; x as in ``group_norm_stats`` (a pair writes the
    normalised concatenation directly)."""
    xa, xb = x if isinstance(x, (tuple, list)) else (x, None)
    _dev(xa, xb, scale, shift)
    N, H, W, C1 = xa.shape
    C = C1 + (xb.shape[-1] if xb is not None else 0)
    assert xa.is_contiguous() and scale.shape == (N, C)
    y = torch.empty((N, H, W + 2 * pad, C), dtype=xa.dtype, device=xa.device)
    if xb is None:
        rc = lib().im360_groupnorm_apply(_p(xa), _p(scale), _p(shift), _p(y), N, H, W, C, pad, int(bool(silu)),
                                         _dt(xa), _stream())
        _check(rc, "im360_groupnorm_apply")
    else:
        assert xb.is_contiguous() and xb.shape[:3] == xa.shape[:3] and xb.dtype == xa.dtype
        rc = lib().im360_groupnorm_apply_cat(_p(xa), _p(xb), _p(scale), _p(shift), _p(y), N, H, W, C1, C - C1, pad,
                                             int(bool(silu)), _dt(xa), _stream())
        _check(rc, "im360_groupnorm_apply_cat")
    _count("gn_apply", 0.0, xa.element_size() * (N * H * W * C + y.numel()))
    return y


# group_norm(): True = ONE launch (im360_groupnorm_fused: statistics, per-image arrival counter, in-kernel reduction,
# normalisation; same bits).  Measured SLOWER than the three-kernel path -- 0.299 vs 0.264 ms on 640 x 32x32x320, 0.315 vs
# 0.101 ms on 32 x 64x128x320 (64 slabs per image wait for each other) -- the arrival waits and the write-through publish
# of the partials cost more than the HBM pass the cache-resident second read saves; and it must not be captured in a
# hipGraph together with kernels it could wait behind.  Kept as an A/B variant, off.
GN_FUSED = False


def group_norm_partials(x, pad=0):
    """Per-image partial sums of x [N, H, W, C] as (buffer fp32 [N][S][2][C], S): the ones the tensor's producer wrote in its
    epilogue (pad == 0 only: the padded statistics weight the wrapped columns twice), else one statistics pass over x."""
    g = _gn_of(x) if (pad == 0 and GN_FROM_PRODUCER) else None
    if g is not None:
        return g
    N, H, W, C = x.shape
    assert x.is_contiguous()
    S = lib().im360_gn_num_slabs(N, H, W)
    buf = torch.empty((N * S * 2 * C,), dtype=torch.float32, device=x.device)
    if pad:
        _check(lib().im360_groupnorm_partial_pad(_p(x), _p(buf), N, H, W, C, pad, _dt(x), _stream()), "im360_groupnorm_partial_pad")
    else:
        _check(lib().im360_groupnorm_partial(_p(x), _p(buf), N, H, W, C, _dt(x), _stream()), "im360_groupnorm_partial")
    _count("gn_stats", 0.0, x.element_size() * x.numel() + 4 * buf.numel())
    return buf, S


# group_norm(): "partials" (default since round 6) = statistics pass only where the producer did not leave partial sums, then ONE
# launch that rebuilds scale / shift per workgroup and normalises (im360_groupnorm_apply_partials: no finalize launch, the
# concatenation in one launch instead of two); "three" = rounds 2 - 5's statistics + finalize + apply (same bits; the A/B partner);
# GN_FUSED below = the single-launch variant with arrival counters (measured slower).
GN_MODE = os.environ.get("IM360_GN_MODE", "partials")


def group_norm(x, gamma, beta, groups, eps, silu=False, pad=0):
    """act(GroupNorm(x)) [N, H, W + 2 pad, C]; x [N, H, W, C] or a pair standing for a channel concatenation (see GN_MODE)."""
    if not GN_FUSED and GN_MODE == "partials":
        xa, xb = x if isinstance(x, (tuple, list)) else (x, None)
        _dev(xa, xb, gamma, beta)
        N, H, W, C1 = xa.shape
        C2 = xb.shape[-1] if xb is not None else 0
        assert xa.is_contiguous() and gamma.dtype == xa.dtype and beta.dtype == xa.dtype and gamma.numel() == C1 + C2
        assert xb is None or (xb.is_contiguous() and xb.shape[:3] == xa.shape[:3] and xb.dtype == xa.dtype)
        pa, Sa = group_norm_partials(xa, pad)
        pb, Sb = group_norm_partials(xb, pad) if xb is not None else (None, 0)
        y = torch.empty((N, H, W + 2 * pad, C1 + C2), dtype=xa.dtype, device=xa.device)
        rc = lib().im360_groupnorm_apply_partials(_p(xa), _p(xb), _p(pa), Sa, _p(pb), Sb, _p(gamma), _p(beta), _p(y), N, H, W, C1, C2,
                                                  groups, pad, float(eps), int(bool(silu)), _dt(xa), _stream())
        _check(rc, "im360_groupnorm_apply_partials")
        _count("gn_apply", 0.0, xa.element_size() * (N * H * W * (C1 + C2) + y.numel()))
        return y
    if not GN_FUSED:
        scale, shift = group_norm_stats(x, gamma, beta, groups, eps, pad)
        return group_norm_apply(x, scale, shift, silu, pad)
    xa, xb = x if isinstance(x, (tuple, list)) else (x, None)
    _dev(xa, xb, gamma, beta)
    N, H, W, C1 = xa.shape
    C2 = xb.shape[-1] if xb is not None else 0
    C = C1 + C2
    assert xa.is_contiguous() and gamma.dtype == xa.dtype and beta.dtype == xa.dtype and gamma.numel() == C
    assert xb is None or (xb.is_contiguous() and xb.shape[:3] == xa.shape[:3] and xb.dtype == xa.dtype)
    S = lib().im360_gn_num_slabs(N, H, W)
    partial = torch.empty((N * S * 2 * C,), dtype=torch.float32, device=xa.device)
    counter = torch.empty((N,), dtype=torch.int32, device=xa.device)
    y = torch.empty((N, H, W + 2 * pad, C), dtype=xa.dtype, device=xa.device)
    rc = lib().im360_groupnorm_fused(_p(xa), _p(xb), _p(gamma), _p(beta), _p(partial), _p(counter), _p(y), N, H, W, C1, C2,
                                     groups, pad, float(eps), int(bool(silu)), _dt(xa), _stream())
    _check(rc, "im360_groupnorm_fused")
    _count("gn_apply", 0.0, xa.element_size() * (N * H * W * C + y.numel()))          # algorithmic: x read once, y written once
    return y


# ------------------------------------------------------------------------------------------ convolution
def pack_conv_weight(w, cin_pad=None):
    """[Cout, Cin, kh, kw] -> packed [CoutPad128, kh*kw, CinPad32] (zero padded)."""
    _dev(w)
    Cout, Cin, kh, kw = w.shape
    taps = kh * kw
    assert taps in (1, 4, 9)
    cin_pad = cin_pad or ((Cin + 31) // 32) * 32
    cout_pad = ((Cout + 127) // 128) * 128
    out = torch.empty((cout_pad, taps, cin_pad), dtype=w.dtype, device=w.device)
    rc = lib().im360_pack_conv_weight(_p(w.contiguous()), _p(out), Cout, Cin, taps, cout_pad, cin_pad, _dt(w), _stream())
    _check(rc, "im360_pack_conv_weight")
    return out


def up2_weights(w):
    """[Cout, Cin, 3, 3] -> [4, Cout, Cin, 2, 2] (fp32): the taps of conv3x3-after-nearest-x2 that land on the same source
    pixel, summed, per output parity (py, px) = (0,0) (0,1) (1,0) (1,1).  Row parity 0 reads source rows (y - 1, y) with
    (k0, k1 + k2); parity 1 reads (y, y + 1) with (k0 + k1, k2); columns alike."""
    w = w.detach().float()
    rows = (torch.stack([w[:, :, 0], w[:, :, 1] + w[:, :, 2]], dim=2), torch.stack([w[:, :, 0] + w[:, :, 1], w[:, :, 2]], dim=2))   # [Cout, Cin, 2, 3]
    out = []
    for py in (0, 1):
        r = rows[py]
        for px in (0, 1):
            out.append(torch.stack([r[..., 0], r[..., 1] + r[..., 2]], dim=-1) if px == 0 else torch.stack([r[..., 0] + r[..., 1], r[..., 2]], dim=-1))
    return torch.stack(out)


def pack_conv_up2_weight(w):
    """Conv weight [Cout, Cin, 3, 3] (Cin % 64 == 0) -> the four packed 4-tap weights of ``conv_up2`` [4, CoutPad, 4, Cin]."""
    _dev(w)
    w4 = up2_weights(w).to(w.dtype)
    return torch.stack([pack_conv_weight(w4[i].contiguous()) for i in range(4)]).contiguous()


def chunk_major(w_packed):
    """Packed token-major weight [rows, 1, K] (``pack_conv_weight`` / ``pack_geglu``) -> the same elements in CHUNK-MAJOR order
    [K / 32][rows][32] (returned with the original shape): the operand layout of the A/B kernel behind knob conv_ring 11, where a
    32-channel half stage of a weight tile is one contiguous block of whole 128-byte lines."""
    r, t, k = w_packed.shape
    assert t == 1 and k % 32 == 0
    return w_packed.reshape(r, k // 32, 32).permute(1, 0, 2).contiguous().reshape(r, 1, k)


def conv_up2(x, w4_packed, cout, bias=None, wrap=False):
    """nearest-x2 upsample + conv3x3 (pad 1, ``wrap``: circular along W) of x [N, Hin, Win, Cin] -> [N, 2 Hin, 2 Win, Cout],
    as four 2 x 2 convolutions of the low-resolution input (4 / 9 of the MACs)."""
    _dev(x, w4_packed, bias)
    N, Hin, Win, Cin = x.shape
    assert x.is_contiguous() and w4_packed.is_contiguous() and w4_packed.shape[0] == 4 and w4_packed.shape[2] == 4 and w4_packed.shape[3] == Cin
    y = torch.empty((N, 2 * Hin, 2 * Win, cout), dtype=x.dtype, device=x.device)
    rc = lib().im360_conv_up2_fwd(_p(x), _p(w4_packed), _p(bias), _p(y), N, Hin, Win, Cin, cout, int(wrap), _dt(x), _stream())
    _check(rc, "im360_conv_up2_fwd")
    _count("conv", 2.0 * N * 4 * Hin * Win * cout * Cin * 9, x.element_size() * (x.numel() + y.numel() + 9 * cout * Cin),
           executed=2.0 * N * 4 * Hin * Win * cout * Cin * 4, shape=f"up2:{Cin}:{cout}:{2 * Hin}x{2 * Win}{'w' if wrap else ''}")
    return y


def conv2d(x, w_packed, cout, bias=None, stride=1, up=False, wrap=False, x_off=0, wout=None,
           temb=None, imgs_per_temb=1, res=None, y_off=0, gn_stats=False):
    """x [N, Hin, Win, Cin] -> y [N, Hout, Wout, Cout] (3x3 pad 1 or 1x1, see im360_conv_fwd)."""
    _dev(x, w_packed, bias, temb, res)
    N, Hin, Win, Cin = x.shape
    taps = w_packed.shape[1]
    assert x.is_contiguous() and w_packed.shape[2] == Cin, (x.shape, w_packed.shape)
    hc, wc = (2 * Hin, 2 * Win) if up else (Hin, Win)
    hout = hc // stride
    if wout is None:
        wout = wc // stride
    y = torch.empty((N, hout, wout, cout), dtype=x.dtype, device=x.device)
    if res is not None:
        assert res.shape == y.shape and res.is_contiguous()
    if temb is not None:
        assert temb.is_contiguous() and temb.shape[1] == cout and temb.shape[0] * imgs_per_temb == N
    gn, slabs = None, 0
    if gn_stats and GN_FROM_PRODUCER and not up:
        slabs = lib().im360_conv_gn_slabs(N, hout, wout, Cin, cout, taps)
        if slabs > 0:
            gn = torch.empty((N * slabs * 2 * cout,), dtype=torch.float32, device=x.device)
    # K-split (knob conv_ksplit): launches whose tile count is not a whole number of rounds of the chip run every tile in `parts` workgroups
    parts = lib().im360_conv_ksplit_plan(N, hout, wout, Cin, cout, taps, int(up), int(wrap), int(gn is not None)) if taps == 9 else 1
    if parts > 1:
        tiles = -(-(N * hout * wout) // 256) * (cout // 320)
        ws = torch.empty((tiles * (parts - 1) * 160 * 512,), dtype=torch.float32, device=x.device)
        cnt = torch.zeros((tiles,), dtype=torch.int32, device=x.device)
        rc = lib().im360_conv_fwd_ksplit(_p(x), _p(w_packed), _p(bias), _p(temb), _p(res), _p(y),
                                         N, Hin, Win, Cin, hout, wout, cout, taps, stride, int(up), int(wrap), x_off, y_off,
                                         imgs_per_temb, _dt(x), _stream(), _p(gn), _p(ws), ws.numel() * 4, _p(cnt), tiles)
        _check(rc, "im360_conv_fwd_ksplit")
    else:
        rc = lib().im360_conv_fwd(_p(x), _p(w_packed), _p(bias), _p(temb), _p(res), _p(y),
                                  N, Hin, Win, Cin, hout, wout, cout, taps, stride, int(up), int(wrap), x_off, y_off,
                                  imgs_per_temb, _dt(x), _stream(), _p(gn))
        _check(rc, "im360_conv_fwd")
    if gn is not None:
        _tag_gn(y, gn, slabs)
    if STATS is not None or SHAPES is not None:
        es = x.element_size()
        linear = taps == 1 and Hin == 1 and Win == 1
        _count("gemm" if linear else "conv", 2.0 * N * hout * wout * Cin * cout * taps,
               es * (x.numel() + cout * taps * Cin + y.numel() * (2 if res is not None else 1)),
               shape=(f"lin:{Cin}:{cout}:{'res' if res is not None else 'nores'}" if linear else
                      f"conv{taps}:{Cin}:{cout}:{hout}x{wout}:s{stride}{'u' if up else ''}{'w' if wrap else ''}{'o' if x_off else ''}"))
    return y


def can_conv1x1_cat(c1, c2):
    return c1 % 64 == 0 and c2 % 64 == 0


def conv1x1_cat(xa, xb, w_packed, cout, bias=None, res=None):
    """1x1 convolution of the channel concatenation [xa | xb] (never materialised): xa [N, H, W, C1], xb [N, H, W, C2],
    w_packed [CoutPad, 1, C1 + C2] -> [N, H, W, Cout] (+ bias, + res).  C1, C2 multiples of 64."""
    _dev(xa, xb, w_packed, bias, res)
    N, H, W, C1 = xa.shape
    C2 = xb.shape[-1]
    assert xa.is_contiguous() and xb.is_contiguous() and xb.shape[:3] == xa.shape[:3] and xb.dtype == xa.dtype
    assert w_packed.shape[1] == 1 and w_packed.shape[2] == C1 + C2, (w_packed.shape, C1, C2)
    y = torch.empty((N, H, W, cout), dtype=xa.dtype, device=xa.device)
    assert res is None or (res.shape == y.shape and res.is_contiguous())
    rc = lib().im360_conv1x1_cat_fwd(_p(xa), _p(xb), _p(w_packed), _p(bias), _p(res), _p(y), N, H, W, C1, C2, cout,
                                     _dt(xa), _stream())
    _check(rc, "im360_conv1x1_cat_fwd")
    _count("conv", 2.0 * N * H * W * (C1 + C2) * cout,
           xa.element_size() * (xa.numel() + xb.numel() + cout * (C1 + C2) + y.numel() * (2 if res is not None else 1)),
           shape=f"conv1cat:{C1}+{C2}:{cout}:{H}x{W}")
    return y


# ------------------------------------------------------------------------------------------ token-major linears
ROW_SLICE = 160          # columns per (sum, sum of squares) pair of the row statistics (one wave's share of a 320-column tile)


def linear(x, w_packed, n, bias=None, res=None, row_stats=False, gn_hw=None):
    """x [..., K] @ W^T + bias (+ res) -> [..., n] on the persistent ring kernel (n % 320 == 0, K % 32 == 0; w_packed from
    ``pack_conv_weight`` of the [n, K, 1, 1] view).  ``row_stats``: also return fp32 [M, n / 160, 2] = per row and
    160-column slice (sum, sum of squares) of the stored output -- the LayerNorm statistics a consumer with the
    normalisation folded in (``linear_ln`` / ``linear_geglu_ln``) needs."""
    _dev(x, w_packed, bias, res)
    k = x.shape[-1]
    m = x.numel() // k
    assert x.is_contiguous() and w_packed.shape[2] == k and w_packed.shape[1] == 1 and n % 320 == 0
    y = torch.empty(x.shape[:-1] + (n,), dtype=x.dtype, device=x.device)
    assert res is None or (res.is_contiguous() and res.numel() == y.numel() and res.dtype == x.dtype)
    st = torch.empty((m, n // ROW_SLICE, 2), dtype=torch.float32, device=x.device) if row_stats else None
    # gn_hw: the rows are images of gn_hw pixels each; when those are whole 256-row tiles the epilogue also writes GroupNorm
    # partial sums (one slab per tile) for the consumer's GroupNorm
    gn = None
    if gn_hw and GN_FROM_PRODUCER and gn_hw % 256 == 0 and m % gn_hw == 0 and k % 64 == 0:
        gn = torch.empty(((m // 256) * 2 * n,), dtype=torch.float32, device=x.device)
    rc = lib().im360_linear_fwd(_p(x), _p(w_packed), _p(bias), _p(res), _p(y), _p(st), m, k, n, _dt(x), _stream(), _p(gn))
    _check(rc, "im360_linear_fwd")
    if gn is not None:
        _tag_gn(y, gn, gn_hw // 256)
    _count("gemm", 2.0 * m * k * n, x.element_size() * (x.numel() + n * k + y.numel() * (2 if res is not None else 1))
           + (0 if st is None else 4 * st.numel()), shape=f"lin{'+stats' if row_stats else ''}:{k}:{n}:{'res' if res is not None else 'nores'}")
    return (y, st) if row_stats else y


def linear_ln(x, w_packed, c1, c2, stats, eps, n, tab=None, tab_div=1, tab_has_c2=False):
    """Linear(LayerNorm(x)) with the normalisation folded into the GEMM: x [..., K] RAW rows, ``stats`` their statistics
    from the producer (``linear(..., row_stats=True)``), w_packed = pack(gamma (.) W), c1 = row sums of the rounded
    gamma (.) W, c2 = W beta + bias (fp32 [n]); ``tab`` fp32 [Q, n]: row r also gets tab[(r // tab_div) % Q].
    The kernel takes table rows that INCLUDE c2 (one column vector per tile, fetched by LDS-DMA): ``tab_has_c2`` says the
    caller folded it already (``layers.ln_linear`` caches the folded table), otherwise it is added here."""
    _dev(x, w_packed, c1, c2, stats, tab)
    if tab is not None and not tab_has_c2:
        tab = (tab + c2[None, :]).contiguous()
    k = x.shape[-1]
    m = x.numel() // k
    assert x.is_contiguous() and w_packed.shape[2] == k and n % 320 == 0
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.shape[0] == m and stats.shape[2] == 2
    for t in (c1, c2):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    assert tab is None or (tab.dtype == torch.float32 and tab.is_contiguous() and tab.shape[-1] == n)
    y = torch.empty(x.shape[:-1] + (n,), dtype=x.dtype, device=x.device)
    rc = lib().im360_linear_ln_fwd(_p(x), _p(w_packed), _p(c1), _p(c2), _p(stats), stats.shape[1], float(eps), _p(tab),
                                   tab_div, tab.shape[0] if tab is not None else 1, _p(y), m, k, n, _dt(x), _stream())
    _check(rc, "im360_linear_ln_fwd")
    _count("gemm", 2.0 * m * k * n, x.element_size() * (x.numel() + n * k + y.numel()) + 4 * stats.numel(), shape=f"lin_ln:{k}:{n}")
    return y


def linear_geglu_ln(x, w_packed, c1, c2, stats, eps, inner):
    """GEGLU(LayerNorm(x)) in one launch: operands as in ``linear_ln`` with the rows of gamma (.) W, c1, c2 in the
    interleaved order of ``pack_geglu``."""
    _dev(x, w_packed, c1, c2, stats)
    k = x.shape[-1]
    m = x.numel() // k
    assert x.is_contiguous() and w_packed.shape[2] == k and w_packed.shape[0] >= 2 * inner
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.shape[0] == m and stats.shape[2] == 2
    for t in (c1, c2):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 2 * inner
    y = torch.empty(x.shape[:-1] + (inner,), dtype=x.dtype, device=x.device)
    rc = lib().im360_linear_geglu_ln(_p(x), _p(w_packed), _p(c1), _p(c2), _p(stats), stats.shape[1], float(eps), _p(y),
                                     m, k, inner, _dt(x), _stream())
    _check(rc, "im360_linear_geglu_ln")
    _count("gemm", 2.0 * m * k * 2 * inner, x.element_size() * (x.numel() + 2 * inner * k + y.numel()) + 4 * stats.numel(),
           shape=f"geglu_ln:{k}:{inner}")
    return y


def fold_layer_norm(weight, bias, gamma, beta):
    """Operands of the LayerNorm-folded GEMMs from a Linear (weight [n, K], bias [n] or None) and the LayerNorm in front
    of it: (gamma (.) W rounded to the weight dtype, c1 = its row sums, c2 = W beta + bias), the vectors in fp32.  c1 is
    taken from the ROUNDED matrix so that the mean term cancels exactly what the MFMA accumulates."""
    wg = (weight.detach().float() * gamma.detach().float()[None, :]).to(weight.dtype)
    c1 = wg.float().sum(dim=1)
    c2 = weight.detach().float() @ beta.detach().float()
    if bias is not None:
        c2 = c2 + bias.detach().float()
    return wg, c1.contiguous(), c2.contiguous()


# ------------------------------------------------------------------------------------------ token-wise
def layer_norm(x, gamma, beta, eps=1e-5, pre=None, post=None, post_div=1):
    """LayerNorm over the last dim of x [..., C] (rows flattened).  ``pre`` [P, C]: added to row r as
    pre[r % P] before normalising; ``post`` [Q, C]: post[(r // post_div) % Q] added to the result."""
    _dev(x, gamma, beta, pre, post)
    C = x.shape[-1]
    assert x.is_contiguous() and gamma.dtype == x.dtype
    rows = x.numel() // C
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    for t in (pre, post):
        assert t is None or (t.is_contiguous() and t.shape[-1] == C and t.dtype == x.dtype)
    rc = lib().im360_layernorm(_p(x), _p(gamma), _p(beta), _p(pre), _p(post), _p(y), rows, C,
                               pre.shape[0] if pre is not None else 1, post_div,
                               post.shape[0] if post is not None else 1, float(eps), _dt(x), _stream())
    _check(rc, "im360_layernorm")
    _count("misc", 0.0, 2 * x.element_size() * x.numel())
    return y


def geglu(h):
    """h [..., 2*I] -> h[..., :I] * gelu(h[..., I:])."""
    _dev(h)
    assert h.is_contiguous()
    I = h.shape[-1] // 2
    out = torch.empty(h.shape[:-1] + (I,), dtype=h.dtype, device=h.device)
    rc = lib().im360_geglu(_p(h), _p(out), h.numel() // (2 * I), I, _dt(h), _stream())
    _check(rc, "im360_geglu")
    _count("misc", 0.0, h.element_size() * (h.numel() + out.numel()))
    return out


def interleave_geglu(weight, bias):
    """Row order of the fused GEGLU GEMM: 32-row blocks of the value half and the gate half alternate, so packed rows
    [64 q, 64 q + 32) are value rows [32 q, 32 q + 32) and packed rows [64 q + 32, 64 q + 64) the matching gate rows."""
    two_i = weight.shape[0]
    i = two_i // 2
    assert i % 32 == 0
    w = torch.stack([weight[:i].reshape(i // 32, 32, -1), weight[i:].reshape(i // 32, 32, -1)], dim=1).reshape(two_i, -1)
    b = None
    if bias is not None:
        b = torch.stack([bias[:i].reshape(i // 32, 32), bias[i:].reshape(i // 32, 32)], dim=1).reshape(two_i).contiguous()
    return w, b


def pack_geglu(weight, bias):
    """GEGLU projection ``weight`` [2I, K] / ``bias`` [2I] (value half, then gate half) -> operands of
    ``linear_geglu``: 32-row blocks of the two halves interleaved (v0, g0, v1, g1, ...), the weight in the conv
    kernel's packed [rows][1][K] layout."""
    two_i, k = weight.shape
    assert (two_i // 2) % 128 == 0 and k % 64 == 0, (two_i, k)
    w, b = interleave_geglu(weight, bias)
    return pack_conv_weight(w.reshape(two_i, k, 1, 1).contiguous()), b


def linear_geglu(x, w_packed, bias_packed, inner):
    """x [..., K] -> (x W_v^T + b_v) * gelu(x W_g^T + b_g) [..., inner] in one launch (operands from ``pack_geglu``)."""
    _dev(x, w_packed, bias_packed)
    assert x.is_contiguous() and w_packed.shape[2] == x.shape[-1] and w_packed.shape[0] >= 2 * inner
    k = x.shape[-1]
    m = x.numel() // k
    y = torch.empty(x.shape[:-1] + (inner,), dtype=x.dtype, device=x.device)
    rc = lib().im360_linear_geglu(_p(x), _p(w_packed), _p(bias_packed), _p(y), m, k, inner, _dt(x), _stream())
    _check(rc, "im360_linear_geglu")
    _count("gemm", 2.0 * m * k * 2 * inner, x.element_size() * (x.numel() + 2 * inner * k + y.numel()), shape=f"geglu:{k}:{inner}")
    return y


FF_FUSED_SHAPE = (320, 1280)          # (K = N, inner) of the feed-forward that ``ff_fused`` / ``ff_fused_ln`` cover


def _ff_fused(x, w1_packed, b1_packed, c1, c2, stats, eps, w2_packed, b2, res, tag):
    _dev(x, w1_packed, b1_packed, c1, c2, stats, w2_packed, b2, res)
    k, inner = FF_FUSED_SHAPE
    m = x.numel() // k
    assert x.shape[-1] == k and x.is_contiguous() and w1_packed.shape[2] == k and w1_packed.shape[0] >= 2 * inner
    assert w2_packed.shape[2] == inner and w2_packed.shape[1] == 1 and w2_packed.shape[0] >= k and w2_packed.dtype == x.dtype
    assert res.is_contiguous() and res.numel() == x.numel() and res.dtype == x.dtype
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    rc = lib().im360_ff_fused(_p(x), _p(w1_packed), _p(b1_packed), _p(c1), _p(c2), _p(stats), 0 if stats is None else stats.shape[1],
                              float(eps), _p(w2_packed), _p(b2), _p(res), _p(y), m, k, inner, k, _dt(x), _stream())
    _check(rc, "im360_ff_fused")
    es = x.element_size()
    _count("gemm", 2.0 * m * k * 2 * inner + 2.0 * m * inner * k,
           es * (x.numel() + 2 * inner * k + k * inner + y.numel() + res.numel()) + (0 if stats is None else 4 * stats.numel()),
           shape=f"{tag}:{k}:{inner}")
    return y


def ff_fused(x, w1_packed, b1_packed, w2_packed, b2, res):
    """GEGLU feed-forward of a 320-channel block + residual in ONE launch: ``linear_geglu(x, w1_packed, b1_packed, 1280)`` followed by
    the [1280 -> 320] Linear with bias ``b2`` and residual ``res`` (w2_packed = ``pack_conv_weight`` of the [320, 1280, 1, 1] view);
    the 1280-wide intermediate stays in LDS.  Same bits as the pair of launches."""
    return _ff_fused(x, w1_packed, b1_packed, None, None, None, 0.0, w2_packed, b2, res, "ff")


def ff_fused_ln(x, w1_packed, c1, c2, stats, eps, w2_packed, b2, res):
    """``ff_fused`` with the LayerNorm in front folded into the first GEMM: operands as in ``linear_geglu_ln``."""
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.shape[0] == x.numel() // x.shape[-1] and stats.shape[2] == 2
    for t in (c1, c2):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 2 * FF_FUSED_SHAPE[1]
    return _ff_fused(x, w1_packed, None, c1, c2, stats, eps, w2_packed, b2, res, "ff_ln")


def softmax_rows(x, scale=1.0, out=None):
    """softmax(x * scale) over the last dim of a 2-D tensor (fp32 inside); ``out`` may be ``x`` (in place)."""
    _dev(x, out)
    assert x.dim() == 2 and x.stride(1) == 1
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    else:
        _written(out)
    rc = lib().im360_softmax_rows(_p(x), _p(out), x.shape[0], x.shape[1], x.stride(0), out.stride(0), float(scale),
                                  _dt(x), _stream())
    _check(rc, "im360_softmax_rows")
    _count("misc", 0.0, 2 * x.element_size() * x.numel())
    return out


def can_single_head_attention(d, nk):
    """Shapes ``single_head_attention`` takes (GEMM K / softmax row granularity); callers keep a torch path for the rest."""
    return d % 32 == 0 and nk % 32 == 0


def single_head_attention(q, k, v, scale):
    """softmax(q k^T * scale) v for ONE head of any width (the VAE's d = 512 AttentionBlock): scores through the MFMA
    GEMM kernel (k as the weight operand), fp32 row softmax of the 16-bit scores, probabilities x v through the GEMM
    kernel again -- the reference's own op order (baddbmm -> softmax(float) -> bmm, diffusers/models/attention.py:
    336-364).  q [Nq, d], k / v [Nk, d]; d % 32 == 0, Nk % 32 == 0."""
    nq, d = q.shape
    nk = k.shape[0]
    if not can_single_head_attention(d, nk):
        raise NotImplementedError(f"single_head_attention: d={d} and Nk={nk} must be multiples of 32")
    kw = k.contiguous().reshape(nk, 1, d) if nk % 128 == 0 else pack_conv_weight(k.reshape(nk, d, 1, 1))
    # the scale goes into q BEFORE the GEMM, so the 16-bit scores that are stored are the scaled ones -- like the reference's
    # baddbmm(alpha=scale); unscaled d = 512 dot products would cost fp16 a factor sqrt(512) of headroom before inf
    s = conv2d((q * scale).contiguous().reshape(nq, 1, 1, d), kw, nk).reshape(nq, nk)
    softmax_rows(s, 1.0, out=s)
    vt = v.t().contiguous()
    vw = vt.reshape(d, 1, nk) if d % 128 == 0 else pack_conv_weight(vt.reshape(d, nk, 1, 1))
    return conv2d(s.reshape(nq, 1, 1, nk), vw, d).reshape(nq, d)


# ------------------------------------------------------------------------------------------ misc
def circular_pad_w(x, pad):
    """x [..., W, C] channels-last -> [..., W + 2 pad, C]."""
    _dev(x)
    assert x.is_contiguous()
    W, C = x.shape[-2], x.shape[-1]
    rows = x.numel() // (W * C)
    y = torch.empty(x.shape[:-2] + (W + 2 * pad, C), dtype=x.dtype, device=x.device)
    rc = lib().im360_circular_pad_w(_p(x), _p(y), rows, W, C, pad, _dt(x), _stream())
    _check(rc, "im360_circular_pad_w")
    return y


def circular_pad_hw(x, left, right, top=0, bottom=0):
    """``F.pad(x, (left, right, top, bottom), mode="circular")`` on the last two axes of a contiguous W-last tensor of
    any dtype (one HBM pass)."""
    _dev(x)
    assert x.is_contiguous() and x.dim() >= 2
    H, W = x.shape[-2], x.shape[-1]
    n = x.numel() // (H * W)
    y = torch.empty(x.shape[:-2] + (H + top + bottom, W + left + right), dtype=x.dtype, device=x.device)
    rc = lib().im360_circular_pad_hw(_p(x), _p(y), n, H, W, left, right, top, bottom, x.element_size(), _stream())
    _check(rc, "im360_circular_pad_hw")
    return y


def remap_cubic_wrap(img, map_x, map_y, wtab):
    """``cv2.remap(img[n], map_x[m], map_y[m], INTER_CUBIC, BORDER_WRAP)`` for every (n, m): img uint8 [N, H, W, C] on the
    device, maps float32 [M, h, w], wtab int16 [1024, 16] -> uint8 [N, M, h, w, C]."""
    _dev(img, map_x, map_y, wtab)
    assert img.dtype == torch.uint8 and img.dim() == 4 and img.is_contiguous()
    assert map_x.dtype == torch.float32 and map_x.shape == map_y.shape and map_x.dim() == 3 and map_x.is_contiguous() and map_y.is_contiguous()
    assert wtab.dtype == torch.int16 and wtab.shape == (1024, 16) and wtab.is_contiguous()
    N, H, W, C = img.shape
    M, h, w = map_x.shape
    out = torch.empty((N, M, h, w, C), dtype=torch.uint8, device=img.device)
    rc = lib().im360_remap_cubic_wrap_u8(_p(img), _p(map_x), _p(map_y), _p(wtab), _p(out), N, M, H, W, C, h, w, _stream())
    _check(rc, "im360_remap_cubic_wrap_u8")
    return out


def max_rect(mask):
    """Largest all-ones rectangle of a host mask [H, W] -> (top, left, width, height) (reference scan order / ties)."""
    import numpy as np
    m = np.ascontiguousarray(np.asarray(mask) == 1, dtype=np.uint8)
    rect = (ctypes.c_int64 * 4)()
    rc = lib().im360_max_rect(m.ctypes.data, m.shape[0], m.shape[1], ctypes.addressof(rect))
    _check(rc, "im360_max_rect")
    return tuple(int(v) for v in rect)


def cfg_ddim_update(uncond, cond, sample, guidance, cx, cv, coef_dev=None):
    """x_prev = cx * sample + cv * (uncond + guidance * (cond - uncond)); ``coef_dev`` = device float32[3]
    (guidance, cx, cv) read by the kernel instead of the scalars (graph replay)."""
    _dev(uncond, cond, sample)
    assert uncond.is_contiguous() and cond.is_contiguous() and sample.is_contiguous()
    assert uncond.shape == cond.shape == sample.shape and uncond.dtype == sample.dtype
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    rc = lib().im360_cfg_ddim_update(_p(uncond), _p(cond), _p(sample), _p(out), sample.numel(),
                                     float(guidance), float(cx), float(cv), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, "im360_cfg_ddim_update")
    return out


DDIM_PRED_MODE = {"epsilon": 0, "v_prediction": 1, "sample": 2}
DDIM_CLIP_SAMPLE, DDIM_CLIPPED_OUTPUT = 4, 8


RESCALE_RECORD = 8         # floats per partial-moment record of the guidance-rescale statistics pass (csrc/sampler_step.hip)


def _rescale_workspace(like):
    """fp32 workspace for the partial-moment records of a guidance-rescale statistics pass over ``like``: a torch allocation (inside
    a graph capture it comes from the graph's pool, like the noise tensors)."""
    return torch.empty(lib().im360_cfg_rescale_records(like.numel()) * RESCALE_RECORD, dtype=torch.float32, device=like.device)


def _rescale_stats(uncond, cond, guidance, coef_dev):
    ws = _rescale_workspace(cond)
    rc = lib().im360_cfg_rescale_stats(_p(uncond), _p(cond), cond.numel(), float(guidance), _p(ws), ws.numel(), _dt(cond), _stream(),
                                       _p(coef_dev))
    _check(rc, "im360_cfg_rescale_stats")
    return ws


def _rescale_factor(ws, like, rescale):
    """The factor from the records ``ws`` of a statistics pass over ``like``: a device float32 scalar."""
    out = torch.empty((), dtype=torch.float32, device=like.device)
    _check(lib().im360_cfg_rescale_factor(_p(ws), ws.numel(), like.numel(), float(rescale), _p(out), _stream()), "im360_cfg_rescale_factor")
    return out


def cfg_rescale_factor(uncond, cond, guidance, rescale, coef_dev=None):
    """The guidance-rescale factor r = rescale * std(cond) / std(m) + (1 - rescale), m = uncond + guidance * (cond - uncond) in fp32,
    std = torch.std (correction 1) over the whole tensor: a device float32 scalar, no synchronisation.  Two launches: the statistics
    pass ``cfg_ddim_step(..., rescale=)`` runs, then the merge of its per-workgroup records that every workgroup of the step kernel
    makes -- the bits the step multiplies by.  ``coef_dev``: device float32 whose element 0 is read as the guidance instead."""
    _dev(uncond, cond, coef_dev)
    assert uncond.is_contiguous() and cond.is_contiguous() and uncond.shape == cond.shape and uncond.dtype == cond.dtype
    return _rescale_factor(_rescale_stats(uncond, cond, guidance, coef_dev), cond, rescale)


def _apg_args(who, apg, rescale=0.0):
    """``apg = (eta, threshold)`` of the step wrappers as the two floats of the ``_apg`` entry points: ``threshold`` None (no clamp)
    becomes +inf.  Refused: a non-finite ``eta``, a ``threshold`` that is not > 0, and ``rescale`` != 0 beside it (the two address the
    same defect; the product of the kernel variants is not built)."""
    if rescale != 0.0:
        raise ValueError(f"{who}: apg and rescale={rescale} cannot be combined")
    eta, threshold = apg
    eta, threshold = float(eta), math.inf if threshold is None else float(threshold)
    if not math.isfinite(eta):
        raise ValueError(f"{who}: apg eta={eta} must be finite")
    if not threshold > 0.0:
        raise ValueError(f"{who}: apg threshold={threshold} must be > 0 (None: no clamp)")
    return eta, threshold


def _apg_stats(uncond, cond, sample, mode, coefs, coef_dev):
    ws = _rescale_workspace(sample)
    rc = lib().im360_cfg_apg_stats(_p(uncond), _p(cond), _p(sample), sample.numel(), float(coefs[1]), float(coefs[2]), int(mode), _p(ws),
                                   ws.numel(), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, "im360_cfg_apg_stats")
    return ws


def _apg_stats_windows(preds, sample, starts, weights, geometry, mode, coefs, coef_dev, ring):
    ws = _rescale_workspace(sample)
    name = "im360_cfg_apg_stats_windows_ring" if ring else "im360_cfg_apg_stats_windows"
    rc = getattr(lib(), name)(_p(preds), _p(sample), _p(starts), _p(weights), *geometry, float(coefs[1]), float(coefs[2]), int(mode), _p(ws),
                              ws.numel(), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, name)
    return ws


def _apg_momentum_args(who, apg, apg_momentum, carry_dev, sample):
    """``apg_momentum = (state, carry)`` / ``carry_dev`` of the guided step wrappers after their checks: ``state`` float32, contiguous,
    on ``sample``'s device and of its element count (the momentum state, ``scheduler.new_apg_state``), ``carry`` a finite float,
    ``carry_dev`` None or a device float32[1] read instead.  Refused without ``apg``: the momentum is that of the projected guidance."""
    if apg is None:
        raise ValueError(f"{who}: apg_momentum needs apg (the momentum is that of the projected guidance)")
    state, carry = apg_momentum
    carry = float(carry)
    if not math.isfinite(carry):
        raise ValueError(f"{who}: apg carry={carry} must be finite")
    _dev(state, carry_dev)
    assert state.dtype == torch.float32 and state.is_contiguous() and state.device == sample.device and state.numel() == sample.numel()
    if carry_dev is not None:
        assert carry_dev.dtype == torch.float32 and carry_dev.numel() == 1 and carry_dev.is_cuda
    return state, carry


def _apg_momentum_stats(uncond, cond, sample, state, carry, carry_dev, mode, coefs, coef_dev):
    ws = _rescale_workspace(sample)
    rc = lib().im360_cfg_apg_momentum_stats(_p(uncond), _p(cond), _p(sample), _p(state), sample.numel(), float(coefs[1]), float(coefs[2]),
                                            int(mode), carry, _p(carry_dev), _p(ws), ws.numel(), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, "im360_cfg_apg_momentum_stats")
    return ws


def _apg_momentum_stats_windows(preds, sample, state, carry, carry_dev, starts, weights, geometry, mode, coefs, coef_dev, ring):
    ws = _rescale_workspace(sample)
    name = "im360_cfg_apg_momentum_stats_windows_ring" if ring else "im360_cfg_apg_momentum_stats_windows"
    rc = getattr(lib(), name)(_p(preds), _p(sample), _p(state), _p(starts), _p(weights), *geometry, float(coefs[1]), float(coefs[2]),
                              int(mode), carry, _p(carry_dev), _p(ws), ws.numel(), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, name)
    return ws


def _apg_scalars(ws, like, mode, coefs, apg, coef_dev):
    """(alpha, s, lambda) from the records ``ws`` of a statistics pass over ``like``: a device float32[3]."""
    eta, threshold = _apg_args("cfg_apg_scalars", apg)
    out = torch.empty(3, dtype=torch.float32, device=like.device)
    rc = lib().im360_cfg_apg_scalars(_p(ws), ws.numel(), like.numel(), *(float(v) for v in coefs[:3]), int(mode), eta, threshold, _p(out),
                                     _stream(), _p(coef_dev))
    _check(rc, "im360_cfg_apg_scalars")
    return out


def cfg_apg_scalars(uncond, cond, sample, mode, coefs, apg, coef_dev=None, apg_momentum=None, carry_dev=None):
    """The three scalars of adaptive projected guidance (arXiv 2410.02416; ``cfg_ddim_step(..., apg=)``) as a device float32[3], no
    synchronisation: ``alpha = <d, q> / <q, q>``, the clamp factor ``s`` and ``lambda = (g - 1) s (1 - eta) alpha`` with d = cond -
    uncond and q = cond + rho * sample, the sums over the whole tensor in fp32.  Two launches: the statistics pass the step wrappers
    run, then the merge of its records that every workgroup of the step kernel makes -- the bits the step uses.  ``mode`` / ``coefs``:
    those of the step (only the prediction type and the first three coefficients are read); ``apg = (eta, threshold)``;
    ``coef_dev``: device float32[6] whose first three elements are read instead.  ``apg_momentum = (state, carry)`` / ``carry_dev``: the
    scalars of the step with momentum (``cfg_ddim_step``), d replaced by e = d + carry * state; the state is read, never written."""
    _dev(uncond, cond, sample, coef_dev)
    assert uncond.is_contiguous() and cond.is_contiguous() and sample.is_contiguous()
    assert uncond.shape == cond.shape == sample.shape and uncond.dtype == cond.dtype == sample.dtype
    if apg_momentum is not None:
        state, carry = _apg_momentum_args("cfg_apg_scalars", apg, apg_momentum, carry_dev, sample)
        return _apg_scalars(_apg_momentum_stats(uncond, cond, sample, state, carry, carry_dev, mode, coefs, coef_dev), sample, mode, coefs,
                            apg, coef_dev)
    return _apg_scalars(_apg_stats(uncond, cond, sample, mode, coefs, coef_dev), sample, mode, coefs, apg, coef_dev)


def _check_step_noise(who, sample, noise, coefs, coef_dev):
    """``noise`` like ``sample`` or None (refused with sigma > 0), ``coef_dev`` a device float32[6] or None: the step wrappers' rule."""
    if noise is not None:
        assert noise.is_contiguous() and noise.shape == sample.shape and noise.dtype == sample.dtype
    elif coef_dev is None and coefs[5] != 0.0:
        raise ValueError(f"{who}: sigma > 0 needs a noise tensor")
    if coef_dev is not None:
        assert coef_dev.dtype == torch.float32 and coef_dev.numel() == 6 and coef_dev.is_cuda


def cfg_ddim_step(uncond, cond, sample, noise, mode, coefs, coef_dev=None, rescale=0.0, apg=None, apg_momentum=None, carry_dev=None):
    """DDIMScheduler.step(uncond + g (cond - uncond), t, sample) for any prediction type / clip / eta in one pass.
    ``mode``: DDIM_PRED_MODE | DDIM_CLIP_SAMPLE | DDIM_CLIPPED_OUTPUT; ``coefs`` = (guidance, sqrt_a, sqrt_b, sqrt_a_prev,
    dir, sigma) (DDIMScheduler.step_coefficients); ``noise``: variance noise like ``sample`` or None (zero noise, refused
    with sigma > 0); ``coef_dev`` = device float32[6] holding ``coefs``, read by the kernel instead (graph replay).
    ``rescale`` != 0: guidance rescale (arXiv 2305.08891, 3.4) -- the step sees r (uncond + g (cond - uncond)) with
    r = rescale * std(cond) / std(uncond + g (cond - uncond)) + (1 - rescale) over the whole tensor; a statistics launch in front of
    the step launch, no host read.  0 is the single launch without it.
    ``apg = (eta, threshold)``: adaptive projected guidance (arXiv 2410.02416, algorithm 1) -- the step sees
    ``cond + (g - 1) s d - lambda q`` (``cfg_apg_scalars``) in place of the combination: the guidance difference split along the text
    branch's denoised prediction, its parallel part scaled by ``eta``, its RMS in x0 units clamped to ``threshold`` (None: no clamp);
    a statistics launch over (uncond, cond, sample) in front of the step launch.  None is the call without it; refused together with
    ``rescale`` != 0.
    ``apg_momentum = (state, carry)`` (with ``apg`` only; None: the calls without it): the paper's momentum -- d is replaced by
    ``e = d + carry * state`` in the sums and in the combination, and ``state`` (float32, contiguous, ``sample``'s element count;
    ``scheduler.new_apg_state``) receives the unclamped e in place.  ``carry`` = ``scheduler.apg_carry(t_prev, t, beta)``; 0 (the
    first guided step of a run): the state is not read, only written, and the result is that of ``apg`` alone bit for bit.
    ``carry_dev``: device float32[1] read instead of ``carry`` (graph replay)."""
    _dev(uncond, cond, sample, noise)
    assert uncond.is_contiguous() and cond.is_contiguous() and sample.is_contiguous()
    assert uncond.shape == cond.shape == sample.shape and uncond.dtype == cond.dtype == sample.dtype
    _check_step_noise("cfg_ddim_step", sample, noise, coefs, coef_dev)
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    if apg_momentum is not None:
        state, carry = _apg_momentum_args("cfg_ddim_step", apg, apg_momentum, carry_dev, sample)
        eta, threshold = _apg_args("cfg_ddim_step", apg, rescale)
        ws = _apg_momentum_stats(uncond, cond, sample, state, carry, carry_dev, mode, coefs, coef_dev)
        rc = lib().im360_cfg_ddim_step_apg_momentum(_p(uncond), _p(cond), _p(sample), _p(noise), _p(state), _p(out), sample.numel(),
                                                    *(float(v) for v in coefs), int(mode), eta, threshold, _p(ws), ws.numel(), carry,
                                                    _p(carry_dev), _dt(sample), _stream(), _p(coef_dev))
        _check(rc, "im360_cfg_ddim_step_apg_momentum")
        return out
    if apg is not None:
        eta, threshold = _apg_args("cfg_ddim_step", apg, rescale)
        ws = _apg_stats(uncond, cond, sample, mode, coefs, coef_dev)
        rc = lib().im360_cfg_ddim_step_apg(_p(uncond), _p(cond), _p(sample), _p(noise), _p(out), sample.numel(), *(float(v) for v in coefs),
                                           int(mode), eta, threshold, _p(ws), ws.numel(), _dt(sample), _stream(), _p(coef_dev))
        _check(rc, "im360_cfg_ddim_step_apg")
        return out
    if rescale != 0.0:
        ws = _rescale_stats(uncond, cond, coefs[0], coef_dev)
        rc = lib().im360_cfg_ddim_step_rescale(_p(uncond), _p(cond), _p(sample), _p(noise), _p(out), sample.numel(),
                                               *(float(v) for v in coefs), int(mode), float(rescale), _p(ws), ws.numel(), _dt(sample),
                                               _stream(), _p(coef_dev))
        _check(rc, "im360_cfg_ddim_step_rescale")
        return out
    rc = lib().im360_cfg_ddim_step(_p(uncond), _p(cond), _p(sample), _p(noise), _p(out), sample.numel(),
                                   *(float(v) for v in coefs), int(mode), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, "im360_cfg_ddim_step")
    return out


def _windows_geometry(preds, sample, starts, weights, halves=2):
    """(nW, outer, F, L, inner) of a windowed step after the layout checks of ``cfg_ddim_step_windows``; ``halves=1``: ``preds`` holds
    the text halves alone (the unguided steps)."""
    assert preds.is_contiguous() and sample.is_contiguous() and preds.dtype == sample.dtype
    assert sample.dim() in (5, 6) and sample.shape[0] == 1, "sample must be [1, 4, F, H, W] or [1, m, 4, F, h, w]"
    fd = sample.dim() - 3
    outer, F, inner = math.prod(sample.shape[:fd]), sample.shape[fd], math.prod(sample.shape[fd + 1:])
    nW, L = preds.shape[0], preds.shape[fd + 1]
    assert tuple(preds.shape) == (nW, halves, *sample.shape[1:fd], L, *sample.shape[fd + 1:]), (tuple(preds.shape), tuple(sample.shape))
    assert starts.dtype == torch.int32 and starts.is_contiguous() and starts.numel() == nW
    assert weights.dtype == torch.float32 and weights.is_contiguous() and weights.numel() == L and 1 <= L <= F
    return nW, outer, F, L, inner


def _rescale_stats_windows(preds, sample, starts, weights, geometry, guidance, coef_dev, ring):
    ws = _rescale_workspace(sample)
    name = "im360_cfg_rescale_stats_windows_ring" if ring else "im360_cfg_rescale_stats_windows"
    rc = getattr(lib(), name)(_p(preds), _p(starts), _p(weights), *geometry, float(guidance), _p(ws), ws.numel(), _dt(sample), _stream(),
                              _p(coef_dev))
    _check(rc, name)
    return ws


def cfg_rescale_factor_windows(preds, sample, starts, weights, guidance, rescale, coef_dev=None, ring=False):
    """``cfg_rescale_factor`` over the per-frame blends of sliding-window predictions (arguments of ``cfg_ddim_step_windows``; only
    the shape of ``sample`` is used): the statistics pass ``cfg_ddim_step_windows(..., rescale=)`` runs, then the merge every
    workgroup of its step kernel makes.  A device float32 scalar, no synchronisation.  ``ring``: the windows lie on a ring."""
    _dev(preds, sample, starts, weights, coef_dev)
    geometry = _windows_geometry(preds, sample, starts, weights)
    return _rescale_factor(_rescale_stats_windows(preds, sample, starts, weights, geometry, guidance, coef_dev, ring), sample, rescale)


def cfg_apg_scalars_windows(preds, sample, starts, weights, mode, coefs, apg, coef_dev=None, ring=False, apg_momentum=None, carry_dev=None):
    """``cfg_apg_scalars`` over the per-frame blends of sliding-window predictions (arguments of ``cfg_ddim_step_windows``): the
    statistics pass ``cfg_ddim_step_windows(..., apg=)`` runs over the blends of both halves and ``sample``, then the merge every
    workgroup of its step kernel makes.  A device float32[3], no synchronisation.  ``ring``: the windows lie on a ring.
    ``apg_momentum`` / ``carry_dev``: as in ``cfg_apg_scalars``, the state in ``sample``'s layout."""
    _dev(preds, sample, starts, weights, coef_dev)
    geometry = _windows_geometry(preds, sample, starts, weights)
    if apg_momentum is not None:
        state, carry = _apg_momentum_args("cfg_apg_scalars_windows", apg, apg_momentum, carry_dev, sample)
        return _apg_scalars(_apg_momentum_stats_windows(preds, sample, state, carry, carry_dev, starts, weights, geometry, mode, coefs,
                                                        coef_dev, ring), sample, mode, coefs, apg, coef_dev)
    return _apg_scalars(_apg_stats_windows(preds, sample, starts, weights, geometry, mode, coefs, coef_dev, ring), sample, mode, coefs, apg,
                        coef_dev)


def cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=None, rescale=0.0, ring=False, apg=None,
                          apg_momentum=None, carry_dev=None):
    """``cfg_ddim_step`` on the per-frame weighted blend of sliding-window predictions, one pass.  ``sample`` (and ``noise`` /
    the result): a panorama latent [1, 4, F, H, W] or a perspective latent [1, m, 4, F, h, w];  ``preds`` [nW, 2, *sample.shape
    with F -> L]: window k's CFG-batched prediction in slot k;  ``starts`` device int32 [nW] ascending window start frames
    (context.context_windows);  ``weights`` device float32 [L] (context.context_weights).  ``mode`` / ``coefs`` / ``coef_dev`` as in
    ``cfg_ddim_step``.  ``rescale`` != 0: guidance rescale with both standard deviations over the whole clip of blends (the text
    halves blended with the same weights), a statistics launch in front of the step launch.  ``ring``: the windows lie on a ring
    of F frames (context.context_windows(loop=True)) -- window k covers the frames (starts[k] + j) mod F, 0 <= starts[k] < F; the
    ``_ring`` entry points, the same blend and step.  ``apg = (eta, threshold)``: adaptive projected guidance as in ``cfg_ddim_step``
    on the blends of the two halves, the sums over the whole clip.  ``apg_momentum = (state, carry)`` / ``carry_dev``: its momentum as
    in ``cfg_ddim_step``, the state on the clip of blends (``sample``'s layout)."""
    _dev(preds, sample, noise, starts, weights)
    nW, outer, F, L, inner = geometry = _windows_geometry(preds, sample, starts, weights)
    _check_step_noise("cfg_ddim_step_windows", sample, noise, coefs, coef_dev)
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    if apg_momentum is not None:
        state, carry = _apg_momentum_args("cfg_ddim_step_windows", apg, apg_momentum, carry_dev, sample)
        eta, threshold = _apg_args("cfg_ddim_step_windows", apg, rescale)
        ws = _apg_momentum_stats_windows(preds, sample, state, carry, carry_dev, starts, weights, geometry, mode, coefs, coef_dev, ring)
        rc = lib().im360_cfg_ddim_step_windows_apg_momentum(_p(preds), _p(sample), _p(noise), _p(state), _p(out), _p(starts), _p(weights), nW,
                                                            outer, F, L, inner, F if ring else 0, *(float(v) for v in coefs), int(mode), eta,
                                                            threshold, _p(ws), ws.numel(), carry, _p(carry_dev), _dt(sample), _stream(),
                                                            _p(coef_dev))
        _check(rc, "im360_cfg_ddim_step_windows_apg_momentum")
        return out
    if apg is not None:
        eta, threshold = _apg_args("cfg_ddim_step_windows", apg, rescale)
        ws = _apg_stats_windows(preds, sample, starts, weights, geometry, mode, coefs, coef_dev, ring)
        rc = lib().im360_cfg_ddim_step_windows_apg(_p(preds), _p(sample), _p(noise), _p(out), _p(starts), _p(weights), nW, outer, F, L, inner,
                                                   F if ring else 0, *(float(v) for v in coefs), int(mode), eta, threshold, _p(ws), ws.numel(),
                                                   _dt(sample), _stream(), _p(coef_dev))
        _check(rc, "im360_cfg_ddim_step_windows_apg")
        return out
    if rescale != 0.0:
        ws = _rescale_stats_windows(preds, sample, starts, weights, geometry, coefs[0], coef_dev, ring)
        name = "im360_cfg_ddim_step_windows_ring_rescale" if ring else "im360_cfg_ddim_step_windows_rescale"
        rc = getattr(lib(), name)(_p(preds), _p(sample), _p(noise), _p(out), _p(starts), _p(weights), nW, outer, F, L, inner,
                                  *(float(v) for v in coefs), int(mode), float(rescale), _p(ws), ws.numel(), _dt(sample), _stream(),
                                  _p(coef_dev))
        _check(rc, name)
        return out
    name = "im360_cfg_ddim_step_windows_ring" if ring else "im360_cfg_ddim_step_windows"
    rc = getattr(lib(), name)(_p(preds), _p(sample), _p(noise), _p(out), _p(starts), _p(weights), nW, outer, F, L, inner,
                              *(float(v) for v in coefs), int(mode), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, name)
    return out


def _check_multistep(who, sample, hist, mode, coefs, coef_dev):
    """``hist`` a contiguous float32 tensor of ``sample``'s element count on its device; no mode bit 8; ``coef_dev`` as in the
    DDIM step wrappers."""
    if hist is None or hist.dtype != torch.float32 or not hist.is_contiguous() or hist.numel() != sample.numel() or hist.device != sample.device:
        raise ValueError(f"{who}: history must be a contiguous float32 tensor of the sample's {sample.numel()} elements on its device")
    if int(mode) & DDIM_CLIPPED_OUTPUT:
        raise ValueError(f"{who}: mode bit {DDIM_CLIPPED_OUTPUT} (use_clipped_model_output) has no meaning for the multistep update")
    assert len(coefs) == 6
    if coef_dev is not None:
        assert coef_dev.dtype == torch.float32 and coef_dev.numel() == 6 and coef_dev.is_cuda


def cfg_multistep_step(uncond, cond, sample, hist, mode, coefs, coef_dev=None, rescale=0.0, apg=None, apg_momentum=None, carry_dev=None):
    """The DPM-Solver++ 2M update (arXiv 2211.01095, algorithm 2) of ``sample`` on uncond + g (cond - uncond), one pass:
    ``cx * sample + c0 * x0 + c1 * hist`` with x0 the prediction-type conversion (and clamp) of ``cfg_ddim_step``; ``hist`` (float32,
    like ``sample``) then holds x0, written in place, and is not read when c1 == 0.  ``mode``: DDIM_PRED_MODE | DDIM_CLIP_SAMPLE;
    ``coefs`` = (guidance, sqrt_a, sqrt_b, cx, c0, c1) (DPMSolverMultistepScheduler.multistep_coefficients); ``coef_dev`` = device
    float32[6] holding them, read by the kernel instead (graph replay).  ``rescale`` != 0: guidance rescale, the statistics launch of
    ``cfg_ddim_step`` in front of the step launch.  ``apg = (eta, threshold)``: adaptive projected guidance as in ``cfg_ddim_step``;
    ``hist`` then holds the x0 of the projected guidance.  ``apg_momentum = (state, carry)`` / ``carry_dev``: its momentum as in
    ``cfg_ddim_step``; ``state`` is a buffer of its own beside ``hist``."""
    _dev(uncond, cond, sample, hist)
    assert uncond.is_contiguous() and cond.is_contiguous() and sample.is_contiguous()
    assert uncond.shape == cond.shape == sample.shape and uncond.dtype == cond.dtype == sample.dtype
    _check_multistep("cfg_multistep_step", sample, hist, mode, coefs, coef_dev)
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    if apg_momentum is not None:
        state, carry = _apg_momentum_args("cfg_multistep_step", apg, apg_momentum, carry_dev, sample)
        eta, threshold = _apg_args("cfg_multistep_step", apg, rescale)
        ws = _apg_momentum_stats(uncond, cond, sample, state, carry, carry_dev, mode, coefs, coef_dev)
        rc = lib().im360_cfg_multistep_step_apg_momentum(_p(uncond), _p(cond), _p(sample), _p(hist), _p(state), _p(out), sample.numel(),
                                                         *(float(v) for v in coefs), int(mode), eta, threshold, _p(ws), ws.numel(), carry,
                                                         _p(carry_dev), _dt(sample), _stream(), _p(coef_dev))
        _check(rc, "im360_cfg_multistep_step_apg_momentum")
        return out
    if apg is not None:
        eta, threshold = _apg_args("cfg_multistep_step", apg, rescale)
        ws = _apg_stats(uncond, cond, sample, mode, coefs, coef_dev)
        rc = lib().im360_cfg_multistep_step_apg(_p(uncond), _p(cond), _p(sample), _p(hist), _p(out), sample.numel(), *(float(v) for v in coefs),
                                                int(mode), eta, threshold, _p(ws), ws.numel(), _dt(sample), _stream(), _p(coef_dev))
        _check(rc, "im360_cfg_multistep_step_apg")
        return out
    ws = _rescale_stats(uncond, cond, coefs[0], coef_dev) if rescale != 0.0 else None
    rc = lib().im360_cfg_multistep_step(_p(uncond), _p(cond), _p(sample), _p(hist), _p(out), sample.numel(), *(float(v) for v in coefs),
                                        int(mode), float(rescale), _p(ws), 0 if ws is None else ws.numel(), _dt(sample), _stream(),
                                        _p(coef_dev))
    _check(rc, "im360_cfg_multistep_step")
    return out


def cfg_multistep_step_windows(preds, sample, hist, starts, weights, mode, coefs, coef_dev=None, rescale=0.0, ring=False, apg=None,
                               apg_momentum=None, carry_dev=None):
    """``cfg_multistep_step`` on the per-frame weighted blend of sliding-window predictions, one pass: ``preds`` / ``starts`` /
    ``weights`` / ``ring`` as in ``cfg_ddim_step_windows``, ``hist`` float32 in ``sample``'s layout.  ``rescale`` != 0: the
    statistics launch over the blends in front of the step launch.  ``apg`` / ``apg_momentum`` / ``carry_dev``: as in
    ``cfg_ddim_step_windows``."""
    _dev(preds, sample, hist, starts, weights)
    nW, outer, F, L, inner = geometry = _windows_geometry(preds, sample, starts, weights)
    _check_multistep("cfg_multistep_step_windows", sample, hist, mode, coefs, coef_dev)
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    if apg_momentum is not None:
        state, carry = _apg_momentum_args("cfg_multistep_step_windows", apg, apg_momentum, carry_dev, sample)
        eta, threshold = _apg_args("cfg_multistep_step_windows", apg, rescale)
        ws = _apg_momentum_stats_windows(preds, sample, state, carry, carry_dev, starts, weights, geometry, mode, coefs, coef_dev, ring)
        rc = lib().im360_cfg_multistep_step_windows_apg_momentum(_p(preds), _p(sample), _p(hist), _p(state), _p(out), _p(starts), _p(weights),
                                                                 nW, outer, F, L, inner, F if ring else 0, *(float(v) for v in coefs),
                                                                 int(mode), eta, threshold, _p(ws), ws.numel(), carry, _p(carry_dev),
                                                                 _dt(sample), _stream(), _p(coef_dev))
        _check(rc, "im360_cfg_multistep_step_windows_apg_momentum")
        return out
    if apg is not None:
        eta, threshold = _apg_args("cfg_multistep_step_windows", apg, rescale)
        ws = _apg_stats_windows(preds, sample, starts, weights, geometry, mode, coefs, coef_dev, ring)
        rc = lib().im360_cfg_multistep_step_windows_apg(_p(preds), _p(sample), _p(hist), _p(out), _p(starts), _p(weights), nW, outer, F, L,
                                                        inner, F if ring else 0, *(float(v) for v in coefs), int(mode), eta, threshold, _p(ws),
                                                        ws.numel(), _dt(sample), _stream(), _p(coef_dev))
        _check(rc, "im360_cfg_multistep_step_windows_apg")
        return out
    ws = _rescale_stats_windows(preds, sample, starts, weights, geometry, coefs[0], coef_dev, ring) if rescale != 0.0 else None
    rc = lib().im360_cfg_multistep_step_windows(_p(preds), _p(sample), _p(hist), _p(out), _p(starts), _p(weights), nW, outer, F, L, inner,
                                                F if ring else 0, *(float(v) for v in coefs), int(mode), float(rescale), _p(ws),
                                                0 if ws is None else ws.numel(), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, "im360_cfg_multistep_step_windows")
    return out


# ---- the unguided forms: a step outside the guidance interval (arXiv 2404.07724; AnimationPipeline guidance_interval), where the model
#      ran the text half alone.  ``pred`` is that one prediction; ``coefs`` / ``coef_dev`` are the SIBLING's vectors (element 0, the
#      guidance, is not read), so both forms of a run share one coefficient buffer.  For finite inputs each returns what its sibling
#      returns for uncond = cond = pred, bit for bit.  No ``rescale``: a prediction rescaled towards its own deviation is itself.
def ddim_update(pred, sample, cx, cv, coef_dev=None):
    """``cfg_ddim_update`` on one prediction: cx * sample + cv * pred; ``coef_dev`` = device float32[3] (guidance, cx, cv)."""
    _dev(pred, sample)
    assert pred.is_contiguous() and sample.is_contiguous() and pred.shape == sample.shape and pred.dtype == sample.dtype
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    rc = lib().im360_ddim_update(_p(pred), _p(sample), _p(out), sample.numel(), float(cx), float(cv), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, "im360_ddim_update")
    return out


def ddim_step(pred, sample, noise, mode, coefs, coef_dev=None):
    """``cfg_ddim_step`` on one prediction: DDIMScheduler.step(pred, t, sample); ``coefs`` the six of ``step_coefficients``."""
    _dev(pred, sample, noise)
    assert pred.is_contiguous() and sample.is_contiguous() and pred.shape == sample.shape and pred.dtype == sample.dtype
    _check_step_noise("ddim_step", sample, noise, coefs, coef_dev)
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    rc = lib().im360_ddim_step(_p(pred), _p(sample), _p(noise), _p(out), sample.numel(), *(float(v) for v in coefs[1:]), int(mode),
                               _dt(sample), _stream(), _p(coef_dev))
    _check(rc, "im360_ddim_step")
    return out


def ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, coef_dev=None, ring=False):
    """``cfg_ddim_step_windows`` on the blend of the text halves alone: ``preds`` [nW, 1, *sample.shape with F -> L]."""
    _dev(preds, sample, noise, starts, weights)
    nW, outer, F, L, inner = _windows_geometry(preds, sample, starts, weights, halves=1)
    _check_step_noise("ddim_step_windows", sample, noise, coefs, coef_dev)
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    name = "im360_ddim_step_windows_ring" if ring else "im360_ddim_step_windows"
    rc = getattr(lib(), name)(_p(preds), _p(sample), _p(noise), _p(out), _p(starts), _p(weights), nW, outer, F, L, inner,
                              *(float(v) for v in coefs[1:]), int(mode), _dt(sample), _stream(), _p(coef_dev))
    _check(rc, name)
    return out


def multistep_step(pred, sample, hist, mode, coefs, coef_dev=None):
    """``cfg_multistep_step`` on one prediction; ``hist`` and ``coefs`` (the six of ``multistep_coefficients``) as there."""
    _dev(pred, sample, hist)
    assert pred.is_contiguous() and sample.is_contiguous() and pred.shape == sample.shape and pred.dtype == sample.dtype
    _check_multistep("multistep_step", sample, hist, mode, coefs, coef_dev)
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    rc = lib().im360_multistep_step(_p(pred), _p(sample), _p(hist), _p(out), sample.numel(), *(float(v) for v in coefs[1:]), int(mode),
                                    _dt(sample), _stream(), _p(coef_dev))
    _check(rc, "im360_multistep_step")
    return out


def multistep_step_windows(preds, sample, hist, starts, weights, mode, coefs, coef_dev=None, ring=False):
    """``cfg_multistep_step_windows`` on the blend of the text halves alone: ``preds`` [nW, 1, *sample.shape with F -> L]."""
    _dev(preds, sample, hist, starts, weights)
    nW, outer, F, L, inner = _windows_geometry(preds, sample, starts, weights, halves=1)
    _check_multistep("multistep_step_windows", sample, hist, mode, coefs, coef_dev)
    out = torch.empty(sample.shape, dtype=sample.dtype, device=sample.device)
    rc = lib().im360_multistep_step_windows(_p(preds), _p(sample), _p(hist), _p(out), _p(starts), _p(weights), nW, outer, F, L, inner,
                                            F if ring else 0, *(float(v) for v in coefs[1:]), int(mode), _dt(sample), _stream(),
                                            _p(coef_dev))
    _check(rc, "im360_multistep_step_windows")
    return out


def _check_latent_tables(who, ref_name, ref, noise, idx, ok):
    """``idx`` int32 / ``ok`` uint8 of one [M, ph, pw] and ``noise`` [1, F, C, h, w] for the latent ``ref`` ([1, C, F, h, w], called
    ``ref_name`` in the messages) of ``noise_latents`` / ``keep_latents``; returns (C, F, h, w, M, ph, pw)."""
    if idx.dtype != torch.int32 or ok.dtype != torch.uint8:
        raise TypeError(f"{who}: idx must be int32 and ok uint8, got {idx.dtype} and {ok.dtype}")
    if ref.dim() != 5 or ref.shape[0] != 1:
        raise ValueError(f"{who}: {ref_name} must be [1, C, F, h, w], got {list(ref.shape)}")
    _, C, F, h, w = ref.shape
    if tuple(noise.shape) != (1, F, C, h, w):
        raise ValueError(f"{who}: noise must be {[1, F, C, h, w]} for {ref_name} {list(ref.shape)}, got {list(noise.shape)}")
    if idx.dim() != 3 or idx.shape != ok.shape:
        raise ValueError(f"{who}: idx and ok must be one [M, ph, pw], got {list(idx.shape)} and {list(ok.shape)}")
    return (C, F, h, w, *idx.shape)


def _check_one_device(who, names, tensors):
    if not all(t.is_contiguous() and t.device == tensors[0].device for t in tensors):
        raise ValueError(f"{who}: {names} must be contiguous and on one device")


def noise_latents(x0, noise, idx, ok, sqrt_a, sqrt_b):
    """The start latents of a run that begins from a given clip, one launch: ``pano = T(sqrt_a * x0 + sqrt_b * noise)`` (fp32, one
    rounding) and ``pers`` = the nearest-neighbour E2P gather of the ROUNDED ``pano``, zero where a view sees nothing.
    ``x0`` 16-bit [1, C, F, h, w] (a clean panorama latent);  ``noise`` float32 [1, F, C, h, w] (the layout ``init_noise`` draws in);
    ``idx`` int32 / ``ok`` uint8 [M, ph, pw]: ``pano_geometry.nearest_e2p_index`` (values of ``idx`` in [0, h * w): a precondition);
    ``sqrt_a``, ``sqrt_b``: ``DDIMScheduler.noise_coefficients``.  Returns (pano [1, C, F, h, w], pers [1, M, C, F, ph, pw])."""
    _dev(x0, noise, idx, ok)
    dt = _dt(x0)
    if noise.dtype != torch.float32:
        raise TypeError(f"noise_latents: noise must be float32 (the dtype init_noise draws in), got {noise.dtype}")
    C, F, h, w, M, ph, pw = _check_latent_tables("noise_latents", "x0", x0, noise, idx, ok)
    _check_one_device("noise_latents", "x0, noise, idx and ok", (x0, noise, idx, ok))
    pano = torch.empty((1, C, F, h, w), dtype=x0.dtype, device=x0.device)
    pers = torch.empty((1, M, C, F, ph, pw), dtype=x0.dtype, device=x0.device)
    rc = lib().im360_noise_latents(_p(x0), _p(noise), _p(idx), _p(ok), _p(pano), _p(pers), F, C, h * w, M, ph * pw, float(sqrt_a),
                                   float(sqrt_b), dt, _stream())
    _check(rc, "im360_noise_latents")
    return pano, pers


def _check_keep(who, ncoef, pano, pers, x0, noise, mask, idx, ok, coef_dev):
    """The argument checks ``keep_latents`` and ``keep_latents_release`` share (``ncoef``: the floats of ``coef_dev``); returns the
    sizes (F, C, HW, M, Q) and the dtype code."""
    _dev(pano, pers, x0, noise, mask, idx, ok, coef_dev)
    dt = _dt(pano)
    if pers.dtype != pano.dtype or x0.dtype != pano.dtype:
        raise TypeError(f"{who}: pano, pers and x0 must have one dtype, got {pano.dtype}, {pers.dtype} and {x0.dtype}")
    if noise.dtype != torch.float32 or mask.dtype != torch.float32:
        raise TypeError(f"{who}: noise and mask must be float32, got {noise.dtype} and {mask.dtype}")
    # (the shapes of noise and idx / ok are checked in front of those of x0 and mask: of two wrong shapes the first of this list is named)
    C, F, h, w, M, ph, pw = _check_latent_tables(who, "pano", pano, noise, idx, ok)
    if x0.shape != pano.shape:
        raise ValueError(f"{who}: x0 must be {list(pano.shape)} like pano, got {list(x0.shape)}")
    if tuple(mask.shape) != (F, h, w):
        raise ValueError(f"{who}: mask must be {[F, h, w]} for pano {list(pano.shape)}, got {list(mask.shape)}")
    if tuple(pers.shape) != (1, M, C, F, ph, pw):
        raise ValueError(f"{who}: pers must be {[1, M, C, F, ph, pw]}, got {list(pers.shape)}")
    _check_one_device(who, "pano, pers, x0, noise, mask, idx and ok", (pano, pers, x0, noise, mask, idx, ok))
    if x0.data_ptr() == pano.data_ptr():
        raise ValueError(f"{who}: x0 aliases pano (the update is in place: the clean clip would be overwritten)")
    if coef_dev is not None:
        if coef_dev.dtype != torch.float32:
            raise TypeError(f"{who}: coef_dev must be float32, got {coef_dev.dtype}")
        if coef_dev.numel() != ncoef or not coef_dev.is_contiguous() or coef_dev.device != pano.device:
            raise ValueError(f"{who}: coef_dev must be a contiguous float32[{ncoef}] on the latents' device")
    return (F, C, h * w, M, ph * pw), dt


def keep_latents(pano, pers, x0, noise, mask, idx, ok, sqrt_a, sqrt_b, coef_dev=None):
    """Regenerating part of a given clip: both latents blended IN PLACE with ``known = T(sqrt_a * x0 + sqrt_b * noise)`` (the expression
    of ``noise_latents``, one rounding), one launch: ``pano = blend(pano, known, mask)`` and, where ``ok``, ``pers = blend(pers, known
    at idx, mask at idx)``; ``blend(x, k, w)`` is x untouched for w >= 1, k bit for bit for w <= 0 and ``T(fma(w, x - k, k))`` between.
    ``pano`` / ``x0`` 16-bit [1, C, F, h, w];  ``pers`` [1, M, C, F, ph, pw];  ``noise`` float32 [1, F, C, h, w];  ``mask`` float32
    [F, h, w] (1: regenerate, 0: keep);  ``idx`` int32 / ``ok`` uint8 [M, ph, pw] as for ``noise_latents``;  ``sqrt_a``, ``sqrt_b``:
    ``DDIMScheduler.keep_coefficients``;  ``coef_dev`` = device float32[2] holding them, read by the kernel instead (graph replay).
    Returns (pano, pers), the tensors given."""
    sizes, dt = _check_keep("keep_latents", 2, pano, pers, x0, noise, mask, idx, ok, coef_dev)
    rc = lib().im360_keep_latents(_p(pano), _p(pers), _p(x0), _p(noise), _p(mask), _p(idx), _p(ok), *sizes,
                                  float(sqrt_a), float(sqrt_b), dt, _stream(), _p(coef_dev))
    _check(rc, "im360_keep_latents")
    return pano, pers


def keep_latents_release(pano, pers, x0, noise, mask, idx, ok, sqrt_a, sqrt_b, tau, coef_dev=None):
    """Release mode of ``keep_latents`` (pipeline ``regenerate_mode="release"``; Differential Diffusion, arXiv 2306.00950): ``mask`` is a
    per-pixel strength and nothing is averaged.  IN PLACE, one launch: an element with ``mask <= tau`` (at ``idx`` for the views, where
    ``ok``) is PINNED -- set to ``known = T(sqrt_a * x0 + sqrt_b * noise)``, the bits ``noise_latents`` writes at the same coefficients --
    and every other element keeps its bits.  The compare is in fp32; ``tau``: ``DDIMScheduler.release_threshold``; a negative ``tau``
    pins nothing.  The tensors and their checks are those of ``keep_latents``;  ``coef_dev`` = device float32[3] holding
    ``(sqrt_a, sqrt_b, tau)``, read by the kernel instead (graph replay).  With a 0 / 1 mask and ``0 <= tau < 1`` the result is that of
    ``keep_latents``, bit for bit.  Returns (pano, pers), the tensors given."""
    sizes, dt = _check_keep("keep_latents_release", 3, pano, pers, x0, noise, mask, idx, ok, coef_dev)
    rc = lib().im360_keep_latents_release(_p(pano), _p(pers), _p(x0), _p(noise), _p(mask), _p(idx), _p(ok), *sizes,
                                          float(sqrt_a), float(sqrt_b), float(tau), dt, _stream(), _p(coef_dev))
    _check(rc, "im360_keep_latents_release")
    return pano, pers


def sphere_distance2(keep, dirs):
    """The squared chord from every pixel of an equirectangular frame to the nearest kept pixel of that frame, one launch, no
    ``HW x HW`` intermediate: ``keep`` bool or uint8 [F, h, w] (non-zero: kept), ``dirs`` float32 [h * w, 3]
    (``pano_geometry.pixel_directions``) -> float32 [F, h, w], ``min_q |dirs[p] - dirs[q]|^2`` over the kept q of the frame in fp32
    from differences, ``+inf`` for a frame that keeps nothing.  The definition is ``pano_geometry.sphere_distance2``."""
    if keep.dtype == torch.bool:
        keep = keep.to(torch.uint8)
    _dev(keep, dirs)
    if keep.dtype != torch.uint8 or dirs.dtype != torch.float32:
        raise TypeError(f"sphere_distance2: keep must be bool or uint8 and dirs float32, got {keep.dtype} and {dirs.dtype}")
    if keep.dim() != 3 or keep.numel() == 0:
        raise ValueError(f"sphere_distance2: keep must be a non-empty [F, h, w], got {list(keep.shape)}")
    F, h, w = keep.shape
    if tuple(dirs.shape) != (h * w, 3):
        raise ValueError(f"sphere_distance2: dirs must be {[h * w, 3]} for keep {list(keep.shape)}, got {list(dirs.shape)}")
    _check_one_device("sphere_distance2", "keep and dirs", (keep, dirs))
    out = torch.empty((F, h, w), dtype=torch.float32, device=keep.device)
    rc = lib().im360_sphere_distance2(_p(keep), _p(dirs), _p(out), F, h * w, _stream())
    _check(rc, "im360_sphere_distance2")
    return out


RESIZE_MODES = {"bilinear": 0, "bicubic": 1}


def resize_pano_latent(x, H, W, mode="bicubic"):
    """A clean panorama latent upscaled as the equirectangular image it is, one launch: ``x`` 16-bit [1, C, F, h, w] -> [1, C, F, H, W]
    with ``H >= h`` and ``W >= w`` (no antialiasing filter: shrinking is refused).  Half-pixel centres (``align_corners=False``) from
    integer coordinates, ``mode`` "bilinear" or "bicubic" (Keys, A = -0.75: torch's), column taps wrap around the +-180 degree seam,
    row taps clamp at the poles; fp32, horizontal pass then vertical, one rounding.  The definition is
    ``pano_geometry.resize_pano_latent``; equal sizes return the input's bits."""
    _dev(x)
    dt = _dt(x)
    if mode not in RESIZE_MODES:
        raise ValueError(f"resize_pano_latent: mode must be one of {sorted(RESIZE_MODES)}, got {mode!r}")
    if x.dim() != 5 or x.shape[0] != 1:
        raise ValueError(f"resize_pano_latent: x must be [1, C, F, h, w], got {list(x.shape)}")
    _, C, F, h, w = x.shape
    if not (isinstance(H, int) and isinstance(W, int)) or isinstance(H, bool) or isinstance(W, bool):
        raise TypeError(f"resize_pano_latent: H and W must be ints, got {H!r} and {W!r}")
    if min(C, F, h, w) < 1:
        raise ValueError(f"resize_pano_latent: x must not be empty, got {list(x.shape)}")
    if H < h or W < w:
        raise ValueError(f"resize_pano_latent: {h} x {w} -> {H} x {W} shrinks (there is no antialiasing filter; H >= h and W >= w)")
    if not x.is_contiguous():
        raise ValueError("resize_pano_latent: x must be contiguous")
    out = torch.empty((1, C, F, H, W), dtype=x.dtype, device=x.device)
    rc = lib().im360_resize_pano_latent(_p(x), _p(out), C, F, h, w, H, W, RESIZE_MODES[mode], dt, _stream())
    _check(rc, "im360_resize_pano_latent")
    return out


RETIME_MODES = {"linear": 0, "cubic": 1}


def retime_pano_latent(x, F, mode="linear", loop=False):
    """A clean panorama latent resampled along its frame axis, one launch: ``x`` 16-bit [1, C, f, h, w] -> [1, C, F, h, w] with
    ``F >= f`` (no temporal antialiasing filter: shrinking is refused).  Output frame j samples source time i0 + t from integers --
    j (f - 1) / max(F - 1, 1) on an open clip (endpoint-aligned), j f / F on a ring (``loop``) -- ``mode`` "linear" (taps i0, i0 + 1) or
    "cubic" (taps i0 - 1 .. i0 + 2, Keys, A = -0.75); tap frames clamp on an open clip and wrap on a ring; fp32, one rounding.  A frame
    with t == 0 is a copy of its source frame, bit for bit.  The definition is ``pano_geometry.retime_pano_latent``."""
    _dev(x)
    dt = _dt(x)
    if mode not in RETIME_MODES:
        raise ValueError(f"retime_pano_latent: mode must be one of {sorted(RETIME_MODES)}, got {mode!r}")
    if x.dim() != 5 or x.shape[0] != 1:
        raise ValueError(f"retime_pano_latent: x must be [1, C, f, h, w], got {list(x.shape)}")
    _, C, f, h, w = x.shape
    if not isinstance(F, int) or isinstance(F, bool):
        raise TypeError(f"retime_pano_latent: F must be an int, got {F!r}")
    if min(C, f, h, w) < 1:
        raise ValueError(f"retime_pano_latent: x must not be empty, got {list(x.shape)}")
    if F < f:
        raise ValueError(f"retime_pano_latent: {f} -> {F} frames shrinks (there is no temporal antialiasing filter; F >= f)")
    if not x.is_contiguous():
        raise ValueError("retime_pano_latent: x must be contiguous")
    out = torch.empty((1, C, F, h, w), dtype=x.dtype, device=x.device)
    rc = lib().im360_retime_pano_latent(_p(x), _p(out), C, f, F, h * w, RETIME_MODES[mode], int(bool(loop)), dt, _stream())
    _check(rc, "im360_retime_pano_latent")
    return out


def free_init_noise(x0, n1, n2, Lf, Lh, Lw, sa, sb):
    """FreeInit's effective noise (arXiv 2312.07537), three launches: ``x0`` 16-bit [1, 4, F, h, w] (the clean clip), ``n1`` / ``n2`` float32
    [1, F, 4, h, w] (the noise the clip was generated from, a fresh draw) -> ``n_eff`` float32 [1, F, 4, h, w] with
    ``sa x0 + sb n_eff = n2 + L (sa x0 + sb n1 - n2)``, L = ``Lf`` (x) ``Lh`` (x) ``Lw``: float32 [F, F], [h, h], [w, w]
    (``pano_geometry.free_init_operator`` in fp64, rounded once).  fp32 fma chains, deterministic; identity operators return ``n1``'s
    bits.  ``sb`` must be positive (pure signal has no noise to replace); 1 / sb is formed in fp64 here.  The definition is
    ``pano_geometry.free_init_noise``."""
    _dev(x0, n1, n2, Lf, Lh, Lw)
    dt = _dt(x0)
    if x0.dim() != 5 or x0.shape[0] != 1:
        raise ValueError(f"free_init_noise: x0 must be [1, C, F, h, w], got {list(x0.shape)}")
    _, C, F, h, w = x0.shape
    if min(C, F, h, w) < 1:
        raise ValueError(f"free_init_noise: x0 must not be empty, got {list(x0.shape)}")
    for name, n in (("n1", n1), ("n2", n2)):
        if n.dtype != torch.float32 or tuple(n.shape) != (1, F, C, h, w):
            raise ValueError(f"free_init_noise: {name} must be float32 [1, {F}, {C}, {h}, {w}], got {n.dtype} {list(n.shape)}")
    for name, L, n in (("Lf", Lf, F), ("Lh", Lh, h), ("Lw", Lw, w)):
        if L.dtype != torch.float32 or tuple(L.shape) != (n, n):
            raise ValueError(f"free_init_noise: {name} must be float32 [{n}, {n}], got {L.dtype} {list(L.shape)}")
    for name, t in (("x0", x0), ("n1", n1), ("n2", n2), ("Lf", Lf), ("Lh", Lh), ("Lw", Lw)):
        if t.device != x0.device:
            raise ValueError(f"free_init_noise: {name} is on {t.device}, x0 on {x0.device}")
        if not t.is_contiguous():
            raise ValueError(f"free_init_noise: {name} must be contiguous")
    sa, sb = float(sa), float(sb)
    if not sb > 0.0:
        raise ValueError(f"free_init_noise: sb={sb} must be positive (pure signal has no noise to replace)")
    out = torch.empty((1, F, C, h, w), dtype=torch.float32, device=x0.device)
    ws = torch.empty(2 * out.numel(), dtype=torch.float32, device=x0.device)
    rc = lib().im360_free_init_noise(_p(x0), _p(n1), _p(n2), _p(Lf), _p(Lh), _p(Lw), _p(out), _p(ws), ws.numel(), C, F, h, w, sa, sb,
                                     1.0 / sb, dt, _stream())
    _check(rc, "im360_free_init_noise")
    return out


# ------------------------------------------------------------------------------------------ tuning knobs
KNOBS = {"attn_qb": 0, "conv_big": 1, "conv_bk": 2, "tattn_scalar": 3, "conv_ring": 4, "attn_hl": 5, "conv_dbg": 6, "conv_halo": 7, "conv_cm": 8, "ln_packed": 9,
         "ring_groups": 10, "attn_x": 11, "attn_ds": 12, "attn_one": 13, "attn_dbg": 14, "attn_hg": 15, "conv_small": 16, "attn_w3": 17, "attn_pipe": 18, "conv_stag": 19, "conv_persist": 20, "gn_apply": 21, "tattn_nt": 22, "nt": 23, "g4": 24, "gn_wgs": 25, "conv_ksplit": 26, "ff_fused": 27}


ATTN_PIPE_DEFAULT = -1         # the library's default for the attn_pipe knob (abi.cpp)


def ablate_build():
    """True when the library was built with `make ablate` (rejected A/B variants and ablation kernels compiled in)."""
    return bool(lib().im360_build_flags() & 1)


def tuning_set(name, value):
    """A/B switches of the launchers (tools/bench_kernels.py).  Defaults are the measured best, see DESIGN.md section 3b';
    conv_halo / conv_cm change the fp32 summation order, attn_x (0 against 1 - 3) and attn_ds the 16-bit rounding points,
    conv_dbg / attn_dbg break results on purpose, the others do not change results."""
    _check(lib().im360_tuning_set(KNOBS[name], int(value)), "im360_tuning_set")


def tuning_get(name):
    """The knob's current value in the library (its default, the IM360_* environment variable or the last ``tuning_set``)."""
    return lib().im360_tuning_get(KNOBS[name])


# ------------------------------------------------------------------------------------------ profiling
def prof_enable(kinds):
    mask = 0
    for k in kinds:
        mask |= 1 << PROF_KINDS[k]
    lib().im360_prof_enable(mask)


def prof_collect(kind):
    ms, n = ctypes.c_double(0.0), ctypes.c_long(0)
    lib().im360_prof_collect(PROF_KINDS[kind], ctypes.byref(ms), ctypes.byref(n))
    return ms.value, n.value
