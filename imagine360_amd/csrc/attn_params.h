// Parameter block shared by the attention kernels (attn_fwd.hip, attn_pipe.hip).  Host + device, gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
namespace im360 {

struct AttnParams {
    const void* q = nullptr; const void* k = nullptr; const void* v = nullptr; const void* bias = nullptr; void* out = nullptr;
    const void* bias_alt = nullptr; const int* bias_sel = nullptr;     // *bias_sel != 0 -> use bias_alt (decided on the device: graph-replay safe)
    int B = 0, H = 0, Nq = 0, Nk = 0;
    int nqt = 0;             // query tiles per (batch, head)
    int kv_group = 0;        // K/V batch index = query batch index / kv_group (context shared by the frames of a video)
    long q_bs = 0, q_rs = 0, k_bs = 0, k_rs = 0, v_bs = 0, v_rs = 0, o_bs = 0, o_rs = 0, bias_rs = 0;   // element strides
    float scale_log2 = 0.f;    // logit scale * log2(e)
    float out_scale = 0.f;     // multiplies the normalised result
    int accumulate = 0;      // out += result instead of out = result
    int bias_packed = 0;     // bias / bias_alt are fp16 matrices pre-multiplied by log2(e) (im360_attn_pack_bias)
    // packed bias only (round 6): one bit per (32-query block, 32-key half), row stride blocks_rs words: 0 = every entry of that 32 x 32
    // block of the packed matrix is zero, the kernel then skips its fragment loads and its two bias MFMAs.  nullptr: no map.
    const uint32_t* bias_blocks = nullptr; const uint32_t* bias_blocks_alt = nullptr; int blocks_rs = 0;
    // optional SECOND key/value set of the same queries (DUAL kernels): out = out_scale * attn(q, k, v) + out_scale2 *
    // attn(q, k2, v2), two independent softmaxes -- the text + IP-adapter cross attention in ONE launch
    const void* k2 = nullptr; const void* v2 = nullptr;
    int Nk2 = 0;
    long k2_bs = 0, k2_rs = 0, v2_bs = 0, v2_rs = 0;
    float out_scale2 = 0.f;
    // resident-K/V cross attention (xattn_resident_kernel): query blocks (32 rows) per image, per (K/V batch, head) pair, in total
    int x_nqb = 0, x_bpp = 0;
    long x_total = 0;
};

// the one-dimensional grid of `nblk` workgroups, for every attention launcher (`who` names it in the message)
static inline int attn_grid(const char* who, long nblk, dim3& grid) {
    if (nblk > 0x7fffffffL) {
        im360_set_error("%s: %ld workgroups exceed the grid limit", who, nblk);
        return IM360_ERR_ARG;
    }
    grid = dim3((unsigned)nblk, 1, 1);
    return IM360_OK;
}

// Software-pipelined d = 64 self-attention (attn_pipe.hip).  Returns IM360_OK, or 1 when the shape is not one it takes
// (the caller then falls back to attn_fwd_kernel).
int launch_attn_pipe(const AttnParams& p, int dtype, hipStream_t stream);

}  // namespace im360
