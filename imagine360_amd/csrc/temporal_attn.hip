// Motion-module temporal self-attention (sequence = frames) for gfx950.
//
// Replaces VersatileAttention's explicit baddbmm -> softmax -> bmm path
// (animatediff/models/motion_module.py:343-429 -> diffusers/models/attention_processor.py:562-591),
// including the '(b f) d c -> (b d) f c' / back layout shuffles (motion_module.py:348, 427): the
// kernel indexes the token-major activations [B, F, P, heads*d] with strides instead of moving them.
//
// HBM-bound by its data (AI ~ 8 flop/B) -- but only if the arithmetic is cheap: a scalar-FMA version spends ~3300
// VALU instructions per query row unpacking 16-bit K/V and runs VALU-bound at ~1.7 TB/s.  Up to 16 frames (the
// shipped configuration) therefore run on 16x16 MFMA tiles: one workgroup stages the q|k|v rows of one pixel (all
// frames) into LDS with coalesced 16-byte loads, each wave takes (pixel, head) pairs: S^T = K Q^T in
// ceil(d/32) MFMAs, softmax on the 4 scores a lane holds (+2 cross-lane exchanges), O^T = V^T P^T in ceil(d/16)
// MFMAs with V gathered by the transposing LDS read, results written over the head's Q slice in LDS and then
// streamed out as whole token rows.  HBM sees q, k, v, o exactly once.  17 .. 64 frames (frame-sharded 48-frame runs)
// run the same scheme on FT x FT tiles (temporal_attn_mfma_long_kernel); the scalar kernel below remains as the
// fallback for head groups that do not fit 64 KB of LDS and behind the tattn_scalar knob.
#include <stdlib.h>
#include "common.h"

namespace im360 {

struct TAttnParams {
    const void* q; const void* k; const void* v; void* out;
    long total;             // B * P * F * heads threads
    int F, P, heads, d;
    long q_fs, q_ps, q_bs;  // element strides of (frame, pixel, batch) for q; k, v share them via offsets
    long k_fs, k_ps, k_bs;
    long v_fs, v_ps, v_bs;
    long o_fs, o_ps, o_bs;
    float scale_log2;
};

// One workgroup = PPB pixels x F frames x heads threads (one query row per thread).  The K and V rows of a
// pixel (F x C each, contiguous 2C-element spans of the fused QKV rows) are staged ONCE into LDS with
// coalesced 16-byte loads issued back to back (deep memory-level parallelism), then every thread reads its
// head's K/V chunks from LDS (threads of one head read the same address -> broadcast).  HBM sees q, k, v, o
// exactly once; the scores never leave registers.
template <typename T, int FMAX>
__global__ __launch_bounds__(512) void temporal_attn_lds_kernel(TAttnParams p, int ppb, int hpb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* kv = (T*)smem;                                   // [ppb][F][k | v][hpb * d]
    const int F = p.F, d = p.d;
    const int G = hpb * d;                              // channels of this block's head group
    const int h0 = blockIdx.y * hpb;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long pix0 = (long)blockIdx.x * ppb;           // flattened (b, pixel)
    const long npix = (long)p.total;                    // B * P
    // ---- stage K and V of the head group: chunk id -> (pixel, frame, k|v, 16-byte chunk)
    const int cpr = G >> 3;
    const int nchunks = ppb * F * 2 * cpr;
    for (int c = tid; c < nchunks; c += nthr) {
        const int ch = c % cpr;
        const int kvsel = (c / cpr) & 1;
        const int f = (c / (2 * cpr)) % F;
        const int pl = c / (2 * cpr * F);
        const long pix = min(pix0 + pl, npix - 1);
        const long b = pix / p.P, px = pix % p.P;
        const T* base = kvsel ? (const T*)p.v + b * p.v_bs + px * p.v_ps + (long)f * p.v_fs
                              : (const T*)p.k + b * p.k_bs + px * p.k_ps + (long)f * p.k_fs;
        *(uint4*)(kv + (long)c * 8) = *(const uint4*)(base + h0 * d + ch * 8);
    }
    __syncthreads();
    // ---- one query row per thread: tid -> (pixel, frame i, head), head fastest
    const int hl = tid % hpb;
    const int i = (tid / hpb) % F;
    const int pl = tid / (hpb * F);
    const long pix = pix0 + pl;
    if (pl >= ppb || pix >= npix) return;
    const long b = pix / p.P, px = pix % p.P;
    const int nch = d >> 3;
    const T* qp = (const T*)p.q + b * p.q_bs + px * p.q_ps + (long)i * p.q_fs + (long)(h0 + hl) * d;
    T* op = (T*)p.out + b * p.o_bs + px * p.o_ps + (long)i * p.o_fs + (long)(h0 + hl) * d;
    const T* kl = kv + (long)pl * F * 2 * G + hl * d;   // + j * 2G (+ G for V)
    float s[FMAX];
#pragma unroll
    for (int j = 0; j < FMAX; ++j) s[j] = 0.f;
    for (int c = 0; c < nch; ++c) {
        float qf[8];
        unpack8<T>(*(const uint4*)(qp + c * 8), qf);
#pragma unroll
        for (int j = 0; j < FMAX; ++j) {
            float kf[8];
            unpack8<T>(*(const uint4*)(kl + (long)min(j, F - 1) * 2 * G + c * 8), kf);
            float acc = s[j];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qf[e], kf[e], acc);
            s[j] = acc;
        }
    }
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < FMAX; ++j) {
        s[j] = (j < F) ? s[j] * p.scale_log2 : -INFINITY;
        m = fmaxf(m, s[j]);
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < FMAX; ++j) {
        s[j] = __builtin_amdgcn_exp2f(s[j] - m);
        l += s[j];
    }
    const float inv = 1.0f / l;
    for (int c = 0; c < nch; ++c) {
        float of[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < FMAX; ++j) {
            float vf[8];
            unpack8<T>(*(const uint4*)(kl + (long)min(j, F - 1) * 2 * G + G + c * 8), vf);
#pragma unroll
            for (int e = 0; e < 8; ++e) of[e] = fmaf(s[j], vf[e], of[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) of[e] *= inv;
        *(uint4*)(op + c * 8) = pack8<T>(of);
    }
}

// ---- F <= 16: one workgroup (4 waves) = one (batch, pixel) x hpb heads
// NT (knob tattn_nt; tools/ab_knob-style A/B in tools/ab_tattn.py): bit 0 = the output rows leave with non-temporal stores, bit 1 = q | k | v
// arrive with non-temporal loads -- both streams are touched exactly once by this kernel.
template <typename T, int NT = 0>
__global__ __launch_bounds__(256) void temporal_attn_mfma_kernel(TAttnParams p, int hpb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* rows = (T*)smem;                                 // [16 frames][q_g | k_g | v_g | 8 pad], g = this block's heads
    const int F = p.F, d = p.d;
    const int G = hpb * d;
    const int pitch = 3 * G + 8;                        // +16 bytes: the 16 frame rows start 4 banks apart
    const int h0 = blockIdx.y * hpb;
    const int tid = threadIdx.x;
    const long pix = blockIdx.x;
    const long b = pix / p.P, px = pix % p.P;
    // ---- stage: chunk id -> (frame, q|k|v, 16-byte chunk); frames >= F are zero rows
    const int cps = G >> 3;
    for (int c = tid; c < 16 * 3 * cps; c += 256) {
        const int ch = c % cps, seg = (c / cps) % 3, f = c / (3 * cps);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (f < F) {
            const T* base = seg == 0 ? (const T*)p.q + b * p.q_bs + px * p.q_ps + (long)f * p.q_fs
                          : seg == 1 ? (const T*)p.k + b * p.k_bs + px * p.k_ps + (long)f * p.k_fs
                                     : (const T*)p.v + b * p.v_bs + px * p.v_ps + (long)f * p.v_fs;
            if constexpr ((NT & 2) != 0) {
                const u32x4 r = __builtin_nontemporal_load((const u32x4*)(base + h0 * d + ch * 8));
                v = make_uint4(r.x, r.y, r.z, r.w);
            } else {
                v = *(const uint4*)(base + h0 * d + ch * 8);
            }
        }
        *(uint4*)(rows + f * pitch + seg * G + ch * 8) = v;
    }
    __syncthreads();
    const int lane = tid & 63, wid = tid >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int nstep = (d + 31) >> 5, ncb = (d + 15) >> 4;
    for (int hl = wid; hl < hpb; hl += 4) {
        // ---- S^T = K Q^T: lane (query i16, g) ends up with the scores of keys 4g .. 4g+3
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int st = 0; st < nstep; ++st) {
            const int k0 = st * 32 + 8 * g;
            uint4 kf = make_uint4(0u, 0u, 0u, 0u), qf = kf;
            if (k0 < d) {                                // d % 8 == 0: an 8-channel chunk is all in or all out
                kf = *(const uint4*)(rows + i16 * pitch + G + hl * d + k0);
                qf = *(const uint4*)(rows + i16 * pitch + hl * d + k0);
            }
            s = Mfma16<T>::k32(kf, qf, s);
        }
        float m = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = (4 * g + r < F) ? s[r] * p.scale_log2 : -INFINITY;
            m = fmaxf(m, s[r]);
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float l = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = __builtin_amdgcn_exp2f(s[r] - m);
            l += s[r];
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
        u32x2 pf;                                        // P^T as the B operand: column = query, k = keys 4g .. 4g+3
        pf.x = pack2<T>(s[0], s[1]);
        pf.y = pack2<T>(s[2], s[3]);
        // ---- O^T = V^T P^T per 16-channel block; lane (query i16, g) gets channels c0 + 4g .. +3
        for (int cb = 0; cb < ncb; ++cb) {
            const int c0 = cb * 16;
            const u32x2 vf = lds_read_tr16(rows + (4 * g + (i16 >> 2)) * pitch + 2 * G + hl * d + c0 + 4 * (i16 & 3));
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            o = Mfma16<T>::k16(vf, pf, o);
            if (c0 + 4 * g < d) {                        // the head's Q slice is dead after QK^T: park the output there
                uint2 w;
                w.x = pack2<T>(o[0] * inv, o[1] * inv);
                w.y = pack2<T>(o[2] * inv, o[3] * inv);
                *(uint2*)(rows + i16 * pitch + hl * d + c0 + 4 * g) = w;
            }
        }
    }
    __syncthreads();
    // ---- whole token rows out
    for (int c = tid; c < 16 * cps; c += 256) {
        const int ch = c % cps, f = c / cps;
        if (f < F) {
            const uint4 w = *(const uint4*)(rows + f * pitch + ch * 8);
            T* dst = (T*)p.out + b * p.o_bs + px * p.o_ps + (long)f * p.o_fs + h0 * d + ch * 8;
            if constexpr ((NT & 1) != 0) __builtin_nontemporal_store(u32x4{w.x, w.y, w.z, w.w}, (u32x4*)dst);
            else *(uint4*)dst = w;
        }
    }
}


// ---- 17 <= F <= 64 (frame-sharded long clips, BASELINE cfg4): the same scheme on FT x FT tiles of 16 x 16.  One workgroup
//      stages the FT * 16 frame rows (q | k | v of its head group) of one pixel; the (head, query tile) pairs are dealt to
//      the four waves; per pair: S^T against all FT key tiles (FT * ceil(d / 32) MFMAs), softmax over the FT * 4 scores a
//      lane holds (+ 2 exchanges), O^T = sum over key tiles of V^T P^T, parked over the head's Q rows of that query tile.
template <typename T, int FT>
__global__ __launch_bounds__(256) void temporal_attn_mfma_long_kernel(TAttnParams p, int hpb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* rows = (T*)smem;                                 // [FT * 16 frames][q_g | k_g | v_g | 8 pad]
    constexpr int NR = FT * 16;
    const int F = p.F, d = p.d;
    const int G = hpb * d;
    const int pitch = 3 * G + 8;
    const int h0 = blockIdx.y * hpb;
    const int tid = threadIdx.x;
    const long pix = blockIdx.x;
    const long b = pix / p.P, px = pix % p.P;
    const int cps = G >> 3;
    for (int c = tid; c < NR * 3 * cps; c += 256) {
        const int ch = c % cps, seg = (c / cps) % 3, f = c / (3 * cps);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (f < F) {
            const T* base = seg == 0 ? (const T*)p.q + b * p.q_bs + px * p.q_ps + (long)f * p.q_fs
                          : seg == 1 ? (const T*)p.k + b * p.k_bs + px * p.k_ps + (long)f * p.k_fs
                                     : (const T*)p.v + b * p.v_bs + px * p.v_ps + (long)f * p.v_fs;
            v = *(const uint4*)(base + h0 * d + ch * 8);
        }
        *(uint4*)(rows + f * pitch + seg * G + ch * 8) = v;
    }
    __syncthreads();
    const int lane = tid & 63, wid = tid >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int nstep = (d + 31) >> 5, ncb = (d + 15) >> 4;
    for (int pair = wid; pair < hpb * FT; pair += 4) {
        const int hl = pair / FT, qi = pair % FT;
        const T* qrow = rows + (qi * 16 + i16) * pitch + hl * d;
        // ---- S^T tiles: lane (query qi * 16 + i16, g) gets the scores of keys kt * 16 + 4g .. + 3
        f32x4 s[FT];
#pragma unroll
        for (int kt = 0; kt < FT; ++kt) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int st = 0; st < nstep; ++st) {
            const int k0 = st * 32 + 8 * g;
            uint4 qf = make_uint4(0u, 0u, 0u, 0u);
            if (k0 < d) qf = *(const uint4*)(qrow + k0);
#pragma unroll
            for (int kt = 0; kt < FT; ++kt) {
                uint4 kf = make_uint4(0u, 0u, 0u, 0u);
                if (k0 < d) kf = *(const uint4*)(rows + (kt * 16 + i16) * pitch + G + hl * d + k0);
                s[kt] = Mfma16<T>::k32(kf, qf, s[kt]);
            }
        }
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < FT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kt][r] = (kt * 16 + 4 * g + r < F) ? s[kt][r] * p.scale_log2 : -INFINITY;
                m = fmaxf(m, s[kt][r]);
            }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        float l = 0.f;
        u32x2 pf[FT];                                    // P^T per key tile as the B operand
#pragma unroll
        for (int kt = 0; kt < FT; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - m);
                l += s[kt][r];
            }
            pf[kt].x = pack2<T>(s[kt][0], s[kt][1]);
            pf[kt].y = pack2<T>(s[kt][2], s[kt][3]);
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
        // ---- O^T = sum over key tiles of V^T P^T, per 16-channel block
        for (int cb = 0; cb < ncb; ++cb) {
            const int c0 = cb * 16;
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kt = 0; kt < FT; ++kt) {
                const u32x2 vf = lds_read_tr16(rows + (kt * 16 + 4 * g + (i16 >> 2)) * pitch + 2 * G + hl * d + c0 + 4 * (i16 & 3));
                o = Mfma16<T>::k16(vf, pf[kt], o);
            }
            if (c0 + 4 * g < d) {                        // this query tile's Q rows of the head are dead: park the output there
                uint2 w;
                w.x = pack2<T>(o[0] * inv, o[1] * inv);
                w.y = pack2<T>(o[2] * inv, o[3] * inv);
                *(uint2*)(rows + (qi * 16 + i16) * pitch + hl * d + c0 + 4 * g) = w;
            }
        }
    }
    __syncthreads();
    for (int c = tid; c < NR * cps; c += 256) {
        const int ch = c % cps, f = c / cps;
        if (f < F)
            *(uint4*)((T*)p.out + b * p.o_bs + px * p.o_ps + (long)f * p.o_fs + h0 * d + ch * 8) =
                *(const uint4*)(rows + f * pitch + ch * 8);
    }
}

// ---- windowed: F <= 64 frames attended as nW sliding windows of L <= 16 frames, the windows' outputs fused per frame (FreeNoise's
//      window-based attention fusion, arXiv 2310.15169 section 3.2).  One workgroup = one (batch, pixel) x hpb heads, as above.  The F base rows
//      q | k | v (the projection WITHOUT the frame PE) and the L projected PE rows are staged once; per window the 16 window rows
//      round_T(base[f] + table[p]) are built in LDS (rows p >= L zero and masked), the 16 x 16 MFMA routine of temporal_attn_mfma_kernel
//      runs per head, and w[p] / (sum of the weights of the windows covering f) times the fp32 output is added into an fp32 accumulator
//      [F][hpb * d] in LDS: each (frame, channel) belongs to one lane per window and the windows are separated by barriers, so plain
//      read-modify-writes do.  Product and sum are rounded separately (no fma): with two windows on a frame the result does not depend on
//      their order.  HBM sees q, k, v once and every output element once, rounded once.
struct TWinParams {
    const void* pe;         // [L][3 * heads * d]: PE rows 0 .. L-1 through the fused QKV weight
    int nW, L, ring;
    int starts[64];
    float weights[16];
};

// a + w * o with the product rounded on its own: an fma would make the sum over two windows depend on which one comes first.  The file
// is built with fast contraction, which the backend applies whatever a pragma says (seen on the MI355X: the order changed the bits), so
// the product passes through an empty asm statement (no instruction, no memory) that the combiner cannot look through.
__device__ __forceinline__ float add_product(float a, float w, float o) {
    float pr = w * o;
    asm volatile("" : "+v"(pr));
    return a + pr;
}

template <typename T>
__global__ __launch_bounds__(256) void temporal_attn_windows_kernel(TAttnParams p, TWinParams w, int hpb) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int F = p.F, d = p.d, L = w.L;
    const int G = hpb * d;
    const int pitch = 3 * G + 8;
    T* base = (T*)smem;                                 // [F][q_g | k_g | v_g | 8 pad]
    T* tab = base + F * pitch;                          // [L][q_g | k_g | v_g]
    T* rows = tab + L * 3 * G;                          // [16 positions][q_g | k_g | v_g | 8 pad]: the window under work
    float* acc = (float*)(rows + 16 * pitch);           // [F][G]
    float* wsum = acc + F * G;                          // [F]: sum of the weights of the windows that cover a frame
    const int h0 = blockIdx.y * hpb;
    const int tid = threadIdx.x;
    const long pix = blockIdx.x;
    const long b = pix / p.P, px = pix % p.P;
    const int C3 = 3 * p.heads * d;
    const int cps = G >> 3;
    // ---- stage the base rows and the table, clear the accumulator and the rows p >= L of the window
    for (int c = tid; c < F * 3 * cps; c += 256) {
        const int ch = c % cps, seg = (c / cps) % 3, f = c / (3 * cps);
        const T* src = seg == 0 ? (const T*)p.q + b * p.q_bs + px * p.q_ps + (long)f * p.q_fs
                     : seg == 1 ? (const T*)p.k + b * p.k_bs + px * p.k_ps + (long)f * p.k_fs
                                : (const T*)p.v + b * p.v_bs + px * p.v_ps + (long)f * p.v_fs;
        *(uint4*)(base + f * pitch + seg * G + ch * 8) = *(const uint4*)(src + h0 * d + ch * 8);
    }
    for (int c = tid; c < L * 3 * cps; c += 256) {
        const int ch = c % cps, seg = (c / cps) % 3, pp = c / (3 * cps);
        *(uint4*)(tab + pp * 3 * G + seg * G + ch * 8) = *(const uint4*)((const T*)w.pe + (long)pp * C3 + seg * (p.heads * d) + h0 * d + ch * 8);
    }
    for (int c = tid; c < (16 - L) * 3 * cps; c += 256)
        *(uint4*)(rows + (L + c / (3 * cps)) * pitch + (c % (3 * cps)) * 8) = make_uint4(0u, 0u, 0u, 0u);
    for (int c = tid; c < F * G; c += 256) acc[c] = 0.f;
    if (tid < F) {
        float sum = 0.f;
        for (int k = 0; k < w.nW; ++k) {
            int pp = tid - w.starts[k];
            if (w.ring && pp < 0) pp += F;
            if (pp >= 0 && pp < L) sum += w.weights[pp];
        }
        wsum[tid] = sum;
    }
    const int lane = tid & 63, wid = tid >> 6;
    const int i16 = lane & 15, g = lane >> 4;
    const int nstep = (d + 31) >> 5, ncb = (d + 15) >> 4;
    const int nsplit = hpb >= 4 ? 1 : 4 / hpb;          // fewer than four heads: the waves share a head's channel blocks
    for (int k = 0; k < w.nW; ++k) {
        const int s0 = w.starts[k];
        __syncthreads();                                 // the staging / the previous window's MFMA reads of `rows` are done
        // ---- window rows: round_T(base[frame of position] + table[position])
        for (int c = tid; c < L * 3 * cps; c += 256) {
            const int cc = c % (3 * cps), pp = c / (3 * cps);
            int f = s0 + pp;
            if (f >= F) f -= F;                          // (ring; on a line s0 + L <= F)
            float x[8], t[8];
            unpack8<T>(*(const uint4*)(base + f * pitch + cc * 8), x);
            unpack8<T>(*(const uint4*)(tab + pp * 3 * G + cc * 8), t);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] += t[e];
            *(uint4*)(rows + pp * pitch + cc * 8) = pack8<T>(x);
        }
        __syncthreads();
        const bool live = i16 < L;
        int fq = live ? s0 + i16 : 0;                    // the frame of this lane's query position
        if (fq >= F) fq -= F;
        const float wq = live ? w.weights[i16] / wsum[fq] : 0.f;
        for (int task = wid; task < hpb * nsplit; task += 4) {
            const int hl = task / nsplit, part = task % nsplit;
            // ---- S^T = K Q^T: lane (query i16, g) ends up with the scores of keys 4g .. 4g+3
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            for (int st = 0; st < nstep; ++st) {
                const int k0 = st * 32 + 8 * g;
                uint4 kf = make_uint4(0u, 0u, 0u, 0u), qf = kf;
                if (k0 < d) {
                    kf = *(const uint4*)(rows + i16 * pitch + G + hl * d + k0);
                    qf = *(const uint4*)(rows + i16 * pitch + hl * d + k0);
                }
                s = Mfma16<T>::k32(kf, qf, s);
            }
            float m = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[r] = (4 * g + r < L) ? s[r] * p.scale_log2 : -INFINITY;
                m = fmaxf(m, s[r]);
            }
            m = fmaxf(m, __shfl_xor(m, 16));
            m = fmaxf(m, __shfl_xor(m, 32));
            float l = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[r] = __builtin_amdgcn_exp2f(s[r] - m);
                l += s[r];
            }
            l += __shfl_xor(l, 16);
            l += __shfl_xor(l, 32);
            const float inv = 1.0f / l;
            u32x2 pf;
            pf.x = pack2<T>(s[0], s[1]);
            pf.y = pack2<T>(s[2], s[3]);
            // ---- O^T = V^T P^T per 16-channel block; lane (query i16, g) gets channels c0 + 4g .. +3 and adds them to its frame
            for (int cb = part; cb < ncb; cb += nsplit) {
                const int c0 = cb * 16;
                const u32x2 vf = lds_read_tr16(rows + (4 * g + (i16 >> 2)) * pitch + 2 * G + hl * d + c0 + 4 * (i16 & 3));
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                o = Mfma16<T>::k16(vf, pf, o);
                if (live && c0 + 4 * g < d) {
                    float4* a = (float4*)(acc + fq * G + hl * d + c0 + 4 * g);
                    float4 v = *a;
                    v.x = add_product(v.x, wq, o[0] * inv);
                    v.y = add_product(v.y, wq, o[1] * inv);
                    v.z = add_product(v.z, wq, o[2] * inv);
                    v.w = add_product(v.w, wq, o[3] * inv);
                    *a = v;
                }
            }
        }
    }
    __syncthreads();
    // ---- whole token rows out, rounded once
    for (int c = tid; c < F * cps; c += 256) {
        const int ch = c % cps, f = c / cps;
        const float* a = acc + f * G + ch * 8;
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = a[e];
        *(uint4*)((T*)p.out + b * p.o_bs + px * p.o_ps + (long)f * p.o_fs + h0 * d + ch * 8) = pack8<T>(o);
    }
}


// ---- host side -----------------------------------------------------------------------------------------------------------
// the scalar fallback; npix = B * P
template <typename T, int FMAX>
static void launch_tattn_v(TAttnParams p, long npix, hipStream_t stream) {
    int hpb = p.heads;                                                  // heads per block: keep one pixel's K|V <= 48 KiB
    while (hpb > 1 && (hpb % 2) == 0 && ((long)p.F * 2 * hpb * p.d * sizeof(T) > 48 * 1024 || p.F * hpb > 512)) hpb /= 2;
    const long bytes_per_pix = (long)p.F * 2 * hpb * p.d * sizeof(T);
    const int per_pix_threads = p.F * hpb;
    int ppb = 256 / per_pix_threads;
    if (ppb < 1) ppb = 1;
    while (ppb > 1 && ppb * bytes_per_pix > 48 * 1024) --ppb;
    const int threads = ((ppb * per_pix_threads + 63) / 64) * 64;
    p.total = npix;
    dim3 grid((unsigned)((npix + ppb - 1) / ppb), (unsigned)(p.heads / hpb));
    hipLaunchKernelGGL((temporal_attn_lds_kernel<T, FMAX>), grid, dim3(threads), (size_t)(ppb * bytes_per_pix), stream, p, ppb, hpb);
}

// The MFMA kernels' workgroup: `nr` frame rows of (3 * hpb * d + 8) elements (+ 64 bytes) in LDS, the heads per workgroup halved until the rows
// fit `budget` bytes (or no further halving is possible: the caller checks lds)
struct TattnRows { int hpb; size_t lds; };
template <typename T>
static TattnRows tattn_rows(const TAttnParams& p, int nr, size_t budget) {
    auto bytes = [&](int hpb) { return (size_t)nr * (3 * hpb * p.d + 8) * sizeof(T) + 64; };
    int hpb = p.heads;
    while (hpb > 1 && (hpb % 2) == 0 && bytes(hpb) > budget) hpb /= 2;
    return TattnRows{hpb, bytes(hpb)};
}

template <typename T>
static int launch_tattn(const TAttnParams& p, hipStream_t stream) {
    const long npix = p.total / ((long)p.F * p.heads);                 // B * P
    const int ft = (p.F + 15) / 16;                                    // 16-frame tiles: 1 = temporal_attn_mfma_kernel, 2 - 4 = the long kernel
    // up to 16 frames: ~32 KB of LDS rows (3 * hpb * d <= 1248 channels); more: whatever fits 64 KB
    const size_t budget = ft == 1 ? (size_t)16 * (1248 + 8) * sizeof(T) + 64 : (size_t)64 * 1024;
    const TattnRows r = tattn_rows<T>(p, ft * 16, budget);
    if (!knob(KNOB_TATTN_SCALAR) && r.lds <= 64 * 1024) {             // (knob tattn_scalar: tuning override)
        const dim3 grid((unsigned)npix, (unsigned)(p.heads / r.hpb));
        if (ft == 1) with_const<0, 1, 2, 3>(knob(KNOB_TATTN_NT) & 3, [&](auto nt) { hipLaunchKernelGGL((temporal_attn_mfma_kernel<T, decltype(nt)::value>), grid, dim3(256), r.lds, stream, p, r.hpb); });
        else with_const<2, 3, 4>(ft, [&](auto f) { hipLaunchKernelGGL((temporal_attn_mfma_long_kernel<T, decltype(f)::value>), grid, dim3(256), r.lds, stream, p, r.hpb); });
        return im360_launch_status();
    }
    with_const<16, 32, 64>(p.F <= 16 ? 16 : (p.F <= 32 ? 32 : 64), [&](auto fmax) { launch_tattn_v<T, decltype(fmax)::value>(p, npix, stream); });
    return im360_launch_status();
}

// The windowed kernel's LDS: base rows, table, window rows, fp32 accumulator, per-frame weight sums
static size_t twin_lds(const TAttnParams& p, int L, int hpb) {
    const size_t G = (size_t)hpb * p.d, pitch = 3 * G + 8;
    return ((size_t)p.F * pitch + (size_t)L * 3 * G + 16 * pitch) * 2 + ((size_t)p.F * G + p.F) * sizeof(float);
}

template <typename T>
static int launch_tattn_windows(const TAttnParams& p, const TWinParams& w, hipStream_t stream) {
    // two workgroups per CU (80 of the 160 KiB) where the head group can be halved that far; one head's rows of a long clip need more
    const size_t want = 80 * 1024, most = 160 * 1024;
    int hpb = p.heads;
    while (hpb > 1 && (hpb % 2) == 0 && twin_lds(p, w.L, hpb) > want) hpb /= 2;
    const size_t lds = twin_lds(p, w.L, hpb);
    IM360_CHECK_ARG(lds <= most, "temporal_attn_windows_fwd: %zu bytes of LDS for %d head(s) of %d channels x %d frames exceed %zu", lds, hpb, p.d, p.F, most);
    static bool raised = false;                                         // (per instantiation) beyond the 64 KB a launch gets unasked
    if (lds > 64 * 1024 && !raised) {
        const hipError_t e = hipFuncSetAttribute((const void*)temporal_attn_windows_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
        if (e != hipSuccess) {
            im360_set_error("temporal_attn_windows_fwd: hipFuncSetAttribute(%zu bytes of LDS): %s", most, hipGetErrorString(e));
            return IM360_ERR_LAUNCH;
        }
        raised = true;
    }
    const long npix = p.total / ((long)p.F * p.heads);
    hipLaunchKernelGGL((temporal_attn_windows_kernel<T>), dim3((unsigned)npix, (unsigned)(p.heads / hpb)), dim3(256), lds, stream, p, w, hpb);
    return im360_launch_status();
}

}  // namespace im360

extern "C" __attribute__((visibility("default"))) int im360_temporal_attn_fwd(const void* q, const void* k, const void* v, void* out,
                                       int64_t B, int64_t F, int64_t P, int64_t heads, int64_t d,
                                       int64_t qkv_fs, int64_t qkv_ps, int64_t qkv_bs,
                                       int64_t o_fs, int64_t o_ps, int64_t o_bs,
                                       float scale, int dtype, void* stream) {
    using namespace im360;
    IM360_CHECK_ARG(q && k && v && out, "temporal_attn_fwd: null pointer");
    IM360_CHECK_ARG(B > 0 && F > 0 && P > 0 && heads > 0 && d > 0, "temporal_attn_fwd: empty problem");
    IM360_CHECK_ARG(F <= 64, "temporal_attn_fwd: %ld frames > 64 (reference PE max_len, prompt-dual.yaml:28)", (long)F);
    IM360_CHECK_ARG((d % 8) == 0, "temporal_attn_fwd: head dim %ld must be a multiple of 8", (long)d);
    IM360_CHECK_ARG((qkv_fs % 8) == 0 && (qkv_ps % 8) == 0 && (qkv_bs % 8) == 0 && (o_fs % 8) == 0 &&
                    (o_ps % 8) == 0 && (o_bs % 8) == 0, "temporal_attn_fwd: strides must be multiples of 8 elements");
    IM360_CHECK_ARG(((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                    ((uintptr_t)out % 16) == 0, "temporal_attn_fwd: misaligned base pointer");
    TAttnParams p;
    p.q = q; p.k = k; p.v = v; p.out = out;
    p.F = (int)F; p.P = (int)P; p.heads = (int)heads; p.d = (int)d;
    p.total = B * P * F * heads;
    p.q_fs = p.k_fs = p.v_fs = qkv_fs; p.q_ps = p.k_ps = p.v_ps = qkv_ps; p.q_bs = p.k_bs = p.v_bs = qkv_bs;
    p.o_fs = o_fs; p.o_ps = o_ps; p.o_bs = o_bs;
    p.scale_log2 = scale * 1.4426950408889634f;
    IM360_CHECK_ARG(F * 2 * d * 2 <= 48 * 1024, "temporal_attn_fwd: one head's K|V rows (%ld frames x %ld) exceed the LDS budget", (long)F, (long)d);
    ProfScope prof(PROF_TEMPORAL, stream);
    return with_dtype(dtype, "temporal_attn_fwd", [&](auto t) { return launch_tattn<typename decltype(t)::type>(p, (hipStream_t)stream); });
}

extern "C" __attribute__((visibility("default"))) int im360_temporal_attn_windows_fwd(const void* q, const void* k, const void* v, const void* pe_qkv, void* out,
                                       int64_t B, int64_t F, int64_t P, int64_t heads, int64_t d,
                                       int64_t qkv_fs, int64_t qkv_ps, int64_t qkv_bs,
                                       int64_t o_fs, int64_t o_ps, int64_t o_bs,
                                       const int32_t* starts, int64_t nW, const float* weights, int64_t L, int ring,
                                       float scale, int dtype, void* stream) {
    using namespace im360;
    IM360_CHECK_ARG(q && k && v && pe_qkv && out && starts && weights, "temporal_attn_windows_fwd: null pointer");
    IM360_CHECK_ARG(B > 0 && F > 0 && P > 0 && heads > 0 && d > 0, "temporal_attn_windows_fwd: empty problem");
    IM360_CHECK_ARG(F <= 64, "temporal_attn_windows_fwd: %ld frames > 64 (longer clips: whole-model context windows)", (long)F);
    IM360_CHECK_ARG(L >= 1 && L <= 16, "temporal_attn_windows_fwd: window length %ld outside 1 .. 16 (the 16 x 16 tile)", (long)L);
    IM360_CHECK_ARG(L <= F, "temporal_attn_windows_fwd: window length %ld > %ld frames", (long)L, (long)F);
    IM360_CHECK_ARG(nW >= 1 && nW <= 64, "temporal_attn_windows_fwd: %ld windows outside 1 .. 64", (long)nW);
    IM360_CHECK_ARG((d % 8) == 0, "temporal_attn_windows_fwd: head dim %ld must be a multiple of 8", (long)d);
    IM360_CHECK_ARG((qkv_fs % 8) == 0 && (qkv_ps % 8) == 0 && (qkv_bs % 8) == 0 && (o_fs % 8) == 0 &&
                    (o_ps % 8) == 0 && (o_bs % 8) == 0, "temporal_attn_windows_fwd: strides must be multiples of 8 elements");
    IM360_CHECK_ARG(((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)v % 16) == 0 && ((uintptr_t)pe_qkv % 16) == 0 &&
                    ((uintptr_t)out % 16) == 0, "temporal_attn_windows_fwd: misaligned base pointer");
    TWinParams w;
    w.pe = pe_qkv; w.nW = (int)nW; w.L = (int)L; w.ring = ring ? 1 : 0;
    int cover[64] = {0};
    for (int i = 0; i < 64; ++i) w.starts[i] = 0;
    for (int i = 0; i < 16; ++i) w.weights[i] = 0.f;
    for (int64_t i = 0; i < nW; ++i) {
        const int64_t s = starts[i];
        IM360_CHECK_ARG(s >= 0 && s < F, "temporal_attn_windows_fwd: window %ld starts at frame %ld, outside [0, %ld)", (long)i, (long)s, (long)F);
        IM360_CHECK_ARG(ring || s + L <= F, "temporal_attn_windows_fwd: window %ld (frames %ld .. %ld) runs past the end of a clip of %ld frames that is no ring",
                        (long)i, (long)s, (long)(s + L - 1), (long)F);
        w.starts[i] = (int)s;
        for (int64_t j = 0; j < L; ++j) ++cover[(s + j) % F];
    }
    for (int64_t j = 0; j < L; ++j) {
        IM360_CHECK_ARG(weights[j] > 0.f && weights[j] <= 3.0e38f, "temporal_attn_windows_fwd: weight %ld must be positive and finite", (long)j);
        w.weights[j] = weights[j];
    }
    for (int64_t f = 0; f < F; ++f) IM360_CHECK_ARG(cover[f] > 0, "temporal_attn_windows_fwd: frame %ld lies in no window", (long)f);
    TAttnParams p;
    p.q = q; p.k = k; p.v = v; p.out = out;
    p.F = (int)F; p.P = (int)P; p.heads = (int)heads; p.d = (int)d;
    p.total = B * P * F * heads;
    p.q_fs = p.k_fs = p.v_fs = qkv_fs; p.q_ps = p.k_ps = p.v_ps = qkv_ps; p.q_bs = p.k_bs = p.v_bs = qkv_bs;
    p.o_fs = o_fs; p.o_ps = o_ps; p.o_bs = o_bs;
    p.scale_log2 = scale * 1.4426950408889634f;
    ProfScope prof(PROF_TEMPORAL, stream);
    return with_dtype(dtype, "temporal_attn_windows_fwd", [&](auto t) { return launch_tattn_windows<typename decltype(t)::type>(p, w, (hipStream_t)stream); });
}
