// The sampler-step family on 16-bit latents, gfx950: classifier-free guidance fused with the scheduler update in one elementwise pass
// (cfg_ddim_kernel, cfg_ddim_step_kernel), the same step on the blend of temporal context windows on a line or a ring
// (cfg_ddim_step_windows_kernel), the statistics pass of the guidance rescale (cfg_rescale_*), and the DPM-Solver++ 2M update
// (arXiv 2211.01095, algorithm 2) on the same combine, blend, rescale and x0 conversion (cfg_multistep_step_kernel,
// cfg_multistep_step_windows_kernel), with its fp32 x0 history updated in place, and the statistics pass and the four guided steps of
// adaptive projected guidance (arXiv 2410.02416; cfg_apg_*, cfg_*_step*_apg_kernel).  Every step kernel has an unguided form
// (GUIDED = false; for cfg_ddim_kernel the kernel ddim_kernel) for a step outside the guidance interval (arXiv 2404.07724): the model
// ran the text half alone, the step takes that one prediction as m -- no second load stream, no guidance read, no combine -- and is
// otherwise the same code.
// Replaces: the guidance combine + scheduler.step of the denoising loop (pipeline_animation_inference_dual.py:791-800) with
// DDIMScheduler.step (diffusers/schedulers/scheduling_ddim.py:251-373; eta = 0, v-prediction: 300-350).  Context windows and the
// guidance rescale have no call site in the reference pipeline: they compose that same step (see their comments).
// Device code first; then the host side: two aggregates with their checks, the launchers, the entry points (fill, check, launch).
#include <cmath>
#include <initializer_list>

#include "common.h"

namespace im360 {

// ---- CFG combine + DDIM v-prediction update (eta = 0), one elementwise pass
//      (pipeline_animation_inference_dual.py:791-800; diffusers/schedulers/scheduling_ddim.py:300-350):
//      v = u + g (c - u);  x_prev = cx * x + cv * v   with cx, cv precomputed on the host in fp64
template <typename T>
__global__ void cfg_ddim_kernel(const T* __restrict__ uncond, const T* __restrict__ cond, const T* __restrict__ x,
                                T* __restrict__ out, long n8, float g, float cx, float cv, const float* __restrict__ coef) {
    if (coef != nullptr) {          // (guidance, cx, cv) read on the device: the launch can be replayed from a hipGraph
        g = coef[0];
        cx = coef[1];
        cv = coef[2];
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8];
        unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = cx * s[e] + cv * (u[e] + g * (c[e] - u[e]));
        ((uint4*)out)[i] = pack8<T>(s);
    }
}

// ---- the unguided form of cfg_ddim_kernel (a step outside the guidance interval: the model ran the text half alone): one prediction,
//      x_prev = cx * x + cv * pred; coef is cfg_ddim_kernel's (guidance, cx, cv), element 0 not read.  A kernel of its own and not a
//      template argument of the one above: that one is the default sampler's launch, it keeps its name (the rocprofv3 summaries under
//      profiles/ name it) and its text -- calling a shared body from it already changes which product hipcc contracts (-ffast-math),
//      i.e. the default path's bits.  The update is spelled as hipcc contracts the guided line -- cx * x rounded, then one fma with
//      the prediction -- because left to itself it fuses the other product in some lanes here, and u == c would then not give
//      cfg_ddim_kernel's bits (tests/test_guidance_interval_gpu.py holds the two to the same bits).
template <typename T>
__global__ void ddim_kernel(const T* __restrict__ pred, const T* __restrict__ x, T* __restrict__ out, long n8, float cx, float cv,
                            const float* __restrict__ coef) {
    if (coef != nullptr) {
        cx = coef[1];
        cv = coef[2];
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float c[8], s[8];
        unpack8<T>(((const uint4*)pred)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = __fmaf_rn(cv, c[e], cx * s[e]);
        ((uint4*)out)[i] = pack8<T>(s);
    }
}

// ---- CFG combine + the full DDIMScheduler.step (diffusers/schedulers/scheduling_ddim.py:251-373), one elementwise pass:
//      m = u + g (c - u);  x0 / e from the prediction type (mode bits 0-1: 0 epsilon, 1 v, 2 sample);  x0 clamped to [-1, 1]
//      (bit 2);  e re-derived from the clamped x0 (bit 3);  out = sa_prev x0 + dir e + sigma z.  sa, sb = sqrt(a_t), sqrt(1 - a_t);
//      dir = sqrt(1 - a_prev - sigma^2), sigma = eta sqrt(var) come from fp64 host math.  noise == nullptr: z = 0.
// The step arithmetic of one element, shared by cfg_ddim_step_kernel and cfg_ddim_step_windows_kernel: m is the guided model output,
// s the sample, z the variance noise (0 without one); isa = 1 / sa, isb = 1 / sb.
struct DdimCoefs {
    float g, sa, sb, sap, dir, sigma, isa, isb;
    int pred;
    bool clip, clipped_out;
};

template <bool GUIDED>
__device__ __forceinline__ DdimCoefs ddim_coefs(float g, float sa, float sb, float sap, float dir, float sigma, int mode,
                                                const float* __restrict__ coef) {
    if (coef != nullptr) {          // (guidance, sa, sb, sa_prev, dir, sigma) read on the device: hipGraph replay
        if (GUIDED) g = coef[0];     // (an unguided step never reads the guidance)
        sa = coef[1];
        sb = coef[2];
        sap = coef[3];
        dir = coef[4];
        sigma = coef[5];
    }
    DdimCoefs k;
    k.g = g, k.sa = sa, k.sb = sb, k.sap = sap, k.dir = dir, k.sigma = sigma;
    k.isa = 1.0f / sa, k.isb = 1.0f / sb;
    k.pred = mode & 3;
    k.clip = (mode & 4) != 0, k.clipped_out = (mode & 8) != 0;
    return k;
}

__device__ __forceinline__ float cfg_combine(float u, float c, float g) { return u + g * (c - u); }

__device__ __forceinline__ float ddim_step_elem(float m, float s, float z, const DdimCoefs& k) {
    float x0, eps;
    if (k.pred == 0) {
        x0 = (s - k.sb * m) * k.isa;
        eps = m;
    } else if (k.pred == 1) {
        x0 = k.sa * s - k.sb * m;
        eps = k.sa * m + k.sb * s;
    } else {
        x0 = m;
        eps = m;                     // the reference's direction term multiplies the model output, i.e. x0 itself
    }
    if (k.clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    if (k.clipped_out) eps = (s - k.sa * x0) * k.isb;
    return k.sap * x0 + k.dir * eps + k.sigma * z;
}

// The x0 of ddim_step_elem alone, for an update that needs no e: prediction type `pred` (mode bits 0-1), clamp with `clip` (mode bit 2),
// isa = 1 / sa.  ddim_step_elem keeps its own interleaved x0 / e branches: routing it through this function changes the code hipcc
// emits for the DDIM kernels (-ffast-math), and the default sampler has to give the bits it gave.
__device__ __forceinline__ float step_x0(float m, float s, int pred, bool clip, float sa, float sb, float isa) {
    float x0;
    if (pred == 0) x0 = (s - sb * m) * isa;
    else if (pred == 1) x0 = sa * s - sb * m;
    else x0 = m;
    if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    return x0;
}

// ---- the DPM-Solver++ 2M update (arXiv 2211.01095, algorithm 2; data prediction, multistep order <= 2) in its linear form
//          out = cx * x + c0 * x0 + c1 * x0_old,      hist <- x0
//      with x0 = step_x0 of the guided prediction (the three prediction types and the clamp of the DDIM step) and x0_old the x0 of
//      the step run before, kept in fp32 (never rounded to 16 bits: |c0|, |c1| reach 2.7 and 1.75 on the shipped grid).  cx, c0, c1
//      come from fp64 host math (DPMSolverMultistepScheduler.multistep_coefficients); a first-order step (the first and the last
//      one of a run, solver_order = 1) has c1 == 0 and then `hist` is NOT read: h is 0 and the term is left out, so whatever the
//      history holds -- NaN included -- cannot reach out.  sa, sb = sqrt(a_t), sqrt(1 - a_t) as in DdimCoefs.
struct MultistepCoefs {
    float g, sa, sb, cx, c0, c1, isa;
    int pred;
    bool clip, hist;                 // hist: c1 != 0, uniform over the launch
};

template <bool GUIDED>
__device__ __forceinline__ MultistepCoefs multistep_coefs(float g, float sa, float sb, float cx, float c0, float c1, int mode,
                                                          const float* __restrict__ coef) {
    if (coef != nullptr) {          // (guidance, sa, sb, cx, c0, c1) read on the device: hipGraph replay
        if (GUIDED) g = coef[0];
        sa = coef[1];
        sb = coef[2];
        cx = coef[3];
        c0 = coef[4];
        c1 = coef[5];
    }
    MultistepCoefs k;
    k.g = g, k.sa = sa, k.sb = sb, k.cx = cx, k.c0 = c0, k.c1 = c1;
    k.isa = 1.0f / sa;
    k.pred = mode & 3;
    k.clip = (mode & 4) != 0;
    k.hist = c1 != 0.0f;
    return k;
}

// One element: m the guided prediction, s the sample, h the old x0 (0 when !k.hist).  Returns out and leaves the new x0 in h.  The two
// value barriers keep m and x0 the values the caller / the history see: this file is built with -ffast-math, and what produced m (the
// blend's division, the rescale) must not be folded into the coefficients differently in the plain and in the windows kernel.
__device__ __forceinline__ float multistep_step_elem(float m, float s, float& h, const MultistepCoefs& k) {
    asm volatile("" : "+v"(m));
    float x0 = step_x0(m, s, k.pred, k.clip, k.sa, k.sb, k.isa);
    asm volatile("" : "+v"(x0));
    float o = __fmaf_rn(k.c0, x0, k.cx * s);
    if (k.hist) o = __fmaf_rn(k.c1, h, o);
    h = x0;
    return o;
}

// the fp32 history of the 8 elements of lane i: two float4
__device__ __forceinline__ void hist_load8(const float* __restrict__ hist, long i, float* h) {
    const float4 a = ((const float4*)hist)[2 * i], b = ((const float4*)hist)[2 * i + 1];
    h[0] = a.x, h[1] = a.y, h[2] = a.z, h[3] = a.w, h[4] = b.x, h[5] = b.y, h[6] = b.z, h[7] = b.w;
}

__device__ __forceinline__ void hist_store8(float* __restrict__ hist, long i, const float* h) {
    ((float4*)hist)[2 * i] = make_float4(h[0], h[1], h[2], h[3]);
    ((float4*)hist)[2 * i + 1] = make_float4(h[4], h[5], h[6], h[7]);
}

// ---- guidance rescale (arXiv 2305.08891, section 3.4): m' = r m with r = phi std(c) / std(m) + (1 - phi), the standard deviations
//      (correction 1) over the whole tensor.  Two launches: a statistics pass writes one record of partial moments per workgroup,
//      and every workgroup of the step kernel merges ALL records itself, in one fixed order, so that all of them multiply by the
//      same bits -- no atomics, no counter, no workgroup waits for another one, nothing read back by the host.
//      Moments are carried as (count, mean, M2 = sum (x - mean)^2) and merged with Chan's formula, never as sum x, sum x^2: the
//      variance of a prediction whose mean is far from zero would cancel in fp32.  c and m share the count.  Counts are fp32
//      (exact below 2^24 elements, 6e-8 relative above).
struct CfgMoments {
    float n, mc, qc, mm, qm;         // count;  mean, M2 of the text prediction c;  mean, M2 of the guided prediction m
};

constexpr int kRescaleMaxRecords = 256;      // grid cap of the statistics pass (about one workgroup per CU) = threads of a consumer
constexpr int kRescaleRecord = 8;            // floats per record (five used)

// a <- a (+) b, Chan et al.; an empty side leaves the other one untouched
__device__ __forceinline__ void moments_merge(CfgMoments& a, const CfgMoments& b) {
    if (b.n == 0.0f) return;
    if (a.n == 0.0f) {
        a = b;
        return;
    }
    const float n = a.n + b.n, f = b.n / n, w = a.n * f;
    const float dc = b.mc - a.mc, dm = b.mm - a.mm;
    a.mc = __fmaf_rn(dc, f, a.mc);
    a.qc = __fmaf_rn(dc * dc, w, a.qc + b.qc);
    a.mm = __fmaf_rn(dm, f, a.mm);
    a.qm = __fmaf_rn(dm * dm, w, a.qm + b.qm);
    a.n = n;
}

// a <- a (+) the cnt (1 .. 8) leading values of c[] / m[]: their own mean first, then the squared distances to it
__device__ __forceinline__ void moments_add(CfgMoments& a, const float* c, const float* m, int cnt) {
    float sc = 0.0f, sm = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (e < cnt) {
            sc += c[e];
            sm += m[e];
        }
    }
    CfgMoments b;
    b.n = (float)cnt;
    b.mc = sc / b.n, b.mm = sm / b.n;
    b.qc = 0.0f, b.qm = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (e < cnt) {
            const float dc = c[e] - b.mc, dm = m[e] - b.mm;
            b.qc = __fmaf_rn(dc, dc, b.qc);
            b.qm = __fmaf_rn(dm, dm, b.qm);
        }
    }
    moments_merge(a, b);
}

// The moments of a workgroup of exactly 256 threads (four waves; every kernel that calls this is launched so and carries
// __launch_bounds__(256)), valid in thread 0: lane l takes lane l + 1, + 2, ... + 32 of its wave (lane 0 ends with
// lanes 0 .. 63 in ascending order), then thread 0 takes the four waves in ascending order.  `lds`: 4 records.
__device__ __forceinline__ CfgMoments moments_block_reduce(CfgMoments a, CfgMoments* lds) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        CfgMoments b;
        b.n = __shfl_down(a.n, o), b.mc = __shfl_down(a.mc, o), b.qc = __shfl_down(a.qc, o);
        b.mm = __shfl_down(a.mm, o), b.qm = __shfl_down(a.qm, o);
        moments_merge(a, b);          // (lanes past 63 - o read their own value: never part of what lane 0 collects)
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = lds[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) moments_merge(a, lds[w]);
    }
    return a;
}

__device__ __forceinline__ void moments_store(float* __restrict__ ws, const CfgMoments& a) {
    float* rec = ws + (long)blockIdx.x * kRescaleRecord;
    rec[0] = a.n, rec[1] = a.mc, rec[2] = a.qc, rec[3] = a.mm, rec[4] = a.qm;
}

// r from the nrec records of a statistics pass, the same bits in every thread of every workgroup that calls it.  One record per
// thread: nrec <= kRescaleMaxRecords = 256 = blockDim.x (im360_cfg_rescale_records caps the statistics grid there).
__device__ __forceinline__ float rescale_factor(const float* ws, int nrec, float phi) {
    __shared__ CfgMoments lds[4];
    __shared__ float r_lds;
    CfgMoments a;
    a.n = a.mc = a.qc = a.mm = a.qm = 0.0f;
    if ((int)threadIdx.x < nrec) {
        const float* rec = ws + (long)threadIdx.x * kRescaleRecord;
        a.n = rec[0], a.mc = rec[1], a.qc = rec[2], a.mm = rec[3], a.qm = rec[4];
    }
    a = moments_block_reduce(a, lds);
    if (threadIdx.x == 0) {
        const float std_c = sqrtf(a.qc / (a.n - 1.0f)), std_m = sqrtf(a.qm / (a.n - 1.0f));
        r_lds = phi * std_c / std_m + (1.0f - phi);          // std_m = 0 or n = 1: inf / NaN, as the formula gives
    }
    __syncthreads();
    return r_lds;
}

// statistics pass over (u, c): n8 16-byte lanes, grid <= kRescaleMaxRecords, one record per workgroup
template <typename T>
__global__ __launch_bounds__(256) void cfg_rescale_stats_kernel(const T* __restrict__ uncond, const T* __restrict__ cond, long n8,
                                                                 float g, const float* __restrict__ coef, float* __restrict__ ws) {
    __shared__ CfgMoments lds[4];
    if (coef != nullptr) g = coef[0];
    CfgMoments a;
    a.n = a.mc = a.qc = a.mm = a.qm = 0.0f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], m[8];
        unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = cfg_combine(u[e], c[e], g);
        moments_add(a, c, m, 8);
    }
    a = moments_block_reduce(a, lds);
    if (threadIdx.x == 0) moments_store(ws, a);
}

// r alone, for tests and tools: one workgroup, the reduction every step workgroup makes
__global__ __launch_bounds__(256) void cfg_rescale_factor_kernel(const float* __restrict__ ws, int nrec, float phi, float* __restrict__ out) {
    const float r = rescale_factor(ws, nrec, phi);
    if (threadIdx.x == 0) out[0] = r;
}

// r * m as ONE fp32 multiplication of exactly these two values.  This file is built with -ffast-math: without the two value barriers
// hipcc folds r into the step's coefficients in one kernel and into the blend's division in another, and the windows kernel would
// no longer give the plain kernel's bits for one uniform window.
__device__ __forceinline__ float rescale_mul(float r, float m) {
    asm volatile("" : "+v"(m));
    float p = r * m;
    asm volatile("" : "+v"(p));
    return p;
}

// RS: the guided prediction is multiplied by rescale_factor(ws, nrec, phi) before the step; those instantiations need workgroups of
// 256 threads and say so in their launch bounds (1024 is the default, i.e. what the kernel without the factor always had).
// GUIDED = false (never with RS: the rescale of a prediction towards its own standard deviation is the identity): m = c, the one
// prediction of a step outside the guidance interval; `uncond` is not read (the entry points pass null) and neither is the guidance.
template <typename T, bool RS, bool GUIDED>
__global__ __launch_bounds__(RS ? 256 : 1024) void cfg_ddim_step_kernel(const T* __restrict__ uncond, const T* __restrict__ cond, const T* __restrict__ x,
                                     const T* __restrict__ noise, T* __restrict__ out, long n8, float g, float sa, float sb,
                                     float sap, float dir, float sigma, int mode, const float* __restrict__ coef,
                                     const float* __restrict__ ws, int nrec, float phi) {
    static_assert(GUIDED || !RS, "no rescaled unguided step");
    const DdimCoefs k = ddim_coefs<GUIDED>(g, sa, sb, sap, dir, sigma, mode, coef);
    float r = 1.0f;
    if (RS) r = rescale_factor(ws, nrec, phi);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8], z[8];
        if (GUIDED) unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
        if (noise != nullptr) unpack8<T>(((const uint4*)noise)[i], z);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float m = GUIDED ? cfg_combine(u[e], c[e], k.g) : c[e];
            s[e] = ddim_step_elem(RS ? rescale_mul(r, m) : m, s[e], z[e], k);
        }
        ((uint4*)out)[i] = pack8<T>(s);
    }
}

// ---- CFG combine + the multistep update above: the loop of cfg_ddim_step_kernel with the history stream.  hist: float[8 n8], read
//      (k.hist only) and written by the thread that owns the lane.  GUIDED: as in cfg_ddim_step_kernel.
template <typename T, bool RS, bool GUIDED>
__global__ __launch_bounds__(RS ? 256 : 1024) void cfg_multistep_step_kernel(const T* __restrict__ uncond, const T* __restrict__ cond, const T* __restrict__ x,
                                     float* __restrict__ hist, T* __restrict__ out, long n8, float g, float sa, float sb, float cx,
                                     float c0, float c1, int mode, const float* __restrict__ coef, const float* __restrict__ ws,
                                     int nrec, float phi) {
    static_assert(GUIDED || !RS, "no rescaled unguided step");
    const MultistepCoefs k = multistep_coefs<GUIDED>(g, sa, sb, cx, c0, c1, mode, coef);
    float r = 1.0f;
    if (RS) r = rescale_factor(ws, nrec, phi);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8], h[8];
        if (GUIDED) unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
        if (k.hist) hist_load8(hist, i, h);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float m = GUIDED ? cfg_combine(u[e], c[e], k.g) : c[e];
            s[e] = multistep_step_elem(RS ? rescale_mul(r, m) : m, s[e], h[e], k);
        }
        hist_store8(hist, i, h);
        ((uint4*)out)[i] = pack8<T>(s);
    }
}

// ---- the same step on the per-frame blend of sliding temporal context windows.  x / noise / out are [outer, F, inner]; the
//      predictions of all windows sit in one buffer pred[nW, 2, outer, L, inner] (window, CFG half, the model's own layout);
//      start[nW] ascending window start frames, weight[L] the blend weight of each position inside a window.  Per element at frame f:
//          m = (sum_k w[f - s_k] (u_k + g (c_k - u_k))) / (sum_k w[f - s_k])   over the windows with s_k <= f < s_k + L, k ascending
//      (a fixed summation order: deterministic), then ddim_step_elem; one rounding, at the store.  V = 8: 16-byte lanes (inner % 8
//      == 0, so a lane never straddles a frame); V = 1: the scalar path for any inner.  The first covering window initialises the
//      sums, so one window with weight 1 gives m = 1 * m_0 / 1 = m_0 exactly: bit-identical to cfg_ddim_step_kernel.
//      wrap = 0: the windows lie on a line (above).  wrap = F: they lie on a ring of F frames, window k covers the frames
//      (s_k + j) mod F, j = 0 .. L - 1, and a frame in front of s_k is at position f - s_k + F.  One integer compare-and-add per
//      window and lane; slot order and float arithmetic are those of the line.  j indexes pred / weight only when 0 <= j < L,
//      whatever the table holds.
// The blend of the V elements from element e0 on (V = 8: one 16-byte lane inside one frame): mb[] = the guided prediction m above;
// cb[] (CB only) = the same blend of the text half c_k alone, what the guidance rescale takes std(c) of.
// GUIDED = false: pred is [nW, 1, outer, L, inner], the text halves alone; mb[] is their blend -- one load per window, and nothing is
// read behind the last window's only half.
template <typename T, int V, bool CB, bool GUIDED = true>
__device__ __forceinline__ void windows_blend(const T* __restrict__ pred, const int* __restrict__ start, const float* __restrict__ weight,
                                              int nW, int F, int L, int wrap, long inner, long half, long e0, float g, float* mb, float* cb) {
    const long r = e0 % inner, of = e0 / inner;
    const int f = (int)(of % F);
    const long o = of / F;
    float acc[V], cacc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = cacc[e] = 0.0f;
    float wsum = 0.0f;
    bool first = true;
    for (int w = 0; w < nW; ++w) {
        int j = f - start[w];
        if (j < 0) j += wrap;
        if (j < 0 || j >= L) continue;
        const float wt = weight[j];
        const long at = (long)w * (GUIDED ? 2 : 1) * half + (o * L + j) * inner + r;
        float u[V], c[V];
        if (V == 8) {
            if (GUIDED) unpack8<T>(*(const uint4*)(pred + at), u);
            unpack8<T>(*(const uint4*)(pred + at + (GUIDED ? half : 0)), c);
        } else {
            if (GUIDED) u[0] = to_f32<T>(pred[at]);
            c[0] = to_f32<T>(pred[at + (GUIDED ? half : 0)]);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float m = wt * (GUIDED ? cfg_combine(u[e], c[e], g) : c[e]);
            acc[e] = first ? m : acc[e] + m;
            if (CB) {
                const float t = wt * c[e];
                cacc[e] = first ? t : cacc[e] + t;
            }
        }
        wsum = first ? wt : wsum + wt;
        first = false;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        mb[e] = acc[e] / wsum;
        if (CB) cb[e] = cacc[e] / wsum;
    }
}

// statistics pass of the guidance rescale over the blends (windows_blend: the step kernel's own m, and c blended the same way), the
// moments over the whole clip [outer, F, inner].  A thread takes the elements in the groups of 8 of cfg_rescale_stats_kernel for
// either V (V = 1: eight scalar blends, the last group may be short), so one uniform window with L = F writes that kernel's records.
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_rescale_stats_windows_kernel(const T* __restrict__ pred, const int* __restrict__ start,
                                                                         const float* __restrict__ weight, int nW, long outer, int F, int L,
                                                                         int wrap, long inner, float g, const float* __restrict__ coef,
                                                                         float* __restrict__ ws) {
    __shared__ CfgMoments lds[4];
    if (coef != nullptr) g = coef[0];
    const long n = outer * F * inner, n8 = (n + 7) / 8;
    const long half = outer * L * inner;
    CfgMoments a;
    a.n = a.mc = a.qc = a.mm = a.qm = 0.0f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float c[8], m[8];
        int cnt = 8;
        if (V == 8) windows_blend<T, 8, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * 8, g, m, c);
        else {
            cnt = (int)(n - i * 8 < 8 ? n - i * 8 : 8);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e < cnt) windows_blend<T, 1, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * 8 + e, g, &m[e], &c[e]);
        }
        moments_add(a, c, m, cnt);
    }
    a = moments_block_reduce(a, lds);
    if (threadIdx.x == 0) moments_store(ws, a);
}

template <typename T, int V, bool RS, bool GUIDED>
__global__ __launch_bounds__(RS ? 256 : 1024) void cfg_ddim_step_windows_kernel(const T* __restrict__ pred, const T* __restrict__ x, const T* __restrict__ noise,
                                             T* __restrict__ out, const int* __restrict__ start, const float* __restrict__ weight,
                                             int nW, long outer, int F, int L, int wrap, long inner, float g, float sa, float sb, float sap,
                                             float dir, float sigma, int mode, const float* __restrict__ coef,
                                             const float* __restrict__ ws, int nrec, float phi) {
    static_assert(GUIDED || !RS, "no rescaled unguided step");
    const DdimCoefs k = ddim_coefs<GUIDED>(g, sa, sb, sap, dir, sigma, mode, coef);
    float r = 1.0f;
    if (RS) r = rescale_factor(ws, nrec, phi);
    const long nv = outer * F * inner / V;
    const long half = outer * L * inner;              // one CFG half of one window
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        float m[V], s[V], z[V];
        windows_blend<T, V, false, GUIDED>(pred, start, weight, nW, F, L, wrap, inner, half, i * V, k.g, m, nullptr);
        if (V == 8) {
            unpack8<T>(((const uint4*)x)[i], s);
            if (noise != nullptr) unpack8<T>(((const uint4*)noise)[i], z);
        } else {
            s[0] = to_f32<T>(x[i]);
            if (noise != nullptr) z[0] = to_f32<T>(noise[i]);
        }
        if (noise == nullptr) {
#pragma unroll
            for (int e = 0; e < V; ++e) z[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = ddim_step_elem(RS ? rescale_mul(r, m[e]) : m[e], s[e], z[e], k);
        if (V == 8) ((uint4*)out)[i] = pack8<T>(s);
        else out[i] = from_f32<T>(s[0]);
    }
}

// the multistep update on the blend of the windows (windows_blend; wrap: line or ring), hist [outer, F, inner] like x
template <typename T, int V, bool RS, bool GUIDED>
__global__ __launch_bounds__(RS ? 256 : 1024) void cfg_multistep_step_windows_kernel(const T* __restrict__ pred, const T* __restrict__ x, float* __restrict__ hist,
                                             T* __restrict__ out, const int* __restrict__ start, const float* __restrict__ weight,
                                             int nW, long outer, int F, int L, int wrap, long inner, float g, float sa, float sb, float cx,
                                             float c0, float c1, int mode, const float* __restrict__ coef,
                                             const float* __restrict__ ws, int nrec, float phi) {
    static_assert(GUIDED || !RS, "no rescaled unguided step");
    const MultistepCoefs k = multistep_coefs<GUIDED>(g, sa, sb, cx, c0, c1, mode, coef);
    float r = 1.0f;
    if (RS) r = rescale_factor(ws, nrec, phi);
    const long nv = outer * F * inner / V;
    const long half = outer * L * inner;              // one CFG half of one window
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        float m[V], s[V], h[V];
        windows_blend<T, V, false, GUIDED>(pred, start, weight, nW, F, L, wrap, inner, half, i * V, k.g, m, nullptr);
        if (V == 8) unpack8<T>(((const uint4*)x)[i], s);
        else s[0] = to_f32<T>(x[i]);
        if (k.hist) {
            if (V == 8) hist_load8(hist, i, h);
            else h[0] = hist[i];
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) h[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = multistep_step_elem(RS ? rescale_mul(r, m[e]) : m[e], s[e], h[e], k);
        if (V == 8) {
            hist_store8(hist, i, h);
            ((uint4*)out)[i] = pack8<T>(s);
        } else {
            hist[i] = h[0];
            out[i] = from_f32<T>(s[0]);
        }
    }
}

// ---- adaptive projected guidance (APG, arXiv 2410.02416, algorithm 1; its momentum: the block behind these kernels): the guidance difference is split into the
//      part parallel to the text branch's denoised prediction and the rest, the parallel part is scaled by eta, and the difference may
//      be clamped to a radius.  The paper works on x0; mapped back to the model's output the x0 conversion's factor on the prediction
//      cancels and what the step takes in place of u + g (c - u) is
//          d = c - u,   q = c + rho x,   rho = -1 / sb (epsilon), -sa / sb (v), 0 (sample)            (q: the x0 of c over that factor)
//          alpha = sum d q / sum q^2,   s = min(1, r / (kp sqrt(sum d^2 / N))),   kp = sb / sa (epsilon), sb (v), 1 (sample)
//          m = c + (g - 1) s d - lambda q,   lambda = (g - 1) s (1 - eta) alpha
//      with the three sums over the whole tensor (the domain of the guidance rescale) and r an RMS in x0 units (+inf: no clamp).
//      Two launches like the guidance rescale and with its record size, grid cap and workspace: a statistics pass leaves one record
//      (count, sum d q, sum q^2, sum d^2) per workgroup, every workgroup of the step kernel merges all records in one fixed order.
//      The sums are plain fp32 sums of products (d and q are differences of like-sized values: nothing to centre), one fma chain per
//      thread, a shuffle tree per wave, the four waves in ascending order.  The step kernels are kernels of their own beside the RS
//      instantiations, not a further template argument of those: the mangled names of the shipped instantiations (the launch ledgers
//      and the profiles name them) and their code stay what they were.  There is no unguided form: there is no u.
struct ApgSums {
    float n, dq, qq, dd;
};
struct ApgScalars {
    float alpha, s, gs, lam;         // gs = (g - 1) s
};

// a + b as one fp32 addition of exactly these two values (-ffast-math may otherwise reassociate a chain differently per kernel)
__device__ __forceinline__ float add_kept(float a, float b) {
    float s = a + b;
    asm volatile("" : "+v"(s));
    return s;
}

__device__ __forceinline__ float apg_rho(int pred, float sa, float sb) {
    const float isb = 1.0f / sb;
    return pred == 0 ? -isb : pred == 1 ? -sa * isb : 0.0f;
}

// d and q of one element, the same bits in the statistics pass and in the step, in the plain and in the windows kernels: the value
// barriers keep a blend's division and rho out of the two operations
__device__ __forceinline__ void apg_dq(float u, float c, float x, float rho, float& d, float& q) {
    asm volatile("" : "+v"(u), "+v"(c));
    d = c - u;
    q = __fmaf_rn(rho, x, c);
    asm volatile("" : "+v"(d), "+v"(q));
}

// a <- a + the cnt (1 .. 8) leading elements, in ascending order
__device__ __forceinline__ void apg_add(ApgSums& a, const float* u, const float* c, const float* x, int cnt, float rho) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (e < cnt) {
            float d, q;
            apg_dq(u[e], c[e], x[e], rho, d, q);
            a.dq = __fmaf_rn(d, q, a.dq);
            a.qq = __fmaf_rn(q, q, a.qq);
            a.dd = __fmaf_rn(d, d, a.dd);
        }
    }
    a.n += (float)cnt;
}

// The sums of a workgroup of exactly 256 threads, valid in thread 0; order and `lds` (4 records) as in moments_block_reduce
__device__ __forceinline__ ApgSums apg_block_reduce(ApgSums a, ApgSums* lds) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        a.n = add_kept(a.n, __shfl_down(a.n, o));
        a.dq = add_kept(a.dq, __shfl_down(a.dq, o));
        a.qq = add_kept(a.qq, __shfl_down(a.qq, o));
        a.dd = add_kept(a.dd, __shfl_down(a.dd, o));
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = lds[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            a.n = add_kept(a.n, lds[w].n), a.dq = add_kept(a.dq, lds[w].dq);
            a.qq = add_kept(a.qq, lds[w].qq), a.dd = add_kept(a.dd, lds[w].dd);
        }
    }
    return a;
}

__device__ __forceinline__ void apg_store(float* __restrict__ ws, const ApgSums& a) {
    float* rec = ws + (long)blockIdx.x * kRescaleRecord;
    rec[0] = a.n, rec[1] = a.dq, rec[2] = a.qq, rec[3] = a.dd;
}

// (alpha, s, (g - 1) s, lambda) from the nrec records of a statistics pass, the same bits in every thread of every workgroup that
// calls it.  One record per thread: nrec <= kRescaleMaxRecords = 256 = blockDim.x.  sum q^2 = 0: alpha = NaN, as the formula gives;
// sum d^2 = 0 (u == c): s = 1 and lambda = 0, i.e. m = c.
__device__ __forceinline__ ApgScalars apg_scalars(const float* ws, int nrec, float g, float sa, float sb, int pred, float eta, float r) {
    __shared__ ApgSums lds[4];
    __shared__ ApgScalars k_lds;
    ApgSums a;
    a.n = a.dq = a.qq = a.dd = 0.0f;
    if ((int)threadIdx.x < nrec) {
        const float* rec = ws + (long)threadIdx.x * kRescaleRecord;
        a.n = rec[0], a.dq = rec[1], a.qq = rec[2], a.dd = rec[3];
    }
    a = apg_block_reduce(a, lds);
    if (threadIdx.x == 0) {
        const float kp = pred == 0 ? sb / sa : pred == 1 ? sb : 1.0f;
        ApgScalars k;
        k.alpha = a.dq / a.qq;
        k.s = r < __builtin_inff() ? fminf(1.0f, r / (kp * sqrtf(a.dd / a.n))) : 1.0f;
        k.gs = (g - 1.0f) * k.s;
        k.lam = k.gs * (1.0f - eta) * k.alpha;
        k_lds = k;
    }
    __syncthreads();
    return k_lds;
}

// m of one element: two products and two additions of exactly these values (rescale_mul's pattern)
__device__ __forceinline__ float apg_combine(float u, float c, float x, float rho, const ApgScalars& a) {
    float d, q;
    apg_dq(u, c, x, rho, d, q);
    float p = a.gs * d;
    asm volatile("" : "+v"(p));
    float t = a.lam * q;
    asm volatile("" : "+v"(t));
    return add_kept(add_kept(c, p), -t);
}

// statistics pass over (u, c, x): n8 16-byte lanes, grid <= kRescaleMaxRecords, one record per workgroup
template <typename T>
__global__ __launch_bounds__(256) void cfg_apg_stats_kernel(const T* __restrict__ uncond, const T* __restrict__ cond, const T* __restrict__ x,
                                                             long n8, float sa, float sb, int mode, const float* __restrict__ coef,
                                                             float* __restrict__ ws) {
    __shared__ ApgSums lds[4];
    if (coef != nullptr) sa = coef[1], sb = coef[2];
    const float rho = apg_rho(mode & 3, sa, sb);
    ApgSums a;
    a.n = a.dq = a.qq = a.dd = 0.0f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8];
        unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
        apg_add(a, u, c, s, 8, rho);
    }
    a = apg_block_reduce(a, lds);
    if (threadIdx.x == 0) apg_store(ws, a);
}

// The same over the blends of the windows: u and c are windows_blend's blends of the two halves (guidance 0 makes its combined
// prediction u + 0 (c - u) = u), x is [outer, F, inner].  Groups of 8 for either V as in cfg_rescale_stats_windows_kernel, so one
// uniform window with L = F writes cfg_apg_stats_kernel's records.
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_apg_stats_windows_kernel(const T* __restrict__ pred, const T* __restrict__ x,
                                                                     const int* __restrict__ start, const float* __restrict__ weight, int nW,
                                                                     long outer, int F, int L, int wrap, long inner, float sa, float sb, int mode,
                                                                     const float* __restrict__ coef, float* __restrict__ ws) {
    __shared__ ApgSums lds[4];
    if (coef != nullptr) sa = coef[1], sb = coef[2];
    const float rho = apg_rho(mode & 3, sa, sb);
    const long n = outer * F * inner, n8 = (n + 7) / 8;
    const long half = outer * L * inner;
    ApgSums a;
    a.n = a.dq = a.qq = a.dd = 0.0f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8];
        int cnt = 8;
        if (V == 8) {
            windows_blend<T, 8, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * 8, 0.0f, u, c);
            unpack8<T>(((const uint4*)x)[i], s);
        } else {
            cnt = (int)(n - i * 8 < 8 ? n - i * 8 : 8);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e < cnt) {
                    windows_blend<T, 1, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * 8 + e, 0.0f, &u[e], &c[e]);
                    s[e] = to_f32<T>(x[i * 8 + e]);
                }
        }
        apg_add(a, u, c, s, cnt, rho);
    }
    a = apg_block_reduce(a, lds);
    if (threadIdx.x == 0) apg_store(ws, a);
}

// (alpha, s, lambda) alone, for tests and tools: one workgroup, the reduction every step workgroup makes
__global__ __launch_bounds__(256) void cfg_apg_scalars_kernel(const float* __restrict__ ws, int nrec, float g, float sa, float sb, int mode,
                                                               float eta, float r, const float* __restrict__ coef, float* __restrict__ out) {
    if (coef != nullptr) g = coef[0], sa = coef[1], sb = coef[2];
    const ApgScalars k = apg_scalars(ws, nrec, g, sa, sb, mode & 3, eta, r);
    if (threadIdx.x == 0) out[0] = k.alpha, out[1] = k.s, out[2] = k.lam;
}

// cfg_ddim_step_kernel on the projected guidance m above instead of u + g (c - u)
template <typename T>
__global__ __launch_bounds__(256) void cfg_ddim_step_apg_kernel(const T* __restrict__ uncond, const T* __restrict__ cond, const T* __restrict__ x,
                                     const T* __restrict__ noise, T* __restrict__ out, long n8, float g, float sa, float sb,
                                     float sap, float dir, float sigma, int mode, const float* __restrict__ coef,
                                     const float* __restrict__ ws, int nrec, float eta, float r) {
    const DdimCoefs k = ddim_coefs<true>(g, sa, sb, sap, dir, sigma, mode, coef);
    const ApgScalars a = apg_scalars(ws, nrec, k.g, k.sa, k.sb, k.pred, eta, r);
    const float rho = apg_rho(k.pred, k.sa, k.sb);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8], z[8];
        unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
        if (noise != nullptr) unpack8<T>(((const uint4*)noise)[i], z);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = ddim_step_elem(apg_combine(u[e], c[e], s[e], rho, a), s[e], z[e], k);
        ((uint4*)out)[i] = pack8<T>(s);
    }
}

// cfg_multistep_step_kernel on the projected guidance
template <typename T>
__global__ __launch_bounds__(256) void cfg_multistep_step_apg_kernel(const T* __restrict__ uncond, const T* __restrict__ cond, const T* __restrict__ x,
                                     float* __restrict__ hist, T* __restrict__ out, long n8, float g, float sa, float sb, float cx,
                                     float c0, float c1, int mode, const float* __restrict__ coef, const float* __restrict__ ws,
                                     int nrec, float eta, float r) {
    const MultistepCoefs k = multistep_coefs<true>(g, sa, sb, cx, c0, c1, mode, coef);
    const ApgScalars a = apg_scalars(ws, nrec, k.g, k.sa, k.sb, k.pred, eta, r);
    const float rho = apg_rho(k.pred, k.sa, k.sb);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8], h[8];
        unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
        if (k.hist) hist_load8(hist, i, h);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = multistep_step_elem(apg_combine(u[e], c[e], s[e], rho, a), s[e], h[e], k);
        hist_store8(hist, i, h);
        ((uint4*)out)[i] = pack8<T>(s);
    }
}

// cfg_ddim_step_windows_kernel on the projected guidance of the blends (u, c: as in cfg_apg_stats_windows_kernel)
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_ddim_step_windows_apg_kernel(const T* __restrict__ pred, const T* __restrict__ x, const T* __restrict__ noise,
                                             T* __restrict__ out, const int* __restrict__ start, const float* __restrict__ weight,
                                             int nW, long outer, int F, int L, int wrap, long inner, float g, float sa, float sb, float sap,
                                             float dir, float sigma, int mode, const float* __restrict__ coef,
                                             const float* __restrict__ ws, int nrec, float eta, float r) {
    const DdimCoefs k = ddim_coefs<true>(g, sa, sb, sap, dir, sigma, mode, coef);
    const ApgScalars a = apg_scalars(ws, nrec, k.g, k.sa, k.sb, k.pred, eta, r);
    const float rho = apg_rho(k.pred, k.sa, k.sb);
    const long nv = outer * F * inner / V;
    const long half = outer * L * inner;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        float u[V], c[V], s[V], z[V];
        windows_blend<T, V, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * V, 0.0f, u, c);
        if (V == 8) {
            unpack8<T>(((const uint4*)x)[i], s);
            if (noise != nullptr) unpack8<T>(((const uint4*)noise)[i], z);
        } else {
            s[0] = to_f32<T>(x[i]);
            if (noise != nullptr) z[0] = to_f32<T>(noise[i]);
        }
        if (noise == nullptr) {
#pragma unroll
            for (int e = 0; e < V; ++e) z[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = ddim_step_elem(apg_combine(u[e], c[e], s[e], rho, a), s[e], z[e], k);
        if (V == 8) ((uint4*)out)[i] = pack8<T>(s);
        else out[i] = from_f32<T>(s[0]);
    }
}

// cfg_multistep_step_windows_kernel on the projected guidance of the blends
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_multistep_step_windows_apg_kernel(const T* __restrict__ pred, const T* __restrict__ x, float* __restrict__ hist,
                                             T* __restrict__ out, const int* __restrict__ start, const float* __restrict__ weight,
                                             int nW, long outer, int F, int L, int wrap, long inner, float g, float sa, float sb, float cx,
                                             float c0, float c1, int mode, const float* __restrict__ coef,
                                             const float* __restrict__ ws, int nrec, float eta, float r) {
    const MultistepCoefs k = multistep_coefs<true>(g, sa, sb, cx, c0, c1, mode, coef);
    const ApgScalars a = apg_scalars(ws, nrec, k.g, k.sa, k.sb, k.pred, eta, r);
    const float rho = apg_rho(k.pred, k.sa, k.sb);
    const long nv = outer * F * inner / V;
    const long half = outer * L * inner;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        float u[V], c[V], s[V], h[V];
        windows_blend<T, V, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * V, 0.0f, u, c);
        if (V == 8) unpack8<T>(((const uint4*)x)[i], s);
        else s[0] = to_f32<T>(x[i]);
        if (k.hist) {
            if (V == 8) hist_load8(hist, i, h);
            else h[0] = hist[i];
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) h[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = multistep_step_elem(apg_combine(u[e], c[e], s[e], rho, a), s[e], h[e], k);
        if (V == 8) {
            hist_store8(hist, i, h);
            ((uint4*)out)[i] = pack8<T>(s);
        } else {
            hist[i] = h[0];
            out[i] = from_f32<T>(s[0]);
        }
    }
}

// ---- APG with the paper's momentum (algorithm 1 in full): the guidance difference the projection and the clamp see is the running
//      average of the run's guided steps, Dbar_t = Delta_t + beta Dbar_prev in x0 units.  The state is kept in the model-output units of
//      the step that wrote it, e_t = Dbar_t / kp_t, so that the update is one fma and everything above holds with d replaced by e:
//          e = d + carry e_prev,   carry = beta kp_prev / kp_t                         (0 on the first guided step of a run)
//          alpha = sum e q / sum q^2,   s = min(1, r / (kp sqrt(sum e^2 / N))),   m = c + (g - 1) s e - lambda q
//      `state`: float[n] indexed like the multistep history (the flat element index of the latent; windows: of the clip of blends),
//      each element read and written by the thread that owns it, 16-byte lanes of 8 as hist_load8 / hist_store8.  The statistics pass
//      reads it, the step reads it again, recomputes e with the same bits and stores the UNclamped e in place.  carry == 0 (uniform
//      over the launch, like k.hist): the state is NOT read, only written, and e = d to the bit -- the records, the scalars and the
//      step are those of the kernels above, and whatever the buffer held (NaN included) cannot leak.  carry is read from carry_dev[0]
//      where that is given (hipGraph replay: it changes per step).  Kernels of their own beside the ones above, sharing their device
//      functions: the shipped instantiations keep their names and their code.
__device__ __forceinline__ float apg_carry(float carry, const float* __restrict__ carry_dev) {
    return carry_dev != nullptr ? carry_dev[0] : carry;
}

// e and q of one element, the same bits in the statistics pass and in the step: apg_dq's d, then one fma of exactly these values
__device__ __forceinline__ void apg_eq(float u, float c, float x, float rho, bool mom, float carry, float ep, float& e, float& q) {
    apg_dq(u, c, x, rho, e, q);
    if (mom) {
        asm volatile("" : "+v"(ep));
        e = __fmaf_rn(carry, ep, e);
        asm volatile("" : "+v"(e));
    }
}

// apg_add on e: a <- a + the cnt (1 .. 8) leading elements, in ascending order; ep[] is read with `mom` only
__device__ __forceinline__ void apg_add_e(ApgSums& a, const float* u, const float* c, const float* x, const float* ep, int cnt, float rho,
                                          bool mom, float carry) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < cnt) {
            float e, q;
            apg_eq(u[i], c[i], x[i], rho, mom, carry, mom ? ep[i] : 0.0f, e, q);
            a.dq = __fmaf_rn(e, q, a.dq);
            a.qq = __fmaf_rn(q, q, a.qq);
            a.dd = __fmaf_rn(e, e, a.dd);
        }
    }
    a.n += (float)cnt;
}

// apg_combine on e; `e` is what the state receives
__device__ __forceinline__ float apg_combine_e(float u, float c, float x, float rho, const ApgScalars& a, bool mom, float carry, float ep,
                                               float& e) {
    float q;
    apg_eq(u, c, x, rho, mom, carry, ep, e, q);
    float p = a.gs * e;
    asm volatile("" : "+v"(p));
    float t = a.lam * q;
    asm volatile("" : "+v"(t));
    return add_kept(add_kept(c, p), -t);
}

// cfg_apg_stats_kernel with the state: reads state when carry != 0, never writes it
template <typename T>
__global__ __launch_bounds__(256) void cfg_apg_momentum_stats_kernel(const T* __restrict__ uncond, const T* __restrict__ cond,
                                                                      const T* __restrict__ x, const float* __restrict__ state, long n8,
                                                                      float sa, float sb, int mode, float carry,
                                                                      const float* __restrict__ carry_dev, const float* __restrict__ coef,
                                                                      float* __restrict__ ws) {
    __shared__ ApgSums lds[4];
    if (coef != nullptr) sa = coef[1], sb = coef[2];
    carry = apg_carry(carry, carry_dev);
    const bool mom = carry != 0.0f;
    const float rho = apg_rho(mode & 3, sa, sb);
    ApgSums a;
    a.n = a.dq = a.qq = a.dd = 0.0f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8], ep[8];
        unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
        if (mom) hist_load8(state, i, ep);
        apg_add_e(a, u, c, s, ep, 8, rho, mom, carry);
    }
    a = apg_block_reduce(a, lds);
    if (threadIdx.x == 0) apg_store(ws, a);
}

// cfg_apg_stats_windows_kernel with the state [outer, F, inner] (groups of 8 for either V; V = 1 reads the state by element)
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_apg_momentum_stats_windows_kernel(const T* __restrict__ pred, const T* __restrict__ x,
                                                                              const float* __restrict__ state, const int* __restrict__ start,
                                                                              const float* __restrict__ weight, int nW, long outer, int F,
                                                                              int L, int wrap, long inner, float sa, float sb, int mode,
                                                                              float carry, const float* __restrict__ carry_dev,
                                                                              const float* __restrict__ coef, float* __restrict__ ws) {
    __shared__ ApgSums lds[4];
    if (coef != nullptr) sa = coef[1], sb = coef[2];
    carry = apg_carry(carry, carry_dev);
    const bool mom = carry != 0.0f;
    const float rho = apg_rho(mode & 3, sa, sb);
    const long n = outer * F * inner, n8 = (n + 7) / 8;
    const long half = outer * L * inner;
    ApgSums a;
    a.n = a.dq = a.qq = a.dd = 0.0f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8], ep[8];
        int cnt = 8;
        if (V == 8) {
            windows_blend<T, 8, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * 8, 0.0f, u, c);
            unpack8<T>(((const uint4*)x)[i], s);
            if (mom) hist_load8(state, i, ep);
        } else {
            cnt = (int)(n - i * 8 < 8 ? n - i * 8 : 8);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e < cnt) {
                    windows_blend<T, 1, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * 8 + e, 0.0f, &u[e], &c[e]);
                    s[e] = to_f32<T>(x[i * 8 + e]);
                    if (mom) ep[e] = state[i * 8 + e];
                }
        }
        apg_add_e(a, u, c, s, ep, cnt, rho, mom, carry);
    }
    a = apg_block_reduce(a, lds);
    if (threadIdx.x == 0) apg_store(ws, a);
}

// cfg_ddim_step_apg_kernel on e, state <- e
template <typename T>
__global__ __launch_bounds__(256) void cfg_ddim_step_apg_momentum_kernel(const T* __restrict__ uncond, const T* __restrict__ cond,
                                     const T* __restrict__ x, const T* __restrict__ noise, float* __restrict__ state, T* __restrict__ out,
                                     long n8, float g, float sa, float sb, float sap, float dir, float sigma, int mode,
                                     const float* __restrict__ coef, const float* __restrict__ ws, int nrec, float eta, float r, float carry,
                                     const float* __restrict__ carry_dev) {
    const DdimCoefs k = ddim_coefs<true>(g, sa, sb, sap, dir, sigma, mode, coef);
    const ApgScalars a = apg_scalars(ws, nrec, k.g, k.sa, k.sb, k.pred, eta, r);
    const float rho = apg_rho(k.pred, k.sa, k.sb);
    carry = apg_carry(carry, carry_dev);
    const bool mom = carry != 0.0f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8], z[8], ep[8];
        unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
        if (noise != nullptr) unpack8<T>(((const uint4*)noise)[i], z);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = 0.0f;
        }
        if (mom) hist_load8(state, i, ep);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) ep[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = ddim_step_elem(apg_combine_e(u[e], c[e], s[e], rho, a, mom, carry, ep[e], ep[e]), s[e], z[e], k);
        hist_store8(state, i, ep);
        ((uint4*)out)[i] = pack8<T>(s);
    }
}

// cfg_multistep_step_apg_kernel on e, state <- e
template <typename T>
__global__ __launch_bounds__(256) void cfg_multistep_step_apg_momentum_kernel(const T* __restrict__ uncond, const T* __restrict__ cond,
                                     const T* __restrict__ x, float* __restrict__ hist, float* __restrict__ state, T* __restrict__ out, long n8,
                                     float g, float sa, float sb, float cx, float c0, float c1, int mode, const float* __restrict__ coef,
                                     const float* __restrict__ ws, int nrec, float eta, float r, float carry,
                                     const float* __restrict__ carry_dev) {
    const MultistepCoefs k = multistep_coefs<true>(g, sa, sb, cx, c0, c1, mode, coef);
    const ApgScalars a = apg_scalars(ws, nrec, k.g, k.sa, k.sb, k.pred, eta, r);
    const float rho = apg_rho(k.pred, k.sa, k.sb);
    carry = apg_carry(carry, carry_dev);
    const bool mom = carry != 0.0f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        float u[8], c[8], s[8], h[8], ep[8];
        unpack8<T>(((const uint4*)uncond)[i], u);
        unpack8<T>(((const uint4*)cond)[i], c);
        unpack8<T>(((const uint4*)x)[i], s);
        if (k.hist) hist_load8(hist, i, h);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = 0.0f;
        }
        if (mom) hist_load8(state, i, ep);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) ep[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = multistep_step_elem(apg_combine_e(u[e], c[e], s[e], rho, a, mom, carry, ep[e], ep[e]), s[e], h[e], k);
        hist_store8(hist, i, h);
        hist_store8(state, i, ep);
        ((uint4*)out)[i] = pack8<T>(s);
    }
}

// cfg_ddim_step_windows_apg_kernel on e, state [outer, F, inner] <- e
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_ddim_step_windows_apg_momentum_kernel(const T* __restrict__ pred, const T* __restrict__ x,
                                             const T* __restrict__ noise, float* __restrict__ state, T* __restrict__ out,
                                             const int* __restrict__ start, const float* __restrict__ weight, int nW, long outer, int F, int L,
                                             int wrap, long inner, float g, float sa, float sb, float sap, float dir, float sigma, int mode,
                                             const float* __restrict__ coef, const float* __restrict__ ws, int nrec, float eta, float r,
                                             float carry, const float* __restrict__ carry_dev) {
    const DdimCoefs k = ddim_coefs<true>(g, sa, sb, sap, dir, sigma, mode, coef);
    const ApgScalars a = apg_scalars(ws, nrec, k.g, k.sa, k.sb, k.pred, eta, r);
    const float rho = apg_rho(k.pred, k.sa, k.sb);
    carry = apg_carry(carry, carry_dev);
    const bool mom = carry != 0.0f;
    const long nv = outer * F * inner / V;
    const long half = outer * L * inner;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        float u[V], c[V], s[V], z[V], ep[V];
        windows_blend<T, V, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * V, 0.0f, u, c);
        if (V == 8) {
            unpack8<T>(((const uint4*)x)[i], s);
            if (noise != nullptr) unpack8<T>(((const uint4*)noise)[i], z);
        } else {
            s[0] = to_f32<T>(x[i]);
            if (noise != nullptr) z[0] = to_f32<T>(noise[i]);
        }
        if (noise == nullptr) {
#pragma unroll
            for (int e = 0; e < V; ++e) z[e] = 0.0f;
        }
        if (mom) {
            if (V == 8) hist_load8(state, i, ep);
            else ep[0] = state[i];
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) ep[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = ddim_step_elem(apg_combine_e(u[e], c[e], s[e], rho, a, mom, carry, ep[e], ep[e]), s[e], z[e], k);
        if (V == 8) {
            hist_store8(state, i, ep);
            ((uint4*)out)[i] = pack8<T>(s);
        } else {
            state[i] = ep[0];
            out[i] = from_f32<T>(s[0]);
        }
    }
}

// cfg_multistep_step_windows_apg_kernel on e, state [outer, F, inner] <- e
template <typename T, int V>
__global__ __launch_bounds__(256) void cfg_multistep_step_windows_apg_momentum_kernel(const T* __restrict__ pred, const T* __restrict__ x,
                                             float* __restrict__ hist, float* __restrict__ state, T* __restrict__ out,
                                             const int* __restrict__ start, const float* __restrict__ weight, int nW, long outer, int F, int L,
                                             int wrap, long inner, float g, float sa, float sb, float cx, float c0, float c1, int mode,
                                             const float* __restrict__ coef, const float* __restrict__ ws, int nrec, float eta, float r,
                                             float carry, const float* __restrict__ carry_dev) {
    const MultistepCoefs k = multistep_coefs<true>(g, sa, sb, cx, c0, c1, mode, coef);
    const ApgScalars a = apg_scalars(ws, nrec, k.g, k.sa, k.sb, k.pred, eta, r);
    const float rho = apg_rho(k.pred, k.sa, k.sb);
    carry = apg_carry(carry, carry_dev);
    const bool mom = carry != 0.0f;
    const long nv = outer * F * inner / V;
    const long half = outer * L * inner;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
        float u[V], c[V], s[V], h[V], ep[V];
        windows_blend<T, V, true>(pred, start, weight, nW, F, L, wrap, inner, half, i * V, 0.0f, u, c);
        if (V == 8) unpack8<T>(((const uint4*)x)[i], s);
        else s[0] = to_f32<T>(x[i]);
        if (k.hist) {
            if (V == 8) hist_load8(hist, i, h);
            else h[0] = hist[i];
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) h[e] = 0.0f;
        }
        if (mom) {
            if (V == 8) hist_load8(state, i, ep);
            else ep[0] = state[i];
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) ep[e] = 0.0f;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = multistep_step_elem(apg_combine_e(u[e], c[e], s[e], rho, a, mom, carry, ep[e], ep[e]), s[e], h[e], k);
        if (V == 8) {
            hist_store8(hist, i, h);
            hist_store8(state, i, ep);
            ((uint4*)out)[i] = pack8<T>(s);
        } else {
            hist[i] = h[0];
            state[i] = ep[0];
            out[i] = from_f32<T>(s[0]);
        }
    }
}

}  // namespace im360

// Records a statistics pass of the guidance rescale writes for n elements = its grid: one workgroup per 256 groups of 8 elements,
// at most kRescaleMaxRecords (every consumer thread reads one record).
extern "C" __attribute__((visibility("default"))) int64_t im360_cfg_rescale_records(int64_t n) {
    const int64_t blocks = ((n + 7) / 8 + 255) / 256;
    return blocks < 1 ? 1 : blocks > im360::kRescaleMaxRecords ? im360::kRescaleMaxRecords : blocks;
}

namespace im360 {
// What a step entry point is given besides its tensors: the coefficients (the kernel reads coef_dev[0 .. 5] instead when that is given),
// the mode bits, the variance noise (may be null) and, with the guidance rescale, the workspace of records and the strength phi.
struct StepArgs {
    float g, sa, sb, sap, dir, sigma;
    int mode;
    const void *noise, *coef_dev, *ws;
    int64_t ws_floats;
    float phi;
};
// The predictions of sliding context windows (layout, tables: cfg_ddim_step_windows_kernel); wrap = 0: on a line, wrap = F: on a ring.
struct Windows {
    const void *pred, *start, *weight;
    int nW, wrap;
    int64_t outer, F, L, inner;
    int64_t elements() const { return outer * F * inner; }
};
// n elements in the tensors `must` (none null) and `may` (null allowed), read and written 16 bytes at a time
static int check_tensors(const char* name, std::initializer_list<const void*> must, const void* may, int64_t n) {
    bool all = true;
    uintptr_t bits = (uintptr_t)may;
    for (const void* p : must) all = all && p, bits |= (uintptr_t)p;
    IM360_CHECK_ARG(all, "%s: null pointer", name);
    IM360_CHECK_ARG(n > 0 && (n % 8) == 0, "%s: n=%ld must be a positive multiple of 8", name, (long)n);
    IM360_CHECK_ARG((bits % 16) == 0, "%s: misaligned pointer", name);
    return IM360_OK;
}
// the workspace of n elements: present, 4-byte aligned, large enough for the grid
static int check_rescale_ws(const char* name, const void* ws, int64_t ws_floats, int64_t n) {
    IM360_CHECK_ARG(ws && ((uintptr_t)ws % 4) == 0, "%s: null or misaligned workspace", name);
    IM360_CHECK_ARG(ws_floats >= im360_cfg_rescale_records(n) * kRescaleRecord, "%s: workspace of %ld floats, %ld needed", name,
                    (long)ws_floats, (long)(im360_cfg_rescale_records(n) * kRescaleRecord));
    return IM360_OK;
}
// StepArgs: mode and noise, which every step entry point checks in the middle of its list ...
static int check_step(const char* name, const StepArgs& s) {
    IM360_CHECK_ARG(s.mode >= 0 && s.mode < 16 && (s.mode & 3) != 3, "%s: mode %d unsupported", name, s.mode);
    IM360_CHECK_ARG(s.noise || s.coef_dev || s.sigma == 0.0f, "%s: sigma=%g needs a noise tensor", name, (double)s.sigma);
    return IM360_OK;
}
// ... and phi and the workspace for n elements, which the _rescale entry points check at the end of theirs
static int check_step_rescale(const char* name, const StepArgs& s, int64_t n) {
    IM360_CHECK_ARG(std::isfinite(s.phi), "%s: rescale=%g must be finite", name, (double)s.phi);
    return check_rescale_ws(name, s.ws, s.ws_floats, n);
}
// Windows; `others`: the entry point's other mandatory pointers are there; `step` (null for a statistics pass) is checked in between.
static int check_windows(const char* name, const Windows& w, bool others, const StepArgs* step) {
    IM360_CHECK_ARG(w.pred && others && w.start && w.weight, "%s: null pointer", name);
    IM360_CHECK_ARG(w.nW > 0 && w.outer > 0 && w.inner > 0 && w.L > 0 && w.L <= w.F && w.F < (1 << 30),
                    "%s: nW=%d outer=%ld F=%ld L=%ld inner=%ld out of range", name, w.nW, (long)w.outer, (long)w.F, (long)w.L, (long)w.inner);
    if (const int rc = step ? check_step(name, *step) : IM360_OK) return rc;
    IM360_CHECK_ARG(((uintptr_t)w.start % 4) == 0 && ((uintptr_t)w.weight % 4) == 0, "%s: misaligned table", name);
    return IM360_OK;
}
// The instantiation a step launch selects: 0 guided, 1 guided with the guidance rescale, 2 unguided (one prediction; never rescaled)
static int step_variant(bool rescale, bool guided) { return guided ? (rescale ? 1 : 0) : 2; }
static unsigned step_blocks(long lanes) { return (unsigned)((lanes + 255) / 256 > 4096 ? 4096 : (lanes + 255) / 256); }

// im360_cfg_ddim_step and, with the guidance rescale, im360_cfg_ddim_step_rescale: checks, then the launch.  !guided (im360_ddim_step):
// `cond` is the one prediction, `uncond` is not looked at.
static int cfg_ddim_step(const char* name, const void* uncond, const void* cond, const void* x, void* out, int64_t n, const StepArgs& s,
                         bool rescale, int dtype, void* stream, bool guided = true) {
    if (const int rc = check_tensors(name, {guided ? uncond : cond, cond, x, out}, s.noise, n)) return rc;
    if (const int rc = check_step(name, s)) return rc;
    if (const int rc = rescale ? check_step_rescale(name, s, n) : IM360_OK) return rc;
    const long n8 = n / 8;
    const int nrec = rescale ? (int)im360_cfg_rescale_records(n) : 0;
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<0, 1, 2>(step_variant(rescale, guided), [&](auto v) {
            constexpr int VAR = decltype(v)::value;
            hipLaunchKernelGGL((cfg_ddim_step_kernel<T, VAR == 1, VAR != 2>), dim3(step_blocks(n8)), dim3(256), 0, (hipStream_t)stream,
                               (const T*)(guided ? uncond : nullptr), (const T*)cond, (const T*)x, (const T*)s.noise, (T*)out, n8, s.g, s.sa, s.sb, s.sap, s.dir,
                               s.sigma, s.mode, (const float*)s.coef_dev, (const float*)s.ws, nrec, s.phi);
        });
        return im360_launch_status();
    });
}

// the four windowed step entry points (w.wrap: line or ring; rescale: with or without the guidance rescale): checks, then the launch
// !guided: w.pred is [nW, 1, outer, L, inner]
static int cfg_ddim_step_windows(const char* name, const Windows& w, const void* x, void* out, const StepArgs& s, bool rescale, int dtype,
                                 void* stream, bool guided = true) {
    if (const int rc = check_windows(name, w, x && out, &s)) return rc;          // (mode and noise of `s` inside: the entry points' order)
    if (const int rc = rescale ? check_step_rescale(name, s, w.elements()) : IM360_OK) return rc;
    const bool vec = (w.inner % 8) == 0 && (((uintptr_t)w.pred | (uintptr_t)x | (uintptr_t)s.noise | (uintptr_t)out) % 16) == 0;
    const long nv = (long)w.elements() / (vec ? 8 : 1);
    const int nrec = rescale ? (int)im360_cfg_rescale_records(w.elements()) : 0;
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) { with_const<0, 1, 2>(step_variant(rescale, guided), [&](auto sv) {
            constexpr int VAR = decltype(sv)::value;
            hipLaunchKernelGGL((cfg_ddim_step_windows_kernel<T, decltype(v)::value, VAR == 1, VAR != 2>), dim3(step_blocks(nv)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)w.pred, (const T*)x, (const T*)s.noise, (T*)out, (const int*)w.start,
                               (const float*)w.weight, w.nW, (long)w.outer, (int)w.F, (int)w.L, w.wrap, (long)w.inner, s.g, s.sa, s.sb, s.sap,
                               s.dir, s.sigma, s.mode, (const float*)s.coef_dev, (const float*)s.ws, nrec, s.phi);
        }); });
        return im360_launch_status();
    });
}

// im360_cfg_rescale_stats_windows (w.wrap = 0) and im360_cfg_rescale_stats_windows_ring (w.wrap = F): checks, then the launch
static int cfg_rescale_stats_windows(const char* name, const Windows& w, float guidance, void* ws, int64_t ws_floats, int dtype, void* stream,
                                     const void* coef_dev) {
    if (const int rc = check_windows(name, w, true, nullptr)) return rc;         // (no other pointer, no step arguments to check)
    if (const int rc = check_rescale_ws(name, ws, ws_floats, w.elements())) return rc;
    const bool vec = (w.inner % 8) == 0 && ((uintptr_t)w.pred % 16) == 0;
    const unsigned blocks = (unsigned)im360_cfg_rescale_records(w.elements());
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) {
            hipLaunchKernelGGL((cfg_rescale_stats_windows_kernel<T, decltype(v)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                               (const T*)w.pred, (const int*)w.start, (const float*)w.weight, w.nW, (long)w.outer, (int)w.F, (int)w.L, w.wrap,
                               (long)w.inner, guidance, (const float*)coef_dev, (float*)ws);
        });
        return im360_launch_status();
    });
}

// What the two multistep entry points are given besides their tensors; `s` carries what the shared checks read (mode, phi, workspace)
struct MultistepArgs {
    StepArgs s;
    float cx, c0, c1;
    void* hist;
    bool rescale() const { return s.ws != nullptr; }
};
static StepArgs multistep_step_args(float g, float sa, float sb, int mode, float phi, const void* ws, int64_t ws_floats, const void* coef_dev) {
    return StepArgs{g, sa, sb, 0.0f, 0.0f, 0.0f, mode, nullptr, coef_dev, ws, ws_floats, phi};
}
// mode bit 8 (use_clipped_model_output) has no meaning for the multistep update; a strength without a workspace is a forgotten
// statistics pass; with a workspace: check_step_rescale for n elements
static int check_multistep(const char* name, const MultistepArgs& a, int64_t n) {
    IM360_CHECK_ARG((a.s.mode & 8) == 0, "%s: mode %d: bit 8 (use_clipped_model_output) unsupported", name, a.s.mode);
    IM360_CHECK_ARG(a.rescale() || a.s.phi == 0.0f, "%s: rescale=%g needs the workspace of a statistics pass", name, (double)a.s.phi);
    return a.rescale() ? check_step_rescale(name, a.s, n) : IM360_OK;
}

// im360_cfg_multistep_step: checks, then the launch.  !guided (im360_multistep_step): `cond` is the one prediction, no workspace.
static int cfg_multistep_step(const char* name, const void* uncond, const void* cond, const void* x, void* out, int64_t n,
                              const MultistepArgs& a, int dtype, void* stream, bool guided = true) {
    if (const int rc = check_tensors(name, {guided ? uncond : cond, cond, x, a.hist, out}, nullptr, n)) return rc;
    if (const int rc = check_step(name, a.s)) return rc;
    if (const int rc = check_multistep(name, a, n)) return rc;
    const long n8 = n / 8;
    const int nrec = a.rescale() ? (int)im360_cfg_rescale_records(n) : 0;
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<0, 1, 2>(step_variant(a.rescale(), guided), [&](auto v) {
            constexpr int VAR = decltype(v)::value;
            hipLaunchKernelGGL((cfg_multistep_step_kernel<T, VAR == 1, VAR != 2>), dim3(step_blocks(n8)), dim3(256), 0, (hipStream_t)stream,
                               (const T*)(guided ? uncond : nullptr), (const T*)cond, (const T*)x, (float*)a.hist, (T*)out, n8, a.s.g, a.s.sa, a.s.sb, a.cx, a.c0,
                               a.c1, a.s.mode, (const float*)a.s.coef_dev, (const float*)a.s.ws, nrec, a.s.phi);
        });
        return im360_launch_status();
    });
}

// im360_cfg_multistep_step_windows (w.wrap: line or ring): checks, then the launch
static int cfg_multistep_step_windows(const char* name, const Windows& w, int64_t wrap, const void* x, void* out, const MultistepArgs& a,
                                      int dtype, void* stream, bool guided = true) {
    if (const int rc = check_windows(name, w, x && a.hist && out, &a.s)) return rc;
    IM360_CHECK_ARG(wrap == 0 || wrap == w.F, "%s: wrap=%ld must be 0 (line) or F=%ld (ring)", name, (long)wrap, (long)w.F);
    IM360_CHECK_ARG(((uintptr_t)a.hist % 4) == 0, "%s: misaligned history", name);
    if (const int rc = check_multistep(name, a, w.elements())) return rc;
    const bool vec = (w.inner % 8) == 0 && (((uintptr_t)w.pred | (uintptr_t)x | (uintptr_t)a.hist | (uintptr_t)out) % 16) == 0;
    const long nv = (long)w.elements() / (vec ? 8 : 1);
    const int nrec = a.rescale() ? (int)im360_cfg_rescale_records(w.elements()) : 0;
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) { with_const<0, 1, 2>(step_variant(a.rescale(), guided), [&](auto sv) {
            constexpr int VAR = decltype(sv)::value;
            hipLaunchKernelGGL((cfg_multistep_step_windows_kernel<T, decltype(v)::value, VAR == 1, VAR != 2>), dim3(step_blocks(nv)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)w.pred, (const T*)x, (float*)a.hist, (T*)out, (const int*)w.start,
                               (const float*)w.weight, w.nW, (long)w.outer, (int)w.F, (int)w.L, w.wrap, (long)w.inner, a.s.g, a.s.sa, a.s.sb,
                               a.cx, a.c0, a.c1, a.s.mode, (const float*)a.s.coef_dev, (const float*)a.s.ws, nrec, a.s.phi);
        }); });
        return im360_launch_status();
    });
}
}  // namespace im360

// out = cx * x + cv * (uncond + g (cond - uncond)), n elements (n % 8 == 0), all same dtype
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_update(const void* uncond, const void* cond, const void* x, void* out, int64_t n,
                                   float guidance, float cx, float cv, int dtype, void* stream, const void* coef_dev) {
    using namespace im360;
    if (const int rc = check_tensors("cfg_ddim_update", {uncond, cond, x, out}, nullptr, n)) return rc;
    return with_dtype(dtype, "cfg_ddim_update", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cfg_ddim_kernel<T>), dim3(step_blocks(n / 8)), dim3(256), 0, (hipStream_t)stream, (const T*)uncond, (const T*)cond,
                           (const T*)x, (T*)out, (long)(n / 8), guidance, cx, cv, (const float*)coef_dev);
        return im360_launch_status();
    });
}

// partial moments of cond and of uncond + g (cond - uncond) over n elements (n % 8 == 0) -> ws
extern "C" __attribute__((visibility("default"))) int im360_cfg_rescale_stats(const void* uncond, const void* cond, int64_t n, float guidance,
                                   void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    using namespace im360;
    if (const int rc = check_tensors("cfg_rescale_stats", {uncond, cond}, nullptr, n)) return rc;
    if (const int rc = check_rescale_ws("cfg_rescale_stats", ws, ws_floats, n)) return rc;
    const unsigned blocks = (unsigned)im360_cfg_rescale_records(n);
    return with_dtype(dtype, "cfg_rescale_stats", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cfg_rescale_stats_kernel<T>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)uncond, (const T*)cond,
                           (long)(n / 8), guidance, (const float*)coef_dev, (float*)ws);
        return im360_launch_status();
    });
}

// the same over the per-frame blends of nW sliding-window predictions (layout and tables of im360_cfg_ddim_step_windows)
extern "C" __attribute__((visibility("default"))) int im360_cfg_rescale_stats_windows(const void* pred, const void* start, const void* weight, int nW,
                                   int64_t outer, int64_t F, int64_t L, int64_t inner, float guidance, void* ws, int64_t ws_floats, int dtype,
                                   void* stream, const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, 0, outer, F, L, inner};
    return im360::cfg_rescale_stats_windows("cfg_rescale_stats_windows", w, guidance, ws, ws_floats, dtype, stream, coef_dev);
}

// the same with the windows on a ring of F frames (tables of im360_cfg_ddim_step_windows_ring).  The host cannot see the tables:
// the caller guarantees 0 <= start[k] < F, every frame covered, L <= F.
extern "C" __attribute__((visibility("default"))) int im360_cfg_rescale_stats_windows_ring(const void* pred, const void* start, const void* weight,
                                   int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float guidance, void* ws, int64_t ws_floats, int dtype,
                                   void* stream, const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, (int)F, outer, F, L, inner};
    return im360::cfg_rescale_stats_windows("cfg_rescale_stats_windows_ring", w, guidance, ws, ws_floats, dtype, stream, coef_dev);
}

// out[0] = r = phi std(c) / std(m) + (1 - phi) from the records a statistics pass over n elements left in ws
extern "C" __attribute__((visibility("default"))) int im360_cfg_rescale_factor(const void* ws, int64_t ws_floats, int64_t n, float phi, void* out,
                                   void* stream) {
    using namespace im360;
    IM360_CHECK_ARG(out && ((uintptr_t)out % 4) == 0 && n > 0, "cfg_rescale_factor: null or misaligned output / empty problem");
    IM360_CHECK_ARG(std::isfinite(phi), "cfg_rescale_factor: rescale=%g must be finite", (double)phi);
    if (const int rc = check_rescale_ws("cfg_rescale_factor", ws, ws_floats, n)) return rc;
    hipLaunchKernelGGL(cfg_rescale_factor_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws,
                       (int)im360_cfg_rescale_records(n), phi, (float*)out);
    return im360_launch_status();
}

// out = DDIMScheduler.step(uncond + g (cond - uncond), x, noise) for any prediction type / clip / eta, n elements (n % 8 == 0),
// all same dtype; noise may be null (zero noise)
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step(const void* uncond, const void* cond, const void* x, const void* noise,
                                   void* out, int64_t n, float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma,
                                   int mode, int dtype, void* stream, const void* coef_dev) {
    const im360::StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    return im360::cfg_ddim_step("cfg_ddim_step", uncond, cond, x, out, n, s, false, dtype, stream);
}

// the same step on r (uncond + g (cond - uncond)), r from the records im360_cfg_rescale_stats left in ws for the same n
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step_rescale(const void* uncond, const void* cond, const void* x,
                                   const void* noise, void* out, int64_t n, float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir,
                                   float sigma, int mode, float phi, const void* ws, int64_t ws_floats, int dtype, void* stream,
                                   const void* coef_dev) {
    const im360::StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, ws, ws_floats, phi};
    return im360::cfg_ddim_step("cfg_ddim_step_rescale", uncond, cond, x, out, n, s, true, dtype, stream);
}

// The step of im360_cfg_ddim_step on the per-frame weighted blend of nW sliding-window predictions (see the kernel's comment):
// x / noise / out [outer, F, inner], pred [nW, 2, outer, L, inner], start int32[nW] and weight float[L] on the device.  The host
// cannot see the tables: the caller guarantees 0 <= start[k] <= F - L and that every frame is covered (imagine360_amd/context.py).
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step_windows(const void* pred, const void* x, const void* noise, void* out,
                                   const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float guidance,
                                   float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, int dtype, void* stream,
                                   const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, 0, outer, F, L, inner};
    const im360::StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    return im360::cfg_ddim_step_windows("cfg_ddim_step_windows", w, x, out, s, false, dtype, stream);
}

// the same on r times the blend, r from the records im360_cfg_rescale_stats_windows left in ws for the same clip
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step_windows_rescale(const void* pred, const void* x, const void* noise,
                                   void* out, const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner,
                                   float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, float phi,
                                   const void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, 0, outer, F, L, inner};
    const im360::StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, ws, ws_floats, phi};
    return im360::cfg_ddim_step_windows("cfg_ddim_step_windows_rescale", w, x, out, s, true, dtype, stream);
}

// im360_cfg_ddim_step_windows with the windows on a ring of F frames: window k covers the frames (start[k] + j) mod F, j = 0 .. L - 1,
// position j of its prediction.  Same blend, same slot order, same step.  The host cannot see the tables: the caller guarantees
// 0 <= start[k] < F, every frame covered, L <= F (imagine360_amd/context.py, loop=True).
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step_windows_ring(const void* pred, const void* x, const void* noise, void* out,
                                   const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float guidance,
                                   float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, int dtype, void* stream,
                                   const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, (int)F, outer, F, L, inner};
    const im360::StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    return im360::cfg_ddim_step_windows("cfg_ddim_step_windows_ring", w, x, out, s, false, dtype, stream);
}

// the same on r times the blend, r from the records im360_cfg_rescale_stats_windows_ring left in ws for the same clip; the
// precondition of im360_cfg_ddim_step_windows_ring: 0 <= start[k] < F, every frame covered, L <= F
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step_windows_ring_rescale(const void* pred, const void* x, const void* noise,
                                   void* out, const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner,
                                   float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, float phi,
                                   const void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, (int)F, outer, F, L, inner};
    const im360::StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, ws, ws_floats, phi};
    return im360::cfg_ddim_step_windows("cfg_ddim_step_windows_ring_rescale", w, x, out, s, true, dtype, stream);
}

// out = the DPM-Solver++ 2M update (arXiv 2211.01095, algorithm 2) of x on uncond + g (cond - uncond), hist <- x0 (fp32, in place);
// n elements (n % 8 == 0), uncond / cond / x / out of the same 16-bit dtype; ws == NULL: without the guidance rescale
extern "C" __attribute__((visibility("default"))) int im360_cfg_multistep_step(const void* uncond, const void* cond, const void* x, void* hist,
                                   void* out, int64_t n, float guidance, float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode,
                                   float phi, const void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    const im360::MultistepArgs a{im360::multistep_step_args(guidance, sqrt_a, sqrt_b, mode, phi, ws, ws_floats, coef_dev), cx, c0, c1, hist};
    return im360::cfg_multistep_step("cfg_multistep_step", uncond, cond, x, out, n, a, dtype, stream);
}

// the same update on the per-frame blend of nW sliding-window predictions (tables and layout of im360_cfg_ddim_step_windows);
// wrap = 0: the windows lie on a line, wrap = F: on a ring (preconditions of im360_cfg_ddim_step_windows_ring)
extern "C" __attribute__((visibility("default"))) int im360_cfg_multistep_step_windows(const void* pred, const void* x, void* hist, void* out,
                                   const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, int64_t wrap,
                                   float guidance, float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode, float phi, const void* ws,
                                   int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, wrap == 0 ? 0 : (int)F, outer, F, L, inner};
    const im360::MultistepArgs a{im360::multistep_step_args(guidance, sqrt_a, sqrt_b, mode, phi, ws, ws_floats, coef_dev), cx, c0, c1, hist};
    return im360::cfg_multistep_step_windows("cfg_multistep_step_windows", w, wrap, x, out, a, dtype, stream);
}

// ---- the unguided forms: a step outside the guidance interval (arXiv 2404.07724), where the model ran the text half alone.  `pred` is
//      that one prediction and takes the place of uncond + g (cond - uncond); there is no guidance argument, and coef_dev is the
//      sibling's vector (element 0, the guidance, is not read).  For finite inputs each gives what its sibling gives when uncond and
//      cond are the same tensor, bit for bit.  No rescale forms: a prediction rescaled towards its own standard deviation is itself.

// out = cx * x + cv * pred; coef_dev: float[3] = (guidance, cx, cv) of im360_cfg_ddim_update
extern "C" __attribute__((visibility("default"))) int im360_ddim_update(const void* pred, const void* x, void* out, int64_t n, float cx, float cv,
                                   int dtype, void* stream, const void* coef_dev) {
    using namespace im360;
    if (const int rc = check_tensors("ddim_update", {pred, x, out}, nullptr, n)) return rc;
    return with_dtype(dtype, "ddim_update", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((ddim_kernel<T>), dim3(step_blocks(n / 8)), dim3(256), 0, (hipStream_t)stream, (const T*)pred, (const T*)x, (T*)out,
                           (long)(n / 8), cx, cv, (const float*)coef_dev);
        return im360_launch_status();
    });
}

// out = DDIMScheduler.step(pred, x, noise): im360_cfg_ddim_step without the combine
extern "C" __attribute__((visibility("default"))) int im360_ddim_step(const void* pred, const void* x, const void* noise, void* out, int64_t n,
                                   float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, int dtype, void* stream,
                                   const void* coef_dev) {
    const im360::StepArgs s{0.0f, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    return im360::cfg_ddim_step("ddim_step", nullptr, pred, x, out, n, s, false, dtype, stream, false);
}

// im360_cfg_ddim_step_windows on the blend of the text halves alone: pred [nW, 1, outer, L, inner]
extern "C" __attribute__((visibility("default"))) int im360_ddim_step_windows(const void* pred, const void* x, const void* noise, void* out,
                                   const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner,
                                   float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, int dtype, void* stream,
                                   const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, 0, outer, F, L, inner};
    const im360::StepArgs s{0.0f, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    return im360::cfg_ddim_step_windows("ddim_step_windows", w, x, out, s, false, dtype, stream, false);
}

// the same with the windows on a ring of F frames (preconditions of im360_cfg_ddim_step_windows_ring)
extern "C" __attribute__((visibility("default"))) int im360_ddim_step_windows_ring(const void* pred, const void* x, const void* noise, void* out,
                                   const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner,
                                   float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, int dtype, void* stream,
                                   const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, (int)F, outer, F, L, inner};
    const im360::StepArgs s{0.0f, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    return im360::cfg_ddim_step_windows("ddim_step_windows_ring", w, x, out, s, false, dtype, stream, false);
}

// out = the DPM-Solver++ 2M update of x on pred, hist <- x0: im360_cfg_multistep_step without the combine
extern "C" __attribute__((visibility("default"))) int im360_multistep_step(const void* pred, const void* x, void* hist, void* out, int64_t n,
                                   float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode, int dtype, void* stream,
                                   const void* coef_dev) {
    const im360::MultistepArgs a{im360::multistep_step_args(0.0f, sqrt_a, sqrt_b, mode, 0.0f, nullptr, 0, coef_dev), cx, c0, c1, hist};
    return im360::cfg_multistep_step("multistep_step", nullptr, pred, x, out, n, a, dtype, stream, false);
}

// im360_cfg_multistep_step_windows on the blend of the text halves alone: pred [nW, 1, outer, L, inner]; wrap = 0 or F
extern "C" __attribute__((visibility("default"))) int im360_multistep_step_windows(const void* pred, const void* x, void* hist, void* out,
                                   const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, int64_t wrap,
                                   float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode, int dtype, void* stream,
                                   const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, wrap == 0 ? 0 : (int)F, outer, F, L, inner};
    const im360::MultistepArgs a{im360::multistep_step_args(0.0f, sqrt_a, sqrt_b, mode, 0.0f, nullptr, 0, coef_dev), cx, c0, c1, hist};
    return im360::cfg_multistep_step_windows("multistep_step_windows", w, wrap, x, out, a, dtype, stream, false);
}

// ---- adaptive projected guidance: the statistics pass, the scalars, and the four guided steps on the projected guidance
namespace im360 {
// What an _apg entry point is given besides its sibling's arguments: eta (the share of the parallel part that is kept), the RMS radius r
// of the clamp in x0 units (INFINITY: no clamp) and the workspace of records a statistics pass wrote for the same tensors
struct ApgArgs {
    float eta, r;
    const void* ws;
    int64_t ws_floats;
};
static int check_apg(const char* name, const ApgArgs& a, int64_t n) {
    IM360_CHECK_ARG(std::isfinite(a.eta), "%s: apg eta=%g must be finite", name, (double)a.eta);
    IM360_CHECK_ARG(a.r > 0.0f, "%s: apg threshold=%g must be > 0 (INFINITY: no clamp)", name, (double)a.r);          // (a NaN fails too)
    return check_rescale_ws(name, a.ws, a.ws_floats, n);
}
// the mode bits of a statistics pass or of the scalars: only the prediction type is read, the whole word is held to the steps' range
static int check_apg_mode(const char* name, int mode) {
    IM360_CHECK_ARG(mode >= 0 && mode < 16 && (mode & 3) != 3, "%s: mode %d unsupported", name, mode);
    return IM360_OK;
}

// im360_cfg_apg_stats_windows (w.wrap = 0) and im360_cfg_apg_stats_windows_ring (w.wrap = F): checks, then the launch
static int cfg_apg_stats_windows(const char* name, const Windows& w, const void* x, float sa, float sb, int mode, void* ws, int64_t ws_floats,
                                 int dtype, void* stream, const void* coef_dev) {
    if (const int rc = check_windows(name, w, x != nullptr, nullptr)) return rc;
    if (const int rc = check_apg_mode(name, mode)) return rc;
    if (const int rc = check_rescale_ws(name, ws, ws_floats, w.elements())) return rc;
    const bool vec = (w.inner % 8) == 0 && (((uintptr_t)w.pred | (uintptr_t)x) % 16) == 0;
    const unsigned blocks = (unsigned)im360_cfg_rescale_records(w.elements());
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) {
            hipLaunchKernelGGL((cfg_apg_stats_windows_kernel<T, decltype(v)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                               (const T*)w.pred, (const T*)x, (const int*)w.start, (const float*)w.weight, w.nW, (long)w.outer, (int)w.F, (int)w.L,
                               w.wrap, (long)w.inner, sa, sb, mode, (const float*)coef_dev, (float*)ws);
        });
        return im360_launch_status();
    });
}

// im360_cfg_ddim_step_windows_apg: the checks of cfg_ddim_step_windows, wrap, the APG arguments, then the launch
static int cfg_ddim_step_windows_apg(const char* name, const Windows& w, int64_t wrap, const void* x, void* out, const StepArgs& s,
                                     const ApgArgs& a, int dtype, void* stream) {
    if (const int rc = check_windows(name, w, x && out, &s)) return rc;
    IM360_CHECK_ARG(wrap == 0 || wrap == w.F, "%s: wrap=%ld must be 0 (line) or F=%ld (ring)", name, (long)wrap, (long)w.F);
    if (const int rc = check_apg(name, a, w.elements())) return rc;
    const bool vec = (w.inner % 8) == 0 && (((uintptr_t)w.pred | (uintptr_t)x | (uintptr_t)s.noise | (uintptr_t)out) % 16) == 0;
    const long nv = (long)w.elements() / (vec ? 8 : 1);
    const int nrec = (int)im360_cfg_rescale_records(w.elements());
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) {
            hipLaunchKernelGGL((cfg_ddim_step_windows_apg_kernel<T, decltype(v)::value>), dim3(step_blocks(nv)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)w.pred, (const T*)x, (const T*)s.noise, (T*)out, (const int*)w.start,
                               (const float*)w.weight, w.nW, (long)w.outer, (int)w.F, (int)w.L, w.wrap, (long)w.inner, s.g, s.sa, s.sb, s.sap,
                               s.dir, s.sigma, s.mode, (const float*)s.coef_dev, (const float*)a.ws, nrec, a.eta, a.r);
        });
        return im360_launch_status();
    });
}
}  // namespace im360

// partial sums of d q, q^2 and d^2 (d = cond - uncond, q = cond + rho x; see the kernels' comment) over n elements (n % 8 == 0) -> ws
extern "C" __attribute__((visibility("default"))) int im360_cfg_apg_stats(const void* uncond, const void* cond, const void* x, int64_t n,
                                   float sqrt_a, float sqrt_b, int mode, void* ws, int64_t ws_floats, int dtype, void* stream,
                                   const void* coef_dev) {
    using namespace im360;
    if (const int rc = check_tensors("cfg_apg_stats", {uncond, cond, x}, nullptr, n)) return rc;
    if (const int rc = check_apg_mode("cfg_apg_stats", mode)) return rc;
    if (const int rc = check_rescale_ws("cfg_apg_stats", ws, ws_floats, n)) return rc;
    const unsigned blocks = (unsigned)im360_cfg_rescale_records(n);
    return with_dtype(dtype, "cfg_apg_stats", [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cfg_apg_stats_kernel<T>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)uncond, (const T*)cond,
                           (const T*)x, (long)(n / 8), sqrt_a, sqrt_b, mode, (const float*)coef_dev, (float*)ws);
        return im360_launch_status();
    });
}

// the same over the per-frame blends of nW sliding-window predictions (layout and tables of im360_cfg_ddim_step_windows)
extern "C" __attribute__((visibility("default"))) int im360_cfg_apg_stats_windows(const void* pred, const void* x, const void* start,
                                   const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float sqrt_a, float sqrt_b,
                                   int mode, void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, 0, outer, F, L, inner};
    return im360::cfg_apg_stats_windows("cfg_apg_stats_windows", w, x, sqrt_a, sqrt_b, mode, ws, ws_floats, dtype, stream, coef_dev);
}

// the same with the windows on a ring of F frames (preconditions of im360_cfg_ddim_step_windows_ring)
extern "C" __attribute__((visibility("default"))) int im360_cfg_apg_stats_windows_ring(const void* pred, const void* x, const void* start,
                                   const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float sqrt_a, float sqrt_b,
                                   int mode, void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, (int)F, outer, F, L, inner};
    return im360::cfg_apg_stats_windows("cfg_apg_stats_windows_ring", w, x, sqrt_a, sqrt_b, mode, ws, ws_floats, dtype, stream, coef_dev);
}

// out[0 .. 2] = (alpha, s, lambda) from the records a statistics pass over n elements left in ws
extern "C" __attribute__((visibility("default"))) int im360_cfg_apg_scalars(const void* ws, int64_t ws_floats, int64_t n, float guidance,
                                   float sqrt_a, float sqrt_b, int mode, float eta, float threshold, void* out, void* stream,
                                   const void* coef_dev) {
    using namespace im360;
    IM360_CHECK_ARG(out && ((uintptr_t)out % 4) == 0 && n > 0, "cfg_apg_scalars: null or misaligned output / empty problem");
    if (const int rc = check_apg_mode("cfg_apg_scalars", mode)) return rc;
    if (const int rc = check_apg("cfg_apg_scalars", ApgArgs{eta, threshold, ws, ws_floats}, n)) return rc;
    hipLaunchKernelGGL(cfg_apg_scalars_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, (int)im360_cfg_rescale_records(n),
                       guidance, sqrt_a, sqrt_b, mode, eta, threshold, (const float*)coef_dev, (float*)out);
    return im360_launch_status();
}

// im360_cfg_ddim_step on the projected guidance m, its scalars from the records im360_cfg_apg_stats left in ws for the same tensors
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step_apg(const void* uncond, const void* cond, const void* x, const void* noise,
                                   void* out, int64_t n, float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma,
                                   int mode, float eta, float threshold, const void* ws, int64_t ws_floats, int dtype, void* stream,
                                   const void* coef_dev) {
    using namespace im360;
    const char* name = "cfg_ddim_step_apg";
    const StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    const ApgArgs a{eta, threshold, ws, ws_floats};
    if (const int rc = check_tensors(name, {uncond, cond, x, out}, noise, n)) return rc;
    if (const int rc = check_step(name, s)) return rc;
    if (const int rc = check_apg(name, a, n)) return rc;
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cfg_ddim_step_apg_kernel<T>), dim3(step_blocks(n / 8)), dim3(256), 0, (hipStream_t)stream, (const T*)uncond,
                           (const T*)cond, (const T*)x, (const T*)noise, (T*)out, (long)(n / 8), guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma,
                           mode, (const float*)coef_dev, (const float*)ws, (int)im360_cfg_rescale_records(n), eta, threshold);
        return im360_launch_status();
    });
}

// im360_cfg_ddim_step_windows (wrap = 0) / im360_cfg_ddim_step_windows_ring (wrap = F) on the projected guidance of the blends, its
// scalars from the records im360_cfg_apg_stats_windows(_ring) left in ws for the same clip
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step_windows_apg(const void* pred, const void* x, const void* noise,
                                   void* out, const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner,
                                   int64_t wrap, float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode,
                                   float eta, float threshold, const void* ws, int64_t ws_floats, int dtype, void* stream,
                                   const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, wrap == 0 ? 0 : (int)F, outer, F, L, inner};
    const im360::StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    return im360::cfg_ddim_step_windows_apg("cfg_ddim_step_windows_apg", w, wrap, x, out, s, im360::ApgArgs{eta, threshold, ws, ws_floats}, dtype,
                                            stream);
}

// im360_cfg_multistep_step on the projected guidance (hist <- its x0)
extern "C" __attribute__((visibility("default"))) int im360_cfg_multistep_step_apg(const void* uncond, const void* cond, const void* x, void* hist,
                                   void* out, int64_t n, float guidance, float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode,
                                   float eta, float threshold, const void* ws, int64_t ws_floats, int dtype, void* stream,
                                   const void* coef_dev) {
    using namespace im360;
    const char* name = "cfg_multistep_step_apg";
    const MultistepArgs m{multistep_step_args(guidance, sqrt_a, sqrt_b, mode, 0.0f, nullptr, 0, coef_dev), cx, c0, c1, hist};
    const ApgArgs a{eta, threshold, ws, ws_floats};
    if (const int rc = check_tensors(name, {uncond, cond, x, hist, out}, nullptr, n)) return rc;
    if (const int rc = check_step(name, m.s)) return rc;
    if (const int rc = check_multistep(name, m, n)) return rc;
    if (const int rc = check_apg(name, a, n)) return rc;
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cfg_multistep_step_apg_kernel<T>), dim3(step_blocks(n / 8)), dim3(256), 0, (hipStream_t)stream, (const T*)uncond,
                           (const T*)cond, (const T*)x, (float*)hist, (T*)out, (long)(n / 8), guidance, sqrt_a, sqrt_b, cx, c0, c1, mode,
                           (const float*)coef_dev, (const float*)ws, (int)im360_cfg_rescale_records(n), eta, threshold);
        return im360_launch_status();
    });
}

// im360_cfg_multistep_step_windows on the projected guidance of the blends; wrap = 0 or F
extern "C" __attribute__((visibility("default"))) int im360_cfg_multistep_step_windows_apg(const void* pred, const void* x, void* hist, void* out,
                                   const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, int64_t wrap,
                                   float guidance, float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode, float eta, float threshold,
                                   const void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    using namespace im360;
    const char* name = "cfg_multistep_step_windows_apg";
    const Windows w{pred, start, weight, nW, wrap == 0 ? 0 : (int)F, outer, F, L, inner};
    const MultistepArgs m{multistep_step_args(guidance, sqrt_a, sqrt_b, mode, 0.0f, nullptr, 0, coef_dev), cx, c0, c1, hist};
    const ApgArgs a{eta, threshold, ws, ws_floats};
    if (const int rc = check_windows(name, w, x && hist && out, &m.s)) return rc;
    IM360_CHECK_ARG(wrap == 0 || wrap == F, "%s: wrap=%ld must be 0 (line) or F=%ld (ring)", name, (long)wrap, (long)F);
    IM360_CHECK_ARG(((uintptr_t)hist % 4) == 0, "%s: misaligned history", name);
    if (const int rc = check_multistep(name, m, w.elements())) return rc;
    if (const int rc = check_apg(name, a, w.elements())) return rc;
    const bool vec = (inner % 8) == 0 && (((uintptr_t)pred | (uintptr_t)x | (uintptr_t)hist | (uintptr_t)out) % 16) == 0;
    const long nv = (long)w.elements() / (vec ? 8 : 1);
    const int nrec = (int)im360_cfg_rescale_records(w.elements());
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) {
            hipLaunchKernelGGL((cfg_multistep_step_windows_apg_kernel<T, decltype(v)::value>), dim3(step_blocks(nv)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)pred, (const T*)x, (float*)hist, (T*)out, (const int*)start, (const float*)weight, nW,
                               (long)outer, (int)F, (int)L, w.wrap, (long)inner, guidance, sqrt_a, sqrt_b, cx, c0, c1, mode,
                               (const float*)coef_dev, (const float*)ws, nrec, eta, threshold);
        });
        return im360_launch_status();
    });
}

// ---- adaptive projected guidance with momentum: the statistics pass and the four guided steps on e = d + carry * state
namespace im360 {
// What an _apg_momentum entry point is given besides its _apg sibling's arguments: the fp32 state of n elements (read when carry != 0;
// written by the steps, never by a statistics pass), the host carry and the optional device carry (float[1], read instead)
struct ApgMomentum {
    const void* state;
    float carry;
    const void* carry_dev;
};
// `vec`: the launch moves the state in 16-byte lanes
static int check_apg_momentum(const char* name, const ApgMomentum& m, bool vec) {
    IM360_CHECK_ARG(m.state && ((uintptr_t)m.state % (vec ? 16 : 4)) == 0, "%s: null or misaligned momentum state", name);
    IM360_CHECK_ARG(std::isfinite(m.carry), "%s: apg carry=%g must be finite", name, (double)m.carry);
    IM360_CHECK_ARG(((uintptr_t)m.carry_dev % 4) == 0, "%s: misaligned device carry", name);
    return IM360_OK;
}

// im360_cfg_apg_momentum_stats_windows (w.wrap = 0) and _ring (w.wrap = F): checks, then the launch
static int cfg_apg_momentum_stats_windows(const char* name, const Windows& w, const void* x, const ApgMomentum& m, float sa, float sb, int mode,
                                          void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    if (const int rc = check_windows(name, w, x != nullptr, nullptr)) return rc;
    if (const int rc = check_apg_mode(name, mode)) return rc;
    if (const int rc = check_rescale_ws(name, ws, ws_floats, w.elements())) return rc;
    const bool vec = (w.inner % 8) == 0 && (((uintptr_t)w.pred | (uintptr_t)x | (uintptr_t)m.state) % 16) == 0;
    if (const int rc = check_apg_momentum(name, m, vec)) return rc;
    const unsigned blocks = (unsigned)im360_cfg_rescale_records(w.elements());
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) {
            hipLaunchKernelGGL((cfg_apg_momentum_stats_windows_kernel<T, decltype(v)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                               (const T*)w.pred, (const T*)x, (const float*)m.state, (const int*)w.start, (const float*)w.weight, w.nW,
                               (long)w.outer, (int)w.F, (int)w.L, w.wrap, (long)w.inner, sa, sb, mode, m.carry, (const float*)m.carry_dev,
                               (const float*)coef_dev, (float*)ws);
        });
        return im360_launch_status();
    });
}
}  // namespace im360

// im360_cfg_apg_stats over e = (cond - uncond) + carry * state: the partial sums of e q, q^2 and e^2 -> ws
extern "C" __attribute__((visibility("default"))) int im360_cfg_apg_momentum_stats(const void* uncond, const void* cond, const void* x,
                                   const void* state, int64_t n, float sqrt_a, float sqrt_b, int mode, float carry, const void* carry_dev,
                                   void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    using namespace im360;
    const char* name = "cfg_apg_momentum_stats";
    if (const int rc = check_tensors(name, {uncond, cond, x}, nullptr, n)) return rc;
    if (const int rc = check_apg_mode(name, mode)) return rc;
    if (const int rc = check_rescale_ws(name, ws, ws_floats, n)) return rc;
    if (const int rc = check_apg_momentum(name, ApgMomentum{state, carry, carry_dev}, true)) return rc;
    const unsigned blocks = (unsigned)im360_cfg_rescale_records(n);
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cfg_apg_momentum_stats_kernel<T>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const T*)uncond,
                           (const T*)cond, (const T*)x, (const float*)state, (long)(n / 8), sqrt_a, sqrt_b, mode, carry,
                           (const float*)carry_dev, (const float*)coef_dev, (float*)ws);
        return im360_launch_status();
    });
}

// the same over the per-frame blends of nW sliding-window predictions, state [outer, F, inner]
extern "C" __attribute__((visibility("default"))) int im360_cfg_apg_momentum_stats_windows(const void* pred, const void* x, const void* state,
                                   const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner,
                                   float sqrt_a, float sqrt_b, int mode, float carry, const void* carry_dev, void* ws, int64_t ws_floats,
                                   int dtype, void* stream, const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, 0, outer, F, L, inner};
    return im360::cfg_apg_momentum_stats_windows("cfg_apg_momentum_stats_windows", w, x, im360::ApgMomentum{state, carry, carry_dev}, sqrt_a,
                                                 sqrt_b, mode, ws, ws_floats, dtype, stream, coef_dev);
}

// the same with the windows on a ring of F frames (preconditions of im360_cfg_ddim_step_windows_ring)
extern "C" __attribute__((visibility("default"))) int im360_cfg_apg_momentum_stats_windows_ring(const void* pred, const void* x,
                                   const void* state, const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L,
                                   int64_t inner, float sqrt_a, float sqrt_b, int mode, float carry, const void* carry_dev, void* ws,
                                   int64_t ws_floats, int dtype, void* stream, const void* coef_dev) {
    const im360::Windows w{pred, start, weight, nW, (int)F, outer, F, L, inner};
    return im360::cfg_apg_momentum_stats_windows("cfg_apg_momentum_stats_windows_ring", w, x, im360::ApgMomentum{state, carry, carry_dev},
                                                 sqrt_a, sqrt_b, mode, ws, ws_floats, dtype, stream, coef_dev);
}

// im360_cfg_ddim_step_apg on e, state <- e; ws: the records of im360_cfg_apg_momentum_stats for the same tensors, state and carry
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step_apg_momentum(const void* uncond, const void* cond, const void* x,
                                   const void* noise, void* state, void* out, int64_t n, float guidance, float sqrt_a, float sqrt_b,
                                   float sqrt_a_prev, float dir, float sigma, int mode, float eta, float threshold, const void* ws,
                                   int64_t ws_floats, float carry, const void* carry_dev, int dtype, void* stream, const void* coef_dev) {
    using namespace im360;
    const char* name = "cfg_ddim_step_apg_momentum";
    const StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    const ApgArgs a{eta, threshold, ws, ws_floats};
    if (const int rc = check_tensors(name, {uncond, cond, x, out}, noise, n)) return rc;
    if (const int rc = check_step(name, s)) return rc;
    if (const int rc = check_apg(name, a, n)) return rc;
    if (const int rc = check_apg_momentum(name, ApgMomentum{state, carry, carry_dev}, true)) return rc;
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cfg_ddim_step_apg_momentum_kernel<T>), dim3(step_blocks(n / 8)), dim3(256), 0, (hipStream_t)stream,
                           (const T*)uncond, (const T*)cond, (const T*)x, (const T*)noise, (float*)state, (T*)out, (long)(n / 8), guidance,
                           sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, (const float*)coef_dev, (const float*)ws,
                           (int)im360_cfg_rescale_records(n), eta, threshold, carry, (const float*)carry_dev);
        return im360_launch_status();
    });
}

// im360_cfg_ddim_step_windows_apg on e, state [outer, F, inner] <- e; wrap = 0 (line) or F (ring)
extern "C" __attribute__((visibility("default"))) int im360_cfg_ddim_step_windows_apg_momentum(const void* pred, const void* x,
                                   const void* noise, void* state, void* out, const void* start, const void* weight, int nW, int64_t outer,
                                   int64_t F, int64_t L, int64_t inner, int64_t wrap, float guidance, float sqrt_a, float sqrt_b,
                                   float sqrt_a_prev, float dir, float sigma, int mode, float eta, float threshold, const void* ws,
                                   int64_t ws_floats, float carry, const void* carry_dev, int dtype, void* stream, const void* coef_dev) {
    using namespace im360;
    const char* name = "cfg_ddim_step_windows_apg_momentum";
    const Windows w{pred, start, weight, nW, wrap == 0 ? 0 : (int)F, outer, F, L, inner};
    const StepArgs s{guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma, mode, noise, coef_dev, nullptr, 0, 0.0f};
    const ApgArgs a{eta, threshold, ws, ws_floats};
    if (const int rc = check_windows(name, w, x && out, &s)) return rc;
    IM360_CHECK_ARG(wrap == 0 || wrap == F, "%s: wrap=%ld must be 0 (line) or F=%ld (ring)", name, (long)wrap, (long)F);
    if (const int rc = check_apg(name, a, w.elements())) return rc;
    const bool vec = (inner % 8) == 0 && (((uintptr_t)pred | (uintptr_t)x | (uintptr_t)noise | (uintptr_t)state | (uintptr_t)out) % 16) == 0;
    if (const int rc = check_apg_momentum(name, ApgMomentum{state, carry, carry_dev}, vec)) return rc;
    const long nv = (long)w.elements() / (vec ? 8 : 1);
    const int nrec = (int)im360_cfg_rescale_records(w.elements());
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) {
            hipLaunchKernelGGL((cfg_ddim_step_windows_apg_momentum_kernel<T, decltype(v)::value>), dim3(step_blocks(nv)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)pred, (const T*)x, (const T*)noise, (float*)state, (T*)out, (const int*)start,
                               (const float*)weight, nW, (long)outer, (int)F, (int)L, w.wrap, (long)inner, guidance, sqrt_a, sqrt_b,
                               sqrt_a_prev, dir, sigma, mode, (const float*)coef_dev, (const float*)ws, nrec, eta, threshold, carry,
                               (const float*)carry_dev);
        });
        return im360_launch_status();
    });
}

// im360_cfg_multistep_step_apg on e (hist <- the x0 of its projected guidance), state <- e
extern "C" __attribute__((visibility("default"))) int im360_cfg_multistep_step_apg_momentum(const void* uncond, const void* cond, const void* x,
                                   void* hist, void* state, void* out, int64_t n, float guidance, float sqrt_a, float sqrt_b, float cx,
                                   float c0, float c1, int mode, float eta, float threshold, const void* ws, int64_t ws_floats, float carry,
                                   const void* carry_dev, int dtype, void* stream, const void* coef_dev) {
    using namespace im360;
    const char* name = "cfg_multistep_step_apg_momentum";
    const MultistepArgs m{multistep_step_args(guidance, sqrt_a, sqrt_b, mode, 0.0f, nullptr, 0, coef_dev), cx, c0, c1, hist};
    const ApgArgs a{eta, threshold, ws, ws_floats};
    if (const int rc = check_tensors(name, {uncond, cond, x, hist, out}, nullptr, n)) return rc;
    if (const int rc = check_step(name, m.s)) return rc;
    if (const int rc = check_multistep(name, m, n)) return rc;
    if (const int rc = check_apg(name, a, n)) return rc;
    if (const int rc = check_apg_momentum(name, ApgMomentum{state, carry, carry_dev}, true)) return rc;
    IM360_CHECK_ARG(state != hist, "%s: the momentum state and the history are one buffer", name);
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((cfg_multistep_step_apg_momentum_kernel<T>), dim3(step_blocks(n / 8)), dim3(256), 0, (hipStream_t)stream,
                           (const T*)uncond, (const T*)cond, (const T*)x, (float*)hist, (float*)state, (T*)out, (long)(n / 8), guidance, sqrt_a,
                           sqrt_b, cx, c0, c1, mode, (const float*)coef_dev, (const float*)ws, (int)im360_cfg_rescale_records(n), eta,
                           threshold, carry, (const float*)carry_dev);
        return im360_launch_status();
    });
}

// im360_cfg_multistep_step_windows_apg on e, state [outer, F, inner] <- e; wrap = 0 or F
extern "C" __attribute__((visibility("default"))) int im360_cfg_multistep_step_windows_apg_momentum(const void* pred, const void* x, void* hist,
                                   void* state, void* out, const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L,
                                   int64_t inner, int64_t wrap, float guidance, float sqrt_a, float sqrt_b, float cx, float c0, float c1,
                                   int mode, float eta, float threshold, const void* ws, int64_t ws_floats, float carry,
                                   const void* carry_dev, int dtype, void* stream, const void* coef_dev) {
    using namespace im360;
    const char* name = "cfg_multistep_step_windows_apg_momentum";
    const Windows w{pred, start, weight, nW, wrap == 0 ? 0 : (int)F, outer, F, L, inner};
    const MultistepArgs m{multistep_step_args(guidance, sqrt_a, sqrt_b, mode, 0.0f, nullptr, 0, coef_dev), cx, c0, c1, hist};
    const ApgArgs a{eta, threshold, ws, ws_floats};
    if (const int rc = check_windows(name, w, x && hist && out, &m.s)) return rc;
    IM360_CHECK_ARG(wrap == 0 || wrap == F, "%s: wrap=%ld must be 0 (line) or F=%ld (ring)", name, (long)wrap, (long)F);
    IM360_CHECK_ARG(((uintptr_t)hist % 4) == 0, "%s: misaligned history", name);
    if (const int rc = check_multistep(name, m, w.elements())) return rc;
    if (const int rc = check_apg(name, a, w.elements())) return rc;
    const bool vec = (inner % 8) == 0 && (((uintptr_t)pred | (uintptr_t)x | (uintptr_t)hist | (uintptr_t)state | (uintptr_t)out) % 16) == 0;
    if (const int rc = check_apg_momentum(name, ApgMomentum{state, carry, carry_dev}, vec)) return rc;
    IM360_CHECK_ARG(state != hist, "%s: the momentum state and the history are one buffer", name);
    const long nv = (long)w.elements() / (vec ? 8 : 1);
    const int nrec = (int)im360_cfg_rescale_records(w.elements());
    return with_dtype(dtype, name, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) {
            hipLaunchKernelGGL((cfg_multistep_step_windows_apg_momentum_kernel<T, decltype(v)::value>), dim3(step_blocks(nv)), dim3(256), 0,
                               (hipStream_t)stream, (const T*)pred, (const T*)x, (float*)hist, (float*)state, (T*)out, (const int*)start,
                               (const float*)weight, nW, (long)outer, (int)F, (int)L, w.wrap, (long)inner, guidance, sqrt_a, sqrt_b, cx, c0,
                               c1, mode, (const float*)coef_dev, (const float*)ws, nrec, eta, threshold, carry, (const float*)carry_dev);
        });
        return im360_launch_status();
    });
}
