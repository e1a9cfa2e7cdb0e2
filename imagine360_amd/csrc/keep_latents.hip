// Regenerating part of a given clip (AnimationPipeline regenerate_mask): after every step of the loop both latents are blended, in
// place, with the clean clip noised to the noise level the latents now have; one launch for both branches.
//
//      known[c, f, p]   = T(sa * x0[c, f, p] + sb * noise[f, c, p])                 `noised` of latent_plane.h, one rounding
//      pano[c, f, p]    = blend(pano[c, f, p], known[c, f, p], mask[f, p])
//      pers[m, c, f, q] = ok[m, q] ? blend(pers[m, c, f, q], known[c, f, idx[m, q]], mask[f, idx[m, q]]) : pers[m, c, f, q]
//
//      blend(x, k, w):  w >= 1 -> x, bits untouched;  w <= 0 -> k, bit for bit;  else T(fma(w, x - k, k)) in fp32 (x + 1 (k - x) is not k)
//      (every fma through fma_f32.h: rounded to fp32, then converted, at every site)
//
// x0 / pano are [C, F, HW], noise is fp32 [F, C, HW], mask is fp32 [F, HW] (1: regenerate, 0: keep; one plane per frame, shared by the
// channels), pers is [M, C, F, Q], idx int32 / ok uint8 are the [M, Q] tables of pano_geometry.nearest_e2p_index.  With mask 0 and
// the same coefficients the two latents are what noise_latents_kernel writes (where ok), bit for bit: one expression, one rounding.
//
// One workgroup per (c, f) plane, as in noise_latents.hip.  `known` is never read back from pano: the plane pass forms it from x0
// and noise and (LDS path, 2 * HW bytes <= kPlaneLdsBytes) keeps the rounded plane in LDS, from which all M * Q perspective elements
// are served after one barrier; larger planes (global path) form every gathered element again from x0 and noise at idx.  Every
// element of pano and pers is read and written by one thread of one workgroup only, so the update in place has no hazard between
// workgroups.  V = 8: 16-byte lanes in both passes (HW % 8 == 0, Q % 8 == 0, every pointer aligned for its widest access; a group of
// eight that changes nothing is not stored); V = 1: scalar.  idx is clamped into [0, HW) (plane_index).
// coef (device float[2], may be null): sa, sb read by the kernel instead of the arguments (graph replay).
//
// RELEASE (AnimationPipeline regenerate_mode="release"; Differential Diffusion, arXiv 2306.00950): the mask is a per-pixel strength s and
// nothing is averaged -- an element is PINNED (`known`, bit for bit, the w <= 0 end of blend) while s <= tau and FREE (bits untouched, the
// w >= 1 end) otherwise; the compare is in fp32, tau is the host's scheduler.release_threshold of the step.  The same kernel, paths and
// stores; `free` takes the place of `w >= 1` and the select that of the fma.  coef is then float[3] = (sa, sb, tau).
#include "latent_plane.h"

namespace im360 {

// bits of blend(x, k, w); x and k as 16-bit patterns of T
template <typename T> __device__ __forceinline__ uint16_t keep_blend(uint16_t x, uint16_t k, float w) {
    if (w >= 1.0f) return x;
    if (w <= 0.0f) return k;
    const float kf = bits16_f32<T>(k);
    return bits16<T>(fma_f32(w, bits16_f32<T>(x) - kf, kf));
}

// RELEASE: is the element left alone (s > tau; a NaN strength is free) / BLEND: w >= 1
template <bool RELEASE> __device__ __forceinline__ bool keep_untouched(float w, float tau) {
    if constexpr (RELEASE) return !(w <= tau);
    else return w >= 1.0f;
}
// the element after the launch: the select of release mode, or blend
template <typename T, bool RELEASE> __device__ __forceinline__ uint16_t keep_element(uint16_t x, uint16_t k, float w, float tau) {
    if constexpr (RELEASE) return w <= tau ? k : x;
    else return keep_blend<T>(x, k, w);
}

template <typename T, int V, bool LDS, bool RELEASE>
__global__ __launch_bounds__(256) void keep_latents_kernel(T* __restrict__ pano, T* __restrict__ pers, const T* __restrict__ x0,
                                                           const float* __restrict__ noise, const float* __restrict__ mask,
                                                           const int* __restrict__ idx, const uint8_t* __restrict__ ok, int F, int C,
                                                           int HW, int M, int Q, float sa, float sb, float tau, const float* __restrict__ coef) {
    extern __shared__ __attribute__((aligned(16))) char keep_plane_smem[];
    uint16_t* plane = (uint16_t*)keep_plane_smem;             // [HW] rounded `known` of this (c, f) plane (LDS path only)
    if (coef) {
        sa = coef[0];
        sb = coef[1];
        if constexpr (RELEASE) tau = coef[2];
    }
    const int c = blockIdx.x / F, f = blockIdx.x - c * F;
    const long xb = (long)blockIdx.x * HW;                    // (c F + f) HW: x0, pano
    const T* xp = x0 + xb;
    const float* np = noise + ((long)f * C + c) * HW;         // (f C + c) HW
    const float* mp = mask + (long)f * HW;
    uint16_t* pp = (uint16_t*)(pano + xb);

    // ---- the plane
    if constexpr (V == 8) {
        for (int i = threadIdx.x; i < HW / 8; i += 256) {
            float x[8];
            unpack8<T>(((const uint4*)xp)[i], x);
            const float4 a = ((const float4*)np)[2 * i], b = ((const float4*)np)[2 * i + 1];
            const float4 wa = ((const float4*)mp)[2 * i], wb = ((const float4*)mp)[2 * i + 1];
            const float n[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            const float w[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = noised(x[e], n[e], sa, sb);
            const uint4 kv = pack8<T>(x);
            if constexpr (LDS) ((uint4*)plane)[i] = kv;
            bool all_new = true;
#pragma unroll
            for (int e = 0; e < 8; ++e) all_new = all_new && keep_untouched<RELEASE>(w[e], tau);
            if (!all_new) {
                uint16_t k[8], cur[8];
                bits16_unpack(kv, k);
                bits16_unpack(((const uint4*)pp)[i], cur);
#pragma unroll
                for (int e = 0; e < 8; ++e) cur[e] = keep_element<T, RELEASE>(cur[e], k[e], w[e], tau);
                ((uint4*)pp)[i] = bits16_pack(cur);
            }
        }
    } else {
        for (int i = threadIdx.x; i < HW; i += 256) {
            const uint16_t k = bits16<T>(noised(to_f32(xp[i]), np[i], sa, sb));
            if constexpr (LDS) plane[i] = k;
            const float w = mp[i];
            if (!keep_untouched<RELEASE>(w, tau)) pp[i] = keep_element<T, RELEASE>(pp[i], k, w, tau);
        }
    }
    if constexpr (LDS) __syncthreads();

    // ---- the M * Q elements of the plane's perspective views; one element: blended with `known` at the clamped index where the
    // view sees the panorama, unchanged elsewhere
    auto element = [&](uint16_t cur, int id, uint8_t valid) -> uint16_t {
        if (!valid) return cur;
        const unsigned p = plane_index(id, HW);
        const float w = mp[p];
        if (keep_untouched<RELEASE>(w, tau)) return cur;
        uint16_t k;
        if constexpr (LDS) k = plane[p];
        else k = bits16<T>(noised(to_f32(xp[p]), np[p], sa, sb));
        return keep_element<T, RELEASE>(cur, k, w, tau);
    };
    const long CF = (long)C * F;
    const int MQ = M * Q;
    uint16_t* vp = (uint16_t*)pers;
    if constexpr (V == 8) {
        for (int j8 = threadIdx.x; j8 < MQ / 8; j8 += 256) {
            const int j = 8 * j8, m = j / Q, q = j - m * Q;       // Q % 8 == 0: the eight elements lie in one view
            const uint2 k2 = ((const uint2*)ok)[j8];
            if ((k2.x | k2.y) == 0u) continue;
            const int4 ia = ((const int4*)idx)[2 * j8], ib = ((const int4*)idx)[2 * j8 + 1];
            const int id[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
            uint4* dst = (uint4*)(vp + ((long)m * CF + blockIdx.x) * Q + q);
            uint16_t cur[8], nxt[8];
            bits16_unpack(*dst, cur);
            bool changed = false;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                nxt[e] = element(cur[e], id[e], ok_byte(k2, e));
                changed = changed || nxt[e] != cur[e];
            }
            if (changed) *dst = bits16_pack(nxt);
        }
    } else {
        for (int j = threadIdx.x; j < MQ; j += 256) {
            if (!ok[j]) continue;
            const int m = j / Q, q = j - m * Q;
            const long o = ((long)m * CF + blockIdx.x) * Q + q;
            const uint16_t cur = vp[o], nxt = element(cur, idx[j], 1);
            if (nxt != cur) vp[o] = nxt;
        }
    }
}

// the common body of the two entry points under the caller's name `who`
template <bool RELEASE>
static int keep_launch(const char* who, void* pano, void* pers, const void* x0, const float* noise, const float* mask, const int32_t* idx,
                       const uint8_t* ok, int64_t F, int64_t C, int64_t HW, int64_t M, int64_t Q, float sqrt_a, float sqrt_b, float tau, int dtype,
                       void* stream, const void* coef_dev) {
    IM360_CHECK_ARG(pano && pers && x0 && noise && mask && idx && ok, "%s: null pointer", who);
    PlaneLaunch pl;
    if (const int rc = plane_launch(who, F, C, HW, M, Q, {x0, noise, mask, idx, pano, pers}, ok, &pl)) return rc;
    IM360_CHECK_ARG(((uintptr_t)noise % 4) == 0 && ((uintptr_t)mask % 4) == 0 && ((uintptr_t)idx % 4) == 0 && ((uintptr_t)coef_dev % 4) == 0,
                    "%s: misaligned noise, mask, idx or coef_dev (4 bytes)", who);
    IM360_CHECK_ARG(((uintptr_t)x0 % 2) == 0 && ((uintptr_t)pano % 2) == 0 && ((uintptr_t)pers % 2) == 0, "%s: misaligned 16-bit tensor", who);
    IM360_CHECK_ARG(x0 != pano, "%s: x0 aliases pano (the clean clip would be overwritten)", who);
    return with_dtype(dtype, who, [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(pl.vec ? 8 : 1, [&](auto v) { with_bool(pl.lds, [&](auto l) {
            hipLaunchKernelGGL((keep_latents_kernel<T, decltype(v)::value, decltype(l)::value, RELEASE>), dim3((unsigned)(C * F)), dim3(256), pl.smem,
                               (hipStream_t)stream, (T*)pano, (T*)pers, (const T*)x0, noise, mask, (const int*)idx, ok, (int)F, (int)C, (int)HW, (int)M,
                               (int)Q, sqrt_a, sqrt_b, tau, (const float*)coef_dev);
        }); });
        return im360_launch_status();
    });
}

}  // namespace im360

// pano / x0 [C, F, HW] and pers [M, C, F, Q] of one 16-bit dtype (pano and pers updated in place), noise fp32 [F, C, HW], mask fp32
// [F, HW], idx int32 [M, Q] with values in [0, HW) (precondition: the host cannot see the table), ok uint8 [M, Q]; coef_dev: null, or
// device float[2] = (sqrt_a, sqrt_b) read instead of the two arguments
extern "C" __attribute__((visibility("default"))) int im360_keep_latents(void* pano, void* pers, const void* x0, const float* noise, const float* mask,
                                  const int32_t* idx, const uint8_t* ok, int64_t F, int64_t C, int64_t HW, int64_t M, int64_t Q,
                                  float sqrt_a, float sqrt_b, int dtype, void* stream, const void* coef_dev) {
    return im360::keep_launch<false>("keep_latents", pano, pers, x0, noise, mask, idx, ok, F, C, HW, M, Q, sqrt_a, sqrt_b, 0.0f, dtype, stream, coef_dev);
}

// release mode: the same tensors, mask = the strength map; an element with mask <= tau is pinned to `known`, every other one keeps its
// bits; coef_dev: null, or device float[3] = (sqrt_a, sqrt_b, tau) read instead of the three arguments
extern "C" __attribute__((visibility("default"))) int im360_keep_latents_release(void* pano, void* pers, const void* x0, const float* noise,
                                  const float* mask, const int32_t* idx, const uint8_t* ok, int64_t F, int64_t C, int64_t HW, int64_t M, int64_t Q,
                                  float sqrt_a, float sqrt_b, float tau, int dtype, void* stream, const void* coef_dev) {
    return im360::keep_launch<true>("keep_latents_release", pano, pers, x0, noise, mask, idx, ok, F, C, HW, M, Q, sqrt_a, sqrt_b, tau, dtype, stream,
                                    coef_dev);
}
