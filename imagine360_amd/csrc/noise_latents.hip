// Start latents of a run that begins from a given clip (AnimationPipeline init_latents / strength): the clean panorama latent noised
// to the first timestep of the shortened schedule, and the perspective start latent as its nearest-neighbour E2P resampling, one launch.
//
//      out_pano[c, f, p]    = T(sa * x0[c, f, p] + sb * noise[f, c, p])             fp32, one rounding, at the store
//      out_pers[m, c, f, q] = ok[m, q] ? out_pano[c, f, idx[m, q]] : 0              the ROUNDED panorama value, bit for bit
//
// x0 / out_pano are [C, F, HW] (the pipeline's [1, 4, F, h, w]), noise is fp32 [F, C, HW] (the layout init_noise draws in), out_pers is
// [M, C, F, Q] (the perspective latent's [1, m, 4, F, h, w]), idx int32 / ok uint8 are the [M, Q] tables of
// pano_geometry.nearest_e2p_index.  The perspective start is the gather of the rounded panorama start and not a second rounding of
// the fp32 sum so that both branches begin from the same numbers, exactly as init_noise derives the perspective noise from the
// panorama noise; a pixel seen by two views, or by a view and the panorama, has one value.
//
// One workgroup per (c, f) plane.  LDS path (2 * HW bytes <= kPlaneLdsBytes): the plane is formed once, written to out_pano and kept
// in LDS as 16-bit values; after one barrier all M * Q gathers of the plane are served from LDS.  Global path (larger planes): the
// plane is formed and stored, then every gathered element is formed again from x0 and noise at idx -- the same `noised` expression on
// the same inputs, hence the same bits as out_pano -- so no workgroup reads what another one (or it itself) has just written.
// V = 8: 16-byte lanes in both phases (HW % 8 == 0, Q % 8 == 0, every pointer aligned for its widest access); V = 1: scalar.
// idx is clamped into [0, HW) (plane_index).  `noised`, the 16-bit patterns and the contract with keep_latents.hip: latent_plane.h.
#include "latent_plane.h"

namespace im360 {

template <typename T, int V, bool LDS>
__global__ __launch_bounds__(256) void noise_latents_kernel(const T* __restrict__ x0, const float* __restrict__ noise,
                                                            const int* __restrict__ idx, const uint8_t* __restrict__ ok,
                                                            T* __restrict__ out_pano, T* __restrict__ out_pers, int F, int C, int HW,
                                                            int M, int Q, float sa, float sb) {
    extern __shared__ __attribute__((aligned(16))) char noise_plane_smem[];
    uint16_t* plane = (uint16_t*)noise_plane_smem;            // [HW] rounded values of this (c, f) plane (LDS path only)
    const int c = blockIdx.x / F, f = blockIdx.x - c * F;
    const long xb = (long)blockIdx.x * HW;                    // (c F + f) HW: x0, out_pano
    const long nb = ((long)f * C + c) * HW;                   // (f C + c) HW: noise
    const T* xp = x0 + xb;
    const float* np = noise + nb;
    T* op = out_pano + xb;

    // ---- the plane
    if constexpr (V == 8) {
        for (int i = threadIdx.x; i < HW / 8; i += 256) {
            float x[8];
            unpack8<T>(((const uint4*)xp)[i], x);
            const float4 a = ((const float4*)np)[2 * i], b = ((const float4*)np)[2 * i + 1];
            const float n[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = noised(x[e], n[e], sa, sb);
            const uint4 v = pack8<T>(x);
            ((uint4*)op)[i] = v;
            if constexpr (LDS) ((uint4*)plane)[i] = v;
        }
    } else {
        for (int i = threadIdx.x; i < HW; i += 256) {
            const uint16_t v = bits16<T>(noised(to_f32(xp[i]), np[i], sa, sb));
            ((uint16_t*)op)[i] = v;
            if constexpr (LDS) plane[i] = v;
        }
    }
    if constexpr (LDS) __syncthreads();

    // ---- the M * Q gathers of the plane; one element: rounded plane value at the clamped index, or 0 where the view sees nothing
    auto gather = [&](int id, uint8_t valid) -> uint16_t {
        const unsigned p = plane_index(id, HW);
        uint16_t v;
        if constexpr (LDS) v = plane[p];
        else v = bits16<T>(noised(to_f32(xp[p]), np[p], sa, sb));
        return valid ? v : (uint16_t)0;
    };
    const long CF = (long)C * F;
    const int MQ = M * Q;
    if constexpr (V == 8) {
        for (int j8 = threadIdx.x; j8 < MQ / 8; j8 += 256) {
            const int j = 8 * j8, m = j / Q, q = j - m * Q;       // Q % 8 == 0: the eight elements lie in one view
            const int4 ia = ((const int4*)idx)[2 * j8], ib = ((const int4*)idx)[2 * j8 + 1];
            const uint2 k2 = ((const uint2*)ok)[j8];
            const int id[8] = {ia.x, ia.y, ia.z, ia.w, ib.x, ib.y, ib.z, ib.w};
            uint16_t g[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] = gather(id[e], ok_byte(k2, e));
            // bits16_pack(g), kept written out: behind the call hipcc packs with shift + or instead of v_perm_b32 and moves the gather's v_cvt
            const uint4 v = {(uint32_t)g[0] | ((uint32_t)g[1] << 16), (uint32_t)g[2] | ((uint32_t)g[3] << 16),
                             (uint32_t)g[4] | ((uint32_t)g[5] << 16), (uint32_t)g[6] | ((uint32_t)g[7] << 16)};
            *(uint4*)(out_pers + ((long)m * CF + blockIdx.x) * Q + q) = v;
        }
    } else {
        for (int j = threadIdx.x; j < MQ; j += 256) {
            const int m = j / Q, q = j - m * Q;
            ((uint16_t*)out_pers)[((long)m * CF + blockIdx.x) * Q + q] = gather(idx[j], ok[j]);
        }
    }
}

}  // namespace im360

// x0 / out_pano [C, F, HW] and out_pers [M, C, F, Q] of one 16-bit dtype, noise fp32 [F, C, HW], idx int32 [M, Q] with values in
// [0, HW) (precondition: the host cannot see the table), ok uint8 [M, Q]
extern "C" __attribute__((visibility("default"))) int im360_noise_latents(const void* x0, const float* noise, const int32_t* idx, const uint8_t* ok,
                                   void* out_pano, void* out_pers, int64_t F, int64_t C, int64_t HW, int64_t M, int64_t Q,
                                   float sqrt_a, float sqrt_b, int dtype, void* stream) {
    using namespace im360;
    IM360_CHECK_ARG(x0 && noise && idx && ok && out_pano && out_pers, "noise_latents: null pointer");
    PlaneLaunch pl;
    if (const int rc = plane_launch("noise_latents", F, C, HW, M, Q, {x0, noise, idx, out_pano, out_pers}, ok, &pl)) return rc;
    IM360_CHECK_ARG(((uintptr_t)noise % 4) == 0 && ((uintptr_t)idx % 4) == 0, "noise_latents: misaligned noise or idx (4 bytes)");
    IM360_CHECK_ARG(((uintptr_t)x0 % 2) == 0 && ((uintptr_t)out_pano % 2) == 0 && ((uintptr_t)out_pers % 2) == 0,
                    "noise_latents: misaligned 16-bit tensor");
    return with_dtype(dtype, "noise_latents", [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(pl.vec ? 8 : 1, [&](auto v) { with_bool(pl.lds, [&](auto l) {
            hipLaunchKernelGGL((noise_latents_kernel<T, decltype(v)::value, decltype(l)::value>), dim3((unsigned)(C * F)), dim3(256), pl.smem, (hipStream_t)stream,
                               (const T*)x0, noise, (const int*)idx, ok, (T*)out_pano, (T*)out_pers, (int)F, (int)C, (int)HW, (int)M, (int)Q,
                               sqrt_a, sqrt_b);
        }); });
        return im360_launch_status();
    });
}
