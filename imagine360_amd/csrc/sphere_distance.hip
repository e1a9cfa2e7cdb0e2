// The spherical feather of a regenerate_mask (AnimationPipeline regenerate_feather): for every pixel of an equirectangular frame the squared
// chord to the nearest KEPT pixel of that frame, measured between unit vectors of the pixel centres -- across the +-180 degree seam and
// around the poles, where a distance counted in columns means nothing.
//
//      d2[f, p] = min over q with keep[f, q] != 0 of |n_p - n_q|^2           +inf for a frame without a kept pixel
//      |n_p - n_q|^2 = fma(dz, dz, fma(dy, dy, dx * dx)),  (dx, dy, dz) = n_p - n_q         fp32, this order, through fma_f32.h
//
// From differences, not 2 - 2 dot: a chord of 1e-3 keeps its relative accuracy.  keep is uint8 [F, HW], dirs fp32 [HW, 3] (the host's
// pano_geometry.pixel_directions: fp64 trigonometry, rounded once; the kernel does none), d2 fp32 [F, HW].  The host turns d2 into an
// angle and a ramp (pano_geometry.feather_pano_mask).  Eagerly this is an HW x HW matrix per frame; here nothing is stored between.
//
// Launch: one workgroup per (frame, kSphereBlock pixels); a thread holds kSpherePixels pixels' vectors in registers.  The candidates are
// streamed through LDS in tiles of kSphereTile (x, y, z, kept) float4s; the kept flag is uniform over the workgroup, so a candidate
// that is not kept costs one LDS read and a branch every lane takes alike.  The minimum of non-negative numbers needs no order: no
// atomics, deterministic.  A setup kernel: it runs once per pipeline call.
#include "common.h"
#include "fma_f32.h"

namespace im360 {

constexpr int kSpherePixels = 2;                          // pixels per thread
constexpr int kSphereBlock = 256 * kSpherePixels;         // pixels per workgroup
constexpr int kSphereTile = 1024;                         // candidates per LDS tile (16 KiB)

__global__ __launch_bounds__(256) void sphere_distance2_kernel(const uint8_t* __restrict__ keep, const float* __restrict__ dirs,
                                                               float* __restrict__ d2, int HW, int blocks) {
    __shared__ float4 tile[kSphereTile];
    const int f = blockIdx.x / blocks, blk = blockIdx.x - f * blocks;
    const uint8_t* kf = keep + (long)f * HW;
    float px[kSpherePixels], py[kSpherePixels], pz[kSpherePixels], best[kSpherePixels];
#pragma unroll
    for (int e = 0; e < kSpherePixels; ++e) {
        const int p = min(blk * kSphereBlock + e * 256 + (int)threadIdx.x, HW - 1);      // (a lane past the end computes and stores nothing)
        px[e] = dirs[3 * (long)p];
        py[e] = dirs[3 * (long)p + 1];
        pz[e] = dirs[3 * (long)p + 2];
        best[e] = __builtin_inff();
    }
    for (int q0 = 0; q0 < HW; q0 += kSphereTile) {
        const int n = min(kSphereTile, HW - q0);
        for (int j = threadIdx.x; j < n; j += 256) {
            const long q = q0 + j;
            tile[j] = make_float4(dirs[3 * q], dirs[3 * q + 1], dirs[3 * q + 2], kf[q] ? 1.0f : 0.0f);
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float4 c = tile[j];
            if (c.w == 0.0f) continue;
#pragma unroll
            for (int e = 0; e < kSpherePixels; ++e) {
                const float dx = px[e] - c.x, dy = py[e] - c.y, dz = pz[e] - c.z;
                best[e] = fminf(best[e], fma_f32(dz, dz, fma_f32(dy, dy, dx * dx)));
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < kSpherePixels; ++e) {
        const int p = blk * kSphereBlock + e * 256 + (int)threadIdx.x;
        if (p < HW) d2[(long)f * HW + p] = best[e];
    }
}

}  // namespace im360

// keep uint8 [F, HW] (non-zero: a kept pixel), dirs fp32 [HW, 3] -> d2 fp32 [F, HW]
extern "C" __attribute__((visibility("default"))) int im360_sphere_distance2(const uint8_t* keep, const float* dirs, float* d2, int64_t F, int64_t HW,
                                                                             void* stream) {
    using namespace im360;
    IM360_CHECK_ARG(keep && dirs && d2, "sphere_distance2: null pointer");
    IM360_CHECK_ARG(F > 0 && HW > 0, "sphere_distance2: F=%ld HW=%ld must be positive", (long)F, (long)HW);
    // int32 inside the kernel: a pixel index plus one block; offsets into keep, dirs and d2 are 64-bit
    IM360_CHECK_ARG(F < ((int64_t)1 << 31) && HW + kSphereBlock < ((int64_t)1 << 31), "sphere_distance2: F=%ld or HW+%d=%ld+%d reaches 2^31", (long)F,
                    kSphereBlock, (long)HW, kSphereBlock);
    const int64_t blocks = (HW + kSphereBlock - 1) / kSphereBlock;
    // the grid: HIP refuses a launch of 2^32 threads or more, i.e. 2^24 workgroups of 256
    IM360_CHECK_ARG(F * blocks < ((int64_t)1 << 24), "sphere_distance2: F*ceil(HW/%d)=%ld*%ld reaches 2^24 workgroups (a launch holds fewer than 2^32 "
                    "threads)", kSphereBlock, (long)F, (long)blocks);
    IM360_CHECK_ARG(((uintptr_t)dirs % 4) == 0 && ((uintptr_t)d2 % 4) == 0, "sphere_distance2: misaligned dirs or d2 (4 bytes)");
    const uintptr_t o0 = (uintptr_t)d2, o1 = o0 + (uintptr_t)(4 * F * HW);
    const uintptr_t k0 = (uintptr_t)keep, k1 = k0 + (uintptr_t)(F * HW), v0 = (uintptr_t)dirs, v1 = v0 + (uintptr_t)(12 * HW);
    IM360_CHECK_ARG((o1 <= k0 || k1 <= o0) && (o1 <= v0 || v1 <= o0), "sphere_distance2: d2 overlaps keep or dirs");
    hipLaunchKernelGGL(sphere_distance2_kernel, dim3((unsigned)(F * blocks)), dim3(256), 0, (hipStream_t)stream, keep, dirs, d2, (int)HW, (int)blocks);
    return im360_launch_status();
}
