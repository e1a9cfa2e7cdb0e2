// Retiming a clean panorama latent (AnimationPipeline init_latents / init_video with FEWER frames than the run, init_retime): a resampling
// along the frame axis under which source frames land exactly on output frames, and which knows a looping clip is a ring of frames.
//
//      out[c, j, p] = T( sum_k wt[j][k] * x[c, frame(j, k), p] )                     fp32, one rounding, at the store
//
// x is [C, f, hw], out is [C, F, hw], F >= f (no temporal antialiasing filter: shrinking is refused).  Output frame j samples source time
// s = i0 + t, from integers:
//      open clip (loop 0): num = j (f - 1), den = max(F - 1, 1)      endpoint-aligned: frame 0 -> frame 0, frame F - 1 -> frame f - 1
//      ring      (loop 1): num = j f,       den = F                  frame F would be frame 0 again
//      i0 = num / den, t = float(num - i0 den) / float(den), one correctly rounded quotient of two integers
//      mode 0, linear: taps i0, i0 + 1, weights (1 - t, t)
//      mode 1, cubic:  taps i0 - 1 .. i0 + 2, the Keys kernel with A = -0.75 (resample_weights.h: the weights of resize_latents.hip)
//      frame = min(max(tap, 0), f - 1) for an open clip, tap mod f for a ring
// A frame with t == 0 (num divisible by den: a keyframe) is a COPY of source frame i0 -- NaNs and the sign of zero included; no weighted
// sum is formed there, and one frame is read instead of four.  Elsewhere the sum is wt[0] * a[0], then fma(wt[k], a[k], sum), through
// fma_f32.h / `opaque` like resize_latents.hip, so the two store paths give the same bits.
//
// Launch: one workgroup per (channel, output frame, tile of kRetimeTile plane elements); i0, t and the weights are uniform over the
// workgroup and computed once per thread from its block index alone.  V = 8: a unit is eight elements, one 16-byte load per tap and one
// 16-byte store (hw % 8 == 0, both pointers 16-byte aligned: every frame then starts on 16 bytes); V = 1: a unit is one element.  No
// LDS, no atomics: every element of a tap frame is read by one thread, once -- a bandwidth kernel that runs once per pipeline call.
#include "common.h"
#include "fma_f32.h"
#include "resample_weights.h"

namespace im360 {

constexpr int kRetimeTile = 4096;                // plane elements per workgroup: two 16-byte units per thread, 16 scalar ones

template <typename T, int V> __device__ __forceinline__ void retime_copy(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int n) {
    for (int u = threadIdx.x; u < n / V; u += 256) {
        if constexpr (V == 8) ((uint4*)dst)[u] = ((const uint4*)src)[u];
        else dst[u] = src[u];
    }
}

// n elements of one output frame from the NT tap frames fr[] (pointers to the tile's first element in each) with weights wt[]
template <typename T, int V, int NT>
__device__ __forceinline__ void retime_blend(const uint16_t* const* fr, const float* wt, uint16_t* __restrict__ dst, int n) {
    for (int u = threadIdx.x; u < n / V; u += 256) {
        float acc[V];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            float a[V];
            if constexpr (V == 8) {
                unpack8<T>(((const uint4*)fr[k])[u], a);
            } else {
                a[0] = to_f32(__builtin_bit_cast(T, fr[k][u]));
            }
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] = k == 0 ? opaque(wt[0] * a[e]) : fma_f32(wt[k], a[e], acc[e]);
        }
        if constexpr (V == 8) {
            ((uint4*)dst)[u] = pack8<T>(acc);
        } else {
            const T t = from_f32<T>(acc[0]);
            dst[u] = __builtin_bit_cast(uint16_t, t);
        }
    }
}

template <typename T, int V, int NT>
__device__ __forceinline__ void retime_frame(const uint16_t* __restrict__ xc, uint16_t* __restrict__ dst, int f, int hw, int e0, int n, int i0,
                                             float t, int loop) {
    float wt[NT];
    tap_weights<NT>(t, wt);
    const uint16_t* fr[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int tap = i0 + k - (NT == 4 ? 1 : 0);          // in [-1, f + 1]
        int fk;
        if (loop) {
            fk = tap % f;                                    // f may be 1
            fk = fk < 0 ? fk + f : fk;
        } else {
            fk = min(max(tap, 0), f - 1);
        }
        fr[k] = xc + (long)fk * hw + e0;
    }
    retime_blend<T, V, NT>(fr, wt, dst, n);
}

template <typename T, int V>
__global__ __launch_bounds__(256) void retime_pano_latent_kernel(const T* __restrict__ x, T* __restrict__ out, int f, int F, int hw, int tiles,
                                                                 int mode, int loop) {
    const int cj = blockIdx.x / tiles, tile = blockIdx.x - cj * tiles;
    const int c = cj / F, j = cj - c * F;
    const long den = loop ? (long)F : (long)max(F - 1, 1);
    const long num = loop ? (long)j * f : (long)j * (f - 1);
    const long i0 = num / den, rem = num - i0 * den;         // i0 <= f - 1: j <= F - 1 (open), j f < F f (ring)
    const int e0 = tile * kRetimeTile, n = min(kRetimeTile, hw - e0);
    const uint16_t* xc = (const uint16_t*)x + (long)c * f * hw;
    uint16_t* dst = (uint16_t*)out + ((long)c * F + j) * hw + e0;
    if (rem == 0) {
        retime_copy<T, V>(xc + i0 * hw + e0, dst, n);
        return;
    }
    // the quotient in fp64 and one rounding to fp32, as in resize_taps: the correctly rounded fp32 quotient whatever the fast-math flags
    // make of a division (den < 2^24 for any clip)
    const float t = opaque((float)((double)rem / (double)den));
    if (mode) retime_frame<T, V, 4>(xc, dst, f, hw, e0, n, (int)i0, t, loop);
    else retime_frame<T, V, 2>(xc, dst, f, hw, e0, n, (int)i0, t, loop);
}

}  // namespace im360

// x [C, f, hw] -> out [C, F, hw] of one 16-bit dtype; mode 0 linear, 1 cubic; loop 0 open clip, 1 ring
extern "C" __attribute__((visibility("default"))) int im360_retime_pano_latent(const void* x, void* out, int64_t C, int64_t f, int64_t F, int64_t hw,
                                        int mode, int loop, int dtype, void* stream) {
    using namespace im360;
    IM360_CHECK_ARG(x && out, "retime_pano_latent: null pointer");
    IM360_CHECK_ARG(C > 0 && f > 0 && F > 0 && hw > 0, "retime_pano_latent: C=%ld f=%ld F=%ld hw=%ld must be positive", (long)C, (long)f, (long)F,
                    (long)hw);
    // int32 inside the kernel: a frame, a (channel, frame) pair, an element index inside a plane; num, den and element offsets are 64-bit
    const int64_t lim = (int64_t)1 << 31;
    const int64_t tiles = (hw + kRetimeTile - 1) / kRetimeTile;
    IM360_CHECK_ARG(C < lim && f < lim && F < lim && hw < lim && C * F < lim && hw + kRetimeTile < lim,
                    "retime_pano_latent: f=%ld, C*F=%ld*%ld or hw+%d=%ld+%d reaches 2^31", (long)f, (long)C, (long)F, kRetimeTile, (long)hw, kRetimeTile);
    // the grid: HIP refuses a launch of 2^32 threads or more, i.e. 2^24 workgroups of 256
    IM360_CHECK_ARG(C * F * tiles < ((int64_t)1 << 24), "retime_pano_latent: C*F*ceil(hw/%d)=%ld*%ld*%ld reaches 2^24 workgroups (a launch holds "
                    "fewer than 2^32 threads)", kRetimeTile, (long)C, (long)F, (long)tiles);
    IM360_CHECK_ARG(((uintptr_t)x % 2) == 0 && ((uintptr_t)out % 2) == 0, "retime_pano_latent: misaligned 16-bit tensor");
    IM360_CHECK_ARG(x != out, "retime_pano_latent: x aliases out (the result has another frame count: there is no update in place)");
    IM360_CHECK_ARG(F >= f, "retime_pano_latent: %ld -> %ld frames shrinks (there is no temporal antialiasing filter)", (long)f, (long)F);
    IM360_CHECK_ARG(mode == 0 || mode == 1, "retime_pano_latent: mode %d unknown (0 linear, 1 cubic)", mode);
    IM360_CHECK_ARG(loop == 0 || loop == 1, "retime_pano_latent: loop %d unknown (0 open clip, 1 ring)", loop);
    const bool vec = (hw % 8) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0;
    hipStream_t s = (hipStream_t)stream;
    return with_dtype(dtype, "retime_pano_latent", [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) {
            hipLaunchKernelGGL((retime_pano_latent_kernel<T, decltype(v)::value>), dim3((unsigned)(C * F * tiles)), dim3(256), 0, s, (const T*)x,
                               (T*)out, (int)f, (int)F, (int)hw, (int)tiles, mode, loop);
        });
        IM360_CHECK_LAUNCH();
        return IM360_OK;
    });
}
