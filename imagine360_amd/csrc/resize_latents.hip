// Upscaling a clean panorama latent (AnimationPipeline init_latents / init_video at a lower resolution than the run, init_resize): a
// resampling that knows the image is equirectangular -- longitude wraps, latitude clamps -- so no seam appears at +-180 degrees.
//
//      out[p, Y, X] = T( sum_r wy[Y][r] * ( sum_j wx[X][j] * x[p, row(Y, r), col(X, j)] ) )          fp32, horizontal pass then vertical, one
//                                                                                                   rounding, at the store
//
// x is [P, h, w], out is [P, H, W] (P = C * F planes of the pipeline's [1, C, F, ., .] latent), H >= h and W >= w (no antialiasing
// filter: shrinking is refused).  Half-pixel centres (align_corners=False), from integers: output column X samples
// s = ((2 X + 1) w - W) / (2 W); num = (2 X + 1) w - W, i0 = floor(num / 2 W), t = float(num - i0 * 2 W) / float(2 W), one correctly rounded
// quotient of two integers -- no float coordinate accumulates, and t is exactly periodic in X for every integer scale.  Rows alike.
//      mode 0, bilinear: taps i0, i0 + 1, weights (1 - t, t)
//      mode 1, bicubic:  taps i0 - 1 .. i0 + 2, the Keys kernel with A = -0.75 in the polynomial forms of torch's upsample_bicubic2d
//      col = tap mod w (wrap), row = min(max(tap, 0), h - 1) (clamp); a clamped row is read and weighted again, never skipped
// A sum is w[0] * a[0], then fma(w[k], a[k], sum) for k = 1 ..; every fma and every step of the weight polynomials goes through
// fma_f32.h / `opaque`, so that no site is contracted, reassociated or folded into the conversion differently from another: the two
// paths of the launcher, and a column and its image under a roll of the input by whole columns, give the same bits.
//
// Launch: one workgroup per (plane, tile of kResizeRows output rows) -- 64 planes alone would leave three quarters of the chip idle
// at 128 x 256 -- whose threads walk the tile's units row by row.  V = 8: a unit is eight output columns and one 16-byte store (W % 8
// == 0, both pointers 16-byte aligned); V = 1: a unit is one element.  Source rows are read directly from global memory with 2-byte
// loads: an input plane is at most 64 KiB at the sizes of the pipeline and stays in the caches, the taps of neighbouring lanes fall
// into the same lines, and the launch runs once per pipeline call; no LDS staging.
#include "common.h"
#include "fma_f32.h"
#include "resample_weights.h"

namespace im360 {

constexpr int kResizeRows = 8;                   // output rows per workgroup: 32 units per row at W = 256, V = 8 -> 256 threads busy

// NT = 2 (bilinear) / 4 (bicubic) taps of output index o along an axis of n_in -> n_out samples: the first tap (unwrapped, unclamped)
// and the weights
template <int NT> __device__ __forceinline__ int resize_taps(int o, int n_in, int n_out, float* wt) {
    const long den = 2L * n_out;
    const long num = (2L * o + 1) * n_in - n_out;            // >= n_in - n_out > -den: i0 >= -1
    const long i0 = num >= 0 ? num / den : -1;
    // the quotient in fp64 and one rounding to fp32: the correctly rounded fp32 quotient whatever the fast-math flags make of a
    // division (for 2 n_out < 2^24, any latent: both integers are exact in fp32 and the fp64 quotient is never within its own error
    // of an fp32 tie; beyond that t may be one fp32 ulp off, still the same value at every site)
    const float t = opaque((float)((double)(num - i0 * den) / (double)den));
    tap_weights<NT>(t, wt);                                  // (resample_weights.h, shared with retime_latents.hip)
    return NT == 2 ? (int)i0 : (int)i0 - 1;
}

template <typename T> __device__ __forceinline__ float resize_load(const uint16_t* p) { return to_f32(__builtin_bit_cast(T, *p)); }

// one output element: rows r[], row weights wy[], the first column tap c0 (unwrapped) and column weights wx[]
template <typename T, int NT>
__device__ __forceinline__ float resize_element(const uint16_t* __restrict__ xp, int w, const int* r, const float* wy, int c0, const float* wx) {
    int c[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        int v = (c0 + j) % w;                                // c0 + j in [-2, w + 1]; w may be 1
        c[j] = v < 0 ? v + w : v;
    }
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const uint16_t* row = xp + (long)r[k] * w;
        float hsum = opaque(wx[0] * resize_load<T>(row + c[0]));
#pragma unroll
        for (int j = 1; j < NT; ++j) hsum = fma_f32(wx[j], resize_load<T>(row + c[j]), hsum);
        acc = k == 0 ? opaque(wy[0] * hsum) : fma_f32(wy[k], hsum, acc);
    }
    return acc;
}

template <typename T, int V, int NT>
__device__ __forceinline__ void resize_tile(const uint16_t* __restrict__ xp, uint16_t* __restrict__ op, int h, int w, int H, int W, int row0) {
    const int rows = min(kResizeRows, H - row0);
    const int upr = W / V;                                   // units per output row
    for (int u = threadIdx.x; u < rows * upr; u += 256) {
        const int ry = u / upr, Y = row0 + ry, X0 = (u - ry * upr) * V;
        float wy[NT];
        int r[NT];
        const int r0 = resize_taps<NT>(Y, h, H, wy);
#pragma unroll
        for (int k = 0; k < NT; ++k) r[k] = min(max(r0 + k, 0), h - 1);
        float res[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float wx[NT];
            const int c0 = resize_taps<NT>(X0 + e, w, W, wx);
            res[e] = resize_element<T, NT>(xp, w, r, wy, c0, wx);
        }
        uint16_t* dst = op + (long)Y * W + X0;
        if constexpr (V == 8) {
            *(uint4*)dst = pack8<T>(res);
        } else {
            const T t = from_f32<T>(res[0]);
            *dst = __builtin_bit_cast(uint16_t, t);
        }
    }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void resize_pano_latent_kernel(const T* __restrict__ x, T* __restrict__ out, int h, int w, int H, int W,
                                                                 int tiles, int mode) {
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const uint16_t* xp = (const uint16_t*)x + (long)plane * h * w;
    uint16_t* op = (uint16_t*)out + (long)plane * H * W;
    if (mode) resize_tile<T, V, 4>(xp, op, h, w, H, W, tile * kResizeRows);
    else resize_tile<T, V, 2>(xp, op, h, w, H, W, tile * kResizeRows);
}

}  // namespace im360

// x [C, F, h, w] -> out [C, F, H, W] of one 16-bit dtype; mode 0 bilinear, 1 bicubic
extern "C" __attribute__((visibility("default"))) int im360_resize_pano_latent(const void* x, void* out, int64_t C, int64_t F, int64_t h, int64_t w,
                                        int64_t H, int64_t W, int mode, int dtype, void* stream) {
    using namespace im360;
    IM360_CHECK_ARG(x && out, "resize_pano_latent: null pointer");
    IM360_CHECK_ARG(C > 0 && F > 0 && h > 0 && w > 0 && H > 0 && W > 0, "resize_pano_latent: C=%ld F=%ld h=%ld w=%ld H=%ld W=%ld must be positive",
                    (long)C, (long)F, (long)h, (long)w, (long)H, (long)W);
    // int32 inside the kernel: a row or column, an index inside a tile; coordinates and element offsets are 64-bit
    const int64_t lim = (int64_t)1 << 31;
    const int64_t tiles = (H + kResizeRows - 1) / kResizeRows;
    IM360_CHECK_ARG(C < lim && F < lim && h < lim && w < lim && H < lim && W < lim && C * F < lim && kResizeRows * W + 256 < lim,
                    "resize_pano_latent: h=%ld, w=%ld, H=%ld, C*F=%ld*%ld or %d*W=%d*%ld reaches 2^31", (long)h, (long)w, (long)H, (long)C,
                    (long)F, kResizeRows, kResizeRows, (long)W);
    // the grid: HIP refuses a launch of 2^32 threads or more, i.e. 2^24 workgroups of 256
    IM360_CHECK_ARG(C * F * tiles < ((int64_t)1 << 24), "resize_pano_latent: C*F*ceil(H/%d)=%ld*%ld*%ld reaches 2^24 workgroups (a launch holds fewer "
                    "than 2^32 threads)", kResizeRows, (long)C, (long)F, (long)tiles);
    IM360_CHECK_ARG(((uintptr_t)x % 2) == 0 && ((uintptr_t)out % 2) == 0, "resize_pano_latent: misaligned 16-bit tensor");
    IM360_CHECK_ARG(x != out, "resize_pano_latent: x aliases out (the result has another size: there is no update in place)");
    IM360_CHECK_ARG(H >= h && W >= w, "resize_pano_latent: %ldx%ld -> %ldx%ld shrinks (there is no antialiasing filter)", (long)h, (long)w,
                    (long)H, (long)W);
    IM360_CHECK_ARG(mode == 0 || mode == 1, "resize_pano_latent: mode %d unknown (0 bilinear, 1 bicubic)", mode);
    const bool vec = (W % 8) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0;
    hipStream_t s = (hipStream_t)stream;
    return with_dtype(dtype, "resize_pano_latent", [&](auto t) {
        using T = typename decltype(t)::type;
        with_const<1, 8>(vec ? 8 : 1, [&](auto v) {
            hipLaunchKernelGGL((resize_pano_latent_kernel<T, decltype(v)::value>), dim3((unsigned)(C * F * tiles)), dim3(256), 0, s, (const T*)x,
                               (T*)out, (int)h, (int)w, (int)H, (int)W, (int)tiles, mode);
        });
        IM360_CHECK_LAUNCH();
        return IM360_OK;
    });
}
