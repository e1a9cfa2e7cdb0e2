// FreeInit's re-noising (arXiv 2312.07537; diffusers' free_init_utils) for an equirectangular clip: the EFFECTIVE NOISE under which
// `noised(x0, n_eff)` is the low-pass of the noised clip plus the high-pass of a fresh noise, with a Gaussian low-pass that is a product
// of three dense 1-D operators -- Lw along the longitude (periodic), Lh along the latitude (mirrored at the poles), Lf along the frames
// (periodic on a looping clip, mirrored otherwise); pano_geometry.free_init_operator builds them.
//
//      d     = fma(sa, x0, fma(sb, n1, -n2))                   fp32: the noised clip minus the fresh noise
//      y     = (Lf (x) Lh (x) Lw) d                            three passes, w then h then F
//      n_eff = fma(y - d, 1 / sb, n1)                          1 / sb formed in fp64 by the host
//
// x0 is [C, F, HW] of a 16-bit type; n1, n2, n_eff are fp32 [F, C, HW]; the operators are fp32 [n, n], row i the weights of output i.
// Every dot product is ONE fp32 fma chain from acc = 0 over j = 0 .. n - 1 in this order (fma_f32.h), whatever the path, so the 16-byte
// and the scalar path give the same bits, and an identity operator gives y == d exactly: n_eff == n1 bit for bit.
//
// Three launches, no atomics, no separate elementwise launch:
//   1. free_init_rows_kernel   ws0[r, i] = sum_j Lw[i, j] d[r, j]   over the F C H rows of W contiguous elements; d is formed on the fly
//   2. free_init_cols_kernel   ws1[b, i, q] = sum_j Lh[i, j] ws0[b, j, q]     b over F C planes, q over W
//   3. free_init_cols_kernel   y[i, q] = sum_j Lf[i, j] ws1[j, q],  out = fma(y - d, 1 / sb, n1)     q over C HW; d formed again at (i, q)
// The rows kernel puts 64 rows x 64 columns of d at a time into LDS (16.3 KiB, rows padded to 65 words: lane r reads word 65 r + j, all
// banks distinct); lane = row, a wave owns kRowsTI outputs i, whose weights are wave-uniform and come through the scalar cache.  The
// cols kernels need no LDS: lane = column (coalesced), a workgroup owns kColsTI outputs i, weights again uniform.  Neither stages a
// whole plane, so no size depends on kPlaneLdsBytes.  V = 4: a unit is four elements -- 16-byte loads and stores of fp32, 8-byte loads
// of x0 -- when W % 4 == 0 and every pointer is aligned for it; V = 1 otherwise.  Any F, H, W >= 1.
#include "common.h"
#include "fma_f32.h"

namespace im360 {

constexpr int kRowsTile = 64;        // rows per workgroup of the rows kernel (one per lane) and columns of d per LDS fill
constexpr int kRowsPad = kRowsTile + 1;
constexpr int kRowsTI = 8;           // outputs per wave in the rows kernel; a workgroup of four waves owns 32
constexpr int kColsTI = 4;           // outputs per thread in the cols kernels

// the one definition of d and of the result; both kernels and both lane widths call these
__device__ __forceinline__ float free_init_d(float x, float a, float b, float sa, float sb) { return fma_f32(sa, x, fma_f32(sb, a, -b)); }
__device__ __forceinline__ float free_init_out(float y, float d, float a, float inv_sb) {
    float r = y - d;
    asm("" : "+v"(r));
    return fma_f32(r, inv_sb, a);
}

template <typename T> __device__ __forceinline__ float load16(const uint16_t* p) { return to_f32(__builtin_bit_cast(T, *p)); }
template <typename T> __device__ __forceinline__ void load16x4(const uint16_t* p, float* f) {
    const uint2 v = *(const uint2*)p;
    f[0] = unpack_lo<T>(v.x); f[1] = unpack_hi<T>(v.x);
    f[2] = unpack_lo<T>(v.y); f[3] = unpack_hi<T>(v.y);
}

// ws[r, i] = sum_j L[i, j] d[r, j]; r = (f C + c) H + y over R = F C H rows, n1 / n2 / ws at r W, x0 at ((c F + f) H + y) W
template <typename T, int V>
__global__ __launch_bounds__(256) void free_init_rows_kernel(const uint16_t* __restrict__ x0, const float* __restrict__ n1,
                                                             const float* __restrict__ n2, const float* __restrict__ L,
                                                             float* __restrict__ ws, int C, int F, int H, int W, int R, int itiles, float sa,
                                                             float sb) {
    __shared__ float xs[kRowsTile * kRowsPad];
    const int rb = blockIdx.x / itiles, it = blockIdx.x - rb * itiles;
    const int r0 = rb * kRowsTile;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int i0 = (it * 4 + wave) * kRowsTI;
    const float* Lr[kRowsTI];
#pragma unroll
    for (int t = 0; t < kRowsTI; ++t) Lr[t] = L + (long)min(i0 + t, W - 1) * W;       // a row past the end repeats the last: loaded, never stored
    float acc[kRowsTI];
#pragma unroll
    for (int t = 0; t < kRowsTI; ++t) acc[t] = 0.0f;
    for (int j0 = 0; j0 < W; j0 += kRowsTile) {
        __syncthreads();
        for (int u = threadIdx.x; u < kRowsTile * kRowsTile / V; u += 256) {
            const int rr = u / (kRowsTile / V), jj = (u - rr * (kRowsTile / V)) * V;
            const int r = r0 + rr, j = j0 + jj;
            float d[V];
#pragma unroll
            for (int e = 0; e < V; ++e) d[e] = 0.0f;
            if (r < R && j < W) {                                   // V = 4: W % 4 == 0, a unit is inside the row or outside it
                const int fc = r / H, y = r - fc * H, f = fc / C, c = fc - f * C;
                const long on = (long)r * W + j, ox = (((long)c * F + f) * H + y) * W + j;
                if constexpr (V == 4) {
                    float x[4];
                    load16x4<T>(x0 + ox, x);
                    const float4 a = *(const float4*)(n1 + on), b = *(const float4*)(n2 + on);
                    d[0] = free_init_d(x[0], a.x, b.x, sa, sb);
                    d[1] = free_init_d(x[1], a.y, b.y, sa, sb);
                    d[2] = free_init_d(x[2], a.z, b.z, sa, sb);
                    d[3] = free_init_d(x[3], a.w, b.w, sa, sb);
                } else {
                    d[0] = free_init_d(load16<T>(x0 + ox), n1[on], n2[on], sa, sb);
                }
            }
#pragma unroll
            for (int e = 0; e < V; ++e) xs[rr * kRowsPad + jj + e] = d[e];
        }
        __syncthreads();
        const int nj = min(kRowsTile, W - j0);
        for (int jj = 0; jj < nj; ++jj) {
            const float x = xs[lane * kRowsPad + jj];
#pragma unroll
            for (int t = 0; t < kRowsTI; ++t) acc[t] = fma_f32(Lr[t][j0 + jj], x, acc[t]);
        }
    }
    const int r = r0 + lane;
    if (r >= R) return;
    float* dst = ws + (long)r * W + i0;
    if constexpr (V == 4) {
#pragma unroll
        for (int t = 0; t < kRowsTI; t += 4)
            if (i0 + t < W) *(float4*)(dst + t) = make_float4(acc[t], acc[t + 1], acc[t + 2], acc[t + 3]);
    } else {
#pragma unroll
        for (int t = 0; t < kRowsTI; ++t)
            if (i0 + t < W) dst[t] = acc[t];
    }
}

// y[b, i, q] = sum_j L[i, j] src[b, j, q] over B blocks of [n, Q]; a thread owns one unit of V columns and kColsTI outputs i.
// EPI (B == 1, n == F, Q == C HW): dst[i, q] = fma(y - d, inv_sb, n1[i, q]) with d formed again from x0 at ((c F + i) HW + p), q = c HW + p.
template <typename T, int V, bool EPI>
__global__ __launch_bounds__(256) void free_init_cols_kernel(const float* __restrict__ src, const float* __restrict__ L, float* __restrict__ dst,
                                                             long units, int n, int Q, int ublocks, const uint16_t* __restrict__ x0,
                                                             const float* __restrict__ n1, const float* __restrict__ n2, int HW, float sa,
                                                             float sb, float inv_sb) {
    const int it = blockIdx.x / ublocks, ub = blockIdx.x - it * ublocks;
    const long u = (long)ub * 256 + threadIdx.x;
    if (u >= units) return;
    const int qu = Q / V;                                        // units per row of Q
    const long b = u / qu;
    const int q = (int)(u - b * qu) * V;
    const int i0 = it * kColsTI;
    const float* Lr[kColsTI];
#pragma unroll
    for (int t = 0; t < kColsTI; ++t) Lr[t] = L + (long)min(i0 + t, n - 1) * n;     // a row past the end repeats the last: loaded, never stored
    float acc[kColsTI][V];
#pragma unroll
    for (int t = 0; t < kColsTI; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[t][e] = 0.0f;
    const float* col = src + b * n * Q + q;
    for (int j = 0; j < n; ++j) {
        float x[V];
        if constexpr (V == 4) {
            const float4 v = *(const float4*)(col + (long)j * Q);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
            x[0] = col[(long)j * Q];
        }
#pragma unroll
        for (int t = 0; t < kColsTI; ++t)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[t][e] = fma_f32(Lr[t][j], x[e], acc[t][e]);
    }
#pragma unroll
    for (int t = 0; t < kColsTI; ++t) {
        const int i = i0 + t;
        if (i >= n) break;
        const long o = (b * n + i) * Q + q;
        float r[V];
        if constexpr (EPI) {
            const int c = q / HW, p = q - c * HW;                 // V = 4: HW % 4 == 0, a unit stays inside one channel
            const long ox = ((long)c * n + i) * HW + p;
            if constexpr (V == 4) {
                float x[4];
                load16x4<T>(x0 + ox, x);
                const float4 a = *(const float4*)(n1 + o), bb = *(const float4*)(n2 + o);
                r[0] = free_init_out(acc[t][0], free_init_d(x[0], a.x, bb.x, sa, sb), a.x, inv_sb);
                r[1] = free_init_out(acc[t][1], free_init_d(x[1], a.y, bb.y, sa, sb), a.y, inv_sb);
                r[2] = free_init_out(acc[t][2], free_init_d(x[2], a.z, bb.z, sa, sb), a.z, inv_sb);
                r[3] = free_init_out(acc[t][3], free_init_d(x[3], a.w, bb.w, sa, sb), a.w, inv_sb);
            } else {
                const float a = n1[o];
                r[0] = free_init_out(acc[t][0], free_init_d(load16<T>(x0 + ox), a, n2[o], sa, sb), a, inv_sb);
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) r[e] = acc[t][e];
        }
        if constexpr (V == 4) *(float4*)(dst + o) = make_float4(r[0], r[1], r[2], r[3]);
        else dst[o] = r[0];
    }
}

}  // namespace im360

// x0 [C, F, H W] 16-bit; n1, n2, out fp32 [F, C, H W]; Lf [F, F], Lh [H, H], Lw [W, W] fp32; ws fp32, ws_elems >= 2 F C H W
extern "C" __attribute__((visibility("default"))) int im360_free_init_noise(const void* x0, const float* n1, const float* n2, const float* Lf,
                                     const float* Lh, const float* Lw, float* out, float* ws, int64_t ws_elems, int64_t C, int64_t F,
                                     int64_t H, int64_t W, float sa, float sb, float inv_sb, int dtype, void* stream) {
    using namespace im360;
    IM360_CHECK_ARG(x0 && n1 && n2 && Lf && Lh && Lw && out && ws, "free_init_noise: null pointer");
    IM360_CHECK_ARG(C > 0 && F > 0 && H > 0 && W > 0, "free_init_noise: C=%ld F=%ld H=%ld W=%ld must be positive", (long)C, (long)F, (long)H,
                    (long)W);
    // int32 inside the kernels: a row (up to one tile past the last), a column, an output index, a workgroup index; element offsets are 64-bit
    const int64_t lim = (int64_t)1 << 31;
    IM360_CHECK_ARG(C < lim && F < lim && H < lim && W < lim && (C * F < lim) && (C * F * H < lim) &&
                    (C * F * H * W + kRowsTile < lim), "free_init_noise: C*F*H*W+%d=%ld*%ld*%ld*%ld+%d reaches 2^31", kRowsTile, (long)C, (long)F,
                    (long)H, (long)W, kRowsTile);
    const int64_t N = C * F * H * W, R = C * F * H, HW = H * W;
    IM360_CHECK_ARG(ws_elems >= 2 * N, "free_init_noise: the workspace holds %ld fp32 elements, 2*C*F*H*W=%ld are needed", (long)ws_elems,
                    (long)(2 * N));
    IM360_CHECK_ARG(sb > 0.0f && inv_sb > 0.0f, "free_init_noise: sb=%g and 1/sb=%g must be positive (pure signal has no noise to replace)",
                    (double)sb, (double)inv_sb);
    IM360_CHECK_ARG(((uintptr_t)x0 % 2) == 0, "free_init_noise: misaligned 16-bit tensor");
    for (const void* p : {(const void*)n1, (const void*)n2, (const void*)Lf, (const void*)Lh, (const void*)Lw, (const void*)out, (const void*)ws})
        IM360_CHECK_ARG(((uintptr_t)p % 4) == 0, "free_init_noise: misaligned fp32 tensor");
    // workgroups per launch: HIP refuses a launch of 2^32 threads or more, i.e. 2^24 workgroups of 256
    const int64_t itiles_w = (W + 4 * kRowsTI - 1) / (4 * kRowsTI), g1 = (R + kRowsTile - 1) / kRowsTile * itiles_w;
    bool vec = (W % 4) == 0 && ((uintptr_t)x0 % 8) == 0;
    for (const void* p : {(const void*)n1, (const void*)n2, (const void*)out, (const void*)ws}) vec = vec && ((uintptr_t)p % 16) == 0;
    const int V = vec ? 4 : 1;
    // columns of the two cols launches: F C planes of W columns each, then one block of C H W columns
    const int64_t units2 = C * F * W / V, ub2 = (units2 + 255) / 256, units3 = C * HW / V, ub3 = (units3 + 255) / 256;
    const int64_t g2 = (H + kColsTI - 1) / kColsTI * ub2, g3 = (F + kColsTI - 1) / kColsTI * ub3;
    const int64_t gl = (int64_t)1 << 24;
    IM360_CHECK_ARG(g1 < gl && g2 < gl && g3 < gl, "free_init_noise: %ld, %ld or %ld workgroups reach 2^24 (a launch holds fewer than 2^32 threads)",
                    (long)g1, (long)g2, (long)g3);
    // the workspace halves are read across whole rows and columns while other workgroups write, and x0, n1, n2 are read again by the
    // last launch: neither the workspace nor the result may overlap anything else
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 4 * (uintptr_t)N, w0 = (uintptr_t)ws, w1 = w0 + 8 * (uintptr_t)N;
    IM360_CHECK_ARG(o1 <= w0 || w1 <= o0, "free_init_noise: out overlaps the workspace");
    for (const void* p : {(const void*)n1, (const void*)n2}) {
        const uintptr_t a0 = (uintptr_t)p, a1 = a0 + 4 * (uintptr_t)N;
        IM360_CHECK_ARG((a1 <= o0 || o1 <= a0) && (a1 <= w0 || w1 <= a0), "free_init_noise: n1 or n2 overlaps out or the workspace");
    }
    {
        const uintptr_t a0 = (uintptr_t)x0, a1 = a0 + 2 * (uintptr_t)N;
        IM360_CHECK_ARG((a1 <= o0 || o1 <= a0) && (a1 <= w0 || w1 <= a0), "free_init_noise: x0 overlaps out or the workspace");
    }
    float* ws0 = ws;
    float* ws1 = ws + N;
    hipStream_t s = (hipStream_t)stream;
    return with_dtype(dtype, "free_init_noise", [&](auto t) {
        using T = typename decltype(t)::type;
        const uint16_t* x = (const uint16_t*)x0;
        with_const<1, 4>(V, [&](auto v) {
            constexpr int VV = decltype(v)::value;
            hipLaunchKernelGGL((free_init_rows_kernel<T, VV>), dim3((unsigned)g1), dim3(256), 0, s, x, n1, n2, Lw, ws0, (int)C, (int)F, (int)H,
                               (int)W, (int)R, (int)itiles_w, sa, sb);
            hipLaunchKernelGGL((free_init_cols_kernel<T, VV, false>), dim3((unsigned)g2), dim3(256), 0, s, (const float*)ws0, Lh, ws1, (long)units2,
                               (int)H, (int)W, (int)ub2, x, n1, n2, (int)HW, sa, sb, inv_sb);
            hipLaunchKernelGGL((free_init_cols_kernel<T, VV, true>), dim3((unsigned)g3), dim3(256), 0, s, (const float*)ws1, Lf, out, (long)units3,
                               (int)F, (int)(C * HW), (int)ub3, x, n1, n2, (int)HW, sa, sb, inv_sb);
        });
        IM360_CHECK_LAUNCH();
        return IM360_OK;
    });
}
