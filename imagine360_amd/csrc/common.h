// Shared device helpers for the gfx950 kernels of imagine360_amd.  CDNA4 only (wave64, MFMA).
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prof.h"

namespace im360 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// 16-byte register chunk as a native vector: copies of HIP's struct uint4 lower to memcpy and keep staging arrays in scratch
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---- element type traits: T is __bf16 or _Float16 (16-bit storage, fp32 math) ---------------
template <typename T> struct Elem;
template <> struct Elem<__bf16> {
    typedef bf16x8 vec8;
    static constexpr uint32_t ones2 = 0x3F803F80u;      // (1.0, 1.0)
    static __device__ __forceinline__ f32x16 mfma32(uint4 a, uint4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct Elem<_Float16> {
    typedef f16x8 vec8;
    static constexpr uint32_t ones2 = 0x3C003C00u;
    static __device__ __forceinline__ f32x16 mfma32(uint4 a, uint4 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};

// 16 x 16 MFMA tiles (fp32 accumulators, 4 per lane): lane l of the A / B operand holds row / column l & 15 and the
// 8 (x32) or 4 (x16) consecutive k elements starting at 8 * (l >> 4) / 4 * (l >> 4); C/D lane l holds column l & 15,
// rows 4 * (l >> 4) .. +3.
typedef short s16x4v __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
template <typename T> struct Mfma16;
template <> struct Mfma16<__bf16> {
    static __device__ __forceinline__ f32x4 k32(uint4 a, uint4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 k16(u32x2 a, u32x2 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4v, a), __builtin_bit_cast(s16x4v, b), c, 0, 0, 0);
    }
};
template <> struct Mfma16<_Float16> {
    static __device__ __forceinline__ f32x4 k32(uint4 a, uint4 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 k16(u32x2 a, u32x2 b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4, a), __builtin_bit_cast(f16x4, b), c, 0, 0, 0);
    }
};

// one ds_read_b64_tr_b16: within a 16-lane group, lane i receives element (i & 3) of the 8-byte chunks addressed by
// lanes (i >> 2), 4 + (i >> 2), 8 + (i >> 2), 12 + (i >> 2) -- i.e. column i of the 4 x 16 matrix whose row j is
// formed by the chunks of lanes 4j .. 4j+3 (checked on hardware by tools/tr_probe.hip)
template <typename T>
__device__ __forceinline__ u32x2 lds_read_tr16(const T* lds_ptr) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lds_ptr));
}

// c + a.lo * b.lo + a.hi * b.hi on two packed 16-bit pairs, fp32 accumulate: one v_dot2c_f32_{bf16,f16}, no unpacking
template <typename T> __device__ __forceinline__ float dot2_acc(uint32_t a, uint32_t b, float c);
template <> __device__ __forceinline__ float dot2_acc<__bf16>(uint32_t a, uint32_t b, float c) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), c, false);
}
template <> __device__ __forceinline__ float dot2_acc<_Float16>(uint32_t a, uint32_t b, float c) {
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), c, false);
}

// The value of this lane and of its partner in the other half-wave (lane ^ 32), in unspecified order -- for symmetric
// reductions (max, sum) across the two halves.  One v_permlane32_swap (VALU) instead of ds_bpermute (an LDS round trip whose
// lgkmcnt wait also drains every prefetched fragment read).  The swap exchanges lanes 32-63 of its first operand with lanes
// 0-31 of the second; fed the same value twice it leaves (x[lane & 31], x[32 + (lane & 31)]).  Issued from inline asm:
// hipcc (ROCm 7.2) drops the SECOND result of __builtin_amdgcn_permlane32_swap when both operands are copies of one value
// (seen in the ISA: max(e.x, e.y) became e.x), also through an opaque copy.  s_nop 1 = the two wait states the hardware
// needs between a VALU write of an operand and the swap.
__device__ __forceinline__ void half_wave_pair(float x, float& a, float& b) {
    uint32_t u = __builtin_bit_cast(uint32_t, x), v = u;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(u), "+v"(v));
    a = __builtin_bit_cast(float, u);
    b = __builtin_bit_cast(float, v);
}

template <typename T> __device__ __forceinline__ float to_f32(T x) { return (float)x; }
template <typename T> __device__ __forceinline__ T from_f32(float x) { return (T)x; }

// pack two fp32 into one dword of two T (lo = first element in memory)
template <typename T> __device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef T tx2 __attribute__((ext_vector_type(2)));
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, tx2));     // one v_cvt_pk_{bf16,f16}_f32
}
template <typename T> __device__ __forceinline__ float unpack_lo(uint32_t w) {
    uint16_t u = (uint16_t)(w & 0xffffu);
    return (float)__builtin_bit_cast(T, u);
}
template <typename T> __device__ __forceinline__ float unpack_hi(uint32_t w) {
    uint16_t u = (uint16_t)(w >> 16);
    return (float)__builtin_bit_cast(T, u);
}
template <typename T> __device__ __forceinline__ void unpack8(uint4 v, float* f) {
    f[0] = unpack_lo<T>(v.x); f[1] = unpack_hi<T>(v.x);
    f[2] = unpack_lo<T>(v.y); f[3] = unpack_hi<T>(v.y);
    f[4] = unpack_lo<T>(v.z); f[5] = unpack_hi<T>(v.z);
    f[6] = unpack_lo<T>(v.w); f[7] = unpack_hi<T>(v.w);
}
template <typename T> __device__ __forceinline__ uint4 pack8(const float* f) {
    uint4 v;
    v.x = pack2<T>(f[0], f[1]); v.y = pack2<T>(f[2], f[3]);
    v.z = pack2<T>(f[4], f[5]); v.w = pack2<T>(f[6], f[7]);
    return v;
}

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }

// exact-GELU x * Phi(x) with erf from Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, far below 16-bit output rounding):
// ~16 VALU instructions instead of libdevice erff's ~50, for epilogues where the activation is not hidden behind HBM
__device__ __forceinline__ float gelu_erf_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float pl = fmaf(1.061405429f, t, -1.453152027f);
    pl = fmaf(pl, t, 1.421413741f);
    pl = fmaf(pl, t, -0.284496736f);
    pl = fmaf(pl, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * z * z);
    const float erf_abs = fmaf(-pl * t, e, 1.0f);                 // erf(|x| / sqrt 2)
    return 0.5f * x + 0.5f * fabsf(x) * erf_abs;                   // x/2 * (1 + sign(x) erf(|x|/sqrt 2))
}

// Two exact-GELU values x * Phi(x) at once, for epilogues where the activation is NOT hidden behind HBM (the fused GEGLU
// GEMM spends a third of its tile time here): erf from Abramowitz & Stegun 7.1.25 (three terms, |error| <= 2.5e-5 in
// erf, <= 2e-5 relative in GELU for x > 0.05 -- 10x below fp16 output rounding), written on float2 so the plain
// multiplies / FMAs become v_pk_*_f32 (two lanes-worth per issue slot); only rcp and exp2 stay scalar.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 gelu_erf_pk(f32x2 x) {
    const f32x2 ax = {fabsf(x.x), fabsf(x.y)};
    const f32x2 den = ax * 0.33267250f + 1.0f;                    // 1 + 0.47047 |x| / sqrt 2
    const f32x2 t = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
    f32x2 pl = t * 0.7478556f + (-0.0958798f);
    pl = pl * t + 0.3480242f;
    const f32x2 q = pl * t;
    const f32x2 w = (x * x) * (-0.72134752f);                     // -x^2 / 2 in log2 units
    const f32x2 e = {__builtin_amdgcn_exp2f(w.x), __builtin_amdgcn_exp2f(w.y)};
    const f32x2 erf_abs = 1.0f - q * e;                           // erf(|x| / sqrt 2)
    return (ax * 0.5f) * erf_abs + x * 0.5f;                      // x/2 * (1 + sign(x) erf(|x| / sqrt 2))
}

// One 16-byte-per-lane LDS-DMA load issued from inline asm: `lds_dst` is the wave-uniform LDS byte address of the KiB the
// wave fills (lane-linear), `gsrc` each lane's source.  hipcc models the builtin form as a pending LDS access of unknown
// order, which turns every ds_read wait of the kernel into lgkmcnt(0); hidden in asm, fragment reads get counted waits.
// The asm loads are absent from hipcc's vmcnt bookkeeping: the kernel waits for them itself (counted vmcnt + barrier),
// and hidden loads can only make hipcc's own waits stricter (completion is in order).  M0 is compiler-reserved and not
// preserved around a statement, so it is saved and restored inside.
__device__ __forceinline__ void lds_dma16_asm(const void* gsrc, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}

// Two exact-GELU values x * Phi(x) with NO transcendental instruction, for the fused GEGLU epilogue: on a gfx950 SIMD the VALU
// work of an epilogue does not hide under the matrix pipe (tools/overlap_probe.hip: MFMA and VALU time add up, also across the
// two waves of a SIMD), and v_rcp / v_exp cost ~10 cycles each against 2 for a plain or packed VALU instruction -- the
// A&S form above is ~31 cycles per value, this one ~13.  Phi(u) - 1/2 = u Q(u^2) on u = clamp(x, -4.2, 4.2), Q of degree 8
// (least squares on Chebyshev nodes; max |error| of Phi 8.9e-6 in fp32 Horner form, checked over [-8, 8] in steps of 4e-5:
// 50x below fp16 output rounding; beyond the clamp Phi stays at Phi(4.2) = 1 - 1.3e-5 / Phi(-4.2) = 1.3e-5).  v_med3 + v_max + 10
// packed fp32 ops per pair.
__device__ __forceinline__ f32x2 gelu_poly_pk(f32x2 x) {
    const f32x2 u = {__builtin_amdgcn_fmed3f(x.x, -4.2f, 4.2f), __builtin_amdgcn_fmed3f(x.y, -4.2f, 4.2f)};
    const f32x2 t = u * u;
    f32x2 q = t * 5.768251115e-11f + (-5.461179957e-09f);
    q = q * t + 2.290590748e-07f;
    q = q * t + (-5.673924703e-06f);
    q = q * t + 9.376540910e-05f;
    q = q * t + (-1.109874304e-03f);
    q = q * t + 9.818162748e-03f;
    q = q * t + (-6.634533366e-02f);
    q = q * t + 3.989019316e-01f;
    // beyond the clamp the factor in front of Phi follows the clamp on the negative side only: x Phi(4.2) = x (1 - 1.3e-5) for
    // large x, but max(x, -4.2) Phi(-4.2) = -5.6e-5 instead of x * 1.3e-5 for very negative gates (exact GELU tends to -0 there;
    // round 3's form grew linearly: -4e-4 at x = -30)
    const f32x2 xm = {fmaxf(x.x, -4.2f), fmaxf(x.y, -4.2f)};
    return xm * (u * q + 0.5f);
}

// compile-time unrolled loop: f(std::integral_constant<int, 0>{}) ... f(<N-1>), for bodies that need the index as
// a constant expression (register arrays, immediate LDS offsets)
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// The MFMA 32x32x16 C/D fragment: lane l, register r holds C[row][col] with
//   col = l & 31,  row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5)
__device__ __forceinline__ int mfma32_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

}  // namespace im360

// status codes of the C ABI
#define IM360_OK 0
#define IM360_ERR_ARG (-1)
#define IM360_ERR_UNSUPPORTED (-2)
#define IM360_ERR_LAUNCH (-3)

// library-internal (hidden: not part of the C ABI; callers read the message through im360_last_error)
extern "C" __attribute__((visibility("hidden"))) void im360_set_error(const char* fmt, ...);
#define IM360_CHECK_ARG(cond, ...)            \
    do {                                       \
        if (!(cond)) {                         \
            im360_set_error(__VA_ARGS__);      \
            return IM360_ERR_ARG;              \
        }                                      \
    } while (0)
#define IM360_CHECK_LAUNCH()                                          \
    do {                                                              \
        hipError_t e_ = hipGetLastError();                            \
        if (e_ != hipSuccess) {                                       \
            im360_set_error("launch failed: %s", hipGetErrorString(e_)); \
            return IM360_ERR_LAUNCH;                                  \
        }                                                             \
    } while (0)
// what a launcher returns behind its launch
static inline int im360_launch_status() {
    IM360_CHECK_LAUNCH();
    return IM360_OK;
}

// ---- value -> template argument (host-side launchers): a run-time dtype / flag / small integer picks an instantiation
namespace im360 {
template <typename T> struct TypeTag { typedef T type; };
// f(TypeTag<__bf16>{}) for dtype 0, f(TypeTag<_Float16>{}) for dtype 1 (f returns the status code); anything else is the
// caller's "<who>: dtype %d unsupported"
template <typename F> static inline int with_dtype(int dtype, const char* who, F&& f) {
    if (dtype == 0) return f(TypeTag<__bf16>{});
    if (dtype == 1) return f(TypeTag<_Float16>{});
    im360_set_error("%s: dtype %d unsupported", who, dtype);
    return IM360_ERR_UNSUPPORTED;
}
// f(std::integral_constant<int, V>{}) for the one V of Vs... that equals v; false: none does, no call
template <int... Vs, typename F> static inline bool with_const(int v, F&& f) {
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}
template <typename F> static inline void with_bool(bool b, F&& f) { b ? f(std::true_type{}) : f(std::false_type{}); }
}  // namespace im360
