// What noise_latents.hip and keep_latents.hip share: one workgroup per (c, f) plane of a [C, F, HW] latent formed from the clean clip and
// fp32 noise, its perspective elements [M, C, F, Q] taken through the [M, Q] tables idx / ok.
// The contract between the two kernels, stated here once: an element is `noised(x0, noise, sa, sb)` in fp32, rounded ONCE to the 16-bit
// type and from then on carried as its bit pattern -- through LDS, the gathers and the stores.  Both kernels, both of their paths (the
// plane kept in LDS, or formed again from global memory at the gathered index) and both lane widths call the definitions below, so the
// same inputs give the same bits wherever an element is formed: keep_latents with mask 0 writes what noise_latents writes.
#pragma once
#include <initializer_list>
#include "common.h"
#include "fma_f32.h"

namespace im360 {
constexpr int kPlaneLdsBytes = 64 * 1024;        // the plane of a 128 x 256 latent; what a workgroup gets without asking for more

// explicit fma: every place that forms an element must round alike whatever hipcc contracts or folds into the conversion (fma_f32.h)
__device__ __forceinline__ float noised(float x, float n, float sa, float sb) { return fma_f32(sa, x, sb * n); }

// a value rounded to T as its 16-bit pattern, and back
template <typename T> __device__ __forceinline__ uint16_t bits16(float v) {
    const T t = from_f32<T>(v);
    return __builtin_bit_cast(uint16_t, t);
}
template <typename T> __device__ __forceinline__ float bits16_f32(uint16_t b) { return to_f32(__builtin_bit_cast(T, b)); }
// eight patterns <-> one 16-byte lane
__device__ __forceinline__ uint4 bits16_pack(const uint16_t* g) {
    uint4 v;
    v.x = (uint32_t)g[0] | ((uint32_t)g[1] << 16);
    v.y = (uint32_t)g[2] | ((uint32_t)g[3] << 16);
    v.z = (uint32_t)g[4] | ((uint32_t)g[5] << 16);
    v.w = (uint32_t)g[6] | ((uint32_t)g[7] << 16);
    return v;
}
__device__ __forceinline__ void bits16_unpack(uint4 v, uint16_t* g) {
    g[0] = (uint16_t)v.x; g[1] = (uint16_t)(v.x >> 16);
    g[2] = (uint16_t)v.y; g[3] = (uint16_t)(v.y >> 16);
    g[4] = (uint16_t)v.z; g[5] = (uint16_t)(v.z >> 16);
    g[6] = (uint16_t)v.w; g[7] = (uint16_t)(v.w >> 16);
}
// idx clamped into [0, HW) as an unsigned value: a table that breaks the precondition gives a wrong element, never one outside the plane
__device__ __forceinline__ unsigned plane_index(int id, int HW) { return min((unsigned)id, (unsigned)(HW - 1)); }
// byte e (0 .. 7) of the eight `ok` flags a 16-byte lane loads as one uint2
__device__ __forceinline__ uint8_t ok_byte(uint2 k2, int e) { return (uint8_t)(((e < 4 ? k2.x : k2.y) >> (8 * (e & 3))) & 0xffu); }
// ---- host: the common head of the two entry points
struct PlaneLaunch {
    bool vec, lds;       // V = 8: HW % 8 == 0, Q % 8 == 0, every pointer aligned for its widest access;  the rounded plane fits kPlaneLdsBytes
    size_t smem;         // dynamic LDS of the launch
};
// Validates the sizes under the caller's name `who` (its status code) and decides the instantiation: `p16` are the pointers a V = 8
// kernel accesses 16 bytes at a time, `ok` the one it reads 8 bytes at a time.
static inline int plane_launch(const char* who, int64_t F, int64_t C, int64_t HW, int64_t M, int64_t Q, std::initializer_list<const void*> p16,
                               const void* ok, PlaneLaunch* out) {
    IM360_CHECK_ARG(F > 0 && C > 0 && HW > 0 && M > 0 && Q > 0, "%s: F=%ld C=%ld HW=%ld M=%ld Q=%ld must be positive", who, (long)F, (long)C,
                    (long)HW, (long)M, (long)Q);
    // int32 inside the kernels: a plane index (idx is int32), a gather index j < M Q, the grid C F; element offsets are 64-bit
    const int64_t lim = (int64_t)1 << 31;
    IM360_CHECK_ARG(F < lim && C < lim && M < lim && Q < lim && HW < lim && C * F < lim && M * Q < lim,
                    "%s: HW=%ld, C*F=%ld*%ld or M*Q=%ld*%ld reaches 2^31", who, (long)HW, (long)C, (long)F, (long)M, (long)Q);
    out->vec = (HW % 8) == 0 && (Q % 8) == 0 && ((uintptr_t)ok % 8) == 0;
    for (const void* p : p16) out->vec = out->vec && ((uintptr_t)p % 16) == 0;
    out->lds = 2 * HW <= kPlaneLdsBytes;
    out->smem = out->lds ? (size_t)((2 * HW + 15) / 16 * 16) : 0;
    return IM360_OK;
}

}  // namespace im360
