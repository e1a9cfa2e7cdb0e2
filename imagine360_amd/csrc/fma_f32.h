// An fp32 fma whose fp32 result exists before anything is converted from it.
//
// Where a kernel rounds fma(a, b, c) to fp16, hipcc may fold the fma and the conversion into one v_fma_mixlo_f16 at one site and keep
// v_fma_f32 + v_cvt_(pk_)f16_f32 at another (a loop unrolled by two took the packed pair for its body and the mixed instruction for its
// remainder), and the two do not give the same bits: a few fp16 elements in 65 538 differed in a test that compares two kernels.  Kernels whose contract is
// "the same expression gives the same bits wherever it is formed" (noise_latents.hip, keep_latents.hip) form it through this function:
// the empty asm makes the fp32 value an operand the compiler cannot look through, so every site rounds to fp32 first and converts after.
#pragma once

namespace im360 {

__device__ __forceinline__ float fma_f32(float a, float b, float c) {
    float r = __fmaf_rn(a, b, c);
    asm("" : "+v"(r));
    return r;
}

}  // namespace im360
