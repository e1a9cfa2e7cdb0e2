// What resize_latents.hip and retime_latents.hip share: the weights of the 2 (linear) or 4 (cubic) taps of a sample at fraction t in [0, 1)
// behind its first tap.  Every product and fma goes through fma_f32.h / `opaque`, so that no site is contracted, reassociated or folded
// into a conversion differently from another: the same t gives the same weights, and the same taps the same bits, wherever they are formed.
#pragma once
#include "fma_f32.h"

namespace im360 {

// a value the compiler cannot look through: what is computed from it is not merged with how it was computed
__device__ __forceinline__ float opaque(float v) {
    asm("" : "+v"(v));
    return v;
}

// torch's cubic_convolution1 (|x| <= 1) and cubic_convolution2 (1 < |x| < 2) with A = -0.75
__device__ __forceinline__ float keys_near(float x) { return fma_f32(opaque(fma_f32(1.25f, x, -2.25f) * x), x, 1.0f); }
__device__ __forceinline__ float keys_far(float x) { return fma_f32(fma_f32(fma_f32(-0.75f, x, 3.75f), x, -6.0f), x, 3.0f); }

// NT = 2: taps i0, i0 + 1, weights (1 - t, t);  NT = 4: taps i0 - 1 .. i0 + 2, the Keys kernel.  t is opaque already.
template <int NT> __device__ __forceinline__ void tap_weights(float t, float* wt) {
    if constexpr (NT == 2) {
        wt[0] = opaque(1.0f - t);
        wt[1] = t;
    } else {
        wt[0] = keys_far(opaque(t + 1.0f));
        wt[1] = keys_near(t);
        wt[2] = keys_near(opaque(1.0f - t));
        wt[3] = keys_far(opaque(2.0f - t));
    }
}

}  // namespace im360
