// GEGLU feed-forward of the 320-channel blocks in ONE launch (ConvParams, tile_epilogue and the launch helpers: conv_tile.h):
//   out[M, 320] = GEGLU(LN(x) W1^T + b1) W2^T + b2 + res          x [M, 320], W1 [2 x 1280, 320], W2 [320, 1280]
// Replaces: FeedForward = GEGLU -> Dropout(0) -> Linear behind norm3 (+ the residual add), diffusers/models/attention_lora.py:493-547,
// activations.py:93-125; animatediff/models/attention.py:503-508, motion_module.py:255-258.  Today's pair of launches
// (im360_linear_geglu[_ln], then im360_conv_fwd on the [M, 1, 1, 1280] view with bias + residual) writes the 1280-wide GEGLU output H
// to memory and reads it straight back; here H never leaves the CU.
//
// One workgroup (512 threads, 8 waves, two per SIMD) per CU, persistent over 128-token tiles in conv_ring_kernel's XCD-aware order.
// Wave w = (tq, ch) = (w >> 1, w & 1): token quarter tq (32 tokens) x column half ch in BOTH GEMMs.
//   * the inner dimension is walked in 20 ascending CHUNKS of 64 channels = 128 packed W1 rows (pack_geglu's interleave: 32 value rows,
//     32 gate rows, twice);
//   * GEMM 1 of a chunk: five ascending 64-channel stages over K = 320; wave (tq, ch) accumulates the value and the gate block of
//     inner channels [32 ch, 32 ch + 32) of the chunk (2 accumulators = 32 registers), v_mfma_f32_32x32x16, D^T[row, token];
//   * GEGLU arithmetic of tile_epilogue<EPI 1 / 4> on those two accumulators, rounded to 16 bits, written TOKEN-MAJOR into the LDS
//     tile H_j [128 tokens][64 channels] with the operand tiles' XOR swizzle: the B operand of GEMM 2;
//   * GEMM 2 of a chunk: OUT[128 x 320] += H_j W2[:, chunk]^T, one 64-channel K stage; wave (tq, ch) owns output blocks 5 ch .. 5 ch + 4
//     (5 accumulators = 80 registers) -- the accumulation order over K = 1280 is today's FF-out's (ascending 16-channel MFMAs);
//   * after chunk 19: tile_epilogue<EPI 2, RESM 1> (bias from LDS, 16-bit rounding, residual, non-temporal row-major stores).
// Weights arrive by LDS-DMA in PIECES of 64 rows x 128 bytes (8 KiB: one 16-byte request per thread, every row segment a whole
// 128-byte line): a W1 stage is two pieces (packed rows [0, 64) and [64, 128) of the chunk), the W2 stage of a chunk five -- piece q
// holds output rows [32 q, 32 q + 32) and [160 + 32 q, 160 + 32 q + 32), i.e. block q of either column half.  A STEP consumes one
// 16 KiB ring slot: eight steps per chunk (five W1 stages; W2 pieces {0, 1}, {2, 3}, {4}), one barrier per step.  The ring has three
// slots: the barrier that opens step t frees the slot of step t - 1, into which step t + 2 is requested; the wait in front of the
// barrier is a counted vmcnt that leaves step t + 1 in flight.  The weight stream does not depend on the tile: it simply wraps from
// chunk 19 to chunk 0, so the first two steps of the next tile arrive under the output epilogue.
//
// LDS map (150 144 bytes):
//   [      0,  81920)  X      the tile's activations, resident for all 20 chunks: five stage images [128 rows][128 B]
//                             -- the output epilogue's transpose staging (8 waves x 32 rows x 320 B: a wave stages its own 160 columns) once the last chunk has read it
//   [  81920, 131072)  RING   3 slots x 16 KiB
//   [ 131072, 147456)  H      [128 tokens][128 B]
//   [ 147456, 149504)  CV     2 sets x 1 KiB: the chunk's column vectors (LN: fp32 c1[128] | c2[128] in packed row order; plain: b1, 16 bit)
//   [ 149504, 150144)  B2     the output bias (16 bit), staged once per workgroup
// Registers: 80 (OUT) + 32 (H_j accumulators) + 48 (fragments of a step) + addressing; no wait on another workgroup anywhere.
#include "conv_tile.h"

namespace im360 {
namespace ff {

constexpr int BM = 128, K1 = 320, INNER = 1280, NOUT = 320, NCHUNK = INNER / 64;
constexpr int STAGE_X = BM * 128;                  // one 64-channel stage image of the activation tile
constexpr int X_OFF = 0, X_BYTES = (K1 / 64) * STAGE_X;
constexpr int PIECE = 64 * 128, SLOT = 2 * PIECE, NSLOT = 3;
constexpr int RING_OFF = X_OFF + X_BYTES;
constexpr int H_OFF = RING_OFF + NSLOT * SLOT, H_BYTES = BM * 128;
constexpr int CV_OFF = H_OFF + H_BYTES, CV_SET = 1024;
constexpr int B2_OFF = CV_OFF + 2 * CV_SET;
constexpr int LDS_BYTES = B2_OFF + NOUT * 2;
static_assert(X_BYTES >= 8 * 32 * (5 * 64), "the output epilogue stages its transpose in the activation tile");
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");

struct Params {
    ConvParams c;           // x, w = packed W1, bias = b2, res, y, M, Cout = 320 and the LayerNorm fields as in im360_linear_geglu_ln
    const void* w2;         // pack_conv_weight([320, 1280, 1, 1])
    const void* b1;         // plain form: pack_geglu's bias (may be null); LN form: unused
};

// W2 pieces of step U = 5, 6, 7 of a chunk
constexpr int step_pieces(int u) { return u == 7 ? 1 : 2; }

template <typename T, bool LN>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void ff_fused_kernel(Params fp) {
    const ConvParams& p = fp.c;
    __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int col = lane & 31, hi = lane >> 5;
    const int wid_s = __builtin_amdgcn_readfirstlane(wid);
    const int tq = wid_s >> 1, ch = wid_s & 1;
    const T* xg = (const T*)p.x;
    const T* zero = (const T*)g_zero_chunk;
    const uint32_t lds_u32 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds);

    // persistent tile walk (conv_ring_kernel's, one cout group): block b sits on XCD b % 8, a round covers gridDim.x consecutive tiles
    const int per_xcd = gridDim.x / 8;
    const long ntiles = (p.M + BM - 1) / BM;
    const long tile_step = gridDim.x;
    long tile = (long)(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (tile >= ntiles) return;

    // ---- producer: thread t supplies LDS position t % 8 of piece row t / 8; the XOR swizzle is applied on the source side
    const int srow = tid >> 3;
    const int pd8 = ((tid & 7) ^ ((srow >> 1) & 7)) * 8;
    const T* const w1p = (const T*)p.w + srow * K1 + pd8;
    const T* const w2p = (const T*)fp.w2 + (srow < 32 ? srow : 128 + srow) * INNER + pd8;
    auto dma = [&](const T* src, int off) { lds_dma16_asm(src, lds_u32 + (uint32_t)off); };
    // step U of chunk jj into ring slot `slot`
    auto issue_step = [&](int jj, auto uc, int slot) {
        constexpr int U = decltype(uc)::value;
        const int base = RING_OFF + slot * SLOT + wid_s * 1024;
        if constexpr (U < 5) {
            dma(w1p + ((128 * jj) * K1 + 64 * U), base);
            dma(w1p + ((128 * jj + 64) * K1 + 64 * U), base + PIECE);
        } else {
            constexpr int q0 = 2 * (U - 5);
            dma(w2p + (q0 * 32 * INNER + 64 * jj), base);
            if constexpr (step_pieces(U) == 2) dma(w2p + ((q0 + 1) * 32 * INNER + 64 * jj), base + PIECE);
        }
    };
    // the column vectors of chunk jj -> set jj & 1 (wave 0; requested IN FRONT of the chunk's first step, so every counted wait that
    // covers that step covers them)
    auto issue_cv = [&](int jj) {
        const uint32_t dst = lds_u32 + (uint32_t)(CV_OFF + (jj & 1) * CV_SET);
        if constexpr (LN) {
            if (tid < 64) lds_dma16_asm((tid < 32 ? p.ln_c1 : p.ln_c2) + 128 * jj + (tid & 31) * 4, dst);
        } else {
            if (tid < 16) lds_dma16_asm(fp.b1 ? (const void*)((const T*)fp.b1 + 128 * jj + tid * 8) : (const void*)zero, dst);
        }
    };
    auto issue_x = [&](long m0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long m = m0 + srow + 64 * i;
            const T* src = m < p.M ? xg + m * K1 + pd8 : zero;
            const int step = m < p.M ? 64 : 0;
#pragma unroll
            for (int s = 0; s < K1 / 64; ++s) dma(src + s * step, X_OFF + s * STAGE_X + i * PIECE + wid_s * 1024);
        }
    };
    auto wait_vm = [&](int n) {
        if (n >= 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else if (n == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };

    // ---- consumer addressing: row R, 16-byte K chunk d of a [rows][128 B] image -> R * 128 + ((d ^ swz(R)) * 16)
    const int swz = (col >> 1) & 7;
    int koff[4];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) koff[kc] = ((kc * 2 + hi) ^ swz) * 16;
    const int xrow = X_OFF + (32 * tq + col) * 128;
    const int w1row = (64 * ch + col) * 128, w2row = (32 * ch + col) * 128;
    const int hrow = H_OFF + (32 * tq + col) * 128;

    // the output bias, once
    if (tid < NOUT / 8) *(uint4*)(lds + B2_OFF + tid * 16) = p.bias ? *(const uint4*)((const T*)p.bias + tid * 8) : uint4{0u, 0u, 0u, 0u};

    issue_x(tile * BM);
    issue_cv(0);
    issue_step(0, std::integral_constant<int, 0>{}, 0);
    issue_step(0, std::integral_constant<int, 1>{}, 1);
    int s0 = 0;                  // ring slot of the current chunk's step 0 (a chunk has 8 steps: + 2 mod 3 per chunk)

    for (;;) {
        const long m0 = tile * BM;
        // mean / rstd of this lane's row from the producer's per-slice (sum, sum of squares): epi_ln_row_stats's loads and sums, the
        // variance in the operation order hipcc gives that function inside conv_ring_kernel's EPI 4 instantiations -- mu * mu rounded,
        // then ONE fma(qq, 1 / K, - mu * mu); left to -ffast-math here it became fma(- mu, mu, qq / K), a last-bit difference of rstd
        // in some rows and the only arithmetic in which this kernel and the pair of launches differed.  The opaque copy pins it.
        float ln_mu[1] = {0.f}, ln_rs[1] = {1.f};
        if constexpr (LN) {
            const long mr = m0 + 32 * tq + col;
            const float* row = p.rs_in + (mr < p.M ? mr : p.M - 1) * p.rs_p * 2;
            float ss = 0.f, qq = 0.f;
            if (p.rs_p == 2) {
                const f32x2 v0 = *(const f32x2*)row, v1 = *(const f32x2*)(row + 2);
                ss = (ss + v0.x) + v1.x;
                qq = (qq + v0.y) + v1.y;
            } else {
                for (int j = 0; j < p.rs_p; ++j) {
                    const f32x2 v = *(const f32x2*)(row + j * 2);
                    ss += v.x;
                    qq += v.y;
                }
            }
            const float mu = ss * p.ln_invc;
            float mu2 = mu * mu;
            asm volatile("" : "+v"(mu2));
            ln_mu[0] = mu;
            ln_rs[0] = __builtin_amdgcn_rsqf(fmaxf(__builtin_fmaf(qq, p.ln_invc, -mu2), 0.f) + p.ln_eps);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the activation tile (its first reader is behind step 0's barrier)

        f32x16 oacc[5][1], hacc[2];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[a][0][r] = 0.f;

        for (int j = 0; j < NCHUNK; ++j) {
            const int jn = j == NCHUNK - 1 ? 0 : j + 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) hacc[0][r] = hacc[1][r] = 0.f;
            u32x4 hf[4];
            static_for<8>([&](auto uc) {
                constexpr int U = decltype(uc)::value;
                int slot = s0 + U % 3;
                slot = slot >= 3 ? slot - 3 : slot;
                int slot2 = slot + 2;
                slot2 = slot2 >= 3 ? slot2 - 3 : slot2;
                // step t landed for every wave (step t + 1 stays in flight); everybody is out of step t - 1's slot; H writes are visible
                wait_vm(step_pieces((U + 1) % 8));
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if constexpr (U == 6) issue_cv(jn);
                if constexpr (U + 2 < 8) issue_step(j, std::integral_constant<int, (U + 2) % 8>{}, slot2);
                else issue_step(jn, std::integral_constant<int, (U + 2) % 8>{}, slot2);
                const char* at = lds + RING_OFF + slot * SLOT;
                if constexpr (U < 5) {
                    u32x4 xf[4], wf[4][2];
#pragma unroll
                    for (int kc = 0; kc < 4; ++kc) {
                        xf[kc] = *(const u32x4*)(lds + xrow + U * STAGE_X + koff[kc]);
#pragma unroll
                        for (int a = 0; a < 2; ++a) wf[kc][a] = *(const u32x4*)(at + w1row + a * (32 * 128) + koff[kc]);
                    }
#pragma unroll
                    for (int kc = 0; kc < 4; ++kc)
#pragma unroll
                        for (int a = 0; a < 2; ++a)
                            hacc[a] = Elem<T>::mfma32(__builtin_bit_cast(uint4, wf[kc][a]), __builtin_bit_cast(uint4, xf[kc]), hacc[a]);
                } else {
                    if constexpr (U == 5) {
#pragma unroll
                        for (int kc = 0; kc < 4; ++kc) hf[kc] = *(const u32x4*)(lds + hrow + koff[kc]);
                    }
                    constexpr int NP = step_pieces(U), q0 = 2 * (U - 5);
                    u32x4 wf[NP][4];
#pragma unroll
                    for (int q = 0; q < NP; ++q)
#pragma unroll
                        for (int kc = 0; kc < 4; ++kc) wf[q][kc] = *(const u32x4*)(at + q * PIECE + w2row + koff[kc]);
#pragma unroll
                    for (int q = 0; q < NP; ++q)
#pragma unroll
                        for (int kc = 0; kc < 4; ++kc)
                            oacc[q0 + q][0] = Elem<T>::mfma32(__builtin_bit_cast(uint4, wf[q][kc]), __builtin_bit_cast(uint4, hf[kc]), oacc[q0 + q][0]);
                }
                if constexpr (U == 4) {
                    // ---- GEGLU of the chunk (tile_epilogue<EPI 1 / 4>'s arithmetic) -> H_j, token-major
                    const char* cv = lds + CV_OFF + (j & 1) * CV_SET;
                    const f32x2 MU = {ln_mu[0], ln_mu[0]}, RS = {ln_rs[0], ln_rs[0]};
                    const f32x16 av = hacc[0], ag = hacc[1];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x2 v01 = {av[4 * g], av[4 * g + 1]}, v23 = {av[4 * g + 2], av[4 * g + 3]};
                        f32x2 t01 = {ag[4 * g], ag[4 * g + 1]}, t23 = {ag[4 * g + 2], ag[4 * g + 3]};
                        const int rv = 64 * ch + 8 * g + 4 * hi, rg = rv + 32;          // packed rows, relative to the chunk
                        if constexpr (LN) {
                            const float* cvec = (const float*)cv;
                            const f32x4 k1v = *(const f32x4*)(cvec + rv), k2v = *(const f32x4*)(cvec + 128 + rv);
                            const f32x4 k1g = *(const f32x4*)(cvec + rg), k2g = *(const f32x4*)(cvec + 128 + rg);
                            v01 = (v01 - MU * k1v.xy) * RS + k2v.xy;
                            v23 = (v23 - MU * k1v.zw) * RS + k2v.zw;
                            t01 = (t01 - MU * k1g.xy) * RS + k2g.xy;
                            t23 = (t23 - MU * k1g.zw) * RS + k2g.zw;
                        } else {
                            const uint2 wv = *(const uint2*)(cv + rv * 2), wg = *(const uint2*)(cv + rg * 2);
                            v01 += f32x2{unpack_lo<T>(wv.x), unpack_hi<T>(wv.x)};
                            v23 += f32x2{unpack_lo<T>(wv.y), unpack_hi<T>(wv.y)};
                            t01 += f32x2{unpack_lo<T>(wg.x), unpack_hi<T>(wg.x)};
                            t23 += f32x2{unpack_lo<T>(wg.y), unpack_hi<T>(wg.y)};
                        }
                        v01 *= gelu_poly_pk(t01);
                        v23 *= gelu_poly_pk(t23);
                        uint2 o;
                        o.x = pack2<T>(v01.x, v01.y);
                        o.y = pack2<T>(v23.x, v23.y);
                        *(uint2*)(lds + hrow + (((4 * ch + g) ^ swz) << 4) + (hi << 3)) = o;
                    }
                }
            });
            s0 = s0 + 2 >= 3 ? s0 - 1 : s0 + 2;
        }

        // ---- output epilogue.  The activation tile was last read in step 4 of chunk 19 (three barriers ago): its LDS is the staging.
        const long next = tile + tile_step;
        int lane_e = lane, wid_e = wid_s;
        asm volatile("" : "+v"(lane_e), "+s"(wid_e));
        tile_epilogue<T, 512, 1, 5, 2, true, false, false, 2, 1>(p, oacc, lds + X_OFF, m0, 0, wid_e >> 1, wid_e & 1, wid_e, lane_e,
                                                                   (const float*)(lds + B2_OFF), NOUT);
        if (next >= ntiles) break;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // every wave is out of the staging
        issue_x(next * BM);
        tile = next;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the wrapped weight stream's last two steps: nothing lands behind the kernel
}

}  // namespace ff
}  // namespace im360

// One launch for the feed-forward of a 320-channel block.  LayerNorm-folded form (c1 given): operands of im360_linear_geglu_ln (w1_packed =
// pack_geglu(gamma (.) W1), fp32 c1 / c2 in packed row order, rowstats [M][rs_p][2]); plain form (c1 == null): operands of im360_linear_geglu
// (b1_packed may be null).  w2_packed = pack_conv_weight of the [N, I, 1, 1] view, b2 [N] or null, res [M, N] (may alias x), y [M, N].
// K = 320, I = 1280, N = 320 only: anything else is IM360_ERR_UNSUPPORTED.
extern "C" __attribute__((visibility("default"))) int im360_ff_fused(const void* x, const void* w1_packed, const void* b1_packed, const void* c1, const void* c2,
                              const void* rowstats, int64_t rs_p, float eps, const void* w2_packed, const void* b2, const void* res, void* y,
                              int64_t M, int64_t K, int64_t I, int64_t N, int dtype, void* stream) {
    using namespace im360;
    IM360_CHECK_ARG(x && w1_packed && w2_packed && res && y, "ff_fused: null pointer");
    IM360_CHECK_ARG(M > 0 && M <= 0x7fffffffL, "ff_fused: M=%ld out of range", (long)M);
    if (K != ff::K1 || I != ff::INNER || N != ff::NOUT) {
        im360_set_error("ff_fused: K=%ld, I=%ld, N=%ld unsupported (320, 1280, 320 only)", (long)K, (long)I, (long)N);
        return IM360_ERR_UNSUPPORTED;
    }
    const bool ln = c1 != nullptr;
    IM360_CHECK_ARG(!ln || (c2 && rowstats && rs_p > 0 && rs_p <= 64), "ff_fused: the LayerNorm-folded form needs c1, c2, rowstats and rs_p in [1, 64]");
    IM360_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)w1_packed % 16) == 0 && ((uintptr_t)w2_packed % 16) == 0 && ((uintptr_t)y % 16) == 0 &&
                    ((uintptr_t)res % 16) == 0 && ((uintptr_t)b1_packed % 16) == 0 && ((uintptr_t)b2 % 16) == 0 && ((uintptr_t)c1 % 16) == 0 &&
                    ((uintptr_t)c2 % 16) == 0 && ((uintptr_t)rowstats % 8) == 0, "ff_fused: misaligned pointer");
    IM360_CHECK_ARG(dtype == 0 || dtype == 1, "ff_fused: dtype %d unsupported", dtype);
    ff::Params fp;
    fp.c = linear_params(x, w1_packed, y, M, K, N);
    fp.c.bias = b2; fp.c.res = res;
    if (ln) {
        fp.c.rs_in = (const float*)rowstats; fp.c.rs_p = (int)rs_p; fp.c.ln_eps = eps; fp.c.ln_invc = 1.0f / (float)K;
        fp.c.ln_c1 = (const float*)c1; fp.c.ln_c2 = (const float*)c2;
    }
    fp.w2 = w2_packed;
    fp.b1 = b1_packed;
    ProfScope prof(PROF_GEMM, stream);
    const unsigned grid = persistent_grid((M + ff::BM - 1) / ff::BM);
    return with_dtype(dtype, "ff_fused", [&](auto t) {
        using T = typename decltype(t)::type;
        with_bool(ln, [&](auto lnc) { hipLaunchKernelGGL((ff::ff_fused_kernel<T, decltype(lnc)::value>), dim3(grid), dim3(512), 0, (hipStream_t)stream, fp); });
        return im360_launch_status();
    });
}
