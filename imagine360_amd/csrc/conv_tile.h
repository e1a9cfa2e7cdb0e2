// What the tile kernels of conv3x3.hip and ff_fused.hip share: the launch parameters, the epilogue of a tile of 32 x 32 MFMA blocks and the
// host-side helpers of the persistent token-major launches.
#pragma once
#include <string.h>

#include "common.h"

namespace im360 {

struct ConvParams {
    const void* x; const void* w; const void* bias; const void* temb; const void* res; void* y;
    int N, Hin, Win, Cin, Hout, Wout, Cout;
    int ntaps;          // 9 (3x3) or 1 (1x1)
    int stride, up, wrap, x_off, y_off;
    int imgs_per_temb;
    long M;             // N * Hout * Wout
    int tiles_n;        // ceil(Cout / 128)
    long nblocks;
    int halo_r, halo_seg, halo_pw, halo_p;      // halo kernel: output rows per tile, rows per image segment, patch width / pixels
    int up2_py, up2_px; // UP2 kernels: output parity (row, column) of this launch
    int dbg;            // ablation switches of the ring kernel (tools/ab_ring.py --ablate): 1 no LDS-DMA in the K loop, 2 no MFMA, 4 no fragment reads, 8 no epilogue
    // 1x1 convolution of a channel concatenation that is never materialised: input channels [0, Cin1) come from x
    // (pixel stride Cin1), channels [Cin1, Cin) from x2 (pixel stride Cin - Cin1); x2 == nullptr: one source
    const void* x2; int Cin1;
    // token-major linears only.  rs_out: the epilogue also writes, per output row and per 160-column wave slice, (sum,
    // sum of squares) of the stored 16-bit values: fp32 [M][Cout / 160][2] -- the LayerNorm statistics of the rows for a
    // consumer GEMM with the normalisation folded in (EPI 3 / 4), which reads them through rs_in ([M][rs_p][2]):
    //   y = rstd_r * (x W'^T - mu_r * c1) + (ln_tab ? ln_tab[(r / tab_div) % tab_mod] : c2)      W' = gamma (.) W; table rows INCLUDE c2
    float* rs_out; const float* rs_in; int rs_p; float ln_eps, ln_invc;
    const float* ln_c1; const float* ln_c2; const float* ln_tab; int tab_div, tab_mod;
    // persistent tile walk of the ring kernel: the cout tiles are split into `ngroups` groups, each walked by 8 / ngroups
    // XCDs over all pixel tiles (keeps one group's weights resident in those XCDs' L2s)
    int ngroups;
    // GroupNorm statistics from the epilogue (GNS kernels, 256 x 320 tiles): per pixel tile and output channel (sum, sum of
    // squares) of the values the tile stores, fp32 [M / 256][2][Cout] -- the layout of groupnorm.hip's per-slab partial sums
    // when an image is a whole number of tiles (H W % 256 == 0: slab s of image n = tile n * (H W / 256) + s), so the consumer's
    // GroupNorm skips its own statistics pass over the tensor (animatediff/models/resnet.py:221-243: norm -> act -> conv, twice)
    float* gn_out;
    // knob nt (default 1; tools/ab_step.py, profiles/r06_step_knobs_ab.log: - 1.5 ms per cfg2 step): the epilogue's output rows leave with
    // non-temporal stores -- tensors of hundreds of MB that should not push the operands out of the L2.  (The same on the attention
    // outputs, which the out-projection reads back at once, cost + 6.7 ms; on the LayerNorm / GEGLU element-wise kernels nothing.)
    int nt_store;
    // K-split of conv_igemm_kernel's 3 x 3 convolutions (taps innermost; round 6): `ksplit` workgroups share one output tile, each over a
    // contiguous range of the 64-channel chunks.  Parts 0 .. ksplit - 2 park their fp32 accumulators in ks_ws ([tile][part][160 * 512]
    // floats, lane-linear) and count themselves into ks_cnt[tile]; the LAST part -- dispatched behind all the others: block ids are part-major --
    // adds them in part order and runs the epilogue.  For launches whose tile count is not a whole number of rounds of 256 CUs (or below one).
    int ksplit;
    float* ks_ws;
    int* ks_cnt;
};

// ConvParams with the optional members cleared
static inline ConvParams conv_params_zero() {
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.ngroups = 1;
    p.nt_store = knob(KNOB_NT) & 1;
    return p;
}

// 16 bytes of zeros that out-of-image taps are pointed at (LDS-DMA loads cannot zero-fill by themselves)
static __device__ uint4 g_zero_chunk[1];

// keep a value alive without code (ablation switches of the ring kernel; a __device__ helper because the host pass of
// hipcc silently drops a __global__ body whose inline asm it cannot type for x86)
__device__ __forceinline__ void keep_alive(u32x4 v) { asm volatile("" ::"v"(v)); }
__device__ __forceinline__ void keep_alive(f32x16 v) { asm volatile("" ::"v"(v)); }

// ---- epilogue shared by the tile kernels.  `lds` is a region of at least (waves * 32 * row bytes) that no wave reads
//      as operand tiles any more; the caller has passed a workgroup barrier since the last operand read.
// UP2: the tile's rows are pixels of the LOW-resolution grid [N, Hout, Wout]; row (n, y, x) is stored at pixel
// (n, 2 y + up2_py, 2 x + up2_px) of the [N, 2 Hout, 2 Wout, Cout] output (sub-pixel form of nearest-x2 + conv3x3).
// cvec (EPI 3 / 4): the tile's fp32 column vectors staged in LDS by the caller, [0, BN) = c1, [BN, 2 BN) = c2, or the tile's table row (which includes c2).
// (row, 16-byte piece) of `lane` in store round `it` of a 32-row block whose rows hold PIECES pieces; false: the lane idles in this
// round (GNS only: every lane keeps ONE piece through all rounds, RPR = 64 / PIECES whole rows per round)
template <int PIECES, bool GNS>
__device__ __forceinline__ bool epi_round_rc(int it, int lane, int& row, int& pc) {
    if constexpr (GNS) {
        constexpr int RPR = 64 / PIECES;
        row = it * RPR + lane / PIECES;
        pc = lane % PIECES;
        const bool act = lane < RPR * PIECES && row < 32;
        row = row < 32 ? row : 31;
        return act;
    } else {
        const int f = it * 64 + lane;
        row = f / PIECES;
        pc = f % PIECES;
        return true;
    }
}
template <int PIECES, bool GNS>
constexpr int epi_rounds() { return GNS ? (32 + 64 / PIECES - 1) / (64 / PIECES) : (32 * PIECES) / 64; }
// EPI 3 (LayerNorm folded into the projection): mean / rstd of this lane's row in each of the wave's TM blocks from the producer's
// per-slice (sum, sum of squares).  All slices of both rows are requested before the first is added (2 / 4 / 8 slices unrolled: a
// run-time loop waits for each load in turn); the persistent kernel calls this right behind its K loop, BEFORE the next tile's
// first LDS-DMA requests: hipcc's wait for these loads is vmcnt(0) -- it does not see the asm requests -- and behind them it would
// also wait for a stage that was requested a moment ago.
template <int TM>
__device__ __forceinline__ void epi_ln_row_stats(const ConvParams& p, long m0, int wm, int col, float (&mus)[TM], float (&rstds)[TM]) {
    float ss[TM], qq[TM];
    const float* rows[TM];
#pragma unroll
    for (int b = 0; b < TM; ++b) {
        const long mr = m0 + wm * (TM * 32) + b * 32 + col;
        rows[b] = p.rs_in + (mr < p.M ? mr : p.M - 1) * p.rs_p * 2;
        ss[b] = qq[b] = 0.f;
    }
    auto sum_n = [&](auto nc) {
        constexpr int NS = decltype(nc)::value;
        f32x2 v[TM][NS];
#pragma unroll
        for (int b = 0; b < TM; ++b)
#pragma unroll
            for (int j = 0; j < NS; ++j) v[b][j] = *(const f32x2*)(rows[b] + j * 2);
#pragma unroll
        for (int b = 0; b < TM; ++b)
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                ss[b] += v[b][j].x;
                qq[b] += v[b][j].y;
            }
    };
    if (p.rs_p == 2) sum_n(std::integral_constant<int, 2>{});
    else if (p.rs_p == 4) sum_n(std::integral_constant<int, 4>{});
    else if (p.rs_p == 8) sum_n(std::integral_constant<int, 8>{});
    else {
#pragma unroll
        for (int b = 0; b < TM; ++b)
            for (int j = 0; j < p.rs_p; ++j) {
                const f32x2 v = *(const f32x2*)(rows[b] + j * 2);
                ss[b] += v.x;
                qq[b] += v.y;
            }
    }
#pragma unroll
    for (int b = 0; b < TM; ++b) {
        mus[b] = ss[b] * p.ln_invc;
        rstds[b] = __builtin_amdgcn_rsqf(fmaxf(qq[b] * p.ln_invc - mus[b] * mus[b], 0.f) + p.ln_eps);
    }
}

// RESM: 0 = residual known at run time only (its loads are unconditional: an absent one reads the zero chunk); 1 = residual
// present; 2 = no residual: the row-major pass moves whole 16-byte pieces LDS -> memory without unpacking them.  Round 4
// (tools/patches/ring_cycle_stamps.patch: cycle stamps of one workgroup): the plain epilogue of a 256 x 320 tile takes 14 000
// cycles and is VECTOR-bound (~ 6 instructions per element, more than half of them the unpack / add / repack of the row-major
// pass), 28 000 with a residual whose two loads per block each expose an HBM latency.  RESM 2 drops the row-major pass's
// arithmetic; requesting the residual pieces of BOTH blocks ahead (RESM 1's first form) put 90 - 110 registers into scratch next
// to the 160 accumulators; requesting block 0's from the kernel right behind its last MFMA (no scratch once the lane id was kept from
// being hoisted: a scratch reload is a VMEM load whose wait also waits for the pieces in front of it) measured 0.318 vs 0.306 ms on the
// level-0 out-projection + residual -- that GEMM moves 1.26 GB in 0.31 ms, it is at the HBM rate, not waiting for a latency.  Both
// dropped: RESM 1 requests per block, half before and half behind its register -> LDS pass.
// Same arithmetic in all three: identical values (RESM 2 keeps the sign of a zero that x + 0 would clear).
// ZACC (the four-wave tile, conv3x3_g4.hip): the accumulators live in AGPRs (asm constraint "a") and the next tile accumulates into
// them from its first MFMA; once a pixel block's values have left the registers its TN accumulators are cleared by one MFMA each with
// zero operands and C = 0 (the matrix pipe is idle during the epilogue; 256 v_accvgpr_write would cost 1000 issue cycles per tile).
template <typename T, bool VG = false> __device__ __forceinline__ void zero_acc_mfma(f32x16& d) {       // VG: this accumulator lives in VGPRs (the 256 x 320 tile's fifth cout block)
    const u32x4 z = {0u, 0u, 0u, 0u};
    if constexpr (VG) {
        if constexpr (std::is_same<T, __bf16>::value) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %1, 0\n\ts_nop 11" : "=v"(d) : "v"(z));
        else asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %1, 0\n\ts_nop 11" : "=v"(d) : "v"(z));
        return;
    }
    // (s_nop 11: the wait states an 8-pass MFMA result needs before anything but an accumulating MFMA may touch it -- hipcc does not know
    //  what the statement is and may copy / spill the output right behind it; s_nop 1 in front: VALU write of z -> MFMA operand)
    if constexpr (std::is_same<T, __bf16>::value) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %1, 0\n\ts_nop 11" : "=a"(d) : "v"(z));
    else asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %1, 0\n\ts_nop 11" : "=a"(d) : "v"(z));
}
template <typename T, int NT, int TM, int TN, int EPI, bool COUT8 = false, bool UP2 = false, bool GNS = false, int WN_ = 2, int RESM = 0, bool ZACC = false>
__device__ __forceinline__ void tile_epilogue(const ConvParams& p, f32x16 (&acc)[TN][TM], char* lds, long m0, int n0,
                                              int wm, int wn, int wid_s, int lane, const float* cvec = nullptr, int bn = 0,
                                              const float* ln_pre = nullptr) {
    const int col = lane & 31, hi = lane >> 5;
    const T* bias = (const T*)p.bias;
    const T* temb = (const T*)p.temb;
    const T* res = (const T*)p.res;
    T* yg = (T*)p.y;
    const int nw0 = n0 + wn * (TN * 32);          // first cout of this wave
    // LDS transpose of one 32-pixel block of this wave: rows of ROWB bytes (TN or TN/2 blocks of 32 couts), unpadded
    // and 16-byte aligned; the 16-byte piece index is XORed with row bits and the two 8-byte halves of a piece are
    // swapped on odd row octets, which makes the fragment-side 8-byte writes of 16 consecutive pixels hit 16
    // different bank pairs (checked exhaustively for 320- and 128-byte rows).  The row-major side reads whole pieces.
    // (256-byte rows -- the four-wave tile's plain epilogue -- take the 128-byte pattern: a row is then a whole number of the
    //  stores' 128-byte bank windows, and the XOR stays inside a group of eight pieces)
    // (64-byte rows -- the GEGLU epilogue of the 256 x 128 tile, TN = 2: four pieces per row, two rows per bank window)
    auto piece_xor = [](int row, int rowb) { return (rowb == 320 || rowb == 64) ? ((row >> 1) & 3) : (row & 7); };
    if constexpr (EPI == 1 || EPI == 4) {
        // GEGLU epilogue (token-major linear only): the packed weight rows alternate 32 value rows / 32 gate rows of the
        // same output channels, so accumulators (2i, 2i+1) hold value and gate of one channel in the same lane and
        // register: out = (value + b) * gelu(gate + b), half as many columns as the GEMM is wide.
        static_assert(TN % 2 == 0, "value / gate blocks come in pairs");
        constexpr int ROWB = (TN / 2) * 64;
        constexpr int PIECES = ROWB / 16;
        static_assert(ROWB == 128 || ROWB == 64, "swizzle pattern");
        const int I = p.Cout / 2;
        const int ow0 = nw0 / 2;                  // first output channel of this wave
        char* wlds = lds + wid_s * (32 * ROWB);
        const int fr = piece_xor(col, ROWB), br = (col >> 3) & 1;
        const T* gb = bias ? bias : (const T*)g_zero_chunk;      // unconditional bias loads (see the plain epilogue)
        const int gbmul = bias ? 1 : 0;
        // the biases of this lane's channels, unpacked once for all TM pixel blocks (the K-loop operand registers are free)
        f32x2 bv[EPI == 1 ? TN / 2 : 1][4][2], bt[EPI == 1 ? TN / 2 : 1][4][2];
        if constexpr (EPI == 1) {
#pragma unroll
        for (int i = 0; i < TN / 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int rv = nw0 + (2 * i) * 32 + 8 * g + 4 * hi, rg = rv + 32;          // packed rows (bias index)
                const uint2 wv = *(const uint2*)(gb + rv * gbmul), wg = *(const uint2*)(gb + rg * gbmul);
                bv[i][g][0] = f32x2{unpack_lo<T>(wv.x), unpack_hi<T>(wv.x)};
                bv[i][g][1] = f32x2{unpack_lo<T>(wv.y), unpack_hi<T>(wv.y)};
                bt[i][g][0] = f32x2{unpack_lo<T>(wg.x), unpack_hi<T>(wg.x)};
                bt[i][g][1] = f32x2{unpack_lo<T>(wg.y), unpack_hi<T>(wg.y)};
            }
        }
        // EPI 4: LayerNorm folded into the projection -- the accumulators hold x W'^T of the RAW rows (W' = gamma (.) W);
        // with the row's mean / rstd from the producer's statistics, value = rstd * (acc - mu * c1) + c2 (fp32 vectors in
        // packed row order: c1 = row sums of W', c2 = W beta + bias).  The statistics of this lane's row in every block are
        // requested up front (one memory latency for the tile instead of one per block).
        float ln_mu[TM], ln_rs[TM];
        if constexpr (EPI == 4) {
            if (ln_pre) {                 // (the persistent kernel computed them behind its K loop, see epi_ln_row_stats)
#pragma unroll
                for (int b = 0; b < TM; ++b) {
                    ln_mu[b] = ln_pre[b];
                    ln_rs[b] = ln_pre[TM + b];
                }
            } else {
                epi_ln_row_stats<TM>(p, m0, wm, col, ln_mu, ln_rs);
            }
        }
        static_for<TM>([&](auto bcc) {
            constexpr int b = decltype(bcc)::value;
            const long mb = m0 + wm * (TM * 32) + b * 32;
            f32x2 MU = {0.f, 0.f}, RS = {1.f, 1.f};
            if constexpr (EPI == 4) {
                MU = f32x2{ln_mu[b], ln_mu[b]};
                RS = f32x2{ln_rs[b], ln_rs[b]};
            }
            static_for<TN / 2>([&](auto icc) {
                constexpr int i = decltype(icc)::value;
                const f32x16 av = acc[2 * i][b], ag = acc[2 * i + 1][b];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    // (the unfused path rounds the projection to 16 bits before the activation; this one does not --
                    //  one rounding less on the way to the fp32 oracle)
                    f32x2 v01 = {av[4 * g], av[4 * g + 1]}, v23 = {av[4 * g + 2], av[4 * g + 3]};
                    f32x2 t01 = {ag[4 * g], ag[4 * g + 1]}, t23 = {ag[4 * g + 2], ag[4 * g + 3]};
                    if constexpr (EPI == 4) {
                        const int rv = nw0 - n0 + (2 * i) * 32 + 8 * g + 4 * hi, rg = rv + 32;      // packed rows, relative to the tile
                        const f32x4 k1v = *(const f32x4*)(cvec + rv), k2v = *(const f32x4*)(cvec + bn + rv);
                        const f32x4 k1g = *(const f32x4*)(cvec + rg), k2g = *(const f32x4*)(cvec + bn + rg);
                        v01 = (v01 - MU * k1v.xy) * RS + k2v.xy;
                        v23 = (v23 - MU * k1v.zw) * RS + k2v.zw;
                        t01 = (t01 - MU * k1g.xy) * RS + k2g.xy;
                        t23 = (t23 - MU * k1g.zw) * RS + k2g.zw;
                    } else {
                    v01 += bv[i][g][0];
                    v23 += bv[i][g][1];
                    t01 += bt[i][g][0];
                    t23 += bt[i][g][1];
                    }
                    v01 *= gelu_poly_pk(t01);
                    v23 *= gelu_poly_pk(t23);
                    uint2 o;
                    o.x = pack2<T>(v01.x, v01.y);
                    o.y = pack2<T>(v23.x, v23.y);
                    *(uint2*)(wlds + col * ROWB + (((i * 4 + g) ^ fr) << 4) + ((hi ^ br) << 3)) = o;
                }
            });
            if constexpr (ZACC) static_for<TN>([&](auto ac) { zero_acc_mfma<T, (TN == 5 && decltype(ac)::value == 4)>(acc[decltype(ac)::value][b]); });
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int it = 0; it < (32 * PIECES + 63) / 64; ++it) {
                const int f = it * 64 + lane;
                const int row = f / PIECES, pc = f % PIECES;
                const long mr = mb + row;
                const int co = ow0 + pc * 8;
                if (row < 32 && mr < p.M && co < I) {
                    uint4 o = *(const uint4*)(wlds + row * ROWB + ((pc ^ piece_xor(row, ROWB)) << 4));
                    if ((row >> 3) & 1) { const uint32_t t0 = o.x, t1 = o.y; o.x = o.z; o.y = o.w; o.z = t0; o.w = t1; }
                    if (p.nt_store) __builtin_nontemporal_store(u32x4{o.x, o.y, o.z, o.w}, (u32x4*)(yg + mr * I + co));
                    else *(uint4*)(yg + mr * I + co) = o;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        });
        return;
    } else {
    // ---- epilogue.  Lane (pixel = col, hi) holds 4 consecutive couts per register group, i.e. stored directly every
    //      lane would write 8 bytes at a pixel-row stride (32 rows x 16 B per instruction).  Instead each wave
    //      transposes its tile through LDS (free after the K loop), 32 pixels at a time: bias / temb are added in
    //      registers, the 16-bit rows are written to LDS, then read back row-major so consecutive lanes store (and
    //      fetch the residual from) consecutive 16-byte pieces of one output row -- whole 128-byte lines.
    if (COUT8 || (p.Cout & 7) == 0) {
        constexpr int ROWB = TN * 64;
        constexpr int PIECES = ROWB / 16;
        static_assert(ROWB == 128 || ROWB == 256 || ROWB == 320, "swizzle pattern");
        static_assert((32 * PIECES) % 64 == 0, "store rounds cover the block exactly");
        static_assert(!GNS || (!UP2 && EPI != 3), "GroupNorm statistics: plain conv / linear epilogues");
        // GNS: every lane keeps ONE 16-byte piece (8 channels) through all store rounds -- RPR whole rows per round on
        // RPR * PIECES lanes (60 of 64 at 320-byte rows: 11 rounds instead of 10) -- so that it can add up its channels'
        // (sum, sum of squares) over the rows it stores in 16 registers
        constexpr int RPR = 64 / PIECES;
        float gsum[GNS ? 8 : 1], gsq[GNS ? 8 : 1];
        if constexpr (GNS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) gsum[e] = gsq[e] = 0.f;
        }
        char* wlds = lds + wid_s * (32 * ROWB);
        const int fr = piece_xor(col, ROWB), br = (col >> 3) & 1;
        // Every global load of the epilogue is UNCONDITIONAL: an absent operand (no bias / temb / residual) reads the
        // 16-byte zero chunk with a zero index multiplier, out-of-range rows / couts are clamped into the tensor (their
        // results are never stored).  A load behind a per-lane or per-operand branch makes hipcc wait vmcnt(0) at every
        // use -- and since stores count in vmcnt too, that serialised the ten store rounds of a block behind each other.
        // Addresses are a wave-uniform 64-bit base (block row 0) + a 32-bit per-lane byte offset: ten 64-bit load and ten
        // 64-bit store addresses per block would otherwise be kept live (and spilled) next to the accumulators.
        const char* zsrc = (const char*)g_zero_chunk;
        const char* bsrc = bias ? (const char*)bias : zsrc;
        const char* tsrc = temb ? (const char*)temb : zsrc;
        const uint32_t bmul = bias ? 2u : 0u, tmul = temb ? 2u : 0u, rmul = res ? 2u : 0u;      // bytes per element, or 0
        const int cmax4 = p.Cout - 4, cmax8 = p.Cout - 8;
        const long hw = (long)p.Hout * p.Wout;
        // EPI 3: LayerNorm folded into the projection (see ConvParams): mean / rstd of this lane's row in every block from the
        // producer's per-slice (sum, sum of squares), all requested up front (one memory latency per tile, not one per block)
        float ln_mus[EPI == 3 ? TM : 1], ln_rstds[EPI == 3 ? TM : 1];
        if constexpr (EPI == 3) {
            if (ln_pre) {                 // (the persistent kernel computed them behind its K loop: [mu_0 .. mu_TM-1, rstd_0 ..])
#pragma unroll
                for (int b = 0; b < TM; ++b) {
                    ln_mus[b] = ln_pre[b];
                    ln_rstds[b] = ln_pre[TM + b];
                }
            } else {
                epi_ln_row_stats<TM>(p, m0, wm, col, ln_mus, ln_rstds);
            }
        }
        constexpr int NIT = epi_rounds<PIECES, GNS>(), NIT1 = NIT / 2;
        u32x4 rvs[1][NIT];
        auto round_rc = [&](int it, int& row, int& pc) { return epi_round_rc<PIECES, GNS>(it, lane, row, pc); };
        auto piece_off_r = [&](int it, int rows, bool& ok) {      // element offset of this lane's piece in round `it` (clamped into the block)
            int row, pc;
            const bool act = round_rc(it, row, pc);
            const int co = nw0 + pc * 8;
            ok = act && row < rows && co < p.Cout;
            return (uint32_t)((row < rows ? row : rows - 1) * p.Cout + (co < cmax8 ? co : cmax8));
        };
        static_for<TM>([&](auto bcc) {
            constexpr int b = decltype(bcc)::value;
            const long mb = m0 + wm * (TM * 32) + b * 32;           // first pixel of the block (wave-uniform)
            // (ZACC = the four-wave tile: M % 256 == 0, every block is whole -- and no control flow splits the accumulators' live ranges)
            if constexpr (!ZACC) {
                if (mb >= p.M) return;
            }
            const int rows = ZACC ? 32 : (p.M - mb < 32 ? (int)(p.M - mb) : 32);  // valid rows of the block
            u32x4 (&rv)[NIT] = rvs[0];
            const char* rbase = res ? (const char*)(res + mb * p.Cout) : zsrc;
            char* ybase = (char*)(yg + mb * p.Cout);
            const long m = mb + (col < rows ? col : rows - 1);
            const uint32_t toff = (uint32_t)((m / hw) / p.imgs_per_temb) * (uint32_t)p.Cout;   // temb row of this lane's pixel
            float ln_mu = 0.f, ln_rstd = 1.f;
            if constexpr (EPI == 3) {
                ln_mu = ln_mus[b];
                ln_rstd = ln_rstds[b];
            }
            // residual pieces of this block: the first half is requested before the register -> LDS pass, the second
            // right after it (the accumulators it frees make room), so the HBM latency overlaps the shuffle work
            auto piece_off = [&](int it, bool& ok) { return piece_off_r(it, rows, ok); };
            auto load_res = [&](int it0, int it1) {
                if constexpr (RESM != 2) {
#pragma unroll
                    for (int it = it0; it < it1; ++it) {
                        bool ok;
                        rv[it] = *(const u32x4*)(rbase + piece_off(it, ok) * (RESM == 1 ? 2u : rmul));
                    }
                }
            };
            load_res(0, NIT1);
            __builtin_amdgcn_sched_barrier(0);    // (hipcc would hoist every load of the block up here and spill)
            static_for<TN>([&](auto acc_c) {
                constexpr int a = decltype(acc_c)::value;
                const f32x16 at = acc[a][b];
                if constexpr (EPI == 3) {
                    // the column vectors come from LDS (staged once per tile by the kernel: from global memory the forty
                    // dependent load rounds of a block cost more than the LayerNorm pass this epilogue replaces)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int cr = nw0 - n0 + a * 32 + 8 * g + 4 * hi;
                        const f32x4 k1 = *(const f32x4*)(cvec + cr), k2 = *(const f32x4*)(cvec + bn + cr);
                        float f[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) f[j] = (at[4 * g + j] - ln_mu * k1[j]) * ln_rstd + k2[j];
                        uint2 o;
                        o.x = pack2<T>(f[0], f[1]);
                        o.y = pack2<T>(f[2], f[3]);
                        *(uint2*)(wlds + col * ROWB + (((a * 4 + g) ^ fr) << 4) + ((hi ^ br) << 3)) = o;
                    }
                } else {
                uint2 wb[4], wt[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = nw0 + a * 32 + 8 * g + 4 * hi;
                    const uint32_t cc = (uint32_t)(co < cmax4 ? co : cmax4);
                    if constexpr (EPI == 2 || EPI == 5) {
                        // (the persistent kernel staged the tile's bias slice in LDS; other callers pass no cvec)
                        // (COUT8 = the persistent kernel: it staged the tile's bias slice in LDS -- a compile-time fact, a run-time test of the
                        //  pointer costs a scalar branch per load, 40 per block)
                        if constexpr (COUT8) wb[g] = *(const uint2*)((const char*)cvec + (co - n0) * 2);
                        else wb[g] = *(const uint2*)(bsrc + cc * bmul);
                    } else {
                        wb[g] = *(const uint2*)(bsrc + cc * bmul);
                    }
                    if constexpr (EPI == 0) wt[g] = *(const uint2*)(tsrc + (toff + cc) * tmul);      // (token-major linears have no temb)
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float f[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) f[j] = at[4 * g + j];
                    f[0] += unpack_lo<T>(wb[g].x); f[1] += unpack_hi<T>(wb[g].x); f[2] += unpack_lo<T>(wb[g].y); f[3] += unpack_hi<T>(wb[g].y);
                    if constexpr (EPI == 0) {
                        f[0] += unpack_lo<T>(wt[g].x); f[1] += unpack_hi<T>(wt[g].x); f[2] += unpack_lo<T>(wt[g].y); f[3] += unpack_hi<T>(wt[g].y);
                    }
                    uint2 o;
                    o.x = pack2<T>(f[0], f[1]);
                    o.y = pack2<T>(f[2], f[3]);
                    *(uint2*)(wlds + col * ROWB + (((a * 4 + g) ^ fr) << 4) + ((hi ^ br) << 3)) = o;
                }
                }
                __builtin_amdgcn_sched_barrier(0);
            });
            if constexpr (ZACC) static_for<TN>([&](auto ac) { zero_acc_mfma<T, (TN == 5 && decltype(ac)::value == 4)>(acc[decltype(ac)::value][b]); });
            load_res(NIT1, NIT);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                int row, pc;
                const bool act = round_rc(it, row, pc);
                uint4 o = *(const uint4*)(wlds + row * ROWB + ((pc ^ piece_xor(row, ROWB)) << 4));
                if ((row >> 3) & 1) { const uint32_t t0 = o.x, t1 = o.y; o.x = o.z; o.y = o.w; o.z = t0; o.w = t1; }
                if constexpr (RESM != 2) {
                const u32x4 w = rv[it];
                float fv[8] = {unpack_lo<T>(o.x) + unpack_lo<T>(w.x), unpack_hi<T>(o.x) + unpack_hi<T>(w.x), unpack_lo<T>(o.y) + unpack_lo<T>(w.y), unpack_hi<T>(o.y) + unpack_hi<T>(w.y),
                               unpack_lo<T>(o.z) + unpack_lo<T>(w.z), unpack_hi<T>(o.z) + unpack_hi<T>(w.z), unpack_lo<T>(o.w) + unpack_lo<T>(w.w), unpack_hi<T>(o.w) + unpack_hi<T>(w.w)};
                o.x = pack2<T>(fv[0], fv[1]);
                o.y = pack2<T>(fv[2], fv[3]);
                o.z = pack2<T>(fv[4], fv[5]);
                o.w = pack2<T>(fv[6], fv[7]);
                }
                bool ok;
                const uint32_t off = piece_off(it, ok);
                if constexpr (GNS) {
                    // statistics of the values as STORED (rounded to 16 bits: what a statistics pass over the tensor would read)
                    const float wgt = ok ? 1.f : 0.f;
                    const float sv[8] = {unpack_lo<T>(o.x), unpack_hi<T>(o.x), unpack_lo<T>(o.y), unpack_hi<T>(o.y), unpack_lo<T>(o.z), unpack_hi<T>(o.z), unpack_lo<T>(o.w), unpack_hi<T>(o.w)};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float v = wgt * sv[e];
                        gsum[e] += v;
                        gsq[e] = fmaf(v, sv[e], gsq[e]);
                    }
                }
                if (EPI == 5 && (!GNS || act)) {
                    // row statistics of the STORED values (what a LayerNorm of this tensor would read): this piece's
                    // (sum, sum of squares) parked in its own staging slot, collected per row after the store rounds
                    float ss = 0.f, qq = 0.f;
                    ss = dot2_acc<T>(o.x, Elem<T>::ones2, ss); qq = dot2_acc<T>(o.x, o.x, qq);
                    ss = dot2_acc<T>(o.y, Elem<T>::ones2, ss); qq = dot2_acc<T>(o.y, o.y, qq);
                    ss = dot2_acc<T>(o.z, Elem<T>::ones2, ss); qq = dot2_acc<T>(o.z, o.z, qq);
                    ss = dot2_acc<T>(o.w, Elem<T>::ones2, ss); qq = dot2_acc<T>(o.w, o.w, qq);
                    *(f32x2*)(wlds + row * ROWB + ((pc ^ piece_xor(row, ROWB)) << 4)) = f32x2{ss, qq};
                }
                if constexpr (UP2) {
                    const int co = nw0 + pc * 8;
                    const long mrow = mb + (row < rows ? row : rows - 1);
                    const long nimg = mrow / hw;
                    const int rem = (int)(mrow - nimg * hw);
                    const int yy = rem / p.Wout, xx = rem - yy * p.Wout;
                    const long orow = (nimg * (2L * p.Hout) + 2 * yy + p.up2_py) * (2L * p.Wout) + 2 * xx + p.up2_px;
                    if (ok) *(uint4*)((char*)yg + (orow * p.Cout + (co < cmax8 ? co : cmax8)) * 2) = o;
                } else if (ok) {
                    if (p.nt_store) __builtin_nontemporal_store(u32x4{o.x, o.y, o.z, o.w}, (u32x4*)(ybase + off * 2u));
                    else *(uint4*)(ybase + off * 2u) = o;
                }
            }
            if constexpr (EPI == 5) {
                // two lanes per row add up the row's pieces in a fixed order (deterministic, unlike atomics) and write the
                // wave slice's (sum, sum of squares) of the row: rs_out[row][Cout / (32 TN)][2]
                static_assert(PIECES % 2 == 0, "two lanes per row");
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int row = lane >> 1, half = lane & 1;
                float ss = 0.f, qq = 0.f;
#pragma unroll
                for (int j = 0; j < PIECES / 2; ++j) {
                    const int pc = half * (PIECES / 2) + j;
                    const f32x2 v = *(const f32x2*)(wlds + row * ROWB + ((pc ^ piece_xor(row, ROWB)) << 4));
                    ss += v.x;
                    qq += v.y;
                }
                ss += __shfl_xor(ss, 1);
                qq += __shfl_xor(qq, 1);
                const int slices = p.Cout / (TN * 32);
                if (half == 0 && row < rows)
                    *(f32x2*)(p.rs_out + ((mb + row) * slices + nw0 / (TN * 32)) * 2) = f32x2{ss, qq};
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();      // the next block overwrites the staging rows
        });
        if constexpr (GNS) {
            // this wave's staging rows are free: park the lane's 16 sums there ([lane][16] floats), then -- after a workgroup
            // barrier -- thread c of the tile adds up channel c over the waves that stored its rows (same wn, every wm) and
            // the RPR row-lanes of each, in a fixed order (deterministic), and writes the tile's (sum, sum of squares)
            float* st = (float*)wlds;
            if (lane < RPR * PIECES) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    st[lane * 16 + e] = gsum[e];
                    st[lane * 16 + 8 + e] = gsq[e];
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            constexpr int WM_ = NT / 64 / WN_, BNT = WN_ * TN * 32;
            const int c = wid_s * 64 + lane;
            if (c < BNT && n0 + c < p.Cout) {
                const int wn_c = c / (TN * 32), chunk = (c % (TN * 32)) / 8, e = c % 8;
                float ss = 0.f, qq = 0.f;
#pragma unroll
                for (int m = 0; m < WM_; ++m)
#pragma unroll
                    for (int r = 0; r < RPR; ++r) {
                        const float* src = (const float*)(lds + (m * WN_ + wn_c) * (32 * ROWB)) + (r * PIECES + chunk) * 16;
                        ss += src[e];
                        qq += src[8 + e];
                    }
                constexpr int BM_ = WM_ * TM * 32;
                float* dst = p.gn_out + (m0 / BM_) * 2 * (long)p.Cout + n0 + c;
                dst[0] = ss;
                dst[p.Cout] = qq;
            }
        }
        return;
    }
    // Cout not a multiple of 8 (conv_out's 4 channels, odd test shapes): stores straight from the fragments
    if constexpr (!COUT8) {
#pragma unroll
    for (int b = 0; b < TM; ++b) {
        const long m = m0 + wm * (TM * 32) + b * 32 + col;
        if (m >= p.M) continue;
        const long img = m / ((long)p.Hout * p.Wout);
        const T* trow = temb ? temb + (img / p.imgs_per_temb) * p.Cout : nullptr;
#pragma unroll
        for (int a = 0; a < TN; ++a) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = nw0 + a * 32 + 8 * g + 4 * hi;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (co + j < p.Cout) {
                        float vv = acc[a][b][4 * g + j];
                        if (bias) vv += to_f32(bias[co + j]);
                        if (trow) vv += to_f32(trow[co + j]);
                        if (res) vv += to_f32(res[m * p.Cout + co + j]);
                        yg[m * p.Cout + co + j] = from_f32<T>(vv);
                    }
                }
            }
        }
    }
    }
    }
}

// ---- persistent launches: one workgroup per CU (`per_cu` = 2: two), grid a multiple of 8 (XCDs)
static unsigned persistent_grid(long nblocks, int per_cu = 1) {
    static const int ncu = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
        return n >= 8 ? n / 8 * 8 : 8;
    }();
    const long want = (nblocks + 7) / 8 * 8, most = (long)per_cu * ncu;
    return (unsigned)(want < most ? want : most);
}

// ConvParams of a token-major Linear y[M, N] = x[M, K] w^T: a 1 x 1 convolution over an [M, 1, 1, K] view
static ConvParams linear_params(const void* x, const void* w_packed, void* y, int64_t M, int64_t K, int64_t N) {
    ConvParams p = conv_params_zero();
    p.x = x; p.w = w_packed; p.y = y;
    p.N = (int)M; p.Hin = 1; p.Win = 1; p.Cin = (int)K; p.Hout = 1; p.Wout = 1; p.Cout = (int)N; p.ntaps = 1;
    p.stride = 1; p.imgs_per_temb = 1;
    p.M = M;
    return p;
}

}  // namespace im360
