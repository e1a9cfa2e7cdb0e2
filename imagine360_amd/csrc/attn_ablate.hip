// Ablation-only launch rules of the attention family: compiled ONLY into `make ablate` builds (-DIM360_ABLATE; im360_build_flags() bit 0), by
// inclusion from attn_fwd.hip and attn_pipe.hip INSIDE their `namespace im360`, behind the kernels and launch helpers used here (attn_fwd.hip:
// the variant tags, launch_variant; attn_pipe.hip: attn_pipe_kernel).  The default build gets the ablate_*() hooks as constant "not taken".
// Compiled on its own this file is an empty translation unit.  The kernels' ablation paths themselves are template parameters of
// attn_fwd_kernel (BL, DS, ABL, HG) and attn_pipe_kernel (ABL) and stay where the kernels are.

#ifdef IM360_ATTN_FWD_INCLUDES_ABLATE
// Rejected / ablation variants (knobs attn_dbg, attn_hl, attn_hg, attn_ds, attn_w3 = 2) are compiled only into `make ablate`
// builds (-DIM360_ABLATE; im360_build_flags() bit 0): in the shipped library those knobs read as 0.
#ifdef IM360_ABLATE
#define IM360_ABL_KNOB(k) knob(k)
#else
#define IM360_ABL_KNOB(k) 0
#endif
// ablation knobs that keep a launch off the three-waves-per-SIMD rule / off the pipelined kernel
static inline bool ablate_no_w3(int qb_env) { return IM360_ABL_KNOB(KNOB_ATTN_DBG) != 0 || (qb_env == 1 && IM360_ABL_KNOB(KNOB_ATTN_DS)); }
static inline bool ablate_no_pipe() { return IM360_ABL_KNOB(KNOB_ATTN_DBG) != 0; }

#ifdef IM360_ABLATE
struct PackedThreeWaves : PackedBias { static constexpr bool three_waves = true, four_waves_only = true; };
struct PackedBiasLds : PackedBias { static constexpr bool bias_lds = true, four_waves_only = true; };
struct PackedHeadGroups : PackedBias { static constexpr bool head_groups = true, four_waves_only = true; };
struct PackedDotSums : PackedBias { static constexpr bool dot_sums = true, four_waves_only = true; };
template <bool HAS_BIAS> struct DotSums : Plain<HAS_BIAS> { static constexpr bool dot_sums = true, four_waves_only = true; };
template <int ABL> struct Ablated : AttnVariant { static constexpr int abl = ABL; static constexpr bool four_waves_only = true; };

// ---- "does an ablation variant take this launch?" -- asked by launch_attn_b for four-wave launches, in front of its shipped kernel of the same
// path; true: launched (or failed), status in rc.  p.nqt and the grid are set, qb = query blocks per wave
// packed bias, d = 32
template <typename T>
static bool ablate_packed(const AttnParams& p, dim3 grid, int qb, hipStream_t stream, int& rc) {
    if (qb == 1) {
        if (knob(KNOB_ATTN_W3) != 2) return false;
        rc = launch_variant<T, 32, 1, PackedThreeWaves>(p, grid, 4, stream);      // A/B (attn_qb 1 + attn_w3 2): WarpAttn with one block per wave at three waves per SIMD -- 1.13 ms against 0.98 for the two-block form (which shares every K fragment and mask prefetch between its blocks) and 1.25 at two waves: off
    }
    else if (knob(KNOB_ATTN_HL) == 2) rc = launch_variant<T, 32, 2, PackedBiasLds>(p, grid, 4, stream);      // A/B: mask rows through the wave's LDS patch (measured 6 % slower: the divergent fragment loads are not the limiter)
    else if (knob(KNOB_ATTN_HG) && ((long)p.B * p.H) % 4 == 0 && (long)p.B * p.H * ((p.Nq + 63) / 64) / 4 <= 0x7fffffffL) {
        // head groups: four (batch, head) pairs per workgroup over the same 64 query rows
        dim3 hgrid((unsigned)((long)p.B * p.H / 4 * ((p.Nq + 63) / 64)), 1, 1);
        rc = launch_variant<T, 32, 2, PackedHeadGroups>(p, hgrid, 4, stream);
    }
    else if (knob(KNOB_ATTN_DS)) rc = launch_variant<T, 32, 2, PackedDotSums>(p, grid, 4, stream);
    else return false;
    return true;
}

// no bias, or a bias read as 16-bit rows
template <typename T, int D, bool HAS_BIAS>
static bool ablate_plain(const AttnParams& p, dim3 grid, int qb, hipStream_t stream, int& rc) {
    if (qb == 1) {
        if (!knob(KNOB_ATTN_DS)) return false;
        rc = launch_variant<T, D, 1, DotSums<HAS_BIAS>>(p, grid, 4, stream);
        return true;
    }
    if (!HAS_BIAS && D == 64 && knob(KNOB_ATTN_DBG)) {
        if constexpr (!HAS_BIAS && D == 64) {
            auto launch = [&](auto a) { rc = launch_variant<T, D, 2, Ablated<decltype(a)::value>>(p, grid, 4, stream); };
            if (!with_const<1, 2, 4, 6, 7, 8>(knob(KNOB_ATTN_DBG), launch)) launch(std::integral_constant<int, 15>{});
        }
        return true;
    }
    if (!knob(KNOB_ATTN_DS)) return false;
    rc = launch_variant<T, D, 2, DotSums<HAS_BIAS>>(p, grid, 4, stream);
    return true;
}

#else   // the default build has no ablation variants

template <typename T> static bool ablate_packed(const AttnParams&, dim3, int, hipStream_t, int&) { return false; }
template <typename T, int D, bool HAS_BIAS> static bool ablate_plain(const AttnParams&, dim3, int, hipStream_t, int&) { return false; }

#endif  // IM360_ABLATE
#endif  // IM360_ATTN_FWD_INCLUDES_ABLATE

#ifdef IM360_ATTN_PIPE_INCLUDES_ABLATE
#ifdef IM360_ABLATE

// knob attn_pipe bits 8-11 -> attn_pipe_kernel's ABL bits (schedule 0, read-ahead 2); [12] = every other value
constexpr int PIPE_ABL[13] = {
    0,
    65 + 32 + 16 + 256,      // MFMA + V reads + waits only
    65 + 32 + 16 + 512,      // MFMA + K reads + waits only
    65 + 32 + 16 + 1024,     // MFMA + all reads at lane-linear addresses
    1024,                    // everything, reads at lane-linear addresses
    65 + 32 + 16 + 8,        // MFMA only
    6 + 32 + 16,      // VALU + reads + waits only
    128,              // reads issued, never waited for
    128 + 32,         // ... and no staging
    32 + 16,          // reads and waits, no staging, no barrier
    65,
    65 + 32 + 16,    // MFMA + reads + waits only
    65 + 128 + 32 + 16,   // MFMA + reads, no waits
};

// launch_nw: q.nqt, the grid and the block are set; abl = the knob's ablation bits.  true: launched (or failed), status in rc
template <typename T, int NW>
static bool ablate_pipe(const AttnParams& q, dim3 grid, dim3 block, int abl, hipStream_t stream, int& rc) {
    if (!(abl && NW != 12)) return false;
    with_const<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12>(abl > 12 ? 12 : abl, [&](auto a) {
        hipLaunchKernelGGL((attn_pipe_kernel<T, NW, 0, 2, PIPE_ABL[decltype(a)::value]>), grid, block, 0, stream, q);
    });
    rc = im360_launch_status();
    return true;
}

#else   // the default build has no ablation variants

template <typename T, int NW> static bool ablate_pipe(const AttnParams&, dim3, dim3, int, hipStream_t, int&) { return false; }

#endif  // IM360_ABLATE
#endif  // IM360_ATTN_PIPE_INCLUDES_ABLATE
