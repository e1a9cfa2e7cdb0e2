/* libim360_kernels.so -- C ABI of the MI355X (gfx950) kernels behind imagine360_amd.
 *
 * The reference (3DTopia/Imagine360) has no FFI: its arithmetic for this path lives in third-party
 * wheels (torch ATen / cuDNN, xformers).  Each entry point below therefore cites the reference call
 * site(s) whose kernel it replaces (paths relative to the reference repository).  Conventions:
 *   - plain device pointers + int64 sizes/strides (in ELEMENTS), no torch types;
 *   - dtype: 0 = bfloat16, 1 = float16 (16-bit storage, fp32 accumulation);
 *   - every function only enqueues work on `stream` (a hipStream_t); no allocation, no sync;
 *   - returns 0, or a negative code with a message available from im360_last_error().
 * Activations are channels-last: images [N, H, W, C] where N = (batch x frame), tokens [B, N, C].
 */
#ifndef IM360_KERNELS_H
#define IM360_KERNELS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 5 since round 6 (3: packed-bias block maps of im360_attn_fwd; 4: im360_groupnorm_partial_pad / im360_groupnorm_apply_partials added;
 * 5: im360_conv_ksplit_plan / im360_conv_fwd_ksplit added).
 * 2 since round 5: im360_conv_fwd / im360_linear_fwd take a trailing gn_partial pointer and the table rows of
 * im360_linear_ln_fwd include c2 (both introduced in round 4 under version 1).  imagine360_amd/kernels.py refuses a mismatch. */
int im360_abi_version(void);
/* bit 0: ablation build (`make ablate`): the rejected A/B kernel variants behind the attn_dbg / attn_hl / attn_hg / attn_ds knobs exist */
int im360_build_flags(void);
const char* im360_last_error(void);

/* softmax(Q K^T * scale + bias) V, head dim D in {32, 64}; head h of batch b lives at
 * base + b*bs + row*rs + h*D.  bias (optional) is ONE [Nq, Nk] matrix shared by all (b, h).
 * accumulate != 0: out += out_scale * result (second KV set of the IP cross attention).
 * bias_alt / bias_sel (optional): a second [Nq, Nk] bias and a device int32; the kernel uses bias_alt when
 *   *bias_sel != 0 (WarpAttn's normal / antipodal mask choice made on the device, so a step can be graph-replayed).
 * kv_group: K/V batch index = query batch index / kv_group (one context per video, F frames of queries).
 * dtype: 0 bf16, 1 fp16; + 256 (D = 32 only, Nk % 8 == 0): bias and bias_alt are fp16 matrices already multiplied by
 *   log2(e) (im360_attn_pack_bias) and are added to the scores by the matrix pipe instead of the vector ALU.
 * bias_blocks / bias_blocks_alt (optional, packed bias only; ABI version 3): block maps of bias / bias_alt -- uint32 words
 *   [ceil(Nq / 32)][blocks_rs], bit (h % 32) of word (h / 32) of row r clear = every entry of the 32 x 32 block (queries 32 r ..,
 *   keys 32 h ..) of the packed matrix is ZERO; the kernel skips such a block's mask loads and mask MFMAs (identical results: they
 *   would add zeros).  The caller makes the common value of a mask zero by subtracting it from the whole matrix -- softmax is
 *   invariant under a per-row constant (WarpAttn: ~ 80 - 90 % of the blocks are background).
 * Replaces: xformers.ops.memory_efficient_attention / F.scaled_dot_product_attention at
 *   diffusers/models/attention_processor.py:1264, 1351, 641 (spatial self / cross attention),
 *   animatediff/models/attention.py:113-148 (text + IP cross attention),
 *   src/modules/transformer.py:72 (WarpAttn cross-view attention with additive mask). */
int im360_attn_fwd(const void* q, const void* k, const void* v, const void* bias, void* out,
                   int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t D,
                   int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs,
                   int64_t v_bs, int64_t v_rs, int64_t o_bs, int64_t o_rs, int64_t bias_rs,
                   int64_t kv_group, float scale, float out_scale, int accumulate, int dtype, void* stream,
                   const void* bias_alt, const void* bias_sel,
                   const void* bias_blocks, const void* bias_blocks_alt, int64_t blocks_rs);

/* out_f16[i] = fp16(clamp(bias[i] * log2(e), -60000, 60000)) for the n elements of a bias matrix of dtype 0 / 1: the packed
 * form accepted by im360_attn_fwd with dtype + 256.  The packed entries must be FINITE (the kernel adds them with an
 * identity-slice MFMA, where 0 * inf would poison the whole score block): this function guarantees it by clamping, so -inf
 * masks are usable (weight exactly 0).  Done once per (resolution, camera rig) -- WarpAttn's masks are cached. */
int im360_attn_pack_bias(const void* bias, void* out_f16, int64_t n, int dtype, void* stream);

/* Two key / value sets for the same queries in one launch (head dim 64, no bias):
 *   out = out_scale * softmax(q k^T scale) v + out_scale2 * softmax(q k2^T scale) v2
 * -- the text tokens and the IP-adapter tokens of the spatial cross attention, which the reference evaluates as two
 * attention calls and an add.  Strides / kv_group as in im360_attn_fwd.  With 65..96 + 33..64 keys, Nq % 32 == 0 and 16-byte
 * aligned output rows (the model's 77 + 64 tokens) the launch keeps BOTH sets resident in LDS per (video, head) and streams the
 * query blocks of all the video's frames past them (knob 11); other shapes take the generic two-pass kernel.
 * Replaces: IPCrossAttention.forward, animatediff/models/attention.py:113-148. */
int im360_attn_fwd2(const void* q, const void* k, const void* v, const void* k2, const void* v2, void* out,
                    int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t Nk2, int64_t D,
                    int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs, int64_t v_bs, int64_t v_rs,
                    int64_t k2_bs, int64_t k2_rs, int64_t v2_bs, int64_t v2_rs, int64_t o_bs, int64_t o_rs,
                    int64_t kv_group, float scale, float out_scale, float out_scale2, int dtype, void* stream);

/* Temporal self-attention over F <= 64 frames on token-major activations [B, F, P, heads*d]
 * (q, k, v are three views with common strides, e.g. slices of a fused QKV projection).
 * Replaces: VersatileAttention.forward -> Attention._attention (baddbmm/softmax/bmm) and its
 *   '(b f) d c <-> (b d) f c' rearranges, animatediff/models/motion_module.py:343-429,
 *   diffusers/models/attention_processor.py:562-591. */
int im360_temporal_attn_fwd(const void* q, const void* k, const void* v, void* out,
                            int64_t B, int64_t F, int64_t P, int64_t heads, int64_t d,
                            int64_t qkv_fs, int64_t qkv_ps, int64_t qkv_bs,
                            int64_t o_fs, int64_t o_ps, int64_t o_bs,
                            float scale, int dtype, void* stream);

/* Window-fused temporal self-attention: the F <= 64 frames are attended as nW sliding windows of L <= 16 consecutive frames
 * (window k: frames starts[k] + p, modulo F when `ring`, at positions p = 0 .. L-1) and the windows' attention outputs are
 * fused per frame, weighted by weights[p] over the sum of the weights of the windows that cover the frame -- FreeNoise's
 * window-based attention fusion (arXiv 2310.15169, section 3.2).  q, k, v: the fused projection WITHOUT the frame PE;
 * pe_qkv [L, 3 * heads * d] (contiguous): PE rows 0 .. L-1 through the same projection; a window row is
 * round(q|k|v[frame] + pe_qkv[p]) in the activation dtype.  One launch: q, k, v are read once, every output element is
 * written once (fp32 fusion, rounded once), no per-window intermediate goes to HBM.  `starts` (nW <= 64) and `weights` (L,
 * positive) are HOST arrays, copied into the launch: every start in [0, F), start + L <= F unless `ring`, every frame
 * covered, L <= F; d % 8 == 0; strides and alignment as in im360_temporal_attn_fwd.
 * Replaces: nothing in the reference (it attends over the whole clip, motion_module.py:343-429); call site:
 *   imagine360_amd.unet3d.VersatileAttention.forward with windows set (context.windowed_temporal_attention is the
 *   eager definition). */
int im360_temporal_attn_windows_fwd(const void* q, const void* k, const void* v, const void* pe_qkv, void* out,
                                    int64_t B, int64_t F, int64_t P, int64_t heads, int64_t d,
                                    int64_t qkv_fs, int64_t qkv_ps, int64_t qkv_bs,
                                    int64_t o_fs, int64_t o_ps, int64_t o_bs,
                                    const int32_t* starts, int64_t nW, const float* weights, int64_t L, int ring,
                                    float scale, int dtype, void* stream);

/* Frame-chunk sharding (one process per GPU, imagine360_amd.dist.FrameShard): frame-sharded tokens [B, Fl, P, C] (16-bit,
 * C % 8 == 0) <-> the buffer of the frame <-> pixel all-to-all, [W][Fl][B][PP][C] (W ranks, PP = ceil(P / W), the tail of
 * the last rank zero-filled); dir 0 packs, 1 unpacks.  The receive side of the exchange is read IN PLACE by
 * im360_temporal_attn_fwd through its frame / batch / pixel strides (frame stride B * PP * C), which also writes the
 * return trip's send buffer directly.  Pre-sized caller-owned buffers: the exchange can be captured in a hipGraph.
 * Replaces: nothing in the reference (single process); it surrounds VersatileAttention, motion_module.py:343-429. */
int im360_shard_pack(const void* src, void* dst, int64_t B, int64_t Fl, int64_t P, int64_t C, int64_t W, int64_t PP,
                     int dir, void* stream);

/* GroupNorm statistics -> per-(image, channel) fp32 scale/shift such that GN(x) = x*scale + shift.
 * pad > 0: statistics of the circularly W-padded tensor (the pano branch pads before norm1,
 * src/models/MVGenModel.py:277-278).  partial: fp32 workspace of N * S * 2 * C floats,
 * S = im360_gn_num_slabs(N, H, W).
 * Replaces: nn.GroupNorm / InflatedGroupNorm statistics, animatediff/models/resnet.py:9-17, 224, 236;
 *   animatediff/models/attention.py:262; motion_module.py:169; unet.py (conv_norm_out); VAE norms. */
int64_t im360_gn_num_slabs(int64_t N, int64_t H, int64_t W);
int im360_groupnorm_stats(const void* x, const void* gamma, const void* beta, void* partial,
                          void* scale, void* shift, int64_t N, int64_t H, int64_t W, int64_t C,
                          int64_t G, int64_t pad, float eps, int dtype, void* stream);

/* y[N, H, W + 2 pad, C] = act(x * scale + shift) with circular W addressing; act 0 = none, 1 = SiLU.
 * Replaces: the normalise + F.silu pass (resnet.py:224-225, 236-243) fused with pad_pano
 *   (src/utils/pano.py:75-95). */
/* Partial sums only: partial fp32 [N][S][2][C], S = im360_gn_num_slabs(N, H, W) (no pad weighting). */
int im360_groupnorm_partial(const void* x, void* partial, int64_t N, int64_t H, int64_t W, int64_t C, int dtype, void* stream);
/* scale / shift [N, C1 + C2] from partial sums of one or two channel ranges: [0, C1) from pa ([N][Sa][2][C1]), [C1, C1 + C2)
 * from pb ([N][Sb][2][C2], null with C2 = 0).  Either may come from im360_groupnorm_partial or from the epilogue of the
 * kernel that produced that tensor (gn_partial of im360_conv_fwd / im360_linear_fwd).  pixels = H * W per image. */
int im360_groupnorm_finalize(const void* pa, int64_t Sa, int64_t C1, const void* pb, int64_t Sb, int64_t C2, const void* gamma,
                             const void* beta, void* scale, void* shift, int64_t N, int64_t G, int64_t pixels, float eps,
                             int dtype, void* stream);
int im360_groupnorm_apply(const void* x, const void* scale, const void* shift, void* y,
                          int64_t N, int64_t H, int64_t W, int64_t C, int64_t pad, int act,
                          int dtype, void* stream);

/* Round 6 (ABI version 4) -- the normalisation straight from PARTIAL SUMS, one launch: no finalize kernel, no scale / shift tensors.
 * im360_groupnorm_partial_pad: im360_groupnorm_partial with the circular-pad weighting of im360_groupnorm_stats (the `pad` wrapped
 *   columns count twice; src/models/MVGenModel.py:277-278).
 * im360_groupnorm_apply_partials: y [N, H, W + 2 pad, C1 + C2] = act(GroupNorm([xa | xb])); the statistics of channels [0, C1)
 *   come from pa ([N][Sa][2][C1]), those of [C1, C1 + C2) from pb ([N][Sb][2][C2]); xb / pb null with C2 = 0.  Every workgroup
 *   rebuilds scale / shift of its image from the partial sums (the reduction order, and the bits, of im360_groupnorm_finalize).
 * Replaces: InflatedGroupNorm / nn.GroupNorm (+ F.silu, + pad_pano, + torch.cat([x, skip])), animatediff/models/resnet.py:9-17,
 *   221-243; animatediff/models/attention.py:206, 262; motion_module.py:128, 169; src/models/MVGenModel.py:407-437. */
int im360_groupnorm_partial_pad(const void* x, void* partial, int64_t N, int64_t H, int64_t W, int64_t C, int64_t pad, int dtype,
                                void* stream);
int im360_groupnorm_apply_partials(const void* xa, const void* xb, const void* pa, int64_t Sa, const void* pb, int64_t Sb,
                                   const void* gamma, const void* beta, void* y, int64_t N, int64_t H, int64_t W, int64_t C1,
                                   int64_t C2, int64_t G, int64_t pad, float eps, int act, int dtype, void* stream);

/* The two GroupNorm passes on the channel concatenation [xa | xb] (xa [N, H, W, C1], xb [N, H, W, C2]) WITHOUT
 * materialising it: gamma / beta / scale / shift / y span C1 + C2 channels, partial holds N * S * 2 * (C1 + C2) floats.
 * Replaces: torch.cat([x, skip], dim=1) -> ResnetBlock3D.norm1 in the decoder, src/models/MVGenModel.py:407, 415, 431,
 *   437 -> animatediff/models/resnet.py:221-225. */
int im360_groupnorm_stats_cat(const void* xa, const void* xb, const void* gamma, const void* beta, void* partial,
                              void* scale, void* shift, int64_t N, int64_t H, int64_t W, int64_t C1, int64_t C2,
                              int64_t G, int64_t pad, float eps, int dtype, void* stream);
int im360_groupnorm_apply_cat(const void* xa, const void* xb, const void* scale, const void* shift, void* y,
                              int64_t N, int64_t H, int64_t W, int64_t C1, int64_t C2, int64_t pad, int act,
                              int dtype, void* stream);

/* The whole GroupNorm (+ SiLU, + circular W pad; on x or on the never-materialised concatenation [xa | xb], xb may be null
 * with C2 = 0) in ONE launch: per-slab partial sums, a per-image arrival counter, every workgroup reduces its image's
 * partials in the fixed order of the two-kernel path (same bits) and normalises its slab -- whose second read comes out of
 * the L2 / Infinity Cache microseconds after the first: 2 HBM passes instead of 3.  partial: N * S * 2 * (C1 + C2) floats
 * with S = im360_gn_num_slabs(N, H, W); counter: N int32 (zeroed by the call, on the stream).
 * Replaces: InflatedGroupNorm / nn.GroupNorm + F.silu + pad_pano, animatediff/models/resnet.py:9-17, 221-243;
 *   attention.py:262; motion_module.py:169; unet.py conv_norm_out; src/utils/pano.py:75-95. */
int im360_groupnorm_fused(const void* xa, const void* xb, const void* gamma, const void* beta, void* partial, void* counter,
                          void* y, int64_t N, int64_t H, int64_t W, int64_t C1, int64_t C2, int64_t G, int64_t pad,
                          float eps, int act, int dtype, void* stream);

/* 3x3 (ntaps = 9) or 1x1 (ntaps = 1) convolution, implicit GEMM on MFMA.  x [N, Hin, Win, Cin],
 * y [N, Hout, Wout, Cout], w_packed from im360_pack_conv_weight.  stride 1|2; up: input is
 * nearest-upsampled x2 on the fly; wrap: circular W addressing; x_off / y_off: column / row offset of the
 * taps (pre-padded input; the VAE downsampler's (0,1,0,1) padding is x_off = y_off = 1).  Epilogue: + bias[Cout] + temb[n / imgs_per_temb][Cout] + res[N, Hout, Wout, Cout].
 * Replaces: InflatedConv3d / nn.Conv2d at animatediff/models/resnet.py:19-27, 84, 128, 183, 205, 218,
 *   227-251; unet.py:134-137, 358; pad_pano/unpad_pano around them (MVGenModel.py:138-143, 276-281,
 *   305-314, 449-456, 474-478); F.interpolate nearest (resnet.py:104); the VAE convs. */
int im360_conv_fwd(const void* x, const void* w_packed, const void* bias, const void* temb,
                   const void* res, void* y,
                   int64_t N, int64_t Hin, int64_t Win, int64_t Cin,
                   int64_t Hout, int64_t Wout, int64_t Cout, int64_t ntaps,
                   int64_t stride, int64_t up, int64_t wrap, int64_t x_off, int64_t y_off,
                   int64_t imgs_per_temb, int dtype, void* stream, void* gn_partial);
/* gn_partial (optional; last argument of im360_conv_fwd / im360_linear_fwd): the epilogue also writes per 256-pixel tile and
 * output channel (sum, sum of squares) of the stored values, fp32 [M / 256][2][Cout] -- GroupNorm partial sums with one slab
 * per tile, consumed by im360_groupnorm_finalize in place of a statistics pass over the tensor
 * (animatediff/models/resnet.py:221-243 is norm -> SiLU -> conv twice).  Only launches for which im360_conv_gn_slabs
 * returns S > 0 (slabs per image) can do it. */
int64_t im360_conv_gn_slabs(int64_t N, int64_t Hout, int64_t Wout, int64_t Cin, int64_t Cout, int64_t ntaps);

/* K-split of a 3x3 convolution launch (ABI version 5): every 256 x 320 output tile is computed by `parts` workgroups, each over a
 * contiguous range of the 64-channel chunks of K; parts 0 .. parts - 2 park their fp32 accumulators in ks_ws, the last one (dispatched
 * behind them) adds them in part order and runs the usual epilogue.  For launches whose tile count is not a whole number of rounds
 * of the chip's 256 CUs (perspective level 2 of cfg2: 640 tiles = 2.5 rounds) or below one round (level 3: 160 tiles).
 * im360_conv_ksplit_plan: parts this launch would run in (1 = none: call im360_conv_fwd; knob conv_ksplit 0 = never).
 * im360_conv_fwd_ksplit: im360_conv_fwd + the scratch: ks_ws >= tiles x (parts - 1) x 327 680 bytes (tiles = ceil(N Hout Wout / 256)
 * x Cout / 320), ks_cnt = `tiles` int32 counters, ZERO on entry and zero again on return.  Deterministic; not bit-identical to the
 * unsplit launch (another order of the fp32 partial sums).  Same call sites as im360_conv_fwd (animatediff/models/resnet.py:19-27). */
int64_t im360_conv_ksplit_plan(int64_t N, int64_t Hout, int64_t Wout, int64_t Cin, int64_t Cout, int64_t ntaps,
                               int64_t up, int64_t wrap, int64_t gn_stats);
int im360_conv_fwd_ksplit(const void* x, const void* w_packed, const void* bias, const void* temb,
                          const void* res, void* y,
                          int64_t N, int64_t Hin, int64_t Win, int64_t Cin,
                          int64_t Hout, int64_t Wout, int64_t Cout, int64_t ntaps,
                          int64_t stride, int64_t up, int64_t wrap, int64_t x_off, int64_t y_off,
                          int64_t imgs_per_temb, int dtype, void* stream, void* gn_partial,
                          void* ks_ws, int64_t ks_ws_bytes, void* ks_cnt, int64_t ks_cnt_n);

/* 1x1 convolution of the channel concatenation [xa | xb] without materialising it: the K loop reads channels [0, C1)
 * from xa and [C1, C1 + C2) from xb (C1, C2 multiples of 64); w_packed [CoutPad][1][C1 + C2]; + bias + res.
 * Replaces: ResnetBlock3D.conv_shortcut on torch.cat([x, skip]), animatediff/models/resnet.py:248-249 after
 *   src/models/MVGenModel.py:407, 415, 431, 437. */
int im360_conv1x1_cat_fwd(const void* xa, const void* xb, const void* w_packed, const void* bias, const void* res,
                          void* y, int64_t N, int64_t H, int64_t W, int64_t C1, int64_t C2, int64_t Cout,
                          int dtype, void* stream);

/* Nearest-x2 upsample followed by conv3x3 (pad 1; wrap: circular along W), computed as four 2 x 2 convolutions of the
 * LOW-resolution input, one per output parity: after the upsample output pixel (2y + py, 2x + px) sees only the 2 x 2 source
 * pixels (y + r + py - 1, x + c + px - 1), so the nine taps collapse into four pre-summed ones -- 4 / 9 of the MACs.
 * x [N, Hin, Win, Cin] (Cin % 64 == 0) -> y [N, 2 Hin, 2 Win, Cout]; w4 = four im360_pack_conv_weight outputs (taps = 4,
 * [CoutPad][4][Cin] each) back to back in parity order (0,0) (0,1) (1,0) (1,1).  The pre-summed weights are rounded to
 * 16 bits once more than the reference's (a stated deviation).
 * Replaces: Upsample3D = F.interpolate(scale 2, nearest) + InflatedConv3d (animatediff/models/resnet.py:71-114), incl. the
 *   pano branch's pad_pano -> upsample -> unpad_pano sandwich (MVGenModel.py). */
int im360_conv_up2_fwd(const void* x, const void* w4, const void* bias, void* y, int64_t N, int64_t Hin,
                       int64_t Win, int64_t Cin, int64_t Cout, int64_t wrap, int dtype, void* stream);

/* PyTorch conv weight [Cout, Cin, kh, kw] -> [CoutPad (mult. of 128)][kh*kw][CinPad (mult. of 32)]. */
int im360_pack_conv_weight(const void* w, void* out, int64_t Cout, int64_t Cin, int64_t taps,
                           int64_t CoutPad, int64_t CinPad, int dtype, void* stream);

/* x [rows, W, C] -> y [rows, W + 2 pad, C], circular along W.
 * Replaces: pad_pano on the latent before VAE decode, pipeline_animation_inference_dual.py:813. */
int im360_circular_pad_w(const void* x, void* y, int64_t rows, int64_t W, int64_t C, int64_t pad,
                         int dtype, void* stream);

/* x [N, H, W] (W last, elements of esize = 1 / 2 / 4 / 8 bytes) -> y [N, H + top + bottom, W + left + right], circular in
 * both axes = torch.nn.functional.pad(x, (left, right, top, bottom), mode="circular"); each pad <= the size of its axis.
 * Replaces: the 360-degree close-loop patch of the super-resolution stage -- padding_pano / pad_pano on NCHW video and
 *   latent tensors and the circular pad_to_fit, sr/video_to_video_model.py:16-29, 99, 160-162; src/utils/pano.py:75-95. */
int im360_circular_pad_hw(const void* x, void* y, int64_t N, int64_t H, int64_t W, int64_t left, int64_t right,
                          int64_t top, int64_t bottom, int64_t esize, void* stream);

/* out = cx * x + cv * (uncond + guidance * (cond - uncond)); cx, cv = DDIM v-prediction coefficients;
 * coef_dev (optional): device float[3] = (guidance, cx, cv) overriding the scalars (hipGraph replay).
 * Replaces: the CFG combine + DDIMScheduler.step elementwise chain,
 *   pipeline_animation_inference_dual.py:791-800; diffusers/schedulers/scheduling_ddim.py:300-350. */
int im360_cfg_ddim_update(const void* uncond, const void* cond, const void* x, void* out, int64_t n,
                          float guidance, float cx, float cv, int dtype, void* stream, const void* coef_dev);

/* The full DDIMScheduler.step on the CFG combination m = uncond + guidance * (cond - uncond), per element in fp32:
 *   mode bits 0-1: prediction type (0 epsilon: x0 = (x - sqrt_b m) / sqrt_a, e = m;  1 v_prediction: x0 = sqrt_a x - sqrt_b m,
 *   e = sqrt_a m + sqrt_b x;  2 sample: x0 = e = m);  bit 2: clip_sample (x0 clamped to [-1, 1]);  bit 3:
 *   use_clipped_model_output (e = (x - sqrt_a x0) / sqrt_b);
 *   out = sqrt_a_prev * x0 + dir * e + sigma * noise, dir = sqrt(1 - a_prev - sigma^2), sigma = eta * sqrt(variance).
 * noise (optional, same shape and dtype): null means zero noise, refused with sigma > 0 unless coef_dev is given.
 * coef_dev (optional): device float[6] = (guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma) overriding the scalars (hipGraph replay).
 * Replaces: the CFG combine + DDIMScheduler.step with eta > 0, clip_sample or use_clipped_model_output,
 *   pipeline_animation_inference_dual.py:791-800; diffusers/schedulers/scheduling_ddim.py:251-373. */
int im360_cfg_ddim_step(const void* uncond, const void* cond, const void* x, const void* noise, void* out, int64_t n,
                        float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode,
                        int dtype, void* stream, const void* coef_dev);

/* im360_cfg_ddim_step on the per-frame blend of sliding temporal context windows (imagine360_amd/context.py).  x / noise / out
 * are viewed as [outer, F, inner] (panorama latent [1,4,F,H,W]: outer 4, inner H*W; perspective latent [1,m,4,F,h,w]: outer 4m,
 * inner h*w).  pred holds the predictions of all nW windows in one buffer [nW, 2, outer, L, inner] (window, CFG half: uncond then
 * cond, then the model's own layout), same 16-bit dtype.  start: device int32[nW], ascending window start frames, 0 <= start[k]
 * <= F - L, every frame covered;  weight: device float[L], positive.  Per element at frame f, in fp32,
 *   m = (sum_k weight[f - start[k]] * (u_k + guidance * (c_k - u_k))) / (sum_k weight[f - start[k]])
 * over the windows with start[k] <= f < start[k] + L, k ascending (fixed order: deterministic), then the step of
 * im360_cfg_ddim_step on m (same mode word, same six coefficients, same optional coef_dev[6]); one rounding, at the store.
 * 16-byte lanes when inner % 8 == 0 and the tensors are 16-byte aligned, a scalar path otherwise.  nW = 1, start = {0}, weight
 * all 1, L = F gives im360_cfg_ddim_step's result bit for bit.
 * Replaces: nothing in the reference (it has no temporal windows); composes the CFG combine + DDIMScheduler.step of
 *   pipeline_animation_inference_dual.py:771-800 over several forwards. */
int im360_cfg_ddim_step_windows(const void* pred, const void* x, const void* noise, void* out, const void* start,
                                const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float guidance,
                                float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, int dtype,
                                void* stream, const void* coef_dev);

/* ---- guidance rescale (arXiv 2305.08891, section 3.4) inside the CFG + DDIM step: the step sees m' = r * m instead of
 * m = uncond + guidance * (cond - uncond), with one scalar per tensor
 *   r = phi * std(cond) / std(m) + (1 - phi),   std = torch.std (correction 1) over all n elements, m formed in fp32.
 * Two launches per step, no host read, no atomics, no counter: a statistics pass writes one record of partial moments
 * (count, mean and M2 = sum (v - mean)^2 of cond and of m; 8 floats, five used) per workgroup into ws, and every workgroup of the
 * step kernel merges all records itself with Chan's formula in one fixed order, so all of them use the same bits and the result is
 * bit-identical from run to run.  std(m) = 0 or n = 1 give inf / NaN, as the formula does. ---- */

/* Number of records the statistics pass writes for n elements (= its grid: one workgroup per 256 groups of 8 elements, at most
 * 256): ws must hold 8 * im360_cfg_rescale_records(n) floats.  Host code. */
int64_t im360_cfg_rescale_records(int64_t n);

/* Statistics pass over cond and m = uncond + guidance * (cond - uncond): n elements (n % 8 == 0, 16-byte aligned), both tensors
 * of the same 16-bit dtype; ws: device float[ws_floats], ws_floats >= 8 * im360_cfg_rescale_records(n).  coef_dev (optional):
 * device float[>= 1] whose element 0 overrides guidance (the coefficient buffer of the step: hipGraph replay).
 * Replaces: nothing in the reference (its pipeline has no guidance_rescale); the std reductions of diffusers' rescale_noise_cfg. */
int im360_cfg_rescale_stats(const void* uncond, const void* cond, int64_t n, float guidance, void* ws, int64_t ws_floats,
                            int dtype, void* stream, const void* coef_dev);

/* The same over the per-frame blends of sliding context windows: layout, tables and preconditions of
 * im360_cfg_ddim_step_windows; m is that entry point's blend, cond is blended with the same weights in the same order,
 *   c = (sum_k weight[f - start[k]] * c_k) / (sum_k weight[f - start[k]]),
 * and the moments span the whole clip [outer, F, inner].  nW = 1, start = {0}, weight all 1, L = F writes the records of
 * im360_cfg_rescale_stats bit for bit (for any inner).
 * Replaces: nothing in the reference (no temporal windows, no guidance_rescale). */
int im360_cfg_rescale_stats_windows(const void* pred, const void* start, const void* weight, int nW, int64_t outer, int64_t F,
                                    int64_t L, int64_t inner, float guidance, void* ws, int64_t ws_floats, int dtype,
                                    void* stream, const void* coef_dev);

/* out[0] (device float) = r from the records a statistics pass over n elements left in ws: one workgroup making the merge every
 * workgroup of the step kernels makes (the same bits).  For tests and tools; phi must be finite.
 * Replaces: nothing in the reference. */
int im360_cfg_rescale_factor(const void* ws, int64_t ws_floats, int64_t n, float phi, void* out, void* stream);

/* im360_cfg_ddim_step on r * m: same arguments, mode word, six coefficients, optional noise and coef_dev[6]; phi (finite) and the
 * records im360_cfg_rescale_stats wrote into ws for the same uncond / cond / n / guidance (ws_floats as there).
 * Replaces: nothing in the reference; diffusers' rescale_noise_cfg between the CFG combine and DDIMScheduler.step. */
int im360_cfg_ddim_step_rescale(const void* uncond, const void* cond, const void* x, const void* noise, void* out, int64_t n,
                                float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode,
                                float phi, const void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_ddim_step_windows on r * m, r from the records of im360_cfg_rescale_stats_windows over the same clip.  One uniform
 * window with L = F gives im360_cfg_ddim_step_rescale's result bit for bit.
 * Replaces: nothing in the reference. */
int im360_cfg_ddim_step_windows_rescale(const void* pred, const void* x, const void* noise, void* out, const void* start,
                                        const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner,
                                        float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma,
                                        int mode, float phi, const void* ws, int64_t ws_floats, int dtype, void* stream,
                                        const void* coef_dev);

/* ---- the windows of a looping clip: im360_cfg_ddim_step_windows with the windows placed on a ring of F frames.  Window k covers
 * the frames (start[k] + j) mod F, j = 0 .. L - 1, and position j of its prediction belongs to that frame: per element at frame f
 * the position is j = f - start[k], plus F when that is negative, and the window takes part when 0 <= j < L.  Blend, slot order
 * (k ascending), step, lanes and arguments are those of im360_cfg_ddim_step_windows; with tables no window of which crosses the
 * end of the clip the result is that entry point's, bit for bit.
 * Precondition (the host cannot see the tables): 0 <= start[k] < F, every frame covered, L <= F.
 * Replaces: nothing in the reference (it has no temporal windows). */
int im360_cfg_ddim_step_windows_ring(const void* pred, const void* x, const void* noise, void* out, const void* start,
                                     const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float guidance,
                                     float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, int dtype,
                                     void* stream, const void* coef_dev);

/* im360_cfg_rescale_stats_windows over the blends of windows on a ring: tables and positions of
 * im360_cfg_ddim_step_windows_ring, everything else as in the linear entry point.
 * Precondition: 0 <= start[k] < F, every frame covered, L <= F.
 * Replaces: nothing in the reference. */
int im360_cfg_rescale_stats_windows_ring(const void* pred, const void* start, const void* weight, int nW, int64_t outer, int64_t F,
                                         int64_t L, int64_t inner, float guidance, void* ws, int64_t ws_floats, int dtype,
                                         void* stream, const void* coef_dev);

/* im360_cfg_ddim_step_windows_ring on r * m, r from the records of im360_cfg_rescale_stats_windows_ring over the same clip.
 * Precondition: 0 <= start[k] < F, every frame covered, L <= F.
 * Replaces: nothing in the reference. */
int im360_cfg_ddim_step_windows_ring_rescale(const void* pred, const void* x, const void* noise, void* out, const void* start,
                                             const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner,
                                             float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma,
                                             int mode, float phi, const void* ws, int64_t ws_floats, int dtype, void* stream,
                                             const void* coef_dev);

/* ---- DPM-Solver++ 2M (arXiv 2211.01095, algorithm 2: data prediction, multistep, order <= 2) on the CFG combination, one
 * elementwise pass.  Per element in fp32, with m = uncond + guidance * (cond - uncond) (times r of the guidance rescale when ws is
 * given) and x0 = the conversion of im360_cfg_ddim_step for mode bits 0-1 (0 epsilon, 1 v_prediction, 2 sample), clamped to
 * [-1, 1] with bit 2:
 *   out  = T(cx * x + c0 * x0 + c1 * hist)        one rounding, at the store
 *   hist = x0                                     fp32, in place, by the thread that read it
 * cx, c0, c1: the linear form of the update, fp64 host math (DPMSolverMultistepScheduler.multistep_coefficients): first order
 * cx = sigma'/sigma, c0 = -alpha' expm1(-h), c1 = 0; second order c0 (1 + 1/(2r)), c1 = -c0/(2r) with h, r of the paper.
 * c1 == 0 means there is no history: hist is then not read (it may hold anything, NaN included) and only written.
 * uncond / cond / x / out: n elements (n % 8 == 0) of the same 16-bit dtype; hist: device float[n]; all 16-byte aligned.
 * Mode 3 and mode bit 3 (use_clipped_model_output, which has no meaning here) are refused.
 * phi, ws, ws_floats: the guidance rescale of im360_cfg_ddim_step_rescale, ws written by im360_cfg_rescale_stats for the same
 * uncond / cond / n / guidance; ws == NULL selects the kernel without it (phi must then be 0).
 * coef_dev (optional): device float[6] = (guidance, sqrt_a, sqrt_b, cx, c0, c1) overriding the scalars (hipGraph replay): the
 * length of im360_cfg_ddim_step's vector, so one buffer and one upload path serve both samplers.
 * Replaces: nothing in the reference (its pipeline has only DDIM); the CFG combine of pipeline_animation_inference_dual.py:791-800
 *   followed by algorithm 2 of arXiv 2211.01095. */
int im360_cfg_multistep_step(const void* uncond, const void* cond, const void* x, void* hist, void* out, int64_t n, float guidance,
                             float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode, float phi, const void* ws,
                             int64_t ws_floats, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_multistep_step on the per-frame blend of sliding temporal context windows: pred, start, weight, nW, outer, F, L, inner
 * and the blend m of im360_cfg_ddim_step_windows; wrap = 0: the windows lie on a line (preconditions of that entry point), wrap = F:
 * on a ring of F frames (those of im360_cfg_ddim_step_windows_ring); any other wrap is refused.  x / out [outer, F, inner] 16-bit,
 * hist device float[outer * F * inner] in the same layout, 4-byte aligned.  16-byte lanes when inner % 8 == 0 and pred, x, hist and
 * out are 16-byte aligned, a scalar path otherwise.  ws: written by im360_cfg_rescale_stats_windows(_ring) for the same clip, or NULL.
 * nW = 1, start = {0}, weight all 1, L = F gives im360_cfg_multistep_step's out and hist bit for bit.
 * Replaces: nothing in the reference (no temporal windows, no multistep solver); arXiv 2211.01095, algorithm 2. */
int im360_cfg_multistep_step_windows(const void* pred, const void* x, void* hist, void* out, const void* start, const void* weight,
                                     int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, int64_t wrap, float guidance,
                                     float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode, float phi, const void* ws,
                                     int64_t ws_floats, int dtype, void* stream, const void* coef_dev);

/* ---- the unguided forms of the step entry points above: a step outside the guidance interval ("Applying Guidance in a Limited
 * Interval", arXiv 2404.07724; AnimationPipeline guidance_interval), where the model was run on the text half alone.  pred is that
 * one prediction and stands where m = uncond + guidance * (cond - uncond) stands in the sibling; everything behind m -- prediction
 * type, clamp, update, history, lanes, the scalar windows path, the checks and their error codes -- is the sibling's.  There is no
 * guidance argument and no second 16-byte load stream.  coef_dev (optional) is the SIBLING's vector, so a captured guided and a
 * captured unguided step share one uploaded buffer; its element 0 (the guidance) is not read.  For windows pred is
 * [nW, 1, outer, L, inner]: the text halves alone, nothing is read behind them.
 * Defining property: for finite inputs each entry point returns, bit for bit, what its sibling returns when uncond and cond are the
 * same tensor (both halves of every window equal), for any guidance: u + g (c - u) with c == u is u up to the sign of a zero.
 * There are no _rescale forms: the guidance rescale of a prediction towards its own standard deviation is the identity.
 * Replaces: nothing in the reference (its pipeline guides every step); DDIMScheduler.step of scheduling_ddim.py:251-373 /
 *   algorithm 2 of arXiv 2211.01095 on a single model output. */

/* out = cx * x + cv * pred: im360_cfg_ddim_update; coef_dev: float[3] = (guidance, cx, cv). */
int im360_ddim_update(const void* pred, const void* x, void* out, int64_t n, float cx, float cv, int dtype, void* stream,
                      const void* coef_dev);

/* im360_cfg_ddim_step on pred; coef_dev: float[6] = (guidance, sqrt_a, sqrt_b, sqrt_a_prev, dir, sigma). */
int im360_ddim_step(const void* pred, const void* x, const void* noise, void* out, int64_t n, float sqrt_a, float sqrt_b,
                    float sqrt_a_prev, float dir, float sigma, int mode, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_ddim_step_windows on the blend of pred [nW, 1, outer, L, inner]. */
int im360_ddim_step_windows(const void* pred, const void* x, const void* noise, void* out, const void* start, const void* weight,
                            int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float sqrt_a, float sqrt_b,
                            float sqrt_a_prev, float dir, float sigma, int mode, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_ddim_step_windows_ring on the blend of pred [nW, 1, outer, L, inner].
 * Precondition: 0 <= start[k] < F, every frame covered, L <= F. */
int im360_ddim_step_windows_ring(const void* pred, const void* x, const void* noise, void* out, const void* start,
                                 const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float sqrt_a,
                                 float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, int dtype, void* stream,
                                 const void* coef_dev);

/* im360_cfg_multistep_step on pred (hist as there); coef_dev: float[6] = (guidance, sqrt_a, sqrt_b, cx, c0, c1). */
int im360_multistep_step(const void* pred, const void* x, void* hist, void* out, int64_t n, float sqrt_a, float sqrt_b, float cx,
                         float c0, float c1, int mode, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_multistep_step_windows on the blend of pred [nW, 1, outer, L, inner]; wrap = 0 (line) or F (ring). */
int im360_multistep_step_windows(const void* pred, const void* x, void* hist, void* out, const void* start, const void* weight,
                                 int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, int64_t wrap, float sqrt_a,
                                 float sqrt_b, float cx, float c0, float c1, int mode, int dtype, void* stream,
                                 const void* coef_dev);

/* ---- adaptive projected guidance (APG, arXiv 2410.02416, algorithm 1; its momentum: the block behind this one) inside the guided step entry points.
 * The step sees, in place of m = uncond + guidance * (cond - uncond),
 *   d = cond - uncond,   q = cond + rho * x,   rho = -1 / sqrt_b (epsilon), -sqrt_a / sqrt_b (v_prediction), 0 (sample)
 *   alpha = sum d q / sum q^2
 *   s = min(1, threshold / (kp * sqrt(sum d^2 / n))),   kp = sqrt_b / sqrt_a (epsilon), sqrt_b (v_prediction), 1 (sample)
 *   m = cond + (guidance - 1) * s * d - lambda * q,   lambda = (guidance - 1) * s * (1 - eta) * alpha
 * i.e. the paper's update of the denoised prediction D(p) = kx x + kp p mapped back to the model's output: the guidance difference
 * D(cond) - D(uncond) split along D(cond) = kp q, its parallel part scaled by eta, its RMS clamped to `threshold` (x0 units;
 * INFINITY: no clamp).  The sums run over all n elements in fp32.  eta = 1 without a clamp is m up to rounding; uncond == cond gives
 * m = cond; sum q^2 = 0 gives NaN.  Two launches like the guidance rescale, with its workspace (8 * im360_cfg_rescale_records(n)
 * floats) and its grid: a statistics pass writes one record (count, sum d q, sum q^2, sum d^2) per workgroup, and every workgroup of
 * the step merges all of them in one fixed order -- no atomics, nothing read back, the same bits on every launch.  sqrt_a, sqrt_b and
 * the guidance are read from coef_dev[1], [2], [0] where coef_dev is given (the steps' six-float vectors: hipGraph replay).
 * Argument errors beyond the siblings': eta not finite, threshold not > 0, a short or misaligned workspace.
 * Replaces: nothing in the reference (its pipeline has plain CFG only); the guider of arXiv 2410.02416 between the model and
 *   DDIMScheduler.step / algorithm 2 of arXiv 2211.01095. */

/* the statistics pass over uncond / cond / x: n elements (n % 8 == 0) of one 16-bit dtype, 16-byte aligned; mode: bits 0-1 select rho */
int im360_cfg_apg_stats(const void* uncond, const void* cond, const void* x, int64_t n, float sqrt_a, float sqrt_b, int mode, void* ws,
                        int64_t ws_floats, int dtype, void* stream, const void* coef_dev);

/* the same over the per-frame blends of nW sliding-window predictions: uncond / cond are the blends of the two halves of pred
 * (layout, tables and preconditions of im360_cfg_ddim_step_windows), x is [outer, F, inner].  One uniform window with L = F writes
 * the records of im360_cfg_apg_stats bit for bit (for any inner). */
int im360_cfg_apg_stats_windows(const void* pred, const void* x, const void* start, const void* weight, int nW, int64_t outer,
                                int64_t F, int64_t L, int64_t inner, float sqrt_a, float sqrt_b, int mode, void* ws,
                                int64_t ws_floats, int dtype, void* stream, const void* coef_dev);

/* the same with the windows on a ring of F frames.  Precondition: 0 <= start[k] < F, every frame covered, L <= F. */
int im360_cfg_apg_stats_windows_ring(const void* pred, const void* x, const void* start, const void* weight, int nW, int64_t outer,
                                     int64_t F, int64_t L, int64_t inner, float sqrt_a, float sqrt_b, int mode, void* ws,
                                     int64_t ws_floats, int dtype, void* stream, const void* coef_dev);

/* out[0 .. 2] = (alpha, s, lambda) on the device from the records a statistics pass over n elements left in ws: one workgroup, the
 * merge every workgroup of a step makes (for tests and tools). */
int im360_cfg_apg_scalars(const void* ws, int64_t ws_floats, int64_t n, float guidance, float sqrt_a, float sqrt_b, int mode,
                          float eta, float threshold, void* out, void* stream, const void* coef_dev);

/* im360_cfg_ddim_step on the projected guidance; ws: the records of im360_cfg_apg_stats for the same uncond / cond / x / n. */
int im360_cfg_ddim_step_apg(const void* uncond, const void* cond, const void* x, const void* noise, void* out, int64_t n,
                            float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode, float eta,
                            float threshold, const void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_ddim_step_windows (wrap = 0) / im360_cfg_ddim_step_windows_ring (wrap = F; any other wrap is refused) on the projected
 * guidance of the blends; ws: the records of im360_cfg_apg_stats_windows(_ring) for the same clip.  One uniform window with L = F
 * gives im360_cfg_ddim_step_apg's result bit for bit. */
int im360_cfg_ddim_step_windows_apg(const void* pred, const void* x, const void* noise, void* out, const void* start,
                                    const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, int64_t wrap,
                                    float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma, int mode,
                                    float eta, float threshold, const void* ws, int64_t ws_floats, int dtype, void* stream,
                                    const void* coef_dev);

/* im360_cfg_multistep_step on the projected guidance (hist <- its x0); ws: the records of im360_cfg_apg_stats. */
int im360_cfg_multistep_step_apg(const void* uncond, const void* cond, const void* x, void* hist, void* out, int64_t n, float guidance,
                                 float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode, float eta, float threshold,
                                 const void* ws, int64_t ws_floats, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_multistep_step_windows on the projected guidance of the blends; wrap = 0 (line) or F (ring); ws: the records of
 * im360_cfg_apg_stats_windows(_ring).  One uniform window with L = F gives im360_cfg_multistep_step_apg's out and hist bit for bit. */
int im360_cfg_multistep_step_windows_apg(const void* pred, const void* x, void* hist, void* out, const void* start,
                                         const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, int64_t wrap,
                                         float guidance, float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode, float eta,
                                         float threshold, const void* ws, int64_t ws_floats, int dtype, void* stream,
                                         const void* coef_dev);

/* ---- APG with the paper's momentum (algorithm 1 in full): the difference that is projected and clamped is the running average of the
 * run's guided steps, Dbar_t = Delta_t + beta * Dbar_prev in x0 units.  The state holds it in the model-output units of the step that
 * wrote it, e_t = Dbar_t / kp_t (kp = -sqrt_b / sqrt_a (epsilon), -sqrt_b (v_prediction), 1 (sample)), so that
 *   e = d + carry * state,   carry = beta * kp_prev / kp_t      (0 on the first guided step of a run; beta for `sample`)
 * is one fma and the block above holds with d replaced by e: alpha = sum e q / sum q^2, s from sum e^2, m = cond + (guidance - 1) s e
 * - lambda q.  `state`: float32[n], indexed like the multistep history (the flat element index of x; windows: of the clip [outer, F,
 * inner] of blends), 16-byte aligned where the launch moves 16-byte lanes (always for the plain entry points), each element read and
 * written by one thread.  A statistics pass reads it; the step reads it again, forms the same bits and stores the UNclamped e in
 * place.  carry == 0: the state is not read at all, only written by the step, and e = d to the bit -- records, scalars and step are
 * those of the _apg entry points, and whatever the buffer held (NaN included) has no effect; so a state never needs clearing.  carry
 * is read from carry_dev[0] (device float32[1]) where carry_dev is given (hipGraph replay; coef_dev keeps its six floats).
 * Argument errors beyond the _apg siblings': a null or misaligned state, a non-finite host carry, a misaligned carry_dev, state ==
 * hist.  im360_cfg_apg_scalars serves the records of either statistics pass.
 * Replaces: nothing in the reference; the momentum buffer of the guider of arXiv 2410.02416. */

/* im360_cfg_apg_stats on e: the records (count, sum e q, sum q^2, sum e^2); the state is not written */
int im360_cfg_apg_momentum_stats(const void* uncond, const void* cond, const void* x, const void* state, int64_t n, float sqrt_a,
                                 float sqrt_b, int mode, float carry, const void* carry_dev, void* ws, int64_t ws_floats, int dtype,
                                 void* stream, const void* coef_dev);

/* im360_cfg_apg_stats_windows on e; state [outer, F, inner].  One uniform window with L = F writes the records of
 * im360_cfg_apg_momentum_stats bit for bit. */
int im360_cfg_apg_momentum_stats_windows(const void* pred, const void* x, const void* state, const void* start, const void* weight,
                                         int nW, int64_t outer, int64_t F, int64_t L, int64_t inner, float sqrt_a, float sqrt_b,
                                         int mode, float carry, const void* carry_dev, void* ws, int64_t ws_floats, int dtype,
                                         void* stream, const void* coef_dev);

/* the same with the windows on a ring of F frames.  Precondition: 0 <= start[k] < F, every frame covered, L <= F. */
int im360_cfg_apg_momentum_stats_windows_ring(const void* pred, const void* x, const void* state, const void* start,
                                              const void* weight, int nW, int64_t outer, int64_t F, int64_t L, int64_t inner,
                                              float sqrt_a, float sqrt_b, int mode, float carry, const void* carry_dev, void* ws,
                                              int64_t ws_floats, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_ddim_step_apg on e, state <- e; ws: the records of im360_cfg_apg_momentum_stats for the same tensors, state and carry. */
int im360_cfg_ddim_step_apg_momentum(const void* uncond, const void* cond, const void* x, const void* noise, void* state, void* out,
                                     int64_t n, float guidance, float sqrt_a, float sqrt_b, float sqrt_a_prev, float dir, float sigma,
                                     int mode, float eta, float threshold, const void* ws, int64_t ws_floats, float carry,
                                     const void* carry_dev, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_ddim_step_windows_apg on e, state [outer, F, inner] <- e; wrap = 0 (line) or F (ring).  One uniform window with L = F
 * gives im360_cfg_ddim_step_apg_momentum's out and state bit for bit. */
int im360_cfg_ddim_step_windows_apg_momentum(const void* pred, const void* x, const void* noise, void* state, void* out,
                                             const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L,
                                             int64_t inner, int64_t wrap, float guidance, float sqrt_a, float sqrt_b,
                                             float sqrt_a_prev, float dir, float sigma, int mode, float eta, float threshold,
                                             const void* ws, int64_t ws_floats, float carry, const void* carry_dev, int dtype,
                                             void* stream, const void* coef_dev);

/* im360_cfg_multistep_step_apg on e (hist <- the x0 of its projected guidance), state <- e. */
int im360_cfg_multistep_step_apg_momentum(const void* uncond, const void* cond, const void* x, void* hist, void* state, void* out,
                                          int64_t n, float guidance, float sqrt_a, float sqrt_b, float cx, float c0, float c1, int mode,
                                          float eta, float threshold, const void* ws, int64_t ws_floats, float carry,
                                          const void* carry_dev, int dtype, void* stream, const void* coef_dev);

/* im360_cfg_multistep_step_windows_apg on e, state [outer, F, inner] <- e; wrap = 0 or F. */
int im360_cfg_multistep_step_windows_apg_momentum(const void* pred, const void* x, void* hist, void* state, void* out,
                                                  const void* start, const void* weight, int nW, int64_t outer, int64_t F, int64_t L,
                                                  int64_t inner, int64_t wrap, float guidance, float sqrt_a, float sqrt_b, float cx,
                                                  float c0, float c1, int mode, float eta, float threshold, const void* ws,
                                                  int64_t ws_floats, float carry, const void* carry_dev, int dtype, void* stream,
                                                  const void* coef_dev);

/* ---- start latents of a run that begins from a given clip (AnimationPipeline init_latents / init_video, strength < 1), one launch:
 *   out_pano[c, f, p]    = T(sqrt_a * x0[c, f, p] + sqrt_b * noise[f, c, p])        fp32, one rounding, at the store
 *   out_pers[m, c, f, q] = ok[m, q] ? out_pano[c, f, idx[m, q]] : 0                 the gather of the ROUNDED panorama start, bit for bit
 * x0 / out_pano: 16-bit [C, F, HW] (the pipeline's panorama latent [1, 4, F, h, w]); noise: fp32 [F, C, HW] (the layout init_noise
 * draws in); idx int32 / ok uint8 [M, Q]: the table and validity flags of pano_geometry.nearest_e2p_index; out_pers: 16-bit
 * [M, C, F, Q] (the perspective latent [1, m, 4, F, h, w]).  sqrt_a, sqrt_b = sqrt(a_t), sqrt(1 - a_t) of the first timestep that is run
 * (DDIMScheduler.noise_coefficients).  One workgroup per (c, f) plane: planes of up to 64 KiB (2 * HW bytes) are kept in LDS and
 * all M * Q gathers served from there; larger planes form every gathered element again from x0 and noise (same expression, same
 * bits).  16-byte lanes when HW % 8 == 0, Q % 8 == 0 and every pointer is aligned for them, a scalar path otherwise.
 * Refused: a null pointer, a size <= 0, HW / C * F / M * Q >= 2^31 (32-bit indices inside a plane, a table and the grid; element
 * offsets are 64-bit), noise or idx off 4 bytes, an unknown dtype.
 * Precondition (the host cannot see the table): 0 <= idx[m, q] < HW.  The kernel clamps, so a bad table gives wrong elements and
 * no read outside the plane.
 * Replaces: pipeline_animation_inference_dual.py:361-387 (the E2P of the noise, applied here to the noised latent) and
 *   DDIMScheduler.add_noise, scheduling_ddim.py:375-396.  The reference pipeline itself has no strength argument: it always starts
 *   from pure noise. */
int im360_noise_latents(const void* x0, const float* noise, const int32_t* idx, const uint8_t* ok, void* out_pano, void* out_pers,
                        int64_t F, int64_t C, int64_t HW, int64_t M, int64_t Q, float sqrt_a, float sqrt_b, int dtype, void* stream);

/* ---- regenerating part of a given clip (AnimationPipeline regenerate_mask): after every step of the loop both latents are blended,
 * IN PLACE, with the clean clip noised to the level the latents now have; one launch after the two step launches:
 *   known[c, f, p]   = T(sqrt_a * x0[c, f, p] + sqrt_b * noise[f, c, p])           the expression of im360_noise_latents, one rounding
 *   pano[c, f, p]    = blend(pano[c, f, p], known[c, f, p], mask[f, p])
 *   pers[m, c, f, q] = ok[m, q] ? blend(pers[m, c, f, q], known[c, f, idx[m, q]], mask[f, idx[m, q]]) : pers[m, c, f, q]
 *   blend(x, k, w):  w >= 1 -> x, not stored;  w <= 0 -> k, bit for bit;  otherwise T(fma(w, x - k, k)) in fp32
 * pano / x0: 16-bit [C, F, HW]; noise: fp32 [F, C, HW]; mask: fp32 [F, HW], 1 = regenerate, 0 = keep, one plane per frame shared by
 * the channels; pers: 16-bit [M, C, F, Q]; idx int32 / ok uint8 [M, Q] as for im360_noise_latents.  sqrt_a, sqrt_b:
 * DDIMScheduler.keep_coefficients; coef_dev: null, or device float[2] holding them, read by the kernel instead (graph replay).
 * With mask 0 the latents are what im360_noise_latents writes for the same coefficients (pers: where ok), bit for bit.
 * One workgroup per (c, f) plane; `known` is formed from x0 and noise (planes of up to 64 KiB are kept in LDS for the M * Q
 * perspective elements, larger ones form them again) and never read back from pano, so the in-place update has no hazard between
 * workgroups.  16-byte lanes when HW % 8 == 0, Q % 8 == 0 and every pointer is aligned for them, a scalar path otherwise.
 * Refused: a null pointer (coef_dev excepted), a size <= 0, HW / C * F / M * Q >= 2^31, noise / mask / idx / coef_dev off 4 bytes,
 * x0 == pano, an unknown dtype.  Precondition: 0 <= idx[m, q] < HW (clamped by the kernel).
 * Replaces: the blend after scheduler.step of diffusers/pipelines/stable_diffusion/pipeline_stable_diffusion_inpaint_legacy.py:565-575
 *   (`init_latents_proper = add_noise(init_latents_orig, noise, t); latents = init_latents_proper * mask + latents * (1 - mask)`, with
 *   the opposite mask polarity), noised to the NEXT timestep as current diffusers does rather than to the step's own. */
int im360_keep_latents(void* pano, void* pers, const void* x0, const float* noise, const float* mask, const int32_t* idx,
                       const uint8_t* ok, int64_t F, int64_t C, int64_t HW, int64_t M, int64_t Q, float sqrt_a, float sqrt_b, int dtype,
                       void* stream, const void* coef_dev);

/* ---- release mode of the keep launch (AnimationPipeline regenerate_mode="release"; Differential Diffusion, arXiv 2306.00950, the
 * "differential img2img" of diffusers' community pipelines): the mask is a per-pixel strength s in [0, 1] and nothing is averaged.
 *   pano[c, f, p]    = mask[f, p] <= tau ? known[c, f, p] : pano[c, f, p]
 *   pers[m, c, f, q] = ok[m, q] && mask[f, idx[m, q]] <= tau ? known[c, f, idx[m, q]] : pers[m, c, f, q]
 * `known`, the tensors, the paths and the refusals are those of im360_keep_latents (the same kernel, instantiated for the select): a
 * pinned element is `known` bit for bit, as blend writes for w <= 0; a free one keeps its bits and a group of eight free ones is not
 * stored.  The compare is in fp32; tau = DDIMScheduler.release_threshold of the step (1 - (i + 1) / n in fp64, rounded once), so s = 1
 * is never pinned, s = 0 always, and a 0 / 1 mask gives the bits of im360_keep_latents at every step.  tau < 0 pins nothing.
 * coef_dev: null, or device float[3] = (sqrt_a, sqrt_b, tau), read by the kernel instead of the three arguments (graph replay).
 * Replaces: the per-step `mask = thresholds[i] > map; latents = original_with_noise * mask + latents * (1 - mask)` of diffusers'
 *   examples/community/pipeline_stable_diffusion_xl_differential_img2img.py, as a select. */
int im360_keep_latents_release(void* pano, void* pers, const void* x0, const float* noise, const float* mask, const int32_t* idx,
                               const uint8_t* ok, int64_t F, int64_t C, int64_t HW, int64_t M, int64_t Q, float sqrt_a, float sqrt_b, float tau,
                               int dtype, void* stream, const void* coef_dev);

/* ---- the spherical feather of a regenerate_mask (AnimationPipeline regenerate_feather), one launch: for every pixel of an
 * equirectangular frame the squared chord to the nearest kept pixel of that frame.
 *   d2[f, p] = min over q with keep[f, q] != 0 of fma(dz, dz, fma(dy, dy, dx * dx)),  (dx, dy, dz) = dirs[p] - dirs[q]     fp32, this order
 * and +inf for a frame without a kept pixel.  keep: uint8 [F, HW]; dirs: fp32 [HW, 3], unit vectors of the pixel centres
 * (pano_geometry.pixel_directions: fp64 on the host, rounded once -- the kernel does no trigonometry); d2: fp32 [F, HW].  From
 * differences, so small distances keep their relative accuracy (2 - 2 dot would not).  The host forms the angle 2 asin(sqrt(d2) / 2) and
 * the ramp (pano_geometry.feather_pano_mask).  One workgroup per (frame, 512 pixels); the candidates stream through LDS in tiles of 1024
 * and those not kept are skipped; no atomics, deterministic, no HW x HW intermediate.
 * Refused: a null pointer, a size <= 0, F or HW + 512 >= 2^31, F * ceil(HW / 512) >= 2^24 workgroups, dirs or d2 off 4 bytes, d2
 * overlapping an input.
 * Replaces: nothing in the reference; a feather (Gaussian blur / distance transform) of the mask on the pixel grid, which neither
 *   crosses the +-180 degree seam nor knows that a column near a pole is a fraction of a degree. */
int im360_sphere_distance2(const uint8_t* keep, const float* dirs, float* d2, int64_t F, int64_t HW, void* stream);

/* ---- upscaling a clean panorama latent (AnimationPipeline init_latents / init_video at a lower resolution than the run, init_resize),
 * one launch: x [C, F, h, w] -> out [C, F, H, W], H >= h, W >= w, one 16-bit dtype; mode 0 bilinear, 1 bicubic.
 *   out[c, f, Y, X] = T(sum_r wy[Y][r] * (sum_j wx[X][j] * x[c, f, row(Y, r), col(X, j)]))     fp32, horizontal pass then vertical, one rounding
 * Half-pixel centres (align_corners=False) from integers: num = (2 X + 1) w - W, i0 = floor(num / 2 W), t = float(num - i0 * 2 W) /
 * float(2 W) (one rounding; exactly periodic in X for every integer scale), rows alike.  Bilinear: taps i0, i0 + 1, weights (1 - t, t);
 * bicubic: taps i0 - 1 .. i0 + 2, Keys kernel, A = -0.75 (the polynomials of torch's upsample_bicubic2d).  The image is
 * equirectangular: column taps wrap (mod w), row taps clamp to [0, h - 1].  Equal sizes return the input's bits (t = 0).
 * One workgroup per (plane, 8 output rows); eight columns per lane and one 16-byte store when W % 8 == 0 and both pointers are
 * 16-byte aligned, a scalar path otherwise, the same bits on both; source rows are read from global memory (cache-resident planes).
 * Refused: a null pointer, a size <= 0, h / w / H / C * F / 8 W >= 2^31 (32-bit rows and columns; coordinates and element offsets
 * are 64-bit), C * F * ceil(H / 8) >= 2^24 workgroups (a launch holds fewer than 2^32 threads), a pointer off 2 bytes, x == out, H < h or W < w (no antialiasing filter), an unknown mode or dtype.
 * Replaces: nothing in the reference (it upscales the decoded video with an external super-resolution stage); the latent-upscale
 *   pass of diffusers (F.interpolate on the latent), made aware of the +-180 degree seam. */
int im360_resize_pano_latent(const void* x, void* out, int64_t C, int64_t F, int64_t h, int64_t w, int64_t H, int64_t W, int mode,
                             int dtype, void* stream);

/* ---- retiming a clean panorama latent (AnimationPipeline.resize_init: init_latents / init_video with fewer frames than the run,
 * init_retime), one launch: x [C, f, hw] -> out [C, F, hw], F >= f, one 16-bit dtype; mode 0 linear, 1 cubic; loop 0 open clip, 1 ring.
 *   out[c, j, p] = T(sum_k wt[j][k] * x[c, frame(j, k), p])                                    fp32, one rounding
 * Output frame j samples source time i0 + t from integers: num = j (f - 1), den = max(F - 1, 1) on an open clip (endpoint-aligned:
 * frame 0 -> frame 0, frame F - 1 -> frame f - 1), num = j f, den = F on a ring (frame F would be frame 0 again); i0 = num / den,
 * t = float(num - i0 den) / float(den), one rounding.  Linear: taps i0, i0 + 1, weights (1 - t, t); cubic: taps i0 - 1 .. i0 + 2, Keys
 * kernel, A = -0.75 (the weights of im360_resize_pano_latent).  Tap frames clamp to [0, f - 1] on an open clip and wrap (mod f) on a
 * ring.  A frame with t == 0 is a copy of source frame i0, bit for bit (NaNs, the sign of zero); F == f returns the input's bits.
 * One workgroup per (channel, output frame, 4096 plane elements); eight elements per unit, one 16-byte load per tap and one 16-byte
 * store when hw % 8 == 0 and both pointers are 16-byte aligned, a scalar path otherwise, the same bits on both; no LDS, no atomics.
 * Refused: a null pointer, a size <= 0, f / F / C * F / hw + 4096 >= 2^31, C * F * ceil(hw / 4096) >= 2^24 workgroups (a launch holds
 * fewer than 2^32 threads), a pointer off 2 bytes, x == out, F < f (no temporal antialiasing filter), an unknown mode, loop or dtype.
 * Replaces: nothing in the reference (it generates its 16 frames in one pass); F.interpolate(..., align_corners=True) along the frame
 *   axis, made aware of the loop point of a looping clip. */
int im360_retime_pano_latent(const void* x, void* out, int64_t C, int64_t f, int64_t F, int64_t hw, int mode, int loop, int dtype,
                             void* stream);

/* ---- FreeInit's re-noising (AnimationPipeline free_init_iters > 1; arXiv 2312.07537, diffusers' free_init_utils: _get_free_init_freq_filter
 * / _apply_freq_filter), three launches: the EFFECTIVE NOISE n_eff under which sa x0 + sb n_eff = n2 + L (sa x0 + sb n1 - n2), i.e. the
 * low-pass of the noised clip plus the high-pass of the fresh noise n2, L = Lf (x) Lh (x) Lw.
 *   d = fma(sa, x0, fma(sb, n1, -n2));   y = L d (along w, then h, then F);   out = fma(y - d, inv_sb, n1)                   all fp32
 * x0 [C, F, H W] of one 16-bit dtype (the clean clip); n1, n2, out fp32 [F, C, H W]; Lf [F, F], Lh [H, H], Lw [W, W] fp32, row i the
 * weights of output i (pano_geometry.free_init_operator in fp64, rounded once; dense, so each axis has its own boundary: periodic
 * longitude, mirrored latitude, frames periodic on a looping clip and mirrored otherwise -- fftn would wrap all three); ws: fp32
 * workspace of ws_elems >= 2 C F H W elements; inv_sb = 1 / sb formed in fp64 by the caller.
 * Every dot product is one fp32 fma chain from 0 over j = 0 .. n - 1; no atomics, deterministic; identity operators give out == n1 bit
 * for bit.  Launch 1 forms d on the fly (64 x 64 slabs in LDS, lane = row); launches 2 and 3 read columns from global memory (lane =
 * column, no LDS), launch 3 forms d again and writes out: no elementwise launch, no whole plane in LDS.  Four elements per unit (16-byte
 * fp32 accesses, 8-byte loads of x0) when W % 4 == 0 and the pointers are aligned for it, a scalar path otherwise, the same bits on both.
 * Refused: a null pointer, a size <= 0, C F H W >= 2^31, a workspace that is too small, sb <= 0 or inv_sb <= 0, a misaligned pointer
 * (2 bytes for x0, 4 for fp32), out or ws overlapping each other or an input, 2^24 workgroups in a launch, an unknown dtype.
 * Replaces: nothing in the reference (one pass from white noise); diffusers' fftn -> fftshift -> Gaussian mask -> ifftn round trip. */
int im360_free_init_noise(const void* x0, const float* n1, const float* n2, const float* Lf, const float* Lh, const float* Lw, float* out,
                          float* ws, int64_t ws_elems, int64_t C, int64_t F, int64_t H, int64_t W, float sa, float sb, float inv_sb,
                          int dtype, void* stream);

/* y[r] = LayerNorm(x[r] + pre[r % pre_period]) * gamma + beta + post[(r / post_div) % post_mod] on token rows
 * [rows, C]; pre / post are optional [*, C] tables (the WarpAttn spherical PE added before norm1, the motion
 * module's frame PE added after the norm).
 * Replaces: nn.LayerNorm at animatediff/models/attention.py:463-507, motion_module.py:249-256 (+ PE add :349-350),
 *   src/modules/transformer.py:156-165 (+ `query + query_pe`, attn_perspano.py:56,63). */
int im360_layernorm(const void* x, const void* gamma, const void* beta, const void* pre, const void* post,
                    void* y, int64_t rows, int64_t C, int64_t pre_period, int64_t post_div,
                    int64_t post_mod, float eps, int dtype, void* stream);

/* out[rows, I] = h[:, :I] * gelu(h[:, I:]) (exact erf GELU).
 * Replaces: GEGLU, diffusers/models/activations.py:93-125; src/modules/transformer.py:10-16. */
int im360_geglu(const void* h, void* out, int64_t rows, int64_t I, int dtype, void* stream);

/* GEGLU feed-forward input projection in one launch: y[m, j] = (x W_v^T + b_v)[m, j] * gelu((x W_g^T + b_g)[m, j]),
 * x [M, K] token-major, y [M, I].  w_packed / bias_packed hold the 2I rows of the projection with 32-row blocks of
 * the value half and the gate half interleaved (v0, g0, v1, g1, ...; see kernels.pack_geglu), the weight in
 * im360_pack_conv_weight's [rows][1][K] layout.  K % 64 == 0, I % 128 == 0.  The projection is rounded to 16 bits
 * before the activation, like the two-kernel path.
 * Replaces: GEGLU.forward, diffusers/models/activations.py:93-125 (Linear + chunk + F.gelu + mul). */
int im360_linear_geglu(const void* x, const void* w_packed, const void* bias_packed, void* y,
                       int64_t M, int64_t K, int64_t I, int dtype, void* stream);

/* Token-major Linear y[M, N] = x[M, K] w^T + bias (+ res) on the persistent MFMA kernel (N % 320 == 0, K % 32 == 0,
 * w_packed = im360_pack_conv_weight of the [N, K, 1, 1] view).  rowstats (optional): fp32 [M][N / 160][2], per row and
 * 160-column slice (sum, sum of squares) of the STORED 16-bit output -- the LayerNorm statistics of y's rows, taken in
 * the epilogue that writes them, for a consumer that folds the normalisation into its GEMM (the two functions below).
 * Replaces: nn.Linear (+ residual add) in front of nn.LayerNorm, animatediff/models/attention.py:264, 461-508;
 *   motion_module.py:172, 230-258; src/modules/transformer.py:156-165. */
int im360_linear_fwd(const void* x, const void* w_packed, const void* bias, const void* res, void* y, void* rowstats,
                     int64_t M, int64_t K, int64_t N, int dtype, void* stream, void* gn_partial);

/* Linear(LayerNorm(x)) with the normalisation folded into the GEMM: x [M, K] are the RAW rows, rowstats [M][rs_p][2] their
 * (sum, sum of squares) slices from im360_linear_fwd, w_packed = pack(gamma (.) W) and
 *   y[r] = rstd_r * (x[r] w^T - mu_r * c1) + (tab ? tab[(r / tab_div) % tab_mod] : c2)
 * with fp32 vectors c1[n] = sum_k w'[n][k] (of the rounded 16-bit w'), c2 = W beta + bias; tab (optional, fp32
 * [tab_mod][N], tab_div % 256 == 0): c2 + the rows added AFTER the normalisation pushed through the projection (the motion
 * module's frame positional encoding; one table row per 256-row tile; since round 4 the rows INCLUDE c2, so that a tile's
 * constant term is one vector the kernel fetches by LDS-DMA).  The LayerNorm pass over the activations and its output tensor do not exist.  Variance = E[x^2] - mu^2 in
 * fp32 from 16-bit data.  N % 320 == 0, K % 32 == 0.
 * Replaces: nn.LayerNorm -> to_q / fused to_q,k,v, animatediff/models/attention.py:470-488; motion_module.py:236-250
 *   (+ pos_encoder :349-350). */
int im360_linear_ln_fwd(const void* x, const void* w_packed, const void* c1, const void* c2, const void* rowstats,
                        int64_t rs_p, float eps, const void* tab, int64_t tab_div, int64_t tab_mod, void* y,
                        int64_t M, int64_t K, int64_t N, int dtype, void* stream);

/* GEGLU(LayerNorm(x)) in one launch: im360_linear_geglu with the normalisation folded in as above; w_packed, c1, c2 in
 * the interleaved row order of kernels.pack_geglu.
 * Replaces: nn.LayerNorm -> GEGLU, animatediff/models/attention.py:503-506; motion_module.py:255-257;
 *   src/modules/transformer.py:164-165. */
int im360_linear_geglu_ln(const void* x, const void* w_packed, const void* c1, const void* c2, const void* rowstats,
                          int64_t rs_p, float eps, void* y, int64_t M, int64_t K, int64_t I, int dtype, void* stream);

/* The whole GEGLU feed-forward of a 320-channel block in one launch (an addition under ABI version 5): the 1280-wide GEGLU output stays in LDS.
 *   y[M, N] = GEGLU(LN(x) W1^T + b1) W2^T + b2 + res          K = 320, I = 1280, N = 320 only (else IM360_ERR_UNSUPPORTED)
 * LayerNorm-folded form (c1 != NULL): w1_packed, c1, c2, rowstats, rs_p, eps as in im360_linear_geglu_ln, b1_packed ignored;
 * plain form (c1 == NULL): w1_packed, b1_packed (optional) as in im360_linear_geglu.  w2_packed = im360_pack_conv_weight of the
 * [N, I, 1, 1] view, b2 [N] optional, res [M, N] required (it may alias x), y [M, N]; pointers 16-byte aligned (rowstats 8).
 * Same MFMA shape, K order, 16-bit rounding of the intermediate and epilogue arithmetic as im360_linear_geglu[_ln] followed by
 * im360_conv_fwd on the [M, 1, 1, I] view with bias and residual.
 * Replaces: FeedForward (GEGLU -> Dropout(0) -> Linear) + residual behind norm3, diffusers/models/attention_lora.py:493-547,
 *   activations.py:93-125; animatediff/models/attention.py:503-508; motion_module.py:255-258. */
int im360_ff_fused(const void* x, const void* w1_packed, const void* b1_packed, const void* c1, const void* c2,
                   const void* rowstats, int64_t rs_p, float eps, const void* w2_packed, const void* b2, const void* res, void* y,
                   int64_t M, int64_t K, int64_t I, int64_t N, int dtype, void* stream);

/* y[r, :] = softmax(x[r, :] * scale), fp32 arithmetic on 16-bit rows (cols and the row strides multiples of 8; in place
 * allowed).  With two launches of im360_conv_fwd as GEMMs it forms the single-head d = 512 attention of the VAE.
 * Replaces: AttentionBlock.forward's softmax(attention_scores.float()), diffusers/models/attention.py:336-364. */
int im360_softmax_rows(const void* x, void* y, int64_t rows, int64_t cols, int64_t x_rs, int64_t y_rs,
                       float scale, int dtype, void* stream);

/* out[n][m] = cv2.remap(img[n], map_x[m], map_y[m], INTER_CUBIC, borderMode=BORDER_WRAP): uint8 images [N, H, W, C]
 * (C = 1, 3, 4) on the device, float32 maps [M, h, w] in source pixel units, out uint8 [N, M, h, w, C]; wtab = the
 * 1024 x 16 int16 bicubic weight table (imagine360_amd.preprocess.cubic_weight_table).  One launch warps every frame through
 * every camera's map.  OpenCV's fixed-point arithmetic restated (parity unpinned: OpenCV is not available to check it).
 * Replaces: the cv2.remap calls of Equirec2Perspec.GetPerspective / Perspec2Equirec.GetEquirec,
 *   src/utils/pano_utils/Equirec2Perspec.py:61, Perspec2Equirec.py:65, looped per frame and view by process_equi /
 *   pers2pano_vid / get_anchor_target (inference_dual_p2e.py:113-144, 291-304; animatediff/utils/video_mask.py:158-217). */
int im360_remap_cubic_wrap_u8(const void* img, const void* map_x, const void* map_y, const void* wtab, void* out,
                              int64_t N, int64_t M, int64_t H, int64_t W, int64_t C, int64_t h, int64_t w, void* stream);

/* Largest all-ones rectangle of a HOST uint8 mask [H, W]: rect[4] = (top, left, width, height), scan order and
 * tie-breaking of the reference's Python loops.  Host code (no GPU involved).
 * Replaces: get_maxrec_cord, src/modules/utils.py:39-73. */
int im360_max_rect(const uint8_t* mask, int64_t H, int64_t W, int64_t* rect);

/* A/B switches of the host-side launchers (knob ids: 0 attention query blocks per wave, 1 conv tile policy: 0 never the
 * 256x320 tile, 2 / 3 two-workgroup 128x320 / 128x256 tiles, 2 force 32-channel K steps, 3 scalar temporal attention,
 * 4 conv/GEMM pipeline: 0 two-stage kernel, 1 persistent ring kernel with interleaved asm LDS-DMA requests, 2 / 3 plain ring
 * (builtin / asm LDS-DMA), 4 staggered wave groups, 5 ring kernel for convolutions too; 5 reserved; 6 ablation bits of the
 * ring kernel; 7 halo-patch kernel for the stride-1 3x3 convolutions; 8 taps-innermost K order of the 3x3 convolutions
 * (default 1); 9 packed-rows LayerNorm at 320 channels (default 1); 10 cout groups of the persistent kernel's tile walk:
 * 0 = by weight size, 2 / 4 / 8 forced; 11 text + IP cross attention: 1 key / value sets resident in LDS, 2 the same
 * with 8-byte output stores, 3 (default) the same on twelve-wave workgroups whose waves fetch their query blocks through private LDS
 * rings, 0 the generic two-pass kernel; 12 attention row sums as dot2 of the packed weights + v_permlane32_swap max exchange (sums
 * the ROUNDED weights: results differ in the last bits; default 0); 13 single-buffer / three-waves-per-SIMD attention when there
 * is one key tile (default 1); 14 ablation builds of the d = 64 two-block attention kernel: results are garbage; 15 WarpAttn head groups: the four waves of a
 * workgroup on four (batch, head) pairs over the same query rows, measured slower, default 0; 16 tiles of
 * convolutions with Cout % 128 in (0, 64] on small grids: 2 (default) 128 x 128, 0 / 1 256 x 64 with 32- / 64-channel K steps; 17 d = 64 attention without a bias on four-wave grids: 1 (default)
 * one query block per wave at three waves per SIMD, 0 the round-2 rule (two blocks per wave on large grids)).  Defaults are the measured best; the IM360_* environment variables seed them at load time.  Knobs 7 and 8
 * change the fp32 summation order, and so do 2 (= 32) and 16 (= 0 / 1) for 3x3 convolutions that the default runs taps-innermost: the 32-channel and
 * the 256 x 64 kernels are tap-major, i.e. they give the bits of knob 8 = 0.  11 (0 against 1 - 3: the scale is folded into K instead of Q) and 12 move
 * the 16-bit rounding points; 0 and 17 (= 0, on large grids) switch between one and two query blocks per wave, which rescale the running sums at
 * different points; 9 reduces a row over other lane groups (last bits); 24 (register-staged four-wave GEMM tiles: bit 0 / 2 GEGLU projection on
 * the 256 x 256 / 256 x 128 tile, bit 1 / 3 the same with LayerNorm folded in; also knob 4 = 12 / 13) is bit-identical for the plain GEGLU epilogue
 * and differs in last bits for the LayerNorm-folded one (same summation order; hipcc contracts the fp32 `(acc - mu c1) rstd + c2` differently in the
 * two kernels).  6 and 14 break results on purpose.  The others -- 1, 2 / 16 where the K order is kept, 10, 13, 17 on small grids, 22 (temporal
 * attention load / store forms), 23 (non-temporal epilogue stores), 25 (GroupNorm apply workgroups) -- do not change a bit
 * (tests/test_kernel_variants_gpu.py). */
int im360_tuning_set(int knob, int value);
/* the knob's current value (an addition under ABI version 5; 0 for an unknown knob): host-side routing reads knob ff_fused through it */
int im360_tuning_get(int knob);

/* ---- diagnostics: the ONLY process-global state behind this ABI (boundary nit).  A production binding needs neither
 * im360_tuning_set (A/B switches; the defaults are the measured best and no compute entry point requires a knob) nor the two
 * profiling calls below (bench.py's per-class HIP events); every compute entry point above is a pure function of its arguments
 * and the knobs' defaults. ---- */

/* HIP-event profiling of kernel classes (bit k of mask enables class k: 0 attn, 1 temporal, 2 conv,
 * 3 gn_stats, 4 gn_apply, 5 layernorm/geglu/elementwise, 6 conv kernel used as a token-major linear).
 * collect() synchronises on the recorded events. */
void im360_prof_enable(unsigned mask);
int im360_prof_collect(int kind, double* total_ms, long* launches);

#ifdef __cplusplus
}
#endif
#endif
