/*
 * udt_kernels.h — C ABI of libudt_kernels.so: the MI355X (gfx950 / CDNA4) kernels behind the
 * UDiffText denoising hot path.
 *
 * The reference (ZYM-PKU/UDiffText) is pure Python and owns no native boundary; its hot path reaches
 * native arithmetic only through third-party wheels.  Each entry point below therefore replaces the
 * third-party call the reference makes at the cited file:line (paths relative to the reference root):
 *
 *   udt_gemm            nn.Linear / nn.Conv2d(1x1) / nn.Conv2d(3x3) call sites:
 *                         sgm/modules/attention.py:47-51,66-70 (GEGLU / FeedForward),
 *                         sgm/modules/attention.py:193-199,215-218 (to_q/to_k/to_v/to_out),
 *                         sgm/modules/attention.py:375,395,407,411 (proj_in / proj_out),
 *                         sgm/modules/diffusionmodules/openaimodel.py:186,223-230,240 (ResBlock convs + skip),
 *                         sgm/modules/diffusionmodules/openaimodel.py:85-101,132-146 (Up/Downsample),
 *                         sgm/modules/diffusionmodules/openaimodel.py:210-216,340-344 (emb_layers, time_embed),
 *                         sgm/modules/diffusionmodules/model.py:59-68,74-85,108-124,128-148 (VAE convs),
 *                         sgm/modules/diffusionmodules/model.py:214-226,232-256 (VAE attention 1x1 convs),
 *                         sgm/models/autoencoder.py:297-298 (quant_conv / post_quant_conv),
 *                         sgm/modules/encoders/modules.py:1103-1104 (nn.TransformerEncoderLayer linears)
 *   udt_attn_fwd        xformers.ops.memory_efficient_attention  sgm/modules/attention.py:246
 *   udt_xattn_fwd       einsum / softmax / einsum               sgm/modules/attention.py:152-172
 *   udt_mattn_fwd       nn.MultiheadAttention (OCR scorer decoder)  src/parseq/strhub/models/parseq/modules.py:57-70
 *                       (also nn.MultiheadAttention inside nn.TransformerEncoderLayer,
 *                        sgm/modules/encoders/modules.py:1103-1104,1164)
 *   udt_softmax_rows    softmax of the VAE single-head attention  sgm/modules/diffusionmodules/model.py:246
 *   udt_gn_stats / udt_gn_apply
 *                       GroupNorm32 + SiLU      sgm/modules/diffusionmodules/util.py:258-275,
 *                                               sgm/modules/diffusionmodules/openaimodel.py:183-187,218-221,536-538
 *                       GroupNorm(eps 1e-6)     sgm/modules/attention.py:82-85,402 ; model.py:48-52,128-143
 *   udt_layernorm       nn.LayerNorm            sgm/modules/attention.py:297,310-311,315-339
 *   udt_unet_input / udt_unet_input_churn / udt_cfg_euler_step
 *                       guider.prepare_inputs + denoiser scaling + CFG + Euler update
 *                       sgm/modules/diffusionmodules/guiders.py:25-40, denoiser.py:22-28,
 *                       denoiser_scaling.py:16-22, sampling_utils.py:8-9,39-40, sampling.py:85-86,348-351
 *   udt_cfg_sampler_step  the same CFG denoise + the update of HeunEDMSampler, EulerAncestralSampler,
 *                       DPMPP2SAncestralSampler, DPMPP2MSampler (sampling.py:140-215,423-567) as one affine form
 *   udt_cfg_multistep_step  the same CFG denoise + the update of LinearMultistepSampler (sampling.py:180-215): to_d and
 *                       the linear multistep sum over up to 8 derivatives
 *   udt_posterior_sample  DiagonalGaussianDistribution.sample  sgm/modules/distributions/distributions.py:24-41
 *   udt_nchw_to_nhwc / udt_nhwc_to_nchw   layout change at the NCHW fp32 plugin boundary
 *                       (rearrange "b c h w -> b (h w) c", sgm/modules/attention.py:405,412)
 *   udt_embed_tokens    nn.Embedding + PositionalEncoding  sgm/modules/encoders/modules.py:1069-1085,1160-1163
 *   udt_timestep_embedding  timestep_embedding  sgm/modules/diffusionmodules/util.py:206-230
 *   udt_mask_downsample SpatialRescaler (bilinear x0.125)  sgm/modules/encoders/modules.py:843-857
 *   udt_crop_resize_aa_f32  the OCR scorer's input side, every box of every image in one launch: the crop results[i, :, t:b, l:r]
 *                       (test.py:81) + Resize(BICUBIC, antialias=True) + Normalize(0.5, 0.5)  sgm/modules/predictors/model.py:24-29
 *   udt_tattn_fused_maps / udt_resize_bilinear_f32   the per-character attention maps (cfgs.detailed): head mean of the t_attn
 *                       probabilities out of the fused kernel, openaimodel.py:559-591, sampling.py:344-346,380; cv2.resize, demo.py:109
 *   udt_lpips_input_f32 / udt_conv2d_f32 / udt_maxpool3s2_f32 / udt_lpips_layer_f32
 *                       lpips.im2tensor + lpips.LPIPS(net='alex').forward on the saved frames  metrics.py:16,24-27 (test.py:94-113,124)
 *   udt_fid_input_f32 / udt_conv2d_rect_f32 / udt_pool3_f32 / udt_mean_pixels_f32 / udt_moments_accum_f64
 *                       pytorch_fid's InceptionV3 pool features and their mean / covariance  metrics.py:5-10 (test.py:119-121)
 *   udt_local_loss_maps head-mean + 3x3 blur + masked max of t_attn maps  sgm/modules/diffusionmodules/loss.py:192-235
 *   the reverse pass (round 6; torch.autograd under attend_and_excite, sgm/modules/diffusionmodules/sampling.py:233-252, and under
 *   DiffusionEngine.training_step, sgm/models/diffusion.py:138-172 with loss.py:131-176,237-286):
 *     udt_attn_bwd, udt_xattn_bwd, udt_xattn_bwd_kv       autograd of the two attention call sites above
 *     udt_gn_bwd, udt_layernorm_bwd, udt_ln_param_grad, udt_geglu_fwd / _bwd   autograd of the norms / GEGLU
 *     udt_local_loss_bwd, udt_local_loss_seg_bwd, udt_diff_loss_grad          FullLoss.get_min_local_loss / get_local_loss / __call__
 *     udt_wgrad_bf16, udt_colsum_bf16                     weight / bias gradients of the trained nn.Linear layers
 *     udt_adamw_f32                                       torch.optim.AdamW.step (diffusion.py:49-51,202-222)
 *     udt_wgrad_bf16_acc, udt_colsum_bf16_acc, udt_ln_param_grad_acc      the same gradients ADDED to their destination: autograd's
 *                                                         accumulation into .grad across the micro-batches of a window
 *                                                         (configs/train.yaml:21 accumulate_grad_batches)
 *     udt_bucket_update_f32, udt_bucket_swap_f32          AdamW.step over every trained tensor + LitEma.forward (sgm/modules/ema.py:33-52),
 *                                                         LitEma.store / copy_to / restore (ema.py:56-86), one launch each
 *     udt_aae_row_update_f32                              the attend-and-excite update and exit rule (sampling.py:247-250), row by row
 *     (backward-data of linears and convolutions: udt_gemm on re-packed weights)
 *   the OCR loss on decoded frames and its gradient (FullLoss.get_ocr_loss, loss.py:178-190; ParseqPredictor.calc_loss,
 *   sgm/modules/predictors/model.py:40-58, under torch.autograd):
 *     udt_ocr_ce_f32                                      F.cross_entropy over the label's characters + clamp(max=1), with its seed
 *     udt_mattn_bwd                                       autograd of udt_mattn_fwd (ViT self-attention, decoder cross-attention)
 *     udt_gelu_fwd / udt_gelu_bwd                         nn.GELU of the ViT / decoder MLPs on stored pre-activations
 *     udt_crop_resize_aa_bwd_f32                          autograd of udt_crop_resize_aa_f32
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; kernels borrow it for the stream-ordered
 *     duration of the launch; the library allocates nothing on the data path and keeps no pointer.
 *   - activations are bf16, channel-last ("NHWC": [batch, pixels, channels]); weights are bf16,
 *     [out_features, K] with K contiguous; statistics / sampler state are fp32.
 *   - return value: 0 on success, a negative udt_status otherwise.  Nothing throws or aborts.
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*).
 */
#ifndef UDT_KERNELS_H
#define UDT_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  UDT_OK = 0,
  UDT_ERR_BAD_SHAPE = -1,     /* dimension not supported by the kernel (alignment / range)      */
  UDT_ERR_BAD_ARG = -2,       /* null pointer / inconsistent flags                                */
  UDT_ERR_WORKSPACE = -3,     /* workspace too small (see udt_gemm_workspace_bytes)               */
  UDT_ERR_HIP = -4,           /* a HIP runtime call failed; see udt_last_hip_error                */
  UDT_ERR_NO_DEVICE = -5,     /* no gfx950 device visible                                         */
  UDT_ERR_ASYNC = -6          /* a stream-K launch timed out waiting for a partner workgroup (its output
                                 tile is NaN-poisoned); reported by udt_check_async_error                */
} udt_status;

/* element types of packed weights (udt_pack_*) */
typedef enum {
  UDT_DTYPE_F32 = 0,
  UDT_DTYPE_BF16 = 1,
  UDT_DTYPE_FP8_E4M3 = 2      /* OCP e4m3 (not the fnuz format of MI300X) + one fp32 scale per output channel */
} udt_dtype;

/* ---- epilogue / mode flags for udt_gemm ------------------------------------------------------- */
#define UDT_GEMM_OUT_F32     (1 << 0)  /* out is fp32 instead of bf16                              */
#define UDT_GEMM_GEGLU       (1 << 1)  /* out[:, j] = x_j * gelu_erf(gate_j); weight rows packed
                                          in [32 x | 32 gate] blocks (see pack_geglu in Python)   */
#define UDT_GEMM_RELU        (1 << 2)
#define UDT_GEMM_TRANSPOSED  (1 << 3)  /* out is [batch_of_row][N][rows_per_batch] (V^T for attn)  */
#define UDT_GEMM_CONV        (1 << 4)  /* implicit-GEMM convolution, A gathered from NHWC sources   */
#define UDT_GEMM_SILU_OUT    (1 << 5)  /* out = silu(acc...) (time_embed MLP)                      */
/* (1 << 6) was UDT_GEMM_FP8 — round 2's first-generation fp8 path (unit block scales, a per-tensor activation scale written by a
   quantising LayerNorm kernel): slower than the LayerNorm-folded bf16 GEMMs, retired in round 5 in favour of UDT_GEMM_MX8. */
#define UDT_GEMM_MX8         (1 << 7)  /* BASELINE config #5: a is an MX8 activation — OCP e4m3
                                          bytes [M, lda] + one E8M0 block scale per 32 K-elements of a
                                          row (a_scale) — and w is e4m3 [N, ldw] + per-channel fp32 scales
                                          (colscale); K % 128 == 0, lda / ldw % 16 == 0.  Plain, LayerNorm-
                                          folded (rowstat_in) and GEGLU epilogues on the lean kernel family;
                                          see the q8_out / rowstat_* fields.                              */

typedef struct {
  /* operands */
  const void* a;        /* bf16 [M, lda] (plain) or NHWC source 1 [B, Hin, Win, C1] (conv)        */
  const void* a2;       /* conv only: optional NHWC source 2 [B, Hin, Win, C2] (channel concat)   */
  const void* w;        /* bf16 [N, K] K-contiguous; conv: k = (ky*ksize + kx)*(C1+C2) + c        */
  const float* bias;    /* [N] fp32 or NULL                                                       */
  const void* residual; /* bf16 [M, ldr] or NULL, added in the epilogue                           */
  const float* rowvec;  /* fp32 [M / rows_per_batch, N] or NULL (time-embedding broadcast add)    */
  void* out;            /* bf16 / fp32 [M, ldo] (or transposed, see flag)                         */
  int32_t M, N, K;
  int32_t lda, ldo, ldr;
  int32_t ldw;          /* elements between rows of w (0 = K)                                       */
  /* batched GEMM (grid.z): element strides between problems; batch = 1 for none                  */
  int32_t batch;
  int64_t stride_a, stride_w, stride_out, stride_res;
  /* conv geometry (UDT_GEMM_CONV)                                                                */
  int32_t Hin, Win, C1, C2, Hout, Wout;
  int32_t ksize;        /* 1 or 3                                                                 */
  int32_t stride;       /* 1 or 2                                                                 */
  int32_t pad_t, pad_l; /* zero padding before the first row / column (bottom/right implicit)     */
  int32_t upsample;     /* 1: sources are read through a nearest x2 upsample
                           2: the same result as four 2x2 phase convolutions of the low-resolution map (3x3 / stride 1 /
                              pad 1 only): `w` is the up4 layout bf16 [4][rows][ldw], phase 2a+b of output pixel
                              (2i+a, 2j+b), k = (2r+s)*C1 + c over low-resolution pixel (i-1+a+r, j-1+b+s), weights
                              summed over the duplicated taps; ldw (0 = 4*C1) counts ITS row, stride_w (0 = N*ldw) the
                              elements between phases, K stays 9*C1.  Ask udt_gemm_up4_ok first.                        */
  int32_t rows_per_batch; /* rows of M belonging to one sample (rowvec / transposed addressing)   */
  int32_t ld_rowvec;    /* elements between rows of rowvec (0 = N)                                 */
  int32_t flags;
  float alpha;          /* acc * alpha before bias (softmax scale for QK^T GEMMs); 1.0 default    */
  /* fused GroupNorm (north star: "3x3 conv + GroupNorm + SiLU fused blocks"; reference chain
     openaimodel.py:183-187,218-231, util.py:258-275, model.py:128-148)                                             */
  const float* colscale;/* UDT_GEMM_MX8 only: fp32 [N] per-output-channel weight scales (in packed row order), or NULL */
  const float* in_scsh; /* 3x3 / stride 1 / pad 1 convolutions only (see udt_gn_silu_conv3x3_fwd): per-(sample,
                           channel) scale / shift from udt_gn_finalize, applied — with in_act — to the input patch
                           as it is staged in LDS: y = act(x * scale + shift); zero padding stays zero.  NULL = off */
  int32_t in_act;       /* 0 none, 1 SiLU                                                                          */
  float* colstats;      /* optional output: per-(row slot, output column) partial (sum, sum of squares) of the
                           result, fp32 [udt_gemm_colstats_slots][N][2]: the GroupNorm statistics of the NEXT
                           layer come out of this layer's epilogue.  NULL = off                                   */
  int32_t cu_share;     /* number of launch streams that share the device with this call (0 / 1: none).
                           The persistent stream-K kernels wait on partner workgroups, so all their
                           workgroups must be resident: the launch is planned for 1/cu_share of the CUs.
                           udt_gemm_workspace_bytes must be asked with the same value.                  */
  /* LayerNorm prologue (udt_ln_gemm_fwd; reference attention.py:310-339 `attn1(norm1(x))` / `ff(norm3(x))`): `a` holds
     the RAW rows x, `w` = gamma o W (LayerNorm scale folded into the weight columns), `bias` = c_n = sum_k beta_k W_nk
     + linear bias, ln_colsum = s_n = sum_k w_nk (fp32 [N], of the bf16-rounded folded weights); the kernel takes every
     row's mean / rstd from the A tiles it streams and computes out = rstd (x w^T - mean s) + c.  K = normalised width. */
  const float* ln_colsum;
  float ln_eps;
  /* MX8 activations (UDT_GEMM_MX8 and the emitting epilogues; reference call sites: every nn.Linear of the transformer blocks,
     attention.py:44-70,193-199,375-411).  An MX8 activation of C columns is (elements: e4m3 bytes [M, ld >= C];
     scales: uint32 [ceil(C / 128)][M], byte j of dword (t, m) = E8M0 scale of columns [128 t + 32 j, + 32) of row m:
     value = e4m3 * 2^(scale - 127)).                                                                                   */
  const void* a_scale;     /* UDT_GEMM_MX8: the block scales of `a`                                                     */
  void* q8_out;            /* optional second output: the result (after bias / residual / GEGLU, as rounded for `out`) again
                              as an MX8 activation for the next GEMM; `out` may then be NULL.  Lean
                              128 x 128 plans and the row-resident LayerNorm-folded K = 320 plan only (udt_gemm_q8_ok), N % 32 == 0
                              (GEGLU: N % 64 == 0)                                                                         */
  void* q8_scale;          /* its block scales (see above)                                                               */
  int32_t ld_q8;           /* bytes between rows of q8_out (% 8 == 0)                                                    */
  int32_t q8_fixed_col;    /* 0 = off; else result columns >= q8_fixed_col (a multiple of 32; 64 on the row-resident plan) are written as e4m3(value * q8_fixed_mul > 0),
                              clamped to +-448, with the unit scale byte 127 instead of block scales: the v third of a q|k|v
                              projection feeding udt_attn_mx8_fwd, whose P V product contracts over keys                        */
  float q8_fixed_mul;
  float* rowstat_out;      /* optional, with q8_out (not GEGLU): fp32 [udt_gemm_rowstat_parts(d)][M][2] partial (sum, sum of
                              squares) of every result row — the LayerNorm statistics of a LayerNorm-folded MX8 consumer  */
  const float* rowstat_in; /* UDT_GEMM_MX8 with ln_colsum: the partial row statistics of `a` its producer emitted,
                              fp32 [rowstat_in_parts][M][2]; summed in index order (deterministic)                        */
  int32_t rowstat_in_parts;
} udt_gemm_desc;

/* workspace (bytes) udt_gemm needs for this problem (split-K slabs); 0 if none.  The first 4 KiB of a workspace are
 * the kernels' slab flags + error word: zero them once when the buffer is allocated (they are zero again after
 * every successful launch) and give concurrent streams separate workspaces. */
size_t udt_gemm_workspace_bytes(const udt_gemm_desc* d);
/* Limits: the MFMA kernels address one operand (one batch element) through 31-bit byte offsets — an A or W operand of 2 GiB or more
 * is only served for outputs of <= 64 columns (the first-generation 256 x 64 kernel); wider problems of that size return
 * UDT_ERR_BAD_SHAPE (udt_gemm_workspace_bytes answers 0 for them: nothing to plan).  No shape of the UNet / VAE comes near. */
int udt_gemm(const udt_gemm_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* Column-statistics geometry of udt_gemm for this problem: rows of the output covered by one slot of `colstats`
 * (32 or 64; slot s covers rows [s*rows, (s+1)*rows) of M for plain GEMMs / gathered convolutions and the same number of
 * pixels of ONE image in tile order for the patch-staged convolution — either way the slots of a sample are contiguous:
 * slots_per_sample = rows_per_batch / rows) and the number of slots.  0 = this problem cannot emit them (transposed /
 * GEGLU / fp32 outputs, first-generation kernel, rows_per_batch not a multiple of the slot). */
int32_t udt_gemm_colstats_rows(const udt_gemm_desc* d);
/* Parts of the partial row statistics (rowstat_out) udt_gemm would emit for this problem = N / (columns per wave of the plan);
 * 0 = the plan has no MX8-emitting epilogue (q8_out / rowstat_out must then be NULL). */
int32_t udt_gemm_rowstat_parts(const udt_gemm_desc* d);
/* 1 if udt_gemm would take this descriptor WITH its q8_out / q8_scale (an MX8-emitting epilogue exists for the plan), else 0. */
int32_t udt_gemm_q8_ok(const udt_gemm_desc* d);
int32_t udt_gemm_colstats_slots(const udt_gemm_desc* d);
/* 1 if udt_gemm accepts `in_scsh` for this problem (patch-staged 3x3 convolution geometry; one or two NHWC sources). */
int32_t udt_gemm_in_scsh_ok(const udt_gemm_desc* d);
/* 1 if udt_gemm serves this descriptor in the phase form (upsample = 2), else 0: the caller then sets upsample = 1 and passes the
 * 3x3 weights (fewer than 128 output channels, C1 not a multiple of 64, two sources, in_scsh, fp32 output, maps that do not tile). */
int32_t udt_gemm_up4_ok(const udt_gemm_desc* d);
/* The north star's fused block under its own name: GroupNorm(+SiLU) applied on the staged input patch -> 3x3 conv ->
 * epilogue (bias, time-embedding row vector, residual) -> optional statistics of the output.  Same as udt_gemm with a
 * descriptor that has UDT_GEMM_CONV, ksize 3, stride 1, pad 1 and in_scsh set; anything else is UDT_ERR_BAD_ARG. */
int udt_gn_silu_conv3x3_fwd(const udt_gemm_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* LayerNorm -> linear in one launch (SURVEY.md §8b `udt_ln_gemm_fwd`; reference attention.py:310-339: `attn1(norm1(x))`,
 * `ff(norm3(x))`, LayerNorm over the last dimension = the GEMM's K).  Descriptor as for udt_gemm with the ln_colsum /
 * ln_eps fields set (see udt_gemm_desc); plain or GEGLU epilogue, optional residual.  UDT_ERR_BAD_SHAPE when the
 * problem is outside the lean GEMM family (N <= 64, fp32 / transposed outputs, batched). */
int udt_ln_gemm_fwd(const udt_gemm_desc* d, void* workspace, size_t workspace_bytes, void* stream);
/* Synchronises `stream` and reports (UDT_ERR_ASYNC) whether any udt_gemm launch that used `workspace` gave up waiting
 * for a partner workgroup since the last check; in that case the header is re-zeroed so the workspace stays usable.
 * Callers check at their natural sync points (the sampler: once per sampling loop). */
int udt_check_async_error(void* workspace, size_t workspace_bytes, void* stream);

/* ---- attention -------------------------------------------------------------------------------- */
/* Flash attention forward, head_dim 64, no mask:  O = softmax(Q K^T * scale) V
 *   q  : bf16, row (b, tok) at q  + b*q_bstride  + tok*ldq + h*64
 *   k  : bf16, row (b, tok) at k  + b*k_bstride  + tok*ldk + h*64
 *   vt : bf16 V transposed: element (b, h*64+d, tok) at vt + b*vt_bstride + (h*64+d)*ldvt + tok
 *   o  : bf16, row (b, tok) at o  + b*o_bstride  + tok*ldo + h*64
 * nk must be a multiple of 8. */
int udt_attn_fwd(const void* q, const void* k, const void* vt, void* o,
                 int32_t batch, int32_t heads, int32_t nq, int32_t nk,
                 int32_t ldq, int32_t ldk, int32_t ldvt, int32_t ldo,
                 int64_t q_bstride, int64_t k_bstride, int64_t vt_bstride, int64_t o_bstride,
                 float scale, void* stream);

/* Short-context attention (context length L <= 16; text cross-attention, LabelEncoder self-attn):
 *   q  : bf16 [batch, nq, heads*head_dim] (ldq), k/v : bf16 rows (b, l) at k + (b*L + l)*ldkv + h*head_dim
 *   o  : bf16 [batch, nq, heads*head_dim] (ldo)
 *   probs (optional, may be NULL): fp32 [batch*heads, nq, L] — the softmax probabilities the
 *   reference caches in attn_map_cache (attention.py:165-169), "(b h) n l" order.
 * head_dim must be a multiple of 64. */
int udt_xattn_fwd(const void* q, const void* k, const void* v, void* o, float* probs,
                  int32_t batch, int32_t heads, int32_t head_dim, int32_t nq, int32_t L,
                  int32_t ldq, int32_t ldkv, int32_t ldo, float scale, void* stream);

/* The same with V row-major like K (row (b, tok) at v + b*v_bstride + tok*ldv + h*64): q, k and v may then be column
 * ranges of ONE q|k|v projection output (reference attention.py:193-199: to_q / to_k / to_v on the same input). */
int udt_attn_rowv_fwd(const void* q, const void* k, const void* v, void* o,
                      int32_t batch, int32_t heads, int32_t nq, int32_t nk,
                      int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                      int64_t q_bstride, int64_t k_bstride, int64_t v_bstride, int64_t o_bstride,
                      float scale, void* stream);
/* The same launch that ALSO writes O as an MX8 activation (udt_gemm_desc "MX8 activations": q8_out e4m3 [batch * nq, ld_q8], column
 * h * 64 + d; q8_scale uint32 [heads * 64 / 128][batch * nq]) for the e4m3 `to_out` GEMM of BASELINE config #5 (reference
 * attention.py:246-262).  heads even, ld_q8 >= heads * 64, ld_q8 % 4 == 0, o_bstride == nq * ldo. */
int udt_attn_rowv_q8_fwd(const void* q, const void* k, const void* v, void* o,
                         int32_t batch, int32_t heads, int32_t nq, int32_t nk,
                         int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                         int64_t q_bstride, int64_t k_bstride, int64_t v_bstride, int64_t o_bstride,
                         float scale, void* q8_out, void* q8_scale, int32_t ld_q8, void* stream);

/* BASELINE config #5's "fp8 attention": the same self-attention on e4m3 operands (v_mfma_scale_f32_32x32x64_f8f6f4 for Q K^T and
 * P V; fp32 softmax).  q, k, v are column ranges of ONE MX8 activation qkv8 [batch * n, ld8] — q at column h * 64, k at C + h * 64,
 * v at 2 C + h * 64, C = heads * 64 — written by the q|k|v projection's emitting epilogue (udt_gemm_desc.q8_out) with
 * q8_fixed_col = 2 C: q and k carry block scales along the head dimension (qkv_scale, uint32 [ld8 / 128 rounded up][batch * n]),
 * v was multiplied by q8_fixed_mul; v_inv = 1 / q8_fixed_mul.  o: bf16 rows b * n + i of ldo elements; q8_out / q8_scale / ld_q8
 * (optional): O again as an MX8 activation, as udt_attn_rowv_q8_fwd (heads even for it).  n % 4 == 0, ld8 % 16 == 0, qkv8 16-byte aligned.
 * Reference: sgm/modules/attention.py:236-248. */
int udt_attn_mx8_fwd(const void* qkv8, const void* qkv_scale, void* o, int32_t batch, int32_t heads, int32_t n,
                     int32_t ld8, int32_t ldo, float scale, float v_inv, void* q8_out, void* q8_scale, int32_t ld_q8,
                     void* stream);

/* Flash attention forward for ONE head of 512 dims: the AutoencoderKL mid-block attention (reference
 * sgm/modules/diffusionmodules/model.py:236-260, MemoryEfficientAttnBlock.attention: xformers.ops.memory_efficient_attention on
 * [B, H*W, 512]; AttnBlock.attention, model.py:169-190, is the same product through softmax(q k^T / sqrt(C)) v).
 *   q, k, v : bf16 rows (b, tok) at x + b*x_bstride + tok*ldx, 512 dims each — they may be column ranges of ONE q|k|v projection
 *   o       : bf16 rows of 512 dims (ldo); nq / nk arbitrary (keys past nk are masked), 16-byte aligned q / k / v, ld % 8 == 0.
 * No [nq, nk] score tensor is materialised (the score tile of 32 queries x 32 keys lives in registers / LDS). */
int udt_attn512_fwd(const void* q, const void* k, const void* v, void* o,
                    int32_t batch, int32_t nq, int32_t nk,
                    int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                    int64_t q_bstride, int64_t k_bstride, int64_t v_bstride, int64_t o_bstride,
                    float scale, void* stream);

/* The same product with the KEYS split over workgroups (flash-decoding form) for grids whose query tiles alone leave most of
 * the 256 CUs idle — a single 512 x 512 image is 64 query tiles, each walking all 4096 keys: the keys are cut into up to 8
 * slices of >= 256 keys, every (query tile, slice) workgroup parks its unnormalised fp32 partial O and (running maximum, row
 * sum) in `workspace`, and a merge launch on the same stream combines the slices in index order (deterministic).
 *   udt_attn512_workspace_bytes : bytes the split form needs for (batch, nq, nk); 0 = the grid is large enough, no split.
 *   udt_attn512_split_fwd       : as udt_attn512_fwd; workspace 16-byte aligned, >= the bytes above (UDT_ERR_WORKSPACE
 *                                 otherwise); with workspace == NULL, or when no split is planned, it IS udt_attn512_fwd. */
size_t udt_attn512_workspace_bytes(int32_t batch, int32_t nq, int32_t nk);
int udt_attn512_split_fwd(const void* q, const void* k, const void* v, void* o,
                          int32_t batch, int32_t nq, int32_t nk,
                          int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                          int64_t q_bstride, int64_t k_bstride, int64_t v_bstride, int64_t o_bstride,
                          float scale, void* workspace, size_t workspace_bytes, void* stream);

/* Masked small attention (the OCR scorer's decoder: nn.MultiheadAttention of PARSeq's DecoderLayer, reference
 * src/parseq/strhub/models/parseq/modules.py:35-36,57-70 -> torch's scaled-dot-product with attn_mask and
 * key_padding_mask).  Few queries against a short key set, any head_dim that is a multiple of 8 up to 64:
 *   q : bf16 rows (b, i) at q + b*q_bstride + i*ldq + h*head_dim      i < nq
 *   k, v : bf16 rows (b, l) at k + b*k_bstride + l*ldk + h*head_dim   l < lk, lk <= 256, lk*head_dim <= 8192
 *   o : bf16 rows (b, i) at o + b*o_bstride + i*ldo + h*head_dim
 *   mask (optional): fp32 [nq, ldmask] added to the scaled scores (-inf = masked), shared by batch and heads
 *   kpm  (optional): uint8 [batch, lk], non-zero = the key is padding (ignored)
 * fp32 scores, softmax and accumulation.  A query whose keys are all masked yields zeros (torch yields NaN). */
int udt_mattn_fwd(const void* q, const void* k, const void* v, void* o, const float* mask, const uint8_t* kpm,
                  int32_t batch, int32_t heads, int32_t head_dim, int32_t nq, int32_t lk,
                  int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo, int32_t ldmask,
                  int64_t q_bstride, int64_t k_bstride, int64_t v_bstride, int64_t o_bstride, float scale, void* stream);

/* The text cross-attention branch of a transformer block as ONE kernel (csrc/tattn.hip):
 *   out = x + to_out(softmax(to_q(LayerNorm(x)) K^T * scale) V) + bias        reference sgm/modules/attention.py:140-174,326-333
 * The context is constant during sampling and has L <= 12 tokens, so udt_tattn_prepare folds it ONCE per batch into
 * per-sample tables, opaque to the caller (exact re-association; stored in the MFMA fragment order of the consuming kernel): A' [B][hp][C] bf16 (LayerNorm gamma, to_q and K folded; hp = udt_tattn_hp(heads)
 * = 16 columns per head, rounded up to 32), sc [B][hp][2] fp32 (the LayerNorm mean / beta terms), BmT [B][C][hp] bf16 (V and
 * to_out folded).  udt_tattn_fused then needs only the raw rows: x, out bf16 [B * n_tok, C]; the kernel is
 * instantiated for the UNet's three widths — C = 64 * heads with heads = 5, 10, 20 — anything else is UDT_ERR_BAD_SHAPE
 * (n_tok % 64 == 0, or % 32 for C = 1280); the first `zero_samples` samples attend to an all-zero context and get
 * x + bias (no tables needed when zero_samples == B).
 *   kv: bf16 [B, L, ldkv], k in columns [0, C), v in [C, 2C) (the hoisted to_k|to_v projection); wq: bf16 [C, ldwq] (to_q
 *   weight, rows = output features), wo: bf16 [C, ldwo] (to_out weight); gamma / beta: t_norm; bias: to_out bias. */
int32_t udt_tattn_hp(int32_t heads);
int udt_tattn_prepare(const void* kv, int32_t ldkv, const void* wq, int32_t ldwq, const void* wo, int32_t ldwo,
                      const float* gamma, const float* beta, void* A, float* sc, void* BmT, int32_t B, int32_t L,
                      int32_t C, int32_t heads, float scale, void* stream);
int udt_tattn_fused(const void* x, void* out, const void* A, const float* sc, const void* BmT, const float* bias,
                    int32_t B, int32_t n_tok, int32_t C, int32_t heads, int32_t zero_samples, float eps, void* stream);
/* The same launch that ALSO writes its result as an MX8 activation (udt_gemm_desc "MX8 activations": q8_out e4m3 [B * n_tok, C],
 * q8_scale uint32 [C / 128][B * n_tok]) and the partial row statistics (rowstat_out fp32 [udt_tattn_rowstat_parts][B * n_tok][2]) for
 * the LayerNorm-folded GEGLU projection that consumes it on the e4m3 path (BASELINE config #5; reference attention.py:326-339:
 * `x = t_attn(...) + x; x = ff(norm3(x)) + x`).  C = 640 / 1280.  udt_tattn_rowstat_parts: 0 = no such instance for the shape. */
int32_t udt_tattn_rowstat_parts(int32_t B, int32_t n_tok, int32_t C);
int udt_tattn_fused_q8(const void* x, void* out, const void* A, const float* sc, const void* BmT, const float* bias,
                       int32_t B, int32_t n_tok, int32_t C, int32_t heads, int32_t zero_samples, float eps, void* q8_out,
                       void* q8_scale, float* rowstat_out, void* stream);
/* udt_tattn_fused (q8_out == NULL) or udt_tattn_fused_q8 (q8_out != NULL: q8_scale and rowstat_out as there) that ALSO writes the
 * per-character attention maps of the launch, the reference's head mean of the text-attention probabilities (cfgs.detailed:
 * sgm/modules/diffusionmodules/openaimodel.py:559-591, sampling.py:344-346,380):
 *   maps[b - map_from][l][t]  (=  or  +=)  weight * (1 / heads) * sum_h P[b, t, h, l]      b >= map_from, l < L, t < n_tok
 * maps fp32 [B - map_from, L, n_tok], token fastest (the reference's permute(0, 2, 1).reshape(b, l, h, w), row-major over the h x w
 * tokens).  Domain: that of the plain entry point, plus 1 <= L <= 12 = the context length the tables were prepared for (the 16 - L
 * padded columns of a head are never read into a map) and zero_samples <= map_from <= B: samples below map_from (the unconditional
 * half of a CFG pair, zero-context rows) have no plane.  accumulate == 0 stores, != 0 adds to what maps holds: the selected layers of
 * one UNet call average into one buffer in launch order (weight = 1 / n_layers; the first stores, the rest add).
 * out, q8_out, q8_scale and rowstat_out are bit-identical to the plain entry point's on the same operands.
 * ROUNDING (maps): each probability is the bf16 value the output GEMM of the kernel reads (the fp32 softmax rounded to bf16 once,
 * to nearest even); the heads are added in ascending order in fp32; the sum is multiplied by fp32(weight / heads) and rounded;
 * accumulate adds that to the stored fp32 value and rounds once more.  One workgroup per token tile writes and nothing is atomic:
 * bit-identical from run to run.
 * UDT_ERR_BAD_ARG: a null maps (and what the plain entry point answers it for); UDT_ERR_BAD_SHAPE: L < 1, L > 12, map_from outside
 * [zero_samples, B] (and what the plain entry point answers it for).  Nothing is launched in either case. */
int udt_tattn_fused_maps(const void* x, void* out, const void* A, const float* sc, const void* BmT, const float* bias,
                         int32_t B, int32_t n_tok, int32_t C, int32_t heads, int32_t zero_samples, float eps, float* maps,
                         int32_t L, int32_t map_from, float weight, int32_t accumulate, void* q8_out, void* q8_scale,
                         float* rowstat_out, void* stream);

/* Row softmax of a bf16 [rows, cols] matrix in place (ld elements between rows), fp32 math. */
int udt_softmax_rows(void* x, int64_t rows, int32_t cols, int32_t ld, void* stream);

/* ---- normalisation ---------------------------------------------------------------------------- */
/* GroupNorm statistics over NHWC bf16 x [B, HW, C] with G groups (C % G == 0, C % 8 == 0).
 * Writes per-chunk partial (sum, sumsq) to `partials` (fp32 [B, nchunks, G, 2]); nchunks is returned
 * by udt_gn_nchunks(HW, C). */
int32_t udt_gn_nchunks(int64_t HW, int32_t C);
int udt_gn_stats(const void* x, const void* x2, float* partials, int32_t B, int64_t HW, int32_t C, int32_t C2,
                 int32_t G, void* stream);
/* y = act((x - mean) * rstd * gamma + beta); act: 0 none, 1 SiLU.  y may alias x when x2 == NULL.
 * x2 (optional, C2 channels) is a second NHWC source concatenated after x's C channels (UNet skip concat,
 * openaimodel.py:620); statistics and output cover the C + C2 concatenated channels, y is [B, HW, C + C2].
 * udt_gn_apply also requires G <= 256 and 256 % G == 0 (its 256 threads combine the chunk partials as G groups x 256 / G lanes);
 * both require C + C2 <= 4096. */
int udt_gn_apply(const void* x, const void* x2, void* y, const float* partials, const float* gamma,
                 const float* beta, int32_t B, int64_t HW, int32_t C, int32_t C2, int32_t G, float eps, int32_t act,
                 void* stream);
/* One-launch GroupNorm (+ optional SiLU) for shapes whose per-sample group strips fit the caches (udt_gn_strip_ok): a
 * workgroup owns a few consecutive groups of one sample, reads them once for the statistics and again (out of L2) to
 * normalise.  Same arguments and result as udt_gn_stats + udt_gn_apply (statistics summed in a different order). */
int32_t udt_gn_strip_ok(int32_t B, int64_t HW, int32_t C1, int32_t C2, int32_t G);
int udt_gn_strip(const void* x, const void* x2, void* y, const float* gamma, const float* beta, int32_t B, int64_t HW,
                 int32_t C1, int32_t C2, int32_t G, float eps, int32_t act, void* stream);

/* GroupNorm statistics from producer epilogues -> per-(sample, channel) scale / shift for udt_gemm's in_scsh.
 *   stats1 fp32 [B * slots1][C1][2] (+ optional stats2 [B * slots2][C2][2] for a channel concat x ‖ x2): the colstats of
 *   the layer(s) that produced the input; slotsN = slots per sample.  Groups run over the C1 + C2 concatenated channels.
 *   scsh out fp32 [B][(C1+C2)/64][2][64]: chunk-blocked (scale of 64 channels, then their shift) — the layout the
 *   convolution's LDS-DMA reads.  scale = rstd * gamma, shift = beta - mean * scale; fp32 partials, fp64 combine.
 *   (C1 + C2) % 64 == 0, (C1 + C2) % G == 0, G <= 256, (C1 + C2) / G <= 128 (one workgroup of 256 threads per (sample, group):
 *   256 / ((C1 + C2) / G) slot lanes per channel). */
int udt_gn_finalize(const float* stats1, int32_t slots1, int32_t C1, const float* stats2, int32_t slots2, int32_t C2,
                    const float* gamma, const float* beta, float* scsh, int32_t B, int64_t HW, int32_t G, float eps,
                    void* stream);

/* GroupNorm (+ SiLU) from a finished scale / shift table: y = act(x * scale[b, c] + shift[b, c]) with `scsh` as written by
 * udt_gn_finalize from the column statistics the PRODUCERS of x (and x2) emitted in their epilogues (udt_gemm_desc.colstats) —
 * the statistics pass over the tensor is gone, this is the one remaining read + write of reference GroupNorm32 -> SiLU
 * (sgm/modules/diffusionmodules/util.py:214-216, openaimodel.py:183-187).  Two sources = the channel concat of a decoder
 * ResBlock's input; C1 + C2 a multiple of 64. */
int udt_gn_apply_scsh(const void* x, const void* x2, void* y, const float* scsh, int32_t B, int64_t HW, int32_t C1,
                      int32_t C2, int32_t act, void* stream);

/* The one-launch strip GroupNorm (udt_gn_strip) when the producers of x (and x2) emitted column statistics
 * (udt_gemm_desc.colstats: fp32 [B * slots][C][2]): the statistics pass over the strip becomes a sum over `slots` records per
 * channel, the launch is the normalise(+SiLU) pass alone.  Same shapes as udt_gn_strip (udt_gn_strip_ok). */
int udt_gn_strip_stats(const void* x, const void* x2, void* y, const float* stats1, int32_t slots1, const float* stats2,
                       int32_t slots2, const float* gamma, const float* beta, int32_t B, int64_t HW, int32_t C1, int32_t C2,
                       int32_t G, float eps, int32_t act, void* stream);

/* LayerNorm over the last dim of bf16 [rows, C] (C % 8 == 0, C <= 4096). */
int udt_layernorm(const void* x, void* y, const float* gamma, const float* beta,
                  int64_t rows, int32_t C, float eps, void* stream);
/* ---- sampler / boundary elementwise ------------------------------------------------------------ */
/* UNet input for one CFG step: x fp32 NCHW [B,4,h,w] -> xin bf16 NHWC [2B, h*w, cpad]; channels 0..3 of
 * both halves = x * c_in; the other channels (mask / masked latent / zero pad) are left untouched. */
int udt_unet_input(const float* x, void* xin, int32_t B, int32_t hw, int32_t cpad, float c_in, void* stream);
/* udt_unet_input of a churned (stochastic) Euler step, one launch: x <- x + kn*noise in place (noise fp32 NCHW [B,4,h,w], not
 * x itself; kn = s_noise*sigma*sqrt(gamma^2 + 2*gamma) from the host), then channels 0..3 of both halves = the STORED x * c_in,
 * bit-equal to udt_unet_input on the updated x.  B*hw <= 0x7fffffff. */
int udt_unet_input_churn(float* x, const float* noise, void* xin, int32_t B, int32_t hw, int32_t cpad, float c_in, float kn,
                         void* stream);
/* eps fp32 [2B, hw, ld_eps] (uncond half first) -> x fp32 NCHW [B,4,h,w] updated in place:
 *   den_u = x + c_out*eps_u ; den_c = x + c_out*eps_c (c_out = -quantised sigma) ; den = den_u + scale*(den_c - den_u)
 *   d = (x - den)/sigma ; x += d*(sigma_next - sigma)          (optionally writes den) */
int udt_cfg_euler_step(float* x, const float* eps, float* denoised_out, int32_t B, int32_t hw, int32_t ld_eps,
                       float c_out, float sigma, float sigma_next, float cfg_scale, void* stream);
/* Generic CFG sampler step (one launch per UNet evaluation of any sampler of this package):
 *   den  = den_u + scale*(den_c - den_u),  den_{u,c} = xin + c_out*eps_{u,c}     (c_out = -quantised sigma)
 *   xout = kx*xin + kd*den + ka*aux + kp*prev + kn*noise     (a null pointer drops its term)
 *   den_out = den                                             (optional)
 * eps fp32 [2B, hw, ld_eps] (uncond half first, 16-byte aligned); xin, aux, prev, noise, xout, den_out fp32 NCHW [B,4,h,w].
 * xout may alias xin or aux; den_out aliases none of the others.  Coefficients are computed on the host (float64, then
 * rounded); e.g. Euler ancestral kx = 1 + (s_down - s)/s, kd = -(s_down - s)/s, kn = s_noise*s_up;
 * DPM++ 2M kx = m1, kd = -m2*m3, kp = m2*m4 (prev = the previous step's den). */
typedef struct {
  float kx, kd, ka, kp, kn;
  float c_out, scale;
} udt_sampler_coefs;
int udt_cfg_sampler_step(const float* xin, const float* eps, const float* aux, const float* prev, const float* noise,
                         float* xout, float* denoised_out, int32_t B, int32_t hw, int32_t ld_eps, udt_sampler_coefs k,
                         void* stream);
/* CFG linear-multistep step (one launch per UNet evaluation of LinearMultistepSampler):
 *   den   = den_u + scale*(den_c - den_u),  den_{u,c} = xin + c_out*eps_{u,c}     (c_out = -quantised sigma)
 *   d     = (xin - den) / sigma                                                  (unquantised sigma: to_d)
 *   xout  = xin + (k[0]*d + k[1]*hist[1] + ... + k[n-1]*hist[n-1])               (summed in this order)
 *   d_out = d
 * eps fp32 [2B, hw, ld_eps] (uncond half first, 16-byte aligned); xin, hist[1..n-1], xout, d_out fp32 NCHW [B,4,h,w].
 * hist[j] is the derivative of j evaluations ago (hist[0] is unused); k[] are the quadrature coefficients of
 * sampling_utils.linear_multistep_coeff, computed on the host in float64 and rounded.  1 <= n <= UDT_MULTISTEP_MAX.
 * xout may alias xin; d_out aliases none of xin, xout and hist[1..n-1]. */
#define UDT_MULTISTEP_MAX 8
typedef struct {
  float c_out, scale, sigma;
  int32_t n;
  float k[UDT_MULTISTEP_MAX];
  const float* hist[UDT_MULTISTEP_MAX];
} udt_multistep_coefs;
int udt_cfg_multistep_step(const float* xin, const float* eps, float* xout, float* d_out, int32_t B, int32_t hw,
                           int32_t ld_eps, udt_multistep_coefs k, void* stream);
/* ---- the same four launches under any preconditioning (denoiser_scaling.py: Eps / V / EDM) and with or without guidance ----
 * F is the network output, fp32 [2B, hw, ld_f] (uncond half first) when pair != 0 (VanillaCFG), fp32 [B, hw, ld_f] when pair == 0
 * (IdentityGuider); 16-byte aligned, ld_f >= 4, ld_f % 4 == 0, B*hw <= 0x7fffffff.  c_skip, c_out, c_in are host floats (float64
 * from the possibly quantised sigma, rounded once).
 *   pair != 0: den_u = c_skip*x + c_out*F_u ; den_c = c_skip*x + c_out*F_c ; den = den_u + scale*(den_c - den_u)
 *   pair == 0: den   = c_skip*x + c_out*F                                     (scale is not read)
 * udt_cfg_euler_step / udt_cfg_sampler_step / udt_cfg_multistep_step are these with c_skip = 1, pair = 1, bit for bit. */
/* UNet input: channels 0..3 of rows [0, B) of xin bf16 NHWC [(pair ? 2B : B), hw, cpad] = x * c_in, and of rows [B, 2B) as well when
 * pair != 0; rows [B, 2B) are not written when pair == 0.  noise != NULL: the churned form, x <- x + kn*noise in place first
 * (noise fp32 NCHW [B,4,h,w], not x itself), the packed value is the STORED x * c_in. */
int udt_precond_unet_input(float* x, const float* noise, void* xin, int32_t B, int32_t hw, int32_t cpad, float c_in, float kn,
                           int32_t pair, void* stream);
/*   d = (x - den)/sigma ; x += d*(sigma_next - sigma)          (optionally writes den; den_out is not x) */
int udt_precond_euler_step(float* x, const float* f, float* denoised_out, int32_t B, int32_t hw, int32_t ld_f, float c_skip,
                           float c_out, float sigma, float sigma_next, float cfg_scale, int32_t pair, void* stream);
/*   xout = kx*xin + kd*den + ka*aux + kp*prev + kn*noise     (a null pointer drops its term) ; den_out = den (optional)
 * c_out and scale are k.c_out and k.scale; aliasing as udt_cfg_sampler_step. */
int udt_precond_sampler_step(const float* xin, const float* f, const float* aux, const float* prev, const float* noise,
                             float* xout, float* denoised_out, int32_t B, int32_t hw, int32_t ld_f, udt_sampler_coefs k,
                             float c_skip, int32_t pair, void* stream);
/*   d = (xin - den)/sigma ; xout = xin + (k[0]*d + k[1]*hist[1] + ... + k[n-1]*hist[n-1]) ; d_out = d
 * c_out, scale and sigma are k.c_out, k.scale and k.sigma; aliasing as udt_cfg_multistep_step. */
int udt_precond_multistep_step(const float* xin, const float* f, float* xout, float* d_out, int32_t B, int32_t hw, int32_t ld_f,
                               udt_multistep_coefs k, float c_skip, int32_t pair, void* stream);
/* z = scale * (mean + exp(0.5*clamp(logvar,-30,20)) * noise); moments fp32 [B, hw, ldm] NHWC (mean ch 0..3,
 * logvar ch 4..7), noise fp32 NCHW [B,4,h,w], z fp32 NCHW [B,4,h,w]. */
int udt_posterior_sample(const float* moments, const float* noise, float* z, int32_t B, int32_t hw, int32_t ldm,
                         float scale, void* stream);
/* fp32 NCHW [B,C,HW] -> bf16 NHWC [B,HW,cpad] (channels >= C zero-filled), value * scale */
int udt_nchw_to_nhwc(const float* x, void* y, int32_t B, int32_t C, int64_t HW, int32_t cpad, float scale,
                     void* stream);
/* bf16 or fp32 NHWC [B,HW,ld] (first C channels) -> fp32 NCHW [B,C,HW] */
int udt_nhwc_to_nchw(const void* x, float* y, int32_t B, int32_t C, int64_t HW, int32_t ld, int32_t src_is_f32,
                     void* stream);
/* write fp32 NCHW [B,C,HW] source into channels [c0, c0+C) of a bf16 NHWC buffer [B,HW,cpad] */
int udt_nhwc_set_channels(const float* src, void* dst, int32_t B, int32_t C, int64_t HW, int32_t cpad, int32_t c0,
                          void* stream);
/* out bf16 [n_tok, D] = table[idx[i]] + pe[i % L]  (table fp32 [V, D], pe fp32 [L, D], idx int32) */
int udt_embed_tokens(const int32_t* idx, const float* table, const float* pe, void* out, int32_t n_tok, int32_t L,
                     int32_t D, void* stream);
/* out bf16 [n, dim]: [cos(t f_k) | sin(t f_k)], f_k = exp(-ln(10000) k / (dim/2)); t fp32, any real value (a timestep index or
 * a continuous c_noise such as EDMScaling's 0.25 ln sigma) */
int udt_timestep_embedding(const float* t, void* out, int32_t n, int32_t dim, void* stream);
/* bilinear x1/8 (align_corners False) of fp32 [B,1,H,W] -> fp32 [B,1,H/8,W/8]: mean of the centre 2x2 */
int udt_mask_downsample(const float* mask, float* out, int32_t B, int32_t H, int32_t W, void* stream);
/* per-layer local-loss term: probs fp32 [B*heads, n, L] (n = size*size), mask fp32 [B,1,Hm,Wm],
 * seg_mask fp32 [B, seg_l] -> loss fp32 [B] (+= accumulate): -min_l( max_n(mask_n * blur3x3(mean_h p)) + 1 - seg ) */
int udt_local_loss(const float* probs, const float* mask, const float* seg_mask, const float* gkernel9,
                   float* loss_accum, int32_t B, int32_t heads, int32_t size, int32_t L, int32_t seg_l,
                   int32_t Hm, int32_t Wm, void* stream);
/* the same for n_samples = k * mask_batch maps scored against mask / seg row (sample % mask_batch): the candidates of the noise
 * search (reference sampling.py get_init_noise, loss.py:192-235) as extra batch entries of one launch; loss_accum fp32 [n_samples] */
int udt_local_loss_tiled(const float* probs, const float* mask, const float* seg_mask, const float* gkernel9,
                         float* loss_accum, int32_t n_samples, int32_t mask_batch, int32_t heads, int32_t size, int32_t L,
                         int32_t seg_l, int32_t Hm, int32_t Wm, void* stream);
/* ---- backward (dX only) for attend-and-excite, SURVEY 8f-4 — reference sampling.py:233-252: torch.autograd.grad(local_loss, x)
 * through the UNet; csrc/backward.hip.  Linears / convolutions have no entry of their own: their backward-data is udt_gemm on
 * re-packed weights (W^T; 180-degree rotated taps with the channel roles swapped). ------------------------------------------------- */
/* flash-attention backward, head_dim 64 (reference attention.py:236-248 xformers memory_efficient_attention under autograd):
 * q, k, v: column ranges of one [batch * n, ldq] bf16 matrix (head h at columns h * 64 of each pointer), o / d_o [batch * n, ldo];
 * dq, dk, dv: column ranges of one [batch * n, ldd] bf16 matrix.  lse_ws / dsum_ws: fp32 [batch * heads * n] scratch each (the
 * log-sum-exp of every score row and rowsum(dO o O), written by the first launch, read by the second).  Two launches, no atomics. */
int udt_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, void* dq, void* dk, void* dv,
                 float* lse_ws, float* dsum_ws, int32_t batch, int32_t heads, int32_t n, int32_t ldq, int32_t ldo, int32_t ldd,
                 float scale, void* stream);
/* flash-attention backward for ONE head of 512 dims, self-attention (the AutoencoderKL mid-block attention under autograd; forward:
 * udt_attn512_fwd; csrc/attn512_bwd.hip).  Rows are (b, tok): row strides ld* and batch strides *_bstride in elements, as the forward
 * takes them; q, k, v may be column ranges of one projection, o / d_o [batch * n, >= 512], dq, dk, dv column ranges of one matrix (row
 * stride ldd, batch stride d_bstride).  lse_ws / dsum_ws: fp32 [batch * n] scratch each (log-sum-exp of every score row and
 * rowsum(dO o O): written by the first launch, read by the second).  Two launches, no [n, n] tensor, no atomics, fixed summation
 * order (bit-identical runs).  Any n >= 1: rows past n are masked and never read.  Every pointer 16-byte aligned, every ld and batch
 * stride a multiple of 8 (refused on the host otherwise, with n < 1 and null pointers).  fp32 scores, statistics and accumulators;
 * P and dS rounded to bf16 once for the second products; results rounded to bf16 once. */
int udt_attn512_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, void* dq, void* dk, void* dv,
                    float* lse_ws, float* dsum_ws, int32_t batch, int32_t n, int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                    int32_t lddo, int32_t ldd, int64_t q_bstride, int64_t k_bstride, int64_t v_bstride, int64_t o_bstride,
                    int64_t do_bstride, int64_t d_bstride, float scale, void* stream);
/* the denoiser's output for the OCR term of the training loss (reference loss.py:178-190 takes model_output = D):
 * out[b, c, pix] = c_skip[b] * noised[b, c, pix] + c_out[b] * f[b, pix, c], c < 4; f fp32 NHWC [B, hw, ld] (16-byte aligned, ld % 4
 * == 0), noised / out fp32 NCHW [B, 4, hw], c_skip / c_out fp32 [B] on the device */
int udt_denoised_f32(const float* f, const float* noised, const float* c_skip, const float* c_out, float* out, int32_t B, int32_t hw,
                     int32_t ld, void* stream);
/* seed[b, pix, c] += c_out[b] * g[b, c, pix], c < 4: the OCR term's gradient with respect to D (g fp32 NCHW [B, 4, hw]) added into the
 * reverse pass's bf16 NHWC loss seed [B, hw, cpad] (8-byte aligned, cpad % 4 == 0; channels 4 .. cpad - 1 untouched); fp32
 * arithmetic, one rounding */
int udt_seed_add_bf16(void* seed, const float* g, const float* c_out, int32_t B, int32_t hw, int32_t cpad, void* stream);
/* text cross-attention backward (reference attention.py:140-175 CrossAttention under autograd; context constant): probs fp32
 * [batch * heads, nq, L] as udt_xattn_fwd wrote them, d_probs (optional) the loss gradient with respect to them, d_o (optional) bf16
 * [batch * nq, ldo] the gradient of the attention output -> dq bf16 [batch * nq, lddq] (head h at columns h * 64); L <= 16, and
 * the sigmoid branch for L == 1. */
int udt_xattn_bwd(const void* k, const void* v, const float* probs, const float* d_probs, const void* d_o, void* dq, int32_t batch,
                  int32_t heads, int32_t head_dim, int32_t nq, int32_t L, int32_t ldkv, int32_t ldo, int32_t lddq, float scale,
                  void* stream);
/* gradient of udt_local_loss_tiled's per-layer term with respect to probs, times `weight` (1 / number of contributing layers),
 * ADDED into d_probs fp32 [n_samples * heads, n, L] (zero-initialised by the caller); loss_accum (optional) += the term itself
 * (reference loss.py:192-235 under autograd: arg-min token, arg-max pixel, the 3x3 blur stencil, the head mean) */
int udt_local_loss_bwd(const float* probs, const float* mask, const float* seg_mask, const float* gkernel9, float* d_probs,
                       float* loss_accum, float* scratch /* n_samples * seg_l * 2 floats: the tokens' scores */, int32_t n_samples,
                       int32_t mask_batch, int32_t heads, int32_t size, int32_t L, int32_t seg_l, int32_t Hm, int32_t Wm, float weight,
                       void* stream);
/* the same on h x w maps (n = h * w tokens in row-major order, token = y * w + x; h * w <= 120 * 120; the mask is resized per axis,
 * nearest: src = floor(dst * in / out)).  udt_local_loss_bwd is this with h = w = size. */
int udt_local_loss_bwd_hw(const float* probs, const float* mask, const float* seg_mask, const float* gkernel9, float* d_probs,
                          float* loss_accum, float* scratch /* n_samples * seg_l * 2 floats */, int32_t n_samples, int32_t mask_batch,
                          int32_t heads, int32_t h, int32_t w, int32_t L, int32_t seg_l, int32_t Hm, int32_t Wm, float weight,
                          void* stream);
/* udt_local_loss_tiled's score on h x w maps, cut like udt_local_loss_bwd_hw (the same kernels, no gradient): one workgroup per
 * (context token, sample), then one per sample; loss_accum fp32 [n_samples] += the term.  Bit-equal to udt_local_loss_tiled
 * for h == w. */
int udt_local_loss_tiled_hw(const float* probs, const float* mask, const float* seg_mask, const float* gkernel9, float* loss_accum,
                            float* scratch /* n_samples * seg_l * 2 floats */, int32_t n_samples, int32_t mask_batch, int32_t heads,
                            int32_t h, int32_t w, int32_t L, int32_t seg_l, int32_t Hm, int32_t Wm, void* stream);
/* LayerNorm backward-data (nn.LayerNorm of attention.py:310-339): x, dy bf16 [rows, C] -> dx bf16 (+ add bf16 [rows, C] if given:
 * the gradient that arrives over the residual connection); statistics recomputed from x; C % 8 == 0, C <= 2048 */
int udt_layernorm_bwd(const void* x, const void* dy, const float* gamma, const void* add, void* dx, int64_t rows, int32_t C, float eps,
                      void* stream);
/* GroupNorm (+ SiLU when silu != 0) backward-data (GroupNorm32 / nn.SiLU of openaimodel.py:183-187, attention.py:375): x, dy bf16
 * NHWC [B, HW, C] -> dx (+ add); statistics recomputed from x; (C / groups) even.  partials: fp32 scratch of
 * 2 * B * udt_gn_nchunks(HW, C) * groups * 2 values — with it (and C % 8 == 0, 256 % groups == 0) the gradient runs as three launches
 * at the forward GroupNorm's parallelism (chunk partials of sum x / sum x^2, of sum t / sum t xhat, then the result); NULL: one
 * workgroup per (sample, group) */
int udt_gn_bwd(const void* x, const void* dy, const float* gamma, const float* beta, const void* add, void* dx, float* partials, int32_t B,
               int32_t HW, int32_t C, int32_t groups, float eps, int32_t silu, void* stream);
/* GEGLU (attention.py:44-52) on STORED pre-activations ag bf16 [rows, 2 * inner] = [x | gate]: out = x * gelu(gate) [rows, inner];
 * backward: dag [rows, 2 * inner] from dy [rows, inner] (the inference path's fused GEMM epilogue keeps no pre-activations) */
int udt_geglu_fwd(const void* ag, void* out, int64_t rows, int32_t inner, void* stream);
int udt_geglu_bwd(const void* ag, const void* dy, void* dag, int64_t rows, int32_t inner, void* stream);
/* nearest x2 upsampling backward (openaimodel.py:99-101 under autograd): dy bf16 NHWC [B, 2H, 2W, C] -> dx [B, H, W, C] = 2 x 2 sums */
int udt_sum2x2_bf16(const void* dy, void* dx, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
/* context tokens minus their per-sample mean over the L tokens, as bf16: x fp32 [B, L, D] -> out bf16 [B, L, D].  The softmax over the
 * tokens (attention.py:155-160) and its backward are invariant under that shift of the keys / values; used by the attend-and-excite
 * tape so that the bf16 k|v projection keeps the DIFFERENCES between the (nearly equal) label-embedding tokens */
int udt_center_tokens(const float* x, void* out, int32_t B, int32_t L, int32_t D, void* stream);
/* ---- training step of the text cross-attention (second half; reference diffusion.py:138-172,202-222, loss.py:131-176,
 * 237-286; configs/train/textdesign_sd_2.yaml:4-6: only t_attn / t_norm are trained).  dW = dY^T X runs as udt_gemm on operands
 * transposed by udt_transpose_bf16. ---------------------------------------------------------------------------------------------- */
/* in bf16 [R, ld] (first C columns) -> out bf16 [C, Rp], Rp >= R a multiple of 64 (columns >= R zero) */
int udt_transpose_bf16(const void* in, void* out, int32_t R, int32_t C, int32_t ld, int32_t Rp, void* stream);
/* out[i] (+)= sum_p in[p * n + i], fp32, fixed order */
int udt_reduce_rows_f32(const float* in, float* out, int32_t P, int64_t n, int32_t accumulate, void* stream);
/* row-block partials of the two column reductions below: partials must hold udt_colparts(rows) * C (colsum) / * 2 C (LayerNorm) floats */
int32_t udt_colparts(int64_t rows);
/* out fp32 [C] = column sums of x bf16 [rows, C] (bias gradient of nn.Linear) */
int udt_colsum_bf16(const void* x, float* partials, float* out, int64_t rows, int32_t C, void* stream);
/* LayerNorm parameter gradients: dgamma_dbeta fp32 [2, C] = (sum_r dy * xhat, sum_r dy), x / dy bf16 [rows, C] */
int udt_ln_param_grad(const void* x, const void* dy, float* partials, float* dgamma_dbeta, int64_t rows, int32_t C, float eps, void* stream);
/* weight gradient of nn.Linear (y = x W^T under autograd; attention.py:108-112,193-199 for the trained t_attn projections):
 * dw fp32 [N, K] = dy^T x for dy bf16 [R, N] (row stride ldy), x bf16 [R, K] (row stride ldx); N, K, ldy, ldx multiples of 8, 16-byte
 * aligned operands.  The rows are cut into udt_wgrad_splits(R, N, K) ranges; partials: fp32 scratch of splits * N * K values (may be
 * NULL when splits == 1), summed in range order */
int32_t udt_wgrad_splits(int64_t R, int32_t N, int32_t K);
int udt_wgrad_bf16(const void* dy, const void* x, float* dw, float* partials, int64_t R, int32_t N, int32_t K, int32_t ldy, int32_t ldx,
                   void* stream);
/* text cross-attention, context side (attention.py:140-175 under autograd): dk, dv bf16 [batch * L, lddkv] (head h at columns h * 64)
 * from q bf16 [batch * nq, ldq], v, probs, d_probs (optional), d_o (optional) as udt_xattn_bwd.  The queries are cut into
 * udt_xattn_kv_splits(nq) ranges, one workgroup per (head, sample, range); partials: fp32 scratch of
 * splits * batch * L * heads * 64 * 2 values, summed in ascending range order */
int32_t udt_xattn_kv_splits(int32_t nq);
int udt_xattn_bwd_kv(const void* q, const void* v, const float* probs, const float* d_probs, const void* d_o, void* dk, void* dv,
                     float* partials, int32_t batch, int32_t heads, int32_t head_dim, int32_t nq, int32_t L, int32_t ldq, int32_t ldkv,
                     int32_t ldo, int32_t lddkv, float scale, void* stream);
/* FullLoss.get_local_loss (loss.py:237-286) per layer and its gradient: seg fp32 [B, seg_l, Hs, Ws] character segment maps,
 * seg_mask fp32 [B, seg_l]; d_probs (zero-initialised) += weight * d f / d probs, loss_accum[b] (optional) += f_b */
int udt_local_loss_seg_bwd(const float* probs, const float* seg, const float* seg_mask, const float* gkernel9, float* d_probs,
                           float* loss_accum, float* scratch /* B * seg_l floats: the tokens' terms */, int32_t B, int32_t heads,
                           int32_t size, int32_t L, int32_t seg_l, int32_t Hs, int32_t Ws, float weight, void* stream);
/* the same on h x w maps (row-major tokens, h * w <= 120 * 120; seg resized per axis, nearest); udt_local_loss_seg_bwd is this with
 * h = w = size */
int udt_local_loss_seg_bwd_hw(const float* probs, const float* seg, const float* seg_mask, const float* gkernel9, float* d_probs,
                              float* loss_accum, float* scratch /* B * seg_l floats */, int32_t B, int32_t heads, int32_t h, int32_t w,
                              int32_t L, int32_t seg_l, int32_t Hs, int32_t Ws, float weight, void* stream);
/* eps-prediction loss (loss.py:60-71,131-150; EpsScaling / EpsWeighting): loss fp32 [B] = mean(sigma^-2 (eps * -sigma + noised -
 * target)^2) and d_eps bf16 NHWC [B, hw, cpad] = d mean_b(loss_b) / d eps; eps fp32 NHWC [B, hw, ld_eps], noised / target fp32 NCHW */
int udt_diff_loss_grad(const float* eps, const float* noised, const float* target, const float* sigma, void* d_eps, float* loss, int32_t B,
                       int32_t hw, int32_t ld_eps, int32_t cpad, void* stream);
/* the same loss under any preconditioning / weighting, per-sample fp32 coefficients c_skip[B], c_out[B], w[B] (host values of
 * denoiser.scaling / denoiser.w): out = c_skip_b*noised + c_out_b*F ; loss fp32 [B] = mean(w_b (out - target)^2) and
 * d_f bf16 NHWC [B, hw, cpad] = d mean_b(loss_b) / d F = 2 w_b c_out_b (out - target) / (B * 4 hw); layout and reduction as
 * udt_diff_loss_grad (which stays the eps path's launch) */
int udt_precond_loss_grad(const float* f, const float* noised, const float* target, const float* c_skip, const float* c_out,
                          const float* w, void* d_f, float* loss, int32_t B, int32_t hw, int32_t ld_f, int32_t cpad, void* stream);
/* torch.optim.AdamW step on fp32 parameters (diffusion.py:49-51,219): g is scaled by grad_scale first (gradient accumulation / world) */
int udt_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, float grad_scale, void* stream);
/* ---- gradient accumulation and the fused optimiser step (configs/train.yaml:21 accumulate_grad_batches; diffusion.py:75-78,178-195 with
 * sgm/modules/ema.py).  The trained tensors' gradients live in ONE flat fp32 bucket; the reverse pass adds into it, the collectives
 * run on it in place, one launch consumes it. ------------------------------------------------------------------------------------- */
/* udt_wgrad_bf16 with accumulate: accumulate != 0 gives dw += dy^T x, the fixed-order sum formed first and added once (what
 * torch.autograd does to .grad on the second backward() of a window); accumulate == 0 is udt_wgrad_bf16, bit for bit.  With one row
 * range (udt_wgrad_splits == 1 after rounding) the add happens in the kernel's epilogue: no temporary of dw's size */
int udt_wgrad_bf16_acc(const void* dy, const void* x, float* dw, float* partials, int64_t R, int32_t N, int32_t K, int32_t ldy, int32_t ldx,
                       int32_t accumulate, void* stream);
/* udt_colsum_bf16 with accumulate: out (+)= column sums (bias gradient, accumulated as above) */
int udt_colsum_bf16_acc(const void* x, float* partials, float* out, int64_t rows, int32_t C, int32_t accumulate, void* stream);
/* udt_ln_param_grad with accumulate: dgamma_dbeta [2, C] (+)= (sum_r dy * xhat, sum_r dy) (t_norm's gradients, accumulated as above) */
int udt_ln_param_grad_acc(const void* x, const void* dy, float* partials, float* dgamma_dbeta, int64_t rows, int32_t C, float eps,
                          int32_t accumulate, void* stream);
/* one trained tensor of the bucket: its fp32 parameter p and EMA shadow (n values each; 16-byte aligned pointers take the 16-byte
 * path, others go element by element), and where its n gradients / moments start in the flat buffers: offset, a multiple of 4 floats */
typedef struct udt_bucket_segment {
  float* p;
  float* shadow;              /* may be NULL when the mode has no EMA bit */
  int64_t offset;
  int64_t n;
} udt_bucket_segment;
/* elements per chunk of the chunk map below */
#define UDT_BUCKET_CHUNK 4096
#define UDT_BUCKET_ADAMW 1
#define UDT_BUCKET_EMA 2
/* The optimiser step over all segments in one launch.  segments: DEVICE table; chunk_map: DEVICE int32 [n_chunks, 2] = (segment,
 * chunk index inside it), every segment cut into ceil(n / UDT_BUCKET_CHUNK) chunks, in any order, each chunk once.  g / m / v: the
 * flat fp32 gradient bucket and AdamW moments (16-byte aligned; NULL allowed without the AdamW bit).  mode:
 *   UDT_BUCKET_ADAMW   p, m, v <- torch.optim.AdamW.step with gradient g * grad_scale: the arithmetic of udt_adamw_f32 (diffusion.py:49-51,
 *                      219; grad_scale = 1 / (accumulate_grad_batches * world))
 *   UDT_BUCKET_EMA     shadow -= one_minus_decay * (shadow - p): LitEma.forward (ema.py:40-52; the host computes the decay, ema.py:36-38)
 *   both               AdamW first, then the EMA on the updated p: optimizer.step() then on_train_batch_end (diffusion.py:178-180)
 * Elements between the segments (padding) are neither read nor written; g is only read. */
int udt_bucket_update_f32(const udt_bucket_segment* segments, const int32_t* chunk_map, int32_t n_chunks, float* g, float* m, float* v,
                          int32_t mode, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, float grad_scale,
                          float one_minus_decay, void* stream);
/* p <-> shadow over the same table and map: LitEma.store + copy_to entering ema_scope, restore leaving it (ema.py:56-86,
 * diffusion.py:182-195); its own inverse */
int udt_bucket_swap_f32(const udt_bucket_segment* segments, const int32_t* chunk_map, int32_t n_chunks, void* stream);
/* x fp32 += a * y fp32: the attend-and-excite update x <- x - alpha * grad (sampling.py:247) */
int udt_axpy_f32(float* x, const float* y, float a, int64_t n, void* stream);
/* The attend-and-excite update with every row of a batch on its own B = 1 loop (sampling.py:240-252), one launch per iteration.
 * x, grad fp32 [B, n] contiguous; loss fp32 [B] (the loss of the evaluation that produced grad); state_in / state_out int32 [2, B]:
 * row 0 the active flags, row 1 the per-row update counts, two DISTINCT buffers the caller swaps between iterations; n_active: one int32.
 * For row b with a = (state_in[b] != 0):
 *   a:      x[b, :] <- fma(-alpha, grad[b, :], x[b, :])   (bit-identical to udt_axpy_f32(x_b, grad_b, -alpha, n))
 *   not a:  x[b, :] is not written, and nothing written anywhere depends on grad[b, :] or loss[b]
 *   it = state_in[B + b] + a;  state_out[B + b] = it
 *   state_out[b] = a && iter_enabled && !(loss[b] <= thres) && !(it > max_iter)      (:249; a NaN loss runs to the cap)
 *   *n_active = sum_b state_out[b]
 * UDT_ERR_BAD_ARG: a null pointer, B < 1, n < 1, max_iter < 0, state_in and state_out overlapping; UDT_ERR_BAD_SHAPE: n % 4 != 0,
 * x / grad not 16-byte aligned, B > 1024.  Nothing is launched in either case. */
int udt_aae_row_update_f32(float* x, const float* grad, const float* loss, const int32_t* state_in, int32_t* state_out, int32_t* n_active,
                           int32_t B, int64_t n, float alpha, float thres, int32_t iter_enabled, int32_t max_iter, void* stream);
/* Crop + antialiased bicubic resize + normalise of N boxes in one launch (test.py:81 + the OCR predictor's transform,
 * sgm/modules/predictors/model.py:24-29): for box n = (image index, top, bottom, left, right), half-open as the slice
 * img[index, :, top:bottom, left:right],
 *   out[n] = mul * F.interpolate(crop[None], size=(out_h, out_w), mode="bicubic", antialias=True, align_corners=False) + add
 * ((mul, add) = (2, -1) is Normalize(0.5, 0.5)).  img fp32 [B, C, H, W], boxes DEVICE int32 [N, 5], out fp32 [N, C, out_h, out_w], all
 * contiguous.  Separable; along an axis of n_in input and n_out output samples, output i uses scale = n_in / n_out,
 * support = 2 scale and inv = 1 / scale when scale >= 1 (else 2 and 1), centre = scale (i + 0.5), the taps
 * lo = max(0, int(centre - support + 0.5)) <= j < hi = min(n_in, int(centre + support + 0.5)) and the weights
 * k((j - centre + 0.5) inv) divided by their sum, k the Keys cubic with a = -0.5.  Taps clamp at the BOX: no pixel outside it reaches out.
 * Tap positions and weights are evaluated in fp64 and rounded to fp32 once; products and sums are fp32.
 * The kernel clamps each box to the image (and to at least one pixel), so it reads no address outside img whatever boxes holds; callers
 * validate boxes on the host.  No workspace, no host read: the grid depends on (N, C, out_h, out_w) only, and box sizes are unbounded.
 * UDT_ERR_BAD_ARG: a null pointer; UDT_ERR_BAD_SHAPE: a dimension < 1, C or N > 65535.  Nothing is launched in either case. */
int udt_crop_resize_aa_f32(const float* img, const int32_t* boxes, float* out, int B, int C, int H, int W, int N, int out_h, int out_w,
                           float mul, float add, void* stream);
/* The adjoint of udt_crop_resize_aa_f32 (its backward with respect to img; `add` has no part in it):
 *   d_img[b, c, y, x] = mul * sum_oy sum_ox wy(oy, y - top) wx(ox, x - left) d_out[n, c, oy, ox]
 * for the box n of image b and (y, x) inside it, with the forward's tap rule and the forward's weights (the same device functions:
 * tap positions and weights evaluated in fp64, each weight rounded to fp32 once).  d_out fp32 [N, C, out_h, out_w], boxes DEVICE int32
 * [N, 5] as in the forward, d_img fp32 [B, C, H, W], all contiguous.
 * EVERY element of d_img is written exactly once: zero outside the boxes and for images without a box — the caller clears nothing.
 * Precondition: every image index appears in at most one box (one box per image, loss.py:184; the Python wrapper validates it on the
 * host).  Given a table that breaks it, the FIRST box of an image is used and the others are ignored: no address outside d_img is
 * touched.  Boxes are clamped to the image exactly as the forward clamps them.
 * Gather form, no atomics: the outputs that read an input sample are one contiguous range per axis; per input pixel, for every output
 * column ox in ascending order, inner = sum over oy ascending of wy * d_out (fp32 FMA), acc += wx * inner (fp32 FMA); the result is
 * mul * acc, rounded once more.  Bit-identical from run to run.  The grid depends on (B, C, H, W) only; no workspace, no host read.
 * UDT_ERR_BAD_ARG: a null pointer; UDT_ERR_BAD_SHAPE: a dimension < 1, H, B * C or N > 65535.  Nothing is launched in either case. */
int udt_crop_resize_aa_bwd_f32(const float* d_out, const int32_t* boxes, float* d_img, int B, int C, int H, int W, int N, int out_h,
                               int out_w, float mul, void* stream);
/* Bilinear resize of fp32 planes in one launch (the character maps at image size: demo.py:109 cv2.resize(seg_map, (W, H)), which is
 * F.interpolate(mode="bilinear", align_corners=False)): in fp32 [planes, h, w], out fp32 [planes, H, W], contiguous.  Half-pixel
 * centres with edge clamp; down-scaling is plain bilinear, no antialiasing.  Along an axis of n_in input and n_out output samples,
 * output i reads the source coordinate max(0, (2 i + 1) n_in - n_out) / (2 n_out), held as that integer fraction: taps
 * i0 = min(floor, n_in - 1) and i1 = min(i0 + 1, n_in - 1) are exact, the weights w1 = frac and w0 = 1 - frac are each the exact
 * rational rounded to fp32 once.
 * ROUNDING: out = fma(wy1, bot, wy0 * top) with top = fma(wx1, in[i0y][i1x], wx0 * in[i0y][i0x]) and bot likewise on row i1y, fp32.
 * Any H, W >= 1.  Bit-identical from run to run.
 * UDT_ERR_BAD_ARG: a null pointer; UDT_ERR_BAD_SHAPE: a dimension < 1, planes * H * W >= 2^40.  Nothing is launched in either case. */
int udt_resize_bilinear_f32(const float* in, float* out, int64_t planes, int32_t h, int32_t w, int32_t H, int32_t W, void* stream);
/* Backward of udt_mattn_fwd: same operands and layout (q, k, v bf16 row views with their ld and batch strides, optional fp32 additive
 * mask [nq, ldmask], optional uint8 kpm [batch, lk]) plus
 *   d_o : bf16 rows (b, i) at d_o + b*do_bstride + i*lddo + h*head_dim, the cotangent of o
 *   dq  : bf16 rows (b, i) at dq + b*dq_bstride + i*lddq + h*head_dim, or NULL (not wanted: the decoder's queries are constants)
 *   dk, dv : bf16 rows (b, l) at dk + b*dk_bstride + l*lddk + h*head_dim (dv likewise)
 * Only the heads*head_dim columns of a row are written; ld gaps are neither read nor written.
 * Domain: that of the forward (head_dim % 8 == 0, head_dim <= 64, lk <= 256, lk*head_dim <= 8192, batch <= 65535) and
 * nq*head_dim <= 8192; every ld >= heads*head_dim.
 * The forward stores no log-sum-exp: scores, softmax P, dP = dO V^T, delta_i = sum_l P_il dP_il and dS = P (dP - delta) are recomputed
 * in fp32 from the bf16 operands, then dv = P^T dO, dk = scale dS^T Q, dq = scale dS K with fp32 accumulation (query rows / keys in
 * ascending order).  ROUNDING: the only values rounded below fp32 are the stored dq, dk, dv (bf16, round to nearest even, once each);
 * P and dS are never rounded to bf16.  A query whose keys are all masked has P = 0: it contributes nothing to dk / dv and gets dq = 0,
 * matching the forward's zeros.  One workgroup per (head, sample), no atomics: bit-identical from run to run.
 * UDT_ERR_BAD_ARG: a null pointer other than dq / mask / kpm; UDT_ERR_BAD_SHAPE: outside the domain.  Nothing is launched in either case. */
int udt_mattn_bwd(const void* q, const void* k, const void* v, const void* d_o, void* dq, void* dk, void* dv, const float* mask,
                  const uint8_t* kpm, int32_t batch, int32_t heads, int32_t head_dim, int32_t nq, int32_t lk,
                  int32_t ldq, int32_t ldk, int32_t ldv, int32_t lddo, int32_t lddq, int32_t lddk, int32_t lddv, int32_t ldmask,
                  int64_t q_bstride, int64_t k_bstride, int64_t v_bstride, int64_t do_bstride, int64_t dq_bstride, int64_t dk_bstride,
                  int64_t dv_bstride, float scale, void* stream);
/* Exact-erf GELU (nn.GELU / F.gelu default) on STORED pre-activations a fp32 [rows, C] contiguous, C % 8 == 0 (the inference path's
 * GEMM epilogue keeps none; fp32 = the GEMM's accumulators under UDT_GEMM_OUT_F32, so the tape-mode forward rounds where the fused
 * epilogue rounds): out bf16 [rows, C] = gelu(a); backward: dy bf16 [rows, C] -> da bf16 [rows, C] = dy * (Phi(a) + a phi(a)).
 * fp32 arithmetic (erf by Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7); ROUNDING: the stored out / da only (bf16, once).
 * da may alias dy.
 * UDT_ERR_BAD_ARG: a null pointer; UDT_ERR_BAD_SHAPE: rows < 1, C < 1, C % 8 != 0.  Nothing is launched in either case. */
int udt_gelu_fwd(const void* a, void* out, int64_t rows, int32_t C, void* stream);
int udt_gelu_bwd(const void* a, const void* dy, void* da, int64_t rows, int32_t C, void* stream);
/* The OCR loss of N rows and its seed in one launch (ParseqPredictor.calc_loss, sgm/modules/predictors/model.py:40-58):
 *   logits  fp32 [N, L, ld], the first n_cls columns of a row are the classes (n_cls <= 256, L <= 256)
 *   targets int32 [N, T], n_chars int32 [N] with 1 <= n_chars[b] <= min(L, T) (validated by the caller on the host; the kernel clamps
 *           both n_chars and the target ids into range, so it reads no address outside a row whatever they hold)
 *   weight  fp32 [N] or NULL (= 1): the upstream cotangent of each row's loss
 *   loss[b] = min(1, m_b),  m_b = mean_{t < n} CE(logits[b, t], targets[b, t])          (the characters only, EOS excluded)
 *   d_logits fp32 [N, L, ld_d]: for rows with m_b <= 1 (torch's clamp rule), d_logits[b, t, c] = weight[b] (softmax_c - onehot_c) / n
 *           for t < n; ZERO everywhere else — every class of a clamped row and every t >= n.  All n_cls columns of all L positions
 *           are written (no memset needed); columns n_cls .. ld_d - 1 are not touched.
 * A NaN cross entropy (a NaN or +inf logit) gives loss[b] = NaN and a zero gradient row (NaN <= 1 is false).
 * ROUNDING: log-sum-exp, softmax, the mean (characters added in ascending order) are evaluated in fp64 from the fp32 logits; the only
 * rounding is the conversion of loss[b] and of each d_logits element to fp32.  One workgroup per row, no atomics.
 * UDT_ERR_BAD_ARG: a null pointer other than weight; UDT_ERR_BAD_SHAPE: N, L, T or n_cls < 1, L or n_cls > 256, ld or ld_d < n_cls.
 * Nothing is launched in either case. */
int udt_ocr_ce_f32(const float* logits, const int32_t* targets, const int32_t* n_chars, const float* weight, float* loss,
                   float* d_logits, int32_t N, int32_t L, int32_t n_cls, int32_t ld, int32_t T, int32_t ld_d, void* stream);
/* ---- LPIPS (AlexNet) in fp32: the second measurement of the reference's test.py (:122-124, metrics.py:12-30) ------------------------
 * LAYOUT: every activation of this family is fp32, channels-last: pixel (n, y, x) of a [N, H, W, C] map starts at element
 * ((n H + y) W + x) ld of its buffer, ld >= C; only the first C elements of a pixel are read or written.  Results are deterministic:
 * no floating-point atomics, every sum in one fixed order, so they are the same bits from run to run and for every ld.
 *
 * udt_conv2d_f32: out = conv(x, w) + bias, ReLU if relu != 0 — square kernel ksize, the same stride and zero padding in both
 * directions — as an implicit GEMM on v_mfma_f32_32x32x2_f32: rows = the N Ho Wo output pixels, columns = Cout,
 * K = ksize ksize Cin, Ho = (H + 2 pad - ksize) / stride + 1 (Wo alike).
 *   x    fp32 [N, H, W, Cin] (ld_x), out fp32 [N, Ho, Wo, Cout] (ld_out); they must not overlap
 *   w    fp32 [Cout][Kp], packed once per module (packing.pack_conv_f32): column k = (ky ksize + kx) Cin + c holds the checkpoint's
 *        weight[o, c, ky, kx]; Kp = K rounded up to a multiple of 16, columns K .. Kp - 1 ZERO.  Rows are not padded.
 *   bias fp32 [Cout] or NULL
 * Zero padding is produced by the gather: a tap outside the image, and a column k >= K, is a zero that is never loaded.
 * ROUNDING: out = fp32(acc + bias); the k axis is cut into blocks of 128, each block is one fp32 fused-multiply-add chain in ascending
 * k starting from 0 (what the MFMA computes: one rounding per term, no wider accumulation), and the blocks' sums are added in ascending
 * order (blocked summation: the error grows with the block length, not with K); for any K,
 * |out - exact| <= (K + 2) 2^-24 (sum |w||x| + |bias|) to first order.
 * UDT_ERR_BAD_ARG: x, w or out NULL.  UDT_ERR_BAD_SHAPE: a count < 1, Cin > 2^20, ld_x < Cin, ld_out < Cout, ksize outside 1 .. 11,
 * stride outside 1 .. 4, pad outside 0 .. ksize - 1, an image with no output pixel, more than 2^31 - 1 row tiles of 128 pixels,
 * more than 65535 column tiles of 64 channels (Cout > 4194240).  Nothing is launched or written then. */
int udt_conv2d_f32(const float* x, const float* w, const float* bias, float* out, int32_t N, int32_t H, int32_t W, int32_t Cin,
                   int32_t ld_x, int32_t Cout, int32_t ld_out, int32_t ksize, int32_t stride, int32_t pad, int32_t relu, void* stream);
/* nn.MaxPool2d(3, stride 2) without padding, floor mode, same layout: x [N, H, W, C] (ld_x) -> out [N, (H - 3) / 2 + 1,
 * (W - 3) / 2 + 1, C] (ld_out).  The maximum starts from the window's first element (all-negative maps are right); no rounding.
 * A NaN in a window makes that output NaN, as nn.MaxPool2d does; of +0 and -0 the first in row-major window order is kept.
 * UDT_ERR_BAD_ARG: x or out NULL.  UDT_ERR_BAD_SHAPE: H or W < 3, a count < 1, ld < C, more than 2^38 output elements.
 * Nothing is launched then. */
int udt_maxpool3s2_f32(const float* x, float* out, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ld_x, int32_t ld_out,
                       void* stream);
/* The network input of N (fake, real) pairs in one launch: samples fp32 [N, 3, H, W] in [0, 1] (the generated frames), images fp32
 * [N, 3, H, W] in [-1, 1] (batch["image"]), both dense NCHW -> out fp32 [2 N, H, W, 3] (ld_out), frames 0 .. N - 1 from samples,
 * N .. 2 N - 1 from images.  Per element, every fp32 operation rounded on its own, in this order:
 *   v = s 255 (samples) or ((x + 1) 0.5) 255 (images): the 8-bit PNG values test.py:94,102,110-113 writes;
 *   v clamped to [0, 255]; quantise != 0: v = trunc(v) (the PNG's uint8; 0 keeps the continuous value);
 *   t = fp32(v / 127.5 - 1 evaluated in fp64) (lpips.im2tensor divides a numpy array by a Python float);
 *   out = (t - shift[c]) / scale[c] (the scaling layer; shift, scale fp32 [3]).
 * A NaN input gives v = 0 (the clamp drops it).
 * UDT_ERR_BAD_ARG: a NULL pointer; UDT_ERR_BAD_SHAPE: a count < 1, ld_out < 3, more than 2^38 pixels (2 N H W).  Nothing is
 * launched then. */
int udt_lpips_input_f32(const float* samples, const float* images, const float* shift, const float* scale, float* out, int32_t N,
                        int32_t H, int32_t W, int32_t ld_out, int32_t quantise, void* stream);
/* One tap of the LPIPS distance: feats fp32 [2 N, P, C] (ld), the features of the stacked frames (pair n = frames n and N + n),
 * w fp32 [C] (the tap's 1x1 "lin" weights) -> out fp32 [N]: out[n] = (accumulate ? out[n] : 0) + mean over the P pixels of
 * sum_c w_c (u0_c - u1_c)^2, u = f / (sqrt(sum_c f_c^2) + 1e-10).  A pixel whose features are all zero gives u = 0.
 * ROUNDING: all fp32, correctly rounded sqrt and divisions; the channel sums over the 64 lanes of a wave, the pixel sum over 16
 * consecutive pixels per wave, 4 waves per workgroup, one partial per 64 pixels in `scratch`, the partials added per pair in a
 * fixed order by a second launch.  scratch: the size the query below states for (N, P), written before it is read.
 * UDT_ERR_BAD_ARG: a NULL pointer; UDT_ERR_BAD_SHAPE: N outside 1 .. 65535, P or C < 1, P above 2^31 - 1 blocks of 64 pixels, ld < C; UDT_ERR_WORKSPACE: scratch_bytes
 * below the stated size.  Nothing is launched then. */
size_t udt_lpips_layer_scratch_bytes(int32_t N, int64_t P);
int udt_lpips_layer_f32(const float* feats, const float* w, float* out, int32_t N, int64_t P, int32_t C, int32_t ld, int32_t accumulate,
                        void* scratch, size_t scratch_bytes, void* stream);
/* ---- FID (InceptionV3 pool features) in fp32 + fp64 moments: the third measurement of the reference's test.py (:119-121,
 * metrics.py:5-10) — csrc/fid.hip.  Same activation family and LAYOUT as LPIPS above: fp32 channels-last [N, H, W, C] with a pixel
 * stride ld >= C.  A channel slice of a wider map is (pointer + first channel, ld of the wide map): Inception's concatenations are
 * written and read that way, no copy.  Deterministic: no floating-point atomics, every sum in one fixed order, the same bits for every
 * ld and every run.
 *
 * udt_conv2d_rect_f32: udt_conv2d_f32 with a kh x kw kernel and a zero padding per axis: k = (ky kw + kx) Cin + c,
 * K = kh kw Cin, Ho = (H + 2 pad_h - kh) / stride + 1, Wo = (W + 2 pad_w - kw) / stride + 1; w fp32 [Cout][Kp] from
 * packing.pack_conv_f32 of a [Cout, Cin, kh, kw] weight.  It is the same kernel (csrc/conv_f32.h): operands, ROUNDING (blocks of 128 k)
 * and bound are those stated for udt_conv2d_f32, and kh == kw, pad_h == pad_w gives udt_conv2d_f32's bits.
 * UDT_ERR_BAD_ARG: x, w or out NULL.  UDT_ERR_BAD_SHAPE: a count < 1, Cin > 2^20, ld_x < Cin, ld_out < Cout, kh or kw outside 1 .. 11,
 * stride outside 1 .. 4, pad_h outside 0 .. kh - 1, pad_w outside 0 .. kw - 1, an image with no output pixel, the grid limits of
 * udt_conv2d_f32.  Nothing is launched or written then. */
int udt_conv2d_rect_f32(const float* x, const float* w, const float* bias, float* out, int32_t N, int32_t H, int32_t W, int32_t Cin,
                        int32_t ld_x, int32_t Cout, int32_t ld_out, int32_t kh, int32_t kw, int32_t stride, int32_t pad_h, int32_t pad_w,
                        int32_t relu, void* stream);
/* 3 x 3 pool, stride 1 or 2, padding 0 or 1, floor mode: x [N, H, W, C] (ld_x) -> out [N, (H + 2 pad - 3) / stride + 1,
 * (W + 2 pad - 3) / stride + 1, C] (ld_out).  Only the taps inside the image take part, in row-major window order.
 *   average == 0: the maximum (nn.MaxPool2d: padding never wins); a NaN in a window makes that output NaN; of +0 and -0 the first is
 *     kept; no rounding.  stride 2, pad 0 gives udt_maxpool3s2_f32's bits.
 *   average != 0: F.avg_pool2d(count_include_pad=False): the fp32 sum of the taps inside the image, added one by one starting from 0,
 *     divided by their number (1 .. 9) — at most eight rounded additions and one correctly rounded division.
 * UDT_ERR_BAD_ARG: x or out NULL.  UDT_ERR_BAD_SHAPE: a count < 1, ld < C, stride outside 1 .. 2, pad outside 0 .. 1, H + 2 pad < 3 or
 * W + 2 pad < 3, more than 2^38 output elements.  Nothing is launched then. */
int udt_pool3_f32(const float* x, float* out, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ld_x, int32_t ld_out, int32_t stride,
                  int32_t pad, int32_t average, void* stream);
/* The Inception input of N (fake, real) pairs in one launch: samples fp32 [N, 3, H, W] in [0, 1], images fp32 [N, 3, H, W] in
 * [-1, 1], dense NCHW -> out fp32 [2 N, size, size, 3] (ld_out), frames 0 .. N - 1 from samples, N .. 2 N - 1 from images
 * (size = 299 for FID).  Per source element, every fp32 operation rounded on its own:
 *   v = s 255 (samples) or ((x + 1) 0.5) 255 (images), clamped to [0, 255]; quantise != 0: v = trunc(v) (the saved PNG's uint8);
 *   p = v / 255 (ToTensor), correctly rounded.
 * Then F.interpolate(size, mode="bilinear", align_corners=False) of p with udt_resize_bilinear_f32's coordinate rule and ROUNDING
 * (exact taps, weights rounded once, top = fma(wx1, p[i0y][i1x], wx0 p[i0y][i0x]), bot alike, r = fma(wy1, bot, wy0 top)), and
 * out = 2 r - 1 (2 r exact, one rounding).  A NaN input gives v = 0.  Any H, W >= 1.
 * UDT_ERR_BAD_ARG: a NULL pointer; UDT_ERR_BAD_SHAPE: a count < 1, size > 4096, ld_out < 3, more than 2^38 output pixels.  Nothing is
 * launched then. */
int udt_fid_input_f32(const float* samples, const float* images, float* out, int32_t N, int32_t H, int32_t W, int32_t size,
                      int32_t ld_out, int32_t quantise, void* stream);
/* Global average pool: x fp32 [N, P, C] (pixel stride ld_x) -> out fp32 [N, C] (row stride ld_out): the P pixels added in ascending
 * order starting from 0 (P rounded additions), then one correctly rounded division by P.
 * UDT_ERR_BAD_ARG: a NULL pointer; UDT_ERR_BAD_SHAPE: a count < 1, P > 2^24, ld < C.  Nothing is launched then. */
int udt_mean_pixels_f32(const float* x, float* out, int32_t N, int64_t P, int32_t C, int32_t ld_x, int32_t ld_out, void* stream);
/* Streaming first and second moments: x fp32 [n, D] (row stride ld) -> sum fp64 [D] += sum_r x_r, outer fp64 [D, D] (dense) += X^T X.
 * Every fp32 value is converted exactly to fp64; the contraction over the rows runs on v_mfma_f64_16x16x4_f64 (fp64 fused
 * multiply-adds, rows in ascending order, four per instruction), starting from 0, and the launch's total is added to the stored value
 * once: |outer_ij - exact| <= n 2^-53 sum_r |x_ri x_rj| + 2^-53 |stored result| to first order; integer data below 2^53 is exact.
 * The FULL matrix is computed (no mirrored triangle); each output element belongs to one wave; sum is added by the waves of the first
 * tile column.  sum and outer must not overlap x; any D >= 1, n >= 1.
 * UDT_ERR_BAD_ARG: a NULL pointer; UDT_ERR_BAD_SHAPE: n < 1, D < 1, D > 2^18, ld < D.  Nothing is launched or written then. */
int udt_moments_accum_f64(const float* x, double* sum, double* outer, int32_t n, int32_t D, int32_t ld, void* stream);
/* x bf16 += y bf16 (n elements, n % 8 == 0) ; utility for residuals outside GEMM epilogues */
int udt_add_bf16(void* x, const void* y, int64_t n, void* stream);

/* Tuning knobs (no reference counterpart); every setting computes the same results: "gemm_impl" (4 or 8: kernel
 * generation), "conv3p" (0/1: patch-staged 3x3 convolution), "rows_epi" (0/1: row-coalesced epilogues), "n_block"
 * (-1 automatic, 0 off, n: N-tiles per block of the GEMM tile order).  Measurement builds of the library
 * (-DUDT_MEASURE) additionally accept the cost-attribution keys "no_xchg", "no_epi", "no_store", "no_res", "no_bias",
 * "no_fast", which switch parts of the finishing code off and give WRONG results; the product library rejects them. */
int udt_debug_set(const char* key, int32_t value);

/* out[r][c] = bf16(x[r][c] + bias[c]); x/out bf16 [rows, C] (may alias), bias fp32 [C], C % 8 == 0.
 * Used where a projection's GEMM input is identically zero (cross-attention over an all-zero context — the
 * unconditional half under force_uc_zero_embeddings, reference sgm/modules/attention.py:150-174 with k = v = 0 — so
 * to_out(...) + x reduces to bias + x). */
int udt_bias_add_bf16(const void* x, const float* bias, void* out, int64_t rows, int32_t C, void* stream);

/* ---- library services -------------------------------------------------------------------------- */
/* ---- packed-weight handles: the only memory the library allocates on a caller's behalf (SURVEY §8b "Ownership") ----------
 * Checkpoint layouts in (the reference's): nn.Linear weight [N, K] fp32 (+ bias [N]), nn.Conv2d weight [N, Cin, kh, kw] fp32,
 * DEVICE pointers; out: an immutable handle whose buffers have the layouts udt_gemm consumes.
 *   udt_pack_linear: bf16 [Npad][Kpad] (K padded to 64, N to 4, zeros) or, dtype = UDT_DTYPE_FP8_E4M3, e4m3 bytes [Npad][Kpad128]
 *     + colscale[n] = max_k |w[n, k]| / 448; geglu != 0: rows permuted into [32 value | 32 gate] blocks for UDT_GEMM_GEGLU
 *     (GEGLU.proj, reference attention.py:83-99), bias permuted the same way.
 *   udt_pack_conv: bf16 [Npad][kh*kw*Cpad], k = (ky*kw + kx)*Cpad + c; `segments` (may be NULL) = channel counts of the
 *     concatenated sources (decoder skip concat), each padded to a multiple of 64 separately; N padded to n_pad_to.
 * udt_packed_dim(h, which): 0 N, 1 Npad, 2 K, 3 Kpad (= the `ldw` / `K` to put into udt_gemm_desc), 4 dtype.
 * The LayerNorm fold of udt_ln_gemm_fwd (W' = gamma * W, colsum, c) is done by the Python front end (packing.pack_ln_linear). */
typedef struct udt_packed udt_packed;
int udt_pack_linear(const float* w, const float* bias, int32_t N, int32_t K, int32_t dtype, int32_t geglu,
                    udt_packed** out, void* stream);
int udt_pack_conv(const float* w, const float* bias, int32_t N, int32_t Cin, int32_t kh, int32_t kw, const int32_t* segments,
                  int32_t n_segments, int32_t n_pad_to, udt_packed** out, void* stream);
const void* udt_packed_weight(const udt_packed* h);
const float* udt_packed_bias(const udt_packed* h);
const float* udt_packed_colscale(const udt_packed* h);
int32_t udt_packed_dim(const udt_packed* h, int32_t which);
int udt_free_packed(udt_packed* h);

/* ---- the names SURVEY §8b lists for the generic entry points (same functions) -------------------------------------------------
 * udt_gemm_fwd = udt_gemm; udt_conv1x1_fwd = udt_gemm restricted to UDT_GEMM_CONV with ksize 1 (nn.Conv2d 1x1: proj_in / proj_out of
 * the VAE attention block, skip_connection); udt_workspace_bytes = udt_gemm_workspace_bytes; udt_sampler_step = udt_cfg_euler_step
 * (VanillaCFG + DiscreteDenoiser scaling + the Euler update, reference sampling.py:68-80, guiders.py:17-22, denoiser.py:23-31). */
int udt_gemm_fwd(const udt_gemm_desc* d, void* workspace, size_t workspace_bytes, void* stream);
int udt_conv1x1_fwd(const udt_gemm_desc* d, void* workspace, size_t workspace_bytes, void* stream);
size_t udt_workspace_bytes(const udt_gemm_desc* d);
int udt_sampler_step(float* x, const float* eps, float* denoised_out, int32_t B, int32_t hw, int32_t ld_eps,
                     float c_out, float sigma, float sigma_next, float cfg_scale, void* stream);

const char* udt_version(void);
const char* udt_status_string(int status);
int udt_last_hip_error(void);            /* hipError_t of the last failing HIP call (0 if none)     */
int udt_device_arch_ok(void);            /* 1 if device 0 reports gfx950                           */

/* Per-op-class HIP-event timing on the launch stream (used by bench.py's roofline object).
 * classes: 0 conv3x3, 1 gemm (linear/1x1), 2 attn, 3 xattn, 4 norm, 5 elementwise.               */
#define UDT_PROF_NCLASS 6
int udt_prof_enable(uint32_t class_mask);
int udt_prof_reset(void);
/* per-launch trace (class, ms, shape tag) of the profiled classes; dump writes a CSV                  */
int udt_prof_trace(int32_t on);
int udt_prof_dump(const char* path);
/* synchronises the recorded events and returns total ms / launch count for a class               */
int udt_prof_get(int32_t op_class, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* UDT_KERNELS_H */
