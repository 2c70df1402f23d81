/*
 * liboess -- C-ABI of the MI355X-native OpenESS hot path (gfx950, hand-written HIP).
 *
 * The reference (ldkong1205/OpenESS) is pure Python: it has no FFI.  Its "plugin surface" is a
 * set of Python call contracts; each entry point below is what a ctypes binding
 * inside the cited reference function would call instead of the NumPy / PyTorch-CPU body.
 * INTEGRATION.md shows the stub for each.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host.
 *   - stream-ordered: the call only ENQUEUES work on `stream` (a hipStream_t passed as void*);
 *     the caller synchronises.  No hidden allocation: outputs and workspaces are caller-owned and
 *     must stay alive until the stream has passed the call; sizes come from *_workspace_bytes().
 *   - returns 0 on success, a negative OESS_E* code otherwise; no exceptions cross the boundary.
 *   - no global mutable state; thread-safe for distinct streams/buffers.
 */
#ifndef OESS_H
#define OESS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OESS_OK 0
#define OESS_EINVAL (-22)   /* bad argument (shape, null pointer, unsupported size)            */
#define OESS_ENOMEM (-12)   /* workspace too small                                             */
#define OESS_ELAUNCH (-5)   /* hipGetLastError() != hipSuccess after a launch                  */

typedef void* oess_stream_t; /* hipStream_t */

/* Library / device identification.  OESS_ABI_VERSION is bumped whenever a signature of this header changes or an entry point
 * is removed; oess_abi_version() returns the value the library was built with and the ctypes binding (openess_amd/_lib.py,
 * ABI_VERSION) refuses a library whose value differs. */
#define OESS_ABI_VERSION 13
int oess_abi_version(void);
const char* oess_build_info(void);           /* "liboess <ver> gfx950 hipcc <ver>" */
const char* oess_strerror(int code);

/* ------------------------------------------------------------------------------------------
 * K1  Tri-linear event voxelizer.
 * Replaces VoxelGrid.convert (DSEC/dataset/representations.py:15-54), called once per segment
 * (sub-window) from Sequence.generate_event_tensor (DSEC/dataset/sequence_ov.py:212-223).
 *
 * x,y,p,t: float32 SoA exactly as passed to VoxelGrid.convert (t already normalised to [0,1] by
 * the caller, sequence_ov.py:155-156).  Segment s owns events [seg_offsets[s], seg_offsets[s+1])
 * and writes output channels [s*C, (s+1)*C).  out is (n_seg*C) x (H-crop_rows) x W float32,
 * every element written exactly once (no pre-zeroing needed).  crop_rows fuses the
 * `event_tensor[:, :-40, :]` crop (sequence_ov.py:307).  count_mode != 0 replaces every weight by
 * 1.0 (integer hit histogram; used by the bit-exact index tests).
 * ------------------------------------------------------------------------------------------ */
/* Workspace for any voxelizer call with at most n_events events in n_seg segments of at most
 * max_seg_len events each (C = accumulated channels: bins for tri-linear, 2*bins for nearest). */
size_t oess_voxelize_workspace_bytes(int64_t n_events, int n_seg, int64_t max_seg_len, int C, int H, int W,
                                     int crop_rows);

int oess_voxelize_trilinear_f32(const float* x, const float* y, const float* p, const float* t,
                                const int64_t* seg_offsets, int n_seg, int64_t max_seg_len,
                                int C, int H, int W, int crop_rows, int count_mode,
                                float* out, void* workspace, size_t workspace_bytes, oess_stream_t stream);

/* Same, straight from raw DSEC event columns (events.h5 `events/{x,y,t,p}`, eventslicer.py:32-98):
 * fuses rectify_events (sequence_ov.py:204-210: rectify_map[y, x] -> (x', y'), map is H x W x 2
 * float32; seg_map[s] selects one of n_maps maps, one per sequence), the float64->float32 time
 * normalisation of events_to_voxel_grid (sequence_ov.py:154-157) and K1. */
int oess_voxelize_dsec_raw(const uint16_t* x, const uint16_t* y, const int64_t* t_us, const uint8_t* p,
                           const float* rectify_maps, const int32_t* seg_map, int n_maps,
                           const int64_t* seg_offsets, int n_seg, int64_t max_seg_len,
                           int C, int H, int W, int crop_rows, int count_mode,
                           float* out, void* workspace, size_t workspace_bytes, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K1' Nearest-xy / linear-t voxelizer.
 * Replaces generate_voxel_grid (datasets/data_util.py:51-117) called per chunk from
 * DDD17Events.__getitem__ (datasets/ddd17_events_loader.py:161-173).
 * events: [N x 4] rows (x, y, t, p), int64 (DDD17 memmap loader) or float64.
 * Output channels per segment: separate_pol ? 2*nbins (pos then neg) : nbins (pos - neg).
 * out is (n_seg*ch) x (H-crop_rows) x W float32.
 * ------------------------------------------------------------------------------------------ */
int oess_voxelize_nearest_i64(const int64_t* events, const int64_t* seg_offsets, int n_seg, int64_t max_seg_len,
                              int nbins, int H, int W, int crop_rows, int separate_pol, int count_mode,
                              float* out, void* workspace, size_t workspace_bytes, oess_stream_t stream);
int oess_voxelize_nearest_f64(const double* events, const int64_t* seg_offsets, int n_seg, int64_t max_seg_len,
                              int nbins, int H, int W, int crop_rows, int separate_pol, int count_mode,
                              float* out, void* workspace, size_t workspace_bytes, oess_stream_t stream);

/* generate_event_histogram (datasets/data_util.py:17-35): 2 x H x W [neg, pos] counts per segment.
 * (The reference does no bounds check; out-of-range events are DROPPED here instead of raising.) */
int oess_event_histogram_i64(const int64_t* events, const int64_t* seg_offsets, int n_seg, int64_t max_seg_len,
                             int H, int W, float* out, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K2  Masked (non-zero) normalisation of a whole tensor.
 * Replaces EventPreprocessor.__call__ normalisation (e2vid/utils/inference_utils.py:78-85) and
 * normalize_voxel_grid (datasets/data_util.py:38-48).  in/out: n float32 (may alias).
 * stats: oess_masked_stats_doubles(1) doubles of caller-owned device scratch: the totals {sum, sumsq, nnz, -} first, then one
 * row of partial sums per workgroup, added in a fixed order by a finalize launch (deterministic: no floating-point atomics).
 * No host sync: the "if num_nonzeros > 0" test happens on the device.
 * ------------------------------------------------------------------------------------------ */
size_t oess_masked_stats_doubles(int n_slices);
int oess_masked_normalize_f32(const float* in, float* out, int64_t n, double* stats, oess_stream_t stream);
/* Strided variant for a channel slice [B, c0:c0+Cs, H, W] of a [B, Ctot, H, W] tensor (the 5-bin
 * sub-window slice event[:, 5i:5i+5], training/pretrain_trainer.py:437-440). out is dense B x Cs x HW. */
int oess_masked_normalize_slice_f32(const float* in, float* out, int B, int Ctot, int c0, int Cs, int64_t HW,
                                    double* stats, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K7  Superpixel scatter-mean (segment mean) and its backward.
 * Replaces the inline sparse one-hot matmul of training/pretrain_trainer.py:445-465.
 * feat: pixel-major [P x Cf] (NHWC flattened, P = B*H*W), float32 or bf16 (is_bf16).
 * ids: [P] int64 raw superpixel ids; the per-sample offset b*superpixel_size is added inside
 * (pixels_per_sample = H*W).  k: [S x Cf] float32, count: [S] float32, both fully written.
 * Pixels whose offset id is outside [0, S) are an error in the reference (S = max id + 1) and are
 * ignored here.
 * Deterministic (bit-repeatable): partial sums meet as 64-bit fixed-point integers (2^-32 units; 96-bit global
 * accumulators in `workspace`, oess_segment_mean_fwd_workspace_bytes(S, Cf) bytes, 16-byte aligned).  Range
 * contract: finite features with |x| < 32768; anything else makes the WHOLE of k NaN.
 * ------------------------------------------------------------------------------------------ */
size_t oess_segment_mean_fwd_workspace_bytes(int S, int Cf);
int oess_segment_mean_fwd(const void* feat, int is_bf16, const int64_t* ids, int64_t P, int64_t pixels_per_sample,
                          int superpixel_size, int Cf, int S, float* k, float* count, void* workspace,
                          size_t workspace_bytes, oess_stream_t stream);
/* grad_feat[p, :] = grad_k[id(p), :] / (count[id(p)] + 1e-6)  (float32 or bf16 output).  workspace (nullable): S * Cf *
 * sizeof(output element) bytes, 16-byte aligned: the S x Cf quotients are then formed once and the per-pixel pass is a row gather. */
int oess_segment_mean_bwd(const float* grad_k, const float* count, const int64_t* ids, int64_t P,
                          int64_t pixels_per_sample, int superpixel_size, int Cf, int S,
                          void* grad_feat, int is_bf16, void* workspace, size_t workspace_bytes, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K9  TaskLoss = DiceLoss + CrossEntropyLoss(ignore_index) forward and backward.
 * Replaces utils/loss_functions.py:17-24 (TaskLoss), :114-135 (DiceLoss), :80-90 (BinaryDiceLoss).
 * logits element (pixel p, class c) lives at logits[p*stride_p + c*stride_c] within a sample of
 * `pixels_per_sample` pixels whose base is b*stride_b (covers NCHW: stride_p=1, stride_c=HW,
 * stride_b=K*HW; and NHWC: stride_p=K, stride_c=1, stride_b=HW*K).  float32 or bf16.
 * target: [P] int64.  sums: oess_task_loss_sums_doubles(K) doubles of scratch: {inter[K], psq[K], ysum[K], ce_sum, n_valid}
 * totals (written by the fwd call, consumed by the bwd call) followed by one row of partial sums per forward workgroup, which
 * the fwd call adds in row order (no atomics: bit-repeatable).  loss_out: 3 floats {total, dice, ce}.
 * flags bit0 = dice, bit1 = cross-entropy.
 * ------------------------------------------------------------------------------------------ */
size_t oess_task_loss_sums_doubles(int K);
int oess_task_loss_fwd(const void* logits, int is_bf16, const int64_t* target, int64_t P, int64_t pixels_per_sample,
                       int64_t stride_b, int64_t stride_p, int64_t stride_c, int K, int ignore_index, int flags,
                       double* sums, float* loss_out, oess_stream_t stream);
int oess_task_loss_bwd(const void* logits, int is_bf16, const int64_t* target, int64_t P, int64_t pixels_per_sample,
                       int64_t stride_b, int64_t stride_p, int64_t stride_c, int K, int ignore_index, int flags,
                       const double* sums, float grad_scale, const float* grad_scale_dev /* nullable: multiplies grad_scale */,
                       void* grad_logits, int grad_is_bf16, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * a16 Consistency losses of the joint OpenESS stage (training/openess_trainer.py:497-503):
 *   oess_l1_mean_*      cons_feat_loss = nn.L1Loss()(feat_a, feat_b)  (mean |a - b| over n elements, same memory order)
 *   oess_cosine_mean_*  cons_pred_loss = mean(1 - F.cosine_similarity(logits_a, logits_b, dim=1)) over P pixels x C
 *                       channels, NHWC with pixel strides in elements, eps = 1e-8 per-norm clamp (torch 2.x formula).
 * Operands bf16 (is_bf16 != 0) or fp32; gradients are written in the operand dtype (either may be null).
 * partials: scratch of oess_loss_partials_bytes() bytes (deterministic two-stage sum); loss / grad_out: device scalars.
 * ------------------------------------------------------------------------------------------ */
size_t oess_loss_partials_bytes(void);
int oess_l1_mean_fwd(const void* a, const void* b, int64_t n, int is_bf16, void* partials, float* loss, oess_stream_t stream);
int oess_l1_mean_bwd(const void* a, const void* b, int64_t n, int is_bf16, const float* grad_out, void* grad_a, void* grad_b,
                     oess_stream_t stream);
int oess_cosine_mean_fwd(const void* a, long long a_pix_stride, const void* b, long long b_pix_stride, int64_t P, int C,
                         int is_bf16, float eps, void* partials, float* loss, oess_stream_t stream);
int oess_cosine_mean_bwd(const void* a, long long a_pix_stride, const void* b, long long b_pix_stride, int64_t P, int C,
                         int is_bf16, float eps, const float* grad_out, void* grad_a, long long ga_pix_stride, void* grad_b,
                         long long gb_pix_stride, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * a14 PointInfoNCE, NCELoss.forward (utils/loss_functions.py:147-154): loss = CrossEntropy(k q^T / T, arange(S)).
 * k, q: fp32 [S x C] (superpixel means).  The forward leaves dL/d(k q^T) = (softmax - I) / (S T) in grad_logits
 * [S x S] fp32, which the backward multiplies out: grad_k = g * G q, grad_q = g * G^T k (either may be null).
 * partials: scratch of >= S doubles; loss / grad_out: device scalars.
 * ------------------------------------------------------------------------------------------ */
int oess_nce_loss_fwd(const float* k, const float* q, int S, int C, float temperature, float* grad_logits, void* partials,
                      size_t partials_bytes, float* loss, oess_stream_t stream);
int oess_nce_loss_bwd(const float* grad_logits, const float* k, const float* q, int S, int C, const float* grad_out, float* grad_k,
                      float* grad_q, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * a18 AdamW step for a whole parameter list in one launch (torch.optim.AdamW as built in
 * training/pretrain_trainer.py:231-243: decoupled weight decay, amsgrad off), ATen's operation order.
 * table: device int64 [n_tensors][5] = {param, grad, exp_avg, exp_avg_sq pointers (fp32), numel};
 * chunk_map: device int32 [n_chunks][2] = {tensor index, chunk index}, chunks of chunk_elems elements.
 * bias_correction1 = 1 - beta1^step, bias_correction2_sqrt = sqrt(1 - beta2^step); all scalars are doubles (the Python
 * optimiser's own values) and are rounded to fp32 once, so 1 - beta2 etc. match the library bit for bit.
 * ------------------------------------------------------------------------------------------ */
int oess_adamw_multi_f32(const int64_t* table, int n_tensors, const int32_t* chunk_map, int n_chunks, int chunk_elems, double lr,
                         double beta1, double beta2, double eps, double weight_decay, double bias_correction1,
                         double bias_correction2_sqrt, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K11 Confusion matrix (evaluation/metrics.py:4-23): conf[gt*K + pred] += 1 over gt != ignore.
 * conf: K*K int64, ACCUMULATED into (caller zeroes once per validation epoch).
 * ------------------------------------------------------------------------------------------ */
int oess_confusion_accumulate(const int64_t* pred, const int64_t* label, int64_t n, int K, int ignore_label,
                              int64_t* conf, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MFMA implicit-GEMM convolution (bf16 in, fp32 accumulate), NHWC with explicit pixel strides.
 * Replaces the ATen/cuDNN conv2d calls behind nn.Conv2d in e2vid/model/submodules.py:7-31,175-214
 * (ConvLayer, ConvLSTM.Gates), models/_resnet.py:74-114 (Bottleneck), models/deeplabv3.py:295-348
 * (ASPP) and models/style_networks.py:252-289 (ReLUINSConv2d / INSResBlock).
 *
 * oess_conv2d_pack_weight: OIHW fp32 (Conv2d.weight) -> packed bf16 [Npad][Kpad], K = (r, s, ci);
 *   flip_for_dgrad == 1 packs the data-gradient operator (taps rotated 180 deg, in/out swapped) so
 *   that dX = conv(dY, packed, pad = dil*(R-1) - pad) for stride-1 convolutions; == 2 packs the forward operator
 *   with ConvLSTM gate-interleaved rows for oess_convlstm_fused_bf16.
 * oess_conv2d_fwd_bf16: out = act(conv(in, w) + bias [+ residual]); Cin must be a multiple of 8
 *   (pad the channel dimension; padded weights are zero).  Exactly one of out_bf16 / out_f32 is used
 *   (out_f32 wins when non-null).  Pixel strides are in ELEMENTS.  relu: 0 = none, 1 = ReLU, 2 = GELU (erf form).
 * ------------------------------------------------------------------------------------------ */
size_t oess_conv2d_packed_bytes(int Cout, int Cin, int R, int S, int flip_for_dgrad);
int oess_conv2d_pack_weight(const float* w_oihw, int Cout, int Cin, int R, int S, int flip_for_dgrad, void* packed,
                            size_t packed_bytes, oess_stream_t stream);
/* The same packing for n weights in ONE launch (all trainable convolutions of a model after an optimiser step); Cout % 8 == 0
 * and Cin % 8 == 0.  table_dev: n rows of eight 64-bit words in DEVICE memory, the last one the problem's first workgroup
 * (problem p owns oess_conv2d_pack_multi_blocks(...) workgroups; total_blocks = their sum).
 *   flip_from_packed == 0: rows {w_oihw fp32, packed forward operand, Cout, Cin, R, S, 0, first block};
 *   flip_from_packed == 1: rows {packed forward operand, packed data-gradient operand, Cout, Cin, R, S, 0, first block}: the
 *                          flip_for_dgrad = 1 operand formed from the (already current) forward operand by tile transposes.
 * Only the valid region of a destination is written: it must have been packed once by oess_conv2d_pack_weight (zero padding).
 * The caller uploads the table (and may cache it while the pointers repeat). */
long long oess_conv2d_pack_multi_blocks(int Cout, int Cin, int R, int S, int flip_from_packed);
int oess_conv2d_pack_weight_multi(const long long* table_dev, int n, long long total_blocks, int flip_from_packed,
                                  oess_stream_t stream);
int oess_conv2d_fwd_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin, const void* w_packed,
                         const float* bias, int Cout, int R, int S, int stride, int pad, int dil, int relu,
                         const void* residual, long long res_pix_stride, void* out_bf16, float* out_f32,
                         long long out_pix_stride, float* tile_stats, void* workspace, size_t workspace_bytes,
                         oess_stream_t stream);
/* Statistics only: the 1x1 stride-1 bias-free convolution in front of a train-mode BatchNorm whose RESULT nobody reads (a frozen
 * network run for its running statistics).  tile_stats gets what oess_conv2d_fwd_bf16 would write there (sums of the bf16-rounded
 * results), no result is stored.  Exists where that call, with a dense aligned output, takes OESS_ROUTE_CONV1X1_W128
 * (oess_conv2d_fwd_route says so); OESS_EINVAL elsewhere: run the storing call. */
int oess_conv2d_stats_only_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin, const void* w_packed, int Cout,
                                float* tile_stats, oess_stream_t stream);
/* workspace (nullable): oess_conv2d_fwd_workspace_bytes(...) bytes of scratch for the split-K form that small-M / long-K layers
 * take (ASPP dilated 3x3 at output stride 16, models/deeplabv3.py:295-348: 140 workgroups x 288 K-slabs otherwise); the query
 * returns 0 for layers that run in one pass.  Without a workspace every layer runs in one pass (same result up to the
 * summation order of the fp32 accumulators). */
size_t oess_conv2d_fwd_workspace_bytes(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil,
                                       int with_tile_stats, int out_is_f32);
/* Which kernel a call takes.  oess_conv2d_fwd_bf16 is one entry point over the kernels below; the choice depends on the geometry,
 * the epilogue flags, the pixel strides, the output pointer's 16-byte alignment and the workspace on offer.
 * oess_conv2d_fwd_route makes the plan the launch itself executes (conv_plan: the dispatch rules) and returns its OESS_ROUTE_*
 * value instead of launching.  Host only: no launch, no attribute call, no allocation; the one runtime call is the
 * rules' query of the device's CU count, which falls back to 256 without a GPU (so the query runs on any machine, and the
 * w128 rules answer for the current device).  The OESS_W128_* environment knobs of the launch apply to the query as well.  Negative = OESS_E*, as the launch would return.  Split-K routes carry the slice count:
 * route = OESS_ROUTE_SPLITK_* | ks << 8; OESS_ROUTE_KERNEL(route) strips it.  oess_convlstm_fused_route is the same query for
 * oess_convlstm_fused_bf16.  Values are stable: new kernels append, OESS_ROUTE_COUNT grows. */
#define OESS_ROUTE_SMALLCIN 1          /* conv_smallcin_kernel<5, 5>: Cin = 8 stencil (E2VID head)                         */
#define OESS_ROUTE_FALLBACK_128 2      /* conv_fwd_kernel<128>: register-staged, no LDS-DMA (input >= 2 GiB, K >= 32768)   */
#define OESS_ROUTE_FALLBACK_64 3       /* conv_fwd_kernel<64>                                                              */
#define OESS_ROUTE_FALLBACK_32 4       /* conv_fwd_kernel<32>                                                              */
#define OESS_ROUTE_S2_HALO 5           /* conv5x5s2_halo_kernel<false>: 5x5 stride-2 pad-2                                 */
#define OESS_ROUTE_SMALLMAP_RING 6     /* conv_fwd_dma_kernel<128, 128, 4, true, 0, 512>: small maps, 4-deep ring          */
#define OESS_ROUTE_CONV3X3_W128 7      /* conv3x3_w128_kernel: persistent 3x3 in front of a BatchNorm                      */
#define OESS_ROUTE_HALO3X3 8           /* conv3x3_halo_kernel<0>: 3x3 'same' row-halo                                      */
#define OESS_ROUTE_HALO3X3_LSTM 9      /* conv3x3_halo_kernel<1>: the same with the fused ConvLSTM epilogue                */
#define OESS_ROUTE_LSTM_FASTK 10       /* conv_fwd_dma_kernel<128, 128, 2, true, 1>: fused ConvLSTM, other geometries      */
#define OESS_ROUTE_LSTM_SLOWK 11       /* conv_fwd_dma_kernel<128, 128, 2, false, 1>                                       */
#define OESS_ROUTE_SPLITK_FASTK 12     /* conv_fwd_dma_kernel<128, 128, 2, true> over ks slices + splitk_reduce_kernel     */
#define OESS_ROUTE_SPLITK_SLOWK 13     /* conv_fwd_dma_kernel<128, 128, 2, false> over ks slices + splitk_reduce_kernel    */
#define OESS_ROUTE_CONV1X1_W128 14     /* conv1x1_w128_kernel: persistent 1x1                                              */
#define OESS_ROUTE_TILE256 15          /* conv_fwd_dma_kernel<256, 256, 2, true>                                           */
#define OESS_ROUTE_RING32 16           /* conv_fwd_dma32_kernel<128, true, 0, 3>: K <= 256, BK = 32 ring                   */
#define OESS_ROUTE_TILE64_FASTK 17     /* conv_fwd_dma_kernel<64, 128, 2, true>: 64-row tiles                              */
#define OESS_ROUTE_TILE64_SLOWK 18     /* conv_fwd_dma_kernel<64, 128, 2, false>                                           */
#define OESS_ROUTE_DMA128_FASTK 19     /* conv_fwd_dma_kernel<128, 128, 2, true>: the general kernel                       */
#define OESS_ROUTE_DMA128_SLOWK 20     /* conv_fwd_dma_kernel<128, 128, 2, false>                                          */
#define OESS_ROUTE_DMA64_FASTK 21      /* conv_fwd_dma_kernel<128, 64, 2, true>                                            */
#define OESS_ROUTE_DMA64_SLOWK 22      /* conv_fwd_dma_kernel<128, 64, 2, false>                                           */
#define OESS_ROUTE_DMA32_FASTK 23      /* conv_fwd_dma_kernel<128, 32, 2, true>                                            */
#define OESS_ROUTE_DMA32_SLOWK 24      /* conv_fwd_dma_kernel<128, 32, 2, false>                                           */
#define OESS_ROUTE_COUNT 24            /* kernels are 1 .. OESS_ROUTE_COUNT                                                */
#define OESS_ROUTE_KERNEL(route) ((route) & 0xff)
#define OESS_ROUTE_KSPLIT(route) ((route) >> 8)
int oess_conv2d_fwd_route(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dil, int has_bias,
                          int relu, int has_residual, int out_is_f32, int with_tile_stats, long long in_pix_stride,
                          long long out_pix_stride, long long res_pix_stride, int out_aligned16, size_t workspace_bytes);
int oess_convlstm_fused_route(int B, int H, int W, int Cin, long long in_pix_stride, int C_hidden, int R, int S, int pad,
                              long long hidden_pix_stride);
int oess_conv2d_route_count(void);             /* == OESS_ROUTE_COUNT of the header the library was built from */
const char* oess_conv2d_route_name(int route); /* kernel name of a route value (static string; "?" for anything else) */
/* tile_stats (nullable): [ceil(M/128)][2][Cout] fp32, per-128-row-tile column sums and sums of squares of the fp32
 * result (BatchNorm batch statistics straight from the accumulators; bias-free, no activation/residual).  Every row is written.
 * One kernel differs: OESS_ROUTE_TILE256 (256 x 256 tiles) puts the sums of its 256 rows into row 2t and zeroes row 2t + 1
 * (where the table has it), so only the sum over rows is kernel-independent; all other routes fill genuine 128-row rows.
 * oess_norm_reduce_finalize_tile_stats turns them into mean / rstd / scale / shift. */

/* Reduce + finalize (G = 1), sums and E[x^2] - E[x]^2 in double, slices added in a FIXED order (bit-repeatable):
 * the tile partials of a conv epilogue -> mean / rstd / scale / shift (+ BatchNorm running statistics;
 * models/image_model.py:113-114 leaves the frozen teacher in .train()).  One launch for <= 64 tiles, otherwise a slice-sum launch
 * and a finalize launch (the kernel boundary is the synchronisation).  `scratch`: caller-owned double[32 * 2 * C] (any
 * content), `counters`: caller-owned uint32[(C + 31) / 32], ZERO on entry and left zero on return (only touched by the opt-in
 * one-launch ticket protocol, environment OESS_BN_ONE_LAUNCH=1, kept for A/B measurements). */
int oess_norm_reduce_finalize_tile_stats(const float* tile_stats, int tiles, int C, double* scratch,
                                         unsigned int* counters, float count, float eps, const float* gamma, const float* beta,
                                         float* running_mean, float* running_var, float momentum, float* mean, float* rstd,
                                         float* scale, float* shift, oess_stream_t stream);

/* Small maps (tiles <= 512, C % 64 == 0): the reduce / finalize above AND oess_norm_apply_nhwc_bf16 in one launch, no
 * cross-workgroup protocol: every workgroup re-reduces the tile partials of its 64 channels (fixed order, double) and
 * applies out = act(x * scale + shift [+ residual]) to its pixel chunk; x may alias out.  mean / rstd nullable. */
int oess_norm_tile_stats_apply_nhwc_bf16(const float* tile_stats, int tiles, int C, float count, float eps, const float* gamma,
                                         const float* beta, float* running_mean, float* running_var, float momentum, float* mean,
                                         float* rstd, const void* x, long long x_pix_stride, const void* residual,
                                         long long res_pix_stride, int relu, long long pixels, void* out, long long out_pix_stride,
                                         oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ConvLSTM gate fusion.  Replaces the chunk/sigmoid/tanh/mul/add tail of ConvLSTM.forward
 * (e2vid/model/submodules.py:205-212).  gates: [P x 4C] bf16 (in, remember, out, cell blocks);
 * cell state fp32 [P x C] (prev_cell may be null = zero state; cell may alias prev_cell);
 * hidden bf16 with its own pixel stride (a channel slice of the cat(x, h) buffer).
 * ------------------------------------------------------------------------------------------ */
int oess_convlstm_gates_bf16(const void* gates, long long gates_pix_stride, const float* prev_cell, float* cell,
                             void* hidden, long long hidden_pix_stride, long long n_pixels, int C, oess_stream_t stream);

/* E2VID head + first encoder conv in ONE kernel (e2vid/model/unet.py:137-146, submodules.py ConvLayer: head = 5x5 stride 1,
 * bins -> 32 channels; encoder 0's conv = 5x5 stride 2, 32 -> 64): out = act_e(conv5x5s2(act_h(conv5x5(x8) + head_bias)) + enc_bias).
 * The 32-channel head output never reaches memory: every 8 x 16-pixel output patch computes the 19 x 35 head pixels under it
 * into LDS.  x8: NHWC bf16 with 8 channels (bins zero-padded); head_w_packed = oess_conv2d_pack_weight of the [32, 8, 5, 5] weight,
 * enc_w_packed of the [64, 32, 5, 5] weight; *_relu in {0, 1}; out: NHWC bf16 [B, (H-1)/2+1, (W-1)/2+1, 64] view, pixel stride
 * out_pix_stride (a channel slice of the ConvLSTM's cat(x, h) buffer), 16-byte aligned.  Same result as the two
 * oess_conv2d_fwd_bf16 calls (the head output rounded to bf16 in between, as there). */
/* The same kernel fed from the fp32 event tensor [B, Ctot, H, W]: the EventPreprocessor apply of the slice events[:, c0:c0+Cs]
 * (e2vid/utils/inference_utils.py:80-85; stats = {sum, sumsq, nnz} from oess_masked_stats_slice(s)_f32, normalize = 0 skips it)
 * and the zero-padded 8-channel bf16 packing happen per patch inside the kernel: the NHWC8 tensor of
 * oess_event_slice_to_nhwc8_bf16 is never written either.  Cs <= 5.  Same result as that call followed by
 * oess_e2vid_head_enc0_bf16. */
int oess_e2vid_events_head_enc0_bf16(const float* events, int B, int Ctot, int c0, int Cs, int H, int W, const double* stats,
                                     int normalize, const void* head_w_packed, const float* head_bias, int head_relu,
                                     const void* enc_w_packed, const float* enc_bias, int enc_relu, void* out,
                                     long long out_pix_stride, oess_stream_t stream);
int oess_e2vid_head_enc0_bf16(const void* x8, long long x8_pix_stride, int B, int H, int W, const void* head_w_packed,
                              const float* head_bias, int head_relu, const void* enc_w_packed, const float* enc_bias, int enc_relu,
                              void* out, long long out_pix_stride, oess_stream_t stream);

/* ConvLSTM step in ONE kernel: Gates convolution (submodules.py:202-203) + the cell update above, fused in the MFMA
 * epilogue.  w_packed_gates comes from oess_conv2d_pack_weight(..., flip_for_dgrad = 2): the 4C Conv2d rows are packed
 * gate-interleaved (row 4*hc + gate) so that one lane of the transposed accumulator owns the four gates of a hidden
 * channel; bias stays in Conv2d order [4C].  in = cat(x, h_prev) NHWC bf16 (Cin = Cx + C); hidden (bf16, own pixel
 * stride) must NOT overlap `in` (neighbouring tiles still read h_prev: ping-pong two cat buffers); cell may alias
 * prev_cell (null = zero state).  C_hidden % 32 == 0, stride 1, dilation 1.  The 4C-channel gate tensor is never
 * written (-512 B/pixel of HBM traffic per step at C = 64 versus conv + oess_convlstm_gates_bf16). */
int oess_convlstm_fused_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin,
                             const void* w_packed_gates, const float* bias, int C_hidden, int R, int S, int pad,
                             const float* prev_cell, float* cell, void* hidden, long long hidden_pix_stride,
                             oess_stream_t stream);

/* n <= 3 INDEPENDENT ConvLSTM steps (arguments as oess_convlstm_fused_bf16) in ONE launch: the three levels of E2VID's recurrent
 * encoder (e2vid/model/unet.py:141-150) on the skewed schedule, where level l works on sub-window s - l, so the three Gates
 * convolutions of a stage have no dependency on each other.  Results are those of n separate calls (same tiles, same arithmetic);
 * what the single launch saves is each level's partial last round of tiles and two launch gaps.  No output (hidden, cell) of one
 * problem may overlap any buffer of another (checked).  Geometries the row-halo kernel does not take run as n launches. */
typedef struct {
    const void* in; long long in_pix_stride; int B, H, W, Cin;
    const void* w_packed_gates; const float* bias; int C_hidden, R, S, pad;
    const float* prev_cell; float* cell; void* hidden; long long hidden_pix_stride;
} oess_convlstm_desc_t;
int oess_convlstm_fused_group_bf16(const oess_convlstm_desc_t* problems, int n, oess_stream_t stream);

/* The same n <= 3 ConvLSTM steps on the round-6 kernel (csrc/conv_lstm_w128.h: persistent workgroups, one wave per SIMD on a
 * 128-pixel x 128-gate-column accumulator block, hand-laid MFMA / LDS / LDS-DMA stream).  Replaces ConvLSTM.forward
 * (e2vid/model/submodules.py:199-214) exactly as oess_convlstm_fused_bf16 does; what differs is the STORAGE of the cell state:
 * prev_cell / cell are in the kernel's own "w128-tiled" layout ([tile of 256 pixels x 64 channels][wave][16][lane][4] fp32 = the
 * accumulator layout, oess_convlstm_w128_cell_bytes(B*H*W, C) bytes: the pixel count is padded to a multiple of 256), so the
 * previous cell arrives and the new cell leaves with coalesced 16-byte accesses and no transposition.  The cell state never
 * leaves the recurrent encoder (submodules.py:205-212 only feeds it back); oess_convlstm_w128_cell_relayout converts to and from
 * the reference's [B,H,W,C] order for state import / export and tests.  cell may equal prev_cell (a tile updates its own block)
 * or be disjoint from it; hidden (NHWC bf16, own pixel stride) must not overlap `in`; no output of one problem may overlap
 * another problem's buffers (checked).  Takes 3 x 3 / pad 1 Gates with Cin % 64 == 0, C_hidden % 64 == 0, H >= 8 and 32-bit
 * extents; anything else returns OESS_EINVAL before any launch (callers fall back to oess_convlstm_fused_group_bf16 on a cell
 * state in [B,H,W,C] order).  Gate arithmetic: bias added inside the exponent's FMA, sigmoid / tanh via exp2 + rcp (the fused
 * kernels' fast forms); results agree with oess_convlstm_fused_bf16 to fp32 rounding of that reassociation. */
size_t oess_convlstm_w128_cell_bytes(long long pixels, int C_hidden);      /* 0 when C_hidden % 64 != 0 */
int oess_convlstm_w128_cell_relayout(const float* src, float* dst, long long pixels, int C_hidden, int to_tiled, oess_stream_t stream);
int oess_convlstm_w128_group_bf16(const oess_convlstm_desc_t* problems, int n, oess_stream_t stream);
/* Host-only: the static tile lists the kernel above walks (one list per persistent workgroup; entry = (problem << 24) | tile of 256
 * pixels x 256 gate columns, -1 ends a list; problems longest-K first, greedy onto the least loaded workgroup of the tile's XCD).
 * lists (may be NULL: only *stride is returned) receives grid x *stride ints; capacity = its size in ints.  No device work: the
 * CPU tests check that every tile of every problem appears exactly once. */
int oess_convlstm_w128_tile_lists(const int* tiles_m, const int* tiles_n, const int* cin, int n, int grid, int* lists, int capacity, int* stride);

/* ------------------------------------------------------------------------------------------
 * K28 ConvGRU (e2vid/model/submodules.py:217-253 of the reference; recurrent_block_type 'convgru').  Additions only: the ABI
 * version and OESS_ROUTE_COUNT stay (these are entry points of their own, not routes of oess_conv2d_fwd_bf16).
 *   u = sigmoid(conv(cat(x, h), Wu) + bu),  r = sigmoid(conv(cat(x, h), Wr) + br)          (gates)
 *   o = tanh(conv(cat(x, r * h), Wo) + bo), h' = h * (1 - u) + o * u                        (output)
 *
 * bf16: TWO launches per step, each an LDS-DMA MFMA convolution with the gate algebra in its epilogue; u, r and o never exist as
 * pre-activation tensors, nothing is concatenated or copied.  h is kept in fp32 ([B H W][C], dense: the "master") next to the
 * bf16 copy the next step convolves, as the ConvLSTM cell is: the blend does not round h to bf16 once per step.
 * Geometry: 3 x 3 / pad 1, C_hidden % 32 == 0, Cin == 2 C_hidden (the two-part window) or Cin == C_hidden (x alone with the
 * x-half weights: the step from a zero state, h_prev must then be NULL), in_pix_stride and the output pixel strides % 8 == 0,
 * every pointer 16-byte aligned, B H W < 2^31 and the input window below 2 GiB.  Anything else -- a 5 x 5 gate, another
 * Cin (input_size != hidden_size), C_hidden % 32 != 0, a null pointer -- returns OESS_EINVAL before any launch; there is no
 * other bf16 form.  Pixel strides are in ELEMENTS.
 *   oess_convgru_gates_bf16: in = the (h | x) window (or x alone), NHWC bf16.  w_packed_gates = oess_conv2d_pack_weight(.., 0) of
 *     the [2 C, Cin, 3, 3] weight whose row 2 hc + g is row hc of Wu (g = 0) / Wr (g = 1), input channels in the window's order;
 *     bias = [bu | br] (2 C floats) or NULL.  h_prev: the fp32 master or NULL (= zero state).  Writes u (fp32 [B H W][C]) and
 *     bf16(r * h_prev) into the window rh (pixel stride rh_pix_stride); rh_f32 (nullable, fp32 [B H W][C]) receives r * h_prev
 *     before that rounding (tests).  No output may overlap `in`, h_prev or another output (checked, OESS_EINVAL): channel windows
 *     of ONE buffer (same pixel stride) that do not share a channel count as disjoint.
 *   oess_convgru_out_bf16: in = the (x | r * h) window (or x alone); w_packed = oess_conv2d_pack_weight(.., 0) of Wo restricted
 *     to the window's channels; bias = bo or NULL; u from the gates launch.  Writes the new master h (fp32; h == h_prev, in
 *     place, is allowed: a value is read and written by the one lane that owns it) and its bf16 rounding into the window h_bf16.
 *     h_bf16 and h must not overlap `in`, u or each other, h_bf16 not h_prev, and h overlaps h_prev only by being it (checked).
 *   One NHWC bf16 buffer [B][H][W][3 C] ordered h | x | r * h serves both: the encoder conv writes x into [C, 2C), the gates
 *   launch convolves [0, 2C) (Wu / Wr with their input-channel halves swapped at pack time) and writes [2C, 3C), the output launch
 *   convolves [C, 3C) in the reference's own channel order and writes [0, C).  No launch writes a window it convolves.
 *   sigmoid / tanh are the fused ConvLSTM's fast forms (exp + rcp).
 *
 * fp32: oess_conv2d_fwd_f32 produces the pre-activations ([B H W][2 C] = u | r, then [B H W][C] = o, dense), two pointwise
 * kernels do the rest: four launches per step.  oess_convgru_f32_workspace_bytes(pixels, C) = room for both pre-activation
 * tensors and u (4 C floats per pixel).  No geometry rule beyond the convolution's own.
 *   oess_convgru_gates_f32: u = sigmoid(pre[:, :C]) -> u (dense), sigmoid(pre[:, C:]) * h_prev -> the view rh.  h_prev NULL = zero.
 *   oess_convgru_blend_f32: h = h_prev * (1 - u) + tanh(pre) * u -> the view h (h may be the view h_prev itself).
 *   Views are B x H x W x C_hidden.  An output may not overlap an input or another output, except rh / h being the very view
 *   h_prev (element-wise in place); NHWC channel windows of one buffer count as disjoint as above, other views by their byte
 *   range; negative strides, null data, pointers off 4 bytes and more than (2^31 - 1) * 256 elements (one thread each on a
 *   one-dimensional grid; the workspace query answers 0 there) are OESS_EINVAL.
 * ------------------------------------------------------------------------------------------ */
int oess_convgru_gates_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin, const void* w_packed_gates,
                            const float* bias, int C_hidden, int R, int S, int pad, const float* h_prev, float* u, void* rh,
                            long long rh_pix_stride, float* rh_f32, oess_stream_t stream);
int oess_convgru_out_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int Cin, const void* w_packed,
                          const float* bias, int C_hidden, int R, int S, int pad, const float* u, const float* h_prev, float* h,
                          void* h_bf16, long long h_bf16_pix_stride, oess_stream_t stream);

/* n <= 2 INDEPENDENT 5x5 / stride-2 / pad-2 convolutions (out = act(conv(in, w) + bias), arguments as oess_conv2d_fwd_bf16 with
 * R = S = 5, stride 2, pad 2, relu in {0, 1}) in ONE launch: the encoder ConvLayers of levels 1 and 2 of E2VID's recurrent encoder
 * (e2vid/model/unet.py:141-150, submodules.py:96-115) on the skewed schedule.  Results are those of separate calls.  Neither output
 * may overlap the other problem's input or output (checked); geometries the 2-D-halo kernel does not take run as n launches. */
typedef struct {
    const void* in; long long in_pix_stride; int B, H, W, Cin;
    const void* w_packed; const float* bias; int Cout, relu;
    void* out; long long out_pix_stride;
} oess_conv_s2_desc_t;
int oess_conv5x5s2_group_bf16(const oess_conv_s2_desc_t* problems, int n, oess_stream_t stream);

/* Statistics of a channel slice without the apply pass (first half of K2): stats = {sum, sumsq, nnz, -}. */
/* ... and of n_slices consecutive Cs-channel slices in ONE launch (the 20 sub-windows of a pre-training sample are known up
 * front, pretrain_trainer.py:437-441): stats[4 z ..] = {sum, sumsq, nnz, -} of in[:, z*Cs : (z+1)*Cs].
 * stats holds oess_masked_stats_doubles(n_slices) doubles (1 for the single-slice form): totals first, partial rows behind. */
int oess_masked_stats_slices_f32(const float* in, int B, int Ctot, int Cs, int n_slices, int64_t HW, double* stats,
                                 oess_stream_t stream);
int oess_masked_stats_slice_f32(const float* in, int B, int Ctot, int c0, int Cs, int64_t HW, double* stats,
                                oess_stream_t stream);
/* EventPreprocessor apply (e2vid/utils/inference_utils.py:80-85) fused with the NCHW fp32 -> NHWC bf16
 * (8 channels, zero padded) re-layout that feeds the E2VID head conv.  normalize == 0 only re-lays out. */
int oess_event_slice_to_nhwc8_bf16(const float* in, int B, int Ctot, int c0, int Cs, long long HW, const double* stats,
                                   int normalize, void* out_nhwc8, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K32 EventPreprocessor's hot-pixel removal and flip (e2vid/utils/inference_utils.py:71-75) inside the event kernels.
 * Order as in the reference: events[:, :, y, x] = 0 for every listed pixel, then torch.flip(events, dims=[2, 3]), then the
 * non-zero mean / std normalisation.  hot_mask: H x W bytes on the device, non-zero = hot, in SOURCE coordinates (null = no
 * list); flip != 0 mirrors H and W.  The input tensor is only read (the reference zeroes the caller's tensor in place).
 * Every *_pre entry point computes what its option-less namesake computes on torch.flip(zeroed copy, [2, 3]); `pre` must not
 * be null.  Statistics: hot pixels add nothing to {sum, sumsq, nnz}; the flip does not change them (read in source order).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const unsigned char* hot_mask; /* [H][W], 1 = hot, may be null */
    int flip;
} oess_event_pre_t;
int oess_masked_stats_slice_pre_f32(const float* in, int B, int Ctot, int c0, int Cs, int H, int W, const oess_event_pre_t* pre,
                                    double* stats, oess_stream_t stream);
int oess_masked_stats_slices_pre_f32(const float* in, int B, int Ctot, int Cs, int n_slices, int H, int W,
                                     const oess_event_pre_t* pre, double* stats, oess_stream_t stream);
/* Statistics + apply to dense fp32 NCHW: out[b, c, y, x] = norm(in'[b, c0 + c, H-1-y, W-1-x]) (flip) with in' = in with the hot
 * pixels zeroed; normalize == 0 only zeroes and mirrors.  The whole tensor is the slice c0 = 0, Cs = Ctot.  out must not
 * alias in.  stats as for oess_masked_normalize_slice_f32. */
int oess_masked_normalize_slice_pre_f32(const float* in, float* out, int B, int Ctot, int c0, int Cs, int H, int W,
                                        const oess_event_pre_t* pre, int normalize, double* stats, oess_stream_t stream);
/* oess_event_slice_to_nhwc8_bf16 with the options (normalize == 0 still zeroes and mirrors). */
int oess_event_slice_to_nhwc8_pre_bf16(const float* in, int B, int Ctot, int c0, int Cs, int H, int W, const oess_event_pre_t* pre,
                                       const double* stats, int normalize, void* out_nhwc8, oess_stream_t stream);
/* oess_e2vid_events_head_enc0_bf16 with the options: the per-patch loader reads the mirrored source pixel and the mask; the
 * zero padding at the image border is unchanged. */
int oess_e2vid_events_head_enc0_pre_bf16(const float* events, int B, int Ctot, int c0, int Cs, int H, int W,
                                         const oess_event_pre_t* pre, const double* stats, int normalize,
                                         const void* head_w_packed, const float* head_bias, int head_relu,
                                         const void* enc_w_packed, const float* enc_bias, int enc_relu, void* out,
                                         long long out_pix_stride, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Normalisation and resampling on NHWC bf16 (pixel strides in elements, C % 8 == 0).
 * Replace nn.BatchNorm2d (train-mode batch statistics; models/_resnet.py:74-114, image_model.py:130-143),
 * nn.InstanceNorm2d + ReLU (models/style_networks.py:252-289), F.interpolate(nearest, x2)
 * (style_networks.py:148-160) and nn.Upsample(x4, bilinear, align_corners=True) + F.normalize
 * (image_model.py:121-143).  G groups of pixels_per_group pixels: G = 1 BatchNorm, G = B InstanceNorm.
 * ------------------------------------------------------------------------------------------ */
/* Statistics are DETERMINISTIC: every workgroup writes its partial sums to `partials` (caller workspace of
 * oess_norm_partials_bytes(G, pixels_per_group, C, backward) bytes; backward = 1 for the two *_bwd entry points) and a second
 * kernel adds the rows in a fixed order in double -- no floating-point atomics anywhere on the training path. */
size_t oess_norm_partials_bytes(int G, long long pixels_per_group, int C, int backward);
/* sum[G x C] = sum of x, sumsq[G x C] = sum of x^2 (overwritten; also the bias gradient: sum of dY over pixels) */
int oess_norm_stats_nhwc_bf16(const void* x, long long x_pix_stride, int G, long long pixels_per_group, int C,
                              float* sum, float* sumsq, float* partials, size_t partials_bytes, oess_stream_t stream);
/* statistics + mean / rstd / scale = gamma*rstd / shift = beta - mean*scale per (group, channel), E[x^2] - E[x]^2 in double;
 * G == 1 and running_mean != NULL: nn.BatchNorm2d's running-statistics update (unbiased variance).  gamma / beta nullable. */
int oess_norm_stats_finalize_nhwc_bf16(const void* x, long long x_pix_stride, int G, long long pixels_per_group, int C, float eps,
                                       const float* gamma, const float* beta, float* running_mean, float* running_var,
                                       float momentum, float* mean, float* rstd, float* scale, float* shift, float* partials,
                                       size_t partials_bytes, oess_stream_t stream);
/* out = act(x*scale + shift [+ residual]) */
int oess_norm_apply_nhwc_bf16(const void* x, long long x_pix_stride, const float* scale, const float* shift,
                              const void* residual, long long res_pix_stride, int relu, int G, long long pixels_per_group,
                              int C, void* out, long long out_pix_stride, oess_stream_t stream);
/* affine-free InstanceNorm (+ReLU) backward; s1/s2 are [G x C] scratch */
/* The two-branch apply: out = act(x * scale + shift + bf16(x2 * scale2 + shift2)), G = 1.  x2 is the RAW result of a second
 * branch (a bottleneck's downsample conv) with its own scale / shift; it is normalised and rounded to bf16 in registers, so the
 * result carries the bits of oess_norm_apply_nhwc_bf16(x2 -> id) followed by oess_norm_apply_nhwc_bf16(x, residual = id) while
 * id is never written.  x may alias out.  C % 8 == 0, C <= 2048; pixel strides in elements, multiples of 8. */
int oess_norm_apply2_nhwc_bf16(const void* x, long long x_pix_stride, const float* scale, const float* shift, const void* x2,
                               long long x2_pix_stride, const float* scale2, const float* shift2, int relu, long long pixels, int C,
                               void* out, long long out_pix_stride, oess_stream_t stream);
int oess_instnorm_bwd_nhwc_bf16(const void* x, long long x_pix_stride, const void* dy, long long dy_pix_stride,
                                const float* mean, const float* rstd, int relu, int G, long long pixels_per_group, int C,
                                float* s1, float* s2, void* dx, long long dx_pix_stride, float* partials, size_t partials_bytes,
                                oess_stream_t stream);
/* nn.BatchNorm2d TRAIN-mode backward fused with the ReLU mask and the residual branch of a Bottleneck
 * (models/_resnet.py:96-114: out = relu(bn3(conv3) + identity)):  g = dy * (y_out > 0 if relu);  d(residual) = g;
 * dbeta[C] = sum g;  dgamma[C] = sum g * xhat;  dx = gamma * rstd * (g - dbeta/N - xhat * dgamma/N).
 * x = the BatchNorm input, y_out = the stored forward output (needed when relu != 0), mean / rstd = the batch statistics
 * of the forward (oess_norm_stats_finalize_nhwc_bf16).  dresidual nullable.  Replaces MIOpenBatchNormBwdSpatial* + the ATen ReLU / add
 * backward kernels on the trainable DeepLabv3 path. */
int oess_batchnorm_bwd_nhwc_bf16(const void* x, long long x_pix_stride, const void* dy, long long dy_pix_stride, const void* y_out,
                                 long long y_pix_stride, const float* mean, const float* rstd, const float* gamma, int relu,
                                 long long pixels, int C, float* dbeta, float* dgamma, void* dx, long long dx_pix_stride,
                                 void* dresidual, long long dres_pix_stride, float* partials, size_t partials_bytes,
                                 oess_stream_t stream);
int oess_upsample_nearest2x_nhwc_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int C, void* out,
                                      long long out_pix_stride, oess_stream_t stream);
/* z[b, s*y, s*x, :] = in[b, y, x, :], zero elsewhere on an Hz x Wz grid: turns the data gradient of a stride-s convolution
 * into the stride-1 product dX = conv(z, oess_conv2d_pack_weight(flip_for_dgrad = 1), pad = dil*(R-1) - pad) with
 * Hz = H_in - dil*(R-1) + 2*pad (replaces aten::convolution_backward for the stride-2 3x3 / 1x1 convolutions of
 * models/_resnet.py:74-114; MIOpen resolved those to a naive 9.4 ms kernel on gfx950). */
int oess_zero_insert_nhwc_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int C, int stride, int Hz, int Wz,
                               void* out, long long out_pix_stride, oess_stream_t stream);
int oess_downsample_sum2x_nhwc_bf16(const void* gout, long long gout_pix_stride, int B, int H, int W, int C, void* gin,
                                    long long gin_pix_stride, oess_stream_t stream);
/* The front half of the E2VID UpsampleConvLayer (e2vid/model/submodules.py:65-93) behind a skip sum, in one pass:
 * out[b, oy, ox, c] = bf16( bilinear2x( f32(x) + f32(skip) ) ), bilinear2x = F.interpolate(scale_factor=2, mode='bilinear',
 * align_corners=False): source coordinate max(0, (o + 0.5) / 2 - 0.5), taps floor and min(floor + 1, n - 1).  Sum and
 * interpolation in fp32, ONE rounding (to nearest even) at the store.  x, skip: [B, H, W, C]; out: [B, 2H, 2W, C]; NHWC bf16,
 * pixel strides in elements (channel slices of wider buffers are fine).  skip nullable (no sum).
 * OESS_EINVAL, nothing launched: C % 8 != 0, a non-positive size, a pixel stride smaller than C or no multiple of 8, a null x or
 * out, an out whose byte range overlaps an input's. */
int oess_upsample_bilinear2x_sum_nhwc_bf16(const void* x, long long x_pix_stride, const void* skip, long long skip_pix_stride, int B,
                                           int H, int W, int C, void* out, long long out_pix_stride, oess_stream_t stream);
/* nn.Upsample(scale, bilinear, align_corners=True) + F.normalize(dim=1) in one pass (models/image_model.py:121-143).  inv_norm
 * (nullable, needs normalize != 0): [B * H*scale * W*scale] fp32, 1 / max(|x|, 1e-12) of every output pixel -- what
 * oess_l2norm_nhwc_bwd needs, so the differentiable head never materialises the un-normalised full-resolution tensor. */
int oess_bilinear_l2norm_nhwc_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int C, int scale,
                                   int normalize, void* out, long long out_pix_stride, float* inv_norm, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bilinear resampling (any size, both align_corners modes) and channel L2 normalisation, forward + adjoint.
 * Replace F.interpolate(size=input_shape, mode='bilinear', align_corners=False) on DeepLabv3's logits and features
 * (models/deeplabv3.py:179-189) and nn.Upsample(x4, bilinear, align_corners=True) + F.normalize(p=2, dim=1) of the
 * teacher (models/image_model.py:121-143) including their autograd backward.  NHWC, pixel strides in elements,
 * bf16 (is_bf16 != 0) or fp32 (same dtype in and out).  The backward is a two-pass deterministic gather; workspace =
 * oess_resize_bilinear_bwd_workspace_bytes(B, W, C, Ho) bytes (fp32 [B, Ho, W, C]).
 * inv_norm: fp32 [P] = 1 / max(|x|, eps) per pixel, written by the forward (nullable) and read by the backward.
 * ------------------------------------------------------------------------------------------ */
int oess_resize_bilinear_nhwc_fwd(const void* in, long long in_pix_stride, int B, int H, int W, int C, int is_bf16, int Ho, int Wo,
                                  int align_corners, void* out, long long out_pix_stride, oess_stream_t stream);
size_t oess_resize_bilinear_bwd_workspace_bytes(int B, int W, int C, int Ho);
int oess_resize_bilinear_nhwc_bwd(const void* grad_out, long long gout_pix_stride, int B, int H, int W, int C, int is_bf16, int Ho,
                                  int Wo, int align_corners, void* workspace, size_t workspace_bytes, void* grad_in,
                                  long long gin_pix_stride, oess_stream_t stream);
int oess_l2norm_nhwc_fwd(const void* x, long long x_pix_stride, int64_t P, int C, int is_bf16, float eps, void* y,
                         long long y_pix_stride, float* inv_norm, oess_stream_t stream);
int oess_l2norm_nhwc_bwd(const void* y, long long y_pix_stride, const void* grad_y, long long gy_pix_stride, const float* inv_norm,
                         int64_t P, int C, int is_bf16, float eps, void* grad_x, long long gx_pix_stride, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Class labels from logits without the full-resolution tensor (K31): out[b, y, x] = argmax_k up(logits)[b, k, y, x], the
 * labels of F.interpolate(logits, size=(H, W), mode='bilinear', align_corners).argmax(1) (the online MaskCLIP teacher) and of
 * logits.argmax(dim=1) (if_switchable_train, training/pretrain_trainer.py:513-514, :556-557).
 *   logits: NHWC [B x h x w x K] fp32 or bf16 (is_bf16 != 0), pixel stride in elements (a channel slice of a wider buffer is fine);
 *   out: int64 [B x H x W], dense.  1 <= K <= 256.
 *   (H, W) == (h, w): no interpolation, the K raw values are compared.  Otherwise every class value is the fp32 blend of
 *   oess_resize_bilinear_nhwc_fwd's general kernel -- same index rule, bf16 taps widened first, same association, no FMA --, so the
 *   labels equal those of the composed path bit for bit.
 *   Argmax rule = torch.argmax: the first index among equal maxima; a NaN is larger than everything; the first NaN wins.
 * OESS_EINVAL, nothing launched, out untouched: a null pointer, K outside 1 ... 256, a non-positive size, pix_stride < K, B * H or
 * B * h above 2^31 - 1, or an element count of logits / out that overflows 64-bit byte offsets.  No geometry is refused for size:
 * source rows that do not fit the kernel's LDS budget are read from global memory. */
int oess_argmax_labels(const void* logits, int is_bf16, long long pix_stride, int B, int K, int h, int w, int H, int W,
                       int align_corners, int64_t* out, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Segmentation maps from logits without the full-resolution tensor (K35, the inference path): per output pixel the class label,
 * the softmax probability of that class and a colour.
 *   logits, pix_stride, B, K, h, w, H, W, align_corners: as oess_argmax_labels; the class values v_k are that entry's values (raw
 *     at the input size, otherwise the fp32 blend in its association) and the label is its label.  1 <= K <= 255.
 *   conf  (fp32 [B x H x W] or null): 1 / sum_k exp(v_k - v_max) in fp32, one walk over K (running maximum and sum).
 *   labels (u8 [B x H x W] or null): the label, or ignore_label where conf < min_conf (false for a NaN conf; min_conf = 0 ignores
 *     nothing).  K <= ignore_label <= 255: it is not a class.
 *   rgb   (u8 [B x H x W x 3] or null): c = palette[label] (palette: u8 [K x 3] on the device), (0, 0, 0) for ignore_label;
 *     with grey (u8 [B x H x W] or null) every channel is (alpha256 * c + (256 - alpha256) * grey + 128) >> 8, 0 <= alpha256 <= 256.
 *   An output that is null is not computed; two calls give the same bits (one lane owns a pixel, no atomics).
 * OESS_EINVAL, nothing launched, outputs untouched: logits null, all three outputs null, rgb without palette, K outside 1 ... 255,
 * ignore_label outside K ... 255, alpha256 outside 0 ... 256, a NaN or negative min_conf, a non-positive size, pix_stride < K,
 * B * H or B * h above 2^31 - 1, or an element count that overflows 64-bit byte offsets. */
int oess_segment_render(const void* logits, int is_bf16, long long pix_stride, int B, int K, int h, int w, int H, int W,
                        int align_corners, const uint8_t* palette, const uint8_t* grey, int alpha256, float min_conf,
                        int ignore_label, uint8_t* labels, float* conf, uint8_t* rgb, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Open-vocabulary rendering (K36): K classes over a vocabulary of P >= K names; class k owns the contiguous channels
 * class_offsets[k] ... class_offsets[k + 1] - 1 (int32 [K + 1] on the device: 0 first, strictly increasing, P last -- the caller's
 * part; the kernels clamp every entry to 0 ... P, so a wrong list gives wrong classes and no read outside the P channels).
 * The class value c_k is torch.amax over the group's name values (a NaN member makes it NaN); label, conf, threshold and rgb are
 * oess_segment_render's over the K class values.  1 <= K <= 255, K <= P <= 1024.
 *   oess_segment_render_grouped: name values = oess_segment_render's values of the P-channel logits.  Singleton groups give
 *     oess_segment_render's bits.  OESS_EINVAL as oess_segment_render, and for null class_offsets, P outside K ... 1024 and
 *     pix_stride < P.
 *   oess_head_render: name values from the map in front of a linear head, without any [B x P x H x W] tensor:
 *     v_p = fmaf(w[p][C-1], x[C-1], ... fmaf(w[p][0], x[0], bias_p) ...), ascending c from the bias (0 when bias is null), bf16 taps
 *     widened first.  x: NHWC [B x H x W x C] fp32 or bf16 with a pixel stride, 1 <= C <= 64; weight fp32 [P x C], bias fp32 [P] or
 *     null, both dense on the device.  class_offsets null: one name per class (P == K).  The weights and the bias sit in LDS:
 *     OESS_EINVAL as well when P > oess_head_render_max_names(C) = 48 KB / (4 (C + 1)), and for pix_stride < C.
 * Adding these entries left OESS_ABI_VERSION unchanged. */
int oess_segment_render_grouped(const void* logits, int is_bf16, long long pix_stride, int B, int K, int P, int h, int w, int H, int W,
                                int align_corners, const int32_t* class_offsets, const uint8_t* palette, const uint8_t* grey,
                                int alpha256, float min_conf, int ignore_label, uint8_t* labels, float* conf, uint8_t* rgb,
                                oess_stream_t stream);
size_t oess_head_render_max_names(int C);
int oess_head_render(const void* x, int is_bf16, long long pix_stride, int B, int C, int H, int W, const float* weight,
                     const float* bias, int K, int P, const int32_t* class_offsets, const uint8_t* palette, const uint8_t* grey,
                     int alpha256, float min_conf, int ignore_label, uint8_t* labels, float* conf, uint8_t* rgb,
                     oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Flip and multi-scale inference (K39): oess_segment_render's outputs from the MEAN class probability of V logit maps of the same
 * B and K, without any full-resolution [B x K x H x W] tensor.  1 <= V <= OESS_RENDER_MAX_VIEWS.
 *   logits, pix_strides, hs, ws, flips: HOST arrays of V entries (copied into the kernel's arguments, nothing is uploaded); view v
 *     is NHWC [B x hs[v] x ws[v] x K] on the device, fp32 or bf16 (is_bf16, one type for all views), with its pixel stride.
 *   Class values of view v at output pixel (oy, ox): oess_segment_render's values at (oy, ox'), ox' = flips[v] ? W - 1 - ox : ox
 *     (raw at the output size, otherwise the fp32 blend): a flipped view is the view rendered as given and then mirrored.
 *   q_vk = exp(v_vk - m_v) / S_v (m_v the view's maximum, S_v = sum_k exp(v_vk - m_v), fp32), p_k = (sum_v q_vk) * (1.0f / V) in
 *     ascending v.  The label is torch.argmax's over p_k (first index among equal maxima, a NaN above everything), conf = p_label;
 *     threshold, ignore_label, palette, grey and the integer blend are oess_segment_render's.
 *   A view with a NaN, a +inf or only -inf at a pixel makes every p_k NaN there: label 0, NaN conf (which keeps its label).
 *   One lane owns a pixel, no atomics: two calls give the same bits.
 * OESS_EINVAL, nothing launched, outputs untouched: a null array or view pointer, V outside 1 ... 8, a flip other than 0 / 1, a
 * non-positive size, a stride below K, what oess_segment_render refuses of the shared arguments, B * H or B * hs[v] above
 * 2^31 - 1, or an element count that overflows 64-bit byte offsets.  Adding this entry left OESS_ABI_VERSION unchanged. */
#define OESS_RENDER_MAX_VIEWS 8
int oess_segment_render_ensemble(const void* const* logits, const long long* pix_strides, const int* hs, const int* ws,
                                 const int* flips, int V, int is_bf16, int B, int K, int H, int W, int align_corners,
                                 const uint8_t* palette, const uint8_t* grey, int alpha256, float min_conf, int ignore_label,
                                 uint8_t* labels, float* conf, uint8_t* rgb, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MaskCLIP ViT-B/16 image tower (models/maskclip_model.py:448-541 TransformerEncoderLayer, :545-851 VisionTransformer):
 * the non-GEMM pieces.  The linear layers (patch embedding, in_proj, out_proj, FFN, proj) run on oess_conv2d_fwd_bf16 as
 * 1x1 / 16x16 convolutions over the token axis (bias, residual and GELU fused in the epilogue).
 *   oess_layernorm_bf16: y = (x - mean) * rsqrt(var + eps) * gamma + beta over C channels of each of `rows` tokens
 *     (nn.LayerNorm, eps 1e-6 in the ViT; build_norm_layer(dict(type='LN', eps=1e-6)) :486-501,:706-718).
 *   oess_attention_d64_bf16: softmax(Q K^T * scale) V for head dimension 64; qkv = nn.MultiheadAttention's packed
 *     in_proj output [B, L, 3 * heads * 64] (q | k | v), out = [B, L, heads * 64] before out_proj
 *     (mmcv MultiheadAttention -> nn.MultiheadAttention.forward, :496-497,:538).
 * Row strides in elements (multiples of 8), pointers 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int oess_layernorm_bf16(const void* x, long long x_row_stride, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                        void* y, long long y_row_stride, oess_stream_t stream);
int oess_attention_d64_bf16(const void* qkv, long long qkv_row_stride, int B, int L, int heads, float scale, void* out,
                            long long out_row_stride, oess_stream_t stream);

/* Weight gradient of oess_conv2d_fwd_bf16's convolution: dW (OIHW fp32, every element WRITTEN: no pre-zeroing)
 * from x (NHWC bf16, Cin_x >= Cin channels present, Cin_x % 8 == 0) and dy (NHWC bf16, Cout % 8 == 0).
 * Replaces the weight half of ATen's convolution_backward behind nn.Conv2d (models/style_networks.py:252-289). */
int oess_conv2d_wgrad_bf16(const void* x, long long x_pix_stride, int B, int H, int W, int Cin_x, const void* dy,
                           long long dy_pix_stride, int Cout, int Cin, int R, int S, int stride, int pad, int dil,
                           float* dw_oihw, void* workspace, size_t workspace_bytes, oess_stream_t stream);
/* workspace: split-K partial tiles; any size >= one padded tile set works (a smaller one is OESS_ENOMEM), 64 MiB lets the
 * kernel use full parallelism.  Nothing beyond workspace_bytes is touched, and what the workspace held before does not matter:
 * every partial that is read was stored by this call. */
/* Which kernel a call takes.  oess_conv2d_wgrad_bf16 is one entry point over the eight gradient kernels below and two reduce
 * kernels; the choice depends on the geometry, on the byte extent of both tensors (pixel strides included) and on the workspace
 * on offer.  oess_conv2d_wgrad_route makes the plan the launch itself executes (wgrad_plan, conv_wgrad.hip) and returns
 * kernel | slices << 8 instead of launching: slices = partial tiles summed per element (>= 16: wgrad_reduce_wide_kernel,
 * fewer: wgrad_reduce_kernel).  Negative = the OESS_E* the launch returns for these numbers (the launch also refuses null
 * pointers).  Host only: no launch, no allocation, no runtime call, no device query. */
#define OESS_WGRAD_REG_32 1            /* conv_wgrad_kernel<32>: register-staged, a tensor's byte extent reaches 2 GiB       */
#define OESS_WGRAD_REG_64 2            /* conv_wgrad_kernel<64>                                                            */
#define OESS_WGRAD_REG_128 3           /* conv_wgrad_kernel<128>                                                           */
#define OESS_WGRAD_DMA_32 4            /* conv_wgrad_dma_kernel<32>: LDS-DMA, the general case (Cout <= 32)                */
#define OESS_WGRAD_DMA_64 5            /* conv_wgrad_dma_kernel<64>: Cout <= 64                                            */
#define OESS_WGRAD_DMA_128 6           /* conv_wgrad_dma_kernel<128>                                                       */
#define OESS_WGRAD_STRIP_32 7          /* conv_wgrad_strip_kernel<32>: narrow full-resolution 3x3 'same' layers            */
#define OESS_WGRAD_STRIP_64 8          /* conv_wgrad_strip_kernel<64>                                                      */
#define OESS_WGRAD_KERNEL(route) ((route) & 0xff)
#define OESS_WGRAD_SLICES(route) ((route) >> 8)
int oess_conv2d_wgrad_route(int B, int H, int W, int Cin_x, int Cout, int Cin, int R, int S, int stride, int pad, int dil,
                            long long x_pix_stride, long long dy_pix_stride, size_t workspace_bytes);

/* ------------------------------------------------------------------------------------------
 * GPU-side decode of 8-bit single-channel PNG maps: pseudo-labels, superpixel ids, ground-truth labels.
 * Replaces np.array(Image.open(path)) + torch.tensor(...).long() [+ torch.flip(..., [1])] of
 * DSEC/dataset/sequence_ov.py:340-358,366-372 and datasets/ddd17_events_loader.py:228-262 for a whole batch:
 *   files    the n_images PNG files back to back (bytes as read from disk), offsets[n_images + 1] their byte offsets (device),
 *            total_file_bytes = offsets[n_images] (host copy: sizes the scratch check)
 *   flip     optional uint8[n_images]: 1 = mirror the map horizontally (the loader's flip augmentation)
 *   out      int64 [n_images][H][W] (the dtype the trainers index with)
 *   scratch  oess_png_decode_scratch_bytes(total bytes, n_images, H, W); scratch_offsets[n_images] (device): byte offset of image
 *            i's region = sum over j < i of (align16(len_j) + H * (W + 1) + 16)
 *   status   int[n_images]: 0 = decoded; otherwise the map is filled with 255 (ignore index) and the code says why
 *            (1 signature, 2 IHDR, 3 not 8-bit grey / palette or interlaced, 4 zlib header, 5 block, 6 code, 7 overrun,
 *            8 size mismatch, 9 filter).  Supported: colour type 0 or 3 (indices), bit depth 8, no interlace, any IDAT split,
 *            stored / fixed / dynamic DEFLATE blocks, all five PNG filters.  Exact (integer work): equals PIL's array.
 * ------------------------------------------------------------------------------------------ */
size_t oess_png_decode_scratch_bytes(long long total_file_bytes, int n_images, int H, int W);
int oess_png_decode_gray8_batch(const uint8_t* files, const int64_t* offsets, long long total_file_bytes, int n_images, int H, int W,
                                const uint8_t* flip, int64_t* out, void* scratch, size_t scratch_bytes, const int64_t* scratch_offsets,
                                int* status, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * GPU-side encode of 8-bit grey / RGB maps into PNG files: oess_segment_render's `labels` and `rgb`, SLIC's
 * superpixel ids.  Replaces Image.fromarray(map).save(path) for a whole batch; the host writes the returned bytes as they are.
 *   images   contiguous u8 [n_images][H][W] (channels = 1) or [n_images][H][W][3] (channels = 3)
 *   files    [n_images][slot_bytes]; image i's file is files[i][0 ... sizes[i]); the bytes of a slot beyond that are
 *            unspecified; nothing outside the n slots and sizes[n_images] is written
 *   scratch  oess_png_encode_scratch_bytes(n_images, H, W, channels) bytes, 16-byte aligned
 * The format is a fixed subset of PNG, so that the bytes are the same from any implementation of this text:
 *   signature; IHDR (W, H, bit depth 8, colour type 0 or 2, no interlace); an IDAT holding 78 01; one IDAT per segment; an IDAT
 *   holding the Adler-32 of the filtered stream; IEND.  Every scanline has filter type 4 (Paeth, ties in the order a, b, c,
 *   pixels outside the image 0).  The filtered stream of S = H (1 + W channels) bytes is cut into segments of
 *   OESS_PNG_ENCODE_SEGMENT bytes (the last one shorter); each is one DEFLATE block that starts on a byte, BFINAL on the last.
 *   Coded form (BTYPE 01, the fixed Huffman code): runs of equal bytes are found inside the segment only; a run of L bytes is
 *   one literal, then matches at distance 1 over the other L - 1 bytes, each as long as fits (at most 258) while at least 3
 *   remain, then the 0 ... 2 bytes left as literals; then end-of-block; a segment that is not the last is closed by an empty
 *   stored block (000, zero bits to the byte, 00 00 FF FF), the last one is padded to the byte with zero bits.
 *   Stored form (BTYPE 00: the header byte, LEN, NLEN, the bytes): used exactly when the coded form with its closing bytes would
 *   not be shorter than 5 + the segment's length.
 * So a file is at most oess_png_encode_bound = 75 + S + 17 ceil(S / OESS_PNG_ENCODE_SEGMENT) bytes (host only; 0 for a size the
 * encoder refuses).  The bytes depend on the input alone: two calls give the same files.
 * OESS_EINVAL before any HIP call, outputs untouched: a null pointer, n_images < 1, channels not 1 or 3, H or W outside
 * 1 ... 16384, slot_bytes below the bound, scratch_bytes below the query, scratch off 16 bytes, n_images times the segments of
 * an image above 2^31 - 1 (the scratch query answers 0 there).  Adding these entries left OESS_ABI_VERSION unchanged.
 * ------------------------------------------------------------------------------------------ */
#define OESS_PNG_ENCODE_SEGMENT 16384
long long oess_png_encode_bound(int H, int W, int channels);
size_t oess_png_encode_scratch_bytes(int n_images, int H, int W, int channels);
int oess_png_encode_batch(const uint8_t* images, int n_images, int H, int W, int channels, uint8_t* files, long long slot_bytes,
                          int* sizes, void* scratch, size_t scratch_bytes, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Linear probe: nn.Conv2d(K, K, 1) on the fp32 logits (models/style_networks.py:113-133,169-170; models/deeplabv3.py:162-170,
 * 186-187), K <= 32.  x, y, grad_*: dense NHWC fp32 [P x K]; w: [K x K] (Conv2d.weight viewed [out, in]); bias nullable in the
 * forward.  Backward: grad_x nullable (frozen producer); grad_w / grad_bias from per-workgroup double partial rows added in a fixed order (bit-repeatable);
 * partials: oess_linear_probe_partials_bytes(K) bytes of caller scratch.
 * ------------------------------------------------------------------------------------------ */
size_t oess_linear_probe_partials_bytes(int K);
int oess_linear_probe_fwd_f32(const float* x, const float* w, const float* bias, long long P, int K, float* y, oess_stream_t stream);
int oess_linear_probe_bwd_f32(const float* x, const float* grad_y, const float* w, long long P, int K, float* grad_x, float* grad_w,
                              float* grad_bias, void* partials, size_t partials_bytes, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backward of k = scatter_mean(F.normalize(nn.Upsample(bilinear)(x)), superpixels) as one node (models/image_model.py:121-143 +
 * training/pretrain_trainer.py:445-465): feat = the saved normalised full-resolution map [B x Ho x Wo x C] bf16, inv_norm its
 * 1 / max(|x|, eps) per pixel (both from oess_bilinear_l2norm_nhwc_bf16), ids raw superpixel ids [B*Ho*Wo], grad_k [S x C] fp32,
 * count [S] (oess_segment_mean_fwd).  grad_in: [B x H x W x C] bf16.  C in {64, 128, 256, 512}.  Deterministic (gather form).
 * ------------------------------------------------------------------------------------------ */
size_t oess_bilinear_l2norm_pool_bwd_workspace_bytes(int B, int W, int C, int Ho, int S);
int oess_bilinear_l2norm_pool_bwd_bf16(const void* feat, long long feat_pix_stride, const float* inv_norm, const int64_t* ids,
                                       const float* grad_k, const float* count, int superpixel_size, int S, int B, int H, int W, int C,
                                       int Ho, int Wo, int align_corners, float eps, void* workspace, size_t workspace_bytes,
                                       void* grad_in, long long gin_pix_stride, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The same node in fp32 WITHOUT a full-resolution tensor (K20): forward and backward recompute the four-corner blend of every
 * output pixel from x, the head's fp32 NHWC conv output [B x H x W x C] (pixel stride x_pix_stride, 16-byte aligned rows),
 * C in {64, 128, 256}, any integer scale >= 1, both align_corners modes, Ho = H * scale, Wo = W * scale.
 *   fwd: k [S x C] and count [S] fp32 = scatter_mean(normalize(upsample(x)), ids + sample * superpixel_size); partial sums meet as
 *        the 2^-32 fixed-point integers of oess_segment_mean_fwd (same workspace: oess_segment_mean_fwd_workspace_bytes(S, C) bytes,
 *        same range / finiteness contract: a non-finite input makes the whole of k NaN); bit-repeatable.
 *   bwd: grad_x [B x H x W x C] fp32 from grad_k [S x C] and count; workspace =
 *        oess_bilinear_l2norm_pool_bwd_workspace_bytes(B, W, C, Ho, S) bytes.  Deterministic (gather form, no atomics).
 * The index rule and eps (1 / max(|u|, eps)) are those of oess_resize_bilinear_nhwc_fwd / oess_l2norm_nhwc_fwd; only the
 * association of the blend differs (rows first, then columns).
 * ------------------------------------------------------------------------------------------ */
int oess_bilinear_l2norm_pool_fwd_f32(const float* x, long long x_pix_stride, const int64_t* ids, int superpixel_size, int S, int B, int H,
                                      int W, int C, int scale, int align_corners, float eps, float* k, float* count, void* workspace,
                                      size_t workspace_bytes, oess_stream_t stream);
int oess_bilinear_l2norm_pool_bwd_f32(const float* x, long long x_pix_stride, const int64_t* ids, const float* grad_k, const float* count,
                                      int superpixel_size, int S, int B, int H, int W, int C, int scale, int align_corners, float eps,
                                      void* workspace, size_t workspace_bytes, float* grad_x, long long gx_pix_stride,
                                      oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * L1 consistency of two bilinearly upsampled fp32 maps WITHOUT a full-resolution tensor (K23; training/openess_trainer.py:497 on
 * the two `feats` of models/deeplabv3.py:184):  loss = mean over B C Ho Wo of |up(a - b)|, a / b [B x h x w x C] fp32 NHWC with
 * pixel strides >= C (elements), b == NULL: d = a.  `up` is the index rule of oess_resize_bilinear_nhwc_fwd, blended rows first.
 *   fwd: workspace = oess_upsampled_l1_workspace_bytes(...) bytes, 8-byte aligned (one double per workgroup, summed in a fixed order
 *        by one block); loss: device scalar.
 *   bwd: grad_a = grad_out / N * up^T(sign(up(d))), sign(0) = 0, grad_b = -grad_a; either may be NULL (grad_b needs b).
 *        Gather form, no atomics: bit-repeatable.
 * Accepted: C % 4 == 0, C <= 1024, Ho >= h, Wo >= w, both align_corners modes, h or w of 1; anything else is OESS_EINVAL.
 * ------------------------------------------------------------------------------------------ */
size_t oess_upsampled_l1_workspace_bytes(int B, int h, int w, int C, int Ho, int Wo);
int oess_upsampled_l1_fwd_f32(const float* a, long long a_pix_stride, const float* b, long long b_pix_stride, int B, int h, int w, int C,
                              int Ho, int Wo, int align_corners, void* workspace, size_t workspace_bytes, float* loss,
                              oess_stream_t stream);
int oess_upsampled_l1_bwd_f32(const float* a, long long a_pix_stride, const float* b, long long b_pix_stride, int B, int h, int w, int C,
                              int Ho, int Wo, int align_corners, const float* grad_out, float* grad_a, long long ga_pix_stride,
                              float* grad_b, long long gb_pix_stride, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Cosine distance of two bilinearly resampled maps on a common output grid WITHOUT a full-resolution tensor (K34; the SAM
 * distillation loss of training/pretrain_trainer.py:519-529):  loss = mean over B Ho Wo of (1 - cos_p),
 *   cos_p = a_p . t_p / (max(|a_p|, eps) max(|t_p|, eps))                       (the rule of oess_cosine_mean_*)
 *   a: student map [B x h x w x C] NHWC, fp32 or bf16 (a_is_bf16), pixel stride >= C (elements), upsampled to Ho x Wo by the index
 *      rule and blend of oess_resize_bilinear_nhwc_fwd, either align_corners mode.
 *   t: teacher map [B x ht x wt x C] NHWC fp32, pixel stride >= C, resized to a VIRTUAL Mh x Mw grid (align_corners = 0, two taps, no
 *      antialiasing: ht, wt may be larger or smaller than Mh, Mw) of which only the top-left Ho x Wo is read.
 *   fwd: workspace = oess_upsampled_cosine_workspace_bytes(...) bytes, 8-byte aligned (one double per workgroup, summed in a fixed
 *        order by one block); loss: device scalar; planes: NULL, or oess_upsampled_cosine_planes_floats(B, Ho, Wo) floats that
 *        receive two scalars per output pixel for the backward.
 *   bwd: grad_a only (the teacher is data), [B x h x w x C] in a's dtype, pixel stride >= C; reads the forward's planes and
 *        recomputes both interpolated vectors.  Gather form, no atomics: bit-repeatable.  Below the clamp (|a_p| <= eps) the norm
 *        carries no gradient, as in oess_cosine_mean_bwd.
 * Accepted: C % 4 == 0, C <= 1024, Ho >= h, Wo >= w, ht, wt >= 1, Mh >= Ho, Mw >= Wo, h or w of 1.  Anything else -- null pointers,
 * strides below C, non-positive sizes, a workspace that is too small or misaligned -- is OESS_EINVAL before anything is launched.
 * ------------------------------------------------------------------------------------------ */
size_t oess_upsampled_cosine_workspace_bytes(int B, int h, int w, int C, int Ho, int Wo);   /* 0: geometry not accepted */
size_t oess_upsampled_cosine_planes_floats(int B, int Ho, int Wo);
int oess_upsampled_cosine_fwd(const void* a, int a_is_bf16, long long a_pix_stride, const float* t, long long t_pix_stride, int B, int h,
                              int w, int C, int Ho, int Wo, int align_corners, int ht, int wt, int Mh, int Mw, float eps, void* workspace,
                              size_t workspace_bytes, float* planes, float* loss, oess_stream_t stream);
int oess_upsampled_cosine_bwd(const void* a, int a_is_bf16, long long a_pix_stride, const float* t, long long t_pix_stride, int B, int h,
                              int w, int C, int Ho, int Wo, int align_corners, int ht, int wt, int Mh, int Mw, const float* planes,
                              const float* grad_out, void* grad_a, long long ga_pix_stride, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Superpixel mean of a bilinearly upsampled map through its pooling matrix (models/deeplabv3.py:184 F.interpolate(feats, size=
 * input, bilinear, align_corners=False) followed by training/pretrain_trainer.py:445-465 on it): k[s] = (sum_q M[s][q] y[q]) /
 * (n[s] + 1e-6) with M[s][q] = the summed bilinear weights of superpixel row s's pixels on low-resolution pixel q.
 *   build: ids [B x Ho x Wo] raw ids (row = id + sample * superpixel_size, rows outside [0, S) dropped) -> matrix
 *          (oess_pool_matrix_bytes(S, B, h, w) bytes, 16-byte aligned; 2^-40 fixed-point sums + pixel counts; order-independent)
 *   fwd:   y [B x h x w x C] bf16 / fp32 -> k [S x C] fp32, count [S] fp32
 *   bwd:   grad_k [S x C] -> grad_y [B x h x w x C];  C <= 1024.  The full-resolution map is never formed.
 * ------------------------------------------------------------------------------------------ */
size_t oess_pool_matrix_bytes(int S, int B, int h, int w);
int oess_pool_matrix_build(const int64_t* ids, int B, int Ho, int Wo, int h, int w, int align_corners, int superpixel_size, int S,
                           void* matrix, size_t matrix_bytes, oess_stream_t stream);
int oess_pool_matrix_fwd(const void* matrix, const void* y, long long y_pix_stride, int is_bf16, int B, int h, int w, int C, int S,
                         float* k, float* count, oess_stream_t stream);
int oess_pool_matrix_bwd(const void* matrix, const float* grad_k, int B, int h, int w, int C, int S, void* grad_y, long long gy_pix_stride,
                         int is_bf16, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Small ops of the DeepLabv3 training path (round 5; they replace the last ATen / MIOpen / hipBLASLt launches of that path).
 *
 * MaxPool2d(kernel 3, stride 2, padding 1) of the ResNet stem (models/_resnet.py:124, 197 of the reference) on NHWC bf16:
 *   out [B x Ho x Wo x C], Ho = (H - 1) / 2 + 1; idx (nullable): [B x Ho x Wo x C] bytes, winning tap 0..8 (row-major, ATen's tie
 *   rule: first maximum, NaN wins); backward: grad_in [B x H x W x C] written once per element (gather form, deterministic).
 * Dropout (models/deeplabv3.py:343 nn.Dropout(0.1)): y = x * keep / (1 - p), keep from Philox-4x32-10 keyed by (seed, offset,
 *   element); the backward pass is the same call on the gradient with the same (seed, offset).  x == y allowed.
 * ASPP image-pooling branch (models/deeplabv3.py:305-316): in_scale * pooled [B x Cin] fp32 (AdaptiveAvgPool2d(1): per-sample
 *   channel sums and in_scale = 1 / (H W)) -> 1x1 conv w [Cout x Cin] -> BatchNorm2d in train mode over the B samples (running
 *   stats updated, unbiased variance) -> ReLU = z [B x Cout] (+ a bf16 copy, nullable); y_pre [B x Cout] and stat [2 x Cout] = {mean, rstd} are kept for
 *   the backward; 2 <= B <= 16.  Backward: grad_z [B x Cout] -> grad_w [Cout x Cin], grad_gamma / grad_beta [Cout], and the
 *   gradient of the per-sample sums as bf16 [B x Cin] (nullable: frozen producer); dy_scratch [B x Cout] floats.
 * ------------------------------------------------------------------------------------------ */
int oess_maxpool3x3s2_fwd_nhwc_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int C, void* out, long long out_pix_stride,
                                    unsigned char* idx, oess_stream_t stream);
/* oess_maxpool3x3s2_fwd_nhwc_bf16 over a RAW map in front of a BatchNorm + ReLU: every tap is bf16(relu(x * scale + shift)) before
 * the comparison (any sign of scale), out-of-range taps are skipped.  The bits of oess_norm_apply_nhwc_bf16(relu = 1) followed by
 * the plain pool; the normalised map is never written.  Forward only, no winner index (the no-autograd path). */
int oess_maxpool3x3s2_affine_relu_fwd_nhwc_bf16(const void* in, long long in_pix_stride, int B, int H, int W, int C, const float* scale,
                                                const float* shift, void* out, long long out_pix_stride, oess_stream_t stream);
int oess_maxpool3x3s2_bwd_nhwc_bf16(const void* grad_out, long long go_pix_stride, const unsigned char* idx, int B, int H, int W, int C,
                                    void* grad_in, long long gi_pix_stride, oess_stream_t stream);
int oess_dropout_nhwc_bf16(const void* x, long long x_pix_stride, void* y, long long y_pix_stride, long long P, int C, float p,
                           unsigned long long seed, unsigned long long offset, oess_stream_t stream);
int oess_aspp_pool_fwd_f32(const float* pooled, float in_scale, const float* w, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, float momentum, float eps, int B, int Cin, int Cout, float* y_pre, float* stat, float* z,
                           void* z_bf16, oess_stream_t stream);
int oess_aspp_pool_bwd_f32(const float* grad_z, const float* pooled, float in_scale, const float* w, const float* gamma, const float* y_pre,
                           const float* stat, const float* z, int B, int Cin, int Cout, float* dy_scratch, float* grad_w,
                           float* grad_gamma, float* grad_beta, void* grad_pooled_bf16, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * E2VID post-processing: the reference's PostProcessor.process (e2vid/image_reconstructor.py:126-140) on the reconstructed frame,
 * UnsharpMaskFilter (e2vid/utils/inference_utils.py:234-252) then IntensityRescaler (:90-129), fused (bilateral filter: no).
 *   img: fp32 [N x 1 x H x W] VIEW, last dimension contiguous, image stride img_stride and row stride row_stride in elements (a crop
 *   window of a larger map is fine: the blur's zero padding sits at the edge of the view).  weights_host: the 25 fp32 weights of
 *   gkern(5, sigma), row-major, read on the host; may be NULL when amount <= 0 (the filter is then skipped, as in the reference).
 *   out_u8 [N x H x W]: trunc(clamp(255 (s - Imin) / (Imax - Imin), 0, 255)); out_f32 (nullable) [N x 1 x H x W]: out_u8 / 255.
 * Fixed bounds: ONE launch; imax > imin required.
 * Auto-HDR: TWO launches, no host synchronisation: the whole-tensor min / max of the sharpened image (all N images together),
 *   clipped to [0, 0.45] / [0.55, 1], enter a window of up to filter_size + 1 entries whose float64 medians are Imin / Imax.
 *   state: caller-owned device buffer of oess_e2vid_postproc_state_bytes(filter_size) bytes, 8-byte aligned, zero-filled for a
 *   fresh window, then passed unchanged to every call of the sequence (same filter_size); it is stream-ordered like any output.
 *   Layout: 48-byte header, then ring_lo[filter_size + 1], ring_hi[filter_size + 1] (float64); the header holds the current
 *   medians as two float64 at byte offset 32 (Imin, Imax).
 * Bit-repeatable (no floating-point atomics).  0 <= filter_size <= OESS_E2VID_POSTPROC_MAX_FILTER.
 * ------------------------------------------------------------------------------------------ */
#define OESS_E2VID_POSTPROC_MAX_FILTER 255
size_t oess_e2vid_postproc_state_bytes(int filter_size);      /* 0 for a filter_size out of range */
int oess_e2vid_postprocess_f32(const float* img, long long img_stride, long long row_stride, int N, int H, int W,
                               const float* weights_host, double amount, double imin, double imax, uint8_t* out_u8, float* out_f32,
                               oess_stream_t stream);
int oess_e2vid_postprocess_auto_hdr_f32(const float* img, long long img_stride, long long row_stride, int N, int H, int W,
                                        const float* weights_host, double amount, int filter_size, void* state, size_t state_bytes,
                                        uint8_t* out_u8, float* out_f32, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K14 fp32 E2VID inference (offline reconstruction, run_reconstruction --precision fp32): the layers of UNetRecurrent
 * (e2vid/model/unet.py:118-170 of the reference) in fp32 on the f32-input MFMA (v_mfma_f32_32x32x2_f32): every output is a
 * k-ordered fmaf chain, written once (no atomics, bit-repeatable).
 *
 * oess_f32_view_t: an fp32 tensor addressed as data[b sb + y sy + x sx + c sc] (strides in ELEMENTS): NHWC, NCHW and channel /
 *   crop views of either.  An output view's data is written.  Dense, 16-byte aligned channels (sc == 1, the other strides
 *   multiples of 4) and Cin % 16 == 0 take the vector operand loads; anything else is read element by element.
 * oess_conv2d_fwd_f32: out = act(conv(in [+ in2]) + bias [+ residual]), act: 0 none, 1 ReLU, 2 sigmoid.  in2 (nullable, same
 *   shape as in) is summed on load (skip_sum); upsample2x == 1 convolves the bilinear x2 (align_corners=False) of in [+ in2],
 *   a (2H) x (2W) map (UpsampleConvLayer).  R x S <= 25 taps, stride 1 or 2, pad < R, S.  out: B x Ho x Wo x Cout,
 *   Ho = (H' + 2 pad - R) / stride + 1 with H' = H or 2H.
 *   w_packed: oess_conv2d_f32_packed_floats(Cout, Cin, R, S) floats, 16-byte aligned: [ceil16(R S Cin)][ceil32(Cout)], row
 *   (r S + s) Cin + ci, column co = weight[co][ci][r][s] (Conv2d OIHW), zeros in the padding.  bias: fp32 [Cout] or NULL.
 * oess_conv_transpose2d_fwd_f32: ConvTranspose2d(kernel 5, stride 2, padding 2, output_padding 1) of in [+ in2] -> out
 *   B x 2H x 2W x Cout, + bias, act; four stride-1 phase sub-convolutions in ONE launch.  w_packed: four blocks (phase
 *   p = 2 py + px, py / px = output row / column parity), each [ceil16(ny nx Cin)][ceil32(Cout)] with ny = 3 - py, nx = 3 - px,
 *   row (ty nx + tx) Cin + ci, column co = weight[ci][co][py + 2 ty][px + 2 tx] (ConvTranspose2d's [Cin][Cout][5][5]).
 * oess_convlstm_step_f32: ConvLSTM (e2vid/model/submodules.py:175-214): gates = conv(xh, w) + bias (R x S, "same" padding) into
 *   ws ([B H W][4 C_hidden], i f o g), then c = sigmoid(f) c + sigmoid(i) tanh(g) (prev_cell_is_zero: sigmoid(i) tanh(g)) in
 *   place in cell (fp32 [B][H][W][C_hidden], dense) and h = sigmoid(o) tanh(c) into the hidden view.  xh has Cin channels
 *   (cat(x, h) = 2 C_hidden, or x alone with the x-half weights when the previous state is zero); w_packed as for
 *   oess_conv2d_fwd_f32 with Cout = 4 C_hidden.  Two launches.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const float* data;
    long long sb, sy, sx, sc;
} oess_f32_view_t;
size_t oess_conv2d_f32_packed_floats(int Cout, int Cin, int R, int S);       /* 0 for an impossible geometry */
size_t oess_conv_transpose2d_f32_packed_floats(int Cout, int Cin);
size_t oess_convlstm_f32_workspace_bytes(long long pixels, int C_hidden);
int oess_conv2d_fwd_f32(const oess_f32_view_t* in, const oess_f32_view_t* in2, int B, int H, int W, int Cin, int upsample2x,
                        const float* w_packed, const float* bias, int Cout, int R, int S, int stride, int pad, int act,
                        const oess_f32_view_t* residual, const oess_f32_view_t* out, oess_stream_t stream);
int oess_conv_transpose2d_fwd_f32(const oess_f32_view_t* in, const oess_f32_view_t* in2, int B, int H, int W, int Cin,
                                  const float* w_packed, const float* bias, int Cout, int act, const oess_f32_view_t* out,
                                  oess_stream_t stream);
int oess_convlstm_step_f32(const oess_f32_view_t* xh, int B, int H, int W, int Cin, const float* w_packed, const float* bias,
                           int C_hidden, int R, int S, int pad, int prev_cell_is_zero, float* cell, const oess_f32_view_t* hidden,
                           void* ws, size_t ws_bytes, oess_stream_t stream);
/* K28: the fp32 ConvGRU step's pointwise halves (contract in the ConvGRU block above) */
size_t oess_convgru_f32_workspace_bytes(long long pixels, int C_hidden);     /* 0 for an impossible geometry */
int oess_convgru_gates_f32(const float* pre, const oess_f32_view_t* h_prev, int B, int H, int W, int C_hidden, float* u,
                           const oess_f32_view_t* rh, oess_stream_t stream);
int oess_convgru_blend_f32(const float* pre, const float* u, const oess_f32_view_t* h_prev, int B, int H, int W, int C_hidden,
                           const oess_f32_view_t* h, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K15 fp32 SemSegE2VID inference (models/style_networks.py:9-198 of the reference, validation with eval_precision: fp32): the
 * decoder's convolutions are oess_conv2d_fwd_f32; these are the two layers it lacked.  Additions only: the ABI version stays.
 *
 * oess_instance_norm_fwd_f32: nn.InstanceNorm2d(affine=False): out = (in - mean) / sqrt(var + eps) [+ residual] [ReLU if relu],
 *   mean and biased variance per (sample, channel) over H x W.  in, residual (nullable) and out are B x H x W x C views; out may
 *   be in itself.  Two launches, no host synchronisation: per-workgroup (mean, M2) partials of shifted sums merged pairwise
 *   (Chan) in a fixed order -- no raw E[x^2] - E[x]^2, no atomics, bit-repeatable.  Dense 16-byte aligned channels (as above) with
 *   C % 4 == 0 in every view take 16-byte loads and stores.  ws: oess_instance_norm_f32_workspace_bytes(B, H, W, C) bytes,
 *   16-byte aligned (0 for an impossible geometry; B <= 65535).
 * oess_upsample_nearest2x_concat_f32: out[:, :, :, :C] = nearest x2 of in (B x H x W x C), out[:, :, :, C:] = skip
 *   (B x 2H x 2W x C_skip; NULL with C_skip == 0: upsample only); out: B x 2H x 2W x (C + C_skip).  Values are moved, not
 *   computed.  H, W <= 16384.
 * ------------------------------------------------------------------------------------------ */
size_t oess_instance_norm_f32_workspace_bytes(int B, int H, int W, int C);
int oess_instance_norm_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, float eps, int relu,
                               const oess_f32_view_t* residual, const oess_f32_view_t* out, void* ws, size_t ws_bytes,
                               oess_stream_t stream);
int oess_upsample_nearest2x_concat_f32(const oess_f32_view_t* in, int B, int H, int W, int C, const oess_f32_view_t* skip,
                                       int C_skip, const oess_f32_view_t* out, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K16 fp32 DeepLabv3-R50 inference (models/deeplabv3.py:128-189 of the reference in its own arithmetic; frame2recon validation
 * through val_logits(..., precision='fp32')).  Additions only: the ABI version stays.
 *
 * oess_conv2d_dilated_fwd_f32: oess_conv2d_fwd_f32 with a dilation and without its geometry limits: the same kernel, tap
 *   (r, s) reads input row q stride - pad + r dilation.  dilation >= 1; any pad >= 0 that leaves Ho, Wo >= 1 with
 *   Ho = (H' + 2 pad - dilation (R - 1) - 1) / stride + 1; R x S <= 25 taps, or the 7 x 7 stem (the one larger size a
 *   network here has and a test runs; oess_conv2d_f32_packed_floats answers 0 for what is refused, as it did for e.g. 6 x 5); (R - 1) dilation and (S - 1) dilation <= 127 (the tap table
 *   holds offsets in signed char).  Weight packing, epilogue (bias, residual, act) and summation order are those of
 *   oess_conv2d_fwd_f32, which is this entry with dilation 1, R x S <= 25 and pad < R, S: bit-identical results.  With
 *   dilation > 1 and the vector operand path a workgroup leaves out the K steps of every tap that reaches the map from none of
 *   its pixels (exact zeros; at rate 36 on a 28 x 40 map six of nine taps never do).
 * oess_maxpool3x3s2_fwd_f32: nn.MaxPool2d(3, 2, 1): in B x H x W x C -> out B x Ho x Wo x C, Ho = (H - 1) / 2 + 1.  Padding never
 *   wins (-inf); a NaN in the window does (ATen).  16-byte loads / stores when C % 4 == 0 and both views have dense aligned channels.
 * oess_global_avg_pool_fwd_f32: nn.AdaptiveAvgPool2d(1): in B x H x W x C -> out fp32 [B][C] (dense).  Two launches: per-range
 *   sums (a thread's own chain of ceil(H W / ranges / rows) terms, ranges <= 64, rows = 4 .. 256 threads per channel, then a
 *   fixed LDS tree) into ws, then the ranges in index order, divided by H W.  fp32 sums, no
 *   atomics, bit-repeatable.  ws: oess_global_avg_pool_f32_workspace_bytes(B, H, W, C) bytes (0 for an impossible geometry;
 *   B <= 65535), 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int oess_conv2d_dilated_fwd_f32(const oess_f32_view_t* in, const oess_f32_view_t* in2, int B, int H, int W, int Cin, int upsample2x,
                                const float* w_packed, const float* bias, int Cout, int R, int S, int stride, int pad, int dilation,
                                int act, const oess_f32_view_t* residual, const oess_f32_view_t* out, oess_stream_t stream);
int oess_maxpool3x3s2_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, const oess_f32_view_t* out,
                              oess_stream_t stream);
size_t oess_global_avg_pool_f32_workspace_bytes(int B, int H, int W, int C);
int oess_global_avg_pool_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, float* out, void* ws, size_t ws_bytes,
                                 oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K17 fp32 image-teacher inference (models/image_model.py:90-143 of the reference, whose frozen ResNet-50 stays in .train()):
 * the convolutions are oess_conv2d_dilated_fwd_f32 without a fold; this is the layer K16 lacked.  Additions only: the ABI
 * version stays.
 *
 * oess_batch_norm_train_fwd_f32: nn.BatchNorm2d in train mode: out = act((in - mean) * (gamma / sqrt(var + eps)) + beta
 *   [+ residual]), act ReLU if relu, mean and biased variance per channel over B x H x W.  in, residual (nullable) and out are
 *   B x H x W x C views; out may be in itself.  gamma, beta: fp32 [C], nullable (1, 0).  save_mean, save_var (nullable): fp32
 *   [C], the batch mean and the biased variance.  running_mean, running_var (both or neither): r = (1 - momentum) r + momentum
 *   stat, with the unbiased variance (var P / (P - 1), P = B H W).  P < 2 is OESS_EINVAL (torch raises there); 0 <= momentum <= 1.
 *   Three launches, no host synchronisation: per-workgroup (mean, M2) partials of shifted sums; one workgroup per channel group
 *   merges them pairwise (Chan) in a fixed order, writes the statistics and the per-channel coefficients; the apply pass.  No raw
 *   E[x^2] - E[x]^2, no atomics, bit-repeatable.  Dense 16-byte aligned channels (as for K14) with C % 4 == 0 in every view
 *   take 16-byte loads and stores; anything else is read element by element.  ws:
 *   oess_batch_norm_train_f32_workspace_bytes(B, H, W, C) bytes, 16-byte aligned (0 for an impossible geometry: B <= 65535,
 *   B H W < 2^30); a smaller one is OESS_ENOMEM.
 * ------------------------------------------------------------------------------------------ */
size_t oess_batch_norm_train_f32_workspace_bytes(int B, int H, int W, int C);
int oess_batch_norm_train_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, const float* gamma, const float* beta,
                                  float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                                  float* save_var, int relu, const oess_f32_view_t* residual, const oess_f32_view_t* out, void* ws,
                                  size_t ws_bytes, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K18 fp32 SemSegE2VID training: the backward of the decoder's three layer types (stride-1 convolution, InstanceNorm2d,
 * nearest x2 + concat) in fp32.  The data gradient of a stride-1 convolution is oess_conv2d_fwd_f32 itself on the rotated,
 * transposed weight (hip.pack_conv_weight_f32_dgrad); these are the kernels that were missing.  Additions only: the ABI version
 * stays.  Nothing here uses an atomic: every result repeats bit for bit, on any device.
 *
 * oess_conv2d_wgrad_f32: dw[co][ci][r][s] (fp32 OIHW, dense) = sum over (b, oy, ox) of dy[b, oy, ox, co] *
 *   x[b, oy - pad + r, ox - pad + s, ci] (zero outside the map); db (nullable) [Cout] = sum of dy.  x: B x H x W x Cin view,
 *   dy: B x H x W x Cout view.  Geometry: stride 1, dilation 1, R == S in {1, 3}, pad == (R - 1) / 2; anything else is
 *   OESS_EINVAL and a workspace of 0.  One GEMM per tap on v_mfma_f32_32x32x2_f32, D[ci][co] reduced over the pixels in steps
 *   of 16; dense 16-byte aligned channels in both views with Cin % 4 == 0 and Cout % 4 == 0 take 16-byte loads, anything else is
 *   read element by element.  The pixel range is split into n ranges, n a function of the shapes alone (never of the device);
 *   each workgroup stores its partial tile into ws and a second launch adds the ranges in index order.
 *   ws: oess_conv2d_wgrad_f32_workspace_bytes(...) = n (R S Cin Cout + Cout) sizeof(float) bytes, 16-byte aligned.
 * oess_instance_norm_train_fwd_f32: oess_instance_norm_fwd_f32 (same kernels, same bits) that also writes the statistics the
 *   backward needs: save_mean, save_rstd fp32 [B][C], rstd = 1 / sqrt(var + eps).  Same workspace.
 * oess_instance_norm_bwd_f32: backward of out = (x - mean) rstd [ReLU if relu].  With xh = (x - mean) rstd and g = dy [xh > 0]
 *   (relu) or dy:  dx = rstd (g - mean_hw(g) - xh mean_hw(g xh)).  x (the forward's INPUT), dy and dx are B x H x W x C views;
 *   dx may be dy itself.  mean, rstd: what the training forward saved.  A residual added after the norm takes dy unchanged (no
 *   kernel).  Two launches: per-range sums of g and g xh (a thread's own chains, a fixed LDS tree), then the ranges in a fixed
 *   order and the apply pass.  16-byte accesses as for the forward (mean, rstd 16-byte aligned too).
 *   ws: oess_instance_norm_bwd_f32_workspace_bytes(B, H, W, C) bytes, 16-byte aligned (0 for an impossible geometry).
 * oess_downsample_sum2x_f32: backward of the nearest x2 gather of oess_upsample_nearest2x_concat_f32:
 *   dx[b, y, x, c] = ((d[2y][2x] + d[2y][2x+1]) + d[2y+1][2x]) + d[2y+1][2x+1] with d = dout (a B x 2H x 2W x C view: the first
 *   C channels of the concat gradient); dx: B x H x W x C view.  The skip's gradient is the remaining channel slice, as it lies.
 * ------------------------------------------------------------------------------------------ */
size_t oess_conv2d_wgrad_f32_workspace_bytes(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int dilation);
int oess_conv2d_wgrad_f32(const oess_f32_view_t* x, const oess_f32_view_t* dy, int B, int H, int W, int Cin, int Cout, int R, int S,
                          int stride, int pad, int dilation, float* dw, float* db, void* ws, size_t ws_bytes, oess_stream_t stream);
int oess_instance_norm_train_fwd_f32(const oess_f32_view_t* in, int B, int H, int W, int C, float eps, int relu,
                                     const oess_f32_view_t* residual, const oess_f32_view_t* out, float* save_mean, float* save_rstd,
                                     void* ws, size_t ws_bytes, oess_stream_t stream);
size_t oess_instance_norm_bwd_f32_workspace_bytes(int B, int H, int W, int C);
int oess_instance_norm_bwd_f32(const oess_f32_view_t* x, const oess_f32_view_t* dy, const float* mean, const float* rstd, int B, int H,
                               int W, int C, int relu, const oess_f32_view_t* dx, void* ws, size_t ws_bytes, oess_stream_t stream);
int oess_downsample_sum2x_f32(const oess_f32_view_t* dout, int B, int H, int W, int C, const oess_f32_view_t* dx, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K21 fp32 ResNet-50 training: the backward half of the fp32 layer set of the dilated backbone (models/_resnet.py of the
 * reference: strided and dilated convolutions, train-mode BatchNorm2d, the stem's max pool).  The data gradient of a stride-1
 * dilated convolution is oess_conv2d_dilated_fwd_f32 itself on the operand of hip.pack_conv_weight_f32_dgrad with
 * pad' = dilation (R - 1) - pad; these are the kernels that were missing.  Additions only: the ABI version stays.  Nothing here
 * uses an atomic: every result repeats bit for bit, on any device.
 *
 * oess_conv2d_dilated_wgrad_f32: oess_conv2d_wgrad_f32 with a stride, a dilation and free padding: dw[co][ci][r][s] = sum over
 *   (b, oy, ox) of dy[b, oy, ox, co] * x[b, oy stride - pad + r dilation, ox stride - pad + s dilation, ci] (zero outside the
 *   map); db (nullable) [Cout] = sum of dy.  x: B x H x W x Cin view, dy: B x Ho x Wo x Cout view, Ho and Wo by the formula of
 *   oess_conv2d_dilated_fwd_f32.  Geometry: R == S in {1, 3, 7}, stride 1 or 2, dilation >= 1 with (R - 1) dilation <= 127, any
 *   pad >= 0 that leaves Ho, Wo >= 1; anything else is OESS_EINVAL and a workspace of 0.  The same kernel, reduced over the
 *   OUTPUT pixels; the ranges and ws (n (R S Cin Cout + Cout) floats) follow B Ho Wo.  A tap that reaches the map from no output
 *   pixel (dilation 12 on a 3 x 4 map: all but the centre) is written as exact zeros without a K loop.  At stride 1, dilation 1,
 *   R in {1, 3} and pad == (R - 1) / 2 result and workspace size are bit-identical to oess_conv2d_wgrad_f32.
 *   R == 7 with Cin % 4 != 0 (the stem, Cin = 3) folds the taps into the GEMM's M: row tap Cin + ci, ceil(49 Cin / 128) tiles
 *   instead of 49, and the split follows that tile count.
 * oess_conv2d_dgrad_s2_f32: data gradient of a stride-2, dilation-1 convolution, R == S in {1, 3}, 0 <= pad < R: dx (B x H x W x
 *   Cin view) from dy (B x Ho x Wo x Cout view, Ho = (H + 2 pad - R) / 2 + 1), as four stride-1 phase sub-convolutions of dy in
 *   ONE launch of the forward kernel: input pixel (2 qy + py, 2 qx + px) gathers the taps r == py + pad, s == px + pad (mod 2)
 *   from dy[qy + (py + pad - r) / 2][qx + (px + pad - s) / 2].  Every element of dx is written exactly once; a pixel no window
 *   reads (the odd rows and columns of a 1 x 1 conv, a last row or column beyond the last window) gets 0.0.
 *   w_packed (hip.pack_conv_weight_f32_dgrad_s2): oess_conv2d_dgrad_s2_f32_packed_floats(Cout, Cin, R) floats, 16-byte aligned:
 *   four blocks, one per tap parity class c = 2 ry + rx in this order, class (ry, rx) holding the taps r = ry + 2 ty,
 *   s = rx + 2 tx (ny = (R - ry + 1) / 2, nx = (R - rx + 1) / 2 of them; none for R == 1 outside class 0); each block is
 *   [ceil16(ny nx Cout)][ceil32(Cin)], row (ty nx + tx) Cout + co, column ci = weight[co][ci][ry + 2 ty][rx + 2 tx], zeros in
 *   the padding.  The layout does not depend on pad: phase (py, px) reads class ((py + pad) & 1, (px + pad) & 1).
 * oess_batch_norm_bwd_f32: backward of out = act((x - mean) gamma rstd + beta [+ residual]), rstd = 1 / sqrt(var + eps).  With
 *   xh = (x - mean) rstd and g = dy [out > 0] (relu) or dy:  dbeta = sum g, dgamma = sum g xh,
 *   dx = gamma rstd (g - mean_P(g) - xh mean_P(g xh)), dres = g.  x (the forward's INPUT), out (the forward's OUTPUT, read only
 *   with relu: the mask is the forward's bit for bit), dy, dx, dres: B x H x W x C views; mean, var: what
 *   oess_batch_norm_train_fwd_f32 saved (batch mean, biased variance); gamma nullable (1).  dx, dgamma, dbeta, dres are each
 *   nullable and nothing not asked for is computed or stored; dres is written only with relu (without, it is dy).  dx may be dy
 *   itself.  Two launches: per-range sums of g and g xh (a thread's own two-level sums, no accumulator longer than 64 terms
 *   until B H W exceeds 4096 pixels per thread; then a fixed LDS tree), then the ranges in a fixed order and the apply pass.
 *   16-byte accesses as for the forward (mean, var, gamma 16-byte aligned too).
 *   ws: oess_batch_norm_bwd_f32_workspace_bytes(B, H, W, C) bytes, 16-byte aligned (0 for an impossible geometry).
 * oess_maxpool3x3s2_bwd_f32: backward of nn.MaxPool2d(3, 2, 1) in gather form: every pixel of dx (B x H x W x C view) recomputes,
 *   from x, the winner of each of the up to four windows that contain it (ATen's scan: row-major, a value wins when it is
 *   greater than the running maximum or is a NaN; padding never wins) and adds the dy (B x Ho x Wo x C view) of the windows it
 *   won, window rows first.  Every element of dx is written once.
 * ------------------------------------------------------------------------------------------ */
size_t oess_conv2d_dilated_wgrad_f32_workspace_bytes(int B, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad,
                                                     int dilation);
int oess_conv2d_dilated_wgrad_f32(const oess_f32_view_t* x, const oess_f32_view_t* dy, int B, int H, int W, int Cin, int Cout, int R,
                                  int S, int stride, int pad, int dilation, float* dw, float* db, void* ws, size_t ws_bytes,
                                  oess_stream_t stream);
size_t oess_conv2d_dgrad_s2_f32_packed_floats(int Cout, int Cin, int R);   /* 0 for an impossible geometry */
int oess_conv2d_dgrad_s2_f32(const oess_f32_view_t* dy, int B, int H, int W, int Cin, const float* w_packed, int Cout, int R, int S,
                             int pad, const oess_f32_view_t* dx, oess_stream_t stream);
size_t oess_batch_norm_bwd_f32_workspace_bytes(int B, int H, int W, int C);
int oess_batch_norm_bwd_f32(const oess_f32_view_t* x, const oess_f32_view_t* out, const oess_f32_view_t* dy, int B, int H, int W, int C,
                            const float* mean, const float* var, float eps, const float* gamma, int relu, const oess_f32_view_t* dx,
                            float* dgamma, float* dbeta, const oess_f32_view_t* dres, void* ws, size_t ws_bytes, oess_stream_t stream);
int oess_maxpool3x3s2_bwd_f32(const oess_f32_view_t* x, const oess_f32_view_t* dy, int B, int H, int W, int C, const oess_f32_view_t* dx,
                              oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K22 fp32 DeepLabv3-R50 training: what the ASPP head (models/deeplabv3.py:305-348 of the reference) needs next to the K18 / K21
 * layer set.  The head's convolutions and BatchNorms are the K21 entries; the pooling branch's forward is
 * oess_global_avg_pool_fwd_f32 + oess_aspp_pool_fwd_f32 (pooled = the means, in_scale = 1, z_bf16 = NULL).  Additions only: the
 * ABI version stays.  No atomics: every result repeats bit for bit.
 *
 * oess_dropout_f32: nn.Dropout(p) on fp32 views: y = x * (1.0f / (1.0f - p)) (one fp32 multiply) where the element is kept, 0.0f
 *   where it is dropped.  x, y: B x H x W x C views with any strides (channel slices included); y may be x.  The keep decision
 *   of element (pixel, c) is oess_dropout_nhwc_bf16's for the same (seed, offset, P = B H W, C): group i = pixel (C / 8) + c / 8
 *   with pixels in dense B H W order, Philox-4x32-10 counter (i, offset) and key seed, 16-bit lane c % 8 of its four words,
 *   kept when lane >= thr = (unsigned)(p 65536 + 0.5).  The backward pass is the same call on the gradient with the same
 *   (seed, offset).  One thread per 8 channels of a pixel and one Philox call; two 16-byte accesses per view when both views have
 *   dense 16-byte aligned channels, element accesses otherwise.  OESS_EINVAL before any launch: a null view, C % 8 != 0, p outside
 *   [0, 1), a non-positive size.
 * oess_aspp_pool_bwd_f32o: oess_aspp_pool_bwd_f32 whose gradient of the pooled vectors leaves as fp32 [B x Cin] (nullable): the
 *   same two kernels, the last one instantiated for a float store.  Every other output has oess_aspp_pool_bwd_f32's bits.
 * ------------------------------------------------------------------------------------------ */
int oess_dropout_f32(const oess_f32_view_t* x, const oess_f32_view_t* y, int B, int H, int W, int C, float p, unsigned long long seed,
                     unsigned long long offset, oess_stream_t stream);
int oess_aspp_pool_bwd_f32o(const float* grad_z, const float* pooled, float in_scale, const float* w, const float* gamma, const float* y_pre,
                            const float* stat, const float* z, int B, int Cin, int Cout, float* dy_scratch, float* grad_w,
                            float* grad_gamma, float* grad_beta, float* grad_pooled, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K24 SLIC superpixels (data_preparation/superpixel_segmenter_dsec_slic.py:19-24 of the reference:
 * skimage.segmentation.slic(img, n_segments, compactness=6, sigma=3.0, start_label=0); its connectivity pass is the block below).
 * Additions only: the ABI version stays.  fp32, no floating-point atomics: every result repeats bit for bit.
 * A centre is five floats (y, x, L, a, b); centre k = i nx + j of the ny x nx lattice.
 *
 * oess_slic_lab_f32 (superpixel_segmenter_dsec_slic.py:19-24): frames, a B x H x W x 3 view with any strides -> lab, dense
 *   [B, H, W, 3]: per channel a separable Gaussian blur (radius int(4 sigma + 0.5), taps exp(-x^2 / 2 sigma^2) normalised to sum
 *   1, border rule reflect: d c b a | a b c d), skimage's sRGB -> CIELAB (D65, 2 degrees), one multiply by 1 / compactness.
 *   centers (nullable): [B, ny nx, 5], centre (i, j) at y = floor((i + 0.5) H / ny), x = floor((j + 0.5) W / nx) with the map's
 *   value there.  OESS_EINVAL before any launch: a null pointer, sigma <= 0 or > 6, compactness <= 0, min(H, W) < radius + 1,
 *   H W > 2^24, with centers a lattice outside 1 <= ny <= H, 1 <= nx <= W, ny nx <= 256.
 * oess_slic_assign_f32 (superpixel_segmenter_dsec_slic.py:19-24): one assignment pass.  Pixel (y, x) is eligible for centre k
 *   iff int(max(cy - 2 step, 0)) <= y < int(min(cy + 2 step + 1, H)) and the same in x; its distance is
 *   ((y - cy)^2 + (x - cx)^2) (1 / step^2) + sum_c (lab_c - colour_c)^2; the lowest wins, ties go to the lowest k, a pixel
 *   eligible for no centre keeps prev_labels' entry.  prev_labels NULL: the index of the pixel's lattice cell,
 *   (y ny / H) nx + x nx / W, and ny nx must be K.  labels may be prev_labels.  OESS_EINVAL: a null pointer, K outside
 *   [1, 256], step < 1, H W > 2^24.
 * oess_slic_update_f32 (superpixel_segmenter_dsec_slic.py:19-24): new_centers[b, k] = the mean (y, x, L, a, b) of the pixels
 *   labelled k, centers[b, k] for a label no pixel carries (new_centers may be centers); labels outside [0, K) are skipped.
 *   counts (nullable): int [B, K], the pixels of every centre.
 *   Integer sums for the count, y and x, 2^-32 fixed point in 64-bit integers for L, a, b (a value is clamped to |v| <= 64
 *   first: below 2^62 over the 2^24 pixels allowed), a mean is the float64 quotient of sum and count rounded to fp32.  workspace: B K 48 bytes,
 *   8-byte aligned, zeroed by the call; smaller is OESS_ENOMEM.
 * ------------------------------------------------------------------------------------------ */
int oess_slic_lab_f32(const oess_f32_view_t* frames, int B, int H, int W, float sigma, float compactness, float* lab, int ny, int nx,
                      float* centers, oess_stream_t stream);
int oess_slic_assign_f32(const float* lab, const float* centers, const int64_t* prev_labels, int B, int H, int W, int K, int step, int ny,
                         int nx, int64_t* labels, oess_stream_t stream);
int oess_slic_update_f32(const float* lab, const int64_t* labels, const float* centers, int B, int H, int W, int K, float* new_centers,
                         int* counts, void* workspace, size_t workspace_bytes, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K24 SLIC connectivity pass (data_preparation/superpixel_segmenter_dsec_slic.py:19-24 of the reference: skimage's slic runs
 * with its default enforce_connectivity=True).  Additions only: the ABI version stays.  Integer atomics only: every result is a
 * function of the input partition and repeats bit for bit.
 *
 * oess_slic_connectivity_i64 (superpixel_segmenter_dsec_slic.py:19-24): labels, out: dense int64 [B, H, W]; labels are compared
 *   for equality only, any values.  A component is a 4-connected set of equal labels, its root its lowest raster index y W + x.
 *   Components of at least min_size pixels are kept and numbered 0 .. n - 1 in the order of their roots; a smaller one takes the
 *   final label of its donor: walking it breadth first from its root (neighbours right, left, down, up), the LAST neighbour
 *   pixel seen that lies in a component with a smaller root; 0 when there is none.  This is skimage's
 *   _enforce_label_connectivity_cython with one deliberate difference: skimage cuts a flood fill at max_size pixels (the cut
 *   depends on the fill order); here a component of max_size pixels or more stays whole, and there is no max_size.
 *   n_labels (nullable): int [B], the kept components of every sample (0: every pixel of the sample is 0).
 *   workspace: oess_slic_connectivity_workspace_bytes(B, H, W) bytes (five int planes and the chunk counts; 0 for a geometry
 *   that is refused), 4-byte aligned, initialised by the call.  Launches on `stream` only, no read-back.
 *   OESS_EINVAL before any launch: a null labels, out or workspace, out == labels, min_size < 0, B, H or W < 1, H W > 2^24,
 *   more than 2^31 - 1 chunks of 256 pixels, a workspace off 4 bytes; OESS_ENOMEM: a short workspace.
 * oess_slic_connectivity_phase_ms (superpixel_segmenter_dsec_slic.py:19-24): a measurement aid (tools/bench_slic.py).  The same
 *   launches with an event around each of the five phases (components | flatten + sizes | ranks | donors | resolve + write);
 *   waits for the last one and fills phase_ms[5] (host memory) with the milliseconds between them.
 * ------------------------------------------------------------------------------------------ */
size_t oess_slic_connectivity_workspace_bytes(int B, int H, int W);
int oess_slic_connectivity_i64(const int64_t* labels, int B, int H, int W, int min_size, int64_t* out, int* n_labels /* nullable, [B] */,
                               void* workspace, size_t workspace_bytes, oess_stream_t stream);
int oess_slic_connectivity_phase_ms(const int64_t* labels, int B, int H, int W, int min_size, int64_t* out, void* workspace,
                                    size_t workspace_bytes, float* phase_ms, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K25 fp32 MaskCLIP ViT-B/16 inference (models/maskclip_model.py:448-541, 545-851 of the reference in its own arithmetic): the
 * frozen image tower behind the dense-CLIP pseudo-labels.  Inference only.  Additions only: the ABI version stays.  Nothing here
 * uses an atomic: every result repeats bit for bit.
 *
 * oess_attention_d64_f32: oess_attention_d64_bf16 on fp32 operands: qkv = packed [B L, 3 heads 64] rows (q | k | v, dense
 *   channels), out = [B L, heads 64].  Both products run on v_mfma_f32_32x32x2_f32 (k-ordered fp32 fma chains), the online
 *   softmax (running max over 64-key tiles, rescale, accurate expf) is fp32 and P stays fp32 between the two products; a row
 *   is normalised by a true division by its sum.  Keys past L are masked and rows past L of a batch are never used as loaded
 *   (zeroed), so what follows the B L rows may be anything.  Row strides in floats, multiples of 4; pointers 16-byte aligned.
 *   OESS_EINVAL before any launch: a null pointer, B, L or heads < 1, a scale that is not positive and finite, qkv_row_stride < 3 heads 64, out_row_stride < heads 64,
 *   a stride or pointer off that alignment, heads > 2^20, B L >= 2^31 or more than 2^31 - 1 workgroups (128 queries each).
 * oess_layernorm_f32: nn.LayerNorm over C channels of each of `rows` fp32 token rows, 1 <= C <= 2048, eps > 0.  One wave per row,
 *   the row held in registers, TWO passes (mean, then the centred sum of squares; biased variance), y = (x - mean) / sqrt(var +
 *   eps) * gamma + beta.  16-byte accesses when C % 4 == 0, both row strides % 4 == 0 and x, y, gamma, beta are 16-byte aligned;
 *   a 4-byte route otherwise.  Row strides in floats, >= C.
 * oess_linear_tokens_f32: y = act(x W^T + b [+ residual]) for fp32 token rows x [rows, Cin] on the kernel template of
 *   oess_conv2d_fwd_f32 (a 1 x 1 geometry over a [1, C, 1, rows] view; w_packed is the operand of
 *   oess_conv2d_f32_packed_floats(Cout, Cin, 1, 1), 16-byte aligned).  act: 0 none, 1 exact GELU 0.5 v (1 + erff(v 0.70710678f))
 *   (nn.GELU's default), an epilogue the convolution entries do not offer.  bias and residual are nullable; x, residual and out
 *   have dense channels and row strides in floats >= their row.  With act 0 the result equals oess_conv2d_fwd_f32 at R = S = 1
 *   on the same operands bit for bit (the same kernel instance, the same k order).  OESS_EINVAL: a null x, w_packed or out,
 *   rows < 1 or >= 2^31, Cin or Cout < 1, Cin > 2^20, act outside {0, 1}, a stride below its row (res_row_stride is
 *   read only with a residual), w_packed off 16 bytes.
 * ------------------------------------------------------------------------------------------ */
int oess_attention_d64_f32(const float* qkv, long long qkv_row_stride, int B, int L, int heads, float scale, float* out,
                           long long out_row_stride, oess_stream_t stream);
int oess_layernorm_f32(const float* x, long long x_row_stride, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                       float* y, long long y_row_stride, oess_stream_t stream);
int oess_linear_tokens_f32(const float* x, long long x_row_stride, int64_t rows, int Cin, const float* w_packed, const float* bias,
                           int Cout, int act, const float* residual, long long res_row_stride, float* out, long long out_row_stride,
                           oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K26 MaskCLIP refinement of the class logits (MaskClipHead.refine_output, models/maskclip_model.py:224-250 of the reference):
 * prompt denoising and key smoothing.  Additions only: the ABI version stays.  fp32 arithmetic whatever the tower's precision,
 * no floating-point atomic, fixed summation order: every result repeats bit for bit.
 *
 * oess_maskclip_refine_f32: logits, out: fp32 [B, K, H, W] by element strides (sb, sc, sy, sx; any layout, out's elements
 *   distinct and apart from logits); L = H W tokens in raster order.
 *   pd_thresh > 0: conf[b, c] = max_l softmax_c(100 logits)[b, c, l]; a class with conf < pd_thresh gets the logit -100 on every
 *   pixel of that image.
 *   k non-null and ks_thresh > 0: P = softmax_c(100 denoised logits); k: [B, L, C] keys of the last encoder layer, fp32
 *   (OESS_MASKCLIP_K_F32) or bf16 (OESS_MASKCLIP_K_BF16), dense channels, k[b, l, c] at k + b k_img_stride + l k_row_stride + c
 *   (element strides: the tower's [B (L + 1), C] token matrix is read in place past its class-token rows); every channel is
 *   divided by max(its 2-norm over the L tokens, 1e-12) (F.normalize's default dim 1); a pixel with max_c P < ks_thresh takes
 *   its row of (k^ k^T) P, evaluated as k (k^T P / n^2) so that no L x L matrix exists, every other pixel keeps P.  out then
 *   holds probabilities.  Otherwise out is the logits with the -100 rows, untouched values copied bit for bit.
 *   The softmax subtracts the row maximum first (100 x reaches 1e4).  Sums over tokens: per 128-token chunk a wave adds every
 *   fourth token in ascending order with fmaf, the four waves and then the chunks are added in order; sums over channels: a
 *   lane adds channels lane, lane + 64, ... with fmaf, the 64 lanes join by a fixed butterfly.
 *   Served: 1 <= K <= 32, 1 <= H W <= 4096, C % 64 == 0 and 64 <= C <= 1024 (read only with k), 1 <= B <= 65535.
 *   workspace: oess_maskclip_refine_workspace_bytes(B, K, H, W, C) bytes (C = 0: a call without k; 0 for a geometry that is
 *   refused), 16-byte aligned, written by the call.  Launches on `stream` only, no read-back.
 *   OESS_EINVAL before any launch: a null logits, out or workspace, a geometry outside the above, a threshold that is negative,
 *   infinite or NaN, a negative stride or one of 2^40 or more, out elements that overlap, an unknown k_dtype, k_row_stride < C,
 *   k_img_stride below the extent of one image's keys (B > 1), a pointer off its element's alignment, a workspace off 16 bytes;
 *   OESS_ENOMEM: a short workspace.
 * oess_maskclip_refine_phase_ms (models/maskclip_model.py:224-250): a measurement aid (tools/bench_maskclip_refine.py).  The same
 *   launches with an event around each of the five kernels (confidence | mask + softmax | k^T P per chunk | chunk sum + norms |
 *   k Hm + select); waits for the last one and fills phase_ms[5] (host memory) with the milliseconds between them.
 * ------------------------------------------------------------------------------------------ */
#define OESS_MASKCLIP_K_F32 0
#define OESS_MASKCLIP_K_BF16 1
size_t oess_maskclip_refine_workspace_bytes(int B, int K, int H, int W, int C);
int oess_maskclip_refine_f32(const float* logits, long long sb, long long sc, long long sy, long long sx, int B, int K, int H, int W,
                             const void* k /* nullable */, int k_dtype, long long k_row_stride, long long k_img_stride, int C,
                             float pd_thresh, float ks_thresh, float* out, long long ob, long long oc, long long oy, long long ox,
                             void* workspace, size_t workspace_bytes, oess_stream_t stream);
int oess_maskclip_refine_phase_ms(const float* logits, long long sb, long long sc, long long sy, long long sx, int B, int K, int H, int W,
                                  const void* k /* nullable */, int k_dtype, long long k_row_stride, long long k_img_stride, int C,
                                  float pd_thresh, float ks_thresh, float* out, long long ob, long long oc, long long oy, long long ox,
                                  void* workspace, size_t workspace_bytes, float* phase_ms, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K27 Reconstructed grey levels -> the augmented student image of frame2recon.  Replaces, for `recon_sources: online_e2vid`,
 * the host code of DSEC/dataset/sequence_ov.py:154-156 (the reconstruction PNG -> float CHW) and :204-221 (torch.flip,
 * adjust_brightness, adjust_contrast, + 0.05 randn on the recon tensor).  Additions only: the ABI version stays.  No atomic:
 * every result repeats bit for bit and a sample's result depends on neither B nor its place in the batch.
 *
 * oess_gray_augment_rgb_f32: u8 = uint8 [B, H, W] dense (PostProcessor.process_u8's bytes), out = fp32 [B, 3, H, W] dense.
 *   Per sample b: v = byte / 255 (IEEE fp32 division) on three channels; flip_host[b] (0 / 1) mirrors along W;
 *   v = clamp(brightness_host[b] v, 0, 1); m = mean of 0.2989 v + 0.587 v + 0.114 v over the sample (fp32 terms in that order;
 *   two-level sum in a fixed order: fp32 partials of 4096 pixels, then their float64 sum);
 *   v = clamp(contrast_host[b] v + (1 - contrast_host[b]) m, 0, 1), skipped for a factor of exactly 1 (the same bits);
 *   noise_seed_host[b] != 0: v += 0.05 n, n ~ N(0, 1) from Philox-4x32-10 keyed by the seed, counter = index of the group of
 *   four consecutive elements of the sample's [3, H, W] block, Box-Muller on u = ((word >> 8) + 1) 2^-24; no clamp afterwards.
 *   The four host arrays are read during the call (they travel as kernel arguments): no device copy, no synchronisation.
 *   scratch: oess_gray_augment_scratch_bytes(B, H, W) bytes, 4-byte aligned, written by the call; read only when some contrast
 *   factor differs from 1 (may be null otherwise).
 *   OESS_EINVAL before any launch: a null u8, out or host array, B, H or W < 1, 3 H W >= 2^31, out off 4 bytes, a flip outside
 *   {0, 1}, a factor that is negative, infinite or NaN, a null or misaligned scratch when one is needed; OESS_ENOMEM: a short one.
 * oess_gray_augment_scratch_bytes: 64-bit sizes in, 0 for a geometry that is refused.
 * ------------------------------------------------------------------------------------------ */
size_t oess_gray_augment_scratch_bytes(int64_t B, int64_t H, int64_t W);
int oess_gray_augment_rgb_f32(const uint8_t* u8, int B, int H, int W, const int32_t* flip_host, const float* brightness_host,
                              const float* contrast_host, const uint64_t* noise_seed_host, float* out, void* scratch,
                              size_t scratch_bytes, oess_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K29 CLIP text tower in fp32 (OpenAI CLIP's text encoder: width 512, 8 heads of 64, 12 pre-LN blocks, context 77, causal
 * mask, QuickGELU, ln_final, the end-of-text row times text_projection): class names -> the [K, 512] text embeddings every
 * classifier here multiplies with.  Inference only.  Additions only: the ABI version stays.  No atomic: every result repeats
 * bit for bit.
 *
 * oess_attention_d64_causal_f32: oess_attention_d64_f32 (same arguments, same checks, same kernel body) where query i of a
 *   sequence sees keys 0 .. i of that sequence.  A workgroup (128 queries) stops after the last 64-key tile one of its queries
 *   sees; a score with key > query is -inf like one with key >= L.  Row 0 of a sequence is its V row.
 * oess_clip_text_embed_f32: out[n L + t, :] = table[ids[n, t], :] + pos[t, :], ids int64 [N, L] dense, table fp32 [V, C], pos fp32
 *   [>= L, C], out [N L, C]; row strides in floats.  One fp32 add per element.  16-byte accesses when C % 4 == 0, the three
 *   strides % 4 == 0 and table, pos, out are 16-byte aligned.  The ids live on the device: the caller checks 0 <= id < V
 *   (an id outside gives a row of NaN and reads nothing outside the table).  OESS_EINVAL: a null pointer, N, L, V or C < 1,
 *   C > 2^20, a stride below C or >= 2^31, N L >= 2^31, ids off 8 bytes, another pointer off 4, more than 2^31 - 1 workgroups.
 * oess_linear_tokens_quick_gelu_f32: oess_linear_tokens_f32 with the epilogue v / (1 + expf(-1.702 v)) (QuickGELU
 *   v sigmoid(1.702 v), accurate expf) after bias and residual; no `act` argument; otherwise its arguments and refusals.
 * oess_clip_text_eot_layernorm_f32: per sequence n, t* = the FIRST largest of ids[n, 0 .. L) (torch.argmax), y[n, :] =
 *   oess_layernorm_f32 of row n L + t* of x [N L, C].  One wave per sequence; the same two routes chosen by the same rule
 *   (C, both strides, the four pointers), so the result equals oess_layernorm_f32 on the gathered rows bit for bit when the
 *   route is the same.  OESS_EINVAL: what oess_layernorm_f32 refuses, a null ids or one off 8 bytes, N or L < 1, N L >= 2^31.
 * oess_prompt_mean_normalize_f32: e fp32 [N, D], 1 <= D <= 2048; class k owns the prompts host_offsets[k] .. host_offsets[k + 1] - 1
 *   (int64 [K + 1], ascending, first 0, last N, no empty class; dev_offsets is the same array in device memory, host_offsets is
 *   read during the call).  out[k] = s / |s|, s = sum over the class's prompts IN THEIR ORDER of e[n] / |e[n]|, | | = sqrtf of
 *   the sum of squares, true divisions.  The mean's 1 / count cancels and is not applied.  A zero row gives NaN.  One wave per
 *   class.  OESS_EINVAL: a null pointer, N, D or K < 1, N >= 2^31, D > 2048, a stride below D or >= 2^31, e or out off 4 bytes,
 *   an offsets array off 8, offsets that do not start at 0, end at N and ascend strictly.
 * ------------------------------------------------------------------------------------------ */
int oess_attention_d64_causal_f32(const float* qkv, long long qkv_row_stride, int B, int L, int heads, float scale, float* out,
                                  long long out_row_stride, oess_stream_t stream);
int oess_clip_text_embed_f32(const int64_t* ids, int N, int L, const float* table, long long table_row_stride, int V, int C,
                             const float* pos, long long pos_row_stride, float* out, long long out_row_stride, oess_stream_t stream);
int oess_linear_tokens_quick_gelu_f32(const float* x, long long x_row_stride, int64_t rows, int Cin, const float* w_packed,
                                      const float* bias, int Cout, const float* residual, long long res_row_stride, float* out,
                                      long long out_row_stride, oess_stream_t stream);
int oess_clip_text_eot_layernorm_f32(const float* x, long long x_row_stride, const int64_t* ids, int N, int L, int C, const float* gamma,
                                     const float* beta, float eps, float* y, long long y_row_stride, oess_stream_t stream);
int oess_prompt_mean_normalize_f32(const float* e, long long e_row_stride, int64_t N, int D, const int64_t* host_offsets,
                                   const int64_t* dev_offsets, int K, float* out, long long out_row_stride, oess_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OESS_H */
