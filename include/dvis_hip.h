/*
 * dvis_hip.h — C ABI of libdvis_hip.so: the MI355X (gfx950) hot path of DVIS++.
 *
 * Every entry point takes plain DEVICE pointers + sizes + a hipStream_t (passed
 * as void*; NULL = the null stream), enqueues asynchronously on that stream,
 * allocates nothing, keeps no reference to its arguments and is re-entrant.
 * Return value: 0 on success, a negative DVIS_E_* code otherwise;
 * dvis_last_error() returns a thread-local human-readable message.  Launch
 * failures are reported (the reference only printf()s them:
 * ops/src/cuda/ms_deform_im2col_cuda.cuh:953-957).
 *
 * Reference interfaces replaced (paths relative to /root/reference/DVIS_Plus):
 *   dvis_msda_forward        <- ms_deform_attn_forward,  mask2former/modeling/pixel_decoder/ops/src/ms_deform_attn.h:25-45
 *                               (kernel ops/src/cuda/ms_deform_im2col_cuda.cuh:242-304, host ms_deform_attn_cuda.cu:25-85)
 *   dvis_msda_backward       <- ms_deform_attn_backward, ops/src/ms_deform_attn.h:47-66 (ms_deform_attn_cuda.cu:88-158)
 *   dvis_msda_fused_forward  <- softmax + location arithmetic + op of MSDeformAttn.forward,
 *                               ops/modules/ms_deform_attn.py:101-117 (no materialised loc / weights)
 *   dvis_mask_logits         <- einsum("bqc,bchw->bqhw"), dvis_Plus/video_mask2former_transformer_decoder.py:363
 *   dvis_mask_logits_backward <- autograd's backward of einsum("lbtqc,btchw->lbqthw") with respect to mask_embed (training),
 *                               dvis_Plus/tracker.py:379 and dvis_Plus/video_mask2former_transformer_decoder.py:363
 *   dvis_attn_mask           <- einsum + F.interpolate + (sigmoid < 0.5) of forward_prediction_heads, ibid. :363-371,
 *                               plus the "fully masked row" reset at :297
 *   dvis_attention_forward_k <- nn.MultiheadAttention core (softmax(QK^T/sqrt(d) [+mask]) V) as used by
 *                               CrossAttentionLayer / SelfAttentionLayer (mask2former_video/.../video_mask2former_transformer_decoder.py:18-136),
 *                               ReferringCrossAttentionLayer (dvis_Plus/tracker.py:8-92), TemporalRefiner (dvis_Plus/refiner.py:104-139)
 *   dvis_attention_backward  <- autograd's backward of that core without a mask (training of the temporal refiner,
 *                               dvis_Plus/refiner.py:104-139)
 *   dvis_masked_attention_backward <- the same with a mask and up to 65 536 keys (training of the masked-attention decoder's
 *                               cross-attention, dvis_Plus/video_mask2former_transformer_decoder.py:294-303)
 *   dvis_add_layernorm      <- `norm(tgt + tgt2)` of every post-norm residual block (msdeformattn.py:125-131,
 *                               video_mask2former_transformer_decoder.py:47-50,108-111,166-170, tracker.py:51-53)
 *   dvis_nchw_to_tokens      <- src.flatten(2).transpose(1, 2) + torch.cat over levels, msdeformattn.py:64-79
 *   dvis_bias_act            <- FrozenBN shift + shortcut add + ReLU after each backbone convolution (detectron2 BottleneckBlock)
 *   dvis_conv1x1_bias_act    <- 1x1 convolution + that epilogue in one pass (conv1 / conv3 / stride-1 shortcut of the bottleneck)
 *   dvis_conv3x3_winograd    <- 3x3 / stride 1 / pad 1 convolution (+ bias + ReLU): the FPN output convolution of the pixel decoder,
 *                               mask2former/modeling/pixel_decoder/msdeformattn.py:262-270 (built), :343-349 (applied), and conv2 of
 *                               the R50 bottlenecks (detectron2 BottleneckBlock)
 *   dvis_conv3x3s2           <- the stride-2 3x3 convolutions of the R50 (conv2 of the first res3 / res4 / res5 bottleneck)
 *   dvis_conv7x7s2           <- the 7x7 / stride 2 stem convolution of the R50 (detectron2 BasicStem.conv1)
 *   dvis_bias_relu_maxpool   <- FrozenBN shift + ReLU + max_pool2d(3, stride 2, padding 1) of the ResNet stem (detectron2 BasicStem)
 *   dvis_upsample_add        <- `cur_fpn + F.interpolate(out[-1], size=..., mode="bilinear")`, msdeformattn.py:347
 *   dvis_group_norm_affine / dvis_scale_shift_act
 *                            <- the GroupNorm (+ReLU) of detectron2's Conv2d wrapper around the FPN lateral / output
 *                               convolutions, msdeformattn.py:280-300 (built) and :343-349 (applied)
 *   dvis_vps_argmax          <- two-stage resize + sigmoid + score-weighted argmax + segment areas of inference_video_vps,
 *                               dvis_Plus/meta_architecture.py:890-925
 *   dvis_resize2_gt0         <- the two F.interpolate calls + `> 0.` of inference_video_vis, dvis_Plus/meta_architecture.py:843-853
 *   dvis_vss_argmax          <- two-stage resize + sigmoid + einsum("qc,qthw->cthw") + max(0) of inference_video_vss,
 *                               dvis_Plus/meta_architecture.py:954-979
 *   dvis_lsap_solve          <- scipy.optimize.linear_sum_assignment as called by Noiser.match_embds, dvis_Plus/noiser.py:43-56
 *   dvis_match_cost / dvis_point_sample_rows / dvis_point_loss_fwd / dvis_point_loss_bwd
 *                            <- the matching cost and the point-sampled mask losses of the set criterion (training),
 *                               mask2former_video/modeling/matcher.py:107-151, criterion.py:21-67
 *   dvis_match_chain         <- the frame-by-frame matching loop of ReferringTracker_noiser.forward, dvis_Plus/tracker.py:210-291
 *   dvis_gemm_nt             <- the projections around every attention / FFN block of the tracker and the refiner
 *                               (nn.MultiheadAttention in/out_proj, linear1/2, MLP: dvis_Plus/tracker.py:293-318,
 *                               dvis_Plus/refiner.py:104-139), the cosine matrices of Noiser.match_embds (noiser.py:43-56)
 *                               and the refiner's nn.Conv1d layers as im2col GEMMs (refiner.py:42-54,116-119)
 *   dvis_gemm_ln             <- projection + the LayerNorm seam in front of it: `tgt = norm(identity + attn)`, `norm(tgt + ffn(tgt))`
 *                               followed by the next in_proj / linear1 / ref_proj layer, dvis_Plus/tracker.py:45-52, 277-318
 *   dvis_x3_linear / dvis_x3_linear_ln / dvis_x3_ffn_ln
 *                            <- the dense layers of MSDeformAttnTransformerEncoderLayer over all pixels of all frames:
 *                               value_proj / sampling_offsets / attention_weights / output_proj
 *                               (ops/modules/ms_deform_attn.py:96-117), `norm1(src + src2)`, forward_ffn =
 *                               `norm2(src + linear2(relu(linear1(src))))` (mask2former/modeling/pixel_decoder/msdeformattn.py:103-131)
 *   dvis_conv1x1_x3          <- the compute-bound 1x1 convolutions of the R50 bottlenecks (as dvis_conv1x1_mfma) in that arithmetic
 *   dvis_bneck_x3            <- the res2 bottlenecks (detectron2 BottleneckBlock.forward: conv2 -> conv3 + shortcut -> the next block's
 *                               conv1) as one kernel per block, 64-channel maps as pre-split operand images
 *   dvis_pan_pair_hist / dvis_sem_confusion / dvis_video_consistency
 *                            <- the pixel passes of the VPS / VSS scoring scripts, utils/eval_vpq_vspw.py:77-216,
 *                               utils/segmentation_and_tracking_quality.py:131-221, utils/eval_miou_vspw.py:43-56,
 *                               utils/eval_vc_vspw.py:8-23 (csrc/video_metrics.hip)
 *   dvis_rle_encode / dvis_rle_strings / dvis_rle_decode / dvis_track_intersections
 *                            <- the RLE and IoU passes of the VIS evaluation, data_video/ytvis_eval.py:256-293,
 *                               ytvis_api/ytvos.py:218-287, ytvis_api/ytvoseval.py:176-222 (csrc/vis_metrics.hip)
 *   dvis_pan_segment_stats / dvis_pan_paint_rgb / dvis_sem_paint
 *                            <- the pixel passes of the VIPSeg / VSPW prediction writers, data_video/vps_eval.py:112-143,
 *                               data_video/vss_eval.py:93-100 (csrc/pred_write.hip)
 *   dvis_resize_frames_u8    <- the test-time ResizeShortestEdge of the demo / eval loaders: detectron2's
 *                               ResizeTransform.apply_image (Pillow BILINEAR on uint8) as called by demo_video/predictor.py:246
 *                               and data_video/dataset_mapper.py:333, plus the [:, :, ::-1] and transpose(2, 0, 1) around it
 *                               (csrc/frame_resize.hip)
 */
#ifndef DVIS_HIP_H
#define DVIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types of floating tensors */
enum { DVIS_F32 = 0, DVIS_F64 = 1, DVIS_F16 = 2, DVIS_BF16 = 3 };

/* error codes */
enum {
  DVIS_OK = 0,
  DVIS_E_ARG = -1,      /* bad argument (null pointer, non-positive size, unsupported dtype) */
  DVIS_E_LAUNCH = -2,   /* hipLaunchKernel / hipGetLastError failed */
  DVIS_E_UNSUPPORTED = -3
};

const char *dvis_last_error(void);
int dvis_version(void);

/*
 * Multi-scale deformable attention, forward.
 *   value   (N, S, M, D)          dtype
 *   shapes  (L, 2) int64 [H_l, W_l]    DEVICE memory (reference contract, ms_deform_attn_cuda.cu:39-41)
 *   level_start (L,) int64              DEVICE memory
 *   loc     (N, Lq, M, L, P, 2)   dtype, normalised (x, y)
 *   w       (N, Lq, M, L, P)      dtype
 *   out     (N, Lq, M*D)          dtype, fully overwritten (no need to pre-zero)
 * out[n,q,m,:] = sum_{l,p} w * bilinear(value[n, level l, :, m, :], (x*W_l - 0.5, y*H_l - 0.5)), zero padding.
 * Any N is accepted (the reference's N % im2col_step constraint is not needed).
 */
int dvis_msda_forward(int dtype, const void *value, const int64_t *shapes, const int64_t *level_start,
                      const void *loc, const void *w, int N, int S, int M, int D, int L, int Lq, int P,
                      void *out, void *stream);

/*
 * Backward.  grad_value (N,S,M,D), grad_loc (N,Lq,M,L,P,2), grad_w (N,Lq,M,L,P): grad_value MUST be
 * zero-filled by the caller (it is accumulated with atomics); grad_loc / grad_w are fully overwritten.
 */
int dvis_msda_backward(int dtype, const void *value, const int64_t *shapes, const int64_t *level_start,
                       const void *loc, const void *w, const void *grad_out,
                       int N, int S, int M, int D, int L, int Lq, int P,
                       void *grad_value, void *grad_loc, void *grad_w, void *stream);

/*
 * The fp32 backward with a run-to-run REPRODUCIBLE grad_value.  The reference accumulates grad_value with float
 * atomics (ops/src/cuda/ms_deform_im2col_cuda.cuh: atomicAdd in every col2im kernel), so two runs of its backward differ in their
 * last bits; dvis_msda_backward does the same.  Here every contribution is rounded on its own to a multiple of 2^-e (e from the
 * launch's max |grad_out| x max |attention weight|: 42 bits below the largest possible contribution) and added as a 64-bit INTEGER
 * atomic — integer addition is associative, the order the atomics land in does not matter — then converted back.  grad_loc / grad_w
 * are per-sample reductions in a fixed order in both entry points.  ws: dvis_msda_backward_det_ws_bytes(N, S, M, D) bytes
 * (8 per value element + 16), 16-byte aligned, zeroed inside.  ABSOLUTE resolution 2^-42 of max |grad_out| x max |weight| (fp32 carries
 * 2^-24 relative to each sum): cells whose whole sum is below 2^-18 of that bound are less precise than with float atomics.
 */
int64_t dvis_msda_backward_det_ws_bytes(int N, int S, int M, int D);
int dvis_msda_backward_det(const float *value, const int64_t *shapes, const int64_t *level_start, const float *loc, const float *w,
                           const float *grad_out, int N, int S, int M, int D, int L, int Lq, int P, float *grad_value, float *grad_loc,
                           float *grad_w, void *ws, void *stream);

/*
 * Fused forward: takes the RAW outputs of the sampling_offsets / attention_weights linears.  `value`, the offset / logit rows and
 * `out` in `dtype`: DVIS_F32, or DVIS_F16 / DVIS_BF16 storage (what the projections of MSDeformAttn.forward,
 * ops/modules/ms_deform_attn.py:97-105, produce under torch.autocast, how the reference evaluates: train_net_video.py:259; 8
 * channels per lane; the reference's own op dispatches float / double only, ms_deform_attn_cuda.cu:69, and its module falls into
 * the grid_sample path there); reference points and arithmetic fp32 in every case.
 *   offsets  rows of (M, L, P, 2) elements, row stride `off_stride` elements, one row per (n, q)
 *   logits   rows of (M, L*P)     elements, row stride `logit_stride` elements
 *   ref      (Nref, Lq, L, 2) reference points; Nref == 1 broadcasts over the batch
 * loc = ref[:, :, None, :, None, :] + offsets / (W_l, H_l);  w = softmax over (L*P) — ms_deform_attn.py:101-109.
 *   shapes_host: NULL, or a HOST copy of `shapes`; when given and sum(H_l*W_l) == Lq == S (encoder self-attention:
 *   the queries are the pixels) blocks own 8x8 pixel tiles instead of 64 consecutive queries (cache locality only;
 *   results are identical).
 */
int dvis_msda_fused_forward(int dtype, const void *value, const int64_t *shapes, const int64_t *level_start,
                            const float *ref, int Nref, const void *offsets, int64_t off_stride, const void *logits,
                            int64_t logit_stride, int N, int S, int M, int D, int L, int Lq, int P, void *out,
                            const int64_t *shapes_host, void *stream);

/*
 * Backward of dvis_msda_fused_forward (fp32; D in {32, 64}, (L, P) in {(1,4), (3,4), (4,4)}, the forward's stride / alignment / 2 GiB requirements, Nref in {1, N} — anything
 * else is an error code before a launch).  Inputs are the forward's own plus grad_out (N, Lq, M*D) contiguous; the kernel recomputes
 * the softmax and the sampling locations per (n, q, m), so neither they nor their gradients exist in memory.
 *   grad_value   (N, S, M, D), fully written by the call
 *   grad_offsets (N*Lq, M*L*P*2) contiguous: d loss / d raw offset
 *   grad_logits  (N*Lq, M*L*P)   contiguous: d loss / d raw logit (through the softmax)
 * The reference points get no gradient.  ws == NULL: grad_value through float atomics.  ws = dvis_msda_fused_backward_ws_bytes bytes,
 * 16-byte aligned: the 64-bit fixed-point form of dvis_msda_backward_det, its scale from max |grad_out| alone (softmaxed weights
 * are <= 1); a non-finite grad_out, or a NaN / +Inf logit, comes back as NaN grad_value.  grad_offsets / grad_logits are the same
 * bits in both forms.
 */
int64_t dvis_msda_fused_backward_ws_bytes(int N, int S, int M, int D);
int dvis_msda_fused_backward(const float *value, const int64_t *shapes, const int64_t *level_start, const float *ref, int Nref,
                             const float *offsets, int64_t off_stride, const float *logits, int64_t logit_stride,
                             const float *grad_out, int N, int S, int M, int D, int L, int Lq, int P, float *grad_value,
                             float *grad_offsets, float *grad_logits, void *ws, void *stream);

/*
 * Mask logits: out[b, q, p] = sum_c embed[b, q, c] * feat[b, c, p]     (fp32, exact-fp32 MFMA)
 *   embed (B, Q, C), feat (B, C, HW), out (B, Q, HW)
 */
int dvis_mask_logits(const float *embed, const float *feat, int B, int Q, int C, int64_t HW,
                     float *out, void *stream);

/*
 * Backward of the mask logits with respect to the embeddings (dvis_Plus/tracker.py:379,
 * dvis_Plus/video_mask2former_transformer_decoder.py:363), fp32, exact-fp32 MFMA, deterministic (no float atomics):
 *   grad_embed[b, r, c] = sum_p g[b, r, p] * feat[b, c, p]      row_sum[b, r] = sum_p g[b, r, p]
 *   g (B, R, HW) = dL/dlogits, feat (B, C, HW), grad_embed (B, R, C), row_sum (B, R).  R = the rows of one frame (in training
 *   layers x queries, all on the frame's one feature map); C <= 256; R * HW * 4 and C * HW * 4 below 2 GiB.
 * The pixels are cut into ceil(HW / 4096) slabs — a function of HW alone —, every slab's partial tile goes to `ws` and the
 * partials are added in slab order: the same inputs give the same bits on every call.  ws: dvis_mask_logits_backward_ws_bytes
 * bytes (0, and ws may be null, when there is one slab).
 */
int64_t dvis_mask_logits_backward_ws_bytes(int B, int R, int C, int64_t HW);
int dvis_mask_logits_backward(const float *g, const float *feat, int B, int R, int C, int64_t HW, float *grad_embed,
                              float *row_sum, void *ws, void *stream);

/*
 * Attention mask of the masked-attention decoder, one launch:
 *   logits = embed x feat at the stride-4 map (never written to HBM), bilinear-resized
 *   (align_corners=False) to (h, w) where H % h == 0, W % w == 0 and the factor is even
 *   (=> the mean of the 2x2 centre pixels of every block, evaluated in torch's order),
 *   blocked = logits < 0  (== sigmoid < 0.5).
 *   embed (B, Q, C), feat (B, C, H, W)  ->  mask (B, Q, h*w) uint8 (1 = blocked), one copy (not per head);
 *   allowed_count (B, Q) int32 = number of un-blocked keys per row (zeroed inside).  A row with count 0 is
 *   "blocked everywhere": dvis_attention_forward_k then ignores the mask for that row, which is the reference's
 *   reset `attn_mask[where(attn_mask.sum(-1) == HW)] = False` (:297) without its host sync.
 */
int dvis_attn_mask(const float *embed, const float *feat, int B, int Q, int C, int H, int W, int h, int w,
                   uint8_t *mask, int32_t *allowed_count, void *stream);
/*
 * The same attention mask from a feature PYRAMID (round 5).  The bilinear down-sizing of forward_prediction_heads
 * (dvis_Plus/video_mask2former_transformer_decoder.py:367, F.interpolate(..., align_corners=False) by an even integer factor) is
 * linear: out = 0.25 ((l_a + l_b) + (l_c + l_d)) over the four centre pixels of a block = the contraction of
 * 0.25 ((f_a + f_b) + (f_c + f_d)).  dvis_center_pool3 forms those averages for the factors 2 / 4 / 8 of a stride-4 map in ONE read
 * (feat: `planes` maps of H x W, H % 8 == W % 8 == 0 -> p2 (H/2 x W/2), p4, p8), once per clip; dvis_attn_mask_pooled contracts a
 * level's pooled map (B, C, h, w) and thresholds: mask (B, Q, h*w) uint8 (1 = blocked), allowed_count as above.  One quarter of
 * dvis_attn_mask's products per layer and no re-read of the stride-4 map in any of the nine decoder layers.  Equal to
 * dvis_attn_mask except where |logit| is of the order of its rounding error (the two orders round differently).
 */
int dvis_center_pool3(const float *feat, int64_t planes, int H, int W, float *p2, float *p4, float *p8, void *stream);
int dvis_attn_mask_pooled(const float *embed, const float *pooled, int B, int Q, int C, int h, int w, uint8_t *mask,
                          int32_t *allowed_count, void *stream);
/* How dvis_mask_logits (mode 0, map H x W), dvis_attn_mask (mode 1, H x W -> h x w) or dvis_attn_mask_pooled (mode 2, pooled map
 * H x W; h, w unused) would run, from the function their launch consults (host only, launches nothing).  aligned: the map and the
 * output are 16-byte aligned; embed_aligned: so is `embed`.  plan[0] = number of passes over the queries (of at most 112), then for
 * each of the first min(passes, capacity) passes 8 words: qbeg (its first query), QT (query tiles of the instantiation: 2, 4 or 7),
 * fullc (C % 32 == 0 and embed aligned: 16-byte reads of embed, no per-channel selects), vec (16-byte map loads and packed stores:
 * modes 0 and 2, HW % 4 == 0, aligned, fullc), gpf (wave groups per frame: of 64 map pixels, mode 1 of 16 outputs), spf (steps of 8
 * groups per frame), total_steps (B * spf) and nwg (workgroups that share the steps out: min(total_steps, 256 at QT = 7, else 512)).
 * plan holds 1 + 8 * capacity words.  Refuses the shapes the three entry points refuse (C > 256, mode 1 without an even factor). */
int dvis_mask_gemm_plan(int mode, int B, int Q, int C, int H, int W, int h, int w, int aligned, int embed_aligned, int32_t *plan,
                        int capacity);

/*
 * softmax(Q K^T * scale [masked]) V for B batch entries x `heads` heads, fp32 in/out, exact-fp32 MFMA.
 *   q (B, heads, Lq, d), k / v (B, heads, Lk, d), out (B, heads, Lq, d) as STRIDED views: x_strides[3] =
 *   {batch, head, row} strides in floats, d contiguous, d in {32, 64}.  (Lets q/k/v be slices of fused
 *   projections and out be the (Lq, B, heads*d) buffer the out-projection reads.)
 *   mask: NULL or uint8 (B, Lq, Lk), 1 = blocked, shared by the heads of a batch entry (4-byte aligned).
 *   allowed_count: NULL or int32 (B, Lq) from dvis_attn_mask; rows with count 0 ignore the mask.
 *   ws: workspace of dvis_attention_ws_bytes_k(B*heads, Lq, Lk, d, kernel) bytes (split-K partials); may be NULL when 0.
 *   kernel: 0 = chosen from the sizes; or chosen by the CALLER: 1 = the short-key latency kernel (Lk <= 128: one workgroup per
 *   (batch, head, 16-query tile), K / V staged in one memory round trip), 2 = below.  A (batch, head)'s result depends on the
 *   kernel, so a caller that needs the same bits for a clip whether it runs alone or batched with others (the referring
 *   tracker's recurrence, dvis_Plus/tracker.py:277-318) pins it.
 */
int dvis_attention_forward_k(const float *q, const int64_t *q_strides, const float *k, const int64_t *k_strides,
                           const float *v, const int64_t *v_strides, float *out, const int64_t *o_strides,
                           const uint8_t *mask, const int32_t *allowed_count, int B, int heads, int Lq, int Lk,
                           int d, float scale, void *ws, void *stream, int kernel);
/* kernel 2: long self-attention at d = 64 without a mask (the ViT blocks of the DINOv2 / ViT-Adapter backbones,
 * dvis_Plus/../vit_adapter: 3681 tokens x 16 heads at 720p) on split-f16 matrix-core products — Q, K, V as two f16 terms each
 * (x3_common.h: three products per fp32 product, fp32 accumulation), softmax in fp32, the probabilities split the same way.
 * Two launches: the operands' two-term images are written once into `ws` (dvis_attention_ws_bytes_k(.., 2) bytes: what Q, K, V
 * take in fp32), then one workgroup per (batch-head, 128 queries) streams K / V from there.  Operands must stay below 4095 (65520 / 2^4) in
 * magnitude (the range guard of dvis_x3_set_range_flag reports a violation). */
int64_t dvis_attention_ws_bytes_k(int BH, int Lq, int Lk, int d, int kernel);
/* Which kernel dvis_attention_forward_k(.., kernel) would launch for these sizes and how it cuts the work — host only, nothing is
 * launched; the launch takes its decision from the same function, so the answer is the dispatch and not a description of it.
 *   k_row / v_row: row strides of k / v in floats (x_strides[2]); has_mask: mask != NULL.
 *   plan[4] = {served_by (DVIS_ATTN_*), nsplit, keys_per_split, qchunks}: nsplit key ranges of keys_per_split keys per (batch, head)
 *   (the last holds Lk - (nsplit - 1) * keys_per_split; partials merged by a second launch when nsplit > 1), qchunks units along the
 *   queries: of 128 queries (DVIS_ATTN_FWD, DVIS_ATTN_X3), 112 (DVIS_ATTN_KEYSPLIT) or 16 (DVIS_ATTN_SHORT).
 * Refuses what the launch refuses for the same arguments (head dim, batch * heads, kernel 1 with Lk > 128, kernel 2 with a mask...). */
enum {
  DVIS_ATTN_FWD = 0,      /* attn_fwd_kernel: query-partitioned, keys in LDS stages, optional split over keys */
  DVIS_ATTN_SHORT = 1,    /* attn_short_kernel: Lk <= 128, one workgroup per 16 queries, keys over 4 waves */
  DVIS_ATTN_X3 = 2,       /* attn_x3_kernel: split-f16 products, d = 64, no mask (kernel = 2 only) */
  DVIS_ATTN_KEYSPLIT = 3  /* attn_keysplit_kernel: d = 32, > 64 queries, >= 512 keys, one key range per wave */
};
int dvis_attention_plan(int BH, int Lq, int Lk, int d, int has_mask, int64_t k_row, int64_t v_row, int kernel, int32_t *plan);

/*
 * Backward of softmax(Q K^T * scale) V without a mask, fp32, exact fp32 FMA arithmetic, deterministic (no float atomics):
 *   P = softmax(Q K^T * scale)   dV = P^T dO   dP = dO V^T   D = rowsum(P o dP)   dS = P o (dP - D)
 *   dQ = scale * dS K            dK = scale * dS^T Q
 * The probabilities are recomputed from q and k; nothing of the forward is needed.
 *   q / grad_out (B, heads, Lq, d), k / v (B, heads, Lk, d) as STRIDED views as in dvis_attention_forward_k (x_strides[3] =
 *   {batch, head, row} in floats, d contiguous, 16-byte aligned, strides multiples of 4 floats); d in {32, 64}; 1 <= Lk <= 256.
 *   dq (Lq, B, heads * d), dk / dv (Lk, B, heads * d): contiguous outputs.
 * One workgroup per (batch entry, head) walks the queries in chunks of 16 in ascending order, so the sums of dK / dV over the
 * queries have one fixed order and the bits of a (batch entry, head) do not depend on B.  No workspace.
 */
int dvis_attention_backward(const float *q, const int64_t *q_strides, const float *k, const int64_t *k_strides,
                            const float *v, const int64_t *v_strides, const float *grad_out, const int64_t *g_strides,
                            float *dq, float *dk, float *dv, int B, int heads, int Lq, int Lk, int d, float scale,
                            void *stream);
/* Threads per workgroup of that launch: 64, 128 or 256 (one per key; the row reductions then run over 4, 8 or 16 lanes per query row);
 * 0 for an Lk the kernel does not serve.  Host only; the launch takes its block size from it. */
int dvis_attention_backward_threads(int Lk);

/*
 * Backward of softmax(Q K^T * scale [+ mask]) V for long key sequences with the forward's mask semantics (training of the
 * segmenter's masked-attention decoder: 100 - 200 queries over every pixel of a feature level), fp32, exact fp32 FMA arithmetic,
 * deterministic (no float atomics):
 *   P = softmax over the allowed keys   dV = P^T dO   dP = dO V^T   D = rowsum(P o dP)   dS = P o (dP - D)
 *   dQ = scale * dS K                   dK = scale * dS^T Q
 * P is recomputed from q and k, and D from that P: nothing of the forward is needed.
 *   q / grad_out (B, heads, Lq, d), k / v (B, heads, Lk, d) as STRIDED views as in dvis_attention_forward_k (x_strides[3] =
 *   {batch, head, row} in floats, d contiguous, 16-byte aligned, strides multiples of 4 floats); d in {32, 64};
 *   1 <= Lq <= 256, 1 <= Lk <= 65536.
 *   mask: NULL or uint8 (B, Lq, Lk), 1 = blocked, shared by the heads (rows need no alignment); a blocked key has P = 0 exactly.
 *   allowed_count: int32 (B, Lq), required beside a mask; a row with count 0 ignores its mask.
 *   dq (Lq, B, heads * d), dk / dv (Lk, B, heads * d): contiguous outputs.
 *   ws: dvis_masked_attention_backward_ws_bytes(B * heads, Lq, Lk, d) bytes, 16-byte aligned (row statistics, per-key-tile
 *   (max, sum, sum of 2^x dP) triples and per-key-tile shares of dQ; 0 for sizes the kernel does not serve).
 * The keys are cut into tiles of `key_tile` over workgroups; four launches (tile statistics, row statistics, dK / dV and the tiles'
 * shares of dQ, dQ).  Every sum has one order that depends on (Lq, Lk, d) alone, so the bits of a (batch entry, head) do not depend
 * on B.
 */
int64_t dvis_masked_attention_backward_ws_bytes(int BH, int Lq, int Lk, int d);
int dvis_masked_attention_backward(const float *q, const int64_t *q_strides, const float *k, const int64_t *k_strides,
                                   const float *v, const int64_t *v_strides,
                                   const float *grad_out, const int64_t *g_strides, const uint8_t *mask,
                                   const int32_t *allowed_count, float *dq, float *dk, float *dv, int B, int heads, int Lq,
                                   int Lk, int d, float scale, void *ws, void *stream);
/* How that launch cuts the work — host only; the launch takes its grid, block and LDS size from the same function.
 *   plan[5] = {key_tile, query_tile, n_key_tiles, threads, lds_bytes}: keys per workgroup, queries per chunk inside a workgroup,
 *   workgroups per (batch entry, head), threads per workgroup (one per key of the tile), dynamic LDS of the two tile launches.
 * Refuses the sizes the launch refuses. */
int dvis_masked_attention_backward_plan(int Lq, int Lk, int d, int32_t *plan);

/*
 * out[r, :] = LayerNorm(x[r, :] + res[r, :]) * gamma + beta, rows x C fp32 (C % 4 == 0, C <= 1024); `res` may be NULL
 * and may have its own row stride (floats).  One pass: 2 reads + 1 write (torch: add kernel + layer_norm kernel).
 * pos / out_pos (both or neither; then pos_rows > 0): a second output  out_pos[r, :] = out[r, :] + pos[r mod pos_rows, :]
 * (pos: pos_rows x C): the deformable encoder's next-layer query `with_pos_embed(src, pos)` (msdeformattn.py:121-123 /
 * ms_deform_attn.py:108) is written while the row is still in registers instead of by an add kernel of its own.
 */
int dvis_add_layernorm(const float *x, const float *res, int64_t res_row_stride, const float *gamma, const float *beta,
                       float *out, const float *pos, int64_t pos_rows, float *out_pos, int64_t rows, int C, float eps,
                       void *stream);

/*
 * out = lateral + F.interpolate(top, size=(H, W), mode="bilinear", align_corners=False) for `planes` = N*C planes;
 * lateral / out (planes, H, W), top (planes, h, w); W % 4 == 0.  (FPN top-down step, msdeformattn.py:347.)
 * lat_scale / lat_shift (both or neither; per plane, from dvis_group_norm_affine): the lateral operand is read as
 * lateral * scale + shift — the lateral convolution's GroupNorm applied on the fly (msdeformattn.py:345-347).
 */
int dvis_upsample_add(const float *lateral, const float *lat_scale, const float *lat_shift, const float *top, float *out,
                      int64_t planes, int H, int W, int h, int w, void *stream);

/*
 * out[n][row0 + p][c] = x[n][c][p]: lays an (N, C, HW) map down as HW rows of an (N, S, C) token matrix — the
 * flatten(2).transpose(1, 2) + torch.cat over levels of MSDeformAttnTransformerEncoderOnly.forward
 * (mask2former/modeling/pixel_decoder/msdeformattn.py:64-79).  x contiguous (N, C, HW), out contiguous (N, S, C).
 * scale / shift: the map is read as x[n][c] * scale[n*C + c] + shift[n*C + c] (the input projection's GroupNorm,
 * msdeformattn.py:231-247, from dvis_group_norm_affine; NULL pair = identity).  pos / out_pos: a second output
 * out_pos[n][row0 + p][c] = out[n][row0 + p][c] + pos[row0 + p][c] (pos: (S, C) token-major position + level embedding;
 * the first encoder layer's query, msdeformattn.py:121-123; NULL pair = not written).
 */
int dvis_nchw_to_tokens(const float *x, const float *scale, const float *shift, const float *pos, float *out, float *out_pos,
                        int64_t N, int C, int64_t HW, int64_t S, int64_t row0, void *stream);
/* The way back for one level: out (N, C, HW) = tok[:, row0 : row0 + HW, :] transposed (tok: (N, S, C)) — the encoder output
 * as the map the FPN's top-down path reads, msdeformattn.py:333-339 (+ :347). */
int dvis_tokens_to_nchw(const float *tok, float *out, int64_t N, int C, int64_t HW, int64_t S, int64_t row0, void *stream);
/* Input normalisation + zero padding of a clip in one pass (dvis_Plus/meta_architecture.py:1310-1311, :186-187, :638-639:
 * `(x - pixel_mean) / pixel_std`, then ImageList.from_tensors(images, size_divisibility)):
 * out (planes, Hp, Wp) = (float(in (planes, H, W)) - mean[p % C]) / std[p % C] inside the image, 0 in the padding; in: uint8
 * (is_u8 = 1) or fp32 planes, planes = frames * C.  The same fp32 subtract and divide as the torch expression: same bits. */
int dvis_normalize_pad(const void *in, int is_u8, float *out, int64_t planes, int C, int H, int W, int Hp, int Wp, const float *mean,
                       const float *stdv, void *stream);

/*
 * 1x1 stride-1 convolution on NCHW with its epilogue in one pass (exact-fp32 MFMA):
 *   out[n, m, p] = relu?( sum_k w[m, k] x[n, k, p] + bias[m] (+ res[n, m, p]) )
 *   x (N, K, HW), w (M, K) (FrozenBN scale folded in), bias (M) or NULL, res (N, M, HW) or NULL, out (N, M, HW); fp32,
 *   16-byte aligned, K % 4 == 0, HW % 4 == 0.  Replaces conv -> dvis_bias_act for the bottleneck's conv1 / conv3 /
 *   stride-1 shortcut (detectron2 BottleneckBlock, FrozenBN folded by the caller) where the layer is memory-bound.
 *   dvis_conv1x1_supported(K, M, HW) != 0 tells whether the shape is served (M <= 64: K <= 512; M <= 128: K <= 256;
 *   wider: K <= 128); other shapes return DVIS_E_ARG — the caller keeps the library contraction for them.
 */
int dvis_conv1x1_supported(int K, int M, int64_t HW);
/*
 * The same operation for the COMPUTE-bound 1x1 layers (many input channels: C % 128 == 0, K % 64 == 0, HW even and >= 64): weights
 * streamed through the MFMA operand layout `uf` (K * C floats, written by dvis_conv1x1_mfma_pack), 64 pixels x 64 output channels
 * per workgroup.  y (N, K, HW) = relu?(w (K, C) x (N, C, HW) + bias[k] + res).
 */
int dvis_conv1x1_mfma_supported(int C, int K, int64_t HW);
int dvis_conv1x1_mfma_pack(const float *w, float *uf, int K, int C, void *stream);
int dvis_conv1x1_mfma(const float *x, const float *uf, const float *bias, const float *res, float *y, int N, int C, int K, int64_t HW,
                      int relu, void *stream);
/* stride 2 (the 1x1 shortcut of the first res3 / res4 / res5 bottleneck): y (N, K, ceil(H/2), ceil(W/2)) = relu?(w x[:, :, ::2, ::2] + bias + res);
 * served when dvis_conv1x1_mfma_supported(C, K, ceil(H/2) * ceil(W/2)) and 2 input images stay below 2 GiB. */
int dvis_conv1x1s2_mfma(const float *x, const float *uf, const float *bias, const float *res, float *y, int N, int C, int K, int H, int W,
                        int relu, void *stream);
int dvis_conv1x1_bias_act(const float *x, const float *w, const float *bias, const float *res, float *out,
                          int N, int K, int M, int64_t HW, int relu, void *stream);

/*
 * y (N, K, H, W) = relu?(conv2d(x (N, C, H, W), w (K, C, 3, 3), stride 1, padding 1) + bias[k]) as Winograd F(2x2, 3x3) on the fp32
 * matrix cores: 4 multiplies per output instead of 9, accumulated in a fixed order (bit-reproducible).  `uf` = the transformed
 * weights (16 * K * C floats), written once per weight by dvis_conv3x3_winograd_pack(w, uf, K, C).  bias (K) or NULL.  fp32, NCHW
 * contiguous, 16-byte aligned.  dvis_conv3x3_winograd_supported(C, K, H, W) != 0 tells whether the shape is served (C % 16 == 0,
 * K % 64 == 0, W even, at least 64 2x2 tiles per image, 2 images < 2 GiB); other shapes return DVIS_E_ARG — the caller keeps the library
 * convolution for them.  Rounding differs from a direct convolution by the usual F(2x2, 3x3) factor (a few fp32 ulps of the
 * accumulated magnitude; tests/test_winograd_gpu.py bounds it against fp64).
 */
int dvis_conv3x3_winograd_supported(int C, int K, int H, int W);
/*
 * The same for stride 2 (padding 1): y (N, K, ceil(H/2), W/2) = relu?(conv2d(x, w, stride 2, padding 1) + bias[k]), direct on the fp32
 * matrix cores (conv2 of the first bottleneck of res3 / res4 / res5 in detectron2's ResNet with STRIDE_IN_1X1 = False).  `uf` =
 * the weights in the MFMA operand layout (12 * K * C floats), written by dvis_conv3x3s2_pack.  Same shape rules (W even).
 */
int dvis_conv3x3s2_supported(int C, int K, int H, int W);
/*
 * The ResNet stem: y (N, 64, H/2, W/2) = relu?(conv2d(x (N, 3, H, W), w (64, 3, 7, 7), stride 2, padding 3) + bias[k]), direct on
 * the fp32 matrix cores (detectron2 BasicStem.conv1).  `uf` = 10 240 floats written by dvis_conv7x7s2_pack(w, uf).  H, W even.
 */
int dvis_conv7x7s2_supported(int C, int K, int H, int W);
int dvis_conv7x7s2_pack(const float *w, float *uf, void *stream);
int dvis_conv7x7s2(const float *x, const float *uf, const float *bias, float *y, int N, int H, int W, int relu, void *stream);
int dvis_conv3x3s2_pack(const float *w, float *uf, int K, int C, void *stream);
int dvis_conv3x3s2(const float *x, const float *uf, const float *bias, float *y, int N, int C, int K, int H, int W, int relu,
                   void *stream);
int dvis_conv3x3_winograd_pack(const float *w, float *uf, int K, int C, void *stream);
int dvis_conv3x3_winograd(const float *x, const float *uf, const float *bias, float *y, int N, int C, int K, int H, int W,
                          int relu, void *stream);

/*
 * In place on `planes` = N*C contiguous planes of HW floats (NCHW): x = relu?(x + bias[c] + res).  bias (C,) or NULL,
 * res same shape as x or NULL.  The folded-FrozenBN bias, bottleneck shortcut add and ReLU after a library convolution
 * in one pass.  HW % 4 == 0.
 */
int dvis_bias_act(float *x, const float *bias, const float *res, int64_t planes, int C, int64_t HW, int relu,
                  void *stream);

/*
 * out (planes, H/2, W/2) = relu(max_pool2d(x (planes, H, W), kernel 3, stride 2, padding 1) + bias[plane % C]) — equal, bit
 * for bit, to max_pool2d(relu(x + bias)) (fp32 add and ReLU are monotonic): the stem's folded-FrozenBN shift, ReLU and
 * pooling in one pass over the stem convolution's output.  bias (C,) or NULL.  H even, W % 8 == 0, x / out 16-byte aligned.
 */
int dvis_bias_relu_maxpool(const float *x, const float *bias, float *out, int64_t planes, int C, int H, int W,
                           void *stream);

/*
 * GroupNorm as two cheap steps (nn.GroupNorm(G, C) on (N, C, HW) fp32, eps as given):
 *   dvis_group_norm_affine  statistics of every (sample, group) in ONE read of x (fp64 sums), returned as the per-plane
 *                           affine  scale[n*C + c] = rstd * gamma[c],  shift[n*C + c] = beta[c] - mean * scale
 *                           (gamma / beta may be NULL = 1 / 0);  (C / G) * HW % 4 == 0, x 16-byte aligned;
 *   dvis_scale_shift_act    in place x[plane] = relu?(x[plane] * scale[plane] + shift[plane]) — GroupNorm (+ReLU) applied;
 *                           (or on the fly: the lat_scale / lat_shift of dvis_upsample_add).
 */
int dvis_group_norm_affine(const float *x, const float *gamma, const float *beta, float *scale, float *shift, int64_t N,
                           int C, int G, int64_t HW, float eps, void *stream);
int dvis_scale_shift_act(float *x, const float *scale, const float *shift, int64_t planes, int64_t HW, int relu,
                         void *stream);
/* dvis_group_norm_affine's (scale, shift) from the partial sums a convolution left in `part` (dvis_conv1x1_x3 / dvis_conv_x3_image,
 * gn_part: (N, G, HW / 32, 2) doubles) instead of a read of the map: the same formula and casts; HW % 32 == 0, C / G <= 64. */
int dvis_group_norm_finalize(const double *part, const float *gamma, const float *beta, float *scale, float *shift, int64_t N, int C,
                             int G, int64_t HW, float eps, void *stream);

/*
 * Depthwise 3 x 3 convolution (padding 1) + bias (+ exact GELU) on a TOKEN-major map: the ConvFFN of the ViT-Adapter extractors
 * (mask2former/modeling/backbones_vitAdapter/adapter_modules.py, DWConv + the GELU that follows it in ConvFFN.forward).  The
 * reference transposes each of the three pyramid levels of its (B, N, C) token tensor to NCHW, runs a grouped Conv2d, transposes
 * back and concatenates; here one call per level reads and writes the token tensor in place of all that:
 *   x / out: level base pointers, token (b, y, x) at base + b * batch_stride + (y * w + x) * C; weight (C, 1, 3, 3) = C x 9; bias C or
 *   NULL; C % 4 == 0; out must not alias x.
 */
int dvis_dwconv3x3_tokens(const float *x, float *out, int64_t batch_stride, int B, int h, int w, int C, const float *weight,
                          const float *bias, int gelu, void *stream);

/*
 * Backward of dvis_dwconv3x3_tokens for one level (csrc/dwconv_tokens_backward.hip).  Replaces what autograd records for the
 * reference's ConvFFN / DWConv (mask2former/modeling/backbones_vitAdapter/adapter.py:61-98): per level a transposed contiguous copy,
 * a grouped Conv2d's data and weight gradients, GeluBackward, the transpose back and the concatenation's split.
 *   x: the forward's input (nothing else is saved); grad_out / grad_x: laid out like x (token (b, y, x) at base + b * batch_stride +
 *   (y * w + x) * C); weight (C, 1, 3, 3) = C x 9; bias C or NULL; gelu: the forward's flag.  z = conv(x) + bias is recomputed in the
 *   forward's tap order, dz = grad_out * gelu'(z) (exact erf form), grad_x = conv(dz, flipped taps), grad_weight (C, 9) and grad_bias (C,
 *   may be NULL) = sums over every token of dz * x-window and dz.
 * Exact fp32, no atomics: the weight / bias sums go through a bounded number of per-workgroup partial rows added in a fixed order, so
 * two calls give the same bits.  ws: dvis_dwconv3x3_tokens_backward_ws_bytes(B, h, w, C) bytes (dz + the partial rows; -1 for bad
 * sizes), 16-byte aligned.  Refused: C % 4 != 0, a batch stride that is not a multiple of 4 floats or < h * w * C, pointers not
 * 16-byte aligned, null pointers, grad_x aliasing grad_out or x.
 */
int64_t dvis_dwconv3x3_tokens_backward_ws_bytes(int B, int h, int w, int C);
int dvis_dwconv3x3_tokens_backward(const float *x, const float *grad_out, const float *weight, const float *bias, int gelu,
                                   int64_t batch_stride, int B, int h, int w, int C, float *grad_x, float *grad_weight, float *grad_bias,
                                   void *ws, void *stream);

/*
 * The stride-4 output of the ViT-Adapter backbone (mask2former/modeling/backbones_vitAdapter/adapter.py, forward:
 * `c1 = self.up(c2) + c1; c1 = c1 + F.interpolate(x1, scale_factor=4, mode="bilinear", align_corners=False); f1 = self.norm1(c1)`).
 * `up` = ConvTranspose2d(C, C, 2, 2) is a GEMM over the stride-8 tokens with 4 C output features ordered (dy, dx, co); the caller
 * runs it with the eval-BatchNorm scale folded into the weights and hands the TOKEN-major result in:
 *   out[b, co, 2y+dy, 2x+dx] = g[(b, y, x), (dy, dx, co)] + scale[co] * (c1[b, co, 2y+dy, 2x+dx] + up4(x1)[b, co, 2y+dy, 2x+dx]) + shift[co]
 *   g (B * h8 * w8, 4 C); c1 / out (B, C, 2 h8, 2 w8) NCHW; x1 (B, (h8 / 2) * (w8 / 2), C) tokens of the stride-16 ViT grid or NULL;
 *   shift = scale * up.bias + (BN beta - mean * scale).  C % 64 == 0, h8 and w8 even, B * h8 <= 65535.
 * One pass over the output (7.2 GB at 30 frames x 1024 channels x 184 x 320) instead of six.
 */
int dvis_adapter_res2(const float *g, const float *c1, const float *x1, const float *scale, const float *shift, float *out, int B, int C,
                      int h8, int w8, void *stream);

/*
 * Panoptic arg-max of a clip in one pass (inference_video_vps, dvis_Plus/meta_architecture.py:890-925):
 *   prob_k = resize2(sigmoid(resize1(logits_k)[:img_h, :img_w])), both resizes bilinear align_corners=False
 *   (stride-4 map (h,w) -> padded input (first_h, first_w) -> crop (img_h, img_w) -> output (out_h, out_w));
 *   ids = argmax_k scores[k] * prob_k (first maximum wins), conf = prob_ids >= 0.5,
 *   areas (3, K) int32 = [ (ids == k).sum(), (prob_k >= 0.5).sum(), ((ids == k) & conf).sum() ]   (zeroed inside).
 *   logits: K x T maps of h*w floats, logits[k][t] at logits + k*stride_k + t*stride_t; 1 <= K <= 256.
 *   ids (T, out_h, out_w) int32, conf (T, out_h, out_w) uint8.  T == 0: logits, ids and conf are empty and may be null; the
 *   areas are still zeroed.
 */
int dvis_vps_argmax(const float *logits, int64_t stride_k, int64_t stride_t, const float *scores, int K, int T,
                    int h, int w, int first_h, int first_w, int img_h, int img_w, int out_h, int out_w,
                    int32_t *ids, uint8_t *conf, int32_t *areas, void *stream);

/*
 * Instance masks of a clip in one pass (inference_video_vis, dvis_Plus/meta_architecture.py:843-853; MinVIS.inference_video
 * :390-399):  out[k][t] = resize2(resize1(logits[k][t])[:img_h, :img_w]) > 0,  both resizes bilinear align_corners=False,
 * evaluated in torch's CPU operation order (csrc/torch_cpu_math.h).  logits: K x T maps of h*w floats at
 * logits + k*stride_k + t*stride_t;  out (K, T, out_h, out_w) uint8 (0 / 1), 4-byte aligned.
 */
int dvis_resize2_gt0(const float *logits, int64_t stride_k, int64_t stride_t, int K, int T, int h, int w, int first_h,
                     int first_w, int img_h, int img_w, int out_h, int out_w, uint8_t *out, void *stream);

/*
 * The float values behind dvis_resize2_gt0 / dvis_vps_argmax:  out[k][t] = resize2(f(resize1(logits[k][t])[:img_h, :img_w])),
 * f = sigmoid when `sigmoid` != 0, identity otherwise — the reference's interpolate -> crop -> (sigmoid) -> interpolate
 * sequence (dvis_Plus/meta_architecture.py:843-853, :899-905) in torch's CPU operation order.  out (K, T, out_h, out_w) float.
 */
int dvis_resize2(const float *logits, int64_t stride_k, int64_t stride_t, int K, int T, int h, int w, int first_h,
                 int first_w, int img_h, int img_w, int out_h, int out_w, int sigmoid, float *out, void *stream);

/*
 * Semantic arg-max of a clip in one pass (inference_video_vss, dvis_Plus/meta_architecture.py:954-979):
 *   prob_q as in dvis_vps_argmax; out[t][y][x] = argmax_c sum_q cls[q][c] * prob_q[t][y][x]   (first maximum wins).
 *   logits: Q x T maps of h*w floats at logits + q*stride_q + t*stride_t; cls: Q rows of cls_row_stride floats, the
 *   first C valid and the rest ZERO (cls_row_stride = C rounded up to a multiple of 32, <= 128), 16-byte aligned.
 *   out (T, out_h, out_w) int64 class indices.
 */
int dvis_vss_argmax(const float *logits, int64_t stride_q, int64_t stride_t, const float *cls, int cls_row_stride, int Q,
                    int C, int T, int h, int w, int first_h, int first_w, int img_h, int img_w, int out_h, int out_w,
                    int64_t *out, void *stream);

/*
 * HOST function: how the four entry points above would run a problem, without launching anything (no GPU needed; only sizes are
 * read).  The launches take their grid and their dispatch from the same function, so the answer is what runs.
 *   op: DVIS_POST_*;  K: the candidates (Q for DVIS_POST_VSS_ARGMAX);  C, cls_row_stride: DVIS_POST_VSS_ARGMAX only, as in the call;
 *   T, img_h, img_w, out_h, out_w: as in the call (the stride-4 and padded sizes decide nothing here).
 *   plan[0] = workgroups launched (256 threads each);  0 when the call launches nothing (T == 0, or K == 0 of the resizes)
 *   plan[1] = grid-stride sweeps = ceil(work items / (workgroups * items per workgroup and sweep)).  A work item is one output pixel
 *             (T out_h out_w of them; vps_argmax and the generic vss_argmax: at most 256 * 16 workgroups of 256), one float
 *             (K T out_h out_w; resize2: at most 256 * 64 of 256), one group of 4 pixels of a row (K T out_h ceil(out_w / 4);
 *             resize2_gt0: at most 256 * 64 of 256) or one 32-pixel wave chunk (ceil(T out_h out_w / 32); the MFMA vss_argmax:
 *             at most 256 * 9 workgroups of 4)
 *   DVIS_POST_VSS_ARGMAX only, 0 otherwise:
 *   plan[2] = 1: the MFMA form (cls_row_stride == 128, Q % 4 == 0, img == out and Q * 132 * 4 bytes <= 64 KB of LDS, that is
 *             Q <= 124), 0: the generic one-pixel-per-thread form
 *   plan[3] = K4 = cls_row_stride / 4 (8, 16, 24 or 32): the float4 of class sums a thread of the generic form holds, its instance
 *   plan[4] = 1: img == out, the second resize is the identity (the generic form's prefetching branch; required by the MFMA form)
 *   plan[5] = dynamic LDS bytes of the launch (Q * 132 * 4 on the MFMA form, else 0)
 * The size checks of the call itself apply and refuse with the call's message (K must be 1..256; C must be 1..128; the row stride).
 */
enum {
  DVIS_POST_VPS_ARGMAX = 0,
  DVIS_POST_VSS_ARGMAX = 1,
  DVIS_POST_RESIZE2 = 2,
  DVIS_POST_RESIZE2_GT0 = 3
};
int dvis_postprocess_plan(int op, int K, int C, int cls_row_stride, int T, int img_h, int img_w, int out_h, int out_w, int32_t *plan);

/*
 * HOST function: minimum-cost assignment of an nr x nc (nr <= nc) row-major double cost matrix,
 * shortest-augmenting-path (Jonker-Volgenant / Crouse 2016) like scipy.optimize.linear_sum_assignment;
 * col4row[i] = column assigned to row i.  Returns 0, or DVIS_E_ARG for nan/-inf entries or nr > nc.
 */
int dvis_lsap_solve(const double *cost, int nr, int nc, int64_t *col4row);

/*
 * HOST function: the tracker's per-clip matching recurrence (ReferringTracker_noiser.forward, dvis_Plus/tracker.py:283-291
 * + Noiser.match_embds) in one call.  cost (T, Q, Q) fp32 HOST memory, cost[i][c][r] = 1 - cos(cur_i[c], ref_i[r]) with
 * ref_i = the UN-permuted embeddings of frame i-1 (frame 0: the carried-over / own embeddings); the column
 * permutation by the previous frame's assignment is applied inside.  indices (T, Q) int64 out.
 */
int dvis_match_chain(const float *cost, int T, int Q, int64_t *indices);

/*
 * Deterministic exact-fp32 GEMM (v_mfma_f32_16x16x4_f32, no atomics, no inter-workgroup waiting):
 *   C[b][m][n] = act( sum_k A[b][m][k] * W[b][n][k] + bias[n] + res[b][m][n] ),   act = 0: identity, 1: ReLU
 * A (M x K, row stride lda), W (N x K, row stride ldw) — i.e. F.linear's weight layout —, C (M x N, row stride ldc),
 * res optional (row stride ldres), bias optional (N); strides in floats; `batch` independent problems at the batch
 * strides (0 = operand shared by the batch).  Needs K, lda, ldw, strideA, strideW multiples of 4 and 16-byte aligned
 * A / W (returns DVIS_E_ARG otherwise).  The summation order of an output element depends on (M, N, K, batch, config)
 * only: two calls with the same arguments return bit-identical results.  config: -1 = chosen from the sizes, else an
 * index < dvis_gemm_num_configs() (tile / K-split variants; tuning aid).
 */
int dvis_gemm_nt(const float *A, int64_t lda, int64_t strideA, const float *W, int64_t ldw, int64_t strideW,
                 const float *bias, const float *res, int64_t ldres, int64_t strideRes, float *C, int64_t ldc,
                 int64_t strideC, int M, int N, int K, int batch, int act, int config, void *stream);
/* Same as dvis_gemm_nt with a bias PER BATCH ENTRY (strideBias floats apart; 0 = dvis_gemm_nt): `batch` projections with
 * their own weights and biases as one launch — the out-projections of the referring tracker's six cross-attention layers,
 * whose attention does not depend on the layer chain (dvis_Plus/tracker.py:293-318: q = reference, k / v = the frame's queries
 * in every layer), batched per frame. */
int dvis_gemm_nt_bb(const float *A, int64_t lda, int64_t strideA, const float *W, int64_t ldw, int64_t strideW,
                    const float *bias, int64_t strideBias, const float *res, int64_t ldres, int64_t strideRes, float *C,
                    int64_t ldc, int64_t strideC, int M, int N, int K, int batch, int act, int config, void *stream);
int dvis_gemm_num_configs(void);
/* The configuration dvis_gemm_nt(config = -1) would choose for these sizes.  A row's result depends on (N, K, config) only,
 * so a caller that wants the SAME bits for a row whether it is computed alone or stacked with other rows (the tracker run
 * for one clip or for two clips at once) pins the configuration of the smaller problem. */
int dvis_gemm_pick_config(int M, int N, int K, int batch);
/* Configuration for these sizes INSIDE the K-split family of `nw` waves (1, 4 or 8; -1 otherwise): all configurations of a
 * family sum an output element's products in the same order, so a row's bits depend on (N, K, nw) only — not on M.  The
 * per-frame segmenter folds the frames of a clip into the batch (dvis_Plus/video_mask2former_transformer_decoder.py:327-335);
 * taking its GEMMs from one family makes a frame's result independent of how many frames share the call (a rank's shard of a
 * clip vs the whole clip: north_star's frame sharding).  dvis_gemm_config_waves: the family of a configuration. */
int dvis_gemm_pick_config_nw(int M, int N, int K, int batch, int nw);
int dvis_gemm_config_waves(int config);

/*
 * GEMM with the LayerNorm(s) of the post-norm transformer blocks folded into its A-operand prologue:
 *   X = LN2( LN1(A) + ADD ),   C = act( X W^T + bias + res ),   a_out = X
 * LN1 / LN2 = LayerNorm over the K columns of a row (two-pass mean / centred variance, eps1 / eps2) with affine
 * (gamma, beta); each is skipped when its gamma is NULL, ADD (M x K, row stride ldadd) when NULL; a_out (M x K, optional)
 * receives the normalised rows.  Replaces the `tgt = norm(identity + attn(...))` / `tgt = norm(tgt + ffn(tgt))` seams of
 * ReferringCrossAttentionLayer / SelfAttentionLayer / FFNLayer (dvis_Plus/tracker.py:45-52,
 * mask2former_video/.../video_mask2former_transformer_decoder.py:47-50,166-170) between two projections: the producing
 * dvis_gemm_nt writes the raw residual sum, the consumer normalises it while its weight fragments are in flight — no
 * LayerNorm launch, no inter-workgroup hand-off.  Forms: none / LN1 / ADD + LN2 / LN1 + ADD + LN2.  K % 16 == 0, K <= 512 (2048
 * without norms), N % 4 == 0, row strides % 4 == 0, 16-byte aligned
 * operands (dvis_gemm_ln_supported; DVIS_E_ARG otherwise).  Deterministic: a row's result depends on (N, K, config) only.
 */
int dvis_gemm_ln(const float *A, int64_t lda, const float *add, int64_t ldadd, const float *gamma1, const float *beta1,
                 float eps1, const float *gamma2, const float *beta2, float eps2, float *a_out, int64_t ldaout,
                 const float *W, int64_t ldw, const float *bias, const float *res, int64_t ldres, float *C, int64_t ldc,
                 int M, int N, int K, int act, int config, void *stream);
/* norms != 0: the call carries LayerNorms / ADD (K <= 512); a plain call (the "everything in one memory round trip" form of
 * dvis_gemm_nt for launch-bound chains) reaches K <= 2048. */
int dvis_gemm_ln_supported(int M, int N, int K, int norms);
int dvis_gemm_ln_num_configs(void);
int dvis_gemm_ln_pick_config(int M, int N, int K);

/*
 * Tall fp32 GEMMs (M = every pixel of every frame, K = 256) on the F16 matrix cores with fp32-grade results: each fp32
 * operand v is carried as two f16 terms hi = rn16(v 2^e), lo = rn16(v 2^e - hi) (22 significand bits) and each product as
 * three matrix-core products lo*hi + hi*lo + hi*hi accumulated in fp32; the result is scaled back by 2^-(xexp + wexp).
 * Measured against fp64 the error is that of an fp32 GEMM (its accumulation rounding dominates; tests/test_gemm_x3_gpu.py).
 * xexp / wexp / hexp: the power-of-two exponents the activations / weights / hidden activations are scaled by before the
 * split; |v 2^e| must stay below 65520 (f16 range: from 65520 on the hi term rounds to +-inf).
 *
 * dvis_x3_pack: W (N x K, row stride ldw) -> `packed` (dvis_x3_packed_bytes(N, K) bytes), the kernels' LDS image (1 KB
 * fragments [pass][k-step][row block][hi, lo][lane][8 halves]; N = 288: ten row blocks per k-step, the tenth zero, so that an item's
 * pieces divide among the streaming kernel's 8 waves — dvis_x3_packed_bytes(288, K) = 320 K 4).  Once per weight.
 */
int64_t dvis_x3_packed_bytes(int N, int K);
/* The dvis_x3_* / dvis_conv*_x3 kernels are persistent (one workgroup per CU for the length of the launch).  A host that runs a
 * second stream of small kernels next to them (DVIS_Plus_offline.stream(): the previous clip's tracker chain) leaves `cus` CUs
 * (a multiple of 8) out of their grids; returns the previous setting.  Default 0 (env DVIS_X3_RESERVE). */
int dvis_x3_set_reserve(int cus);
/* Range guard of the split-f16 kernels.  The reference computes this path in fp32 (an explicit fp32 island,
 * mask2former/modeling/pixel_decoder/msdeformattn.py:314,320): no activation magnitude breaks it.  Here an activation with
 * |v 2^xexp| >= 65520 becomes (inf, -inf) in the split and its output row non-finite; the epilogues' ReLU keeps a NaN (as torch.relu does), but a
 * pre-activation of -inf would still leave it as 0.  Every dvis_x3_* / dvis_conv*_x3 launch therefore tests its PRE-activation outputs
 * (an operand-image epilogue also the values it stores against the image's own exponent) and, on a non-finite value,
 * stores the launch's tag (dvis_x3_set_tag, per host thread, > 0; returns the previous tag) into the int32 device word
 * registered for the current device (dvis_x3_set_range_flag; NULL = guard off, the default).  The word is sticky: the host
 * zeroes it, reads it once per clip and maps the tag back to the layer (dvis_plus_amd/functions.py: X3RangeError). */
int dvis_x3_set_range_flag(int32_t *device_word);
int dvis_x3_set_tag(int tag);
int dvis_x3_pack(const float *W, int64_t ldw, int N, int K, int wexp, void *packed, void *stream);
/* which (N, K) the projection kernels serve (ln != 0: the LayerNorm form) */
int dvis_x3_linear_supported(int N, int K, int ln);
/* out (M x N, row stride ldo) = act( x (M x K, row stride ldx) W^T + bias ),  act = ReLU if relu != 0; bias may be NULL.
 * Replaces nn.Linear over the flattened (frames x pixels) batch: ms_deform_attn.py:96-99 (value_proj), :101-102
 * (sampling_offsets | attention_weights as one stacked weight), and the masked-attention decoder's key / value projections of
 * every pixel for all layers of a level at once (mask2former_video/.../video_mask2former_transformer_decoder.py:81-88,
 * nn.MultiheadAttention in_proj), and the DINOv2 blocks' qkv / proj / fc1 / fc2 over every token of every frame
 * (mask2former/modeling/backbones_vitAdapter/.../vision_transformer blocks).  K % 64 == 0; N in {128, 192, 256} or N % 256 == 0
 * (output features in passes of 256 over one tile of x); N = 288 at K = 256. */
int dvis_x3_linear(const float *x, int64_t ldx, int64_t M, int K, const void *packed, int N, int xexp, int wexp,
                   const float *bias, int relu, float *out, int64_t ldo, void *stream);
/* The same with the activations x[t] + xadd[t mod xadd_rows] (xadd: xadd_rows x K, the position embedding shared by the frames;
 * the sum is formed in registers and never written): `query = with_pos_embed(src, pos)` in front of sampling_offsets /
 * attention_weights, msdeformattn.py:99-101,122, and the decoder's keys `with_pos_embed(memory, pos)`,
 * video_mask2former_transformer_decoder.py:81-88.  K = 256 (the row's fragments stay in registers for every pass over N). */
int dvis_x3_linear_add(const float *x, int64_t ldx, int64_t M, int K, const void *packed, int N, int xexp, int wexp,
                       const float *xadd, int64_t xadd_rows, const float *bias, int relu, float *out, int64_t ldo, void *stream);
/* dvis_x3_linear / dvis_x3_linear_add on rows read WHERE THEY LIE in a (batches, S, K) tensor: row r of the call (0 <= r < M,
 * M a whole number of batches) is at x + (r / rows_per_batch) * batch_stride + (r % rows_per_batch) * ldx floats — one level's rows
 * of every frame of the encoder memory, without the compaction a single row stride needs.  batch_stride % 4 == 0 and
 * >= rows_per_batch * ldx; xadd's row stays r mod xadd_rows; out is M x N with the single stride ldo.  The same summation order per
 * row as the single-stride entries (the same bits).  Served for N % 256 == 0 (K = 256 for the _add form). */
int dvis_x3_linear_rows(const float *x, int64_t ldx, int64_t rows_per_batch, int64_t batch_stride, int64_t M, int K, const void *packed,
                        int N, int xexp, int wexp, const float *bias, int relu, float *out, int64_t ldo, void *stream);
int dvis_x3_linear_add_rows(const float *x, int64_t ldx, int64_t rows_per_batch, int64_t batch_stride, int64_t M, int K,
                            const void *packed, int N, int xexp, int wexp, const float *xadd, int64_t xadd_rows, const float *bias,
                            int relu, float *out, int64_t ldo, void *stream);
/* dvis_x3_linear with the activation chosen by `act` (0 none, 1 ReLU, 2 the exact GELU of nn.GELU(): 0.5 t (1 + erf(t / sqrt 2)))
 * and an optional residual added AFTER it: out = act(x W^T + bias) + res (res: M x N, row stride ldres floats, 16-byte aligned; may
 * alias nothing the kernel writes).  The ViT blocks of the DINOv2 / ViT-Adapter backbones (mask2former/modeling/
 * backbones_vitAdapter: `x = x + ls1(attn(norm1(x)))`, `Mlp: fc2(act(fc1(x)))`) take their GELU and their residual adds here
 * instead of in two more passes over the 452 MB token tensor of a 30-frame clip. */
int dvis_x3_linear_res(const float *x, int64_t ldx, int64_t M, int K, const void *wp, int N, int xexp, int wexp, const float *bias, int act,
                       const float *res, int64_t ldres, float *out, int64_t ldo, void *stream);

/*
 * The same `out = act(x W^T + bias) + res` for the LARGE tall GEMMs of the ViT blocks (K = 1024 .. 4096; qkv / proj / fc1 / fc2 of
 * mask2former/modeling/backbones_vitAdapter at 110 430 tokens per 30-frame clip), csrc/gemm_x3_tile.hip: workgroup tiles of
 * 128 tokens x 256 features with BOTH operands staged through LDS (the rows split into their two f16 terms once per tile), so a
 * row tile is read once per 256 output features from the L2 of the XCD that owns it — the streaming kernels above re-read and
 * re-split it per pass from HBM.  N % 256 == 0, K % 32 == 0 (dvis_x3_tile_supported); weights packed once with dvis_x3_tile_pack
 * into dvis_x3_tile_packed_bytes(N, K) bytes (the LDS image per (feature tile, k-step of 16), scaled by 2^wexp; order 0, or the
 * order of a row image's producer, below).
 * A row's result does not depend on M.  Same range guard as the other split-f16 kernels.
 */
int dvis_x3_tile_supported(int N, int K);
int64_t dvis_x3_tile_packed_bytes(int N, int K);
int dvis_x3_tile_pack(const float *w, int64_t ldw, int N, int K, int wexp, int order, void *packed, void *stream);
int dvis_x3_tile_linear(const float *x, int64_t ldx, int64_t M, int K, const void *wp, int N, int xexp, int wexp, const float *bias, int act,
                        const float *res, int64_t ldres, float *out, int64_t ldo, void *stream);
/* The ViT blocks' fused qkv projection + attention operands (backbones_vitAdapter attention: `qkv = self.qkv(x)`, then softmax(q k^T
 * / sqrt(d)) v per head): dvis_x3_tile_linear_qkv computes x W^T + bias for N = 3 * heads * 64 columns ordered (q | k | v, head, dim)
 * and writes, instead of the fp32 qkv tensor, the two-term f16 operand images of the split-f16 attention kernel into `ws`
 * (dvis_attention_ws_bytes_k(B * heads, L, L, 64, 2) bytes; rows of x = B batch entries of L tokens; qscale = softmax scale x log2(e)
 * x 2^4); dvis_attention_x3_packed then runs that kernel's main launch on `ws` (out: (B, heads, L, 64) view, strides in floats as in
 * dvis_attention_forward_k).  Saves the 1.36 GB qkv tensor's write + re-read and the pack launch per block. */
int dvis_x3_tile_linear_qkv(const float *x, int64_t ldx, int64_t M, int K, const void *wp, int N, int xexp, int wexp, const float *bias,
                            int heads, int L, float qscale, void *ws, void *stream);
int dvis_attention_x3_packed(const void *ws, float *out, const int64_t *o_strides, int B, int heads, int L, void *stream);
/*
 * ROW IMAGES (round 6): the row operand of the tiled GEMM pre-split by its PRODUCER — [row tile of 128][k-tile of 16][hi, lo][chunk of
 * 8 k][128 rows][8 halves], values x 2^xexp, dvis_x3_rows_image_bytes(M, K) bytes (the fp32 tensor's size, rows padded to 128) — so
 * that both operands of the ViT blocks' GEMMs (block.py:36-104: norm1 -> qkv -> attention -> proj, norm2 -> fc1 -> GELU -> fc2) are
 * LDS-DMA streams and no fp32 activation is written between a normalisation / activation / attention and the GEMM behind it.
 *   producers: dvis_x3_rows_image (fp32 rows; k order 0), dvis_layernorm_rows_image (LayerNorm of fp32 rows, C <= 1024; order 0),
 *              dvis_x3_tile_linear_image with act = 2 (GELU; order 1), dvis_attention_x3_packed_image (order 2);
 *   consumers: dvis_x3_tile_linear_image (act 0 / 1: fp32 rows out, + residual), dvis_x3_tile_linear_qkv_image; their weights
 *              packed with dvis_x3_tile_pack(order of the image's producer): the k slots of a k-tile are a free permutation
 *              as long as both operands use the same one.
 * Rows past M of the last row tile are written as zeros by every producer.  Results per row as dvis_x3_tile_linear (the same three
 * products per k-tile, fp32 accumulate; orders 1 / 2 add the k-tile's terms in another order).
 */
int64_t dvis_x3_rows_image_bytes(int64_t M, int K);
int dvis_x3_rows_image(const float *x, int64_t ldx, int64_t M, int K, int xexp, void *image, void *stream);
int dvis_layernorm_rows_image(const float *x, const float *gamma, const float *beta, int64_t M, int C, float eps, int xexp, void *image,
                              void *stream);
int dvis_x3_tile_linear_image(const void *ximg, int64_t M, int K, const void *wp, int N, int xexp, int wexp, const float *bias, int act,
                              const float *res, int64_t ldres, float *out, int64_t ldo, void *oimg, int oexp, void *stream);
int dvis_x3_tile_linear_qkv_image(const void *ximg, int64_t M, int K, const void *wp, int N, int xexp, int wexp, const float *bias, int heads,
                                  int L, float qscale, void *ws, void *stream);
int dvis_attention_x3_packed_image(const void *ws, void *image, int B, int heads, int L, int xexp, void *stream);
/* out = LayerNorm( x W^T + bias + res ) over the N = 256 features (gamma, beta, eps; two-pass statistics as torch);
 * pos (pos_rows x N, optional): out2[t] = out[t] + pos[t mod pos_rows] (the next layer's `with_pos_embed(src, pos)`,
 * msdeformattn.py:99-101,122).  Replaces output_proj + `src = norm1(src + dropout1(src2))`, msdeformattn.py:124-125. */
int dvis_x3_linear_ln(const float *x, int64_t ldx, int64_t M, int K, const void *packed, int N, int xexp, int wexp,
                      const float *bias, const float *res, int64_t ldres, const float *gamma, const float *beta, float eps,
                      const float *pos, int64_t pos_rows, float *out, float *out2, int64_t ldo, void *stream);
/* The FFN block in one kernel: out = LayerNorm( x + linear2( relu( linear1(x) ) ) ), K = N = 256, H % 128 == 0; the
 * (M x H) hidden tensor is never written.  Replaces forward_ffn, msdeformattn.py:116-120 (+ :130).
 * dvis_x3_ffn_pack interleaves W1 (H x K) and W2 (N x H) in the order the kernel streams them (W2's k in accumulator order). */
int64_t dvis_x3_ffn_packed_bytes(int K, int H, int N);
/*
 * The compute-bound 1x1 convolutions of the R50 bottlenecks in the same arithmetic, on NCHW:
 *   y (N, K, OH, OW) = relu?( w (K, C) x (N, C, H, W)[:, :, ::stride, ::stride] + bias[k] + res ),  stride 1 or 2,
 * bias (K) / res (N, K, OH, OW) optional.  Replaces conv1 / conv3 / the stride-2 shortcut of detectron2's BottleneckBlock with
 * the FrozenBN folded by the caller (`build_resnet_backbone`, configs/dvis_Plus/.../Base-*.yaml:2-16).
 * C % 64 == 0, K = 64 / 128 or K % 256 == 0, every tensor below 2 GiB (dvis_conv1x1_x3_supported).  `packed`: dvis_conv1x1_x3_pack
 * of the (K x C) weight, dvis_conv1x1_x3_packed_bytes(C, K) bytes.
 */
int dvis_conv1x1_x3_supported(int C, int K, int64_t N, int64_t HW_in, int64_t HW_out);
int64_t dvis_conv1x1_x3_packed_bytes(int C, int K);
int dvis_conv1x1_x3_pack(const float *w, int K, int C, int wexp, void *packed, void *stream);
/* The GroupNorm around a convolution, folded into the launch (the pixel decoder's mask path; all NULL / 0 = the plain launch):
 *   in_scale / in_shift (N * C)  x is read as in_relu?(x * in_scale[n*C + c] + in_shift[n*C + c]): dvis_scale_shift_act's arithmetic
 *                                on the way into the split, without its pass over the map; stride 1, C = 256;
 *   gn_part                      N * (K / 8) * (H * W / 32) * 2 doubles: per (image, group of 8 channels, 32 pixels) the sum and
 *                                the sum of squares of y as stored — dvis_group_norm_finalize turns them into GroupNorm(K / 8, K)'s
 *                                (scale, shift).  Every element is written; a function of the image's data alone.
 * Either needs dvis_conv_x3_gn_fold_supported(K, K / 8, H * W): K % 256 == 0, H * W % 32 == 0; one of the two per launch. */
int dvis_conv_x3_gn_fold_supported(int K, int G, int64_t HW);
int dvis_conv1x1_x3(const float *x, const void *packed, const float *bias, const float *res, float *y, int N, int C, int K, int H,
                    int W, int stride, int xexp, int wexp, int relu, void *stream, const float *in_scale, const float *in_shift,
                    int in_relu, double *gn_part);
/* The last 1x1 convolution of a down-sampling bottleneck TOGETHER with its shortcut (detectron2 BottleneckBlock with a
 * projection shortcut, SURVEY.md App. B: out = relu(conv3(a) + shortcut(x))): one accumulation over the concatenated channels
 * [a (N, C, H, W) | x2 (N, C2, H2, W2) sampled with stride2], `packed` = dvis_conv1x1_x3_pack of the (K, C + C2) matrix
 * [W3 | Ws], bias = b3 + bs.  The shortcut's (N, K, H, W) map is neither written nor read back. */
int dvis_conv1x1_x3_dual(const float *x, const float *x2, const void *packed, const float *bias, const float *res, float *y, int N,
                         int C, int C2, int K, int H, int W, int H2, int W2, int stride2, int xexp, int wexp, int relu, void *stream);
/* The 3x3 / padding 1 / stride 1 or 2 convolution through the same kernel: nine taps = nine times the input channels, each
 * chunk of 64 channels read at the tap's pixel (outside the image: an out-of-range buffer offset, i.e. exact zero padding).
 * w (K, C, 3, 3).  Serves the stride-2 conv2 of the first res3 / res4 / res5 bottleneck (detectron2 BottleneckBlock). */
int64_t dvis_conv3x3_x3_packed_bytes(int C, int K);
int dvis_conv3x3_x3_pack(const float *w, int K, int C, int wexp, void *packed, void *stream);
int dvis_conv3x3_x3(const float *x, const void *packed, const float *bias, const float *res, float *y, int N, int C, int K, int H,
                    int W, int stride, int xexp, int wexp, int relu, void *stream);
/*
 * The res2 bottlenecks as a chain (csrc/bneck_x3.hip; detectron2 BottleneckBlock, 64 middle / 256 output channels):
 * one launch = conv2 (3x3) + ReLU -> conv3 + shortcut + ReLU -> the NEXT block's conv1 + ReLU, per 32-pixel group, without
 * conv2's map or a second read of the block output touching memory.  The 64-channel maps between blocks are OPERAND IMAGES:
 * per group (n, y, x / 32) 8 KB = [k-step][hi, lo f16 term][32 g + x % 32][8 halves] in accumulator channel order
 * (dvis_bneck_x3_image_bytes(N, H, W) bytes), written by dvis_conv1x1_x3_image (the stage's first conv1) or by the previous
 * dvis_bneck_x3.  res: the identity shortcut (N, 256, H, W); or NULL with x2 = the block input (N, 64, H, W) and a stream packed
 * with the projection shortcut ws (first block).  out: NULL (last block: no chained conv1, packed without w1) or the next image.
 * y (N, 256, H, W); b2 / b3 (+ bs) / b1: folded-BN shifts (64 / 256 / 64).  e2 / e3 / e1: the weights' scaling exponents.
 */
int dvis_bneck_x3_supported(int64_t N, int H, int W);
int64_t dvis_bneck_x3_image_bytes(int64_t N, int H, int W);
int64_t dvis_bneck_x3_packed_bytes(int tail, int dual);
int dvis_bneck_x3_pack(const float *w2, const float *w3, const float *ws, const float *w1, int e2, int e3, int e1, void *packed,
                       void *stream);
int dvis_bneck_x3(const void *a1, const float *res, const float *x2, const void *packed, const float *b2, const float *b3,
                  const float *b1, float *y, void *out, int N, int H, int W, int xexp, int e2, int e3, int e1, void *stream);
int dvis_conv1x1_x3_image(const float *x, const void *packed, const float *bias, void *image, int N, int C, int H, int W, int xexp,
                          int wexp, int oexp, int relu, void *stream);
/*
 * Operand images on either side of csrc/conv1x1_x3.hip (the maps INSIDE the res3 - res5 bottlenecks and the FPN output convolution's
 * input): C channels = C / 64 chunks of 8 KB per 32-pixel group (n, y, x / 32), each [k-step][hi, lo f16 term][32 g + x % 32][8 halves]
 * in accumulator channel order.  The producer's epilogue splits once; a 3x3 consumer's nine taps re-read the image: 8 loads of 16 bytes
 * per 64-channel chunk and lane instead of 32 of 4 bytes, no split arithmetic in the loop.
 *   dvis_conv_x3_pack_image  weights (K, C, taps 1 | 9) for an image-INPUT launch (channels of a chunk in accumulator order)
 *   dvis_conv_x3_image       relu?(conv + bias + res): ximg | x in, image | y out (at least one image); K = 128 or K % 256 == 0
 *   dvis_upsample_add_image  dvis_upsample_add with the sum written as an operand image (the FPN's top-down path)
 */
int64_t dvis_conv_x3_image_bytes(int64_t N, int C, int H, int W);
int dvis_conv_x3_pack_image(const float *w, int K, int C, int taps, int wexp, void *packed, void *stream);
int dvis_conv_x3_image(const void *ximg, const float *x, const void *packed, const float *bias, const float *res, float *y, void *image,
                       int N, int C, int K, int H, int W, int stride, int taps, int xexp, int wexp, int oexp, int relu, void *stream,
                       double *gn_part);      /* gn_part: as dvis_conv1x1_x3 (image in, fp32 map out), or NULL */
int dvis_upsample_add_image(const float *lateral, const float *lat_scale, const float *lat_shift, const float *top, void *image, int N,
                            int C, int H, int W, int h, int w, int oexp, void *stream);
/* dvis_upsample_add_image has two kernels that write the same bytes.  The second one (16-byte lateral loads, the block's top taps
 * staged once in LDS, the fragments transposed through LDS) serves shapes with dvis_upsample_add_image_v2_supported — W % 4 == 0, a
 * 16-byte aligned lateral, up-sampling by about 2 or more — unless DVIS_UPSAMPLE_IMAGE_V2=0 / dvis_upsample_add_image_set_v2(0); every
 * other shape takes the first.  _set_v2 returns the previous setting (on < 0: reads it only).
 * dvis_upsample_add_image_tokens: `top` read where it lies in a token-major (N, S, C) tensor, the map's h * w tokens at rows
 * [row0, row0 + h * w) of every frame (the finest level of the encoder memory, never transposed to a map); v2-supported shapes only. */
int dvis_upsample_add_image_v2_supported(int N, int C, int H, int W, int h, int w);
int dvis_upsample_add_image_set_v2(int on);
int dvis_upsample_add_image_tokens(const float *lateral, const float *lat_scale, const float *lat_shift, const float *tokens, int64_t S,
                                   int64_t row0, void *image, int N, int C, int H, int W, int h, int w, int oexp, void *stream);
int dvis_x3_ffn_pack(const float *W1, int64_t ldw1, const float *W2, int64_t ldw2, int K, int H, int N, int w1exp, int w2exp,
                     void *packed, void *stream);
int dvis_x3_ffn_ln(const float *x, int64_t ldx, int64_t M, int K, int H, int N, const void *packed, int xexp, int w1exp,
                   int hexp, int w2exp, const float *b1, const float *b2, const float *gamma, const float *beta, float eps,
                   const float *pos, int64_t pos_rows, float *out, float *out2, int64_t ldo, void *stream);

/*
 * Video metrics (csrc/video_metrics.hip): integer counts over (T, H, W) int32 id maps, u64 atomics only — run-to-run identical.
 * Outputs are zeroed inside.  `bad` (one int64): pixels whose prediction lies outside the declared range (not counted elsewhere).
 *
 * dvis_pan_pair_hist: per-frame (GT segment, predicted segment) pixel counts, out (T, Ng + 2, Np + 1) int64.  GT rows: 0 = VOID
 *   (id 0), 1 + i = gt_table[i] (the video's GT ids, sorted ascending, non-zero, Ng <= 16384), Ng + 1 = an id that the table does
 *   not list (the reference skips those segments, utils/eval_vpq_vspw.py:167-170, but their pixels still count in the prediction
 *   areas); prediction columns 0..Np.  Replaces the np.unique of uint64 `gt * 2^24 + pred` tubes per window start and length
 *   (utils/eval_vpq_vspw.py:142-148) and the per-frame pair counts of utils/segmentation_and_tracking_quality.py:131-221.
 *   H * W < 2^31.
 */
int dvis_pan_pair_hist(const int32_t *gt, const int32_t *pred, const int32_t *gt_table, int Ng, int Np, int T, int64_t HW,
                       int64_t *out, int64_t *bad, void *stream);
/* dvis_sem_confusion: the class confusion of utils/eval_miou_vspw.py:_generate_matrix over n pixels, out (num_class, num_class) int64
 *   (num_class <= 256): gt taken as uint8, 0 -> 255, then - 1 in uint8, rows >= num_class dropped; bin = num_class * gt + pred (a
 *   prediction >= num_class lands in the next row, as in the reference's bincount); pred < 0 or a bin past the matrix -> bad. */
int dvis_sem_confusion(const int32_t *gt, const int32_t *pred, int64_t n, int num_class, int64_t *out, int64_t *bad, void *stream);
/* dvis_video_consistency: utils/eval_vc_vspw.py:get_common in one pass over the frames per pixel.  For each window length ks[j]
 *   (HOST array, 1 <= nk <= 4) and start i in the reference's range(T - k) (i < T - k; the last valid window is not scored there):
 *   gt_const[j][i] = pixels whose GT is constant over frames [i, i + k), both_const[j][i] = those whose prediction is constant
 *   there too.  Outputs (nk, T) int64, entries i >= T - k zero.  2 * nk * T <= 16384. */
int dvis_video_consistency(const int32_t *gt, const int32_t *pred, int T, int64_t HW, const int32_t *ks, int nk, int64_t *gt_const,
                           int64_t *both_const, void *stream);

/*
 * VIS scoring (csrc/vis_metrics.hip).  Masks are row-major (N, H, W) bytes (bool / uint8, non-zero = set), H * W < 2^31.  RLE is
 * COCO's: the runs of a mask's pixels in column-major order (index x * H + y), zeros first (a leading 0 when pixel (0, 0) is set).
 *
 * dvis_rle_encode: replaces the per-frame mask_util.encode of data_video/ytvis_eval.py:275-280.  Two phases around a host-side
 *   exclusive scan.  phase 0: trans (N, W, ceil(H / 128)) int64 = transitions per (mask, column, 128-row chunk), area (N) int64 =
 *   set pixels (zeroed inside).  phase 1: toff = the exclusive scan of trans (same shape), moff (N + 1) = each mask's first
 *   transition (moff[N] = the total); writes the transition positions to the int32 workspace bnd (moff[N] entries) and the runs,
 *   uint32, mask n's moff[n+1] - moff[n] + 1 runs starting at runs[moff[n] + n].
 */
int dvis_rle_encode(const uint8_t *masks, int64_t N, int H, int W, int phase, int64_t *trans, int64_t *area, const int64_t *toff,
                    const int64_t *moff, int32_t *bnd, uint32_t *runs, void *stream);
/* dvis_rle_strings: the `counts` strings of ytvis_eval.py:279-283 (cocoapi rleToString) for N masks whose runs (uint32) lie at
 *   run_off[n] .. run_off[n + 1].  chars == NULL: lens[n] = string length in bytes.  Else the string of mask n is written to
 *   chars + str_off[n] (no terminator). */
int dvis_rle_strings(const uint32_t *runs, const int64_t *run_off, int64_t N, const int64_t *str_off, int64_t *lens, uint8_t *chars,
                     void *stream);
/* dvis_rle_decode: ground-truth RLE -> masks, replacing the annToRLE / merge of ytvis_api/ytvos.py:268-287 and ytvoseval.py:206-213.
 *   ends: per mask the cumulative run ends (int32; mask n's at run_off[n] .. run_off[n + 1], the last = H * W); out (N, H, W) uint8
 *   0 / 1. */
int dvis_rle_decode(const int32_t *ends, const int64_t *run_off, int64_t N, int H, int W, uint8_t *out, void *stream);
/* dvis_track_intersections: the intersections of ytvoseval.py:203-217's iou_seq for all P x G track pairs of one video, out (P, G)
 *   int64 = sum over frames t < T of |pred[p, t] & gt[g, t]|; frame t of track k at base + k * stride + t * HW (byte strides).
 *   accumulate != 0 adds to out (frame chunks), else out is zeroed first.  (P + G) * 128 + P * G * 4 <= 65536. */
int dvis_track_intersections(const uint8_t *pred, int64_t pred_stride, int P, const uint8_t *gt, int64_t gt_stride, int G, int T,
                             int64_t HW, int accumulate, int64_t *out, void *stream);

/*
 * Prediction files (csrc/pred_write.hip): integer only, run-to-run identical.  Maps are contiguous (T, H, W) int32; the paint
 * kernels take them as one flat run of npx = T * H * W pixels and need `map` and `out` 16-byte aligned.
 *
 * dvis_pan_segment_stats: replaces the per-segment `pan_seg_result == id`, mask[i].sum() and np.where bbox of
 *   data_video/vps_eval.py:112-143.  out (T, n + 1, 5) int64 = per frame and id 0..n: area, xmin, ymin, xmax, ymax (inclusive
 *   pixel coordinates; all five zero where the id has no pixel).  bad (one int64) = pixels whose id lies outside 0..n (the
 *   reference ignores ids that segments_infos does not list).  Outputs are zeroed inside.  H * W < 2^31, n < 2^30.
 */
int dvis_pan_segment_stats(const int32_t *map, int T, int H, int W, int n, int64_t *out, int64_t *bad, void *stream);
/* dvis_pan_paint_rgb: replaces `pan_format[mask] = color` of data_video/vps_eval.py:121-123.  out (npx, 3) uint8 = the colour
 *   lut[id] (0x00BBGGRR, nlut entries) of every pixel as r, g, b bytes; ids outside 0..nlut - 1 become (0, 0, 0). */
int dvis_pan_paint_rgb(const int32_t *map, int64_t npx, const int32_t *lut, int nlut, uint8_t *out, void *stream);
/* dvis_sem_paint: replaces the astype(np.uint8) and per-class id mapping of data_video/vss_eval.py:93-100.  out (npx) uint8 =
 *   lut[map & 255], lut (256 int32, device) = the dataset id 0..255 of each class byte (255 for the ignore label), or -1 when the
 *   class has no mapping: such pixels are written as 255 and counted in bad[class] (256 int64, zeroed inside), so the host can
 *   raise the reference's KeyError. */
int dvis_sem_paint(const int32_t *map, int64_t npx, const int32_t *lut, uint8_t *out, int64_t *bad, void *stream);

/*
 * dvis_resize_frames_u8 (csrc/frame_resize.hip): Pillow's 8-bit BILINEAR resample (ImagingResample, PRECISION_BITS = 22) of
 *   T uint8 HWC frames in (T, H, W, 3) to out (T, 3, h, w) uint8 CHW, byte-identical to Image.resize((w, h), BILINEAR).
 *   xtab (w, kx + 2) / ytab (h, ky + 2) int32 (device): per output index [first input index, taps, kx / ky fixed-point
 *   coefficients], Pillow's precompute_coeffs + normalize_coeffs_8bpc (built on the host: functions.resize_tables).  Horizontal
 *   pass first, vertical second, each clip8(2^21 + sum in * coef); an unchanged axis takes the identity table [x, 2, 2^22, 0].
 *   reverse != 0: plane c of the output is input channel 2 - c (BGR <-> RGB).  `in` and `out` 16-byte aligned.  Integer only,
 *   run-to-run identical.  DVIS_E_UNSUPPORTED when a 4 x 1 output tile's inputs exceed 64 KB of LDS (down-scales by ~100x).
 */
int dvis_resize_frames_u8(const uint8_t *in, int T, int H, int W, uint8_t *out, int h, int w, const int32_t *xtab, int kx,
                          const int32_t *ytab, int ky, int reverse, void *stream);

/*
 * Set-prediction supervision (csrc/criterion.hip): the matching cost of VideoHungarianMatcher / HungarianMatcher
 * (mask2former_video/modeling/matcher.py:107-151) and the point-sampled mask losses of VideoSetCriterion / SetCriterion
 * (mask2former_video/modeling/criterion.py:21-67, :150-200).  Sampling everywhere is F.grid_sample(x, 2 c - 1, bilinear, zeros,
 * align_corners=False) at normalised points c = (x, y) in [0, 1]: pixel coordinate c * W - 0.5, taps outside the map are zero.
 * fp32 arithmetic; every map is contiguous; a target map is fp32 (tgt_u8 = 0) or one byte per pixel (uint8 / bool, tgt_u8 = 1).
 * Every forward result is run-to-run identical (fixed split of the points, partials added in index order, no float atomics).
 *
 * A prediction map is H x W, a target map Ht x Wt (the targets are at the padded image's size, the predictions at a quarter of
 * it): both are sampled at the same normalised points.
 * dvis_match_cost: pred (Q, T, H, W), tgt (G, T, Ht, Wt), coords (K, 2) shared by all masks and frames, logits (Q, NC),
 *   tgt_ids (G) int64 in [0, NC) ->  C (Q, G) = w_mask * cost_mask + w_class * cost_class + w_dice * cost_dice  and, when terms is
 *   not null, terms (3, Q, G) = [cost_class, cost_mask, cost_dice] unweighted:  cost_class = -softmax(logits)[q, ids[g]],
 *   cost_mask = sum_n (softplus(-x) t + softplus(x) (1 - t)) / (T K),  cost_dice = 1 - (2 sum sigmoid(x) t + 1) / (sum sigmoid(x) +
 *   sum t + 1)  over the T K sampled values x of query q and t of target g.  ws: dvis_match_cost_ws_bytes(Q, G, T, K) bytes.
 * dvis_point_sample_rows: rows (R, H, W) fp32 or bytes, coords (R, P, 2) -> out (R, P) fp32.
 * dvis_point_loss_fwd: src (R, H, W), tgt (R, Ht, Wt), coords (R, P, 2) -> out (R, 3) = per row [sum_p bce(x, t),
 *   a = sum_p sigmoid(x) t, b = sum_p sigmoid(x) + sum_p t].  ws: dvis_point_loss_ws_bytes(R) bytes.  R < 65536.
 * dvis_point_loss_bwd: grad_src (R, H, W) (zeroed inside, by a kernel) of  g_mask * sum_r mean_p bce / num_masks + g_dice *
 *   sum_r (1 - (2 a + 1) / (b + 1)) / num_masks;  sums = the forward's out, g_mask / g_dice = one DEVICE float each.  det_ws null:
 *   fp32 vector atomics (last bits vary run to run); det_ws = R * H * W * 8 bytes (8-byte aligned): 64-bit fixed-point
 *   accumulation, the same bits every run (targets in [0, 1]).
 */
int64_t dvis_match_cost_ws_bytes(int Q, int G, int T, int K);
int dvis_match_cost(const float *pred, const void *tgt, int tgt_u8, const float *coords, const float *logits,
                    const int64_t *tgt_ids, int Q, int G, int T, int H, int W, int Ht, int Wt, int K, int NC, float w_class,
                    float w_mask, float w_dice, float *C, float *terms, void *ws, void *stream);
int dvis_point_sample_rows(const void *rows, int rows_u8, const float *coords, int64_t R, int P, int H, int W, float *out,
                           void *stream);
int64_t dvis_point_loss_ws_bytes(int64_t R);
int dvis_point_loss_fwd(const float *src, const void *tgt, int tgt_u8, const float *coords, int R, int P, int H, int W, int Ht, int Wt,
                        float *out, void *ws, void *stream);
int dvis_point_loss_bwd(const float *src, const void *tgt, int tgt_u8, const float *coords, const float *sums, const float *g_mask,
                        const float *g_dice, int R, int P, int H, int W, int Ht, int Wt, float num_masks, float *grad_src,
                        void *det_ws, void *stream);

/*
 * Contrastive item losses of CTVIS's CTCLPlugin (csrc/contrastive_items.hip; dvis_Plus/ctvis.py:753-769, 817-861).
 * src (R, C) fp32, C % 4 == 0, 16-byte aligned.  Item i of n: anchor row anchor[i], positive rows pos_idx[pos_ptr[i] .. pos_ptr[i + 1]),
 * negative rows neg_idx[neg_ptr[i] .. neg_ptr[i + 1]) (int32, device; ptr arrays non-decreasing from 0, indices in [0, R): the
 * caller checks them where the lists still live on the host, the kernels clamp).  S = pos_ptr[n] + neg_ptr[n] slots in all; slot s
 * of item i (positives first) has the global number pos_ptr[i] + neg_ptr[i] + s.
 * dvis_contrastive_items: one launch ->  reid (n) = softplus(LSE_j(n_j . a) + LSE_k(-p_k . a)) (0 for an empty side),
 *   aux (n) = (sum_k (cos(p_k, a) - 1)^2 + sum_j cos(n_j, a)^2) / (P_i + N_i) with F.normalize's cosine (norms clamped at 1e-12);
 *   saved for the backward: dots (S), norms (S) per slot and stats (n, 3) = [LSE_neg, LSE_pos, |a|].  n = 0 launches nothing.
 * dvis_contrastive_items_backward: grad_src (R, C), every row written once (rows no item references: exactly 0), of
 *   sum_i grad_reid[i] reid[i] + grad_aux[i] aux[i].  row_ptr (R + 1) / occ_slot / occ_item: per source row its occurrences as a
 *   positive or negative, as (global slot, item), in (item, slot) order; arow_ptr (R + 1) / arow_item: the items a row anchors,
 *   ascending (functions.contrastive_items_transpose builds both on the host).  ws: dvis_contrastive_items_backward_ws_bytes(n,
 *   S, C) bytes, 16-byte aligned (-1 for bad sizes).  Exact fp32, no atomics, fixed reduction order: the same bits every call.
 * dvis_contrastive_items_tile: the slots one pass of a workgroup's per-item reductions covers.
 */
int dvis_contrastive_items_tile(void);
int dvis_contrastive_items(const float *src, int64_t R, int C, const int32_t *anchor, const int32_t *pos_ptr, const int32_t *pos_idx,
                           const int32_t *neg_ptr, const int32_t *neg_idx, int n, int64_t S, float *reid, float *aux, float *dots,
                           float *norms, float *stats, void *stream);
int64_t dvis_contrastive_items_backward_ws_bytes(int n, int64_t S, int C);
int dvis_contrastive_items_backward(const float *src, int64_t R, int C, const int32_t *anchor, const int32_t *pos_ptr,
                                    const int32_t *pos_idx, const int32_t *neg_ptr, const int32_t *neg_idx, int n, int64_t S,
                                    const int32_t *row_ptr, const int32_t *occ_slot, const int32_t *occ_item, const int32_t *arow_ptr,
                                    const int32_t *arow_item, const float *dots, const float *norms, const float *stats,
                                    const float *grad_reid, const float *grad_aux, float *grad_src, void *ws, void *stream);

/*
 * Shifted-window attention of the Swin backbone (csrc/window_attention.hip; mask2former/modeling/backbone/swin.py:131-171, 235-295,
 * 413-440): pad, cyclic shift, window partition, per-head relative-position bias, region mask, softmax, P V, window reverse, reverse
 * shift and crop in one launch.
 * qkv (B, H W, 3 C) fp32: the block's qkv projection on the UNPADDED token grid, columns [3][heads][d], C = heads * d;
 * qkv_bias (3 C) or null; bias_table ((2 ws - 1)^2, heads) raw; out (B, H W, C), columns [heads][d].  qkv, qkv_bias, out 16-byte aligned.
 * Hp = ceil(H / ws) ws, Wp likewise.  The token at shifted coordinate (ys, xs) comes from source ((ys + shift) % Hp, (xs + shift) %
 * Wp); a source at or beyond (H, W) is a pad token whose q / k / v is qkv_bias (zeros when null): the reference pads AFTER norm1.
 * Window (ys / ws, xs / ws) holds N = ws^2 tokens in row-major local order.  score(i, j) = scale q_i . k_j + table[(iy - jy + ws - 1)
 * (2 ws - 1) + (ix - jx + ws - 1)][head], plus -100 (additive) when shift > 0 and the region ids of i and j differ, region id of a
 * shifted coordinate = 3 r(ys, Hp) + r(xs, Wp), r(n, N) = (n >= N - ws) + (n >= N - shift).  Softmax over j with the row maximum
 * subtracted, times v.  Only rows at un-padded source positions are written (each exactly once).  0 <= shift < ws; the shift is
 * applied even when the map is smaller than one window.
 * Exact fp32 (v_mfma_f32_16x16x4_f32), no workspace, no atomics, no memset: capturable; the same bits every call, and a frame's
 * bits do not depend on B.  One frame's qkv must be below 2^31 bytes (per-frame bases are 64-bit).
 * dvis_window_attention_supported: 1 where (ws, d) is served (d = 32 with ws = 7 or 12); the call refuses every other pair.
 */
int dvis_window_attention_supported(int ws, int d);
int dvis_window_attention(const float *qkv, const float *qkv_bias, const float *bias_table, float *out, int B, int H, int W, int heads,
                          int d, int ws, int shift, float scale, void *stream);

/*
 * Mask pooling of the open-vocabulary (FC-CLIP) heads (csrc/mask_pool.hip; MaskPooling,
 * ov_dvis/video_mask2former_transformer_decoder_ov.py:39-67, without its mean):
 *   sum[b, q, c] = sum over the pixels p with logits[b, q, p] > 0 of x[b, c, p]      count[b, q] = the number of those pixels
 *   x (B, C, HW) contiguous; logits: (HW) planes, contiguous each, at logits + b * l_bstride + q * l_qstride (strides in ELEMENTS,
 *   l_qstride >= HW: a frame of the (1, Q, T, H, W) inference logits is pooled in place); sum (B, Q, C) fp32; count (B, Q) int32.
 * Membership is a select on the loaded logit: 0.0, -0.0 and NaN are outside, every positive value (denormals included) inside.  The
 * selected 0 / 1 operand and x go through the exact-fp32 MFMA (a k-ordered fma chain): a non-finite x of a frame reaches every row
 * of that frame, as through the reference's einsum, and no other frame.  The mean, its `+ 1e-8` and any combination over frames
 * are the caller's.
 * Served: 1 <= Q <= 256, C % 4 == 0 up to 2048 (chunks of 128 channels), any HW >= 1 (rows need not be 16-byte aligned), one
 * frame of x and of the logits below 2^31 bytes, 16 consecutive query planes spanning less than 2^31 bytes; anything else is
 * refused before the launch, naming the value.
 * The pixels are cut into ceil(HW / 512) slabs — a function of HW alone (dvis_mask_pool_plan: the served-shape checks of the call
 * itself, then plan[0] = the slab size, plan[1] = the slab count; no GPU needed) —, partials go to `ws` and are added in slab order: no float atomics, the same bits on every call, a frame's
 * bits do not depend on B; every element of sum and count is written.  No memset, no host synchronisation: capturable.
 * ws: dvis_mask_pool_ws_bytes bytes (0, and ws may be null, when there is one slab).
 */
int dvis_mask_pool_plan(int B, int Q, int C, int64_t HW, int32_t *plan);
int64_t dvis_mask_pool_ws_bytes(int B, int Q, int C, int64_t HW);
int dvis_mask_pool(const float *x, const float *logits, int64_t l_bstride, int64_t l_qstride, int B, int Q, int C, int64_t HW,
                   float *sum, int32_t *count, void *ws, void *stream);

/*
 * Epilogue of get_classification_logits (ov_dvis/video_mask2former_transformer_decoder_ov.py:17-36) on the products of the exact
 * GEMM (csrc/ov_class_logits.hip):
 *   out[r, k] = max over n in [seg_ptr[k], seg_ptr[k + 1]) of  s * dots[r, n] / max(||x_r||, 1e-12),  s = min(exp(*logit_scale), 100)
 *   x (R, D) and dots (R, N) = x text^T with row strides in elements; logit_scale: ONE DEVICE float; seg_ptr (K1 + 1) int32 DEVICE
 *   prefix sums of num_templates over the K1 = K + 1 groups (the void group last), seg_ptr[0] = 0, seg_ptr[K1] = N, no empty
 *   group (the caller checks the list); out (R, K1).  One launch, fixed-order norm: the same bits on every call.
 */
int dvis_text_class_logits(const float *x, int64_t x_stride, const float *dots, int64_t dots_stride, const float *logit_scale,
                           const int32_t *seg_ptr, int R, int D, int N, int K1, float *out, void *stream);

/*
 * Geometric ensemble of the open-vocabulary meta-architectures (ov_dvis/meta_architecture_ov.py:603-642), one launch:
 *   in_logits, out_logits, out (R, K + 1) contiguous; overlapping (K) fp32, non-zero = seen category; valid (R) int32 or null
 *   (ENSEMBLE_ON_VALID_MASK: a row with valid <= 0 takes a = 0).
 *   p_in, p_out = softmax of the first K logits; a_k = (overlapping_k ? alpha : beta) * (valid_r > 0);
 *   c_k = log(p_in_k^(1 - a_k) p_out_k^(a_k)); p_void = softmax(in_logits[r, :K + 1])[K];
 *   out[r] = log(cat(softmax(c) * (1 - p_void), p_void) + 1e-8).
 * The geometric mean is evaluated in the log domain (c_k = (1 - a_k) log p_in_k + a_k log p_out_k from log-sum-exps): the
 * reference's fp32 `p ** a` underflows to log 0 at CLIP's logit scale; after the final `+ 1e-8` both forms agree wherever the
 * reference's is finite.  Served: 1 <= K <= 2048.
 */
int dvis_ov_ensemble(const float *in_logits, const float *out_logits, const float *overlapping, const int32_t *valid, float alpha,
                     float beta, int R, int K, float *out, void *stream);

/*
 * First half of a ConvNeXt block on a TOKEN-major map (csrc/dwconv_ln.hip): depthwise 7 x 7 convolution (padding 3) + bias, then
 * LayerNorm over the channels — conv_dw, the permute to NHWC and norm of timm's ConvNeXtBlock, up to the input of mlp.fc1.
 *   x: token (b, y, x) at x + b * batch_stride + (y * w + x) * C (the layout convention of dvis_dwconv3x3_tokens); out (B h w, C)
 *   contiguous rows, not overlapping x; weight (C, 1, 7, 7) = C x 49; bias (C) or null; gamma, beta (C).
 *   z[c] = bias[c] + sum_ky sum_kx weight[c, ky, kx] * x[b, y + ky - 3, x + kx - 3, c]   (zeros outside the map)
 *   out  = (z - mean_c z) / sqrt(var_c z + eps) * gamma + beta                           (biased variance)
 * Exact fp32.  The 49 taps of an output are one fma chain, ky outer and kx inner, a padding tap contributing a zero (not a skipped
 * step); the mean is reduced first, then the sum of squared deviations from it, both from the z values held in registers, with a
 * cross-lane shape that depends on C alone: an output's bits do not depend on its position in a tile, on B or on its batch mates.
 * No atomics, no workspace, no memset, no host synchronisation: capturable; every output element is written; the same bits every call.
 * Served: C % 4 == 0, 8 <= C <= 1536, any h, w >= 1, one frame (h w C floats) below 2^31 bytes, 16-byte aligned pointers,
 * batch_stride % 4 == 0 and >= h w C.  Everything else is refused before the launch, naming the value.
 * dvis_dwconv7x7_ln_tokens_supported: 1 where C is served.
 */
int dvis_dwconv7x7_ln_tokens_supported(int C);
int dvis_dwconv7x7_ln_tokens(const float *x, float *out, int64_t batch_stride, int B, int h, int w, int C, const float *weight,
                             const float *bias, const float *gamma, const float *beta, float eps, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVIS_HIP_H */
