/*
 * pmn_hip.h -- C ABI of libpmn_hip.so: the MI355X (gfx950) kernels behind PatchmatchNet's learned-PatchMatch
 * hot path.  This is the drop-in boundary: plain pointers and sizes, no torch types.
 *
 * The reference (FangjinhuaWang/PatchmatchNet) is pure Python over PyTorch and has no FFI of its own; each entry
 * point below replaces the PyTorch op sequence at the cited reference lines.  INTEGRATION.md shows the ctypes
 * binding a reference maintainer would add to models/patchmatch.py / models/module.py.
 *
 * Contract common to every entry point
 *   - all tensor arguments are DEVICE pointers to contiguous float32 buffers owned (and pre-allocated) by the
 *     caller; the library never allocates, never synchronises, and launches on `stream` (a hipStream_t; pass the
 *     caller's current stream, NULL = default stream);
 *     (exceptions: pmn_view_scores, the COLMAP import's view selection, takes float64 / int32 / int64 buffers, pmn_depth_metrics
 *     writes float64 rows, and the point-cloud searches pmn_nn_distance / pmn_reduce_round take int64 keys, int32 / uint8 / uint32
 *     state and write float64 distances, as declared);
 *   - arguments named *_host are small HOST arrays (neighbour tables) copied into the kernel-argument segment;
 *   - returns PMN_OK (0) or a negative PMN_ERR_* code; nothing is launched when an argument check fails;
 *   - entry points never block: each one only ENQUEUES kernels (no hip*Synchronize, no hipMalloc / hipFree, no hipMemcpy /
 *     hipMemset, no stream or event waits), so a call costs microseconds, a whole forward is HIP-graph capturable, and a binding
 *     may call in without releasing its interpreter lock (patchmatchnet_amd/_lib.py uses ctypes.PyDLL);
 *     tests/test_abi.py::test_entry_points_never_block enforces it on the sources;
 *   - entry points are re-entrant; the only process state is a cache of per-(kernel, device) launch attributes.
 *
 * Layouts
 *   feature maps    channels-last  [B, h, w, C]           (source views stacked: [N, B, hs, ws, C])
 *   hypotheses      [B, D, h, w]   (D <= PMN_MAX_DEPTH)   depth_sample of the reference
 *   per-view weight [B, N, h, w]
 *   offsets         [B, 2K, h, w]  output of the reference's propa_conv / eval_conv (channel 2k -> x, 2k+1 -> y)
 *   neighbour table host int[2K]   (dy,dx) pairs, reference models/patchmatch.py:331-392
 *   MLP block       DEVICE float[PMN_MLP_FLOATS], BatchNorm folded, packed once per model by
 *                   patchmatchnet_amd/params.py: 16 records of 20 floats, one per hidden unit j
 *                   { w0[j][0..7] (first G used) | w1[0..7][j] | t0[j] | 3 pad }, then t1[8] | w2[8] | b2 | 3 pad
 */
#ifndef PMN_HIP_H
#define PMN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMN_ABI_VERSION 25
#define PMN_MLP_FLOATS 340
#define PMN_MAX_DEPTH 64
#define PMN_MAX_NEIGHBORS 17
#define PMN_MAX_FUSE_SRC 32
#define PMN_TSDF_MAX_VIEWS 16 /* views of one pmn_tsdf_integrate launch */
#define PMN_TSDF_MARK_SPAN 8 /* blocks per axis one pixel of pmn_tsdf_mark_blocks may mark; a larger box is counted, not marked */
#define PMN_RASTER_MAX_DIM 16384 /* largest height / width of a rendered view: the guard band of pmn_raster_triangles in pixels */
#define PMN_RASTER_MAX_BOX 64    /* pixels of a triangle's bounding box up to which one thread draws it (max_box = 0) */
#define PMN_SPLAT_MAX_RADIUS 32  /* largest footprint radius of pmn_splat_points in pixels */

#define PMN_OK 0
#define PMN_ERR_ARG (-1)     /* null pointer / size out of range */
#define PMN_ERR_SHAPE (-2)   /* unsupported channel / group / neighbour / hypothesis count */
#define PMN_ERR_LAUNCH (-3)  /* hipGetLastError() after the launch */

/* ABI version of the loaded library (== PMN_ABI_VERSION of the header it was built from). */
int pmn_abi_version(void);

/* Human-readable text for a PMN_ERR_* code. */
const char *pmn_error_string(int code);

/* [B,C,h,w] -> [B,h,w,C].  Feeds FeatureNet outputs (reference models/net.py:203-208) to the kernels below.
 * `out` may be a slot of the stacked source buffer. */
int pmn_nchw_to_nhwc(const float *in, float *out, int B, int C, int h, int w, void *stream);

/* FeatureWeightNet.forward (reference models/patchmatch.py:603-624) fused with get_grid (:396-426):
 * gather the K evaluation neighbours of every reference pixel (bilinear, border, align_corners=False on a grid
 * normalised with (size-1)/2), group-wise correlation with the centre feature, MLP, sigmoid.
 * out_feature_weight [B,K,h,w].  C in {16,32,64}, G in {4,8} with C/G in {4,8}, K in {9,17}. */
int pmn_feature_weight(const float *ref_nhwc, const float *eval_offsets, const int *eval_table_host,
                       const float *mlp, int B, int C, int G, int K, int h, int w,
                       float *out_feature_weight, void *stream);

/* DepthInitialization.forward + Propagation.forward (reference models/patchmatch.py:53-94, 115-124), fused:
 *   noise != NULL : first iteration on the coarsest stage; 48 hypotheses from the caller's torch.rand draw
 *                   noise [B,48,h,w] (the RNG stays with the caller so it matches the reference stream);
 *   noise == NULL : num_sample hypotheses around `depth` ([B,1,h>>depth_shift,w>>depth_shift]; depth_shift=1
 *                   reads the previous stage's map through the nearest x2 up-sampling of net.py:274);
 *                   num_sample == 1 passes depth through.
 *   K > 0         : the centre hypothesis (index D0/2) is gathered at the K propagation neighbours, appended, and
 *                   the D = D0 + K values are sorted ascending per pixel.
 * depth_min/depth_max: device float[B].  PRECONDITION of every entry point that takes them or depth hypotheses: finite,
 * 0 < depth_min < depth_max, previous depths finite and > 0 -- the kernels' divisions are hipcc's IEEE fma sequence without its
 * v_div_scale / v_div_fixup shell (csrc/pmn_common.hpp), bit-identical for normal operands; a zero or infinite divisor (a degenerate
 * range) yields NaN where the reference's division yields inf.  eval.py refuses such samples before upload (its _check_depth_range).
 * Outputs: depth_sample [B,D,h,w] and its normalised inverse depth
 * xnorm = (1/d - 1/dmax)/(1/dmin - 1/dmax) (reference :655-657), stored HYPOTHESIS-LAST [B,h,w,D] for
 * pmn_aggregate_regress (its only consumer: one bilinear corner of a neighbour = D contiguous floats). */
int pmn_init_hypotheses(const float *noise, const float *depth, int depth_shift, const float *depth_min,
                        const float *depth_max, int num_sample, float interval_scale, const float *propa_offsets,
                        const int *propa_table_host, int K, int B, int h, int w, float *depth_sample,
                        float *xnorm, void *stream);

/* The fused hot kernel.  Evaluation.forward up to and including SimilarityNet's pointwise MLP
 * (reference models/patchmatch.py:192-217, 570; differentiable_warping models/module.py:130-181;
 * PixelwiseNet :695-702):  for every source view: homography warp of the D hypotheses, bilinear (zeros,
 * align_corners=True) gather of the source features, group-wise correlation with the reference feature;
 * view weights either read from view_weights_in ([B,N,h>>vw_shift,w>>vw_shift]; vw_shift = 1 / 2 reads a
 * coarser stage's map through the nearest x2 / x4 up-sampling of net.py:275) or -- view_weights_in == NULL -- computed by PixelwiseNet (max over D of the
 * sigmoid response) and written to view_weights_out [B,N,h,w] (+ optional arg-max index vw_argmax_out);
 * weighted aggregation over views; SimilarityNet MLP -> cost_out, stored HYPOTHESIS-LAST [B,h,w,D] (consumed only by
 * pmn_aggregate_regress).
 * rel_proj [B,N,4,4] = src_proj @ inverse(ref_proj).  similarity_out (optional) receives the aggregated
 * similarity [B,G,D,h,w] (the tensor the reference materialises at :217).
 * The warped volume [B,C,D,h,w] is never materialised. */
int pmn_warp_correlate(const float *ref_nhwc, const float *src_nhwc, const float *rel_proj,
                       const float *depth_sample, const float *view_weights_in, int vw_shift,
                       const float *similarity_mlp, const float *pixelwise_mlp, int B, int N, int C,
                       int G, int D, int h, int w, int hs, int ws, float *cost_out, float *view_weights_out,
                       int *vw_argmax_out, float *similarity_out, void *stream);

/* The same, with the source views handed over as a DEVICE table of N addresses (64-bit each) of per-view [B,hs,ws,C] channels-last maps
 * instead of one stacked [N,B,hs,ws,C] tensor: the maps stay where their producer left them.  eval.py's per-scan feature cache uses it
 * (every view's pyramid is encoded once and read by ~num_views samples; stacking would copy 0.5 GB per 1600x1200 sample), the table
 * itself is a static device buffer a HIP graph can keep reading while the host rewrites it between replays.  Reference: the list
 * `src_features` of models/patchmatch.py:179-191 -- a list of separately allocated tensors there too. */
int pmn_warp_correlate_views(const float *ref_nhwc, const void *src_view_table, const float *rel_proj,
                             const float *depth_sample, const float *view_weights_in, int vw_shift,
                             const float *similarity_mlp, const float *pixelwise_mlp, int B, int N, int C,
                             int G, int D, int h, int w, int hs, int ws, float *cost_out, float *view_weights_out,
                             int *vw_argmax_out, float *similarity_out, void *stream);

/* Adaptive spatial cost aggregation + softmax + regression: depth_weight (reference models/patchmatch.py:650-669),
 * weight normalisation (:509-510), SimilarityNet's neighbour gather and weighted sum (:569-577),
 * exp(log_softmax) (:221) and depth regression (:226-237).
 * cost and xnorm are hypothesis-last [B,h,w,D] (as pmn_warp_correlate / pmn_init_hypotheses write them); depth_sample
 * [B,D,h,w]; score_out [B,D,h,w] = probabilities, depth_out [B,h,w].  is_inverse selects the inverse-depth regression. */
int pmn_aggregate_regress(const float *cost, const float *depth_sample, const float *xnorm,
                          const float *feature_weight, const float *eval_offsets, const int *eval_table_host,
                          int K, float interval_scale, int is_inverse, int B, int D, int h, int w,
                          float *score_out, float *depth_out, void *stream);

/* Photometric-confidence epilogue (reference models/net.py:288-299): 4-wide window sum of the stage-1
 * probabilities around trunc(sum_d d*p_d), nearest resize to [B,H,W].  depth_index_out (optional) [B,h,w]. */
int pmn_confidence(const float *score, int B, int D, int h, int w, int H, int W, float *confidence_out,
                   int *depth_index_out, void *stream);

/* Direct fp32 convolution with fused epilogue for the small-channel CNNs around the hot path: FeatureNet's ConvBnReLU
 * stack and FPN head (reference models/net.py:17-67), the offset heads propa_conv / eval_conv
 * (models/patchmatch.py:288-311, 467-471).  out = [relu]( conv(in, W) + shift [+ bilinear_x2(up)] ).
 *   in       [N,H,W,cin] channels-last, or [N,cin,H,W] when in_nchw (cin = 3 or 1: the image / depth planes)
 *   weights  DEVICE float [K][K][cin][coutp], coutp = cout rounded up to 8 (cout <= 8) or a multiple of 16, BatchNorm scale
 *            folded in (patchmatchnet_amd/params.py: pack_conv); shift DEVICE float[coutp] (folded BN shift or conv bias)
 *   up       optional [N,up_h,up_w,cout] map, bilinearly up-sampled x2 (align_corners=False) and added (net.py:60,65)
 *   out      [N,Ho,Wo,cout] channels-last, or planar [N,cout,Ho,Wo] when out_nchw (the offset planes the PatchMatch
 *            kernels read).  Supported (cin,K,stride): (3|1,3,1 nchw-in), (8|16|32|64,3,1), (8|16|32,5,2), (16|32|64,1,1). */
int pmn_conv2d(const float *in, const float *weights, const float *shift, const float *up, float *out, int N, int H,
               int W, int cin, int cout, int K, int stride, int pad, int dil, int relu, int in_nchw, int out_nchw,
               int up_h, int up_w, void *stream);

/* Fused tail of FeatureNet's FPN (reference models/net.py:64-67): out = output3( bilinear_x2(up) + inner2(x) ) without
 * materialising the 64-channel half-resolution map.  x [N,H,W,16], up [N,H/2,W/2,64], w_in [16][64] / b_in [64] and
 * w_out [64][16] in pack_conv layout (device) -> out [N,H,W,16]. */
int pmn_fpn_tail(const float *x, const float *up, const float *w_in, const float *b_in, const float *w_out, float *out,
                 int N, int H, int W, int cin, int cmid, int cout, void *stream);

/* The same convolution (+ folded BatchNorm shift / bias, optional ReLU) as fp32 implicit GEMM on the matrix cores
 * (v_mfma_f32_32x32x2_f32: exact fp32, bitwise a k-ordered fmaf chain).  in [N,H,W,cin] channels-last; weights DEVICE float
 * [K*K][cin/8][coutp/32][64][4] with coutp = cout rounded up to 32 (patchmatchnet_amd/params.py: pack_conv_mfma); shift
 * DEVICE float[coutp].
 *   planar == 0  the 1x1 form (cin 64, cout <= 128, K 1, stride 1, pad 0): channels [0,ca) -> out [N,H,W,ca], [ca,cout) -> out_b
 *                [N,H,W,cout-ca] -- the 1/8-resolution level of the folded FPN head (reference models/net.py:36-70), same arithmetic
 *                as pmn_fpn_level.  This is the ONLY shape of the product library since round 4 (ABI 17): everything else returns
 *                PMN_ERR_SHAPE.  The research build (pmn_hip_experimental.h) additionally keeps rounds 1-2's forms: FeatureNet's wide
 *                layers (cin,cout,K,stride) = (64,64,3,1), (32,32,3,1), (32,64,5,2), (16,32,5,2) with out [N,Ho,Wo,cout], and
 *   planar == 1  the offset heads of one stage as ONE dilated 3x3 convolution ((cin,dil) = (64,2), (32,4), (16,6), cout <= 64;
 *                channels [0,ca) -> out [N,ca,Ho,Wo], the rest -> out_b, planar) -- superseded by pmn_conv2d_f16s /
 *                pmn_offset_heads_f16s in round 3. */
int pmn_conv2d_mfma(const float *in, const float *weights, const float *shift, float *out, float *out_b, int N, int H, int W,
                    int cin, int cout, int ca, int K, int stride, int pad, int dil, int relu, int planar, void *stream);

/* ---- fp16-split entry points (pmn_conv2d_f16s, pmn_offset_heads_f16s, pmn_stem_f16s, pmn_refine_fused): accepted magnitudes ----
 * Every activation and weight x is split as hi = fp16(x), lo = fp16((x - hi) * 2048) and the product sum is taken as
 * hi*hi + (hi*lo + lo*hi) / 2048 with fp32 accumulation.  That reproduces an fp32 convolution (2-4e-7 of the output scale) for
 *     6.1e-5 <= |x| < 65504   (fp16's normal range: 22 significant bits per factor);
 * below 6.1e-5 `hi` is a subnormal (absolute error <= 3e-8 per factor -- irrelevant next to factors of normal size; an operand
 * tensor that is ENTIRELY below 1e-6 loses relative precision); at |x| >= 65504 `hi` becomes +-inf and the output is inf / NaN where
 * an fp32 convolution is finite.  The kernels do not check (opt-in: pmn_check_f16_domain, PMN_CHECK_F16_DOMAIN=1).  WEIGHTS are checked on the host when they are packed
 * (patchmatchnet_amd/params.py raises F16DomainError for a BatchNorm-folded weight outside (-65504, 65504), and the modules then use
 * the fp32 kernels pmn_stem / pmn_conv2d / pmn_refine_front + pmn_refine_tail and say so); ACTIVATIONS are the caller's contract:
 * images in [0, 1] (or any range below 6e4) and the reference checkpoint keep every intermediate below 1e2.
 * tests/test_hip_parity.py::test_f16_split_domain documents both ends of the range on the GPU. */

/* FeatureNet's ConvBnReLU layers conv2..conv10 (reference models/net.py:20-31: 3x3 stride 1 with cin == cout in {16,32,64}; 5x5
 * stride 2 with (cin,cout) in {(8,16),(16,32),(32,64)}) on the FP16 matrix cores with SPLIT operands: every activation and every
 * weight is x = hi + lo/2048 (hi = fp16(x), lo = fp16((x-hi)*2048): 22 significant bits), and sum x*w is evaluated as
 * sum hi*hi + (sum hi*lo + sum lo*hi)/2048 -- three v_mfma_f32_16x16x32_f16 per k-step with fp32 accumulation, 16/3 the rate of
 * v_mfma_f32_16x16x4_f32, the error of an fp32 direct convolution (2-4e-7 of the output scale; scripts/fp16_split_study.py).
 * in [N,H,W,cin] channels-last float32; weights DEVICE float16 [cin/CC][k-steps][cout/16][2][64][8] (hi | lo B operands in lane
 * order, BatchNorm scale folded in float64: patchmatchnet_amd/params.py pack_conv_f16s); shift DEVICE float[cout]; out
 * [N,(H-1)/stride+1,(W-1)/stride+1,cout] float32 (padding k/2). */
int pmn_conv2d_f16s(const float *in, const void *weights, const float *shift, float *out, int N, int H, int W, int cin, int cout,
                    int k, int stride, int relu, void *stream);

/* ABI 22.  Two consecutive 3x3 / stride-1 / 16 -> 16 ConvBnReLU layers in ONE launch (FeatureNet conv3 + conv4 at half resolution,
 * reference models/net.py:21-22, 52): the 184 MB intermediate map of six 1600x1200 views never goes to HBM (the first layer is
 * evaluated on each 14 x 14 tile's 16 x 16 halo region and kept in LDS as split fp16 planes).  in / out [N,H,W,16] channels-last
 * float32; weights_* / shift_* exactly as pmn_conv2d_f16s takes them for a (k 3, stride 1, 16 -> 16) layer; relu applies to both
 * layers.  Bit-identical to two pmn_conv2d_f16s calls.  channels != 16: PMN_ERR_SHAPE (the other layer pairs of FeatureNet do not
 * pay: profiles/r06_conv_fusion_bound.log). */
int pmn_conv2d_f16s_pair(const float *in, const void *weights_a, const float *shift_a, const void *weights_b, const float *shift_b,
                         float *out, int N, int H, int W, int channels, int relu, void *stream);

/* The offset heads of one PatchMatch stage -- propa_conv rows first, then eval_conv (reference models/patchmatch.py:288-311, :467, :471) --
 * as ONE dilated 3x3 convolution with bias on the fp16 matrix cores with split operands (see pmn_conv2d_f16s), planar outputs.
 * in [N,H,W,cin] channels-last; weights DEVICE float16 [cin/16][k-steps][coutp/16][2][64][8] with coutp = cout rounded up to 16
 * (patchmatchnet_amd/params.py pack_offset_heads_f16s); shift DEVICE float[coutp]; out_a [N,ca,H,W] = channels [0,ca), out_b
 * [N,cout-ca,H,W] = the rest (NULL when ca == cout).  Supported (cin, dilation): (64,2), (32,4), (16,6) -- the reference's three stages
 * -- with cout rounded up to 32, 48 or 64; PMN_ERR_SHAPE otherwise (the caller then uses pmn_conv2d). */
int pmn_offset_heads_f16s(const float *in, const void *weights, const float *shift, float *out_a, float *out_b, int N, int H, int W,
                          int cin, int cout, int ca, int dil, void *stream);

/* One level of FeatureNet's FPN head in FOLDED form (reference models/net.py:57-67).  The head is linear (1x1 convolutions,
 * bilinear x2 up-sampling, sums), so output_k(upsample(intra) + inner_k(conv)) is evaluated as
 *   out[c] = bilinear_x2(u)[c] + b[c] + sum_ci x[ci] * w[ci][c]
 * with w = output . inner and b = output . bias_inner formed in float64 on the host (patchmatchnet_amd/params.py: fold_fpn):
 *   1/8:  [feature3 | u8] = W8 conv10          (cin 64, cout 112, ca 64, u = NULL)
 *   1/4:  [feature2 | u4] = up(u8) + W4 conv7   (cin 32, cout 48,  ca 32)
 *   1/2:   feature1       = up(u4) + W2 conv4   (cin 16, cout 16,  ca 16)
 * x [N,H,W,cin]; u [N,H/2,W/2,cout] or NULL; w DEVICE float [cin][cout]; b DEVICE float [cout]; channels [0,ca) go to
 * out_a [N,H,W,ca], the remaining cout-ca to out_b [N,H,W,cout-ca] (NULL when ca == cout). */
int pmn_fpn_level(const float *x, const float *u, const float *w, const float *b, float *out_a, float *out_b, int N, int H,
                  int W, int cin, int cout, int ca, void *stream);

/* ConvTranspose2d(8, 8, k=3, stride=2, padding=1, output_padding=1, bias=False) + BatchNorm + ReLU of the Refinement net
 * (reference models/net.py:86-88, 114).  in [N,Hi,Wi,8]; weights DEVICE float [3][3][8][8] ([ky][kx][ci][co], BatchNorm scale
 * folded in: patchmatchnet_amd/params.py pack_deconv); shift DEVICE float[8] -> out [N,2Hi,2Wi,8]. */
int pmn_deconv3x3s2(const float *in, const float *weights, const float *shift, float *out, int N, int Hi, int Wi, int cin,
                    int cout, int relu, void *stream);

/* Full-resolution half of the Refinement network (reference models/net.py:73-126) in two launches.
 * pmn_refine_front: x16 = cat( relu(bn(deconv(t2))), conv0(img) ) (net.py:110-117): img [B,3,H,W] planar, t2 [B,H/2,W/2,8]
 *   channels-last (conv2 output); w0 [3][3][3][8] / s0 [8] = pack_conv of conv0, wd [3][3][8][8] / sd [8] = pack_deconv of
 *   deconv + bn (DEVICE) -> x16 [B,H,W,16].  H, W even.
 * pmn_refine_tail: depth = (nearest_x2(dnorm) + res(conv3(x16))) * (depth_max - depth_min) + depth_min (net.py:117-122):
 *   w3 [2][3][3][16][4] / s3 [8] and wr [3][3][8] from patchmatchnet_amd/params.py pack_refine_tail (DEVICE); dnorm
 *   [B,1,H/2,W/2] normalised input depth; depth_min / depth_max DEVICE float[B] -> out [B,1,H,W]. */
int pmn_refine_front(const float *img, const float *t2, const float *w0, const float *s0, const float *wd, const float *sd,
                     float *x16, int B, int H, int W, void *stream);
int pmn_refine_tail(const float *x16, const float *w3, const float *s3, const float *wr, const float *dnorm,
                    const float *depth_min, const float *depth_max, float *out, int B, int H, int W, void *stream);

/* The same half in ONE launch (what Refinement.forward_hip runs): pmn_refine_front's and pmn_refine_tail's arguments without the x16
 * buffer between them, and conv3 on the fp16 matrix cores with split operands -- w3a DEVICE float16 [5][2][64][8] / s3 [8] from
 * patchmatchnet_amd/params.py pack_refine_conv3_f16s (conv3's weights as MFMA A operands, hi | lo, BatchNorm folded).  The x16
 * intermediate (123 MB per 1600x1200 depth map) stays in LDS.  H, W even. */
int pmn_refine_fused(const float *img, const float *t2, const float *w0, const float *s0, const float *wd, const float *sd,
                     const void *w3a, const float *s3, const float *wr, const float *dnorm, const float *depth_min,
                     const float *depth_max, float *out, int B, int H, int W, void *stream);

/* Relative projections of every (stage, batch element, source view): rel = P_src @ inverse(P_ref) with
 * P = [[K_s @ E[:3,:4]], [E[3,:]]] and K_s = K with rows 0,1 scaled by scale0 * 2^stage (reference models/net.py:225-231,
 * models/module.py:148).  intrinsics [B,V,3,3], extrinsics [B,V,4,4] (view 0 = reference) -> rel [nstages,B,V-1,4,4]. */
int pmn_stage_projections(const float *intrinsics, const float *extrinsics, int B, int V, int nstages, float scale0,
                          float *rel, void *stream);

/* Fused full-resolution stem of FeatureNet: conv0 (3->8) + conv1 (8->8), each 3x3 + BatchNorm + ReLU (reference
 * models/net.py:17-19, 51).  img [N,3,H,W] planar; w0 [3][3][3][8] / s0 [8], w1 [3][3][8][8] / s1 [8] (pack_conv layout, device)
 * -> out [N,H,W,8] channels-last. */
int pmn_stem(const float *img, const float *w0, const float *s0, const float *w1, const float *s1, float *out, int N, int H,
             int W, void *stream);

/* The same stem with conv1 (72 % of its multiplies) on the FP16 matrix cores with split operands (see pmn_conv2d_f16s): conv0 on the
 * fp32 VALU into LDS, split into hi / lo fp16 planes there, conv1 as three v_mfma_f32_16x16x32_f16 per k-step with the output channels
 * as MFMA rows.  w1a DEVICE float16 [3][2][64][8] (patchmatchnet_amd/params.py pack_stem_conv1_f16s); everything else as pmn_stem. */
int pmn_stem_f16s(const float *img, const float *w0, const float *s0, const void *w1a, const float *s1, float *out, int N, int H,
                  int W, void *stream);

/* pmn_stem_f16s for `views` separately allocated images of one size (reference models/net.py:203-208: FeatureNet runs per image of
 * the `images` list): img_table DEVICE array of `views` addresses, entry v = a dense [B,3,H,W] float32 tensor, every address 16-byte
 * aligned (caller's contract); out [views*B,H,W,8] view-major.  The table is read when the kernel runs: a captured launch follows
 * whatever the table holds at replay time, so a HIP graph reads each sample's images in place (patchmatchnet_amd/graph.py). */
int pmn_stem_f16s_views(const float *const *img_table, int views, const float *w0, const float *s0, const void *w1a,
                        const float *s1, float *out, int B, int H, int W, void *stream);

/* Added under ABI 25 (purely additive: tests of the existing suite pin the number).  pmn_stem_f16s followed by pmn_conv2d_f16s for
 * FeatureNet's conv2 (8 -> 16, 5x5, stride 2, ReLU) in ONE launch: conv1's full-resolution map [N,H,W,8] stays in LDS and never
 * reaches memory.  img, w0, s0, w1a, s1 as pmn_stem_f16s; w2b / s2 = conv2 as pmn_conv2d_f16s takes it (params.py pack_conv_f16s)
 * -> out [N,Ho,Wo,16] channels-last, Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1: the same BITS as the two calls. */
int pmn_stem_conv2_f16s(const float *img, const float *w0, const float *s0, const void *w1a, const float *s1, const void *w2b,
                        const float *s2, float *out, int N, int H, int W, void *stream);

/* The same through a device table of image addresses, as pmn_stem_f16s_views: out [views*B,Ho,Wo,16] view-major. */
int pmn_stem_conv2_f16s_views(const float *const *img_table, int views, const float *w0, const float *s0, const void *w1a,
                              const float *s1, const void *w2b, const float *s2, float *out, int B, int H, int W, void *stream);

/* Stand-alone differentiable_warping (reference models/module.py:130-181) for API completeness and unit
 * parity: src_nchw [B,C,hs,ws], rel_proj [B,4,4], depth [B,D,h,w] -> warped [B,C,D,h,w].  Not on the fast path. */
int pmn_differentiable_warping(const float *src_nchw, const float *rel_proj, const float *depth, int B, int C,
                               int D, int h, int w, int hs, int ws, float *warped, void *stream);

/* Photometric + geometric consistency filtering of ONE reference view against its n_src source views and the fused world points
 * (reference eval.py:86-190 reproject_with_depth / check_geometric_consistency, :207-281 filter_depth), one launch, a thread per
 * reference pixel.  maps: the per-scan buffer [V][2][H][W] (slot v = depth, confidence of view v -- what the per-scan all-gather
 * leaves on every rank), slot_stride floats between slots; ref_slot and src_slots_host[n_src] (HOST ints, n_src <=
 * PMN_MAX_FUSE_SRC) index it.  H x W is the REFERENCE view's size; src_hw_host (HOST int[2*n_src]: height, width of every source
 * view's maps; NULL = all H x W) gives every source map its own size, as the reference reads every view's file at its own size
 * (eval.py:203-237; --image_max_dim on a scan with mixed image sizes): slot v holds depth [h_v][w_v] then confidence [h_v][w_v]
 * packed at the start of the slot, slot_stride >= 2*h*w of the largest view.  mats (DEVICE float32, built by patchmatchnet_amd/fusion.py with numpy's own
 * float32 inverse / matmul so that they are the reference's matrices): 48 floats for the reference view -- [0..8] inverse(K_ref),
 * [9..17] K_ref, [18..33] inverse(E_ref) -- then 64 floats per source view -- [0..15] E_src @ inverse(E_ref), [16..24] K_src,
 * [25..33] inverse(K_src), [34..49] E_ref @ inverse(E_src).  Outputs: masks [3][H][W] bytes (photo = confidence > photo_thres,
 * geo = consistent sources >= geo_mask_thres, final = both), xyz [H][W][3] world point of the averaged depth (meaningful where
 * final), optional depth_avg [H][W] float64 and geo_sum [H][W] int32.  Numeric types follow the reference's numpy dtype flow;
 * cv2.remap(INTER_LINEAR) is restated with OpenCV's 1/32-pixel fixed-point coordinates (oracle/fusion_oracle.py). */
int pmn_fuse_view(const float *maps, long long slot_stride, int ref_slot, const int *src_slots_host,
                  const int *src_hw_host, int n_src, const float *mats, int H, int W, float geo_pixel_thres, float geo_depth_thres, int geo_mask_thres,
                  float photo_thres, unsigned char *masks, float *xyz, double *depth_avg, int *geo_sum, void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  pmn_fuse_view that writes each surface point once
 * (DESIGN.md section 22): every argument of pmn_fuse_view with its meaning, and masks, xyz, depth_avg, geo_sum bit for bit what
 * pmn_fuse_view writes (one kernel body, instantiated with and without the claims).  claimed: DEVICE bytes, one slot per map slot,
 * claim_stride bytes apart (>= h*w of the largest view); slot v is view v's map [h_v][w_v] at its own size, 1 = a view fused
 * earlier wrote a point that covers this pixel.  The caller zeroes it before a scan's first view and fuses the views on ONE stream.
 * emit [H][W] bytes = final && !claimed[ref_slot]: the pixels whose points belong in the file.  Every FINAL pixel (emitted or not)
 * then claims, in each source view s whose consistency test it passed, the pixel (rintf(xs), rintf(ys)) of its forward projection
 * (the float32 coordinates that feed the bilinear sample), provided that pixel lies inside view s's map and view s's own depth d
 * there agrees with the point's float32 depth z in that camera: fabsf(d - z) / z < geo_depth_thres.  A claim is a plain byte store
 * of 1: the launch reads claimed[ref_slot] only and writes claimed[src_slots] only, so ref_slot inside src_slots_host is
 * PMN_ERR_ARG, as are a null claimed or emit and a claim_stride below H*W or below a source view's h*w. */
int pmn_fuse_view_merged(const float *maps, long long slot_stride, int ref_slot, const int *src_slots_host,
                         const int *src_hw_host, int n_src, const float *mats, int H, int W, float geo_pixel_thres,
                         float geo_depth_thres, int geo_mask_thres, float photo_thres, unsigned char *masks, float *xyz,
                         double *depth_avg, int *geo_sum, unsigned char *claimed, long long claim_stride, unsigned char *emit,
                         void *stream);

/* ABI 19.  The point list of one fused reference view as PLY vertex records, packed on the device (reference eval.py:270-281: the
 * valid pixels' world points and colours, row-major; :283-297: plyfile's vertex element = x, y, z little-endian float32 + red,
 * green, blue uint8 = 15 bytes).  final_mask [H][W] bytes and xyz [H][W][3] are pmn_fuse_view's outputs; image_hwc [H][W][3] is
 * the reference view's image, uint8 as decoded (image_is_float = 0: the bytes are the colours) or float32 in [0,1]
 * (image_is_float = 1: (unsigned char)(f * 255.0f), the reference's (color * 255).astype(uint8)).  The records of the pixels whose
 * mask byte is non-zero are APPENDED to `records` (device bytes, room for capacity_points records) at record index *cursor
 * (DEVICE int64), in row-major pixel order; then *cursor += count and *view_count (DEVICE int32) = count.  If the view does not
 * fit, nothing is written, the cursor stays and *view_count = -1.  scratch: DEVICE int64[ceil(H*W / 1024)].  Three launches on
 * `stream`; consecutive calls on one stream append view after view -- a scan's whole PLY body as one device buffer. */
int pmn_pack_points(const unsigned char *final_mask, const float *xyz, const void *image_hwc, int image_is_float, int H, int W,
                    unsigned char *records, long long capacity_points, long long *cursor, int *view_count, long long *scratch,
                    void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  pmn_pack_points with the normal columns of an oriented
 * cloud: normals_chw [3][H][W] is the view's camera-frame normal map (pmn_depth_normals), rotation the camera-to-world rotation,
 * DEVICE float32, row-major with rotation_stride (>= 3) floats between rows -- 3 for a packed 3x3, 4 for the upper-left block of
 * inverse(E_ref) inside pmn_fuse_view's mats (mats + 18).  Records are 27 bytes: x y z nx ny nz little-endian float32, red green blue
 * uint8; the world normal is rotation . normal in float32 (products summed left to right, not re-normalised; a zero normal stays
 * zero).  `records` has room for capacity_points 27-byte records.  Everything else -- which pixels, their order, the cursor,
 * *view_count = -1 when the view does not fit, the scratch size, three launches -- is pmn_pack_points (the count and the scan are
 * the same kernels). */
int pmn_pack_points_normals(const unsigned char *final_mask, const float *xyz, const float *normals_chw, const float *rotation,
                            int rotation_stride, const void *image_hwc, int image_is_float, int H, int W, unsigned char *records,
                            long long capacity_points, long long *cursor, int *view_count, long long *scratch, void *stream);

/* Added under ABI 25 (purely additive).  Surface normals of a depth map in the camera frame of its image (the
 * reference writes no normal maps).  depth [H][W], any H, W >= 1; intrinsics_host HOST float[9] = K row-major (fx, skew, cx, fy, cy
 * are read; all nine must be finite); pixel (x, y) has the ray inverse(K) (x, y, 1)^T with integer pixel coordinates.
 * normals_out is PLANAR [3][H][W] (the channel order of COLMAP's .bin body).  Per pixel p: the pixels q of the (2 radius + 1)^2 window
 * that are inside the image, valid (finite, > 0) and satisfy fabsf(z_q - z_p) <= rel_thres * z_p (float32, one rounding each side)
 * are accepted; 1 / z_q - 1 / z_p = (z_p - z_q) / (z_p z_q) is fitted by a dx + b dy + c over them (unweighted least squares, the
 * normal equations' integer determinant and adjugate exact); m = (fx a, skew a + fy b, 1 / z_p + c + a (cx - x_p) + b (cy - y_p)),
 * n = -m / |m|: unit length, facing the camera (n . ray < 0).  n = (0, 0, 0) where p is invalid, where the determinant is 0 (fewer
 * than three non-collinear accepted pixels) or where |m| is zero or not finite.  IEEE divisions and square root, no contraction.
 * radius outside 1..3: PMN_ERR_SHAPE; rel_thres not finite or <= 0, a non-finite intrinsic: PMN_ERR_ARG.  One launch. */
int pmn_depth_normals(const float *depth, int H, int W, const float *intrinsics_host, int radius, float rel_thres,
                      float *normals_out, void *stream);

/* ABI 20.  Refinement's input normalisation (reference models/net.py:104-106): out = (depth - depth_min[b]) / (depth_max[b] -
 * depth_min[b]) over n floats per batch element, IEEE subtraction and correctly rounded division = the bits of the torch expression.
 * With it a whole forward consists of launches of this library only, which is what makes it recordable as a launch plan. */
int pmn_normalize_depth(const float *depth, const float *depth_min, const float *depth_max, int B, int n, float *out,
                        void *stream);

/* ABI 21.  Opt-in range check for the fp16-split entry points (see "accepted magnitudes" above): ORs 1 into *flag (DEVICE int, zeroed by
 * the caller) when some element of x[0..n) is not finite or has |x| >= 65504 -- the magnitude at which the split's `hi` half becomes inf.
 * patchmatchnet_amd/ops.py runs it on the inputs of pmn_conv2d_f16s / pmn_offset_heads_f16s / pmn_stem_f16s / pmn_refine_fused when
 * PMN_CHECK_F16_DOMAIN=1 and raises from ops.f16_domain_check(); intermediates that never leave a fused kernel (the stem's conv0 output,
 * pmn_refine_fused's x16) are covered through the next layer's input. */
int pmn_check_f16_domain(const float *x, long long n, int *flag, void *stream);

/* ---- ABI 20: launch plans -------------------------------------------------------------------------------------------------------
 * A plan is a recorded list of kernel launches that pmn_plan_launch replays on a stream with plain hipLaunchKernel calls from C: the
 * whole forward (reference models/net.py:176-301, the body of the loop at eval.py:56-65) as ONE library call per sample, without a
 * HIP graph (same replay rate; nothing but kernel launches to depend on; the plan's contents can be listed).
 *
 *   pmn_plan_create(&plan)
 *   pmn_plan_begin(plan)          from now on every pmn_* entry point called BY THIS THREAD validates its arguments as usual but
 *   ... pmn_* calls ...           appends its launches (kernel, grid, LDS size, a copy of the by-value arguments, neighbour tables
 *   pmn_plan_end(plan)            included) to the plan instead of enqueuing them; their `stream` argument is ignored
 *   pmn_plan_launch(plan, stream) enqueues the recorded launches, in order, on `stream`; any number of times, from any thread
 *   pmn_plan_destroy(plan)
 *
 * The plan holds the DEVICE addresses that were passed while recording: the caller keeps those buffers alive and in place for the
 * life of the plan and feeds new inputs by writing into them (or into the device address tables of pmn_warp_correlate_views /
 * pmn_stem_f16s_views) before each launch, on the same stream.  One recording per thread at a time; a plan is recorded once.
 * pmn_plan_count = number of recorded entries; pmn_plan_kernel_name(plan, i) = the i-th kernel's symbol name (diagnostics).
 * Like every entry point, none of these synchronises, allocates device memory or copies.
 *
 * Added under ABI 25 (purely additive: tests of the existing suite pin the number).  ONE fork/join region per plan -- a stretch of the
 * recording whose launches fall into two branches that do not depend on each other, so that a replay may run them side by side:
 *
 *   pmn_plan_fork(plan)            opens the region; launches are tagged main (0) until switched
 *   pmn_plan_switch(plan, branch)  0 = main, 1 = side: the tag of the launches recorded from here on
 *   pmn_plan_join(plan)            closes the region; everything recorded afterwards depends on both branches
 *
 * All three are valid only while the calling thread records that plan and return PMN_ERR_ARG for a join without a fork, a nested or
 * second fork, a switch outside the region and a branch other than 0 / 1; pmn_plan_end with the region still open fails too (and
 * the plan is then unusable).  Fork and join are recorded as marker entries: they count in pmn_plan_count, pmn_plan_kernel_name
 * gives "<fork>" / "<join>" for them, and pmn_plan_entry_branch(plan, i) is the i-th entry's tag (markers: 0).
 *
 * pmn_plan_launch replays a plan with a region exactly as one without: every launch, in recorded order, on `stream` -- correct, no
 * overlap.  pmn_plan_launch_part(plan, part, stream) enqueues ONE part, in recorded order, on `stream`: PMN_PLAN_PART_PRE the launches
 * before the fork (all of them in a plan without a region), _SIDE / _MAIN the region's two branches, _POST those after the join.  The
 * ordering BETWEEN streams is the caller's, because no entry point of this library creates a stream or waits for an event:
 *
 *   launch_part(PRE, s);  record e0 on s;  make `side` wait for e0;  launch_part(SIDE, side);  launch_part(MAIN, s);
 *   record e1 on side;  make s wait for e1;  launch_part(POST, s)
 *
 * (patchmatchnet_amd/graph.py: PlannedForward._replay).  Two replays of one plan stay ordered on `s`: replay n+1's e0 is recorded
 * behind replay n's wait for e1. */
#define PMN_PLAN_PART_PRE 0
#define PMN_PLAN_PART_SIDE 1
#define PMN_PLAN_PART_MAIN 2
#define PMN_PLAN_PART_POST 3
int pmn_plan_create(void **plan_out);
int pmn_plan_begin(void *plan);
int pmn_plan_end(void *plan);
int pmn_plan_count(const void *plan);
const char *pmn_plan_kernel_name(const void *plan, int index);
int pmn_plan_launch(const void *plan, void *stream);
int pmn_plan_destroy(void *plan);
int pmn_plan_fork(void *plan);
int pmn_plan_switch(void *plan, int branch);
int pmn_plan_join(void *plan);
int pmn_plan_entry_branch(const void *plan, int index);
int pmn_plan_launch_part(const void *plan, int part, void *stream);

/* ABI 23.  View selection of the COLMAP import (reference colmap_input.py:336-366): the full N x N float64 score matrix of every
 * image pair, score[i][j] = score[j][i] = sum over the observations of image min(i,j), in that image's order, of the points also
 * observed by image max(i,j), of exp(-(theta - theta0)^2 / (2 sigma^2)) (theta = the triangulation angle in degrees, sigma = sigma1
 * for theta <= theta0, else sigma2); score[i][i] = 0.  Every entry is written (no memset needed).  Inputs, all DEVICE and contiguous:
 *   cam_centers [N][3] float64 (-R^T t), xyz [P][3] float64 (points indexed densely 0..P-1);
 *   obs_ptr [N+1] int64 / obs_pt [n_obs] int32: per image its observations in the image's own order, untriangulated entries dropped,
 *     duplicates kept (CSR; obs_ptr[N] == n_obs);
 *   trk_ptr [P+1] int64 / trk_img [n_trk] int32: per point the DISTINCT images observing it, ascending (CSR; trk_ptr[P] == n_trk).
 * Each score is a sequential float64 sum in that order: the same bits on every run; IEEE operations without contraction, so a point
 * at a camera centre (or an acos argument beyond +-1) gives NaN as numpy does.  One launch of N x ceil(N / 4096) one-wave workgroups. */
int pmn_view_scores(const double *cam_centers, const double *xyz, const long long *obs_ptr, const int *obs_pt,
                    const long long *trk_ptr, const int *trk_img, int N, int P, long long n_obs, long long n_trk,
                    double theta0, double sigma1, double sigma2, double *score, void *stream);

/* ABI 24.  Ground-truth depth metrics of validation (train.py --mode test; reference train.py:127-181, utils.py:170-221,
 * models/net.py:321-342), for one batch: one row of RAW float64 sums and exact counts per sample, from which the host forms the
 * reference's loss, depth-error-stage-i and threshold-{t}mm-error (patchmatchnet_amd/validate.py).
 *   depth_gt [B][H][W] float32, depth_min [B] float32: the valid pixels of stage 0 are depth_gt >= depth_min[b] (IEEE: NaN is not valid);
 *     stage s reads the nearest down-sampling gt[y << s][x << s] and its mask, as F.interpolate(scale_factor=2^-s, mode="nearest");
 *   maps_host: HOST array of DEVICE pointers, stage-major: stage s contributes iters_host[s] maps (1..PMN_METRICS_MAX_ITERS) of
 *     [B][H >> s][W >> s] float32 each, in iteration order -- depth_patchmatch of the forward, stage 0 = the refined map;
 *   hw_host: HOST int[2 * stages], each stage's map height and width; anything but floor(H / 2^s) x floor(W / 2^s), or an empty stage,
 *     is PMN_ERR_SHAPE (the model's maps of an image whose sides are not multiples of 8 are not down-samplings of its ground truth);
 *   thresholds_host: HOST float[n_thresholds], n_thresholds <= PMN_METRICS_MAX_THRESHOLDS (the reference uses 1, 2, 4, 8).
 * Row of sample b (rows [B][PMN_METRICS_ROW] float64; entries of absent stages / iterations / thresholds are 0):
 *   [PMN_METRICS_COUNT + s]                           valid pixels of stage s
 *   [PMN_METRICS_ABS + s]                             sum |d - gt| over them, d = the LAST map of stage s
 *   [PMN_METRICS_THR + t]                             count of |d - gt| > thresholds[t] at stage 0 (last map)
 *   [PMN_METRICS_SL1 + s * PMN_METRICS_MAX_ITERS + k] sum smooth-L1(d - gt), beta = 1, of iteration k of stage s
 * Per element fp32 as torch computes it (z = |d - gt|; z < 1 ? 0.5 * z * z : z - 0.5), a NaN estimate is not above any threshold but
 * makes the sums NaN, the sums are fp64.  scratch: DEVICE float64 of at least PMN_METRICS_SCRATCH(B, H, W) elements (per-workgroup
 * partial rows; the caller owns it, nothing needs zeroing).  Two launches: the partial rows, then their sum in workgroup order --
 * deterministic, the same bits on every run and stream. */
#define PMN_METRICS_MAX_STAGES 4
#define PMN_METRICS_MAX_ITERS 5
#define PMN_METRICS_MAX_THRESHOLDS 8
#define PMN_METRICS_COUNT 0
#define PMN_METRICS_ABS 4
#define PMN_METRICS_THR 8
#define PMN_METRICS_SL1 16
#define PMN_METRICS_ROW 36
#define PMN_METRICS_PIXELS_PER_BLOCK 4096
#define PMN_METRICS_MAX_BLOCKS 128
/* workgroups per sample: ceil(H * W / PMN_METRICS_PIXELS_PER_BLOCK), at most PMN_METRICS_MAX_BLOCKS */
#define PMN_METRICS_BLOCKS(H, W)                                                                                                     \
    ((int)((((long long)(H) * (W) + PMN_METRICS_PIXELS_PER_BLOCK - 1) / PMN_METRICS_PIXELS_PER_BLOCK) > PMN_METRICS_MAX_BLOCKS        \
               ? PMN_METRICS_MAX_BLOCKS                                                                                               \
               : (((long long)(H) * (W) + PMN_METRICS_PIXELS_PER_BLOCK - 1) / PMN_METRICS_PIXELS_PER_BLOCK)))
#define PMN_METRICS_SCRATCH(B, H, W) ((long long)(B) * PMN_METRICS_BLOCKS(H, W) * PMN_METRICS_ROW)
int pmn_depth_metrics(const float *depth_gt, const float *depth_min, const float *const *maps_host, const int *iters_host,
                      const int *hw_host, int stages, const float *thresholds_host, int n_thresholds, int B, int H, int W,
                      double *scratch, long long scratch_doubles, double *rows, void *stream);

/* ABI 25.  The two searches of the DTU point-cloud score (reference evaluations/dtu/MaxDistCP.m and reducePts_haa.m, MATLAB KD-trees on
 * the CPU; patchmatchnet_amd/pointcloud.py and eval_dtu.py are the callers).  Both read a UNIFORM GRID OVER SORTED POINTS that the caller
 * builds (pointcloud.build_grid):
 *   origin_host HOST double[3], cell > 0, dims_host HOST int[3] (1 .. 2^30 each, product < 2^62, else PMN_ERR_SHAPE);
 *   a point's cell along an axis is floor((double(p) - origin) / cell), 0 <= cell index < dims, its key
 *   (cz * dims[1] + cy) * dims[0] + cx;  xyz [n][3] float32 and keys [n] int64 hold the points and their keys in ASCENDING KEY ORDER.
 *   There is no cell table: x is the fastest axis of the key, so a row of cells is one contiguous range of the sorted points, found by
 *   binary search over the keys, and the memory of a grid does not depend on its extent.
 * Every distance is sqrt(dx*dx + dy*dy + dz*dz) of the float32 coordinates widened to float64, products and sums in float64 in x, y, z
 * order, no fused multiply-add; "nearest" and "within dst" are decided on that value.  Non-finite coordinates are the caller's error
 * (the Python layer counts and rejects them).  n, n_to, n_from: 1 .. 2^31 - 65.
 *
 * pmn_nn_distance: for each of the n_from query points ([n_from][3] float32, any position, inside the grid or not) the distance to the
 * nearest of the n_to grid points, capped: dist[q] = min(d, max_dist) (float64 [n_from], indexed as `query`).  index, if not NULL
 * (int32 [n_from]), receives the position IN THE SORTED ORDER of a nearest point, -1 where the result is the cap (tests use it).
 * order, if not NULL (int32 [n_from], a permutation), is the sequence in which queries are taken: pass the queries' own cell order so
 * that the lanes of a wave walk the same cells (any order gives the same output).  The search visits the query's cell, then shells of
 * growing Chebyshev radius, and ends when the best distance is no larger than the distance to the nearest face of the next shell or the
 * shell lies beyond max_dist.  The kernel knows nothing of DTU: MaxDistCP.m's 60-unit blocks are applied by the caller, and where the
 * MATLAB (which searches only the to-points of the block grown by MaxDist and does not clamp) returns some value >= MaxDist for a point
 * with no neighbour within MaxDist, this returns MaxDist.  Every consumer keeps only distances < 20, so no score can differ.
 * One launch of ceil(n_from / 64) one-wave workgroups.
 *
 * pmn_reduce_round: one round of the parallel form of reducePts_haa.m (visit the points in a given order; a point still kept removes
 * every point within dst, distance <= dst, and stays: the greedy maximal independent set of that order).  rank [n] int32: the position
 * of each SORTED point in the visiting order (a permutation of 0..n-1).  state [n] uint8, zeroed by the caller before the first round:
 * 0 undecided, 1 kept, 2 removed.  In a round every undecided point scans its neighbours within dst: it becomes removed if one of lower
 * rank is kept, kept if every one of lower rank is removed, and otherwise stays undecided.  state is updated IN PLACE and only ever
 * leaves 0: a decision rests on neighbours' final states alone, so reading a neighbour before or after it was decided in the same round
 * changes when a point is decided, never what it becomes.  The number of points still undecided after the round is ADDED to *counter
 * (uint32, zeroed by the caller; one atomicAdd per wave).  The caller launches rounds until a round adds zero; the fixed point is the
 * sequential greedy set of the order, the same bits on every run.  Identical points (distance 0) are neighbours like any others.
 * dst >= 0; dst / cell above 1024 is PMN_ERR_SHAPE (cells of about 2 dst keep the candidate lists short). */
int pmn_nn_distance(const float *to_xyz, const long long *to_keys, long long n_to, const double *origin_host, double cell,
                    const int *dims_host, const float *query, const int *order, long long n_from, double max_dist, double *dist,
                    int *index, void *stream);
int pmn_reduce_round(const float *xyz, const long long *keys, long long n, const double *origin_host, double cell,
                     const int *dims_host, double dst, const int *rank, unsigned char *state, unsigned int *counter, void *stream);

/* Added under ABI 25 (purely additive: three tests of the existing suite pin the number).  A surface mesh from the depth maps (the reference has no mesher; tests/tsdf_ref.py is the numpy form).
 *
 * The volume is a dense lattice of dims_host = {nx, ny, nz} samples (HOST int[3]; nz <= 65535, nx * ny * nz < 2^31, else PMN_ERR_SHAPE),
 * x fastest, sample (i, j, k) at origin_host[c] + (float)index * voxel per coordinate (HOST float[3], world units).  Planes, all DEVICE
 * float32 [nz][ny][nx] owned and initialised by the caller: tsdf (1), weight (0) and -- both or neither -- rgb [3][nz][ny][nx] and
 * cweight (0).
 *
 * pmn_tsdf_integrate folds n_views (1 .. PMN_TSDF_MAX_VIEWS) depth maps into the volume in ONE launch.  The views are addressed as
 * pmn_fuse_view addresses them: maps + slots_host[v] * slot_stride is the depth map [h_v][w_v] of view v, hw_host = HOST int[2 n_views]
 * (height, width; h * w <= slot_stride).  masks_host / images_host: NULL, or HOST arrays of n_views DEVICE pointers (entries may be NULL)
 * to a uint8 mask [h][w] (pmn_fuse_view's final mask: zero = ignore the pixel) and a uint8 image [h][w][3].  cams_host: HOST
 * float[21 n_views] = K row-major at the MAP's size, then the upper 3 x 4 of the world-to-camera extrinsic row-major; all finite.
 * Per sample p and per view, in view order, float32, no contraction, IEEE division:
 *   pc_r = ((R_r0 p.x + R_r1 p.y) + R_r2 p.z) + t_r; skip if pc.z <= 0.  q_r = (K_r0 pc.x + K_r1 pc.y) + K_r2 pc.z.
 *   fx = floorf(q.x / q.z + 0.5f), fy likewise; skip unless 0 <= fx < w and 0 <= fy < h (as floats; NaN is outside); nearest pixel.
 *   d = depth[fy][fx]; skip unless 0 < d < inf and the mask byte is non-zero.  sdf = d - pc.z; skip if sdf < -trunc.
 *   obs = fminf(1, sdf / trunc); tsdf = (tsdf * weight + obs) / (weight + 1); weight += 1; with colour planes, an image and
 *   sdf <= trunc: rgb_c = (rgb_c * cweight + (float)byte_c) / (cweight + 1); cweight += 1.
 * A batch of V views leaves exactly the bits of V single-view calls.  voxel, trunc > 0 and finite, else PMN_ERR_ARG.
 *
 * pmn_mt_count / pmn_mt_emit: the iso-surface tsdf = 0 by marching tetrahedra on the Kuhn split (six tetrahedra {0, a, a|b, 7} per cell,
 * (a, b) in lexicographic order over the axis bits 1, 2, 4), indexed and closed wherever the volume is observed.  A cell is live iff its
 * eight corners have weight >= min_weight; an edge lo -> hi (lo a subset of hi) belongs to the sample at lo with class hi ^ lo (1..7) and
 * carries a vertex iff tsdf < 0 differs at its ends and a live cell contains it.  pmn_mt_count writes vertex_mask [nz][ny][nx] (bit
 * class - 1 = the sample owns a vertex on its edge of that class) and cell_triangles [nz][ny][nx] (0..12, indexed by the cell's corner 0;
 * a sample on the last plane of an axis owns no cell and gets 0).  The caller scans both (INCLUSIVE int32 prefix sums of
 * popcount(vertex_mask) and of cell_triangles, x fastest; the totals must fit int32) and allocates the outputs.  pmn_mt_emit writes
 * vertices [Nv][3] (p_lo + t (p_hi - p_lo) per coordinate, t = v_lo / (v_lo - v_hi)), colors [Nv][3] uint8 or NULL (needs the colour
 * planes; floorf(c + 0.5f) of the interpolated colour; an end with cweight 0 takes the other end's, both 0 give 128), normals [Nv][3] or
 * NULL (the central differences tsdf[s + e] - tsdf[s - e] of both ends interpolated with t, normalised; zero where one of the twelve
 * neighbours is outside the lattice or below min_weight) and faces [Nt][3] int32, wound so that the normal points from tsdf < 0 to
 * tsdf > 0.  Order: vertices by owning sample then class; triangles by cell, tetrahedron, triangle.  One launch each. */
int pmn_tsdf_integrate(float *tsdf, float *weight, float *rgb, float *cweight, const int *dims_host, const float *origin_host,
                       float voxel, float trunc, const float *maps, long long slot_stride, const int *slots_host,
                       const int *hw_host, const void *const *masks_host, const void *const *images_host, const float *cams_host,
                       int n_views, void *stream);
int pmn_mt_count(const float *tsdf, const float *weight, const int *dims_host, float min_weight, unsigned char *vertex_mask,
                 unsigned char *cell_triangles, void *stream);
int pmn_mt_emit(const float *tsdf, const float *weight, const float *rgb, const float *cweight, const int *dims_host,
                const float *origin_host, float voxel, float min_weight, const unsigned char *vertex_mask,
                const unsigned char *cell_triangles, const int *vertex_scan, const int *triangle_scan, float *vertices,
                unsigned char *colors, float *normals, int *faces, void *stream);

/* Added under ABI 25 (purely additive, as above).  The same volume stored in blocks: a scene whose dense lattice
 * would not fit keeps its natural voxel.  dims_host = {nx, ny, nz} is the VIRTUAL lattice, defined as above (2 <= n < 2^19 per axis, so
 * (float)index is exact); it is cut into blocks of 8 x 8 x 8 samples, nb = ceil(n / 8) per axis, nbx * nby * nbz <= 2^28, else
 * PMN_ERR_SHAPE.  All arrays are the caller's:
 *   table  DEVICE int32 [nbz][nby][nbx]  the block's slot in the pool, or -1
 *   blocks DEVICE int32 [n_blocks]       the linear block index ((bz * nby + by) * nbx + bx) of every slot, ascending;
 *                                        1 <= n_blocks, n_blocks * 512 < 2^31, else PMN_ERR_SHAPE
 *   pool   DEVICE float32 tsdf [n_blocks][8][8][8] (initially 1), weight (0) and -- both or neither -- rgb [3][n_blocks][8][8][8] and
 *          cweight (0); x fastest inside a block
 * A sample of a border block with an index >= n is outside the lattice: never integrated, never meshed.  A sample outside the lattice or
 * in a block without a slot reads as tsdf 1, weight 0, cweight 0.
 *
 * pmn_tsdf_mark_blocks sets flags (DEVICE uint8 [nbz][nby][nbx], zeroed by the caller once; several calls accumulate) to 1 for every
 * block that may hold a sample which pmn_tsdf_integrate would map to a valid pixel (finite depth > 0, mask byte non-zero) with
 * |sdf| <= trunc: per pixel (u, v) of depth d the section of the pyramid through (u +- 0.5, v +- 0.5) between the camera depths
 * max(d - trunc, 0) and d + trunc is taken to the world, its axis-aligned box grown by one voxel and clipped to the lattice, and every
 * block the box touches is flagged.  inv_cams_host: HOST float[21 n_views] = K^-1 row-major, then the upper 3 x 4 of the
 * CAMERA-TO-WORLD matrix E^-1 row-major, inverted by the caller in float64; all finite.  The other view arguments are
 * pmn_tsdf_integrate's.  A box that touches more than PMN_TSDF_MARK_SPAN blocks on an axis, or has no finite position, is not marked:
 * it adds 1 to *overflow (DEVICE int32, zeroed by the caller), which the caller reads together with the flags.  The flags are a
 * superset of the band; the caller dilates them by one block in all 26 directions before it builds table, blocks and pool, which makes
 * the mesh below the dense one bit for bit (the argument is in DESIGN.md section 18).
 *
 * pmn_tsdf_integrate_blocks is pmn_tsdf_integrate on the samples of the listed blocks: the same operations in the same order, so a
 * pool sample holds the bits the dense volume holds at that lattice index.
 *
 * pmn_mt_count_blocks / pmn_mt_emit_blocks are pmn_mt_count / pmn_mt_emit over the pool, with neighbours across block faces found
 * through table.  min_weight > 0 (else PMN_ERR_ARG): a sample without a slot is unobserved.  vertex_mask, cell_triangles and the two
 * INCLUSIVE int32 scans are [n_blocks][8][8][8] in pool order; so is the output: vertices by slot, sample within the block (x fastest),
 * class; triangles by slot, cell, tetrahedron, triangle.  One launch each; no atomics decide a position. */
int pmn_tsdf_mark_blocks(unsigned char *flags, int *overflow, const int *dims_host, const float *origin_host, float voxel, float trunc,
                         const float *maps, long long slot_stride, const int *slots_host, const int *hw_host,
                         const void *const *masks_host, const float *inv_cams_host, int n_views, void *stream);
int pmn_tsdf_integrate_blocks(float *tsdf, float *weight, float *rgb, float *cweight, const int *blocks, int n_blocks,
                              const int *dims_host, const float *origin_host, float voxel, float trunc, const float *maps,
                              long long slot_stride, const int *slots_host, const int *hw_host, const void *const *masks_host,
                              const void *const *images_host, const float *cams_host, int n_views, void *stream);
int pmn_mt_count_blocks(const float *tsdf, const float *weight, const int *table, const int *blocks, int n_blocks,
                        const int *dims_host, float min_weight, unsigned char *vertex_mask, unsigned char *cell_triangles, void *stream);
int pmn_mt_emit_blocks(const float *tsdf, const float *weight, const float *rgb, const float *cweight, const int *table,
                       const int *blocks, int n_blocks, const int *dims_host, const float *origin_host, float voxel, float min_weight,
                       const unsigned char *vertex_mask, const unsigned char *cell_triangles, const int *vertex_scan,
                       const int *triangle_scan, float *vertices, unsigned char *colors, float *normals, int *faces, void *stream);

/* Added under ABI 25 (purely additive, as above).  A mesh or a cloud drawn into one camera (the reference has no
 * renderer; tests/render_ref.py is the numpy form).  cam_host: HOST float[21] = K row-major at the OUTPUT's size, then the upper 3 x 4 of
 * the world-to-camera extrinsic row-major (tsdf.camera21), all finite.  1 <= h, w <= PMN_RASTER_MAX_DIM, else PMN_ERR_SHAPE.
 *
 * keys: DEVICE uint64 [h][w], set to all ones by the caller; key = (uint64)float_bits(depth) << 32 | primitive index, updated with one
 * 64-bit atomic min per covered pixel: the nearest depth wins and, among equal depths, the lowest index -- independent of the order of
 * the primitives, of the launch shape and of the run.  Several calls may draw into the same keys (the indices are then the caller's to
 * tell apart).  counters: DEVICE int32[4], zeroed by the caller before EVERY call: [0] primitives with a vertex whose camera-frame
 * position is not finite or has z <= 0 (or, for a triangle, a vertex index outside [0, n_vertices)), [1] primitives with a vertex
 * outside the guard band, [2] zero-area triangles, [3] triangles handed to the wave-per-triangle kernel.  Primitives counted in
 * [0]..[2] are NOT DRAWN; there is no near-plane clipping.
 *
 * Projection of a world point p, float32, no contraction, IEEE division:
 *   pc_r = ((R_r0 p.x + R_r1 p.y) + R_r2 p.z) + t_r;  q_r = (K_r0 pc.x + K_r1 pc.y) + K_r2 pc.z;  u = q.x / q.z;  v = q.y / q.z
 *   X = rintf(u * 256.0f), Y = rintf(v * 256.0f) (half to even); guard band |X|, |Y| <= 2^22 (16384 px): coordinate differences stay
 *   within 2^23 and the 64-bit edge functions within 2^47.  Pixel centres are at integer coordinates: P = (256 px, 256 py).
 * pmn_raster_triangles (vertices [n_vertices][3] float32 world, faces [n_faces][3] int32), all coverage arithmetic in integers:
 *   orient(a, b, c) = (b.X - a.X)(c.Y - a.Y) - (b.Y - a.Y)(c.X - a.X);  w0 = orient(v1, v2, P), w1 = orient(v2, v0, P),
 *   w2 = orient(v0, v1, P), area = orient(v0, v1, v2), s = sign(area) (both windings are drawn, area = 0 is dropped).  Edge i (v1->v2,
 *   v2->v0, v0->v1) with (dx, dy) = s (end - start) is top-left iff dy < 0 or (dy = 0 and dx > 0); P is covered iff for every i
 *   s w_i > 0, or s w_i = 0 and edge i is top-left.  Depth: b_i = (float)(s w_i) / (float)(s area), c_i = b_i / pc_i.z,
 *   depth = 1.0f / ((c0 + c1) + c2); written only if 0 < depth < inf.
 *   A triangle whose bounding box (clipped to the image) holds at most max_box pixels (0 = PMN_RASTER_MAX_BOX) is drawn by one thread;
 *   a larger one is appended to worklist (DEVICE int32 [n_faces], contents undefined afterwards) and drawn by waves of a second
 *   kernel (eight per triangle, a lane per pixel).  Two launches, nothing is read back.
 * pmn_splat_points (points [n_points][3], n_points < 2^31: the index plane is int32): depth = pc.z, index = the point's.  Footprint: the nearest pixel
 *   ((X + 128) >> 8, (Y + 128) >> 8) always and, with r > 0, every pixel with (256 px - X)^2 + (256 py - Y)^2 <= Rq^2,
 *   Rq = (int)rintf(r * 256.0f); r = radius_px (0 .. PMN_SPLAT_MAX_RADIUS) or, with radius_world > 0 (then radius_px must be 0),
 *   fminf((radius_world * K_00) / pc.z, PMN_SPLAT_MAX_RADIUS).  A cloud sparser than its footprint is see-through.  One launch.
 * pmn_raster_resolve, one thread per pixel: depth [h][w] float32 (0 where the key is untouched), index [h][w] int32 (-1), and, if not
 *   NULL, rgb [h][w][3] uint8 (0) and normal [h][w][3] float32 camera frame (0).  faces = NULL (n_faces = 0): the primitives were points
 *   and vertices are the points.  colors [n_vertices][3] uint8 or NULL (then 128), normals [n_vertices][3] float32 world or NULL.  For a
 *   triangle the winner's c_i are recomputed from the same integers and an attribute a is ((c0 a0 + c1 a1) + c2 a2) * depth
 *   (perspective-correct), the camera-frame position p likewise from the pc_i; vertex normals are interpolated in the world frame and
 *   then rotated, n_r = (R_r0 n.x + R_r1 n.y) + R_r2 n.z; without vertex normals n = (pc1 - pc0) x (pc2 - pc0).  A point takes its own
 *   colour, normal and pc.  n = n / sqrtf((n.x n.x + n.y n.y) + n.z n.z) (0 if that length is 0 or not finite), negated if
 *   d = (n.x p.x + n.y p.y) + n.z p.z > 0 (COLMAP's convention: the normal faces the camera).  With shade != 0 and a non-zero normal the
 *   colour is multiplied by |d| / |p| (head-light Lambert); bytes are floorf(c + 0.5f) clamped to 0..255, as pmn_mt_emit rounds. */
int pmn_raster_triangles(const float *vertices, int n_vertices, const int *faces, int n_faces, const float *cam_host, int h, int w,
                         long long max_box, unsigned long long *keys, int *counters, int *worklist, void *stream);
int pmn_splat_points(const float *points, long long n_points, const float *cam_host, int h, int w, float radius_px, float radius_world,
                     unsigned long long *keys, int *counters, void *stream);
int pmn_raster_resolve(const unsigned long long *keys, int h, int w, const float *cam_host, const float *vertices, long long n_vertices,
                       const int *faces, long long n_faces, const unsigned char *colors, const float *normals, int shade, float *depth,
                       int *index, unsigned char *rgb, float *normal, void *stream);

/* Added under ABI 25 (purely additive, as above).  The registration, downsample and crop behind the Tanks and Temples F-score (DESIGN.md
 * section 17; patchmatchnet_amd/registration.py and eval_tnt.py are the callers, tests/tnt_ref.py is the numpy form).  Float64 throughout,
 * products and sums in the written order, no fused multiply-add.  A pose is pose_host = HOST double[12], row-major 3 x 4 [R | t], finite;
 * the posed point is p'_r = R_r0 * x + R_r1 * y + R_r2 * z + t_r, evaluated from left to right on the float32 coordinates widened to
 * float64.  n: 1 .. 2^31 - 65.
 *
 * pmn_icp_accumulate: one ICP iteration's search and reduction in one pass.  The first six arguments are pmn_nn_distance's grid (the
 * TARGET cloud).  For each of the n source points (src [n][3] float32; order as pmn_nn_distance's, NULL = identity) the nearest target
 * point q of the query p' is found exactly as pmn_nn_distance finds it -- same shell walk, same comparisons; p' is NOT rounded to
 * float32 -- and a pair whose distance is at or beyond max_dist is no match.  With a = p' - centre and b = (double)q - centre
 * (centre_host = HOST double[3], finite) sums [PMN_ICP_SUMS] float64 receives over the matched pairs: [0] their number, [1..3] the sum of
 * a, [4..6] of b, [7..15] of a_i * b_j (row-major, each product rounded once), [16] of |q - p'|^2 = dx * dx + dy * dy + dz * dz.
 * Every sum is EXACT up to its last step: a term is scaled by a power of two derived on the host from the grid's extent, centre and
 * max_dist (which bound every term of a matched pair), cut into PMN_ICP_LIMBS signed 32-bit digits and added in 64-bit INTEGERS -- a
 * wave by a butterfly, a workgroup (one wave, PMN_ICP_BLOCK_POINTS points) into its row of scratch, a second launch over the rows --
 * and, the carries propagated, the integer total is rounded to float64 ONCE (to nearest, ties to even).  Integer addition is
 * associative, so sums does not depend on the schedule, on the run, on the launch shape, on the grid's cell or on order, bit for bit;
 * there are no atomics.  Its error is below half an ulp of the sum + n * 2^-155 * (bound of the sum's terms).  No match at all
 * gives seventeen zeros.  scratch: DEVICE, PMN_ICP_SCRATCH(n) 8-byte words (scratch_doubles states its size, else PMN_ERR_ARG),
 * contents undefined before and after.  PMN_ERR_SHAPE if a bound's exponent leaves +-800.  Two launches.
 *
 * pmn_voxel_mean: the mean of every run of a sorted grid.  xyz [n][3] float32 and, if not NULL, attr [n][channels] float32
 * (1 .. PMN_VOXEL_MAX_CHANNELS columns: colours, normals), both in ascending key order; starts [m + 1] int64 = the first index of every
 * run of equal keys, then n (strictly increasing, starts[0] = 0: the caller's to get right).  Per run and column: the float64 sum of the
 * run's values divided by its length in float64, rounded to float32 once, into out_xyz [m][3] / out_attr [m][channels].  A run of at most
 * PMN_VOXEL_LONG_RUN points is summed by one lane in index order, starting from 0.0.  A longer run is summed by a wave: lane l adds
 * the points l, l + 64, ... of the run in index order to 0.0, and the 64 values meet in the butterfly x_l += x_(l ^ 32), then ^ 16, 8,
 * 4, 2, 1 -- a fixed tree (tnt_ref.voxel_mean restates it).  One launch.
 *
 * pmn_crop_prism: mask [n] uint8 = 1 for the points inside a polygon extruded along a coordinate axis (the toolbox's crop volume).
 * polygon: DEVICE double [k][2], 3 <= k <= PMN_CROP_MAX_VERTICES (else PMN_ERR_SHAPE), the vertices in cyclic order, given in the two
 * axes other than axis in ascending order ((y, z) for axis 0, (x, z) for 1, (x, y) for 2).  pose_host, if not NULL, is applied first.
 * With c the coordinate along axis and (px, py) the other two, a point is inside iff axis_min <= c && c <= axis_max and `inside` is set
 * after   for i in 0..k-1, j = i - 1 (cyclically):  if ((yi > py) != (yj > py) && px < (xj - xi) * (py - yi) / (yj - yi) + xi)
 * inside = !inside   (even-odd rule; float64, that order of operations).  One launch. */
#define PMN_ICP_SUMS 17
#define PMN_ICP_LIMBS 5
#define PMN_ICP_BLOCK_POINTS 256
#define PMN_ICP_BLOCKS(n) (((long long)(n) + PMN_ICP_BLOCK_POINTS - 1) / PMN_ICP_BLOCK_POINTS)
#define PMN_ICP_SCRATCH(n) (PMN_ICP_BLOCKS(n) * PMN_ICP_SUMS * PMN_ICP_LIMBS)
#define PMN_VOXEL_LONG_RUN 256
#define PMN_VOXEL_MAX_CHANNELS 8
#define PMN_CROP_MAX_VERTICES 4096
int pmn_icp_accumulate(const float *to_xyz, const long long *to_keys, long long n_to, const double *origin_host, double cell,
                       const int *dims_host, const float *src, const int *order, long long n, const double *pose_host,
                       const double *centre_host, double max_dist, double *scratch, long long scratch_doubles, double *sums,
                       void *stream);
int pmn_voxel_mean(const float *xyz, const float *attr, int channels, long long n, const long long *starts, long long m, float *out_xyz,
                   float *out_attr, void *stream);
int pmn_crop_prism(const float *xyz, long long n, const double *polygon, int k, int axis, double axis_min, double axis_max,
                   const double *pose_host, unsigned char *mask, void *stream);

/* Added under ABI 25 (purely additive, as above).  Operations on an indexed triangle mesh (the reference has none;
 * patchmatchnet_amd/meshops.py is the caller, tests/meshops_ref.py the numpy form).  faces: DEVICE int32 [n_faces][3] into n_vertices
 * vertices (vertices: DEVICE float32 [n_vertices][3]); 1 <= n_vertices, n_faces <= 2^31 - 256, else PMN_ERR_SHAPE.  A face with an index
 * outside [0, n_vertices) is NEVER dereferenced: the kernel that meets it skips it and adds 1 to *invalid (DEVICE int32, zeroed by the
 * caller), which the caller reads together with the host read it needs anyway.  Integer atomics only; no result depends on the order
 * of the faces' arrival, on the launch shape or on the run.
 *
 * pmn_mesh_components: label [n_vertices] int32 = the SMALLEST vertex index of the vertex's connected component; two vertices are
 * connected when some face names both, a vertex that no face names is its own component, (a, a, b) unites a and b, (a, a, a) nothing.
 * n_faces may be 0 (faces is then not read).  Union-find in label itself: an init launch (label[v] = v), a launch with a thread per face
 * that unites (a, b) and (b, c) -- find both roots, hook the larger root under the smaller with a 32-bit compare-and-swap on the larger
 * root's slot, on failure go on from the value the swap returned -- and a launch that replaces every entry by its root.  Slots only ever
 * decrease, so every walk and every retry loop descends and ends whatever it reads, no lane waits for another lane (no lock, no flag, no
 * spin), and the final root is the component's minimum whatever the interleaving.  All accesses of label in the last two launches are
 * relaxed agent-scope atomics; path halving is a best-effort store of a smaller ancestor.  Three launches.
 *
 * pmn_mesh_face_samples / pmn_mesh_sample: points on the triangles at `density` (finite, > 0) points per unit area, a function of
 * (mesh, density, seed) alone.  All randomness comes from the splitmix64 finaliser
 *   mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31        (mod 2^64)
 *   h(face, k) = mix(mix(seed + G) + (((uint64)face << 32 | k) + 1) * G),  G = 0x9E3779B97F4A7C15
 *   r1 = (h >> 40) * 2^-24,  r2 = ((h >> 16) & 0xFFFFFF) * 2^-24        (exact in float32, in [0, 1))
 * Float32, no contraction, IEEE sqrtf, with A, B, C the face's vertices in its order:
 *   counts[f] (int32 [n_faces]) = floor((double)area * density + (double)u) in float64, u = the r1 of k = 2^32 - 1 (unbiased rounding),
 *   area = sqrtf((c.x c.x + c.y c.y) + c.z c.z) * 0.5f, c = (B - A) x (C - A) = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z,
 *   e1.x e2.y - e1.y e2.x); 0 for an area that is not finite or not > 0 and for a face with a bad index; clamped at 2^31 - 1.
 *   The caller scans the counts (INCLUSIVE, int64: sample_scan [n_faces]) and reads the total n_samples (1 .. 2^31 - 1).
 *   Sample i (a thread each) belongs to the first face f with sample_scan[f] > i (binary search), k = i - sample_scan[f - 1]:
 *   s = sqrtf(r1), b0 = 1 - s, b1 = s * (1 - r2), b2 = s * r2;  points [n_samples][3] = (b0 * A + b1 * B) + b2 * C per coordinate;
 *   face [n_samples] int32 = f; and, if out_colors is not NULL (then colors, uint8 [n_vertices][3], must not be), out_colors
 *   [n_samples][3] uint8 = the same blend of the bytes as floats, floorf(c + 0.5f) clamped to 0..255, as pmn_mt_emit rounds.
 *   Samples are ordered by face, then k.  One launch each. */
int pmn_mesh_components(const int *faces, int n_faces, int n_vertices, int *label, int *invalid, void *stream);
int pmn_mesh_face_samples(const float *vertices, int n_vertices, const int *faces, int n_faces, double density, unsigned long long seed,
                          int *counts, int *invalid, void *stream);
int pmn_mesh_sample(const float *vertices, int n_vertices, const int *faces, int n_faces, const unsigned char *colors,
                    const long long *sample_scan, long long n_samples, unsigned long long seed, float *points, int *face,
                    unsigned char *out_colors, void *stream);

/* Added under ABI 25.  Image undistortion of the COLMAP import (colmap_input.py --undistort): resamples a
 * distorted picture into an ideal pinhole camera.  src [Hs][Ws][channels] uint8 and dst [Hd][Wd][channels] uint8 are DEVICE,
 * contiguous, channels 1 or 3, each below 2^31 bytes.  model is COLMAP's camera model id and src_params_host its parameters in
 * COLMAP's order (HOST float64): 0 SIMPLE_PINHOLE (f cx cy), 1 PINHOLE (fx fy cx cy), 2 SIMPLE_RADIAL (f cx cy k), 3 RADIAL
 * (f cx cy k1 k2), 4 OPENCV (fx fy cx cy k1 k2 p1 p2), 5 OPENCV_FISHEYE (fx fy cx cy k1 k2 k3 k4), 6 FULL_OPENCV (fx fy cx cy k1 k2
 * p1 p2 k3 k4 k5 k6), 8 SIMPLE_RADIAL_FISHEYE (f cx cy k), 9 RADIAL_FISHEYE (f cx cy k1 k2); 7 (FOV), 10 (THIN_PRISM_FISHEYE) and
 * every other id are PMN_ERR_ARG.  dst_pinhole_host: HOST float64 fx' fy' cx' cy' of the output camera.  All parameters travel by
 * value in the kernel arguments.  Per output pixel (x, y), in float64, IEEE, without contraction, in this order:
 *   u = ((x + 0.5) - cx') / fx', v = ((y + 0.5) - cy') / fy';  (ud, vd) = the model's distortion of (u, v);
 *   sx = (fx * ud + cx) - 0.5, sy = (fy * vd + cy) - 0.5;  x0 = floor(sx), y0 = floor(sy), ax = sx - x0, ay = sy - y0;
 *   val = (1 - ay) * ((1 - ax) * s00 + ax * s01) + ay * ((1 - ax) * s10 + ax * s11) per channel, s.. = src[y0 + ..][x0 + ..];
 *   dst = floor(val + 0.5).
 * The pixel is valid iff x0 >= 0, y0 >= 0, x0 + 1 <= Ws - 1 and y0 + 1 <= Hs - 1, tested on the doubles so that NaN and infinity
 * fail; an invalid pixel is 0 in every channel and reads nothing.  valid (DEVICE uint8 [Hd][Wd], 1 / 0) and coords (DEVICE float64
 * [Hd][Wd][2] = (sx, sy) of every pixel, valid or not) may each be NULL.  Every byte of dst / valid / coords is written.  One launch. */
int pmn_undistort_image(const unsigned char *src, int Hs, int Ws, int channels, int model, const double *src_params_host,
                        const double *dst_pinhole_host, int Hd, int Wd, unsigned char *dst, unsigned char *valid, double *coords,
                        void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  The two searches behind outlier removal on a point cloud
 * (clean_cloud.py, pointcloud.statistical_outliers / radius_outliers; the reference has no counterpart).  Both
 * take pmn_nn_distance's grid (first six arguments), query, order and n_from, walk the grid as pmn_nn_distance walks it, and keep its
 * distance contract: squares dx*dx + dy*dy + dz*dz of the float32 coordinates widened to float64, x, y, z order, no contraction.
 * same_cloud != 0 says "query i IS grid point i" (n_from == n_to, else PMN_ERR_ARG): a query is never reported as, or counted among,
 * its own neighbours.  The exclusion is by index, never by distance: a duplicate at distance 0 is a neighbour.
 *
 * pmn_knn_distance: the k nearest grid points of every query, 1 <= k <= 32, max_dist positive and finite (else PMN_ERR_ARG).  Outputs,
 * each may be NULL: d2 [n_from][k] float64, the squared distances ascending; index [n_from][k] int32, their positions IN THE SORTED
 * ORDER, ties at equal d2 to the lower sorted index whatever the grid's cell; mean [n_from] float64 = (sum_j sqrt(d2_j)) / k, added
 * smallest first in float64.  A slot for which no point lies nearer than max_dist (d < max_dist, as pmn_nn_distance) holds
 * max_dist * max_dist and index -1, and enters the mean as max_dist itself.  A search ends when the walk's reach, slack included,
 * passes the k-th best.  One lane per query; the k-best list lives in registers (kernels specialised on a capacity of 8, 16 or 32).
 *
 * pmn_radius_count: count [n_from] int32 = the number of grid points with sqrt(d2) <= radius (decided on the rooted value), radius
 * finite and >= 0.  One launch each of ceil(n_from / 64) one-wave workgroups. */
int pmn_knn_distance(const float *to_xyz, const long long *to_keys, long long n_to, const double *origin_host, double cell,
                     const int *dims_host, const float *query, const int *order, long long n_from, int k, double max_dist,
                     int same_cloud, double *d2, int *index, double *mean, void *stream);
int pmn_radius_count(const float *to_xyz, const long long *to_keys, long long n_to, const double *origin_host, double cell,
                     const int *dims_host, const float *query, const int *order, long long n_from, double radius, int same_cloud,
                     int *count, void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  Normals of a point cloud from its neighbourhoods
 * (pointcloud.knn_normals / estimate_normals, cloud_normals.py; tests/cloud_normals_ref.py is the numpy form; the
 * reference has no counterpart).  The grid, query, order, n_from, k, max_dist and same_cloud are pmn_knn_distance's, and so is the
 * search: the same walk, the same comparisons, the same cap, the same exclusion of the query by index.  What differs is what the lane
 * does with its list.  Everything below is float64, IEEE, without contraction, from the float32 coordinates widened to float64.
 *
 * Neighbourhood: the slots of pmn_knn_distance's list that hold a point (index >= 0), in rank order j = 0 .. c - 1; a capped slot is
 * no neighbour, the point uses what it has.  The point set is the query q itself plus those c neighbours, m = 1 + c (on a cloud's own
 * points that is Open3D's knn = k + 1).
 * Moments: d_j = p_j - q per axis; s_a = sum_j d_ja (3 sums), M_ab = sum_j d_ja * d_jb (6 sums: xx xy xz yy yz zz), each started at 0
 * and added in rank order.  q is the zero delta and enters through m alone.  C_ab = M_ab - (s_a * s_b) / m.
 * Eigenvectors: A = C, V = I, then PMN_NORMAL_SWEEPS = 6 sweeps over the pairs (p, q) = (0, 1), (0, 2), (1, 2), r the third index.
 * A pair whose A_pq is exactly 0 is skipped; otherwise
 *   theta = (A_qq - A_pp) / (2 * A_pq);  root = |theta| + sqrt(theta * theta + 1);  t = theta < 0 ? -1 / root : 1 / root;
 *   c = 1 / sqrt(t * t + 1);  s = t * c;  h = t * A_pq;  A_pp -= h;  A_qq += h;  A_pq = 0;
 *   (A_rp, A_rq) = (c * A_rp - s * A_rq, s * A_rp + c * A_rq);  (V_ip, V_iq) = (c * V_ip - s * V_iq, s * V_ip + c * V_iq), i = 0, 1, 2.
 * The eigenvalues are the diagonal of A, sorted ascending l0 <= l1 <= l2 with equal values in column order; the normal is the column
 * of V that belongs to l0, as it stands (a product of rotations: a unit vector to a few ulp of float64; it is not renormalised).
 * Degenerate: the normal is (0, 0, 0) and the variation 0 when m < 3, when l2 == 0, or when l1 <= line_ratio * l2 (points on a line
 * define no plane; line_ratio finite and >= 0).  No other tolerance decides which points have a normal.
 * Sign: canonical = the component of largest magnitude is positive, the lowest axis among equal magnitudes.  With n_viewpoints > 0
 * (viewpoints: DEVICE float64 [n_viewpoints][3], at most 4096) the viewpoint c nearest to q is found by e = c - q per axis,
 * e.x * e.x + e.y * e.y + e.z * e.z, a later viewpoint winning only with a strictly smaller value; the canonical normal is negated
 * when n.x * e.x + n.y * e.y + n.z * e.z < 0, evaluated on the unrounded vector, and kept when that is exactly 0.  This is a
 * HEURISTIC: a fused cloud does not record which view wrote a point, so "the nearest camera saw it" is an assumption, wrong for
 * surfaces that face away from the camera that happens to be nearest.
 * Outputs, indexed as query: normal [n_from][3] float32 (not NULL), the float64 vector rounded once per component; variation [n_from]
 * float64 or NULL = l0 / (l0 + l1 + l2), the surface variation (rounding may leave it a few ulp below 0 on an exact plane); count
 * [n_from] int32 or NULL = m - 1, the neighbours used.  PMN_ERR_ARG for pmn_knn_distance's reasons, for n_viewpoints outside 0 ..
 * 4096 or non-zero with viewpoints NULL, and for a line_ratio that is negative or not finite.  One launch of ceil(n_from / 64) one-wave
 * workgroups, one lane per query, kernels specialised on the list's capacity (8, 16, 32); the lists are never written. */
#define PMN_NORMAL_SWEEPS 6
#define PMN_NORMAL_MAX_VIEWPOINTS 4096
int pmn_knn_normals(const float *to_xyz, const long long *to_keys, long long n_to, const double *origin_host, double cell,
                    const int *dims_host, const float *query, const int *order, long long n_from, int k, double max_dist,
                    int same_cloud, const double *viewpoints, int n_viewpoints, double line_ratio, float *normal, double *variation,
                    int *count, void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  Density clustering of a point cloud: DBSCAN with an
 * order-free border rule (pointcloud.cluster_dbscan, cluster_cloud.py; tests/dbscan_ref.py is the numpy form;
 * the reference has no counterpart).  The first six arguments are pmn_nn_distance's grid over the n points (n <= 2^31 - 256); the
 * cloud is its own query set with pmn_radius_count's same_cloud meaning, and every per-point array below is DEVICE, [n], in the
 * grid's SORTED order.  eps is finite and >= 0 with eps * eps finite, else PMN_ERR_ARG.  A pair (i, j) is WITHIN EPS when
 * sqrt(d2) <= eps, d2 = dx*dx + dy*dy + dz*dz of the float32 coordinates widened to float64, x, y, z order, no contraction: exactly
 * pmn_radius_count's test.
 *
 * pmn_cloud_core: core [n] uint8 = 1 where the points within eps of point i, ITSELF INCLUDED, number at least min_points (>= 1, else
 * PMN_ERR_ARG), that is pmn_radius_count(same_cloud) + 1 >= min_points, else 0.  One launch of ceil(n / 64) one-wave workgroups.
 *
 * pmn_cloud_dbscan: from core (as written by pmn_cloud_core with the same grid and eps),
 *   parent [n] int32: for a core point the smallest sorted index of its CLUSTER, the connected component of the graph on the core
 *     points whose edges are the core pairs within eps; for any other point its own index.  A lock-free union-find in parent itself
 *     (relaxed agent-scope integer atomics; no lane waits for another: csrc/union_find.hpp, csrc/cloud_cluster.hip).
 *   label [n] int32, or NULL (then orig is NULL too and the border launch is left out): a core point's parent; for a point that is not
 *     core the parent of the core point within eps that is least in (d2, orig) lexicographic order, a BORDER point, or -1 where no
 *     core point is within eps, NOISE.  orig [n] int32 names every sorted point's index in the caller's own order (the grid's
 *     permutation): the order of the sorted points inside a cell is the sort's, not the cloud's, so it must not decide a tie.
 * Core flags, the partition into clusters and the noise set are a function of (points, eps, min_points) alone -- not of the cell, the
 * order inside a cell, the launch shape or the run; only a cluster's NAME, a sorted index, depends on the grid.  Four launches
 * (init, link, flatten, border; one lane per point, the walking launches in one-wave workgroups); no floating-point atomics. */
int pmn_cloud_core(const float *xyz, const long long *keys, long long n, const double *origin_host, double cell, const int *dims_host,
                   double eps, long long min_points, unsigned char *core, void *stream);
int pmn_cloud_dbscan(const float *xyz, const long long *keys, long long n, const double *origin_host, double cell,
                     const int *dims_host, double eps, const unsigned char *core, const int *orig, int *parent, int *label,
                     void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  Planes in a point cloud: the two kernels of a seeded RANSAC
 * with a least-squares refit (pointcloud.segment_plane / segment_planes, segment_cloud.py; tests/plane_ref.py is
 * the numpy form; the reference has no counterpart).  xyz: DEVICE float32 [n][3], finite, 1 <= n <= 2^31 - 65; normals: DEVICE float32
 * [n][3] or NULL; active: DEVICE uint8 [n] or NULL (= every point).  Float64 throughout, products and sums in the written order, no fused
 * multiply-add; x, y, z, nx, ny, nz are the float32 values widened to float64.  For a plane (a, b, c, d) the residual of a point is
 * r = a * x + b * y + c * z + d, from left to right, and the point is an INLIER when fabs(r) <= threshold and, if min_cos > 0,
 * fabs(a * nx + b * ny + c * nz) >= min_cos (a normal of 0 0 0 fails).  With min_cos == 0 normals is not read.  A point with
 * active[i] == 0 is never an inlier.  threshold finite and >= 0, min_cos in [0, 1], min_cos > 0 only with normals, else PMN_ERR_ARG.
 *
 * pmn_plane_score: counts [n_planes] int32 (DEVICE; zeroed by the entry point, on the stream) = the number of inliers of every row of
 * planes, DEVICE float64 [n_planes][4]; a row with a non-finite entry scores 0.  1 <= n_planes <= PMN_PLANE_MAX_HYPOTHESES, else
 * PMN_ERR_SHAPE.  A lane holds four points in registers and walks 64 hypotheses, whose coefficients are scalar loads; a hypothesis's count
 * over a wave is the popcount of a ballot per point slot, lane h % 64 keeps the running count of hypothesis h over the tiles its
 * persistent wave takes and ends with one relaxed agent-scope int32 atomic add.  Integer sums of integers: counts does not depend on the
 * launch shape, on the waves' order or on the run.  Two launches (zero, score).
 *
 * pmn_plane_inliers: for ONE plane (plane_host = HOST double[4], finite) mask [n] uint8 (DEVICE, or NULL) = 1 for its inliers, and
 * sums [PMN_PLANE_SUMS] float64 (DEVICE) over its inliers with a = (x, y, z) - centre, each difference and each product rounded once
 * (centre_host = HOST double[3], finite): [0] their number, [1..3] the sum of a, [4..9] of ax * ax, ax * ay, ax * az, ay * ay, ay * az,
 * az * az.  The sums are EXACT up to one rounding, by pmn_icp_accumulate's digits (csrc/exact_sum.hpp): each term is scaled by a power of
 * two, cut into PMN_PLANE_LIMBS signed 32-bit digits, added in 64-bit integers (a lane's PMN_PLANE_BLOCK_POINTS / 64 points, the wave by
 * a butterfly, the workgroups by a second launch) and the total rounded to float64 once (to nearest, ties to even).  The powers of two
 * come from extent_host (HOST double[3], finite, >= 0) alone: the CALLER's bound of |(double)p_c - centre_c| over the active points, for
 * instance half the active bounding box around its centre; an inlier beyond it makes the sums meaningless (nothing is written out of
 * bounds).  So mask and sums are a function of the arguments alone, bit for bit -- not of the launch shape or the run -- and a term
 * loses only what lies below 2^-157 of its sum's bound.  scratch: DEVICE, PMN_PLANE_SCRATCH(n) 8-byte words (scratch_doubles states its
 * size, else PMN_ERR_ARG), contents undefined before and after.  PMN_ERR_SHAPE if a bound's exponent leaves +-800.  No atomics.  Two
 * launches. */
#define PMN_PLANE_MAX_HYPOTHESES 4096
#define PMN_PLANE_SUMS 10
#define PMN_PLANE_LIMBS 5
#define PMN_PLANE_BLOCK_POINTS 1024
#define PMN_PLANE_BLOCKS(n) (((long long)(n) + PMN_PLANE_BLOCK_POINTS - 1) / PMN_PLANE_BLOCK_POINTS)
#define PMN_PLANE_SCRATCH(n) (PMN_PLANE_BLOCKS(n) * PMN_PLANE_SUMS * PMN_PLANE_LIMBS)
int pmn_plane_score(const float *xyz, const float *normals, const unsigned char *active, long long n, const double *planes, int n_planes,
                    double threshold, double min_cos, int *counts, void *stream);
int pmn_plane_inliers(const float *xyz, const float *normals, const unsigned char *active, long long n, const double *plane_host,
                      double threshold, double min_cos, const double *centre_host, const double *extent_host, double *scratch,
                      long long scratch_doubles, unsigned char *mask, double *sums, void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  A signed distance from an ORIENTED point cloud, written into
 * the pool planes of the block-sparse volume above, which pmn_mt_count_blocks / pmn_mt_emit_blocks then mesh (pointcloud.cloud_sdf /
 * mesh_from_cloud, mesh_cloud.py; tests/cloud_sdf_ref.py is the numpy form; the reference has no counterpart).
 * The first six arguments are pmn_nn_distance's grid over the n_to points; normals (DEVICE float32 [n_to][3]) and colors (DEVICE uint8
 * [n_to][3], or NULL) are in the grid's SORTED order.  blocks, n_blocks, volume_dims_host, volume_origin_host, voxel, trunc and the
 * pool planes tsdf, weight, rgb, cweight are pmn_tsdf_integrate_blocks'; rgb and cweight are given exactly when colors is.
 * 1 <= k <= 32; radius, boundary, radius * radius and boundary * boundary positive and finite, else PMN_ERR_ARG.
 *
 * Per sample (i, j, k) of a listed block, everything float64, IEEE, without contraction, from float32 data widened to float64:
 * Position: x_c = origin_c + (float)index_c * voxel in FLOAT32, as pmn_tsdf_integrate forms it, then widened.  A sample of a border
 * block with an index >= n on some axis is outside the lattice and is not written.
 * Neighbourhood: pmn_knn_distance's list for the query x with max_dist = radius: the k nearest points with d2 < R2 = radius * radius
 * strictly, ascending (d2, sorted index); the sample is a position, never a point, so nothing is excluded.  c = the slots that hold a
 * point, j = 0 .. c - 1 their rank.
 * Weights: u = 1 - d2_j / R2, u2 = u * u, w_j = u2 * u2 (no exponential: the host model is exact).
 * Distance: s_j = (n.x * (x.x - p.x) + n.y * (x.y - p.y)) + n.z * (x.z - p.z);  W = sum_j w_j, S = sum_j w_j * s_j, both started at 0 and
 * added in rank order;  f = S / W.
 * Open boundaries (Hoppe's rule): t2 = d2_0 - s_0 * s_0 for the nearest neighbour j = 0, the squared distance along its tangent plane.
 * The sample is UNOBSERVED when c = 0, when t2 > boundary * boundary, or when W is not above 0 (every neighbour so close to the radius
 * that its weight rounded to 0: f would be 0 / 0).
 * Outputs: unobserved: tsdf = 1, weight = 0, rgb = 0, cweight = 0.  Observed: tsdf = (float)fmin(1, fmax(-1, f / (double)trunc)),
 * weight = (float)c -- pmn_mt_count_blocks' min_weight then reads "at least this many neighbours" -- and with colours
 * rgb_ch = (float)((sum_j w_j * colour_j,ch) / W), the sum in rank order, cweight = (float)c.
 * Sign: the volume's own: positive on the side the normals point to, so the extracted normals and winding face that side.
 * Every sample of every listed block inside the lattice is written, by plain stores.  One launch of 8 * n_blocks one-wave workgroups
 * (a wave per 8 x 8 layer of a block, a lane per sample), kernels specialised on the list's capacity (8, 16, 32); no atomics, the
 * lists are never written. */
int pmn_cloud_sdf_blocks(const float *to_xyz, const long long *to_keys, long long n_to, const double *origin_host, double cell,
                         const int *dims_host, const float *normals, const unsigned char *colors, const int *blocks, int n_blocks,
                         const int *volume_dims_host, const float *volume_origin_host, float voxel, float trunc, int k, double radius,
                         double boundary, float *tsdf, float *weight, float *rgb, float *cweight, void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  Moving least squares on a point cloud: every query is
 * projected onto a plane (degree 1) or a quadric (degree 2) fitted to its neighbourhood, which takes the noise along the viewing rays
 * out of a fused cloud (pointcloud.knn_mls / smooth_mls, smooth_cloud.py; tests/mls_ref.py is the numpy form; PCL's
 * MovingLeastSquares is the filter meant, the reference has no counterpart).  The grid, query, order, n_from, k and same_cloud are
 * pmn_knn_distance's, and so is the search with max_dist = radius.  radius and radius * radius positive and finite, degree 1 or 2,
 * line_ratio finite and >= 0, position not NULL, else PMN_ERR_ARG.  Everything below is float64, IEEE, without contraction, from the
 * float32 coordinates widened to float64; sums of three products are (x + y) + z.
 *
 * Neighbourhood: the slots of pmn_knn_distance's list that hold a point: the k nearest with d2 < R2 = radius * radius strictly, in rank
 * order j = 0 .. c - 1 (ascending (d2, sorted index)); count = c.  Under same_cloud the query's own index is not in the list, and the
 * query is a MEMBER of the fit: the delta 0 with weight 1, before rank 0.  Otherwise the query is a position and no member.  m = the
 * number of members, c + 1 or c.
 * Weights: u = 1 - d2_j / R2, u2 = u * u, w_j = u2 * u2 (pmn_cloud_sdf_blocks' weight; no exponential: the host model is exact).
 * Moments: d_j = p_j - q per axis.  W starts at 1 under same_cloud (the query's weight; its delta adds nothing to the other sums) and at
 * 0 otherwise; the other nine sums start at 0.  Per neighbour in rank order, with wd_a = w_j * d_ja:  W += w_j;  s_a += wd_a;
 * M_ab += wd_a * d_jb for ab = xx xy xz yy yz zz.  Centroid c_a = s_a / W.  Covariance A_ab = M_ab - (s_a * s_b) / W.
 * Frame: pmn_knn_normals' eigen-solver on A, unchanged: V = I, PMN_NORMAL_SWEEPS sweeps over (0, 1), (0, 2), (1, 2), a pair with
 * A_pq == 0 skipped, the ascending sort with equal values in column order.  (l0, n), (l1, e1), (l2, e2) are the eigenpairs; each of the
 * three vectors gets the canonical sign: its component of largest magnitude positive, the lowest axis among equal magnitudes.
 * Validity: m >= 3 and W > 0 and l2 != 0 and l1 > line_ratio * l2.  Otherwise status = 0, position = the query's float32 coordinates
 * as they are, normal = 0 0 0, displacement = 0.
 * Plane step (both degrees): t = (n.x * c.x + n.y * c.y) + n.z * c.z;  x0 = t * n per axis;  delta = x0, normal = n, status = 1.
 * Quadric step, only for degree == 2 and m >= PMN_MLS_QUADRIC_MIN: per member in the same order (the query first under same_cloud, with
 * r = 0 - x0 and w = 1), r = d_j - x0 per axis,  a = ((e1.x * r.x + e1.y * r.y) + e1.z * r.z) / radius,  b likewise with e2,
 * h = (n.x * r.x + n.y * r.y) + n.z * r.z,  phi = (1, a, b, a * a, a * b, b * b).  With wp_0 = w and wp_j = w * phi_j for j > 0:
 * g_j += wp_j * h, and G_ij += wp_j * phi_i for j <= i (21 sums, all started at 0).
 * Cholesky G = L L^T by columns j = 0 .. 5:  v = G_jj, then v = v - L_jk * L_jk for k = 0 .. j - 1;  the pivot v must be
 * > PMN_MLS_PIVOT_MIN * W;  L_jj = sqrt(v);  for i = j + 1 .. 5:  u = G_ij, then u = u - L_ik * L_jk for k = 0 .. j - 1;  L_ij = u / L_jj.
 * Forward, i = 0 .. 5:  v = g_i, then v = v - L_ik * y_k for k = 0 .. i - 1;  y_i = v / L_ii.  Back, i = 5 .. 0:  v = y_i, then
 * v = v - L_ki * c_k for k = i + 1 .. 5;  c_i = v / L_ii.
 * delta = x0 + c_0 * n per axis.  The step is taken when every pivot passed and (delta.x * delta.x + delta.y * delta.y) + delta.z *
 * delta.z <= R2; then status = 2 and the normal is u = (n - (c_1 / radius) * e1) - (c_2 / radius) * e2 per axis, divided by
 * sqrt((u.x * u.x + u.y * u.y) + u.z * u.z) (u . n = 1 before the division: the side of n is kept).  Otherwise the plane step stands:
 * status = 1.  (The plane step cannot leave the radius: |t| <= |c| < radius.)
 * Outputs, indexed as query, for status > 0: position_a = (float)(q_a + delta_a); normal_a = (float) of the component; displacement =
 * sqrt((delta.x * delta.x + delta.y * delta.y) + delta.z * delta.z).  position [n_from][3] float32; normal [n_from][3] float32 or NULL;
 * displacement [n_from] float64 or NULL; status [n_from] int32 or NULL; count [n_from] int32 or NULL.
 * PMN_MLS_PIVOT_MIN is a SETTING, not a measured optimum: with a and b scaled by 1 / radius the entries of G are of the order of W, a
 * pivot below 1e-10 W leaves fewer than six of float64's digits in the coefficients, and a fit that loose is not worth taking.
 * One launch of ceil(n_from / 64) one-wave workgroups, one lane per query, kernels specialised on the list's capacity (8, 16, 32) and
 * on the degree; the quadric's sums are a second pass over the list; no LDS, no atomics, the lists are never written. */
#define PMN_MLS_QUADRIC_MIN 6
#define PMN_MLS_PIVOT_MIN 1e-10
int pmn_knn_mls(const float *to_xyz, const long long *to_keys, long long n_to, const double *origin_host, double cell,
                const int *dims_host, const float *query, const int *order, long long n_from, int k, double radius, int same_cloud,
                int degree, double line_ratio, float *position, float *normal, double *displacement, int *status, int *count,
                void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  The exact distance from points to a triangle mesh
 * (patchmatchnet_amd/meshops.py build_face_grid / point_mesh_distance; tests/mesh_distance_ref.py is the numpy
 * form; the reference has no counterpart).  vertices, faces, n_vertices, n_faces and invalid as in the mesh entry points above: a face
 * with an index outside [0, n_vertices) is counted into *invalid by a launch of its own and belongs to no result.
 *
 * The first six arguments are pmn_nn_distance's grid, built over n_ref REFERENCE POINTS of the faces; entry_face [n_ref] (DEVICE int32,
 * in the grid's sorted order) names the face each of them belongs to (a value outside [0, n_faces) is skipped), and radius (finite,
 * >= 0) is a covering radius: the caller guarantees that every point of every face lies within `radius` of at least one of that face's
 * reference points as stored.  Under that guarantee the result is the minimum over ALL faces (the argument: csrc/meshops.hip); nothing
 * else about the reference points matters, a face may have any number of them.
 *
 * For each of the n_query points (query [n_query][3] float32, any finite position; order as pmn_nn_distance's, NULL = identity; 1 <=
 * n_query < 2^31 - 64), in float64 from the float32 coordinates, no contraction, IEEE division and sqrt, sums of three products left to
 * right in x, y, z order, with A, B, C the face's vertices in its order:
 *   segment(P, Q): e = Q - P, w = q - P, l2 = e.e, t = l2 > 0 ? (w.e) / l2 : 0 clamped to [0, 1], c = P + t * e, d2 = |q - c|^2;
 *   plane: e1 = B - A, e2 = C - A, n = e1 x e2, nn = n.n, w = q - A; only if nn > 0: u = ((e1 x w).n) / nn, v = ((w x e2).n) / nn; only
 *   if u >= 0, v >= 0, u + v <= 1: c = q - ((w.n) / nn) * n, d2 = (w.n)(w.n) / nn;
 *   the face's d2 = the least of segment(A, B), segment(B, C), segment(C, A), plane, in this order, the first among equals.
 * Faces (a, a, b), (a, a, a) and collinear faces are thereby segments or points.  Among faces with bit-equal d2 the lower face index
 * wins, so every output is a function of (mesh, query) alone, whatever the order of the faces, the reference points or the grid.
 *   dist [n_query] float64 = sqrt(d2) of the nearest face; a face counts only with d2 < max_dist * max_dist (max_dist and its square
 *   positive and finite), otherwise dist = max_dist itself (pmn_nn_distance's convention);
 *   face [n_query] int32, may be NULL: the index into faces, -1 at the cap;
 *   closest [n_query][3] float64, may be NULL: the point c of that face, NaN at the cap.
 * Two launches: a thread per face for *invalid, then ceil(n_query / 64) one-wave workgroups, one lane per query, no scratch memory. */
int pmn_mesh_distance(const float *ref_xyz, const long long *ref_keys, long long n_ref, const double *origin_host, double cell,
                      const int *dims_host, const int *entry_face, double radius, const float *vertices, int n_vertices,
                      const int *faces, int n_faces, const float *query, const int *order, long long n_query, double max_dist,
                      double *dist, int *face, double *closest, int *invalid, void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  Mesh simplification by vertex clustering
 * (patchmatchnet_amd/meshops.py simplify_clustering; tests/simplify_ref.py is the numpy form; the reference has
 * no counterpart).  The caller sorts the vertices into cubic cells of side `cell` whose lattice has its corner at origin_host (HOST
 * double[3]) and dims_host (HOST int[3], each 1 .. 2^30) cells; a CLUSTER is an occupied cell, clusters are numbered 0 .. n_clusters - 1
 * in ascending order of the key (z * dims[1] + y) * dims[0] + x, cluster [n_vertices] int32 names every vertex's, and every cluster's
 * mean position comes from pmn_voxel_mean.  vertices, faces, n_vertices and invalid as in the mesh entry points above; n_faces is
 * 1 .. PMN_MESH_SIMPLIFY_MAX_FACES (3 * n_faces fits an int32), else PMN_ERR_SHAPE.  No floating-point atomics, no LDS, no lane waits
 * for another lane: every output is a function of the mesh and the parameters alone, whatever the launch shape or the run.
 *
 * pmn_mesh_remap_faces, a thread per face (a, b, c): corner_cluster [n_faces][3] int32 = (cluster[a], cluster[b], cluster[c]) in the
 * face's own order; flag [n_faces] uint8 = 1 if two of the three agree (out_faces [n_faces][3] int32 is then that triple), else 0 and
 * out_faces = the triple ROTATED so that its smallest entry comes first, which keeps the orientation.  A face with an index outside
 * [0, n_vertices) adds 1 to *invalid and gets flag 2, out_faces (-1, -1, -1) and corner_cluster (n_clusters, n_clusters, n_clusters);
 * nothing is read through it.  One launch; the int32 counter is the feature's only atomic.
 *
 * pmn_mesh_cluster_place, a lane per cluster r: out [n_clusters][3] float32, the cluster's representative.  corners [3 * n_faces] int32
 * holds the entries 3 * f + c of all face corners, STABLY sorted by corner_cluster (entries of invalid faces last), and corner_starts
 * [n_clusters + 1] int64 the first position of every cluster's run, so a run is in ascending (face, corner) order; cluster_keys
 * [n_clusters] int64 the clusters' keys; mean [n_clusters][3] float32.  Float64, products and sums in the written order, no
 * contraction, IEEE division and sqrt, everything RELATIVE TO THE CELL'S CENTRE ctr_k = origin_k + ((double)cell_k + 0.5) * cell:
 *   per run entry, f = entry / 3 with vertices A, B, C in the face's order:  a = (double)A - ctr (b, c likewise);  e1 = b - a, e2 = c - a;
 *   n = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x);  w = sqrt((n.x n.x + n.y n.y) + n.z n.z); nothing if w is
 *   zero or not finite;  h = n / w;  q = (h.x a.x + h.y a.y) + h.z a.z;  g = w * h;
 *   Sxx += g.x h.x, Sxy += g.x h.y, Sxz += g.x h.z, Syy += g.y h.y, Syz += g.y h.z, Szz += g.z h.z;  t += q * g;  W += w.
 * A face with two or three corners in the cluster is in the run once per corner and contributes that often.  A run of at most
 * PMN_MESH_PLACE_LONG_RUN entries is summed by one lane in run order from 0.0; a longer run by a wave: lane l adds the entries l,
 * l + 64, ... in run order to 0.0 and the 64 values meet in pmn_voxel_mean's butterfly (x_l += x_(l ^ 32), then 16, 8, 4, 2, 1).
 *   lambda = stiffness * W (stiffness finite, > 0), mt = (double)mean - ctr;  (S + lambda I) x = t + lambda mt  by LDL^T:
 *   d0 = Sxx + lambda;  l10 = Sxy / d0;  l20 = Sxz / d0;  d1 = (Syy + lambda) - l10 * Sxy;  u = Syz - l10 * Sxz;  l21 = u / d1;
 *   d2 = ((Szz + lambda) - l20 * Sxz) - l21 * u;  y0 = t.x + lambda * mt.x;  y1 = (t.y + lambda * mt.y) - l10 * y0;
 *   y2 = ((t.z + lambda * mt.z) - l20 * y0) - l21 * y1;  x.z = y2 / d2;  x.y = y1 / d1 - l21 * x.z;  x.x = (y0 / d0 - l10 * x.y) - l20 * x.z.
 * S is positive semi-definite with trace W, so the condition number of S + lambda I is at most (1 + stiffness) / stiffness.  W zero
 * or not finite gives x = mt.  x is clamped per component to [-cell / 2, cell / 2] and out = (float)(ctr + x), one rounding.  Every
 * vertex of the cluster lies in the same cell, hence within sqrt(3) * cell of out.  One launch, no scratch memory. */
#define PMN_MESH_PLACE_LONG_RUN 256
#define PMN_MESH_SIMPLIFY_MAX_FACES 715827882
int pmn_mesh_remap_faces(const int *faces, int n_faces, int n_vertices, const int *cluster, int n_clusters, int *corner_cluster,
                         int *out_faces, unsigned char *flag, int *invalid, void *stream);
int pmn_mesh_cluster_place(const float *vertices, int n_vertices, const int *faces, int n_faces, const int *corners,
                           const long long *corner_starts, const long long *cluster_keys, int n_clusters, const float *mean,
                           const double *origin_host, double cell, const int *dims_host, double stiffness, float *out, void *stream);

/* Added under ABI 25 (purely additive: the version number did not move).  Mesh smoothing by umbrella steps and vertex normals from the
 * faces (patchmatchnet_amd/meshops.py smooth_taubin / smooth_laplacian / vertex_normals; tests/smooth_ref.py is
 * the numpy form; the reference has no counterpart).  No floating-point atomics, no LDS, no lane waits for another lane: every output
 * is a function of the mesh and the parameters alone, whatever the launch shape or the run.  Float64 from the float32 coordinates,
 * products and sums in the written order, no contraction, IEEE division and sqrt.
 *
 * THE ROW RULE of both entry points.  A row (a run of a CSR structure) of at most PMN_MESH_SMOOTH_LONG_ROW entries is summed by one
 * lane in row order from 0.0; a longer row by a wave: lane l adds the entries l, l + 64, ... in row order to 0.0 and the 64 values
 * meet in pmn_voxel_mean's butterfly (x_l += x_(l ^ 32), then 16, 8, 4, 2, 1) -- the rule of pmn_mesh_cluster_place.
 *
 * pmn_mesh_smooth: n_steps umbrella steps over xyz [n_vertices][3] float32 (1 <= n_vertices <= 2^31 - 256, else PMN_ERR_SHAPE).
 * starts [n_vertices + 1] int64 and neighbours [n_entries] int32 are the vertex adjacency in CSR form (row i = the neighbours of
 * vertex i; n_entries >= 0, neighbours may be NULL only then); pinned [n_vertices] uint8 or NULL; factors_host: HOST double
 * [n_steps], each finite (else PMN_ERR_ARG), 0 <= n_steps <= PMN_MESH_SMOOTH_MAX_STEPS.  Taubin's filter is lambda, mu, lambda, mu,
 * ...; the plain Laplacian lambda, lambda, ....  One step, for vertex i with row r of d entries (starts clamped to [0, n_entries], a
 * start beyond its end is an empty row), reading p and writing p':
 *   d == 0 or pinned[i] != 0:  p'_i = p_i, bit for bit;
 *   otherwise per component:   s = the row rule's sum over j in r of ((double)p_j - (double)p_i);  p'_i = (float)((double)p_i +
 *   factor * (s / (double)d)):  the division, the product and the sum are rounded once each in float64, then one rounding to float32.
 * The differences are taken relative to the vertex itself, so a scene at coordinates of 10^4 keeps them.  The CSR is not trusted: an
 * entry outside [0, n_vertices) adds nothing to s (d stays the row's length) and, in the FIRST step only, 1 to *invalid (int32, zeroed
 * by the caller), so *invalid is the number of such entries when n_steps >= 1.
 * Steps ping-pong between out and scratch (each [n_vertices][3] float32) so that the last step writes out: step k (from 0) writes out
 * when n_steps - 1 - k is even, step 0 reads xyz, xyz is never written.  n_steps = 0 copies xyz to out.  scratch may be NULL when
 * n_steps <= 1.  out or scratch overlapping xyz or each other: PMN_ERR_ARG.  Every argument check returns before any launch.
 * max(n_steps, 1) launches of ceil(n_vertices / 256) workgroups, a lane per vertex, no scratch memory.
 *
 * pmn_mesh_vertex_normals: out [n_vertices][3] float32, the area-weighted normal of every vertex.  faces [n_faces][3] int32 (1 ..
 * PMN_MESH_SIMPLIFY_MAX_FACES, else PMN_ERR_SHAPE); corners [3 * n_faces] int32 holds the entries 3 * f + c of the face corners STABLY
 * sorted by the vertex they name, and corner_starts [n_vertices + 1] int64 the first position of every vertex's run, so a run is in
 * ascending (face, corner) order of the faces AS HANDED IN (meshops.vertex_normals hands them in _canonical_face_order, so that the
 * order of the caller's faces changes no bit).  For vertex i, with A, B, C the vertices of face f = entry / 3 in the face's stored
 * order:  e1 = (double)B - (double)A, e2 = (double)C - (double)A;  n += (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y -
 * e1.y e2.x) by the row rule (the cross product carries the area weight);  length = sqrt((n.x n.x + n.y n.y) + n.z n.z);
 * out_i = (float)(n / length), or zero when length is zero or not finite; flip != 0 negates the result (exactly).  The normal
 * follows the right-hand rule of the stored winding.  An entry outside [0, 3 * n_faces) or a face with an index outside [0,
 * n_vertices) adds nothing; such faces are counted into *invalid by a launch of their own.  Two launches, no scratch memory. */
#define PMN_MESH_SMOOTH_LONG_ROW 256
#define PMN_MESH_SMOOTH_MAX_STEPS 65536
int pmn_mesh_smooth(const float *xyz, int n_vertices, const long long *starts, const int *neighbours, long long n_entries,
                    const unsigned char *pinned, const double *factors_host, int n_steps, float *out, float *scratch, int *invalid,
                    void *stream);
int pmn_mesh_vertex_normals(const float *vertices, int n_vertices, const int *faces, int n_faces, const int *corners,
                            const long long *corner_starts, int flip, float *out, int *invalid, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PMN_HIP_H */
