/*
 * xfeat_hip.h -- C ABI of libxfeat_hip.so: the XFeat inference hot path on MI355X (gfx950).
 *
 * The reference (verlab/accelerated_features) is pure Python on PyTorch and has NO native
 * boundary; its drop-in boundary is the Python class modules/xfeat.py::XFeat.  This header
 * is the native boundary that class is re-hosted on: one entry point per block of ATen work
 * the reference's methods execute.  Each declaration cites the reference code it replaces.
 * A host in any language binds these symbols (ctypes stub: accelerated_features_amd/_lib.py,
 * other hosts: INTEGRATION.md).
 *
 * Conventions
 *   - Plain C types only.  All tensor pointers are DEVICE pointers (HBM) unless the name
 *     starts with host_.  Layouts are dense, row-major in the index order written.
 *   - The library never allocates in the hot path: the caller provides a workspace of
 *     xfh_*_workspace_bytes() bytes (256-byte aligned).  Only xfh_create allocates (weights).
 *   - Workspace and outputs need no initialisation -- every word a call reads from them it has written first, and every byte of an
 *     output is determined by the call's inputs unless its entry says otherwise -- and nothing outside them is written
 *     (tests/test_gpu_buffers.py holds every entry to this between guard bands, at exactly the named workspace size).
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream).  No hidden synchronisation.  Process-wide state is limited to: the
 *     thread-local error string and per-device "kernel attribute set" flags (idempotent).  The library reads
 *     no environment variables; kernel-variant switches are per handle (xfh_set_option), and so are the
 *     debugging hooks xfh_debug_trace / xfh_profile_select (not for concurrent use on one handle).
 *   - Return value: XFH_OK (0) or a negative XFH_ERR_* code; xfh_last_error() gives a
 *     message for the calling thread.  No C++ exception crosses the boundary.
 *   - A handle's weights are immutable after xfh_create and it may be shared by threads/streams,
 *     provided each concurrent call uses its own workspace (the profiling hooks above write
 *     into the handle: switch them off for concurrent use).
 *   - Ragged results use fixed capacity + device-side counts: the host reads the counts back
 *     once per batch (the reference synchronises B times per batch: xfeat.py:254-261,99-103).
 */
#ifndef XFEAT_HIP_H
#define XFEAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XFH_VERSION 303          /* major*10000 + minor*100 + patch */

enum {
    XFH_OK = 0,
    XFH_ERR_ARG = -1,            /* bad shape / null pointer / unsupported size          */
    XFH_ERR_WEIGHTS = -2,        /* weight table malformed                               */
    XFH_ERR_WORKSPACE = -3,      /* workspace too small or misaligned                    */
    XFH_ERR_UNSUPPORTED = -4,    /* valid request outside what this build implements     */
    XFH_ERR_HIP = -5,            /* a HIP runtime call failed (message has the hipError) */
    XFH_ERR_DEVICE = -6          /* not a gfx950 device / no device                      */
};

typedef struct xfh_context* xfh_handle;
typedef void* xfh_stream;        /* hipStream_t */

int xfh_version(void);
const char* xfh_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Weights.  Replaces XFeat.__init__ / net.load_state_dict (modules/xfeat.py:23-35) and the
 * parameter containers of XFeatModel (modules/model.py:33-111).
 *
 * host_arrays: HOST pointers to the fp32 arrays of a reference state_dict in the canonical
 * order below (n_arrays must equal xfh_num_weight_arrays()).  Eval-mode BatchNorm
 * (affine=False, eps 1e-5) is folded into the preceding conv / linear at create time.
 *
 *   for each conv in execution order (accelerated_features_amd/spec.py::CONVS):
 *       BasicLayer : <name>.layer.0.weight (Cout,Cin,k,k), .layer.1.running_mean, .layer.1.running_var
 *       plain conv : <name>.weight (Cout,Cin,k,k), <name>.bias
 *   then fine_matcher: for L in 0,3,6,9: L.weight (out,in), L.bias, (L+1).running_mean, (L+1).running_var
 *                      then 12.weight, 12.bias
 * ---------------------------------------------------------------------------------------- */
int xfh_num_weight_arrays(void);
/* number of floats the i-th array must hold (for host-side validation) */
size_t xfh_weight_array_floats(int i);
int xfh_create(const float* const* host_arrays, int n_arrays, int device, xfh_handle* out);
void xfh_destroy(xfh_handle h);

/* ------------------------------------------------------------------------------------------
 * Bilinear resize, align_corners=False, NCHW planes.  Replaces F.interpolate in
 * preprocess_tensor (modules/xfeat.py:239, size given => scale = in/out) and in
 * extract_dualscale (modules/xfeat.py:380-381, scale_factor given => scale = 1/scale_factor).
 * src (planes,Hin,Win) -> dst (planes,Hout,Wout); scale_h/scale_w are the source-per-
 * destination steps PyTorch would use.
 * ---------------------------------------------------------------------------------------- */
int xfh_resize_bilinear(const float* src, int planes, int Hin, int Win, float* dst, int Hout, int Wout,
                        float scale_h, float scale_w, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Kernel switches of ONE handle.  Every layer has ONE default kernel and ONE fallback with fp32's range; the options choose between them (and two
 * test switches).  Results of either choice satisfy the same parity contract; the defaults are the shipped path.  Not for concurrent use with calls
 * on the same handle.
 *   "fx"            bitmask of XFH_FX_*, DEFAULT XFH_FX_ALL.  A set bit runs that layer family in the fp16-pair arithmetic on the fp16 matrix cores
 *                           (x = xh + 2^-11 xl, three fp16 MFMAs per product, fp32 accumulation: fp32-equivalent results for |x| < 65504, |w| < 31);
 *                           a cleared bit runs it on the f32 matrix cores (v_mfma_f32_32x32x2_f32: fp32's range).  A layer with a weight beyond the pair's range
 *                           runs on the f32 kernel whatever the bit says.
 *                             XFH_FX_CONV64 (1)    the 64- and 128-channel 3x3 convolutions: conv_rs64_kernel (weights resident in registers; block3.1 + .2, block4.1,
 *                                                  block4.2, block5.1, block5.2, block_fusion.0, block_fusion.1 + .2) and conv_bx64s2x_kernel (stride 2: block4.0, block5.0)
 *                             XFH_FX_CONV24 (2)    the 24-channel 3x3 convolutions (block2.0, block2.1, block3.0): conv_bx_kernel, conv_bxs2_kernel
 *                             XFH_FX_HEADS (8)     keypoint_head and heatmap_head: head_bx_kernel   (cleared: head_f32r_kernel)
 *                             XFH_FX_FINE (2048)   the fine_matcher's five linear layers (xfh_refine_matches, xfh_fine_matcher) as one chain: linear_fx_kernel (first / last
 *                                                  layer) and linear_fxd_kernel (the 512 -> 512 layers, LDS-DMA), the activations between them as fp16 pairs in the workspace
 *                                                  (csrc/linear_fx_body.hpp)   (cleared: linear_mfma_kernel)
 *                           Every other bit is rejected.
 *   "block1"        5 | 7   DEFAULT 7: block1.2 (8 -> 8) and block1.3 (8 -> 24, stride 2) on the fp16 matrix cores in the fp16-pair arithmetic (block1_mx_kernel);
 *                           5: every layer of block1 on the vector ALUs (block1_fused_kernel: fp32's range).  Both recompute conv1 inside conv2 (no c1 tile in LDS).
 *   "match_exact"   0 | 1   1: xfh_match_mnn computes every similarity on the f32 matrix cores (no fp16 filter): the kernel the default is tested against
 *   "match_sweep"   0..2    DEFAULT 0: the filter's pass over the fp16 product multiplies every 32 x 32 tile ONCE (mnn_f16_sweep2_kernel: column-direction block maxima over
 *                           the rows that meet in a lane) when P, N1, N2 give it enough wave tasks to fill the chip, else in both orientations (mnn_f16_sweep_kernel: finer
 *                           work split); 1 / 2: always the two- / one-orientation form.  The same matches in every case: decisions are taken on exact fp32 dot products.
 *   "resize2"       0 | 1   DEFAULT 1.  The fused two-stage resize of the dual-scale dense path (xfh_backbone_resized): 1 = the tile's input region staged in LDS by
 *                           16-byte loads (needs Win % 4 == 0; otherwise, and with 0: four-byte gathers per tap).  Same bits either way.
 * THE RANGE FALLBACK: on XFH_STATUS_FX_RANGE (below) repeat the call with fx = 0 and block1 = 5 -- every kernel then has fp32's range and none converts to fp16,
 * so the status bit cannot be set again.
 * Every kernel choice the options leave open is made by the IMAGE's size, never by the batch size: an image's results do not depend on the batch it travels in.
 * xfh_set_option returns XFH_ERR_ARG for an unknown key or value; xfh_get_option writes the current value.
 * ---------------------------------------------------------------------------------------- */
enum { XFH_FX_CONV64 = 1, XFH_FX_CONV24 = 2, XFH_FX_HEADS = 8, XFH_FX_FINE = 2048, XFH_FX_ALL = 1 | 2 | 8 | 2048 };
int xfh_set_option(xfh_handle h, const char* key, int value);
int xfh_get_option(xfh_handle h, const char* key, int* value);
/* Status word of a handle's calls: a caller-owned DEVICE int32 (NULL = none) into which kernels OR status bits; the caller zeroes and reads it (e.g. with
 * the read-back of the key-point counts).  XFH_STATUS_FX_RANGE: a convolution in the fp16-pair arithmetic (option "fx") met an activation of magnitude
 * >= 65504, which the fp16 high part cannot hold -- the outputs of that call are not valid; repeat it with fx = 0 and block1 = 5 (the f32-MFMA / vector-ALU kernels have fp32's range).
 * Set by xfh_backbone*, xfh_conv_layer, xfh_debug_block1, xfh_refine_matches, xfh_fine_matcher.  The pointer is read at launch time; it may be changed between calls. */
enum { XFH_STATUS_FX_RANGE = 1 };
int xfh_set_status_buffer(xfh_handle h, int32_t* device_word);

/* ------------------------------------------------------------------------------------------
 * Backbone.  Replaces XFeatModel.forward (modules/model.py:123-154) plus
 * XFeat.get_kpts_heatmap (modules/xfeat.py:242-247).
 *
 *   img      (B,C,H,W) fp32, H%32==0, W%32==0, C>=1; finite values.  A NaN or Inf pixel is NOT propagated the way F.relu / torch.max propagate it in the
 *            reference: block1's ReLU is a v_med3_f32 (k_conv_direct.hip is compiled with -fno-honor-nans, as is the matcher's maximum search), so a non-finite
 *            input gives unspecified finite-or-not values in that image (other images of the batch are unaffected).  Validate on the host if the source can produce them.
 *   feats    (B,H/8,W/8,64)  "M1", channels-last (a (B,64,h,w) tensor in channels_last memory format)
 *   logits   (B,H/8,W/8,65)  "K1", channels-last; may be NULL (then not written)
 *   heat     (B,H,W)         softmax(K1)[:64] depth-to-space 8x8; may be NULL (then logits must not be)
 *   reliab   (B,H/8,W/8)     "H1" after the sigmoid
 *   invnorm  (B,H/8,W/8)     optional (may be NULL): 1 / max(||feats[b,i,j,:]||, 1e-12), the per-cell factor of F.normalize(M1, dim=1)
 *                            (modules/xfeat.py:70) -- a by-product of the reliability head; hand it to xfh_detect_sparse to save that pass
 * ---------------------------------------------------------------------------------------- */
size_t xfh_backbone_workspace_bytes(int B, int C, int H, int W);
int xfh_backbone(xfh_handle h, const float* img, int B, int C, int H, int W,
                 float* feats, float* logits, float* heat, float* reliab, float* invnorm,
                 void* workspace, size_t workspace_bytes, xfh_stream stream);

/* Same network from uint8 pixels: replaces the host-side conversion in front of it --
 * XFeat.parse_input's `torch.tensor(x).permute(0,3,1,2) / 255` for numpy images (modules/xfeat.py:396-403, divisor 255,
 * layout XFH_LAYOUT_NHWC) and preprocess_tensor's `x.float()` for uint8 tensors (modules/xfeat.py:232, divisor 1,
 * layout XFH_LAYOUT_NCHW).  Per channel v = float(u8) / divisor; results are bit-identical to converting first. */
#define XFH_LAYOUT_NCHW 0
#define XFH_LAYOUT_NHWC 1
int xfh_backbone_u8(xfh_handle h, const uint8_t* img, int layout, float divisor, int B, int C, int H, int W,
                    float* feats, float* logits, float* heat, float* reliab, float* invnorm,
                    void* workspace, size_t workspace_bytes, xfh_stream stream);

/* The dual-scale dense path (XFeat.extract_dualscale, modules/xfeat.py:379-394): F.interpolate(x, scale_factor=s) to
 * (Hmid,Wmid), then preprocess_tensor's resize to multiples of 32 (modules/xfeat.py:234-238) to (Hout,Wout), then the
 * network.  Identical to xfh_resize_bilinear(img -> mid, scale1) + xfh_resize_bilinear(mid -> out, scale2) +
 * xfh_backbone(out) -- the gray plane the network consumes is bit-identical -- without writing either resized image.
 * img: (B,C,Hin,Win) fp32; workspace: xfh_backbone_workspace_bytes(B, C, Hout, Wout).  scale2 must be < 2
 * (XFH_ERR_UNSUPPORTED otherwise: materialise the images with xfh_resize_bilinear). */
int xfh_backbone_resized(xfh_handle h, const float* img, int B, int C, int Hin, int Win, int Hmid, int Wmid,
                         float scale1_h, float scale1_w, int Hout, int Wout, float scale2_h, float scale2_w,
                         float* feats, float* logits, float* heat, float* reliab, float* invnorm, void* workspace,
                         size_t workspace_bytes, xfh_stream stream);

/* One conv layer of the network in isolation (parity tests against per-layer oracle
 * activations).  layer = index into spec.CONVS; in (B,Cin,Hin,Win) NCHW, out (B,Cout,Hout,Wout)
 * NCHW with the layer's own stride/padding, folded BN and ReLU where the reference has them.
 * variant: XFH_CONV_VARIANT_*.  DEFAULT = the kernel the backbone uses for this layer under the handle's options; GENERIC = a plain direct convolution on the
 * vector ALUs (any layer: the independent device-side check); FX = the layer's fp16-pair kernel and F32 = its f32-MFMA kernel, each without fallback
 * (XFH_ERR_UNSUPPORTED where the layer has none); FX_PAIR / FX_PAIR_NHWC = this 3x3 layer AND the 1x1 layer behind it in one launch of conv_rs64_kernel
 * (layers block3.1, block_fusion.1: out = the 1x1's output, NCHW / channels-last). */
enum { XFH_CONV_VARIANT_DEFAULT = 0, XFH_CONV_VARIANT_GENERIC = 1, XFH_CONV_VARIANT_FX = 2, XFH_CONV_VARIANT_F32 = 3, XFH_CONV_VARIANT_FX_PAIR = 4, XFH_CONV_VARIANT_FX_PAIR_NHWC = 5 };
int xfh_conv_layer(xfh_handle h, int layer, const float* in, int B, int Hin, int Win, float* out,
                   int variant, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Sparse detection.  Replaces XFeat.NMS (modules/xfeat.py:249-263), the score / top-k /
 * descriptor block of detectAndCompute (modules/xfeat.py:70-103) and the three
 * InterpolateSparse2d calls (modules/interpolator.py:21-33).
 *
 *   heat (B,H,W), reliab (B,H/8,W/8), feats (B,H/8,W/8,64) as produced by xfh_backbone
 *   invnorm          (B,H/8,W/8) from the same xfh_backbone call, or NULL (then computed here in one extra pass over feats)
 *   threshold        detection threshold (strict >).  May be negative: a pixel outside the image never takes part in a
 *                    window's maximum (-inf padding), whatever the sign of the values.
 *   top_k            any positive value (fewer candidates than top_k => shorter lists, like the reference)
 *   nms_capacity     capacity of the candidate list per image.  If n_candidates[b] comes back
 *                    larger, candidates were dropped in row-major order: re-run with a
 *                    capacity >= max(n_candidates) (H*W is always enough).
 *   rw, rh           original/processed size ratios (key-points are returned multiplied by them)
 * outputs (fixed capacity, entries past n_valid[b] are zero-filled):
 *   kpts (B,top_k,2) fp32 (x,y) ; scores (B,top_k) descending, EQUAL scores in candidate order (row-major: y, then x,
 *   among the first nms_capacity candidates) ; desc (B,top_k,64) unit norm (a zero row where every feature under the
 *   key-point's sixteen taps is zero)
 *   desc_f16 (B,top_k,64) optional (may be NULL): fp16 (round-to-nearest-even) of 256 * desc, the operand of xfh_match_mnn's filter sweep
 *   n_valid (B) int32       = number of returned points with score > 0 (they form a prefix)
 *   n_candidates (B) int32  = NMS candidates found (uncapped)
 * ---------------------------------------------------------------------------------------- */
size_t xfh_detect_workspace_bytes(int B, int H, int W, int top_k, int nms_capacity);
int xfh_detect_sparse(xfh_handle h, const float* heat, const float* reliab, const float* feats, const float* invnorm,
                      int B, int H, int W, float threshold, int top_k, int nms_capacity, float rw, float rh,
                      float* kpts, float* scores, float* desc, uint16_t* desc_f16, int32_t* n_valid, int32_t* n_candidates,
                      void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Semi-dense extraction.  Replaces XFeat.extractDense after the backbone
 * (modules/xfeat.py:362-375): top-k of the reliability map (descending), RAW 64-D features of
 * those cells and their corner coordinates (8*(j,i)*(rw,rh)) / scale_div (scale_div = s of
 * extract_dualscale, modules/xfeat.py:388; 1 otherwise).  Cells of EQUAL reliability come out lower cell index
 * (i*w + j) first.  (Both tie rules hold for values without NaN; -0.0 and +0.0 are not promised to tie.)
 *   kpts (B,k,2), desc (B,k,64), cell_index (B,k) int32 (may be NULL); k <= h*w
 * ---------------------------------------------------------------------------------------- */
size_t xfh_dense_workspace_bytes(int B, int h, int w, int k);
int xfh_extract_dense(xfh_handle h, const float* reliab, const float* feats, int B, int hc, int wc, int k,
                      float rw, float rh, float scale_div, float* kpts, float* desc, int32_t* cell_index,
                      void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Mutual nearest neighbour matching.  Replaces XFeat.match (modules/xfeat.py:327-348) and
 * XFeat.batch_match (modules/xfeat.py:265-290) for P independent pairs.
 *
 *   pair p uses d1 + p*pair_stride1 (N1 x 64, row-major) and d2 + p*pair_stride2 (N2 x 64)
 *   n1/n2: DEVICE int32 arrays; pair p uses n1[p*n_stride] rows and n2[p*n_stride+n_offset2]
 *          rows (so the n_valid array of xfh_detect_sparse can be passed for consecutive
 *          frame pairs with n_stride=2, n_offset2=1).  NULL => all N1 / N2 rows.
 *   d1_f16/d2_f16: optional (both or neither): fp16 round-to-nearest-even copies of 256 * d1 / 256 * d2 with the same pair strides (in elements,
 *          multiples of 8), valid ONLY for L2-normalised rows (|row| <= 1.00001) -- what xfh_detect_sparse's desc_f16 holds.  They spare the call its
 *          two conversion passes; every decision is still taken on exact fp32 dot products of d1 / d2 (results identical with or without them).
 *   The fp16 product only selects which 32-wide blocks of a row / column can hold its arg-max (window derived in k_match_f16.hip); the arg-max
 *   itself, ties included, comes from fp32 dot products of d1 / d2 in a fixed summation order.
 *   min_cossim <= 0 disables the similarity test (reference: `if min_cossim > 0`).
 *   pair_stride1/2 are in floats.
 * outputs: idx0, idx1 (P,N1) int64 (idx0 ascending), n_matches (P) int32; the entries from n_matches[p] to N1 are written as -1.
 * Arg-max ties resolve to the lowest index, like torch.max / torch.argmax.
 * ---------------------------------------------------------------------------------------- */
size_t xfh_match_workspace_bytes(int P, int N1, int N2);
int xfh_match_mnn(xfh_handle h /* may be NULL */, const float* d1, size_t pair_stride1, const float* d2, size_t pair_stride2,
                  const uint16_t* d1_f16, const uint16_t* d2_f16,
                  const int32_t* n1, const int32_t* n2, int n_stride, int n_offset2,
                  int P, int N1, int N2, float min_cossim,
                  int64_t* idx0, int64_t* idx1, int32_t* n_matches,
                  void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Guided matching: mutual nearest neighbours among the candidates that agree with a known two-view model (a fundamental
 * matrix, an essential matrix brought to pixels, a homography) -- the arg-max of xfh_match_mnn taken again under the geometry
 * the estimators below found.  Element (i, j) takes part in row i's and in column j's arg-max only if key-point i of image 0
 * and key-point j of image 1 pass the gate; every similarity is an fp32 dot product on the f32 matrix cores (the exact kernel
 * of xfh_match_mnn, csrc/k_match.hip, with the gate in its epilogue: csrc/k_match_guided.hip, no fp16 filter).
 *
 *   d1/d2, pair strides, n1/n2, n_stride, n_offset2, min_cossim, idx0/idx1/n_matches: as for xfh_match_mnn
 *   kpts1/kpts2: (x,y) fp32 pixel coordinates of the rows of d1 / d2; pair p at kpts + p*kpt_stride (strides in floats)
 *   models: P x 9 fp64 row-major (device), one model M per pair; max_error: the gate's threshold thr in pixels
 *
 *   kind XFH_GUIDE_FUNDAMENTAL (model M with x1' M x0 = 0, the convention of xfh_find_fundamental; for E pass
 *   F = K1^-T E K0^-1): the Sampson error, the quantity xfh_find_fundamental thresholds, without its division.
 *   Element (i, j) passes iff
 *       e^2 <= thr^2 * (rho_i + gamma_j)
 *   with l = M (x0_i, 1), rho_i = l0^2 + l1^2, m = M' (x1_j, 1), gamma_j = m0^2 + m1^2, e = (l0 x1_j.x + l1 x1_j.y) + l2.
 *   The per-row constants (l, rho) and the per-column constant (gamma) are computed once in fp64 from the fp64 model (scaled
 *   by 1 / max |M_ab| first: the gate does not depend on the model's scale) and rounded to fp32, thr^2 folded into rho and
 *   gamma before the rounding; only e, the sum and the compare run per element, in fp32.
 *
 *   kind XFH_GUIDE_HOMOGRAPHY (forward transfer error, as cv2.findHomography thresholds it):
 *   (U,V) = dehom(H (x0_i, 1)), computed once per row in fp64 and rounded to fp32.  Element (i, j) passes iff
 *       (U - x1_j.x)^2 + (V - x1_j.y)^2 <= thr^2.
 *   A row whose homogeneous w is non-finite or |w| <= DBL_EPSILON * |row 3 of H| passes nothing.
 *
 *   A row or column without a passing element has no match.  An all-zero model (what the estimators write where nothing was
 *   found) and a model with a non-finite entry give no matches for their pair.  max_error <= 0 or non-finite: XFH_ERR_ARG.
 *   N2 <= 2^21 (XFH_ERR_UNSUPPORTED beyond).
 * outputs: idx0, idx1 (P,N1) int64 (idx0 ascending), n_matches (P) int32, the entries from n_matches[p] to N1 written as -1; ties resolve
 * to the lowest index.
 * ---------------------------------------------------------------------------------------- */
#define XFH_GUIDE_FUNDAMENTAL 0
#define XFH_GUIDE_HOMOGRAPHY  1
size_t xfh_match_guided_workspace_bytes(int P, int N1, int N2);
int xfh_match_mnn_guided(const float* d1, size_t pair_stride1, const float* d2, size_t pair_stride2,
                         const float* kpts1, size_t kpt_stride1, const float* kpts2, size_t kpt_stride2,   /* (x,y) fp32, strides in floats */
                         const int32_t* n1, const int32_t* n2, int n_stride, int n_offset2, int P, int N1, int N2,
                         const double* models /* P x 9 row-major, device */, int kind, double max_error, float min_cossim,
                         int64_t* idx0, int64_t* idx1, int32_t* n_matches, void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Match refinement.  Replaces XFeat.refine_matches (modules/xfeat.py:306-325),
 * XFeat.subpix_softmax2d (modules/xfeat.py:292-304) and XFeatModel.fine_matcher
 * (modules/model.py:97-111) for P pairs at once.
 *
 *   desc0/desc1 (P,N,64), kp0/kp1 (P,N,2), scale0 (P,N)  -- detectAndComputeDense outputs
 *   idx0/idx1 (P,N) int64 with n_matches (P) int32 (device) -- xfh_match_mnn outputs
 *   out (P,N,4) fp32 rows (x0,y0,x1,y1) of the matches with conf > fine_conf, order kept, the rows from n_out[p] to N written as
 *   zeros; n_out (P) int32.
 * ---------------------------------------------------------------------------------------- */
size_t xfh_refine_workspace_bytes(int P, int N);
int xfh_refine_matches(xfh_handle h, const float* desc0, const float* desc1, const float* kp0, const float* kp1,
                       const float* scale0, const int64_t* idx0, const int64_t* idx1, const int32_t* n_matches,
                       int P, int N, float fine_conf, float* out, int32_t* n_out,
                       void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Stand-alone helpers behind the reference's public helper methods.
 *   xfh_kpts_heatmap : XFeat.get_kpts_heatmap (modules/xfeat.py:242-247); logits (B,h,w,65)
 *                      channels-last -> heat (B,8h,8w).
 *   xfh_nms          : XFeat.NMS (modules/xfeat.py:249-263), any odd kernel_size (the reference's generic
 *                      max_pool2d(k, 1, k/2) window; 5 is what the hot path uses and has the tiled kernel).
 *                      xy (B,capacity,2) int64 (x,y) in row-major order, zero padded; n_candidates (B) int32
 *                      uncapped (beyond capacity the LAST candidates in row-major order are dropped).  The threshold
 *                      may be negative: windows are clipped to the image (-inf padding) for values of any sign.  workspace: xfh_detect_workspace_bytes(B,H,W,1,capacity).
 *   xfh_sample_sparse: InterpolateSparse2d.forward (modules/interpolator.py:10-33; the XFeat.interpolator attribute,
 *                      modules/xfeat.py:37): x (B,C,Hm,Wm) NCHW, pos (B,N,2) fp32 (x,y) in an H x W frame ->
 *                      out (B,N,C); grid_sample semantics (align_corners=False, zeros padding) with the reference's
 *                      fp32 coordinate arithmetic.  The hot path fuses its three sampling sites and does not call this.
 *   xfh_fine_matcher : XFeatModel.fine_matcher (modules/model.py:97-111): x (n,128) -> out (n,64).
 *                      workspace: xfh_refine_workspace_bytes(1, n).
 * ---------------------------------------------------------------------------------------- */
int xfh_kpts_heatmap(const float* logits, int B, int hc, int wc, float* heat, xfh_stream stream);
int xfh_nms(xfh_handle h, const float* heat, int B, int H, int W, float threshold, int kernel_size, int capacity, int64_t* xy,
            int32_t* n_candidates, void* workspace, size_t workspace_bytes, xfh_stream stream);
enum { XFH_SAMPLE_NEAREST = 0, XFH_SAMPLE_BILINEAR = 1, XFH_SAMPLE_BICUBIC = 2 };
int xfh_sample_sparse(const float* x, const float* pos, int B, int C, int Hm, int Wm, int N, int H, int W, int mode, float* out,
                      xfh_stream stream);
int xfh_fine_matcher(xfh_handle h, const float* x, int n, float* out, void* workspace, size_t workspace_bytes,
                     xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Robust homography from the matches -- the consumer of the demo:
 *     H, inliers = cv2.findHomography(points1, points2, cv2.USAC_MAGSAC, ransac_thr, maxIters=700, confidence=0.995)
 * (realtime_demo.py:225), for P pairs at once.  OpenCV (opencv-contrib-python-headless 4.10.0.84, requirements.txt:1) is not
 * part of the reference tree: the algorithm is the published one (RANSAC + MAGSAC++ quality and sigma-consensus++ weights,
 * Barath et al., CVPR 2020) as specified in DESIGN.md 3.7 / csrc/k_homography.hip -- same estimate, not OpenCV's random stream.
 *   pts0/pts1 (P,cap,2) fp32 pixel coordinates (device), pair p uses its first counts[p] rows (device int32; NULL: n_const
 *   for all).  All max_iters (<= 4096) hypotheses are scored on the device; the stopping rule (confidence) is then applied
 *   to the score list as the sequential loop would apply it, so the result is a function of the arguments and `seed` only.
 *   H (P,9) fp64 row-major with H[8] = 1 (zeros when nothing was found); mask (P,cap) uint8, 1 = forward transfer error
 *   < ransac_thr; info (P,8) int32: found, winning hypothesis, hypotheses the loop would have run, inliers, accepted
 *   refinement steps, n, quality (lo, hi word).  Fewer than 4 correspondences / inliers: found = 0 (cv2 returns None).
 *   xfh_find_homography_matches: the same on the matcher's output without materialising the point lists: correspondence i of
 *   pair p is (kpts0[p][idx0[p][i]], kpts1[p][idx1[p][i]]), kpts (P,kpt_cap,2) fp32, idx (P,cap) int64 and n_matches (P) int32 as
 *   xfh_match_mnn writes them (realtime_demo.py:209-211: points1 = kpts1[idx0], points2 = kpts2[idx1]).
 *   xfh_homography_tables: the 4096-entry quality (20-bit fixed point) / weight tables over r^2 in [0, (2 thr)^2).
 * ---------------------------------------------------------------------------------------- */
size_t xfh_homography_workspace_bytes(int P, int max_iters);
int xfh_find_homography(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap,
                        double ransac_thr, int max_iters, double confidence, uint64_t seed,
                        double* H, uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_find_homography_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                                const int32_t* n_matches, int P, int cap, double ransac_thr, int max_iters, double confidence, uint64_t seed,
                                double* H, uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_homography_tables(double ransac_thr, uint32_t* score_table, double* weight_table, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Relative pose from the matches -- the step the evaluation takes after matching:
 *     pose, info = poselib.estimate_relative_pose(kpts0, kpts1, cam0, cam1, {"max_epipolar_error": thr}, {})
 * (modules/eval/megadepth1500.py, scannet1500.py), for P pairs at once.  poselib is not part of the reference tree: the
 * algorithm is the published one (five-point essential RANSAC, Nister 2004, MSAC on the Sampson error, Gauss-Newton
 * refinement), specified in DESIGN.md 3.10 / csrc/k_relpose.hip -- same estimate, not poselib's random stream.
 *   pts0/pts1 (P,cap,2) fp32 pixel coordinates (device), pair p uses its first counts[p] rows (device int32; NULL: n_const
 *   for all); K0/K1 (P,3,3) fp64 PINHOLE intrinsics (device).  All max_iters (<= 16384; larger is an error) hypotheses are
 *   scored on the device, the stopping rule (min_iters, success_prob) applied to the cost list afterwards.
 *   R (P,9) fp64 row-major, t (P,3) fp64 unit norm, E = [t]x R (P,9); mask (P,cap) uint8, 1 = Sampson error below the
 *   threshold; info (P,8) int32: found, winning hypothesis, hypotheses the loop would have run, inliers, accepted refinement
 *   steps, n, cost (lo, hi word).  Fewer than 5 correspondences / inliers: found = 0 and zeros in R, t, E and the mask.
 *   xfh_estimate_relpose_matches: the same on the matcher's output (kpts + idx0/idx1 + n_matches), as for the homography.
 * ---------------------------------------------------------------------------------------- */
size_t xfh_relpose_workspace_bytes(int P, int max_iters);
int xfh_estimate_relpose(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap,
                         const double* K0, const double* K1, double max_epipolar_error, int min_iters, int max_iters,
                         double success_prob, uint64_t seed, double* R, double* t, double* E, uint8_t* mask, int32_t* info,
                         void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_estimate_relpose_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                                 const int32_t* n_matches, int P, int cap, const double* K0, const double* K1,
                                 double max_epipolar_error, int min_iters, int max_iters, double success_prob, uint64_t seed,
                                 double* R, double* t, double* E, uint8_t* mask, int32_t* info,
                                 void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Relative pose at T RANSAC thresholds in one pass -- the protocol of modules/eval/scannet1500.py, which runs
 *     estimate_pose(kpts0, kpts1, K0, K1, thresh)
 * over all pairs at twelve thresholds (0.5 ... 6.0 px).  Slice j of the result IS xfh_estimate_relpose at
 * max_epipolar_errors[j] with the other arguments unchanged, bit for bit: a hypothesis does not depend on the threshold, so it
 * is solved once and every Sampson error is evaluated once; only the cost lists, the stopping rule and the refinement are per
 * threshold (DESIGN.md 3.10 / csrc/k_relpose.hip).
 *   max_epipolar_errors: T values in pixels in HOST memory (read before the call returns), 1 <= T <= 16, each finite and
 *   positive, in any order, repeats allowed.  The other inputs as for xfh_estimate_relpose.
 *   R (P,T,9), t (P,T,3), E (P,T,9) fp64; mask (P,T,cap) uint8; info (P,T,8) int32, the same eight words per (pair, threshold).
 *   xfh_estimate_relpose_sweep_matches: the same on the matcher's output (kpts + idx0/idx1 + n_matches).
 * ---------------------------------------------------------------------------------------- */
size_t xfh_relpose_sweep_workspace_bytes(int P, int max_iters, int T);
int xfh_estimate_relpose_sweep(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap,
                               const double* K0, const double* K1, const double* max_epipolar_errors, int T, int min_iters,
                               int max_iters, double success_prob, uint64_t seed, double* R, double* t, double* E, uint8_t* mask,
                               int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_estimate_relpose_sweep_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                                       const int32_t* n_matches, int P, int cap, const double* K0, const double* K1,
                                       const double* max_epipolar_errors, int T, int min_iters, int max_iters, double success_prob,
                                       uint64_t seed, double* R, double* t, double* E, uint8_t* mask, int32_t* info,
                                       void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Absolute pose from 2D-3D correspondences -- localisation against a model, or against a reference image with a depth map:
 *     pose, info = poselib.estimate_absolute_pose(points2D, points3D, camera, {"max_reproj_error": thr}, {})
 * for P query images at once.  poselib is not part of the reference tree: the algorithm is the published one (P3P RANSAC on
 * the classical quartic, MSAC on the reprojection error, Gauss-Newton refinement), specified in DESIGN.md 3.12 /
 * csrc/k_abspose.hip -- same estimate, not poselib's random stream.
 *   pts2d (P,cap,2) fp32 pixel coordinates in the query image, pts3d (P,cap,3) fp32 points in any world frame (device), row
 *   i of one matches row i of the other; pair p uses its first counts[p] rows (device int32; NULL: n_const for all); K
 *   (P,3,3) fp64 PINHOLE intrinsics of the query camera (device).  max_reproj_error in pixels (converted with (fx + fy) / 2).
 *   All max_iters (<= 16384; larger is an error) hypotheses are scored on the device, the stopping rule (min_iters,
 *   success_prob) applied to the cost list afterwards.
 *   R (P,9) fp64 row-major, t (P,3) fp64 with X_cam = R X_world + t (t in the world's unit, not normalised); mask (P,cap)
 *   uint8, 1 = reprojection error below the threshold and the point in front of the camera; info (P,8) int32: found,
 *   winning hypothesis, hypotheses the loop would have run, inliers, accepted refinement steps, n, cost (lo, hi word).
 *   Fewer than 3 correspondences / inliers: found = 0 and zeros in R, t and the mask.  A correspondence with a coordinate
 *   that is not finite is never sampled into a model and never an inlier.
 *   xfh_estimate_abspose_matches: the same on key-points (P,cap2d,2), 3D points (P,cap3d,3) -- the two capacities are
 *   independent -- and the matcher's lists: correspondence i of pair p is (kpts2d[p][idx2d[p][i]], points3d[p][idx3d[p][i]])
 *   for i < n_matches[p]; idx (P,cap) int64.
 * ---------------------------------------------------------------------------------------- */
size_t xfh_abspose_workspace_bytes(int P, int max_iters);
int xfh_estimate_abspose(const float* pts2d, const float* pts3d, const int32_t* counts, int n_const, int P, int cap,
                         const double* K, double max_reproj_error, int min_iters, int max_iters, double success_prob,
                         uint64_t seed, double* R, double* t, uint8_t* mask, int32_t* info,
                         void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_estimate_abspose_matches(const float* kpts2d, int cap2d, const float* points3d, int cap3d, const int64_t* idx2d,
                                 const int64_t* idx3d, const int32_t* n_matches, int P, int cap, const double* K,
                                 double max_reproj_error, int min_iters, int max_iters, double success_prob, uint64_t seed,
                                 double* R, double* t, uint8_t* mask, int32_t* info,
                                 void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * 3D-3D alignment: the similarity (with_scale != 0) or rigid (with_scale = 0, s = 1) transform B ~= s R A + t between two sets
 * of corresponding 3D points, for P pairs at once -- the metric pose of an RGB-D pair, the scale between two
 * reconstructions, the registration of a reconstruction to a metric frame.  RANSAC over a 3-point solver, MSAC on the point
 * distance, a closed-form least-squares refit of the consensus set (Horn's quaternion method), as specified in DESIGN.md
 * 3.15 / csrc/k_align.hip.
 *   pts_a, pts_b (P,cap,3) fp32 (device), row i of one matches row i of the other; pair p uses its first counts[p] rows
 *   (device int32; NULL: n_const for all).  A row with a coordinate that is not finite ("no point") is never sampled into a
 *   model and never an inlier.  max_error is a distance in B's unit (positive, finite).  All max_iters (<= 16384; larger is
 *   an error) hypotheses are scored on the device, the stopping rule (min_iters, success_prob) applied to the cost list
 *   afterwards.
 *   R (P,9) fp64 row-major (a proper rotation), t (P,3) fp64, s (P) fp64; mask (P,cap) uint8, 1 = |B - (s R A + t)| below
 *   max_error; info (P,8) int32: found, winning hypothesis, hypotheses the loop would have run, inliers, accepted refits, n,
 *   cost (lo, hi word).  Fewer than 3 correspondences / inliers: found = 0 and zeros in R, t, s and the mask.
 *   xfh_estimate_alignment_matches: the same on two point tables (P,cap_a,3), (P,cap_b,3) -- the two capacities are
 *   independent -- and index lists: correspondence i of pair p is (points_a[p][idx_a[p][i]], points_b[p][idx_b[p][i]]) for
 *   i < n_matches[p]; idx (P,cap) int64.  An index outside its table makes the correspondence "no point".
 * ---------------------------------------------------------------------------------------- */
size_t xfh_align_workspace_bytes(int P, int max_iters);
int xfh_estimate_alignment(const float* pts_a, const float* pts_b, const int32_t* counts, int n_const, int P, int cap,
                           int with_scale, double max_error, int min_iters, int max_iters, double success_prob,
                           uint64_t seed, double* R, double* t, double* s, uint8_t* mask, int32_t* info,
                           void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_estimate_alignment_matches(const float* points_a, int cap_a, const float* points_b, int cap_b, const int64_t* idx_a,
                                   const int64_t* idx_b, const int32_t* n_matches, int P, int cap, int with_scale,
                                   double max_error, int min_iters, int max_iters, double success_prob, uint64_t seed,
                                   double* R, double* t, double* s, uint8_t* mask, int32_t* info,
                                   void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Two-view structure: the 3D points of the correspondences under a relative pose, and the pose of an essential matrix
 *     n, R, t, mask = cv2.recoverPose(E, points1, points2, cameraMatrix[, distanceThresh])    (modules/eval/scannet1500.py:84)
 * for P pairs at once.  OpenCV is not available offline, so nothing is pinned to it: Lindstrom's optimal correction
 * (niter2) and the closed-form depths of the corrected rays, as specified in DESIGN.md 3.14 / csrc/k_triangulate.hip.
 * No workspace.  Every argument check returns before any launch.
 *   pts0/pts1, counts/n_const, K0/K1 and the _matches forms (kpts + idx0/idx1 + n_matches; kpt_cap rows per key-point
 *   list): as for xfh_estimate_relpose.  An index outside [0, kpt_cap) makes the correspondence "not finite".
 *   xfh_triangulate: R (P,3,3), t (P,3) fp64 with X1 = R X0 + t (the outputs of xfh_estimate_relpose; zeros = no pose);
 *     mask (P,cap) uint8 or NULL: a zero masks the correspondence out; max_reproj_error in pixels (positive, finite);
 *     cos_min = cos(minimal parallax angle), in [-1, 1]; max_depth > 0 in the unit of t (+inf: no limit).
 *     points3d (P,cap,3) fp32 in camera 0's frame, NaN unless status is 0; status (P,cap) uint8: XFH_TRI_*;
 *     reproj_error (P,cap) fp32 pixels, NaN for XFH_TRI_MASKED / XFH_TRI_NOT_FINITE; rows at or beyond the pair's count are
 *     written as masked.  info (P,8) int32: n, valid, masked, not finite, behind, far, reprojection, parallax (of the n rows).
 *     points3d_ref (P,kpt_cap,3) fp32 or NULL (_matches only): the valid points at image 0's key-point rows idx0[i], NaN
 *     elsewhere -- what xfh_estimate_abspose_matches takes as points3d.  One-to-one index lists are the contract; with
 *     duplicate rows in idx0 a row holds one of its candidates.
 *   xfh_recover_pose: E (P,3,3) fp64 at any scale or sign (x1' E x0 = 0 in calibrated coordinates; E = K1' F K0 for an F);
 *     mask_in as above; distance_thresh > 0 (+inf: no limit).  R, t (unit) of the pose, of the four E decomposes into, under
 *     which most correspondences have a depth in (0, distance_thresh) in both cameras (ties: the lower pose index, order
 *     (Ra,t) (Ra,-t) (Rb,t) (Rb,-t)); good (P,4) int32 the four counts; mask (P,cap) uint8 = mask_in and passes under the
 *     winner; points3d (P,cap,3) fp32 or NULL: the winner's points, NaN where the mask is 0; info (P,8) int32: found, pose
 *     index (-1: none), 0, the winner's count, 0, n, 0, 0.  An unusable E or a best count of 0: found = 0 and zeros.
 * ---------------------------------------------------------------------------------------- */
#define XFH_TRI_VALID 0
#define XFH_TRI_MASKED 1
#define XFH_TRI_NOT_FINITE 2
#define XFH_TRI_BEHIND 3
#define XFH_TRI_FAR 4
#define XFH_TRI_REPROJ 5
#define XFH_TRI_PARALLAX 6
int xfh_triangulate(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap,
                    const double* K0, const double* K1, const double* R, const double* t, const uint8_t* mask,
                    double max_reproj_error, double cos_min, double max_depth, float* points3d, uint8_t* status,
                    float* reproj_error, int32_t* info, xfh_stream stream);
int xfh_triangulate_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                            const int32_t* n_matches, int P, int cap, const double* K0, const double* K1, const double* R,
                            const double* t, const uint8_t* mask, double max_reproj_error, double cos_min, double max_depth,
                            float* points3d, uint8_t* status, float* reproj_error, int32_t* info, float* points3d_ref,
                            xfh_stream stream);
int xfh_recover_pose(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap,
                     const double* K0, const double* K1, const double* E, const uint8_t* mask_in, double distance_thresh,
                     double* R, double* t, int32_t* good, uint8_t* mask, float* points3d, int32_t* info, xfh_stream stream);
int xfh_recover_pose_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                             const int32_t* n_matches, int P, int cap, const double* K0, const double* K1, const double* E,
                             const uint8_t* mask_in, double distance_thresh, double* R, double* t, int32_t* good, uint8_t* mask,
                             float* points3d, int32_t* info, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Multi-view triangulation of key-point tracks: the point of every key-point of a reference view from all the views that see
 * it, for S scenes at once (DESIGN.md 3.16 / csrc/k_triangulate.hip).  Scene s has n_views[s] <= V <= 32 views with PINHOLE
 * intrinsics and world -> camera poses x_v = R_v X + t_v (the form xfh_estimate_abspose returns; (I, 0) and the R, t of
 * xfh_estimate_relpose are the two-view case); view 0 is the reference view, a track is a row of its key-point table.
 * No workspace.  Every argument check returns before any launch.
 *   xfh_build_tracks: idx_ref, idx_view (S,V-1,cap) int64, n_matches (S,V-1) int32: the matcher's lists of the pairs
 *     (view 0, view v), v = 1 .. V-1 (NULL allowed when cap is 0).  tracks (S,K,V) int32: [s,k,0] = k, [s,k,v] = the row of
 *     view v (< kpt_cap) matched to row k of view 0, or -1; an index outside either table is ignored; of duplicate reference
 *     rows the largest candidate row stays (reproducible).
 *   xfh_triangulate_views: kpts (S,V,kpt_cap,2) fp32 pixels; tracks as above; n_views (S,) int32 or NULL (= V); Ks, Rs
 *     (S,V,3,3), ts (S,V,3) fp64; max_reproj_error, cos_min, max_depth as for xfh_triangulate; min_views in [2, 32].
 *     Per track: hypotheses of the pairs (0, v) scored by MSAC over the views that see it, the inlier views of the best one,
 *     a Gauss-Newton refit on them, the gates.  points3d (S,K,3) fp32 in the world frame, NaN unless status is 0 (what
 *     xfh_estimate_abspose_matches takes as points3d, indexed by the reference rows); status (S,K) uint8: XFH_TRI_* with
 *     XFH_MV_UNOBSERVED for 1 (view 0 or every other view does not see the track); n_inliers (S,K) uint8; inlier_views (S,K)
 *     int32, bit v = view v; reproj_error (S,K) fp32 = the largest inlier error in pixels, NaN for status 1 and 2; info (S,8)
 *     int32: K, then the number of tracks per status 0 .. 6.
 * ---------------------------------------------------------------------------------------- */
#define XFH_MV_UNOBSERVED 1
#define XFH_MV_MAX_VIEWS 32
int xfh_build_tracks(const int64_t* idx_ref, const int64_t* idx_view, const int32_t* n_matches, int S, int V, int cap, int K,
                     int kpt_cap, int32_t* tracks, xfh_stream stream);
int xfh_triangulate_views(const float* kpts, int kpt_cap, const int32_t* tracks, const int32_t* n_views, int S, int K, int V,
                          const double* Ks, const double* Rs, const double* ts, double max_reproj_error, double cos_min,
                          double max_depth, int min_views, float* points3d, uint8_t* status, uint8_t* n_inliers,
                          int32_t* inlier_views, float* reproj_error, int32_t* info, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Tracks over an arbitrary graph of view pairs, and their triangulation (DESIGN.md 3.18 / csrc/k_tracks.hip,
 * csrc/k_triangulate.hip).  Every argument check returns before any launch; asynchronous, no host synchronisation inside.
 *   xfh_build_tracks_graph: view_pairs (S,P,2) int32, idx_a, idx_b (S,P,cap) int64, n_matches (S,P) int32: match i of pair
 *     p = (a, b) joins row idx_a[i] of view a with row idx_b[i] of view b (tables of K rows, V <= 32 views).  A pair with
 *     a == b or a view outside [0, V) and an index outside [0, K) are ignored; a pair may occur more than once.  A track is a
 *     connected component of the match graph with at most one key-point per view (others are dropped whole) that spans at
 *     least min_length (in [2, 32]) views; its id is the rank of its smallest node id v K + row within the scene; ids at or
 *     beyond max_tracks (in [1, V K]) are dropped and counted.  The result does not depend on the order of the lists.
 *     tracks (S,max_tracks,V) int32: a row or -1, rows >= n_tracks[s] all -1; track_of (S,V,K) int32: the track of a
 *     key-point or -1; n_tracks (S,) int32; info (S,8) int32: nodes matched, components, tracks kept, dropped inconsistent,
 *     dropped short, dropped over capacity, status (XFH_TRACKS_*), 0.  Every loop of the kernels is bounded by V K; status
 *     XFH_TRACKS_BOUND says that a thread reached its bound and gave up (the tables are then not to be used).
 *     workspace: xfh_track_graph_workspace_bytes(S, V, K) bytes, 256-byte aligned (0: bad shape).
 *   xfh_triangulate_tracks: the arguments and outputs of xfh_triangulate_views for tracks that view 0 need not see.  The
 *     anchor of a track is the lowest view that observes it: hypotheses of the pairs (anchor, v), status XFH_MV_UNOBSERVED
 *     only with fewer than two observing views, the anchor among the inliers or status 5, parallax against the anchor.  A
 *     track whose anchor is view 0 gets the bits of xfh_triangulate_views.
 * ---------------------------------------------------------------------------------------- */
#define XFH_TRACKS_OK 0
#define XFH_TRACKS_BOUND 2
size_t xfh_track_graph_workspace_bytes(int S, int V, int K);
int xfh_build_tracks_graph(const int32_t* view_pairs, const int64_t* idx_a, const int64_t* idx_b, const int32_t* n_matches, int S,
                           int P, int cap, int V, int K, int min_length, int max_tracks, int32_t* tracks, int32_t* track_of,
                           int32_t* n_tracks, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_triangulate_tracks(const float* kpts, int kpt_cap, const int32_t* tracks, const int32_t* n_views, int S, int K, int V,
                           const double* Ks, const double* Rs, const double* ts, double max_reproj_error, double cos_min,
                           double max_depth, int min_views, float* points3d, uint8_t* status, uint8_t* n_inliers,
                           int32_t* inlier_views, float* reproj_error, int32_t* info, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment: the poses of the free views and the points of the valid tracks of S scenes refined together by
 * Levenberg-Marquardt on the Huber-robust reprojection error (DESIGN.md 3.17 / csrc/k_triangulate.hip).  Asynchronous; no host
 * synchronisation inside.  Every argument check returns before any launch.
 *   kpts, tracks, n_views, Ks, Rs, ts as for xfh_triangulate_views; inlier_views (S,K) int32 and points3d (S,K,3) fp32 are its
 *   results.  Observation (k, w): bit w of inlier_views[k], w < n_views, an entry in range, a finite pixel, a usable pose, a
 *   finite point, depth > 0 and a finite error at the input state.  A track with fewer than 2 observations is not refined; a
 *   view is free when its bit in fixed_views is clear and it keeps at least 6 observations, every other view is held (its
 *   observations still constrain the points).  With only one view held the global scale is free: damping keeps it near the
 *   start, nothing pins it; hold two views for a pinned gauge.  max_iterations in [0, 1000]; huber_px > 0, +inf = plain squares.
 *   Outputs: Rs_out (S,V,3,3), ts_out (S,V,3) fp64 (held views: the input's bits); points3d_out (S,K,3) fp32 (refined tracks
 *   rounded once, every other row the input's bits); refined (S,K) uint8; free_views (S,) int32 mask; cost (S,2) fp64 = the
 *   robust cost before and after; info (S,8) int32: refined points, observations, free views, iterations, accepted steps,
 *   status (XFH_BA_*), 0, 0.  workspace: xfh_bundle_workspace_bytes(S, K, V) bytes, 256-byte aligned (0: bad shape).
 * ---------------------------------------------------------------------------------------- */
#define XFH_BA_OK 0
#define XFH_BA_NOTHING 1
#define XFH_BA_NOT_FINITE 2
size_t xfh_bundle_workspace_bytes(int S, int K, int V);
int xfh_bundle_adjust(const float* kpts, int kpt_cap, const int32_t* tracks, const int32_t* inlier_views, const float* points3d,
                      const int32_t* n_views, int S, int K, int V, const double* Ks, const double* Rs, const double* ts,
                      uint32_t fixed_views, int max_iterations, double huber_px, double* Rs_out, double* ts_out,
                      float* points3d_out, uint8_t* refined, int32_t* free_views, double* cost, int32_t* info, void* workspace,
                      size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Pose-graph initialisation: the world -> camera poses of the V <= 32 views of S scenes from the relative poses of P pairs of
 * views per scene: a spanning tree, robust rotation averaging and robust position averaging on the directions (DESIGN.md 3.19 /
 * csrc/k_triangulate.hip).  One launch, one workgroup per scene; asynchronous; no host synchronisation inside; two calls give
 * the same bits.  Every argument check returns before any launch.
 *   view_pairs (S,P,2) int32; edge p = (a, b) carries R_rel (S,P,3,3) and t_rel (S,P,3) fp64 with x_b = R_rel x_a + t_rel (what
 *   xfh_estimate_relpose returns with image 0 = a; only the direction of t_rel is used) and weight (S,P) fp64 >= 0.  n_views (S,)
 *   int32 or NULL = V.  An edge is valid when a != b, both views are in [0, n_views), the weight is finite and > 0 and R_rel is
 *   finite; it has a direction when t_rel is finite and not zero.  Duplicate pairs and pairs given as (b, a) are edges of their own.
 *   iterations in [1, 1000] rounds of each solve, the last redescend of them with Cauchy's factor, the others with Huber's;
 *   rot_scale_rad: the rotation residual's scale in radians; pos_scale_sin: the sine of the direction residual's scale;
 *   min_pivot_ratio: the smallest pivot^2 / diagonal of the position system below which the graph counts as not parallel-rigid.
 *   Gauge R_0 = I, c_0 = 0; the weighted mean of the baselines projected on their directions is 1.
 *   Outputs: Rs_out (S,V,3,3), ts_out (S,V,3) fp64, NaN for a view that the edges do not connect to view 0; registered (S,) int32
 *   mask of the connected views; edge_factor (S,P,2) fp64: the final rotation and position factors, 0 for an edge that took no
 *   part; info (S,8) int32: valid edges, registered views, edges with a direction, rotation edges with a final factor < 0.5,
 *   position edges likewise, unknowns of the position solve, status (XFH_PG_*), 0.  XFH_PG_NOTHING: no valid edge at view 0;
 *   XFH_PG_ROTATIONS_ONLY: the positions are not determined (Rs_out valid, ts_out of every view but 0 NaN);
 *   XFH_PG_NOT_FINITE: an output is not finite.  workspace: xfh_pose_graph_workspace_bytes(S, P, V) bytes, 256-byte aligned (0: bad shape).
 * ---------------------------------------------------------------------------------------- */
#define XFH_PG_OK 0
#define XFH_PG_NOTHING 1
#define XFH_PG_ROTATIONS_ONLY 2
#define XFH_PG_NOT_FINITE 3
size_t xfh_pose_graph_workspace_bytes(int S, int P, int V);
int xfh_average_poses(const int32_t* view_pairs, const double* R_rel, const double* t_rel, const double* weight,
                      const int32_t* n_views, int S, int P, int V, int iterations, int redescend, double rot_scale_rad,
                      double pos_scale_sin, double min_pivot_ratio, double* Rs_out, double* ts_out, int32_t* registered,
                      double* edge_factor, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Baseline scales from shared tracks (DESIGN.md 3.20 / csrc/posescale_body.hpp): what gives a chain of pairs (v, v + 1) positions.
 * Asynchronous; no host synchronisation inside; two calls give the same bits.  Every argument check returns before any launch.
 *   xfh_baseline_ratios: kpts (S,V,K,2) fp32; tracks (S,T,V), track_of (S,V,K) int32 as xfh_build_tracks_graph writes them;
 *     view_pairs, R_rel, t_rel, weight, n_views as for xfh_average_poses; Ks (S,V,3,3) fp64; the gates max_reproj_error (pixels),
 *     cos_min (the cosine of the smallest parallax) and max_depth of xfh_triangulate; P <= 512, K <= 4096.  A wedge is a pair of
 *     edges p < q, both valid and with a direction, whose view sets share exactly one view v.  Every track with a key-point in v
 *     and in the other view of either edge is triangulated under both edges; where both are valid the quotient of its two depths
 *     in v is a value, and the wedge's ratio |baseline p| / |baseline q| is the lower median (element (n - 1) / 2 in ascending
 *     order) of its n values when n >= min_common.
 *     Outputs, all (S,P,P) and fully written: ratio fp64 (NaN: none), count int32 (n, 0: no wedge), shared_view int32 (-1: no
 *     wedge); entries with p >= q are (NaN, 0, -1).  info (S,8) int32: wedges, wedges with a ratio, tracks examined, tracks
 *     valid, status (XFH_PS_*), 0, 0, 0.  workspace: xfh_baseline_ratios_workspace_bytes(S, P, V, K) bytes (0: bad shape).
 *   xfh_average_poses_ratios: xfh_average_poses with the ratios in its position rounds (P <= 512): a wedge whose two edges are
 *     both in the registered component, with a finite ratio > 0 and ratio_count > 0, adds (scale_weight ratio_count factor) h h'
 *     to the position system, h the gradient of u_p / sqrt(r) - sqrt(r) u_q, u the baseline projected on its direction; the
 *     factor is 1 in the first round and then Huber's or Cauchy's (as the edges') of |u_p - r u_q| / (u_p + r u_q) at scale_tol
 *     in (0, 1].  ratio_factor (S,P,P) fp64: the final factors, 0 for a wedge that took no part.  Everything else as
 *     xfh_average_poses.  workspace: xfh_pose_graph_ratios_workspace_bytes(S, P, V) bytes, 256-byte aligned (0: bad shape).
 * ---------------------------------------------------------------------------------------- */
#define XFH_PS_OK 0
size_t xfh_baseline_ratios_workspace_bytes(int S, int P, int V, int K);
int xfh_baseline_ratios(const float* kpts, const int32_t* tracks, const int32_t* track_of, const int32_t* view_pairs,
                        const double* R_rel, const double* t_rel, const double* weight, const double* Ks, const int32_t* n_views,
                        int S, int P, int V, int K, int T, double max_reproj_error, double cos_min, double max_depth,
                        int min_common, double* ratio, int32_t* count, int32_t* shared_view, int32_t* info, void* workspace,
                        size_t workspace_bytes, xfh_stream stream);
size_t xfh_pose_graph_ratios_workspace_bytes(int S, int P, int V);
int xfh_average_poses_ratios(const int32_t* view_pairs, const double* R_rel, const double* t_rel, const double* weight,
                             const int32_t* n_views, const double* ratio, const int32_t* ratio_count, int S, int P, int V,
                             int iterations, int redescend, double rot_scale_rad, double pos_scale_sin, double min_pivot_ratio,
                             double scale_weight, double scale_tol, double* Rs_out, double* ts_out, int32_t* registered,
                             double* edge_factor, double* ratio_factor, int32_t* info, void* workspace, size_t workspace_bytes,
                             xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Map rows for localisation (DESIGN.md 3.21 / csrc/k_map.hip): a 3D point with a descriptor for every usable track of a
 * triangulation, to be matched against a query image as side 2 of xfh_match_mnn, and the pixels of the rows under a pose as the
 * key-points of xfh_match_mnn_guided.  Asynchronous; no host synchronisation inside; two calls give the same bytes.  Every
 * argument check returns before any launch.
 *   xfh_build_map: desc (S,V,kpt_cap,64) fp32, the L2-normalised descriptor tables of the views (16-byte aligned); tracks
 *     (S,T,V) int32, points3d (S,T,3) fp32, status (S,T) uint8, inlier_views (S,T) int32 as xfh_triangulate_views /
 *     xfh_triangulate_tracks write them.  V <= 32 (XFH_ERR_UNSUPPORTED beyond), min_views in [1, 32], max_points = M >= 1.
 *     View v contributes to track t iff bit v of inlier_views[t] is set (read as unsigned), 0 <= tracks[t,v] < kpt_cap and all 64
 *     components of that row are finite.  A track is selected unless, tested in this order: status != 0; a coordinate of its point
 *     is not finite; fewer than min_views contributing views; the sum of the contributing rows (per component, fp32, views
 *     ascending) has a squared norm n2 that is not finite or below FLT_MIN.  The selected tracks fill the rows 0, 1, ... in
 *     ascending track id; those beyond M are dropped and counted.
 *     Outputs: points (S,M,3) fp32 (the input's bits), map_desc (S,M,64) fp32 = sum * (1 / sqrt(n2)), map_desc_f16 (S,M,64) the
 *     fp16 round-to-nearest-even of 256 * map_desc (d2_f16 of xfh_match_mnn), track (S,M) int32 the track id, n_obs (S,M) uint8 the
 *     contributing views, coherence (S,M) fp32 = sqrt(n2) / n_obs (1: all observations agree, 0: they cancel), n_points (S,) int32.
 *     Rows from n_points on: NaN point, zero descriptors, track -1, n_obs 0, coherence 0.  info (S,8) int32: T, rows written,
 *     skipped by status, by the point, by the views, by the norm, dropped over capacity, 0.
 *     workspace: xfh_map_workspace_bytes(S, T, V) bytes, 256-byte aligned (0: bad shape).
 *   xfh_map_project: points (Q,M,3) fp32, n_points (Q,) int32 or NULL = M, R (Q,3,3), t (Q,3), K (Q,3,3) fp64 row-major (device).
 *     uv (Q,M,2) fp32 = K (R X + t) in fp64, dehomogenised and rounded once; NaN for a row >= n_points, a depth that is not finite
 *     or not > 0, a pixel that is not finite and, when an image size is given (width, height > 0; 0, 0: none), a pixel more than
 *     margin outside [0, width] x [0, height].
 * ---------------------------------------------------------------------------------------- */
size_t xfh_map_workspace_bytes(int S, int T, int V);
int xfh_build_map(const float* desc, int kpt_cap, const int32_t* tracks, const float* points3d, const uint8_t* status,
                  const int32_t* inlier_views, int S, int T, int V, int min_views, int max_points, float* points, float* map_desc,
                  uint16_t* map_desc_f16, int32_t* track, uint8_t* n_obs, float* coherence, int32_t* n_points, int32_t* info,
                  void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_map_project(const float* points, const int32_t* n_points, int Q, int M, const double* R, const double* t, const double* K,
                    double width, double height, double margin, float* uv, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Geometric verification of match lists before they become tracks (DESIGN.md 3.22 / csrc/k_matchfilter.hip, csrc/k_triangulate.hip).
 * Asynchronous; no host synchronisation inside; no workspace; two calls give the same bytes.  Every argument check returns before
 * any launch.
 *   xfh_filter_matches: the order-preserving compaction of L match lists by a mask.  idx_a, idx_b (L,cap) int64, n_matches (L,)
 *     int32 (read clamped to [0, cap]), mask (L,cap) uint8 (non-zero keeps an entry; the inlier mask of any estimator), keep (L,)
 *     uint8 or NULL (zero empties the list), min_keep >= 0 (a list that keeps fewer entries is emptied).  Outputs: out_a, out_b
 *     (L,cap) int64 = the kept entries in their original order, then -1; src (L,cap) int32 = the original position of each kept
 *     entry, then -1 (to gather scores, refined coordinates or a second mask); n_out (L,) int32; info (L,4) int32: entries read,
 *     entries whose mask is set, the reason the list was emptied (XFH_FILTER_*), 0.  L = 0 or cap = 0 return without a launch;
 *     L above 2^31 - 1 is XFH_ERR_UNSUPPORTED.  The call is not in-place: an output range that overlaps an input range (or
 *     another output) is XFH_ERR_ARG.
 *   xfh_verify_matches: the epipolar test of every match of the pairs of a pair graph under the world poses of the views.
 *     kpts (S,V,K,2) fp32 (8-byte aligned); view_pairs (S,P,2) int32, idx_a, idx_b (S,P,cap) int64, n_matches (S,P) int32 as for
 *     xfh_build_tracks_graph; n_views (S,) int32 or NULL = V; Ks (S,V,3,3), Rs (S,V,3,3), ts (S,V,3) fp64, x_v = R_v X + t_v;
 *     max_epipolar_error in pixels, finite and > 0; V <= 32 (XFH_ERR_UNSUPPORTED beyond).  Per pair (a, b): status
 *     XFH_VERIFY_PAIR when a == b or a view is outside [0, n_views); XFH_VERIFY_POSE when a pose has an entry that is not finite
 *     or an all-zero R; XFH_VERIFY_BASELINE when t_rel = t_b - R_rel t_a is zero (R_rel = R_b R_a'); else E = [t_rel]x R_rel and
 *     the threshold max_epipolar_error / f, f the mean of the four focal lengths (what xfh_estimate_relpose uses).  A match is
 *     evaluated when the pair is ok, both rows are in [0, K) and its four pixel coordinates are finite: r2 = its Sampson error
 *     in normalised coordinates (fp64), mask = r2 finite and r2 < threshold^2 (strict).  No cheirality test.
 *     Outputs: mask (S,P,cap) uint8, 0 for every entry that is not evaluated; err (S,P,cap) fp32 or NULL = sqrt(r2) f in pixels,
 *     rounded once, NaN where nothing was evaluated; pair_info (S,P,4) int32: status, entries read, entries kept, 0.
 * ---------------------------------------------------------------------------------------- */
#define XFH_FILTER_NONE 0
#define XFH_FILTER_BY_KEEP 1
#define XFH_FILTER_BY_MIN_KEEP 2
#define XFH_VERIFY_OK 0
#define XFH_VERIFY_PAIR 1
#define XFH_VERIFY_POSE 2
#define XFH_VERIFY_BASELINE 3
int xfh_filter_matches(const int64_t* idx_a, const int64_t* idx_b, const int32_t* n_matches, const uint8_t* mask, const uint8_t* keep,
                       int64_t L, int cap, int min_keep, int64_t* out_a, int64_t* out_b, int32_t* src, int32_t* n_out, int32_t* info,
                       xfh_stream stream);
int xfh_verify_matches(const float* kpts, const int32_t* view_pairs, const int64_t* idx_a, const int64_t* idx_b,
                       const int32_t* n_matches, const int32_t* n_views, int S, int P, int cap, int V, int K, const double* Ks,
                       const double* Rs, const double* ts, double max_epipolar_error, uint8_t* mask, float* err, int32_t* pair_info,
                       xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Image retrieval (DESIGN.md 3.23 / csrc/k_retrieval.hip): which images to match and which map to query.  VLAD global descriptors of
 * the local descriptors over a codebook learned by spherical k-means from those descriptors, top-k shortlists from the inner
 * products of the global vectors, and the pair list of a scene from its shortlists.  All fp32 (the k-means objective fp64) in
 * orders of summation that the shapes fix: two calls give the same bytes.  Asynchronous; no host synchronisation inside.  Every
 * argument check returns before any launch: XFH_ERR_UNSUPPORTED for C, D, k or V beyond the limits, XFH_ERR_ARG otherwise,
 * XFH_ERR_WORKSPACE for the workspace (256-byte aligned; the *_workspace_bytes functions return 0 for a bad shape).
 *   desc (G,K,64) fp32 unit rows (16-byte aligned), counts (G,) int32 or NULL = K (read clamped to [0, K]), codebook (C,64) fp32,
 *   C in {32, 64, 128, 256}.  Row i of group g is valid iff i < counts[g] and its 64 components are finite.  assign (G,K) int32 =
 *   the centroid with the largest inner product (a chain over the 64 components) among the finite ones, the lowest index among
 *   equals; -1 for a row that is not valid or has no finite score.
 *   xfh_vlad: G K <= 2^24.  Per (group, centroid) the residuals row - codebook[c] of the rows assigned to c are summed in ascending
 *     row order (chunks of 1024 rows, the chunk sums added ascending); a 64-block whose squared norm n2 is finite and >= FLT_MIN is
 *     multiplied by 1 / sqrt(n2), any other becomes zero; the vector is multiplied by 1 / sqrt(m), m the number of non-zero blocks.
 *     vlad (G,C*64) fp32, n_assigned (G,C) int32, info (G,4) int32: valid rows, rows below the count that are not finite, m,
 *     1 when m = 0 (an all-zero vector).
 *   xfh_kmeans_step: one step of spherical k-means over the G K <= 2^22 rows as ONE set (in the order (g, i)).  codebook_out (C,64)
 *     = the ordered sum of the rows of a cluster times 1 / sqrt(n2); a cluster that is empty or whose n2 is not finite or below
 *     FLT_MIN keeps its centroid.  n_assigned (C,) int32; objective: one fp64 value, the fixed-order sum of the winning scores;
 *     info (4,) int32: valid rows, rows below the count that are not finite, clusters that kept their centroid, 0.
 *     codebook_out must not be codebook.
 *   xfh_retrieve_topk: q (G,Q,D), db (G,N,D) fp32 (16-byte aligned), n_db (G,) int32 or NULL = N; D a multiple of 64, D <= 16384;
 *     1 <= k <= 128; exclude_self != 0: query j never returns database row j.  The score is the fp32 inner product (chains over
 *     the 64 components of a block, over the 16 blocks of a segment and over the segments).  idx (G,Q,k) int32, score (G,Q,k) fp32:
 *     the rows below n_db with a finite score by score descending, then index ascending; -1 and NaN past the number found.
 *   xfh_pairs_from_shortlists: idx (S,V,k) int32, n_views (S,) int32 or NULL = V, 2 <= V <= 32, k <= 128.  view_pairs (S,Pcap,2)
 *     int32, Pcap = min(V k, V (V - 1) / 2): the undirected union of the edges (v, idx[s,v,j]) as pairs a < b in ascending (a, b)
 *     order without duplicates, then (-1, -1); entries that are negative, not below n_views or equal to v are ignored.
 *     n_pairs (S,) int32.  No workspace.
 * ---------------------------------------------------------------------------------------- */
size_t xfh_vlad_workspace_bytes(int G, int K, int C);
int xfh_vlad(const float* desc, const int32_t* counts, int G, int K, const float* codebook, int C, float* vlad, int32_t* assign,
             int32_t* n_assigned, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream);
size_t xfh_kmeans_workspace_bytes(int G, int K, int C);
int xfh_kmeans_step(const float* desc, const int32_t* counts, int G, int K, const float* codebook, int C, float* codebook_out,
                    int32_t* assign, int32_t* n_assigned, double* objective, int32_t* info, void* workspace,
                    size_t workspace_bytes, xfh_stream stream);
size_t xfh_retrieve_workspace_bytes(int G, int Q, int N);
int xfh_retrieve_topk(const float* q, const float* db, const int32_t* n_db, int G, int Q, int N, int D, int k, int exclude_self,
                      int32_t* idx, float* score, void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_pairs_from_shortlists(const int32_t* idx, const int32_t* n_views, int S, int V, int k, int32_t* view_pairs,
                              int32_t* n_pairs, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Fundamental matrix from the matches -- match verification for uncalibrated, non-planar pairs:
 *     F, inliers = cv2.findFundamentalMat(points1, points2, cv2.USAC_MAGSAC, ransac_thr, confidence, maxIters)
 * for P pairs at once.  OpenCV is not part of the reference tree (which never calls it): the algorithm is the published one
 * (7-point RANSAC with the oriented epipolar constraint, MAGSAC++ quality and sigma-consensus++ re-weighted 8-point
 * refinement) as specified in DESIGN.md 3.11 / csrc/k_fundamental.hip -- same estimate, not OpenCV's random stream.
 *   pts0/pts1 (P,cap,2) fp32 pixel coordinates (device), pair p uses its first counts[p] rows (device int32; NULL: n_const
 *   for all).  method XFH_FM_USAC_MAGSAC: all max_iters (<= 16384; larger is an error) hypotheses are scored on the device,
 *   the stopping rule (confidence) applied to the score list afterwards; XFH_FM_8POINT: one least-squares 8-point fit on
 *   all n >= 8 points; XFH_FM_7POINT: the 7-point solver on exactly 7 points, every real root.
 *   F (P,3,9) fp64 row-major, model m of pair p at F[p][m]: one model (m = 0) except for XFH_FM_7POINT (up to 3); scaled to
 *   F[8] = 1 when |F[8]| > FLT_EPSILON after normalising to unit Frobenius norm; zeros where there is no model.
 *   mask (P,cap) uint8, 1 = Sampson error < ransac_thr (pixels) under the final F (non-robust methods: 1 for every point
 *   used); info (P,8) int32: found, winning hypothesis (-1: none / non-robust), hypotheses the loop would have run (non-robust:
 *   the number of models), inliers, accepted refinement steps, n, quality (lo, hi word).  found = 0 with fewer than 7
 *   inliers (cv2 returns None).  xfh_find_fundamental_matches: the same on the matcher's output (kpts + idx0/idx1 +
 *   n_matches), as for the homography.
 * ---------------------------------------------------------------------------------------- */
enum { XFH_FM_7POINT = 1, XFH_FM_8POINT = 2, XFH_FM_USAC_MAGSAC = 38 };
size_t xfh_fundamental_workspace_bytes(int P, int max_iters);
int xfh_find_fundamental(const float* pts0, const float* pts1, const int32_t* counts, int n_const, int P, int cap, int method,
                         double ransac_thr, int max_iters, double confidence, uint64_t seed,
                         double* F, uint8_t* mask, int32_t* info, void* workspace, size_t workspace_bytes, xfh_stream stream);
int xfh_find_fundamental_matches(const float* kpts0, const float* kpts1, int kpt_cap, const int64_t* idx0, const int64_t* idx1,
                                 const int32_t* n_matches, int P, int cap, int method, double ransac_thr, int max_iters,
                                 double confidence, uint64_t seed, double* F, uint8_t* mask, int32_t* info,
                                 void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * LighterGlue: the attention matcher of XFeat.match_lighterglue (modules/xfeat.py:131-162), i.e.
 * kornia.feature.lightglue.LightGlue.forward under the configuration of modules/lighterglue.py:12-27 (input 64-D,
 * d = 96, one head, 6 layers, no early stop, width pruning 0.95, filter threshold = min_conf), for ONE pair
 * (the reference asserts B = 1).  Its own checkpoint (weights/xfeat-lighterglue.pt) -> its own handle.
 *
 *   host_arrays : fp32 arrays in kornia's module order after the reference loader's renaming
 *                 (modules/lighterglue.py:41-46): input_proj.{weight,bias}, posenc.Wr.weight, per layer
 *                 transformers.i.self_attn.{Wqkv,out_proj,ffn.0,ffn.1,ffn.3}.{weight,bias},
 *                 transformers.i.cross_attn.{to_qk,to_v,to_out,ffn.0,ffn.1,ffn.3}.{weight,bias}, then
 *                 log_assignment.i.{matchability,final_proj}.{weight,bias}, then token_confidence.i.token.0.{weight,bias}
 *                 (xfh_lg_num_weight_arrays() = 169; sizes from xfh_lg_weight_array_floats).
 *   xfh_lg_match: kpts (N,2) pixel coordinates, desc (N,64), image size (W,H) per image.  prune_min_kpts: after every
 *                 layer but the last, a set that still has MORE than this many key-points drops those whose
 *                 matchability is <= 1 - width_confidence (the published pruning_keypoint_thresholds: -1 on CPU =
 *                 always, 1024 on CUDA, 1536 on CUDA with flash attention); XFH_LG_NO_PRUNING disables it.  Output: matches (<= min(N0,N1), 2) int64 indices into the input
 *                 lists, ascending in column 0; scores; n_matches (1) int32 -- all device memory, asynchronous.  The rows from n_matches
 *                 to min(N0,N1) are written as (-1,-1) with score 0.
 * ---------------------------------------------------------------------------------------- */
#define XFH_LG_NO_PRUNING (1 << 30)
typedef struct xfh_lg_context* xfh_lg_handle;
int xfh_lg_num_weight_arrays(void);
size_t xfh_lg_weight_array_floats(int index);
int xfh_lg_create(const float* const* host_arrays, int n_arrays, int device, xfh_lg_handle* out);
void xfh_lg_destroy(xfh_lg_handle h);
size_t xfh_lg_workspace_bytes(int N0, int N1);
int xfh_lg_match(xfh_lg_handle h, const float* kpts0, const float* desc0, int N0, float W0, float H0,
                 const float* kpts1, const float* desc1, int N1, float W1, float H1, float min_conf, int prune_min_kpts,
                 int64_t* matches, float* scores, int32_t* n_matches, void* workspace, size_t workspace_bytes,
                 xfh_stream stream);

/* bench.py hook: HIP events on the launch stream around every attention launch of this handle (lg_attention_kernel, both
 * images per launch) while enabled; xfh_lg_profile_read returns their number, summed duration and algorithmic FLOPs
 * (4 N_q N_k 96 per image and launch, at the key-point capacities -- run with XFH_LG_NO_PRUNING for exact figures) and resets. */
int xfh_lg_profile(xfh_lg_handle h, int enable);
int xfh_lg_profile_read(xfh_lg_handle h, int* n_launches, double* total_ms, double* total_flops);

/* The batch form used with xfh_detect_sparse's fixed-capacity outputs: frames (2p, 2p+1) of kpts (2P,cap,2) /
 * desc (2P,cap,64) / counts (2P) int32 (all device memory) form pair p; every image has size (W,H).  No host
 * read-back of the counts; pairs run back to back on `stream` and share one workspace of
 * xfh_lg_workspace_bytes(cap, cap).  Outputs: matches (P,cap,2) int64, scores (P,cap), n_matches (P) int32; the rows of pair p from
 * n_matches[p] to cap are written as (-1,-1) with score 0. */
int xfh_lg_match_pairs(xfh_lg_handle h, const float* kpts, const float* desc, const int32_t* counts, int P, int cap,
                       float W, float H, float min_conf, int prune_min_kpts, int64_t* matches, float* scores,
                       int32_t* n_matches, void* workspace, size_t workspace_bytes, xfh_stream stream);

/* ------------------------------------------------------------------------------------------
 * Kernel timing hooks for bench.py (HIP events recorded around one kernel family on the
 * launch stream).  which: see XFH_PROF_* ; xfh_profile_read synchronises the recorded events
 * and returns the number of launches and their summed duration in milliseconds.
 * ---------------------------------------------------------------------------------------- */
enum { XFH_PROF_NONE = 0, XFH_PROF_CONV_MFMA = 1, XFH_PROF_MATCH = 2, XFH_PROF_BLOCK1 = 3, XFH_PROF_HEADS = 4,
       XFH_PROF_CONV_64_64_S1 = 5 /* launches of conv_mfma_kernel<64,64,3,1,..>: the 64->64 3x3 stride-1 layers */,
       XFH_PROF_CONV_24_24 = 6 /* the two 24->24 3x3 stride-1 layers (block2.0 / block2.1): one kernel instantiation, two launches per step */,
       XFH_PROF_CONV_LAYER0 = 100 /* + index into spec.CONVS: one MFMA conv layer only */,
       XFH_PROF_ALL = 1000 /* every kernel (or tight kernel group) of xfh_backbone / xfh_detect_sparse / xfh_match_mnn as its own span: read with xfh_profile_read_spans */ };
/* span ids reported under XFH_PROF_ALL (next to XFH_PROF_BLOCK1 and XFH_PROF_CONV_LAYER0 + layer) */
enum { XFH_SPAN_GRAY = 200, XFH_SPAN_PYRAMID = 201, XFH_SPAN_HEAD_REL = 202, XFH_SPAN_HEAD_KP = 203,
       XFH_SPAN_NMS_FLAGS = 210, XFH_SPAN_NMS_COMPACT = 211, XFH_SPAN_TOPK = 212, XFH_SPAN_DESCRIPTOR = 213,
       XFH_SPAN_MATCH_ZERO = 220, XFH_SPAN_MATCH_PREP = 221, XFH_SPAN_MATCH_SWEEP = 222, XFH_SPAN_MATCH_REFINE = 223, XFH_SPAN_MATCH_FINALIZE = 224,
       XFH_SPAN_MATCH_EXACT = 225 };
int xfh_profile_select(xfh_handle h, int which);
/* the spans recorded since the last read, in launch order: ids[i], ms[i] for i < min(*n_spans, capacity); synchronises; resets */
int xfh_profile_read_spans(xfh_handle h, int* ids, double* ms, int capacity, int* n_spans);
/* debug: 24 int64 s_memtime stamps per MFMA-conv workgroup are written to device_buffer (NULL = off) */
int xfh_debug_trace(xfh_handle h, long long* device_buffer);
/* debug / torture (process-wide, not for production): with enable != 0 every matrix-core kernel of the backbone invalidates the instruction cache when a
 * workgroup starts, so that its first tile runs on instruction-fetch misses -- the condition under which round 3's split-bf16 key-point head (deleted in round 6) was found to
 * deliver a wrong 16-cell block; the concurrency / cold-start soaks of tests/test_gpu_parity.py, tools/final_soak.py and the code-position scan
 * (tools/bench_src/scan_probe.cpp) use it.
 * WHY THE HOOK SHIPS IN THE PRODUCTION LIBRARY instead of a debug build: the hazard it provokes depends on where a kernel's instructions lie relative to the
 * instruction-cache lines (3 of 16 code positions failed for that head).  Evidence gathered on a debug twin -- the same source compiled with another flag, i.e.
 * other offsets -- would say nothing about the shipped bytes.  The in-suite soak and the scans therefore torture THE library that ships; the price is one scalar
 * compare at kernel entry (cold == 0: not taken) and this one process-wide int, which no product path writes.  The xfh_debug_* entry points that only probe
 * (block1, trace, match_occupancy) are thin launchers of shipped kernels: they add no state. */
int xfh_debug_cold_start(int enable);
/* debug: block1 + skip1 alone in the form option "block1" selects: gray (B,H,W) raw gray image, coef (B,2) the per-image {alpha, beta} of the instance
 * normalisation (x -> alpha x + beta), x1 (B,24,H/4,W/4); H % 4 == W % 4 == 0.  For the variant-against-variant tests of tests/test_gpu_parity.py. */
int xfh_debug_block1(xfh_handle h, const float* gray, const float* coef, int B, int H, int W, float* x1, xfh_stream stream);
/* debug: resident workgroups per CU the runtime reports for mnn_sim_kernel */
int xfh_debug_match_occupancy(void);
int xfh_profile_read(xfh_handle h, int* n_launches, double* total_ms, double* total_flops, double* total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* XFEAT_HIP_H */
