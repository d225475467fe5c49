/* libicematch — C ABI of the MI355X (gfx950) learned extraction + matching hot path.
 *
 * The reference (franioli/icepy4d) is pure Python: its "plugin" seam for this path is
 * `ImageMatcherBase._match_images(image0, image1, **config)` (`src/icepy4d/matching/matchers.py:276-302`),
 * implemented by `LightGlueMatcher._match_images` (`:1226-1304`) and `SuperGlueMatcher._match_images`
 * (`:892-940`), which call torch modules.  This library is what those two methods bind instead of torch:
 * the host side (`icepy4d_amd/matching/matchers.py`, ctypes) keeps the reference's class / method names.
 *
 * Conventions
 *   - every `d_*` pointer is a DEVICE pointer owned by the caller (e.g. a torch tensor); `h_*` is host memory
 *   - `stream` is a `hipStream_t` passed as void*; calls only enqueue work (no host sync) unless stated
 *   - return value: 0 = ok, negative = error (see `im_last_error`); no exceptions cross the boundary
 *   - a context is not re-entrant: use one context per (process, device, stream)
 *   - dynamic sizes (keypoint counts) stay in device memory: `d_n*` are `int32` device scalars
 */
#ifndef ICEMATCH_H
#define ICEMATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct im_ctx im_ctx;

/* ---- context ------------------------------------------------------------------------------------ */
int im_version(void);
/* Binds to HIP device `device` (replaces `.to(device)` at `matchers.py:852, 1256-1258`). */
int im_ctx_create(int device, im_ctx** out);
void im_ctx_destroy(im_ctx* ctx);
const char* im_last_error(im_ctx* ctx);
/* Allocates every workspace for images up to max_h x max_w, `max_images` images per call and `max_kpts`
 * keypoints per image. Must be called before any forward; may be called again to grow. Synchronises. */
int im_ctx_reserve(im_ctx* ctx, int max_h, int max_w, int max_images, int max_kpts);

/* Per-launch timing with HIP events recorded on the launch stream (what bench.py's roofline leg reads).
 * begin: synchronises and arms; end: synchronises and writes a JSON object {"kernel": {"count", "total_ms"}}. */
int im_profile_begin(im_ctx* ctx);
int im_profile_end(im_ctx* ctx, char* buf, size_t cap);

/* ---- weights: tensors are passed under their OFFICIAL state-dict key names --------------------------
 * model: "superpoint" (`lightglue/superpoint.py:118-137` == `SuperGlue/models/superpoint.py:122-140`),
 *        "lightglue"  (`lightglue/lightglue.py:350-373`), "superglue" (`SuperGlue/models/superglue.py:221-242`).
 * `h_data` is host fp32, `numel` elements, torch-contiguous layout. Replaces `load_state_dict`
 * (`lightglue/superpoint.py:139-140`, `lightglue/lightglue.py:376-392`, `superglue.py:244-247`). */
int im_set_tensor(im_ctx* ctx, const char* model, const char* key, const float* h_data, size_t numel);
/* Checks that every tensor of `model` was provided, re-packs (conv slabs, head-major q/k/v, folded BatchNorm)
 * and uploads. Synchronises. */
int im_finalize_weights(im_ctx* ctx, const char* model);

/* ---- SuperPoint: `SuperPoint.extract` / `.forward` -----------------------------------------------
 * (`lightglue/superpoint.py:146-231`, `SuperGlue/models/superpoint.py:151-220`).
 * d_img: uint8 [n_images][h][w][channels], channels = 1 (gray) or 3 (RGB, the layout `core/images.py:75` hands to
 * `match()`); the u8 -> float conversion of `_frame2tensor` (`matchers.py:263-274, 1212-1220`) and, for 3 channels, the gray
 * conversion happen per pixel inside the first convolution's producer, exactly as the reference orders them:
 *   flavour 0 = LightGlue: scale to float, then kornia's weights on the FLOAT image (`lightglue/utils.py:35-36`);
 *               border := -1 before the threshold (`lightglue/superpoint.py:177-184`)
 *   flavour 1 = SuperGlue: cv2.cvtColor(RGB2GRAY) on the UINT8 image (fixed point), then scale (`matchers.py:911-917`);
 *               threshold, then the coordinate border mask (`SuperGlue/models/superpoint.py:176-189`)
 * channels = 4 is a float32 gray image [n_images][h][w] (4 bytes per pixel) the caller has already scaled to [0, 1]: the
 * `resize` option of `SuperPoint.extract` (`lightglue/utils.py:30-33`), whose kornia resize runs on the host.
 * max_kpts <= 0 means unlimited (bounded by the reserved max_kpts: see im_superpoint_candidates).
 * Outputs (row stride = reserved max_kpts): d_kpts [n_images][max_kpts][2] (x, y), d_scores [n_images][max_kpts],
 * d_desc [n_images][max_kpts][256] (L2-normalised), d_n [n_images]. */
int im_superpoint_forward(im_ctx* ctx, const uint8_t* d_img, int n_images, int h, int w, int channels,
                          int nms_radius, float threshold, int border, int max_kpts, int flavour,
                          float* d_kpts, float* d_scores, float* d_desc, int32_t* d_n, void* stream);
/* Number of candidates (NMS survivors above the threshold, inside the border) each image of the LAST im_superpoint_forward
 * had BEFORE the top-k / capacity cut; h_counts: host int32 [n_images]. Synchronises the stream. `max_keypoints = -1`
 * (`SuperGlue/models/superpoint.py:176-203`, icepy4d's SuperGlue default `matchers.py:859`) means "all of them": the caller
 * compares with the reserved max_kpts, grows the workspace (im_ctx_reserve) and repeats the forward if any were cut. */
int im_superpoint_candidates(im_ctx* ctx, int n_images, int32_t* h_counts, void* stream);

/* ---- LightGlue: `LightGlue._forward` on the reference's CPU path (`lightglue/lightglue.py:436-556`) ----
 * Inputs for image 0/1 are the two slices of the SuperPoint outputs above (same strides, n_images = 2).
 * h_size: host [2][2] = (W, H) of image 0 and 1 (`image_size`, `lightglue/superpoint.py:229`).
 * Outputs: d_matches [2][max_kpts] int32 (-1 = none; row 0 = matches0, row 1 = matches1),
 * d_mscores [2][max_kpts], d_prune [2][max_kpts] int32, d_info int32[4] = {stop, n0_final, n1_final, 0}. */
typedef struct {
    double depth_confidence; /* <= 0 disables early stop   (`lightglue.py:317`); doubles: the reference holds */
    double width_confidence; /* <= 0 disables point pruning (`lightglue.py:318`); Python floats and derives   */
    double filter_threshold; /* `lightglue.py:319`                                 1 - width_confidence in double */
    int n_layers;            /* 9 */
    int pruning_min_kpts;    /* an image is pruned after a layer only while it holds MORE live points than this
                                (`lightglue.py:326-331, 495, 503, 581-585`): -1 = the reference's CPU path (always), 1024 = its CUDA
                                path, 1536 = CUDA with FlashAttention */
} im_lightglue_conf;
int im_lightglue_forward(im_ctx* ctx, const float* d_kpts, const float* d_desc, const int32_t* d_n,
                         const float* h_size, const im_lightglue_conf* conf,
                         int32_t* d_matches, float* d_mscores, int32_t* d_prune, int32_t* d_info, void* stream);

/* The same for n_pairs independent pairs in ONE sequence of launches (a batch dimension over pairs inside every kernel):
 * image 2p / 2p + 1 of the inputs are pair p; all pairs share h_size (equal-shape tile pairs of an epoch, `matchers.py:367-394`;
 * the epochs of a sequence, `main_dev.py:60`). Needs im_ctx_reserve(max_images >= 2 n_pairs). Outputs: d_matches / d_mscores /
 * d_prune [2 n_pairs][max_kpts] (rows 2p, 2p + 1 = matches0, matches1 of pair p), d_info [n_pairs][4]. Results are
 * bit-identical to n_pairs single calls. */
int im_lightglue_forward_pairs(im_ctx* ctx, int n_pairs, const float* d_kpts, const float* d_desc, const int32_t* d_n,
                               const float* h_size, const im_lightglue_conf* conf, int32_t* d_matches, float* d_mscores,
                               int32_t* d_prune, int32_t* d_info, void* stream);

/* ---- SuperGlue: `SuperGlue.forward` (`SuperGlue/models/superglue.py:250-305`) ---------------------------
 * d_desc rows are [max_kpts][256] (the transposed view of the reference's [256, K]); h_shape: host [2][2] = (H, W)
 * of the image tensors (`data['image0'].shape`). Outputs as for LightGlue (d_info = {0, n0, n1, 0}). */
typedef struct {
    int sinkhorn_iterations; /* icepy4d default 20 (`matchers.py:857`) */
    double match_threshold;  /* icepy4d default 0.3 (`matchers.py:864`) */
    int n_layers;            /* 18 */
} im_superglue_conf;
int im_superglue_forward(im_ctx* ctx, const float* d_kpts, const float* d_scores, const float* d_desc,
                         const int32_t* d_n, const float* h_shape, const im_superglue_conf* conf,
                         int32_t* d_matches, float* d_mscores, int32_t* d_info, void* stream);

/* Match-table record of one pair for the sharded sequence driver (replaces the per-epoch bookkeeping of
 * `main_dev.py:160-173`): int32 [8 + 2 * max_kpts] = {epoch, n0, n1, n_matches, stop, 0, 0, 0}, matches0, scores0 bits. */
int im_pack_record(im_ctx* ctx, const int32_t* d_n, const int32_t* d_matches0, const float* d_mscores0,
                   const int32_t* d_info, int epoch, int32_t* d_record, void* stream);
/* n_pairs records at once from the outputs of im_lightglue_forward_pairs (epochs first_epoch .. first_epoch + n_pairs - 1);
 * d_records [n_pairs][8 + 2 * max_kpts]. With d_kpts != NULL (the [2 n_pairs][max_kpts][2] keypoints of im_superpoint_forward)
 * every record also carries the keypoints of both images as float32 bit patterns: d_records [n_pairs][8 + 6 * max_kpts]
 * (the 98 KB record of a sharded run whose gathered table must be self-contained; the reference keeps them in
 * `Epoch.features`, `main_dev.py:160-173`). */
int im_pack_records(im_ctx* ctx, int n_pairs, const int32_t* d_n, const int32_t* d_matches, const float* d_mscores,
                    const int32_t* d_info, int first_epoch, int32_t* d_records, const float* d_kpts, void* stream);
/* Copies an internal buffer of the last forward ("lg_x", "lg_cos", "lg_sin", "sim", "md", "sp_smap", "sp_nms") for
 * stage-level parity tests. Of the last assignment stage (im_assign_from_sim, or pair 0 of a matcher forward), as raw 32-bit
 * words counted in nfloats: "rmax", "rlog", "cmax", "clog", "rval" (float per row / column), "ridx" (int32 per row), "cbest"
 * (uint64 key per column = two words, low word first: ordered score bits << 32 | ~row), "lz" (log-sigmoid certainties
 * [2][max_kpts]); of im_superglue_forward's Sinkhorn potentials: "u" (m rows + dustbin), "v" (n columns + dustbin), "norm" (1). */
int im_debug_read(im_ctx* ctx, const char* name, float* d_dst, size_t nfloats, void* stream);
/* Measurement aid (no reference counterpart): the shader clock the two matrix-core kernel classes hold INSIDE their main loops. arm = 1: from
 * now on every attention launch (the matchers' self / cross blocks) and every Winograd convolution launch of this context has the first wave of
 * each block store the shader cycles and the 100 MHz reference ticks of its main loop into probe words nothing else reads; arm = 2: read,
 * stay armed; arm = 0: read and disarm. h_out[4] = {attention MHz (median over blocks), blocks, convolution MHz, blocks}. bench.py emits them
 * as `roofline.sustained_clock_mhz` (MI355X_MICROARCH.md, DVFS give-back item 6: cycles / reference ticks x 100 MHz). */
int im_debug_clock_probe(im_ctx* ctx, int arm, double* h_out, void* stream);
/* Debugging aid (no reference counterpart; GPU AddressSanitizer is unavailable on the MI355X pool): with IM_DEBUG_GUARDS=1 in the
 * environment when a context is created, every device buffer the library allocates (workspace of im_ctx_reserve, packed weights,
 * scratch) carries 256 bytes of guard words on both sides; they are compared by a small kernel at the end of every forward /
 * stage entry point, before a buffer is freed and in im_ctx_destroy. A changed word fails that call with -90 (im_last_error names
 * the buffer and the side) and is counted here: number of guard failures seen by this process so far (0 when the mode is off). */
int im_debug_guard_failures(void);
/* Self-test of that mode: issues one stray 4-byte store right behind the newest library buffer, expects the check to fail with
 * -90, restores the word. Returns 0 when the stray store was caught, -93 when the mode is off, -94 when it went unnoticed. */
int im_debug_guard_selftest(im_ctx* ctx, void* stream);
/* Compares the guard words now, from the host (0 when the mode is off or every word is intact, -90 otherwise). Forwards recorded into
 * a HIP graph carry no check of their own (a captured check would keep the buffer table of the capture): callers that replay graphs
 * call this after a replay. */
int im_debug_guards_check(im_ctx* ctx, void* stream);

/* ---- stage entry points (what the stage-isolated parity tests call; also usable on their own) ----------- */
/* C[m][n] = alpha * (sum_k A[m][k] W[n][k] + bias[n]); fp32 GEMM. bias may be NULL. big_tile bit 0: 128x128 tiles; bit 1: the product on
 * the bf16 matrix cores with fp32 accuracy (operands cut into three bf16 values, six products per fp32 product) instead of the f32-input MFMA. */
int im_gemm_nt(im_ctx* ctx, const float* d_a, const float* d_w, const float* d_bias, float* d_c,
               int m, int n, int k, float alpha, int big_tile, void* stream);
/* The feed-forward tail of a transformer block / GNN layer in one kernel:
 *   x[z][m][0..256) += W3 . act(W0 . [x[z][m] | att[z][m]] + b0) + b3   for the first d_n[z] (NULL: n_rows) rows of each image z
 * act 0: gelu(layernorm(.)) = LightGlue's ffn (`lightglue/lightglue.py:144-149, 160-162, 212-216`); act 1: relu(.) = SuperGlue's
 * mlp with its BatchNorm folded into W0 / b0 (`SuperGlue/models/superglue.py:51-61, 104-116`; h_ln_g / h_ln_b unused, may be NULL).
 * d_x / d_att: [n_images][n_rows][256]; weights on the HOST in torch layout (W0 [512][512] acting on cat([x, att]), b0 [512],
 * LayerNorm g / b [512], W3 [256][512], b3 [256]): packed + uploaded inside; synchronises. */
int im_ffn_fused(im_ctx* ctx, int act, float* d_x, const float* d_att, const float* h_w0, const float* h_b0, const float* h_ln_g,
                   const float* h_ln_b, const float* h_w3, const float* h_b3, int n_images, int n_rows, const int32_t* d_n, void* stream);
/* 3x3 conv, NHWC fp32, weights in torch layout [cout][cin][3][3] on the HOST (packed + uploaded inside; synchronises) */
int im_conv3x3(im_ctx* ctx, const float* d_in, const float* h_weight, const float* h_bias, float* d_out,
               int b, int h, int w, int cin, int cout, int relu, int pool, void* stream);
/* the same convolution in Winograd F(2x2, 3x3) form (2.25x fewer matrix-core FLOPs; what the forward pass uses) */
int im_conv3x3_winograd(im_ctx* ctx, const float* d_in, const float* h_weight, const float* h_bias, float* d_out,
                        int b, int h, int w, int cin, int cout, int relu, int pool, void* stream);
/* fp32 flash attention: q, k, v [batch][heads][n_max][64]; out [batch][n_max][heads*64]; cross bit 0: kv of image z^1; bit 1: the kernel on the
 * f32-input MFMA (rounds 1-5) instead of the bf16-plane kernel, for A/B; bit 2: the bf16-plane kernel cuts K / V itself while it stages them
 * (the form for callers without the plane workspace) instead of reading the planes of its first launch */
int im_flash_attn(im_ctx* ctx, const float* d_q, const float* d_k, const float* d_v, float* d_out,
                  const int32_t* d_n, int n_max, int batch, int heads, int cross, float scale, void* stream);
/* The head of one LightGlue block as the forward pass launches it: the K = 256 projection of d_x [2 n_pairs][n_max][256], the K / V planes of the
 * attention, and - d_att not NULL - the attention into d_att [2 n_pairs][n_max][256]. cross 0: h_w [768][256] = Wqkv, rotary with d_cs / d_sn
 * [2 n_pairs][n_max][32] (NULL: none), q / k / v; cross 1: h_w [512][256] = [to_qk ; to_v], d_q = alpha * qk (query of its own image, key of the
 * other one), d_v. d_q / d_k / d_v: [2 n_pairs][4][n_max][64] fp32; d_planes: 2 * 2 n_pairs * 4 * n_max * 384 bytes,
 * [K | V][image][head][row][3 planes][64] bf16. By default the projection writes q and the planes and leaves d_k (and d_v) alone; with
 * IM_PROJ_ROWS32=1 / IM_PROJ_TILED=1 it writes fp32 q / k / v and a pass of its own cuts the planes: same bits. d_n [n_pairs][2]: live rows per
 * image; d_active (NULL: all) [n_pairs][2]: a pair whose first int is 0 is skipped. Rows at or past the live count are never written. Weights
 * on the HOST (packed + uploaded inside; synchronises). */
int im_block_proj_attn(im_ctx* ctx, int cross, const float* d_x, const float* h_w, const float* h_bias, const float* d_cs, const float* d_sn,
                       float alpha, const int32_t* d_n, const int32_t* d_active, int n_pairs, int n_max, float* d_q, float* d_k, float* d_v,
                       void* d_planes, float* d_att, float scale, void* stream);
/* `simple_nms` (`lightglue/superpoint.py:50-65`): d_scores, d_out [n_images][h][w] */
int im_nms(im_ctx* ctx, const float* d_scores, float* d_out, int n_images, int h, int w, int radius, void* stream);
/* border / threshold / row-major compaction / top-k (`lightglue/superpoint.py:177-200`) on an NMS map */
int im_select_topk(im_ctx* ctx, const float* d_nms, int n_images, int h, int w, int border, float threshold,
                   int max_kpts, float* d_kpts, float* d_scores, int32_t* d_n, void* stream);
/* `sample_descriptors` (`lightglue/superpoint.py:75-87`) incl. the dense per-cell L2 normalisation (`:205`):
 * d_dense_raw = convDb output, NHWC [n_images][hc][wc][256]; d_desc [n_images][max_kpts][256] */
int im_sample_descriptors(im_ctx* ctx, const float* d_dense_raw, int n_images, int hc, int wc,
                          const float* d_kpts, const int32_t* d_n, float* d_desc, void* stream);
/* `sigmoid_log_double_softmax` + `filter_matches` (`lightglue/lightglue.py:253-306`) on a given similarity matrix:
 * d_sim [m][ld], d_z0 [m], d_z1 [n] -> d_matches [2][max(m,n)] int32 etc. (compact index space) */
int im_assign_from_sim(im_ctx* ctx, const float* d_sim, int m, int n, int ld, const float* d_z0, const float* d_z1,
                       float threshold, int32_t* d_m0, int32_t* d_m1, float* d_ms0, float* d_ms1, void* stream);
/* `log_optimal_transport` (`SuperGlue/models/superglue.py:152-186`): d_scores [m][ld] -> d_out [(m+1)][(n+1)] */
int im_log_optimal_transport(im_ctx* ctx, const float* d_scores, int m, int n, int ld, float bin_score, int iters,
                             float* d_out, void* stream);

/* ---- Gaussian pyramid steps on uint8 images [n_images][h][w][channels] (channels interleaved, 1..4), what `Quality` resizing and
 * tile preselection call through OpenCV in the reference (`cv2.pyrDown` / `cv2.pyrUp`, `matchers.py:529-530, 599-609`):
 * im_pyr_down -> [n_images][(h + 1) / 2][(w + 1) / 2][channels], im_pyr_up -> [n_images][2 h][2 w][channels]. Enqueue only. */
int im_pyr_down(im_ctx* ctx, const uint8_t* d_in, uint8_t* d_out, int n_images, int h, int w, int channels, void* stream);
int im_pyr_up(im_ctx* ctx, const uint8_t* d_in, uint8_t* d_out, int n_images, int h, int w, int channels, void* stream);

/* ---- tile mode (`ImageMatcherBase._match_by_tile`, `matchers.py:304-469`) -----------------------------------------------
 * The tail of the tile loop for ALL tile pairs of an image pair in one call (`matchers.py:402-448`): valid matches of every
 * pair are shifted to image coordinates ((kpt + tile origin) + image origin, fp32), concatenated in tile-pair order, and
 * `np.unique(mkpts0, axis=0, return_index=True)` is applied: rows in lexicographic (x, y) order, first occurrence kept.
 *   d_matches [n_pairs][max_kpts] int32 : matches0 of every tile pair (-1 = none), rows = keypoints of its first tile
 *   d_slots   [n_pairs][2] int32        : which entry of the feature bank holds tile 0 / tile 1 of the pair
 *   d_off     [n_pairs][4] float        : (x, y) origin of tile 0 and of tile 1 in their images (`lim0[0:2]`, `lim1[0:2]`)
 *   h_origin  [4] float (host)          : `t0_origin`, `t1_origin`
 *   d_kp_bank [n_tiles][max_kpts][2], d_n_bank [n_tiles] : keypoints and keypoint counts of every extracted tile
 * Outputs (capacity n_pairs * max_kpts rows): d_count = number of unique rows S; d_idx0 / d_idx1 [S] = flat bank row
 * (tile * max_kpts + keypoint) of each surviving match in image 0 / 1 (for im_gather_rows on descriptors and scores);
 * d_kp0 / d_kp1 [S][2] = the matched points in image coordinates. Enqueues only. */
int im_merge_tile_matches(im_ctx* ctx, int n_pairs, int max_kpts, const int32_t* d_matches, const int32_t* d_slots, const float* d_off,
                          const float* h_origin, const float* d_kp_bank, const int32_t* d_n_bank, int32_t* d_count, int32_t* d_idx0,
                          int32_t* d_idx1, float* d_kp0, float* d_kp1, void* stream);
/* d_dst[r][:] = d_src[d_idx[r]][:] for r < n, rows of row_floats floats (descriptor / score banks -> matched features). */
int im_gather_rows(im_ctx* ctx, const float* d_src, int row_floats, const int32_t* d_idx, int n, float* d_dst, void* stream);

/* Fundamental-matrix RANSAC over matched keypoints (`src/icepy4d/matching/geometric_verification.py:11-102`, which
 * calls pydegensac / cv2 USAC_MAGSAC on the CPU): n_hyp seeded 8-point hypotheses scored by Sampson error in parallel.
 * d_p0, d_p1 [n][2] float (x, y); d_F [9] double = matrix of the best hypothesis (unit Frobenius norm); d_mask [n] uint8
 * its inliers; d_info {inlier count, hypothesis index}. When the best count is 0 (every sample degenerate, e.g. duplicated or
 * collinear correspondences), d_info = {0, 0}, d_F = 0 and the mask is all false. The least-squares refit on the inliers is left
 * to the caller. */
int im_ransac_fundamental(im_ctx* ctx, const float* d_p0, const float* d_p1, int n, int n_hyp, double threshold,
                          unsigned int seed, double* d_F, uint8_t* d_mask, int32_t* d_info, void* stream);

/* Relative orientation, device stage (replaces the RANSAC inside `cv2.findEssentialMat`, `src/icepy4d/sfm/geometry.py:64-66`):
 * like im_ransac_fundamental on NORMALISED image coordinates (d_x0, d_x1 [n][2] float), every 8-point hypothesis projected onto
 * the essential manifold (two equal singular values, one zero) before it is scored; d_E [9] double = the best hypothesis
 * (x1^T E x0 = 0, unit Frobenius norm), d_mask / d_info as above (also when no hypothesis is valid, a failed projection
 * included: d_info = {0, 0}, d_E = 0, no inlier). The cheirality test (`cv2.recoverPose`, `geometry.py:70-75`)
 * and the 5-7 correspondence case (five-point solver) stay on the host: one 3 x 3 matrix. */
int im_ransac_essential(im_ctx* ctx, const float* d_x0, const float* d_x1, int n, int n_hyp, double threshold,
                        unsigned int seed, double* d_E, uint8_t* d_mask, int32_t* d_info, void* stream);

/* Linear two-view triangulation of n points on the device (replaces the per-point Python loop of
 * `src/icepy4d/sfm/triangulation.py:153-186`): h_P0, h_P1 = the two 3 x 4 projection matrices (row-major doubles in HOST
 * memory), d_x0, d_x1 [n][3] double homogeneous image points, d_X [n][4] double = homogeneous points normalised to X[3] = 1.
 * The reference's formulation (unknowns X and one depth per view, 6 x 6 system per point, right singular vector of the smallest singular
 * value): equal to the reference's outputs within 1e-9 relative (tests/golden/g10_triangulation.npz). n = 0 enqueues nothing, and
 * d_x0 / d_x1 / d_X may then be null. */
int im_triangulate_linear(im_ctx* ctx, const double* h_P0, const double* h_P1, const double* d_x0, const double* d_x1, int n,
                          double* d_X, void* stream);

/* ---- template matching: orientation correlation (`src/icepy4d/matching/templatematch.py`) ---------------------------------
 * im_forient replaces `forient` (`templatematch.py:332-340`): d_img [n_images][h][w] of dtype 0 = uint8, 1 = float32; d_out
 * [n_images][h][w] float2 (re, im) = the 3 x 3 complex gradient with zero padding, divided by its modulus (0 -> 1). Enqueue only. */
int im_forient(im_ctx* ctx, const void* d_img, int dtype, int n_images, int h, int w, float* d_out, void* stream);
/* Replaces the per-point loop of `OC` (`templatematch.py:258-329`) for many (point, B image) pairs against ONE A map in one call.
 *   d_a [ha][wa] float2: orientation map of A;  d_b [n_b][hb][wb] float2: orientation maps of the B images
 *   d_pairs [n_pairs][4] double: u, v, initialdu, initialdv;  d_bidx [n_pairs] int32: the B image of every pair
 *   T, S: template / search width (1 <= T < S);  conj_b: the reference's `B = np.conj(B)` was applied (1) or not (0)
 *   d_out [6][n_pairs] double: pu, pv (the centres used), du, dv, peakCorr, meanAbsCorr; NaN wherever the reference leaves NaN, which
 *   includes every pair whose T x T template or S x S search window holds a NaN or an infinity (its FFT spreads it over all of C).
 * C = Re(corr(A window, conj B window)) over the (S - T)^2 valid offsets is computed directly in fp32. Enqueue only. */
int im_template_match_oc(im_ctx* ctx, const float* d_a, int ha, int wa, const float* d_b, int n_b, int hb, int wb, const double* d_pairs,
                         const int32_t* d_bidx, int n_pairs, int T, int S, int conj_b, double* d_out, void* stream);
/* The block C of im_template_match_oc itself, for tests: the same inputs, the same kernel and plan, written to d_c [n_pairs][S - T][S - T]
 * float instead of the library's scratch. The plane of a pair that the reference does not correlate is left untouched. The sums are raw:
 * the rule that a NaN or an infinity in either window of a pair turns that pair's du, dv, peakCorr and meanAbsCorr into NaN belongs to
 * im_template_match_oc alone. Both refuse bad arguments with -72. Enqueue only. */
int im_template_match_corr(im_ctx* ctx, const float* d_a, int ha, int wa, const float* d_b, int n_b, int hb, int wb, const double* d_pairs,
                           const int32_t* d_bidx, int n_pairs, int T, int S, int conj_b, float* d_c, void* stream);

/* ---- DSM and orthophoto rasters (`src/icepy4d/utils/dsm_orthophoto.py`, `sfm/interpolate_colors.py`, `sfm/geometry.py`) ------------
 * The binning of `build_dsm` (`dsm_orthophoto.py:40-81`) in two calls around three stable sorts done by the caller:
 * im_dsm_round replaces `round_to_val` (`:39-40`, `:64-66`): d_pts [n][3] float64; d_xr / d_yr [n] float32 = rint(x / step) * step in
 * float32 (half to even); sort keys [n] int64 whose ascending order is the value order with -0.0 == 0.0: d_xykey of (x_r, y_r),
 * d_ykey of y_r, d_zkey of z (NaN last, all NaN equal). Enqueue only.
 * The caller forms the reference's `np.lexsort((y_r, z))` order (`:69-70`) as d_perm_b = stable sorts by d_ykey, then by d_zkey, and
 * the group order as d_perm_c = d_perm_b stably sorted by d_xykey.
 * im_dsm_group_mean replaces `df.groupby(["x_round", "y_round"]).mean()` (`:73-81`): d_bx / d_by / d_bz [n] float32 (capacity n) get
 * the groups in ascending (x, y), z the Kahan mean of the group's non-NaN z in ascending-z order (pandas' group_mean; NaN when there
 * is none); *d_n_groups the number of groups. A key of zero keeps the sign of its first row in d_perm_b order. Enqueue only. */
int im_dsm_round(im_ctx* ctx, const double* d_pts, long long n, float step, float* d_xr, float* d_yr, long long* d_xykey,
                 long long* d_ykey, long long* d_zkey, void* stream);
int im_dsm_group_mean(im_ctx* ctx, const double* d_pts, const float* d_xr, const float* d_yr, const long long* d_xykey,
                      const long long* d_perm_b, const long long* d_perm_c, long long n, float* d_bx, float* d_by, float* d_bz,
                      long long* d_n_groups, void* stream);
/* Replaces `LinearNDInterpolator(...)(grid_x, grid_y)` of `build_dsm` (`:85-96`) once qhull has triangulated the binned points on the
 * host: d_simplices [T][3] int32 and d_transform [T][3][2] float64 are scipy's `Delaunay.simplices` / `.transform`, h_bounds its
 * min_bound (x, y) and max_bound (x, y); d_xq [nx] / d_yq [ny] the grid axes (np.arange), xq[c] == x0 + c * dx. Every cell takes the
 * lowest-index simplex that contains it (scipy's inside test, eps = 100 DBL_EPSILON) and z = ((0 + c0 v0) + c1 v1) + c2 v2 with
 * v = float64 of d_bz; cells in none get `fill`. d_z [ny][nx] float64. T below 0x7f7f7f7f, the mark of a cell without a triangle
 * (-72 from there upward). Scratch from the context. Enqueue only. */
int im_dsm_rasterize(im_ctx* ctx, const float* d_bx, const float* d_by, const float* d_bz, const int32_t* d_simplices,
                     const double* d_transform, long long n_simplices, const double* h_bounds, const double* d_xq, int nx,
                     const double* d_yq, int ny, double x0, double dx, double y0, double dy, double fill, double* d_z, void* stream);
/* Replaces `project_points` (`sfm/geometry.py:79-100`: cv2.projectPoints, restated in float64) and `interpolate_point_colors` /
 * `bilinear_interpolate` (`sfm/interpolate_colors.py:13-92`), and the colouring of `generate_ortophoto` (`dsm_orthophoto.py:176-211`).
 * Items (r, c) of a rows x cols table; coordinate plane P has element (r, c) at d_P[r * sPr + c * sPc]. cells = 1: a NaN z is an
 * invalid cell (black in d_ortho). h_cam [28] float64: fx, fy, cx, cy, R (9, row-major), t (3), k1 k2 p1 p2 k3 k4 k5 k6 s1..s4 (zeros
 * where absent). d_img [h][w][cin] uint8; output channel ch samples image channel h_chmap[ch] (0 <= cout <= 4, whatever is asked for) as float32(v) / 255.
 * Outputs, each optional: d_proj [n][2] float32 projections, d_col [n][cout] float64 colours (the float64 sum of the reference),
 * d_ortho [n][3] uint8 = np.uint8(float32(colour) * 255). Enqueue only. */
int im_project_colors(im_ctx* ctx, const double* d_x, long long sxr, long long sxc, const double* d_y, long long syr, long long syc,
                      const double* d_z, long long szr, long long szc, int rows, int cols, int cells, const double* h_cam,
                      const unsigned char* d_img, int h, int w, int cin, const int32_t* h_chmap, int cout, float* d_proj,
                      double* d_col, unsigned char* d_ortho, void* stream);

/* ---- reconstruction of matched points (`src/icepy4d/sfm/geometry.py`: `undistort_points`; `thirdparty/triangulation.py`:
 * `iterative_LS_triangulation`, `linear_LS_triangulation`; `sfm/triangulation.py`: `Triangulate`); csrc/sfm.hip ---------------------
 * A camera's h_cam is [12] float64 in HOST memory: fx, fy, cx, cy, k1 k2 p1 p2 k3 k4 k5 k6 (zeros where absent); a projection matrix
 * h_P is 3 x 4 row-major float64 in HOST memory. One thread per point, float64, the operations of tests/sfm_oracle.py. Enqueue only.
 *
 * im_undistort_points restates cv2.undistortPoints(pts, K, dist, None, K) with the default criteria: x0 = (u - cx) / fx, five
 * fixed-point iterations of the Brown / rational model (OpenCV's icdist < 0 guard falls back to x0, y0), fx x + cx, float32.
 * d_pts, d_out [n][2] float32. */
int im_undistort_points(im_ctx* ctx, const float* d_pts, long long n, const double* h_cam, float* d_out, void* stream);
/* n point pairs d_u1, d_u2 [n][2] (float32, or float64 with f64 = 1) and one camera pair -> d_X [n][3] float64, d_status [n] int32.
 * The reference's recurrence: at most max_solves (1..10) least-squares solves of the 4 x 3 system (one-sided Jacobi SVD, singular
 * values <= 2 DBL_EPSILON * their sum treated as zero, as cv2.solve(DECOMP_SVD)), cumulative re-weighting by 1 / depth, stop when
 * both depths move by <= tolerance (absolute). status = (d1 > 0 and d2 > 0) - (d1 <= 0) - 2 (d2 <= 0): 1, -1, -2 or -3 (0 only for a
 * NaN depth; the reference's documented 0 for non-convergence cannot occur). max_solves = 1 is `linear_LS_triangulation`: status 1.
 * h_cam1 and h_cam2 both given (float32 points only): the points are undistorted first, in the same launch, and rounded to float32
 * as `undistort_points` returns them; d_und1 / d_und2 [n][2] float32 (optional) receive the points the triangulation used. */
int im_triangulate_iterative(im_ctx* ctx, const void* d_u1, const void* d_u2, int f64, long long n, const double* h_P1,
                             const double* h_P2, const double* h_cam1, const double* h_cam2, double tolerance, int max_solves,
                             double* d_X, int32_t* d_status, float* d_und1, float* d_und2, void* stream);
/* The same for every record of a gathered match table (`sequence.py`: d_table int32 [n_records][8 + 6 max_kpts] with the keypoint
 * payload; word [3] = n_matches, -1 for a failed pair = no points; matches0 at word 8, keypoints0 at 8 + 2K, keypoints1 at 8 + 4K).
 * d_cams [n_cams][2][24] float64 in DEVICE memory, n_cams = n_records or 1: per camera P (12), fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6.
 * d_offsets [n_records + 1] int64 = exclusive scan of max(n_matches, 0) (always written; with m_cap = 0 nothing else is). Record e
 * fills rows d_offsets[e] .. d_offsets[e + 1] - 1 of d_X [m_cap][3], d_status [m_cap] and (optional) d_und0 / d_und1 [m_cap][2] with
 * its matched keypoints in ascending keypoint-0 index (the reference's `kpts0[matches0 > -1]` order). Rows >= m_cap are dropped (the
 * caller compares d_offsets[n_records] with m_cap); a record with fewer valid matches0 entries than n_matches leaves the remaining
 * rows NaN with status 0. max_kpts <= 16384 (the compaction uses 4 max_kpts bytes of LDS). */
int im_triangulate_table(im_ctx* ctx, const int32_t* d_table, int n_records, int max_kpts, const double* d_cams, int n_cams,
                         int undistort, double tolerance, int max_solves, long long m_cap, long long* d_offsets, double* d_X,
                         int32_t* d_status, float* d_und0, float* d_und1, void* stream);

/* ---- velocity fields (`src/icepy4d/utils/binned_stats.py`: `compute_binned_stats2D`, `compute_binned_stats3D` over
 * `scipy.stats.binned_statistic_2d / _dd`; `utils/tracking_features_utils.py`: `tracked_points_time_series`, `tracked_dict_to_df`);
 * csrc/binned.hip. float64, the reference's operations in the reference's order: outputs are bit-identical (tests/golden/g14_velocity.npz).
 *
 * im_binned_cells restates scipy's `_bin_numbers` (`_binned_statistic.py:766-795`) for dims = 1..3: d_pts [n][dims]; d_edges = the edge
 * arrays one behind the other, h_n_edges[d] doubles each, ascending (`bins_from_nodes`: `binned_stats.py:12-31`, `:197-221`). Per
 * dimension b = np.digitize(x, edges) (a search over the edge doubles; NaN beyond the last edge), one bin to the left when
 * x >= edges[-1] and np.around(x, decimal) == np.around(edges[-1], decimal), with h_scale[d] = 10 ** |decimal| and h_mode[d] = sign of
 * decimal (np.around multiplies, rounds and divides for decimal > 0, divides first for decimal < 0). The call carries n_sets point sets
 * that share the edges: set e = rows d_offsets[e] .. d_offsets[e + 1] - 1 (d_offsets [n_sets + 1] int64, from 0 to n). d_key [n] int64 =
 * set * cells + cell (row-major over the dimensions) for a point inside in every dimension, n_sets * cells otherwise. Enqueue only.
 * The caller sorts d_key stably (values -> d_sorted_key, indices -> d_perm): every cell is then a segment of points in input order.
 * im_binned_stats replaces the statistics of `binned_statistic_dd` (`:596-647`) for n_values columns d_values [n_values][n] at once.
 * h_slots [7] int32 in the order count, sum, mean, std, min, max, median: the plane of d_out [planes][n_sets][n_values][cells] that
 * receives the statistic, or -1. count and sum fill empty cells with 0, the others with NaN. sum adds in input order from +0.0
 * (np.bincount), std = sqrt(sum((v - sum / count)^2) / count) in the same order, min ignores NaN, max is NaN when the cell holds one,
 * median = (a[(n - 1) / 2] + a[n / 2]) / 2 of the values sorted as numbers (-0.0 == 0.0, NaN last, ties to the lower input index).
 * Cells of up to im_binned_lds_capacity() points are selected in LDS, larger ones from global memory; both are exact. Scratch from the
 * context. Enqueue only. */
int im_binned_lds_capacity(void);
int im_binned_cells(im_ctx* ctx, const double* d_pts, long long n, int dims, const double* d_edges, const int32_t* h_n_edges,
                    const double* h_scale, const int32_t* h_mode, const long long* d_offsets, int n_sets, long long* d_key, void* stream);
int im_binned_stats(im_ctx* ctx, const long long* d_sorted_key, const long long* d_perm, long long n, int n_sets, long long cells,
                    const double* d_values, int n_values, const int32_t* h_slots, double* d_out, void* stream);
/* The table of `tracked_dict_to_df` (`tracking_features_utils.py:219-300`) from the series of `tracked_points_time_series` (`:123-169`).
 * The epochs' rows are concatenated: epoch e = rows d_offsets[e] .. d_offsets[e + 1] - 1 of d_xyz [n_rows][3] (and of every camera's
 * d_image_points [n_cams][n_rows][2], optional); the caller sorts the track ids stably (d_sorted_ids, d_perm), which orders them by
 * (id, epoch). d_days [n_epochs] int64 day numbers. Per id: the epochs in which it occurs, inside h_volume (min x y z, max x y z,
 * inclusive, `geospatial.py:113-117`; null = no volume); tracked when there are at least max(1, min_tracked_epochs); ini / fin = the
 * first / last of them; d = fin - ini, dt = day_fin - day_ini, v = d / (double)dt, V = sqrt((vx vx + vy vy) + vz vz). Rows are kept
 * when dt >= *h_min_dt (null = no bound) and lo <= v < hi on every axis whose h_vlims [3][2] lo is not NaN, compacted in ascending id.
 * d_int_cols [6][n_rows] int64: fid, num_tracked_eps, ep_ini, ep_fin (epoch indices), dt, the row's index among the tracked ids (the
 * DataFrame's index); d_f64_cols [13 + 4 n_cams][n_rows]: X_ini Y_ini Z_ini X_fin Y_fin Z_fin dX dY dZ vX vY vZ V, then per camera
 * x_ini y_ini x_fin y_fin. d_member [n_rows] uint8: the input row belongs to the series of a tracked id. *d_n_rows: rows kept. An id
 * occurs at most once per epoch (the caller checks). Scratch from the context. Enqueue only. */
int im_tracked_points(im_ctx* ctx, const long long* d_sorted_ids, const long long* d_perm, long long n_rows, const long long* d_offsets,
                      int n_epochs, const double* d_xyz, const long long* d_days, const double* h_volume, long long min_tracked_epochs,
                      const long long* h_min_dt, const double* h_vlims, const double* d_image_points, int n_cams, long long* d_int_cols,
                      double* d_f64_cols, unsigned char* d_member, long long* d_n_rows, void* stream);

/* ---- image stabilisation (`src/icepy4d/sfm/geometry.py`: `undistort_image`; `utils/homography.py`: `homography_warping`); csrc/warp.hip.
 * The reference calls cv2.undistort(src, K, dist, None, K) and cv2.warpPerspective(src, H, (w, h)) on 8-bit images; both are restated
 * here as OpenCV documents its 8-bit INTER_LINEAR path with BORDER_CONSTANT 0: a float64 source coordinate per output pixel, rounded
 * to 1/32 pixel (ties to even), four taps with integer weights that sum to 32768, (sum + 16384) >> 15 (csrc/warp_pixel.h,
 * tests/warp_oracle.py: bit-identical; parity with an OpenCV binary is not pinned). Images are [n_images][h][w][channels] uint8 in
 * DEVICE memory, channels interleaved and independent. One thread per output pixel. Enqueue only.
 * im_undistort_image: one camera for all images, h_cam [21] float64 in HOST memory = the inverse of K (9, row-major, by cofactors),
 * fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6 (zeros where absent); d_dst has the shape of d_src.
 * im_warp_perspective: d_minv [n_images][9] float64 in DEVICE memory, the INVERSE of every image's homography (output -> source,
 * row-major); d_dst [n_images][oh][ow][channels]. A pixel whose homogeneous w is exactly 0 samples source pixel (0, 0), as OpenCV does.
 * Both return -74 for a null pointer, source and destination ranges that overlap, channels outside 1..4, a side (h, w, oh, ow) outside
 * 1..32766 or n_images outside 1..65535. */
int im_undistort_image(im_ctx* ctx, const uint8_t* d_src, int n_images, int h, int w, int channels, const double* h_cam, uint8_t* d_dst,
                       void* stream);
int im_warp_perspective(im_ctx* ctx, const uint8_t* d_src, int n_images, int h, int w, int channels, const double* d_minv, int oh, int ow,
                        uint8_t* d_dst, void* stream);

/* ---- point-cloud neighbourhoods (`src/icepy4d/core/point_cloud.py`: `PointCloud.sor_filter`; `post_processing/open3d_fun.py`:
 * `MeshingPoisson.SOR`, `estimate_normals`); csrc/knn.hip, csrc/knn_point.h. The exact k nearest neighbours of every point of a cloud
 * within the same cloud, through a uniform grid: origin = the cloud's minimum corner, cubic cells of side s, nx x ny x nz cells,
 * h_grid [4] float64 in HOST memory = origin x y z, s. The cell of a point is min(n_a - 1, floor((p_a - o_a) / s)) per axis, its key
 * (iz * ny + iy) * nx + ix. float64, d2 = ((dx*dx) + (dy*dy)) + (dz*dz), no fused operations (tests/knn_oracle.py: bit-identical).
 * The grid must hold the whole cloud (a point outside is clamped into it: memory-safe, but the neighbours are then not guaranteed).
 * im_knn_max_cells: the largest nx * ny * nz accepted (2^24).
 * im_knn_cells: d_pts [n][3] float64 -> d_key [n] int64. The caller sorts the keys (stable) and hands the sorted keys and the
 * permutation (sorted position -> original index) to the next two calls.
 * im_knn_cell_ranges: d_sorted_keys [n] -> d_start [cells + 1] int32, the first sorted position of every cell (d_start[cells] = n).
 * im_knn_self: for every point the k (1..64) nearest points of the cloud, itself included at distance 0, ascending by d2, the lower
 * original index first among equal distances (which also decides who is kept at the k-th place). radius2 = +inf: plain search;
 * otherwise a neighbour is dropped iff d2 > radius2 (Open3D's hybrid search). Outputs, each may be NULL, all addressed by ORIGINAL point
 * index: d_count [n] int32 (min(k, n), fewer under a radius), d_idx [n][k] int32 and d_d2 [n][k] float64 (unused slots -1 / +inf),
 * d_mean [n] float64 = (sum of sqrt(d2_j), j ascending, from 0.0) / (double)count, -1.0 for count 0 (the statistic of statistical outlier
 * removal), d_normal [n][3] float64 = unit eigenvector of the smallest eigenvalue of the two-pass covariance of the neighbours (cyclic
 * Jacobi; first non-zero of (n_z, n_y, n_x) positive; (0, 0, 1) for count < 3), d_rings [n] int32 = rings of cells visited, the query's cell counted (statistics);
 * negated when the rings had cost more than 1024 + n / 32 steps of 64 rows or candidates and the search ended by one scan of the whole
 * cloud instead, which bounds the work of a query far from everything whatever the grid.
 * One wave per query; the cloud in cell order lives in scratch of the context. Enqueue only.
 * All three return -75, without launching, for a null required pointer (d_pts, d_key; d_sorted_keys, d_start; d_pts, d_perm, d_start,
 * h_grid), n < 0 or n >= 2^31, k outside 1..64, s or an origin coordinate non-finite or s <= 0, a grid dimension below 1, more cells
 * than im_knn_max_cells(), radius2 negative or NaN. n == 0 returns 0 and launches nothing. */
int im_knn_max_cells(void);
int im_knn_cells(im_ctx* ctx, const double* d_pts, long long n, const double* h_grid, int nx, int ny, int nz, long long* d_key, void* stream);
int im_knn_cell_ranges(im_ctx* ctx, const long long* d_sorted_keys, long long n, long long cells, int32_t* d_start, void* stream);
int im_knn_self(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid, int nx,
                int ny, int nz, int k, double radius2, int32_t* d_count, int32_t* d_idx, double* d_d2, double* d_mean, double* d_normal,
                int32_t* d_rings, void* stream);

/* ---- geometric features of the ball around every point (`scripts/pcd_postprocessing/top_border.py`: CloudCompare's
 * `computeFeature(Linearity, 2.0)` and `computeFeature(Verticality, 0.15)`); csrc/ballfeat.hip, csrc/ball_point.h. CloudCompare is not a
 * dependency: the features have a definition of their own (tests/ball_oracle.py: bit-identical); PARITY WITH A CLOUDCOMPARE
 * BINARY IS UNPINNED. The grid, d_perm and d_start are those of the k-NN above (the same three calls prepare them).
 * The neighbours of point q are the points p of the cloud, q included, with d2(q, p) <= fl(radius * radius). Each offset component
 * fl(p - q) is quantised to the integer rint(u / h), h = radius * 2^-18, clamped to +-(2^18 + 1); ten exact int64 sums per query
 * (count, Sx Sy Sz, Sxx Sxy Sxz Syy Syz Szz) are therefore a function of the input alone, whatever the grid and the order of accumulation.
 * Covariance in quantised units in float64 (m_a = S_a / count, c_ab = S_ab / count - m_a m_b, no fused operations), eigenvalues by cyclic
 * Jacobi, descending, negative ones 0.0, scaled by h * h to squared metres; the normal is the unit eigenvector of the smallest one with the
 * first non-zero of (n_z, n_y, n_x) positive. count < 3 or the largest eigenvalue 0 gives NaN for eig, normal and every feature.
 * Outputs, each may be NULL, all addressed by ORIGINAL point index: d_count [n] int32, d_sums [n][10] int64, d_eig [n][3] float64,
 * d_normal [n][3] float64, d_feat [n][n_kinds] float64 (column j = the feature h_kinds[j], HOST memory, codes below; d_feat may be NULL only
 * with n_kinds 0 or as an unwanted output), d_steps [n] int32 = the steps of 64 rows looked up or 64 candidates read that the query took,
 * negated where the box of cells would have cost more row lookups than 1024 + n / 32 and the whole sorted cloud was scanned instead.
 * One wave per query; the cloud in cell order lives in scratch of the context (shared with im_knn_self). Enqueue only.
 * Returns -75, without launching, for a null required pointer (d_pts, d_perm, d_start, h_grid; h_kinds when n_kinds > 0), n < 0 or
 * n > 2^26, a radius that is not finite and positive or whose h is not a normal number, a grid im_knn_self refuses, n_kinds outside 0..16,
 * an unknown kind. n == 0 returns 0 and launches nothing. */
enum im_ball_kind {
    IM_BALL_EIGENVALUES_SUM = 0,      /* (l1 + l2) + l3 */
    IM_BALL_PCA1 = 1,                 /* l1 / sum */
    IM_BALL_PCA2 = 2,                 /* l2 / sum */
    IM_BALL_SURFACE_VARIATION = 3,    /* l3 / sum */
    IM_BALL_LINEARITY = 4,            /* (l1 - l2) / l1 */
    IM_BALL_PLANARITY = 5,            /* (l2 - l3) / l1 */
    IM_BALL_ANISOTROPY = 6,           /* (l1 - l3) / l1 */
    IM_BALL_SPHERICITY = 7,           /* l3 / l1 */
    IM_BALL_VERTICALITY = 8,          /* 1 - |n_z| */
    IM_BALL_EIGENVALUE1 = 9,
    IM_BALL_EIGENVALUE2 = 10,
    IM_BALL_EIGENVALUE3 = 11,
    IM_BALL_NUMBER_OF_NEIGHBORS = 12, /* (double)count */
    IM_BALL_KINDS = 13
};
int im_ball_features(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid,
                     int nx, int ny, int nz, double radius, const int32_t* h_kinds, int n_kinds, int32_t* d_count, long long* d_sums,
                     double* d_eig, double* d_normal, double* d_feat, int32_t* d_steps, void* stream);

/* ---- distances between two clouds (CloudCompare's cloud-to-cloud distance and M3C2, Lague et al. 2013; Open3D's
 * `compute_point_cloud_distance`); csrc/cloud_distance.hip, csrc/cyl_point.h, csrc/knn_list.h. Neither tool is a dependency and the
 * reference calls neither: every quantity has a definition of its own (tests/cloud_distance_oracle.py: bit-identical); PARITY
 * WITH A CLOUDCOMPARE OR OPEN3D BINARY IS UNPINNED. The three query calls ask a TARGET cloud, given exactly as to the ball features (d_pts,
 * d_perm, d_start, n, h_grid, nx, ny, nz, prepared by the k-NN's three calls above), at m external queries d_q [m][3] float64. A query may
 * lie anywhere, far outside the target's grid included: its cell is clamped into the grid and the stop rules stay conservative. d_qorder
 * [m] int64 or NULL is the order in which the waves take the queries (a permutation of 0..m-1; an entry outside is clamped); every output
 * is addressed by the query's own index and does not depend on d_qorder. Every output may be NULL. One wave per query; the target in cell
 * order lives in scratch of the context (shared with the k-NN). Enqueue only.
 * The cross k-NN: the k (1..64) nearest target points of every query, ascending by d2, the lower original index first among equal
 * distances, dropped iff d2 > radius2 (+inf: no radius). d_count [m] int32, d_idx [m][k] int32 and d_d2 [m][k] float64 (unused slots -1 /
 * +inf), d_rings [m] int32 as the k-NN's (negated after the whole-cloud scan). A query with a non-finite coordinate gets count 0, rings 0.
 * The cross ball: the ball features' sums around the query, offsets fl(p - q) relative to it; the query is no neighbour unless a target point
 * coincides with it. d_count [m] int32, d_sums [m][10] int64, d_eig [m][3], d_normal [m][3] float64, d_steps [m] int32, all as the ball
 * features define them. A query with a non-finite coordinate gets count 0, zero sums, NaN, steps 0.
 * The cylinder statistics: d_nrm [m][3] float64 is used as given, never renormalised. A target point p is inside iff |t| <= half_length
 * and d2 - t*t <= fl(radius * radius), u = fl(p - q), t = ((ux*nx) + (uy*ny)) + (uz*nz), d2 = ((ux*ux) + (uy*uy)) + (uz*uz): cap and wall
 * are inside. it = rint(t / h), h = half_length * 2^-18, clamped to +-(2^18 + 1); exact int64 sums count, St, Stt. d_count [m] int32,
 * d_sums [m][2] int64 (St, Stt), d_mean [m] = (St / count) * h (NaN for count 0), d_std [m] = sqrt(max(0, Stt / count - (St / count)^2) *
 * (count / (count - 1))) * h (NaN for count < 2), d_steps [m] int32: the steps of 64 rows looked up or 64 candidates read over the
 * cylinder's axis-aligned box of cells, negated where the box would have cost more row lookups than 1024 + n / 32 and the whole sorted
 * cloud was scanned instead. A query with a non-finite coordinate or normal component gets count 0, NaN, steps 0.
 * The M3C2 finish, elementwise over m core points from the counts and sums of two cylinder calls with the same half_length: d_dist [m] =
 * mean2 - mean1, d_lod [m] = 1.96 * (sqrt(std1^2 / count1 + std2^2 / count2) + reg_error), NaN where either count is below min_points,
 * d_sig [m] uint8 = |dist| > lod (0 on NaN).
 * All four return -79, without launching and with the outputs untouched, for a null required pointer (d_pts, d_perm, d_start, h_grid, d_q;
 * d_nrm; the counts and sums), n or m negative or above 2^26, a grid the k-NN refuses, k outside 1..64, radius2 negative or NaN, a radius
 * or half-length that is not finite and positive, a radius (cross ball) or half-length times 2^-18 that is not a normal number, reg_error
 * negative or not finite, min_points below 2. n == 0 or m == 0 returns 0 and launches nothing. */
int im_knn_cross(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid, int nx,
                 int ny, int nz, const double* d_q, const long long* d_qorder, long long m, int k, double radius2, int32_t* d_count,
                 int32_t* d_idx, double* d_d2, int32_t* d_rings, void* stream);
int im_ball_cross(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid, int nx,
                  int ny, int nz, const double* d_q, const long long* d_qorder, long long m, double radius, int32_t* d_count, long long* d_sums,
                  double* d_eig, double* d_normal, int32_t* d_steps, void* stream);
int im_cyl_stats(im_ctx* ctx, const double* d_pts, const long long* d_perm, const int32_t* d_start, long long n, const double* h_grid, int nx,
                 int ny, int nz, const double* d_q, const double* d_nrm, const long long* d_qorder, long long m, double radius,
                 double half_length, int32_t* d_count, long long* d_sums, double* d_mean, double* d_std, int32_t* d_steps, void* stream);
int im_m3c2_finish(im_ctx* ctx, const int32_t* d_count1, const long long* d_sums1, const int32_t* d_count2, const long long* d_sums2,
                   long long m, double half_length, double reg_error, int min_points, double* d_dist, double* d_lod, uint8_t* d_sig,
                   void* stream);

/* ---- co-registration of two clouds (ICP) and rigid transforms (`src/icepy4d/utils/transformations.py`: `Rotrotranslation`;
 * Open3D's `registration_icp`, CloudCompare's fine registration); csrc/icp.hip, csrc/icp_point.h. Definitions in DESIGN §4, restated in
 * tests/icp_oracle.py: bit-identical; parity with an Open3D or CloudCompare binary is unpinned. float64, contraction off, only + - * / sqrt.
 * im_icp_chunk: ICP_CHUNK (1024), the source points per partial; part of the definition of every sum.
 * im_transform_points: d_out [n][3] = M applied to d_in [n][3] (d_out == d_in allowed), M = d_M [16] row-major 4x4 in DEVICE memory, last
 * row taken as (0, 0, 0, 1): p_a = ((M_a0*x + M_a1*y) + M_a2*z) + M_a3; as_vectors != 0 leaves the + M_a3 out (normals).
 * im_icp_accumulate: d_src [n][3] the transformed source, d_tgt [n_tgt][3], d_nrm [n_tgt][3] (NULL allowed for method 0), d_idx [n] int32
 * and d_d2 [n] float64 as im_knn_cross(k = 1) returned them, h_centre [3] in HOST memory, method 0 = point to point, 1 = point to plane,
 * n_chunks = ceil(n / ICP_CHUNK). Source point i is usable iff 0 <= d_idx[i] < n_tgt, its coordinates are finite and (method 1) the
 * normal is finite; an unusable point adds +0.0. Writes one partial of 32 doubles per chunk (21 upper entries of J^T J, 6 of J^T r,
 * sum r^2, sum d2, count, two zeros) into d_partials [n_chunks][32], or into the context's scratch when d_partials is NULL.
 * im_icp_finish: sums the partials (d_partials, or the context's scratch when NULL), solves A x = -b by LDL^T without pivoting and writes
 * d_record [64] float64: M_next [16], fitness = count / n, inlier_rmse = sqrt(sum d2 / count), count, status (0 OK, 1 EMPTY: count 0,
 * 2 DEGENERATE: count < 6 or a pivot d_k <= 2^-40 A_kk or NaN), x [6] = (w, t), the six pivots, the 30 sums and two zeros.
 * M_next = [R | fl(fl(t + c) - R c)] o M with R the Cayley map of w, M = d_M [16] in DEVICE memory (may be the M_next of another record);
 * M_next = M with a status other than OK and with solve == 0 (the evaluation only: x and the pivots are 0, the status EMPTY or OK).
 * All three return -81, without launching and with the outputs untouched, for a null required pointer, n or n_tgt outside 0..2^26, a
 * non-finite centre, a method outside {0, 1}, method 1 without normals, solve outside {0, 1}, n_chunks != ceil(n / ICP_CHUNK), or a
 * finish from the context's scratch before an accumulate of as many chunks. n == 0: transform and accumulate return 0 and launch nothing;
 * the finish writes the EMPTY record. Enqueue only. */
int im_icp_chunk(void);
int im_transform_points(im_ctx* ctx, const double* d_M, const double* d_in, double* d_out, long long n, int as_vectors, void* stream);
int im_icp_accumulate(im_ctx* ctx, const double* d_src, long long n, const double* d_tgt, const double* d_nrm, long long n_tgt,
                      const int32_t* d_idx, const double* d_d2, const double* h_centre, int method, long long n_chunks, double* d_partials,
                      void* stream);
int im_icp_finish(im_ctx* ctx, const double* d_partials, long long n, long long n_chunks, const double* d_M, const double* h_centre, int solve,
                  double* d_record, void* stream);

/* ---- two-view bundle adjustment with control points (the driver's last step, `chunk.optimizeCameras(fit_f=True)` in
 * `MetashapeProject.run_full_workflow`, with a definition of its own); csrc/ba.hip, csrc/ba_point.h. Definitions in DESIGN §4, restated in
 * tests/ba_oracle.py: bit-identical; parity with a Metashape binary is unpinned. float64, contraction off, only + - * / sqrt.
 * Levenberg-Marquardt with the points eliminated, batched over E epochs. All arrays in DEVICE memory unless named h_:
 * d_off [E + 1] int64, the first point of every epoch and the end; M points in all; max_points bounds the points of an epoch (the grid).
 * PRECONDITION: max_points >= d_off[e + 1] - d_off[e] for every epoch. The offsets are in device memory, so the entry points cannot check
 * it: with a smaller value the chunks beyond max_points of a longer epoch are not computed, and im_ba_solve / im_ba_decide, which sum
 * ceil(n_e / 256) partials per epoch, would add whatever those slots held.
 * d_pts2 [2][M][3] and d_cams2 [2][E][2][24] are double-buffered: an epoch's current ones are those of its parity. A camera is R [9]
 * row-major, C [3], fx fy cx cy, k1 k2 p1 p2 k3 k4 k5 k6 with Xc = R (X - C). d_obs [M][4] = (u0, v0, u1, v1) pixels, a NaN = not seen;
 * d_sig [M] pixels; d_prior [M][6] = (X0 [3], sX [3]), sX_k > 0 puts a prior on component k; d_cprior [E][2][6] likewise for the centres.
 * d_state [E][8] = lambda, parity, done, status (-1 running, 0 OK, 1 MAX_ITER, 2 STALLED, 3 EMPTY, 4 DEGENERATE), iterations recorded, 3 spare:
 * the caller writes (lambda_0, 0, 0, -1, 0) before the first iteration, and may hand a returned state back to go on.
 * im_ba_chunk: BA_CHUNK (256), the points per partial; part of the definition of every sum.
 * One iteration is the four calls in this order, none of which reads back; the blocks of a finished epoch return at once.
 * im_ba_accumulate: one partial of 448 doubles per chunk (406 upper entries of the reduced 28 x 28 system, 28 right-hand sides, cost, usable
 * count, 12 zeros) into d_parts [M / 256 + E + 1][448] (the context's scratch when NULL) at slot off[e] / 256 + e + chunk, and 95 doubles
 * per point for the back-substitution into the context's scratch.
 * im_ba_solve: the partials in ascending order, centre priors, damping, the mask (bit p frees parameter p of 28: per camera w [3], dC [3],
 * df, dcx, dcy, dk1, dk2, dp1, dp2, dk3), LDL^T without pivoting with im_icp_finish's pivot rule; d_sol [E][512] = the 448 sums and the
 * draft of the record; the candidate cameras go into the other half of d_cams2.
 * im_ba_step_points: the back-substitution, candidate points into the other half of d_pts2, one cost partial per chunk into d_cparts
 * [M / 256 + E + 1] (the context's scratch when NULL).
 * im_ba_decide: accept iff the candidate's cost is strictly lower; h_opts [5] in HOST memory = lambda floor, lambda ceiling, ftol, max_iter, ctol;
 * writes the record [64] = cost before, cost after, lambda, accepted, count, status after, x [28], pivots [28], iteration, 0 to d_history
 * [hist_rows][E][64] at the row of the epoch's iteration count, and updates d_state.
 * im_ba_residuals: d_res [M][2][3] = (u - u_obs, v - v_obs, norm) in pixels per camera of the current state, NaN where not seen.
 * All five return -82, without launching, for a null required pointer, E outside 1..65535, M outside 0..2^26, max_points outside 0..M, a
 * mask outside 28 bits, options outside 0 < floor <= ceiling, ftol >= 0, 1 <= max_iter <= hist_rows, ctol >= 0, or a call that finds the context's
 * scratch smaller than an im_ba_accumulate of the same E and M left it. Enqueue only. */
int im_ba_chunk(void);
int im_ba_accumulate(im_ctx* ctx, const long long* d_off, int E, long long M, long long max_points, const double* d_pts2, const double* d_obs,
                     const double* d_sig, const double* d_prior, const double* d_cams2, const double* d_state, double* d_parts, void* stream);
int im_ba_solve(im_ctx* ctx, const long long* d_off, int E, long long M, const double* d_parts, double* d_cams2, const double* d_cprior,
                const double* d_state, unsigned mask, double* d_sol, void* stream);
int im_ba_step_points(im_ctx* ctx, const long long* d_off, int E, long long M, long long max_points, double* d_pts2, const double* d_obs,
                      const double* d_sig, const double* d_prior, const double* d_cams2, const double* d_state, const double* d_sol,
                      double* d_cparts, void* stream);
int im_ba_decide(im_ctx* ctx, const long long* d_off, int E, long long M, const double* d_cparts, const double* d_cams2, const double* d_cprior,
                 double* d_state, const double* d_sol, const double* h_opts, double* d_history, long long hist_rows, void* stream);
int im_ba_residuals(im_ctx* ctx, const long long* d_off, int E, long long M, long long max_points, const double* d_pts2, const double* d_obs,
                    const double* d_cams2, const double* d_state, double* d_res, void* stream);

/* ---- two-view dense stereo: depth maps, their consistency and the dense cloud (what the driver gets from Metashape's
 * `chunk.buildDepthMaps` and `chunk.buildDenseCloud`, `metashape.py:198-240`, straight after the bundle adjustment); csrc/dense.hip,
 * csrc/dense_pixel.h. Metashape's matcher is closed and is NOT reproduced: the stage has a definition of its own, restated in
 * tests/dense_oracle.py: bit-identical; parity with Metashape is unpinned by construction. All arrays in DEVICE memory unless named h_.
 * im_dense_sweep: a plane sweep over D fronto-parallel planes of the ref view, inverse depths w_k = w_first + k w_step. d_ref [h0][w0] and
 * d_src [h1][w1] are undistorted 8-bit grey images; h_A = K1 R inv(K0) and h_B = K1 t e3^T inv(K0), [9] row-major in HOST memory, with
 * X1 = R X0 + t. Per plane and ref pixel H = A + w_k B, (x, y, z) = H (u, v, 1); the sample is invalid if z <= 0, a coordinate is not
 * finite or one of the four taps lies outside src; x / z and y / z are rounded to 1/32 pixel (im_warp_perspective's rounding) and the
 * warped value is the 18-bit integer b = sum of 5-bit weight products times pixel. Window of radius r, n = (2 r + 1)^2: exact integer sums;
 * VA = n Saa - Sa^2, VB = n Sbb - Sb^2, C = n Sab - Sa Sb; invalid if the window leaves ref, holds an invalid sample, VA < n^2 min_var,
 * VB < n^2 min_var 2^20 or a variance is zero; else s = C / sqrt(VA VB). The best plane is the largest s (ties to the lower index); the
 * sub-plane offset 0.5 (s- - s+) / (s- - 2 s0 + s+) applies for 1 <= k <= D - 2 with both neighbours valid and a negative denominator.
 * d_plane [h0][w0] int16 (-1: no plane scored or s0 < min_score; then w and score are 0), d_w [h0][w0] float64 = w_first + (k + off) w_step,
 * d_score [h0][w0] float32. One block per im_dense_tile_w() x im_dense_tile_h() pixels; the tile is no part of the definition.
 * im_dense_consistency: d_keep [h0][w0] uint8 = 1 where map 0 holds a plane and (check = 1) its point X1 = R (inv(K0) (u, v, 1) / w) + t
 * lies in front of view 1, projects (rint) onto a pixel of map 1 that holds a plane, and |w1 - 1 / X1.z| <= tol. h_pose [30] in HOST memory
 * = inv(K0) [9], R [9], t [3], K1 [9]. check = 0: d_keep = (plane0 >= 0), map 1 and the pose may be NULL.
 * im_dense_cloud: the kept pixels in row-major order: d_xyz [capacity][3] float64 = R0^T (X0 - t0), d_rgb [capacity][3] uint8 = the bytes
 * of d_img [h][w][channels] (1 or 3 channels; grey three times), d_nrm [capacity][3] float64 = the unit cross product of the differences
 * of the neighbours' points along u and v (central where both neighbours are kept, one-sided where one is, zero where a direction has
 * none), turned towards the camera centre, d_conf [capacity] float32 = the score. h_cam [21] in HOST memory = inv(K0) [9], R0 [9], t0 [3].
 * *d_count = the number of kept pixels; rows from min(count, capacity) on are left untouched.
 * All three return -83, without launching and with the outputs untouched, for a null required pointer, h or w outside 1..16384, D outside
 * 1..4096, r outside 1..7, min_var negative or above 2^26, check outside 0..1, a negative or NaN tol, channels other than 1 or 3, a
 * negative capacity or a camera that is not finite. Enqueue only. */
int im_dense_tile_w(void);
int im_dense_tile_h(void);
int im_dense_sweep(im_ctx* ctx, const uint8_t* d_ref, int h0, int w0, const uint8_t* d_src, int h1, int w1, const double* h_A, const double* h_B,
                   double w_first, double w_step, int D, int r, long long min_var, double min_score, int16_t* d_plane, double* d_w, float* d_score,
                   void* stream);
int im_dense_consistency(im_ctx* ctx, const int16_t* d_plane0, const double* d_w0, int h0, int w0, const int16_t* d_plane1, const double* d_w1, int h1,
                         int w1, const double* h_pose, double tol, int check, uint8_t* d_keep, void* stream);
int im_dense_cloud(im_ctx* ctx, const uint8_t* d_keep, const double* d_w, const float* d_score, const uint8_t* d_img, int channels, int h, int w,
                   const double* h_cam, long long capacity, double* d_xyz, uint8_t* d_rgb, double* d_nrm, float* d_conf, long long* d_count,
                   void* stream);

/* ---- semi-global regularisation of a depth map (csrc/dense_sgm.hip, csrc/sgm_pixel.h): the smoothness term the winner-take-all sweep
 * above lacks, where the driver asks Metashape for filtered depth maps (`metashape.py:198-240`). A definition of this project's own
 * (DESIGN §4), restated in tests/sgm_oracle.py: bit-identical; it is NOT Metashape's filter. All arrays in DEVICE memory unless named h_.
 * im_dense_costs: the sweep's (valid, s) of every ref pixel and plane (same arguments, same arithmetic as im_dense_sweep), quantised:
 * d_cost [h0][w0][D] uint8, planes contiguous, = 255 where the plane did not score, else min(254, max(0, floor((1 - s) 127))).
 * im_dense_sgm: d_sum [h0][w0][D] uint16 = the sum over `paths` (4 or 8) directions (dy, dx) = (0,1) (0,-1) (1,0) (-1,0), then (1,1)
 * (-1,-1) (1,-1) (-1,1), of L(p, d) = c(p, d) where q = p - (dy, dx) lies outside the image, else
 * c(p, d) + min(L(q, d), L(q, d - 1) + P1, L(q, d + 1) + P1, m + P2) - m with m = min_k L(q, k); terms with d - 1 < 0 or d + 1 >= D are
 * absent; an invalid cost enters as the plain value 255. 0 <= P1 <= P2 <= 4095, so L <= 4350 and the sum <= 34800. One wave per path
 * line, four planes per lane: D <= im_dense_sgm_max_planes() = 256. Every element of d_sum is written; it need not be cleared.
 * im_dense_sgm_choose: per pixel, among the planes with c != 255 the least sum (ties to the lower plane) k; the sub-plane offset
 * 0.5 (S- - S+) / (S- - 2 S0 + S+) applies for 1 <= k <= D - 2 with both neighbours valid at the pixel and a positive integer denominator;
 * d_w = w_first + (k + off) w_step; d_score = float(1 - c(p, k) / 127); d_plane = -1, w = score = 0 where no plane is valid or the
 * score is below min_score. The three maps have the types and the meaning of im_dense_sweep's: im_dense_consistency and im_dense_cloud
 * take them as they are.
 * All three return -83, without launching and with the outputs untouched, for a null pointer, h or w outside 1..16384, D outside 1..256,
 * r outside 1..7, min_var negative or above 2^26, P1 < 0, P1 > P2, P2 > 4095, paths other than 4 or 8, or h0 w0 D > 2^32. Enqueue only. */
int im_dense_sgm_max_planes(void);
int im_dense_costs(im_ctx* ctx, const uint8_t* d_ref, int h0, int w0, const uint8_t* d_src, int h1, int w1, const double* h_A, const double* h_B,
                   double w_first, double w_step, int D, int r, long long min_var, uint8_t* d_cost, void* stream);
int im_dense_sgm(im_ctx* ctx, const uint8_t* d_cost, int h0, int w0, int D, int P1, int P2, int paths, uint16_t* d_sum, void* stream);
int im_dense_sgm_choose(im_ctx* ctx, const uint8_t* d_cost, const uint16_t* d_sum, int h0, int w0, int D, double w_first, double w_step,
                        double min_score, int16_t* d_plane, double* d_w, float* d_score, void* stream);

/* ---- depth-map clean-up: connected components, speckle removal and hole filling (csrc/depth_clean.hip, csrc/depth_pixel.h), where the
 * driver asks Metashape for filtered depth maps (`metashape.py:198-240`). A definition of this project's own, restated in
 * tests/depth_oracle.py: bit-identical; it is NOT OpenCV's filterSpeckles and NOT Metashape's filter. All arrays in DEVICE memory.
 * Pixels are neighbours when they share an edge (4-connectivity). d_plane [h][w] int16 is the sweep's map; a pixel holds a plane when
 * plane >= 0. mode 0 (surfaces): the members are the pixels that hold a plane, two neighbouring members are joined when
 * |plane_p - plane_q| <= max_diff (integers). mode 1 (holes): the members hold no plane, any two neighbouring members are joined.
 * im_depth_components: the connected components of the join graph (joining is transitive: 3-4-5 is one component at max_diff = 1).
 * d_label [h][w] int32 = the least linear index y w + x of the pixel's component, -1 for a non-member; d_size [h][w] int32 = the number of
 * pixels of that component, 0 for a non-member. A union-find over d_label in four launches (tiles of im_depth_tile_w() x im_depth_tile_h()
 * pixels in LDS, the joins across tile edges, the roots and their counts, the sizes); the tile is no part of the definition.
 * im_depth_drop_small: in place on the three maps; d_size is the mode-0 size of d_plane. A pixel that holds a plane and whose component
 * has size < min_size gets plane = -1, w = 0, score = 0 (what the sweep writes for a dropped pixel); every other pixel is untouched.
 * *d_count (int64) = the number of pixels dropped. min_size = 1 drops nothing.
 * im_depth_fill_holes: d_label and d_size are the mode-1 results for the same d_plane. A hole qualifies when none of its pixels lies in
 * the first or last row or column, its size is at most max_hole, and hi - lo <= max_diff with lo / hi the least / greatest plane over the
 * plane-holding pixels that neighbour any of its pixels. A pixel (x, y) of a qualifying hole has the nearest plane-holding pixels xl < x < xr
 * in its row and yu < y < yd in its column; in float64, exactly these operations in this order, no contraction:
 *   a = w[y][xl] + (w[y][xr] - w[y][xl]) * (double(x - xl) / double(xr - xl)),  b = w[yu][x] + (w[yd][x] - w[yu][x]) * (double(y - yu) / double(yd - yu)),
 *   w_out = 0.5 * (a + b),  plane_out = min(D - 1, max(0, rint((w_out - w_first) / w_step))) (ties to even),  score_out = 0 (a filled pixel).
 * Every other pixel is copied through. d_filled [h][w] uint8 = 1 on the filled pixels, 0 elsewhere; *d_count (int64) = their number. The
 * outputs are arrays of their own: a filled pixel must never be read as a rim pixel by another thread.
 * All three return -83, without launching and with the outputs untouched, for a null pointer, h or w outside 1..16384, mode other than 0
 * or 1, max_diff outside 0..4095, min_size < 1, max_hole outside 1..4096, D outside 1..4096, w_first not finite, w_step not finite or
 * zero, or (im_depth_fill_holes) an output map that is its input. Enqueue only. */
int im_depth_tile_w(void);
int im_depth_tile_h(void);
int im_depth_components(im_ctx* ctx, const int16_t* d_plane, int h, int w, int mode, int max_diff, int* d_label, int* d_size, void* stream);
int im_depth_drop_small(im_ctx* ctx, const int* d_size, int h, int w, int min_size, int16_t* d_plane, double* d_w, float* d_score, long long* d_count,
                        void* stream);
int im_depth_fill_holes(im_ctx* ctx, const int16_t* d_plane, const double* d_w, const float* d_score, const int* d_label, const int* d_size, int h, int w,
                        int max_hole, int max_diff, double w_first, double w_step, int D, int16_t* d_plane_out, double* d_w_out, float* d_score_out,
                        uint8_t* d_filled, long long* d_count, void* stream);

/* ---- fusion of the two depth maps: one point per surface sample, placed by both views (csrc/dense_fuse.hip, csrc/fuse_pixel.h), where
 * the driver asks Metashape for `buildDenseCloud(point_confidence=True)` (`metashape.py:198-240`). A definition of this project's own
 * (DESIGN §4), restated in tests/fuse_oracle.py: bit-identical; it is NOT Metashape's merge, and parity with Metashape is unpinned by
 * construction. All arrays in DEVICE memory but the poses. View a is the base, view b the other one; keep masks are uint8, non-zero = kept,
 * as im_dense_consistency writes them. h_pose [30] = inv(Ka), R, t, Kb with Xb = R Xa + t (the layout of im_dense_consistency); tol >= 0
 * is an inverse depth of the view linked INTO. float64, exactly these operations in this order, no contraction.
 * The link of kept pixel p = (u, v) of view a: Xa = inv(Ka) (u, v, 1) / w_a[p], Xb = R Xa + t as im_dense_consistency computes them; it
 * fails unless Xb.z > 0; j = (rint(px / pz), rint(py / pz)) of Kb Xb; it fails unless j lies inside view b (a NaN fails) and keep_b[j] != 0,
 * and unless |w_b[j] - 1 / Xb.z| <= tol. link[p] = j as a linear index, else -1; -1 where keep_a[p] == 0.
 * The second measurement on p's ray: d_i = (Ki[3i] u + Ki[3i+1] v) + Ki[3i+2], g = (R[6] d_0 + R[7] d_1) + R[8] d_2,
 * w' = g / (1.0 / w_b[j] - t[2]); usable when w' is finite and > 0.
 * im_dense_fuse_link: clears d_claimed [hb][wb], then per pixel p of view a. Linked: a = max(double(score_a[p]), 0),
 * b = max(double(score_b[j]), 0); if w' is usable, w_out = (a w + b w') / (a + b) when a + b > 0, else 0.5 (w + w'), and
 * score_out = max(score_a[p], score_b[j]); if it is not, w_out = w and score_out = score_a[p]; either way views[p] = 2 and claimed[j] = 1.
 * Kept and unlinked: copied through with views = 1. Not kept: w_out = 0, score_out = 0, views = 0. Several p may claim one j; each keeps
 * its own point, and the stores of the same byte need no atomic.
 * im_dense_fuse_rest: h_pose_ba is the inverted pose (inv(Kb), R^T, -R^T t, Ka), tol_a an inverse depth of view a. rest[q] = 1 iff
 * keep_b[q] != 0, claimed[q] == 0 and the link of q into view a fails: a surface that view a does not represent; else 0.
 * Both write every element of every output, and return -83, without launching and with the outputs untouched, for a null pointer, a side
 * outside 1..16384, a negative or NaN tolerance, or an output that is one of the inputs. Enqueue only. */
int im_dense_fuse_link(im_ctx* ctx, const uint8_t* d_keep_a, const double* d_w_a, const float* d_score_a, int ha, int wa, const uint8_t* d_keep_b,
                       const double* d_w_b, const float* d_score_b, int hb, int wb, const double* h_pose, double tol, int* d_link, double* d_w_out,
                       float* d_score_out, uint8_t* d_views, uint8_t* d_claimed, void* stream);
int im_dense_fuse_rest(im_ctx* ctx, const uint8_t* d_keep_b, const double* d_w_b, int hb, int wb, const uint8_t* d_keep_a, const double* d_w_a, int ha,
                       int wa, const double* h_pose_ba, double tol_a, const uint8_t* d_claimed, uint8_t* d_rest, void* stream);

/* ---- slanted-window refinement of a depth map (csrc/dense_refine.hip, csrc/refine_pixel.h): im_dense_sweep warps every sample of a window
 * with the centre's inverse depth (fronto-parallel); this pass lets the window follow the surface's slant. A definition of this project's
 * own, restated in tests/refine_oracle.py: bit-identical; it is NOT Metashape's matcher, and parity with Metashape is unpinned
 * by construction. All arrays in DEVICE memory unless named h_. A map is (d_plane int16, d_w float64, d_score float32) as im_dense_sweep
 * writes it, with the step w_step of its schedule; a pixel is kept when plane >= 0. Slants are in plane steps per pixel.
 * im_dense_slant: per kept pixel i, over the kept pixels j of its (2 fit_radius + 1)^2 neighbourhood inside the map (i included):
 * d = (w_j - w_i) / w_step; j counts when fabs(d) <= max_diff (a NaN fails), at the integer height q = llrint(1024 d). Exact int64 sums over
 * the counting j of 1, dx, dy, dx^2, dy^2, dx dy, q, q dx, q dy give a11 = n Sxx - Sx^2, a22 = n Syy - Sy^2, a12 = n Sxy - Sx Sy,
 * b1 = n Sqx - Sx Sq, b2 = n Sqy - Sy Sq, det = a11 a22 - a12^2. Fitted when n >= min_count and det > 0:
 * gu = (double(a22 b1 - a12 b2) / double(det)) / 1024, gv = (double(a11 b2 - a12 b1) / double(det)) / 1024; else gu = gv = 0.
 * d_slant [h][w][2] float64 = (gu, gv), d_fitted [h][w] uint8; a dropped pixel gets zeros. Every element is written.
 * im_dense_refine: ref, src, h_A, h_B, r and min_var as im_dense_sweep takes them. A pixel (u, v) is refined when it is kept and its window
 * of radius r lies inside ref; every other pixel is copied through. Candidates c = -span sub .. span sub; sample (dx, dy) of candidate c is
 * im_dense_sweep's sample of ref pixel (u + dx, v + dy) under H = A + w_s B, w_s = w_i + t w_step, t = double(c) / double(sub) + (gu dx + gv dy).
 * A candidate with an invalid sample is invalid; else it scores the sweep's s of the integer window sums. The best is chosen in the order
 * 0, -1, +1, -2, +2, ..., a later candidate replacing it only on a strictly greater score; off is the sweep's parabola over the best's two
 * neighbours when both lie in the range, both are valid and the denominator is negative. Taken when s0 > double(score_i), strictly:
 * w_out = w_i + ((double(c) + off) / double(sub)) w_step, score_out = float(s0); else w_out = w_i, score_out = score_i. d_plane is never
 * changed. d_taken [h0][w0] uint8. The outputs are arrays of their own; every element is written; no score falls.
 * Both return -83, without launching and with the outputs untouched, for a null pointer, a side outside 1..16384, fit_radius or r outside
 * 1..7, max_diff not in (0, 64], min_count outside 3..225, span outside 1..4, sub outside 1..8, min_var outside 0..2^26, or a w_step that
 * is zero or not finite. One block per im_dense_tile_w() x im_dense_tile_h() pixels; the tile is no part of the definition. Enqueue only. */
int im_dense_slant(im_ctx* ctx, const int16_t* d_plane, const double* d_w, int h, int w, double w_step, int fit_radius, double max_diff, int min_count,
                   double* d_slant, uint8_t* d_fitted, void* stream);
int im_dense_refine(im_ctx* ctx, const uint8_t* d_ref, int h0, int w0, const uint8_t* d_src, int h1, int w1, const double* h_A, const double* h_B,
                    const int16_t* d_plane, const double* d_w, const float* d_score, const double* d_slant, double w_step, int r, long long min_var, int span,
                    int sub, double* d_w_out, float* d_score_out, uint8_t* d_taken, void* stream);

/* ---- dense surface displacement between two epochs (csrc/dense_flow.hip, csrc/flow_pixel.h): the pixel of one camera's image at epoch B
 * that shows what a pixel of its image at epoch A shows, and both ends lifted to world points through each epoch's own depth map and pose.
 * The reference has no such step (its velocities come from tracked keypoints): a definition of this project's own, restated
 * in tests/flow_oracle.py: bit-identical. Parity with any image-correlation package is unpinned. All arrays in DEVICE memory unless named h_.
 * im_flow_match: d_a, d_b [h][w] uint8. A candidate (dx, dy), |dx|, |dy| <= search, compares the (2 r + 1)^2 window of a centred on (u, v)
 * with the window of b centred on (u + prior_u + dx, v + prior_v + dy); it is invalid if either window leaves its image. With n = (2 r + 1)^2
 * and the exact integer sums: VA = n saa - sa^2, VB = n sbb - sb^2, C = n sab - sa sb; invalid if VA < n^2 min_var, VB < n^2 min_var, VA <= 0
 * or VB <= 0, else s = double(C) / sqrt(double(VA) double(VB)). Candidates are visited in ascending (dx^2 + dy^2, dy, dx), a later one replacing
 * the best only on a strictly greater score. The pixel is invalid if no candidate scored or the best is below min_score. Along x (and y
 * likewise): if both neighbours (dx - 1, dy), (dx + 1, dy) lie in the search range and score, and den = (sm - 2 s0) + sp < 0, then
 * off = (0.5 (sm - sp)) / den, else 0. d_du = double(prior_u + dx) + offx, d_dv likewise (float64), d_score = float(s0), d_valid uint8; zeros
 * where invalid or where d_ask [h][w] uint8 (NULL = every pixel) is 0. One block per im_dense_tile_w() x im_dense_tile_h() pixels.
 * im_flow_check: a valid forward pixel (u, v) is kept when j = (rint(u + du), rint(v + dv)) lies inside the image, the backward field is
 * valid at j and (du + du_b[j])^2 + (dv + dv_b[j])^2 <= tol^2; a NaN fails. d_keep [h][w] uint8.
 * im_flow_lift: h_cam_a, h_cam_b [21] = inv(K), R, t as im_dense_cloud takes them. A pixel is lifted when d_keep, d_valid are set and
 * d_plane_a >= 0. P = the world point of (u, v, w_a). With x = u + du, y = v + dv: the four taps floor(x) .. floor(x) + 1, floor(y) ..
 * floor(y) + 1 must lie inside map b [hb][wb] (a tap of weight zero included), have plane_b >= 0 and keep_b set, and their inverse depths
 * span at most max_diff |w_step_b|; w = top + ty (bot - top), top = w00 + tx (w01 - w00), bot = w10 + tx (w11 - w10). Q = the world point
 * of (x, y, w) through camera b, D = Q - P. d_P, d_D [h][w][3] float64, d_ok [h][w] uint8; zeros where not lifted.
 * All write every element of every output, and return -83, without launching and with the outputs untouched, for a null required pointer,
 * a side outside 1..16384, r outside 1..15, search outside 0..16, a prior outside -4096..4096, min_var outside 0..2^26, a min_score that
 * is not finite, a tol or max_diff that is not finite or not > 0, or a w_step_b that is zero or not finite. Enqueue only. */
int im_flow_match(im_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int h, int w, int r, int search, int prior_u, int prior_v, long long min_var,
                  double min_score, const uint8_t* d_ask, double* d_du, double* d_dv, float* d_score, uint8_t* d_valid, void* stream);
int im_flow_check(im_ctx* ctx, const double* d_du, const double* d_dv, const uint8_t* d_valid, const double* d_du_b, const double* d_dv_b,
                  const uint8_t* d_valid_b, int h, int w, double tol, uint8_t* d_keep, void* stream);
int im_flow_lift(im_ctx* ctx, const double* d_du, const double* d_dv, const uint8_t* d_valid, const uint8_t* d_keep, const int16_t* d_plane_a,
                 const double* d_w_a, int h, int w, const double* h_cam_a, const int16_t* d_plane_b, const double* d_w_b, const uint8_t* d_keep_b, int hb,
                 int wb, const double* h_cam_b, double w_step_b, double max_diff, double* d_P, double* d_D, uint8_t* d_ok, void* stream);

/* ---- coarse-to-fine dense displacement (csrc/dense_flow_field.hip, csrc/flow_field_pixel.h): a prior per pixel in place of im_flow_match's
 * one global prior, and the prior of a level from the field of the level above. Level l + 1 of the pyramid is im_pyr_down of level l with
 * one channel, so coarse pixel (x, y) sits on fine pixel (2 x, 2 y) and a displacement halves per level. A definition of this project's own
 * (DESIGN §4), restated in tests/pyrflow_oracle.py: bit-identical. All arrays in DEVICE memory.
 * im_flow_prior_up: d_du_c, d_dv_c float64 and d_valid_c uint8 [hc][wc] are a field of the coarse level, hc = (h + 1) / 2, wc = (w + 1) / 2.
 * For fine pixel (u, v): the coarse pixels of the (2 median_radius + 1)^2 neighbourhood of (u >> 1, v >> 1) inside the coarse image that are
 * valid and whose du and dv are both finite, n of them. n < min_count: have = 0, pu = pv = 0. Else pu = (int) rint(2.0 * med_u) with med_u
 * element (n - 1) / 2 of the ascending du values (the lower median, no averaging), pv likewise from the dv values, independently; if
 * |pu| > 4096 or |pv| > 4096, have = 0 and both are zero. d_pu, d_pv int16 [h][w], d_have uint8 [h][w].
 * im_flow_match_field: im_flow_match with the prior (d_pu, d_pv) of each pixel in place of (prior_u, prior_v). A pixel is matched when
 * d_have is not 0 there, d_ask (NULL = every pixel) is not 0 there and both components of its prior lie in -4096..4096; its candidates are
 * its own prior + (dx, dy), |dx|, |dy| <= search, exact ties go to the smallest displacement from its own prior, and the parabola takes
 * neighbours inside its own range only. Every other pixel gets zeros and d_valid = 0. With a constant field this is im_flow_match with that
 * prior, bit for bit. Safe for any content of d_pu, d_pv, d_have, d_ask: neither image is read outside its bounds. One block per
 * im_dense_tile_w() x im_dense_tile_h() pixels; d_tile_path (NULL, or uint8 [blocks_y][blocks_x]) receives the path each tile took, a pure
 * function of its inputs: 0 = no pixel of the tile is to be matched with its window inside a, else with the box [lo_u, hi_u] x [lo_v, hi_v]
 * of those pixels' priors, 1 (tiled, from LDS) where hi_u - lo_u <= E and hi_v - lo_v <= E, 2 (direct, from global memory) otherwise;
 * E = the greatest value <= 8 at which the tiled path's LDS for a box of E x E fits 64512 bytes at this r and search. Both paths give the
 * same bits.
 * Both write every element of every output, and return -83, without launching and with the outputs untouched, for a null pointer other
 * than d_ask and d_tile_path, a side outside 1..16384, hc != (h + 1) / 2 or wc != (w + 1) / 2, median_radius outside 0..2, min_count outside
 * 1..(2 median_radius + 1)^2, r outside 1..15, search outside 0..16, min_var outside 0..2^26 or a min_score that is not finite. Enqueue only. */
int im_flow_prior_up(im_ctx* ctx, const double* d_du_c, const double* d_dv_c, const uint8_t* d_valid_c, int hc, int wc, int h, int w,
                     int median_radius, int min_count, int16_t* d_pu, int16_t* d_pv, uint8_t* d_have, void* stream);
int im_flow_match_field(im_ctx* ctx, const uint8_t* d_a, const uint8_t* d_b, int h, int w, int r, int search, const int16_t* d_pu,
                        const int16_t* d_pv, const uint8_t* d_have, long long min_var, double min_score, const uint8_t* d_ask, double* d_du,
                        double* d_dv, float* d_score, uint8_t* d_valid, uint8_t* d_tile_path, void* stream);

/* ---- volume variations (`scripts/pcd_postprocessing/volume_variations.py`; `post_processing/cloudcompare_fun.py`:
 * `DemOfDifference.compute_volume` over CloudCompare's `ComputeVolume25D`; `post_processing/open3d_fun.py`: `filter_pcd_by_polyline`);
 * csrc/dod.hip, csrc/dod_cell.h. The DEM of difference of P pairs (ground, ceil) over E clouds that lie one behind the other in d_pts
 * [n][3] float64, DEVICE memory; h_offsets [E + 1] int64 in HOST memory = the first point of every cloud, h_offsets[0] = 0; h_pairs [P][2]
 * int32 in HOST memory = cloud indices (ground, ceil). vert_dim d in 0..2: heights along d, the grid over X = (d + 1) % 3 and
 * Y = (d + 2) % 3. A point with a non-finite coordinate is ignored. Per pair: min / max over the kept points of both clouds,
 * w = 1 + floor((max_x - min_x) / step + 0.5), h likewise, a point in column floor((x - min_x) / step + 0.5), cell j w + i; per cloud
 * and cell the mean of the d-coordinates summed in ascending point index from +0.0; H = mean_ceil - mean_ground where both clouds fill
 * the cell, NaN elsewhere; a cell is valid when H is finite. No kept point: w = h = 0. float64, no fused operations
 * (tests/dod_oracle.py: bit-identical; parity with a CloudCompare binary is not pinned).
 * im_dod_chunk: B (1024). The three sums over cells run over chunks of B consecutive cells in ascending cell index from +0.0, the chunk
 * partials are added in ascending chunk index: the order depends on nothing else.
 * im_dod_max_cells: the largest w * h of a pair (2^24). im_dod_max_batch_cells: the most cells the pairs of one call hold together
 * (2^26); they also hold fewer than 2^31 points (a cloud counts once per pair it is part of); E and P are at most 65535.
 * im_dod_bounds: d_bounds [E][4] float64 = min_x, min_y, max_x, max_y of every cloud's kept points (+inf, +inf, -inf, -inf without one;
 * of zeros of either sign the minimum is -0.0 and the maximum +0.0), d_dropped [E] int64 = its ignored points.
 * im_dod_keys: h_bounds [E][4] = d_bounds downloaded; h_grids [P][4] float64 in HOST memory receives min_x, min_y, w, h of every pair;
 * d_key [items] int64, items = the points of all pairs' clouds in the order pair, side, point: the segment of each (a dropped point:
 * the number of segments, 2 * sum of w * h); d_key may be NULL: the grids alone, nothing is launched. The caller sorts the keys (stable) and hands the sorted keys and the permutation on.
 * im_dod_reduce: d_H, may be NULL: the rasters [h][w] float64 of the pairs one behind the other; d_report [P][16] float64 = volume,
 * addedVolume, removedVolume, surface, matchingPercent, groundNonMatchingPercent, ceilNonMatchingPercent, averageNeighborsPerCell,
 * validCells, cellCount, gridWidth, gridHeight, min_x, min_y, step, step * step. With a = step * step: volume = a * sum H, added =
 * a * sum of H > 0, removed = a * (0 - sum of H < 0), surface = a * validCells, the percents (100 * count) / cellCount with cellCount the
 * cells either cloud fills, averageNeighborsPerCell = (valid cells among the 8 in-grid neighbours, summed over valid cells) /
 * validCells. Without a valid cell the first nine are +0.0.
 * im_crop_polygon: d_mask [n] uint8 = 1 where point (p[axis_x], p[axis_y]) is inside (inside != 0) or outside the closed polygon h_poly
 * [n_verts][2] float64 in HOST memory, by the even-odd rule: for every edge (x0, y0) -> (x1, y1), from the last vertex to the first and
 * then in order, toggle if (y0 > y) != (y1 > y) and x < (x1 - x0) * (y - y0) / (y1 - y0) + x0; a non-finite coordinate is not
 * inside. d_index [n] int64 receives the kept indices in ascending order, d_count [1] int64 their number.
 * The calls wait for the upload of their tables, then enqueue. All return -76, without launching, for a null required pointer, a step
 * that is not finite or not > 0, vert_dim outside 0..2, a pair naming a cloud outside 0..E-1, offsets that do not start at 0 or
 * descend (a negative count), a NaN bound, a pair whose w * h exceeds im_dod_max_cells(), a batch over the limits above; the crop for
 * axes that are not two of 0..2, n outside 0..2^31-1, n_verts outside 3..1024, a non-finite vertex. P == 0 returns 0 and launches nothing. */
int im_dod_chunk(void);
int im_dod_max_cells(void);
int im_dod_max_batch_cells(void);
int im_dod_bounds(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, int vert_dim, double* d_bounds, long long* d_dropped,
                  void* stream);
int im_dod_keys(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, const int32_t* h_pairs, int n_pairs, int vert_dim,
                double step, const double* h_bounds, double* h_grids, long long* d_key, void* stream);
int im_dod_reduce(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, const int32_t* h_pairs, int n_pairs, int vert_dim,
                  double step, const double* h_bounds, const long long* d_sorted_keys, const long long* d_perm, double* d_H, double* d_report,
                  void* stream);
int im_crop_polygon(im_ctx* ctx, const double* d_pts, long long n, int axis_x, int axis_y, const double* h_poly, int n_verts, int inside,
                    unsigned char* d_mask, long long* d_index, long long* d_count, void* stream);

/* Voxel grids, voxel down-sampling and voxel box meshes (csrc/voxel.hip; definition in DESIGN §4, restated in tests/voxel_oracle.py and
 * csrc/voxel_cell.h). Open3D's `VoxelGrid.create_from_point_cloud_within_bounds`, `create_from_point_cloud`, `voxel_down_sample` and the
 * cube mesh of the reference's `scripts/pcd_postprocessing/voxelization.py`; parity with an Open3D binary is unpinned. float64, contraction off.
 * One call serves n_clouds = E clouds in one buffer d_pts [n][3] float64, cloud e = points h_offsets[e] .. h_offsets[e + 1] - 1 (h_offsets
 * [E + 1] int64 in HOST memory, starting at 0). h_grids [G][7] float64 in HOST memory = origin = min_bound [3], max_bound [3], voxel_size
 * s per grid: G = 1 grid for all clouds (per_cloud == 0) or G = E, one per cloud. n_a = floor((max_a - min_a) / s) + 1 voxels per axis.
 * A point is kept iff every coordinate is finite and min_a <= p_a <= max_a on every axis; its index is i_a = floor((p_a - min_a) / s), a
 * true division; its voxel key (i_x n_y + i_y) n_z + i_z.
 * im_voxel_max_points: the most points of one call (2^26).
 * im_voxel_bounds: d_bounds [E][6] float64 = min x y z, max x y z of every cloud's points with three finite coordinates (+inf x 3, -inf x 3
 *   without one).
 * im_voxel_keys: d_key [n] int64 = the first key of the point's cloud (the voxels of the grids before it: e * n_x n_y n_z under one grid,
 *   the prefix sum of the per-cloud products otherwise) + the voxel key, or 2^63 - 1 for a point that is not kept; d_dropped [E] int64 =
 *   the points of every cloud that are not kept. The caller sorts the keys (stable, ascending as signed integers).
 * im_voxel_reduce: d_sorted_keys, d_perm [n] int64 = the sorted keys and the permutation (sorted position -> point). d_nvox [E + 1] int64
 *   receives the first voxel of every cloud and, at [E], the number of voxels V. The voxels of all clouds are listed one cloud behind the
 *   other in ascending key. Every other output is sized [n] rows by the caller, receives V rows and may be NULL (then it is not
 *   written): d_grid_index [.][3] int32, d_count [.] int32, d_first [.] int32 = the voxel's first point, counted from its cloud's first
 *   point, d_mean_pts / d_mean_colors / d_mean_normals [.][3] float64 = sum / count of the voxel's rows of d_pts / d_colors / d_normals
 *   ([n][3] float64, each may be NULL: then its mean is not written), every column summed in ascending point index from +0.0.
 * im_voxel_mesh_corners: one grid h_grid [7], d_grid_index [V][3] int32 in ascending voxel key; d_corner_keys [8 V] int64 = for voxel v
 *   and local corner l at 8 v + l the key (c_x (n_y + 1) + c_y)(n_z + 1) + c_z of c = grid_index + d(l), d(l) = (l & 1, (l >> 2) & 1,
 *   (l >> 1) & 1). The caller sorts them (stable).
 * im_voxel_mesh: d_sorted_keys, d_perm [8 V] int64 of that sort; d_n_vertices [1] int64 = the number of unique corners U; d_vertices
 *   [8 V][3] float64 receives U rows origin + c * s in ascending corner key; d_vertex_colors [8 V][3] float64 (written only when it and
 *   d_colors [V][3] float64 are given) the mean of the colours of the at most 8 voxels that share the corner, summed in ascending voxel
 *   from +0.0; d_triangles [12 V][3] int32 = per voxel the triangles (4,7,5) (4,6,7) (0,2,4) (2,6,4) (0,1,2) (1,3,2) (1,5,7) (1,7,3)
 *   (2,3,7) (2,7,6) (0,4,1) (1,4,5) of its local corners, as vertex numbers.
 * Keys, permutations and grid indices that are none give meaningless figures but no access outside a buffer.
 * The calls wait for the upload of their tables, then enqueue. All return -77, without launching and with the outputs untouched, for a
 * null required pointer, a voxel size that is not finite or not > 0, a bound that is not finite, max < min, offsets that do not start
 * at 0 or descend, more than 2^26 points, E outside 0..65535, grids that hold more than 2^62 voxels together (under one grid: n_x n_y n_z
 * E), a mesh grid with more than 2^62 corner keys, V < 0 or 8 V > 2^27. E == 0 (V == 0) returns 0 and launches nothing; so does n == 0,
 * which zeroes d_dropped and d_nvox. */
int im_voxel_max_points(void);
int im_voxel_bounds(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, double* d_bounds, void* stream);
int im_voxel_keys(im_ctx* ctx, const double* d_pts, const long long* h_offsets, int n_clouds, const double* h_grids, int per_cloud, long long* d_key,
                  long long* d_dropped, void* stream);
int im_voxel_reduce(im_ctx* ctx, const long long* h_offsets, int n_clouds, const double* h_grids, int per_cloud, const long long* d_sorted_keys,
                    const long long* d_perm, const double* d_pts, const double* d_colors, const double* d_normals, long long* d_nvox,
                    int32_t* d_grid_index, int32_t* d_count, int32_t* d_first, double* d_mean_pts, double* d_mean_colors, double* d_mean_normals,
                    void* stream);
int im_voxel_mesh_corners(im_ctx* ctx, const double* h_grid, const int32_t* d_grid_index, long long n_voxels, long long* d_corner_keys, void* stream);
int im_voxel_mesh(im_ctx* ctx, const double* h_grid, long long n_voxels, const double* d_colors, const long long* d_sorted_keys, const long long* d_perm,
                  long long* d_n_vertices, double* d_vertices, double* d_vertex_colors, int32_t* d_triangles, void* stream);

/* Triangle-mesh filters, the convex-hull crop and uniform mesh sampling (csrc/mesh.hip; definitions in DESIGN §4, restated in
 * tests/mesh_oracle.py and csrc/mesh_tri.h): what the reference's `MeshingPoisson.run()` does behind the Poisson solve. Parity with an
 * Open3D binary is unpinned. Vertices, colours, normals [V][3] float64; triangles [T][3] int32; float64 arithmetic with contraction off.
 * im_mesh_max_items: the most vertices, triangles or samples of one call (2^26). im_mesh_hull_chunk: facets staged in LDS at a time (512).
 * im_mesh_select: a triangle is kept iff d_triangle_keep [T] uint8 (NULL = all) allows it, each of its three indices lies in [0, V),
 *   is - through d_vertex_merge [V] int32 (NULL = identity; vertex -> the vertex that stands for it) - again in [0, V) and allowed by
 *   d_vertex_keep [V] uint8 (NULL = all), and, with drop_degenerate, the three are distinct. A vertex is kept iff d_vertex_keep allows it
 *   and, with drop_unreferenced, a kept triangle references it. d_vertex_map [V] int32 = the new number of every vertex, -1 where dropped;
 *   d_vertex_list [V] int32 = the kept vertices in ascending old index (the first d_counts [0] are written); d_triangles_out [T][3] int32
 *   = the kept triangles in their old order, renumbered, and d_triangle_pos [T] int32 their old positions (the first d_counts [1]);
 *   d_counts [2] int64. A triangle with an index outside [0, V) is skipped: it is dropped.
 * im_mesh_triangle_keys: d_key0, d_key1 [T] int64 = a and b << 32 | c of the index triple rotated to smallest-index-first (orientation
 *   counts). im_mesh_vertex_keys: d_key0..2 [V] int64 = the bits of x, y, z with -0.0 as +0.0; a vertex with a NaN coordinate gets
 *   (0x7ff8000000000000, its index, 0) and equals nothing. im_mesh_edge_keys: d_keys [3 T] int64, item 3 t + e = min << 32 | max of
 *   corners e and (e + 1) % 3 of triangle t. None of the three reads a vertex through an index.
 * im_mesh_first_of_segment: d_key0 (and d_key1, d_key2 or NULL) [n] int64 in item order, d_perm [n] int64 = sorted position -> item of
 *   successive stable sorts by the last key first. d_first [n] int32 = per item the first item (lowest index) of the run of equal keys
 *   it lies in, d_keep [n] uint8 = the item is that first one; either may be NULL.
 * im_mesh_edge_census: d_sorted_keys [n] int64 (n <= 3 * 2^26); d_count [1] int64 = the keys that occur more than twice.
 * im_mesh_in_hull: h_facets [F][4] float64 in HOST memory (n_x, n_y, n_z, d; scipy.spatial.ConvexHull.equations), 1 <= F <= 2^22;
 *   d_inside [n] uint8 = max_f (((n_x x + n_y y) + n_z z) + d) <= 0, the maximum running in facet order from -inf; a NaN value sticks,
 *   so a point with a NaN coordinate is outside.
 * im_mesh_sample_table: area_t = 0.5 |(v1 - v0) x (v2 - v0)|, 0 when not finite or when an index lies outside [0, V) (the triangle is
 *   skipped); q_t = floor(area_t / max area * 2^32) as int64, c_t their inclusive prefix sums (integers: exact in any order), C = c_T;
 *   d_count_end [T] int64 = rint(c_t / C * N): sample i belongs to the first triangle with d_count_end > i. d_area [T] float64 (NULL =
 *   not wanted) the areas, *h_total (HOST, NULL = not wanted) = C. The call waits for C before it writes an output.
 * im_mesh_sample: d_points [N][3] = (a v0 + b v1) + c v2 with s = sqrt(r1), a = 1 - s, b = s (1 - r2), c = s r2; r1, r2 = the top 53
 *   bits times 2^-53 of splitmix64's finaliser of seed + (2 i + 1) g and seed + (2 i + 2) g, g = 0x9E3779B97F4A7C15: a function of
 *   (seed, i) alone. d_colors [N][3] (NULL, or no d_vertex_colors: not written) likewise; d_normals [N][3] (NULL = not wanted) the
 *   same blend of d_vertex_normals, not renormalised, or without them the triangle's cross / |cross|; d_triangle_index [N] int32 (NULL =
 *   not wanted). An index outside [0, V) of a triangle the table leads to is clamped.
 * Keys that are not sorted, a permutation that is none, a table that is none give meaningless figures but no access outside a buffer.
 * All return -78, without launching and with the outputs untouched, for a null required pointer, a negative count, V, T, n or N above
 * 2^26, F outside 1..2^22, a facet that is not finite, samples (N > 0) of a mesh with no vertex or no triangle; im_mesh_sample_table
 * returns -78 with the outputs untouched, after its area pass, when N > 0 and C == 0. Zero-size calls return 0 and launch nothing
 * (im_mesh_select and im_mesh_edge_census zero their counts). */
int im_mesh_max_items(void);
int im_mesh_hull_chunk(void);
int im_mesh_select(im_ctx* ctx, const unsigned char* d_vertex_keep, long long n_vertices, const int32_t* d_triangles, long long n_triangles,
                   const int32_t* d_vertex_merge, const unsigned char* d_triangle_keep, int drop_degenerate, int drop_unreferenced, int32_t* d_vertex_map,
                   int32_t* d_vertex_list, int32_t* d_triangles_out, int32_t* d_triangle_pos, long long* d_counts, void* stream);
int im_mesh_triangle_keys(im_ctx* ctx, const int32_t* d_triangles, long long n_triangles, long long* d_key0, long long* d_key1, void* stream);
int im_mesh_vertex_keys(im_ctx* ctx, const double* d_vertices, long long n_vertices, long long* d_key0, long long* d_key1, long long* d_key2, void* stream);
int im_mesh_edge_keys(im_ctx* ctx, const int32_t* d_triangles, long long n_triangles, long long* d_keys, void* stream);
int im_mesh_first_of_segment(im_ctx* ctx, long long n, const long long* d_key0, const long long* d_key1, const long long* d_key2, const long long* d_perm,
                             int32_t* d_first, unsigned char* d_keep, void* stream);
int im_mesh_edge_census(im_ctx* ctx, const long long* d_sorted_keys, long long n_items, long long* d_count, void* stream);
int im_mesh_in_hull(im_ctx* ctx, const double* d_points, long long n_points, const double* h_facets, int n_facets, unsigned char* d_inside, void* stream);
int im_mesh_sample_table(im_ctx* ctx, const double* d_vertices, long long n_vertices, const int32_t* d_triangles, long long n_triangles, long long n_samples,
                         double* d_area, long long* d_count_end, long long* h_total, void* stream);
int im_mesh_sample(im_ctx* ctx, const double* d_vertices, long long n_vertices, const int32_t* d_triangles, long long n_triangles, const long long* d_count_end,
                   long long n_samples, long long seed, const double* d_vertex_colors, const double* d_vertex_normals, double* d_points, double* d_colors,
                   double* d_normals, int32_t* d_triangle_index, void* stream);

/* Poisson surface reconstruction of an oriented cloud on the dense grid of the finest octree level (csrc/poisson.hip; definition in
 * DESIGN §4, restated in tests/poisson_oracle.py and csrc/poisson_node.h). It stands in for Open3D's solve in the reference's
 * `post_processing/open3d_fun.py:191-203` (`MeshingPoisson.poisson_meshing`: `create_from_point_cloud_poisson(pcd, depth, width=0,
 * scale=1.1, linear_fit=False)` and its densities). Open3D's adaptive-octree solver is not reproduced and parity with an Open3D binary
 * is unpinned. A grid is h_grid [4] float64 in HOST memory (origin x, y, z and the cell size h > 0) and a depth in [2, 9]: R = 2^depth
 * cells and M = R + 1 nodes per axis, node (i, j, k) at (k M + j) M + i. Fields are [M^3] float64 device arrays of the caller.
 * float64 arithmetic with contraction off.
 * im_poisson_max_depth: 9. im_poisson_max_points: the most samples of a splat and vertices or triangles of an extraction (2^26).
 * im_poisson_splat: d_fields [4][M^3] = W, V_x, V_y, V_z. Per sample and axis u = (p - o) / h, the cell c = floor u clamped to
 *   [0, R - 1], the fraction t = u - c clamped to [0, 1]; the unit normal n / sqrt((n_x^2 + n_y^2) + n_z^2); at each of the 8 nodes of
 *   the cell the weight w = (w_x w_y) w_z, w_a = t_a or 1 - t_a; W receives rint(w 2^32) and V_a rint((w n_a) 2^32) as int64 (a NaN adds
 *   nothing), summed by integer atomics - exact in any order, below 2^58 for 2^26 samples - and the fields are the sums times 2^-32.
 * im_poisson_divergence: d_vectors [3][M^3]; d_rhs = (((V_x[i+1] - V_x[i-1]) + (V_y[j+1] - V_y[j-1])) + (V_z[k+1] - V_z[k-1])) / (2 h)
 *   on the interior nodes, 0 on the boundary.
 * im_poisson_jacobi: d_out = u + 6/7 (((s - h2 f) / 6) - u) on the interior nodes, s = ((((x- + x+) + y-) + y+) + z-) + z+ of u, and u
 *   on the boundary; h2 is the squared node spacing of the level. d_out may not be d_u.
 * im_poisson_restrict: d_residual [M^3] = f - (s - 6 u) / h2 (0 on the boundary), then d_coarse_f [Mc^3], Mc = 2^(depth-1) + 1 = its
 *   full weighting (1/4 a + 1/2 b) + 1/4 c along x, then y, then z on the interior coarse nodes, 0 on the boundary. d_residual may be
 *   neither d_u nor d_f.
 * im_poisson_prolong: d_u [M^3] += the trilinear interpolation of d_coarse_e [Mc^3] along x, then y, then z (a node between two coarse
 *   nodes takes 1/2 (a + b)), on the interior nodes.
 * im_poisson_coarse: the level of 3 nodes per axis: d_u [27] = 0 but for its centre, (h2 f) / -6.
 * im_poisson_reduce: d_out [ceil(n / 1024)]: per chunk of 1024 items v = a, or a b with d_b (NULL = none), zero beyond n: lane t of 256
 *   takes ((v[t] + v[t+256]) + v[t+512]) + v[t+768], then lane t += lane t + s for s = 128 .. 1. Applied again to its own output until
 *   one item is left it is the ordered sum of the iso-value, iso = sum (W chi) / sum W.
 * im_poisson_census: a node is inside iff chi < iso. d_mask [M^3] uint8: bit d - 1 = the edge from the node towards direction d = 1..7
 *   (bit 0 of d = +x, bit 1 = +y, bit 2 = +z) stays in the grid and its ends differ; d_base [M^3] int32 = the crossing edges of all nodes
 *   before it (the first vertex of the node); d_counts [2] int64 = the vertices and the triangles.
 * im_poisson_extract: d_vertices [V][3], d_weights [V] in ascending edge key 8 node + d: t = (iso - f_a) / (f_b - f_a) from the lower
 *   node a, position (o + i h) + t (step h) per axis, weight w_a + t (w_b - w_a) of d_weight_field. d_triangles [T][3] int32 ordered by
 *   (cell, tetrahedron, triangle): the six Kuhn tetrahedra of a cell in lexicographic order of their axis orders, the cases by rule
 *   (poisson_node.h), wound so that the normal points towards higher chi. d_mask and d_base are the census's; ones that are not lead to
 *   meaningless figures but to no access outside a buffer.
 * All return -80, without launching and with the outputs untouched, for a null required pointer, a depth outside [2, 9], a negative
 * count, more than 2^26 points, vertices or triangles, a grid that is not finite or has h <= 0, and buffers that may not coincide.
 * Zero-size calls return 0 and launch nothing. */
int im_poisson_max_depth(void);
int im_poisson_max_points(void);
int im_poisson_splat(im_ctx* ctx, const double* d_points, const double* d_normals, long long n_points, const double* h_grid, int depth, double* d_fields, void* stream);
int im_poisson_divergence(im_ctx* ctx, const double* d_vectors, int depth, double h, double* d_rhs, void* stream);
int im_poisson_jacobi(im_ctx* ctx, const double* d_u, const double* d_f, int depth, double h2, double* d_out, void* stream);
int im_poisson_restrict(im_ctx* ctx, const double* d_u, const double* d_f, int depth, double h2, double* d_residual, double* d_coarse_f, void* stream);
int im_poisson_prolong(im_ctx* ctx, const double* d_coarse_e, int depth, double* d_u, void* stream);
int im_poisson_coarse(im_ctx* ctx, const double* d_f, double h2, double* d_u, void* stream);
int im_poisson_reduce(im_ctx* ctx, const double* d_a, const double* d_b, long long n, double* d_out, void* stream);
int im_poisson_census(im_ctx* ctx, const double* d_chi, double iso, int depth, unsigned char* d_mask, int32_t* d_base, long long* d_counts, void* stream);
int im_poisson_extract(im_ctx* ctx, const double* d_chi, const double* d_weight_field, double iso, int depth, const double* h_grid, const unsigned char* d_mask,
                       const int32_t* d_base, long long n_vertices, long long n_triangles, double* d_vertices, double* d_weights, int32_t* d_triangles, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICEMATCH_H */
