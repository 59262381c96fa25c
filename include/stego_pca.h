/*
 * stego_pca.h - C ABI of the feature pictures: the three-principal-component false colouring of a backbone feature map or of the
 * segmentation code, exported by the same libstego_corr.so.
 *
 * Replaces, on the device, what the reference draws on the host (src/train_crf.py:145-150):
 *     p = PCA(n_components=3).fit_transform(code);  imshow(clip((p + 1) / 2, 0, 1))
 *
 * The map is float32 [B, C, h, w] with arbitrary element strides; a token is one (b, y, x), its row the C channels.  The tokens are
 * fitted in groups: STEGO_PCA_PER_IMAGE has one group per image (G = B, n = h w tokens each: the reference's), STEGO_PCA_JOINT one
 * group of all n = B h w tokens (G = 1: a batch shares its colours).  Five stages, each one launch or two, no atomics anywhere:
 * repeat calls are bitwise equal.
 *
 *   (a) mean[g][c]      the fp64 sum over the group's tokens / n, stored as float32.  Per slab of tokens fp64 partial sums, added in
 *                       slab order.
 *   (b) cov[g][i][j]    sum over the tokens of (x_i - mean_i)(x_j - mean_j) / (n - 1), fp64 [G, C, C].  The mean (the float32 of (a))
 *                       is subtracted in fp32 while the tokens are staged, the products run on the fp32-input matrix instruction
 *                       (32x32x2), an fp32 accumulator tile takes at most STEGO_PCA_FOLD = 1024 tokens before it is added to an fp64
 *                       one.  Only the 32 x 32 tiles with j >= i are computed; the tokens of a group are split into S slabs whose
 *                       fp64 tiles are added in slab order by a second launch, which mirrors them.
 *   (c) basis, stats    the three largest eigenpairs of cov[g], in fp64, one workgroup per group: subspace iteration on
 *                       min(8, C) columns from a fixed start (an integer hash of (channel, column), no random numbers), n_iter times
 *                       Z = cov Q and two passes of modified Gram-Schmidt (a column that loses 12 digits to the columns in front of
 *                       it becomes a zero column), then Rayleigh-Ritz on the projected 8 x 8 matrix by cyclic Jacobi, sorted
 *                       descending.  Sign: the loading of largest magnitude of a component is positive, ties go to the lowest
 *                       channel (sklearn's svd_flip on the components).  A component with lambda_i <= 2^-20 trace(cov) is dropped:
 *                       its basis row is zero and its statistics are zero.
 *                       basis float32 [G, 3, C]; stats float32 [G, 3, 3] = (lambda_i, lambda_i / trace, |cov v - lambda_i v| /
 *                       lambda_1 from fp64): convergence can be judged from stats with no synchronising call.
 *   (d) scores, range   scores[b][y][x][i] = sum_c (x_c - mean_g[c]) basis_g[i][c], float32 [B, h, w, 3]; range[g][i] = (min, max)
 *                       of component i over the group's tokens, float32 [G, 3, 2], from per-workgroup partials (NaNs passed over).
 *                       With the model of an earlier fit in `mean` / `basis` this is the first and only read of the map.
 *   (e) the picture     one launch that reads only the scores.  Per output pixel the three scores are resized to H x W -
 *                       STEGO_PCA_BILINEAR: ATen's align_corners=False source index in fp32 (scale = in / out, s = max(scale (dst +
 *                       0.5) - 0.5, 0), taps i0 = min((int)s, in - 1) and i0 + (i0 < in - 1)); STEGO_PCA_NEAREST: the source
 *                       min((int)floorf(dst * scale), in - 1) - and mapped to v': STEGO_PCA_UNIT (s + 1) / 2 (the reference's, meant
 *                       for L2-normalised codes), STEGO_PCA_RANGE (s - lo) / (hi - lo) with the group's range of component i, 0 where
 *                       hi == lo.  u8 = (uint8) clamp(v' * 255, 0, 255), truncated, NaN -> 0: stego_render's byte rules.  The target
 *                       is stego_render's as well: a base pointer with byte strides per image and row and no alignment, exactly the
 *                       B * H * 3 W bytes of the panel written, row bodies as 16-byte stores of aligned addresses staged through
 *                       LDS, heads and tails as byte stores.
 *
 * No float tensor of the output's resolution and no [B, C, H, W] tensor is ever written: what leaves the kernels is mean, cov and its
 * partial tiles, basis, stats, scores, range and the bytes.
 *
 * Workspace.  S = min(ceil(n / 1024), max(1, 16 / G)) slabs of ceil(n / S) tokens rounded up to 1024: at most 16 slab tiles sets
 * are ever kept beside one per group.  With nt = ceil(C / 32) the partial tiles take G S nt (nt + 1) / 2 * 8 KB - for a joint fit
 * (G = 1) at C = 768 at most 16 * 300 * 8 KB = 39.3 MB, however many tokens; for a per-image fit at most max(G, 16) / G times half of
 * what cov itself takes.  The means' partial sums (G S C doubles) and the ranges' partials (at most max(B, 8192) * 6 floats) are small.
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_PCA_H
#define STEGO_PCA_H

#include "stego_render.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_PCA_DIM = 170,        /* C outside [3, STEGO_PCA_MAX_C]                                                               */
    STEGO_ERR_PCA_SIZE = 171,       /* B outside [1, 65535], h or w outside [1, STEGO_PCA_MAX_SIDE], B * h * w > STEGO_PCA_MAX_TOKENS,
                                       fewer than 4 tokens in a group, or H or W outside [1, STEGO_STITCH_MAX_SIDE]                 */
    STEGO_ERR_PCA_ITER = 172,       /* n_iter outside [1, STEGO_PCA_MAX_ITER]                                                       */
    STEGO_ERR_PCA_MODE = 173        /* group, resize or scale outside their two values                                              */
};

enum { STEGO_PCA_PER_IMAGE = 0, STEGO_PCA_JOINT = 1 };      /* StegoPcaDesc.group  */
enum { STEGO_PCA_BILINEAR = 0, STEGO_PCA_NEAREST = 1 };     /* StegoPcaDesc.resize */
enum { STEGO_PCA_UNIT = 0, STEGO_PCA_RANGE = 1 };           /* StegoPcaDesc.scale  */

#define STEGO_PCA_MAX_C 768
#define STEGO_PCA_MAX_SIDE 4096
#define STEGO_PCA_MAX_TOKENS (1 << 28)
#define STEGO_PCA_MAX_ITER 256
#define STEGO_PCA_DEFAULT_ITER 32
#define STEGO_PCA_FOLD 1024

typedef struct StegoPcaDesc {
    int32_t B, C, h, w;             /* the map: images (1 .. 65535), channels (3 .. 768), rows, columns (1 .. 4096)  */
    int32_t H, W;                   /* the picture's rows, columns (1 .. STEGO_STITCH_MAX_SIDE)                       */
    int32_t group;                  /* STEGO_PCA_PER_IMAGE / STEGO_PCA_JOINT                                          */
    int32_t n_iter;                 /* iterations of stage (c) (1 .. 256; STEGO_PCA_DEFAULT_ITER)                     */
    int32_t resize;                 /* STEGO_PCA_BILINEAR / STEGO_PCA_NEAREST                                         */
    int32_t scale;                  /* STEGO_PCA_UNIT / STEGO_PCA_RANGE                                               */
    int64_t out_stride_n, out_stride_h;     /* of the picture's target, in bytes                                      */
} StegoPcaDesc;

/* Bytes of workspace stego_pca_fit and stego_pca_scores need for `desc` (the larger of the two); 0 for an invalid descriptor.
 * Host only. */
size_t stego_pca_workspace_bytes(const StegoPcaDesc* desc);

/* Stages (a) - (c): five launches.
 *   map       : float32 [B, C, h, w] with arbitrary strides
 *   mean      : float32 [G, C]
 *   cov       : float64 [G, C, C]
 *   basis     : float32 [G, 3, C]
 *   stats     : float32 [G, 3, 3]
 *   workspace : at least stego_pca_workspace_bytes(desc) bytes, 16-byte aligned, needs no initialisation
 * G = B (PER_IMAGE) or 1 (JOINT).  Returns STEGO_ERR_NULL, STEGO_ERR_PCA_*, STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN (map, mean, basis
 * or stats not 4-byte aligned, cov not 8-byte, the workspace not 16-byte aligned). */
int stego_pca_fit(const StegoPcaDesc* desc, const StegoMap* map, float* mean, double* cov, float* basis, float* stats, void* workspace,
                  size_t workspace_bytes, stego_stream_t stream);

/* Stage (d): two launches.  `mean` and `basis` are a model's, [G, C] and [G, 3, C] with the descriptor's G: a joint model applies to
 * any batch.
 *   scores    : float32 [B, h, w, 3], dense
 *   range     : float32 [G, 3, 2]
 * Returns as stego_pca_fit. */
int stego_pca_scores(const StegoPcaDesc* desc, const StegoMap* map, const float* mean, const float* basis, float* scores, float* range,
                     void* workspace, size_t workspace_bytes, stego_stream_t stream);

/* Stage (e): one launch.
 *   scores : float32 [B, h, w, 3] of stego_pca_scores
 *   range  : float32 [G, 3, 2] (STEGO_PCA_RANGE), else not read
 *   out    : the target, B * H * 3 * W bytes at out + b * out_stride_n + y * out_stride_h + 3 * x
 * Returns STEGO_ERR_NULL, STEGO_ERR_PCA_*, STEGO_ERR_ALIGN (scores or range not 4-byte aligned). */
int stego_pca_paint(const StegoPcaDesc* desc, const float* scores, const float* range, uint8_t* out, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
