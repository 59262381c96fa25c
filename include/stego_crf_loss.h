/*
 * stego_crf_loss.h - C ABI of the fused ContrastiveCRFLoss (forward and backward), exported by the same libstego_corr.so.
 *
 * Replaces the chain train_segmentation.py:202-208 / modules.py:437-469 of the reference,
 *     crf(resize(img, 56), norm(resize(code, 56))).mean()
 * which builds two full maps of which crf_samples cells are read, a [B, G, N, N] tensor of guidance differences and several [B, N, N]
 * tensors, by one call of three launches that keeps only the N sampled rows, the [B, N, K] product k . x^ and the gradient.
 *
 * Inputs: a guidance map [B, G, hg, wg], a code map [B, K, h, w] (any strides) and N integer points (row, column) on an H x W grid,
 * the same points for every image.  For point n at (r, c):
 *   x_n  = the code interpolated at grid cell (r, c): the value F.interpolate(code, (H, W), mode="bilinear", align_corners=False) has
 *          there - scale = (float)in / out, src = max(scale * (dst + 0.5) - 0.5, 0), i0 = (int)src, i1 = i0 + (i0 < in - 1),
 *          l1 = src - i0, value h0 * (w0 * c00 + w1 * c01) + h1 * (w0 * c10 + w1 * c11): the rule of stego_probe.h, any ratio.  With
 *          (h, w) == (H, W) the weights are exactly 1, 0, 0, 0 and x_n is the stored vector.
 *   g_n  = the guidance, interpolated the same way from (hg, wg).
 *   x^_n = x_n / max(|x_n|, 1e-10) with STEGO_CRFLOSS_NORMALIZE (modules.norm), x_n without it (the module called directly).
 *   k_ab = w1 * exp(-d2_ab / (2 alpha) - |g_a - g_b|^2 / (2 beta)) + w2 * exp(-d2_ab / (2 gamma)) - shift, d2_ab the squared integer
 *          distance of the two points.
 *   per_image[i] = -(1 / N^2) sum_{a, b} k_ab (x^_a . x^_b) of image i,   loss = mean_i per_image[i].
 * Backward (k is symmetric): dL/dx^_a = -(2 / (B N^2)) sum_b k_ab x^_b; through the normalisation
 * dx_a = (dx^_a - (dx^_a . x^_a) x^_a) / max(|x_a|, 1e-10), and for |x_a| < 1e-10, as torch's clamp, dx_a = dx^_a / 1e-10 without the
 * projection; d_code is the transpose of the four-tap interpolation: every cell sums weight * dx_n over every tap of every point
 * that touches it (duplicate points count once each).  The guidance receives no gradient.
 *
 * Both GEMMs run on the fp32-input matrix instruction: exact fp32 products, fp32 accumulation.  No float atomics: the per-workgroup
 * loss partials are added in a fixed order in fp64, every cell's taps in the order of a sort, so repeat launches give the same bits.
 * Coordinates outside the grid cannot be checked on the host: the kernel clamps them to [0, H - 1] x [0, W - 1].
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream` (capturable into a
 * HIP graph), STEGO_OK or an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_CRF_LOSS_H
#define STEGO_CRF_LOSS_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_CRFLOSS_DIM = 80,     /* K outside [1, STEGO_CRFLOSS_MAX_K] or G outside [1, STEGO_CRFLOSS_MAX_G]                  */
    STEGO_ERR_CRFLOSS_POINTS = 81,  /* N outside [1, STEGO_CRFLOSS_MAX_POINTS]                                                  */
    STEGO_ERR_CRFLOSS_SIZE = 82,    /* B outside [1, 65535], or a side of the code, the guidance or the grid outside [1, MAX_SIDE] */
    STEGO_ERR_CRFLOSS_PARAM = 83,   /* alpha, beta or gamma not finite or <= 0; w1, w2 or shift not finite                       */
    STEGO_ERR_CRFLOSS_FLAGS = 84    /* an unknown flag bit                                                                       */
};

enum {
    STEGO_CRFLOSS_NORMALIZE = 1     /* x^ = x / max(|x|, 1e-10) (the training composition); without it x^ = x                    */
};

#define STEGO_CRFLOSS_MAX_K 128        /* code channels            */
#define STEGO_CRFLOSS_MAX_G 8          /* guidance channels        */
#define STEGO_CRFLOSS_MAX_POINTS 4096  /* sampled points           */
#define STEGO_CRFLOSS_MAX_SIDE 2048    /* rows / columns of a map  */
#define STEGO_CRFLOSS_LAUNCHES 3

typedef struct StegoCrfLossDesc {
    int32_t B;                   /* images (1 .. 65535)                                  */
    int32_t K;                   /* code channels (1 .. STEGO_CRFLOSS_MAX_K)             */
    int32_t G;                   /* guidance channels (1 .. STEGO_CRFLOSS_MAX_G)         */
    int32_t h, w;                /* code rows, columns                                   */
    int32_t hg, wg;              /* guidance rows, columns                               */
    int32_t H, W;                /* the grid the points live on                          */
    int32_t N;                   /* points (1 .. STEGO_CRFLOSS_MAX_POINTS)               */
    float alpha, beta, gamma;    /* > 0                                                  */
    float w1, w2, shift;
    int32_t flags;               /* STEGO_CRFLOSS_*                                      */
} StegoCrfLossDesc;

/* Bytes of workspace stego_crf_loss needs for `desc` (x^, k . x^, the point records, the sorted taps, the loss partials); 0 for an
 * invalid descriptor. */
size_t stego_crf_loss_workspace_bytes(const StegoCrfLossDesc* desc);

/* Host only: the LDS bytes of one workgroup and the number of workgroups of each of the three launches (prepare, pairs, finish) of a
 * call with a gradient.  Returns STEGO_OK, or the descriptor's error with both arrays zeroed.  Touches no device. */
int stego_crf_loss_plan(const StegoCrfLossDesc* desc, size_t lds_bytes[STEGO_CRFLOSS_LAUNCHES], int64_t workgroups[STEGO_CRFLOSS_LAUNCHES]);

/* Loss and gradient for B images.
 *   guidance  : float32 [B, G, hg, wg] with arbitrary strides
 *   code      : float32 [B, K, h, w] with arbitrary strides (the head's channels-last view goes in without a copy)
 *   coords    : int64 [2, N] contiguous: the rows, then the columns
 *   loss      : float32 [1]
 *   per_image : float32 [B], or NULL
 *   d_code    : NULL (forward only: the loss has the same bits), or float32 [B, K, h, w] described by its own four strides - it can
 *               take the code's layout; `data` is written.  Every element is written, cells no tap touches get 0.  It holds
 *               d loss / d code for a unit upstream.
 *   workspace : at least stego_crf_loss_workspace_bytes(desc) bytes, 16-byte aligned; needs no initialisation
 * Returns STEGO_ERR_NULL, STEGO_ERR_CRFLOSS_FLAGS, _DIM, _POINTS, _SIZE, _PARAM, STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN (a float pointer
 * not 4-byte aligned, coords not 8-byte aligned, the workspace not 16-byte aligned). */
int stego_crf_loss(const StegoCrfLossDesc* desc, const StegoMap* guidance, const StegoMap* code, const int64_t* coords, float* loss,
                   float* per_image, const StegoMap* d_code, void* workspace, size_t workspace_bytes, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
