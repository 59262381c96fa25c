/*
 * stego_crf.h - C ABI of the fully-connected CRF the reference evaluates with, exported by the same libstego_corr.so.
 *
 * Replaces src/crf.py:37-45 of the reference (pydensecrf's DenseCRF2D: unary_from_softmax, addPairwiseGaussian(sxy = POS_XY_STD,
 * compat = POS_W), addPairwiseBilateral(sxy = Bi_XY_STD, srgb = Bi_RGB_STD, compat = Bi_W), inference(MAX_ITER)) for a batch of
 * images, on the device:
 *     U  = -log(clip(p, 1e-5, 1)),   Q0 = softmax_c(-U)
 *     Q <- softmax_c(-U + pos_w * K_g(Q) + bi_w * K_b(Q))              (n_iter times, Potts compatibility)
 *     K(Q) = s * L(s * Q),  s = 1 / sqrt(L(1) + 1e-20)                  (densecrf NORMALIZE_SYMMETRIC)
 * where L is the permutohedral-lattice Gaussian filter (Adams, Baek, Davis 2010) in densecrf's form, on the features
 *     K_g: (x / pos_xy_std, y / pos_xy_std)                              d = 2
 *     K_b: (x / bi_xy_std, y / bi_xy_std, B / bi_rgb_std, G / bi_rgb_std, R / bi_rgb_std)     d = 5
 * csrc/dense_crf.hip has the construction (embedding, sort, vertices, neighbours) and the per-iteration kernels.  The result is
 * bitwise identical run to run (no float atomics, no hash table).  Arithmetic is fp32 but for the softmax over c and the log of the
 * unary, which are evaluated in double and rounded once (the mean-field multiplies what each iteration's rounding adds).
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code.
 */
#ifndef STEGO_CRF_H
#define STEGO_CRF_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_CRF_LIMITS = 20,  /* C outside [1, STEGO_CRF_MAX_C] or H * W * 6 >= 2^31                                   */
    STEGO_ERR_CRF_RANGE = 21    /* a lattice coordinate could leave the packed 64-bit key (image too large for its stds) */
};

#define STEGO_CRF_MAX_C 64

typedef struct StegoCrfDesc {
    int32_t B, C, H, W;          /* images (1 .. 65535), labels (1 .. STEGO_CRF_MAX_C), rows, columns   */
    int32_t n_iter;              /* mean-field iterations (crf.py:14 MAX_ITER = 10); 0 = softmax(-U)    */
    float pos_w;                 /* crf.py:15 POS_W = 3                                                  */
    float pos_xy_std;            /* crf.py:16 POS_XY_STD = 1                                             */
    float bi_w;                  /* crf.py:17 Bi_W = 4                                                   */
    float bi_xy_std;             /* crf.py:18 Bi_XY_STD = 67                                             */
    float bi_rgb_std;            /* crf.py:19 Bi_RGB_STD = 3                                             */
} StegoCrfDesc;

/* Bytes of workspace stego_crf_run needs for `desc`: sized for the worst case of N * (d + 1) lattice vertices per image (0 for an
 * invalid descriptor).  Host only: no device is touched. */
size_t stego_crf_workspace_bytes(const StegoCrfDesc* desc);

/* crf.py:22-45 for B images at once.
 *   bgr_u8 : [B, H, W, 3] uint8, the image in BGR order (crf.py:23, `[:, :, ::-1]`)
 *   probs  : [B, C, H, W] float32 label probabilities at the image's resolution (crf.py:27-29: the softmax of the resized logits)
 *   q_out  : [B, C, H, W] float32, the marginals Q after n_iter iterations (crf.py:42-44)
 *   workspace : stego_crf_workspace_bytes(desc) bytes, 256-byte aligned
 * Returns STEGO_ERR_SHAPE (B, H, W <= 0, B > 65535, n_iter < 0, a std <= 0 or not finite), STEGO_ERR_CRF_LIMITS, STEGO_ERR_CRF_RANGE,
 * STEGO_ERR_NULL, STEGO_ERR_WORKSPACE; every check is on the host, before anything is enqueued. */
int stego_crf_run(const StegoCrfDesc* desc, const uint8_t* bgr_u8, const float* probs, float* q_out, void* workspace,
                  size_t workspace_bytes, stego_stream_t stream);

/* Test hook: the bilateral (which = 1) or Gaussian (which = 0) lattice of image `b` as stego_crf_run built it in `workspace`.
 * Writes the number of vertices to *n_vertices and, when keys is not NULL, the first min(M, max_keys) packed vertex keys in ascending
 * order (coordinate i + 2^(bits - 1) in bits [i * bits, (i + 1) * bits), bits = 32 for d = 2, 12 for d = 5).  Synchronises `stream`. */
int stego_crf_lattice_info(const StegoCrfDesc* desc, const void* workspace, size_t workspace_bytes, int32_t b, int32_t which,
                           int32_t* n_vertices, uint64_t* keys, int32_t max_keys, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
