/*
 * stego_rec.h - C ABI of the fused reconstruction loss (forward and backward), exported by the same libstego_corr.so.
 *
 * Replaces the chain train_segmentation.py:183-187 of the reference,
 *     rec_loss = -(norm(self.decoder(code)) * norm(feats)).sum(1).mean()
 * with decoder = Conv2d(K, C, 1), which writes the reconstructed map [B, C, h, w], its normalised copy, a normalised copy of feats and
 * their product, by one call of two launches that writes no [T, C] tensor at all.
 *
 * Tokens t = 0 .. T - 1 run over (b, y, x), T = B h w.  With x_t the code [K], f_t the feature [C], r_t = W x_t + b, eps = 1e-10:
 *     nr_t = max(|r_t|, eps)    nf_t = max(|f_t|, eps)    c_t = (r_t . f_t) / (nr_t nf_t)
 *     loss = -(1 / T) sum_t c_t
 *     g_t  = d loss / d r_t = -(1 / T) (f_t / nf_t - [|r_t| >= eps] c_t r_t / nr_t) / nr_t      (torch's clamp_min rule)
 *     d_code_t = W^T g_t        d_weight = sum_t g_t x_t^T  [C, K]        d_bias = sum_t g_t  [C]
 * feats receives no gradient (the backbone is frozen).
 *
 * All three contractions (r = X W^T, d_code = G W, d_weight = G^T X) run on the fp32-input matrix instruction: exact fp32 products,
 * fp32 accumulation; K and C are zero-padded to 32 inside the kernels.  Launch 1 (a workgroup per tile of 32 tokens) reads feats from
 * memory once: the tile stays in LDS from the norms to d_code, and r is computed again (K is small) instead of being kept; it leaves
 * alpha_t, beta_t (g_t = alpha_t f_t + beta_t r_t) of every token in the workspace.  Launch 2 forms d_weight / d_bias from them:
 * workgroup (one of at most STEGO_REC_MAX_WORKGROUPS token ranges, one 32-channel chunk) keeps its chunk's sum in registers over its
 * tiles; this is a second read of code and feats, served from the caches that launch 1 has just filled (both fit the 256 MB Infinity
 * Cache at the training shape).  No float atomics: a range's partial goes to its slab, and the workgroup that a counter shows to be
 * the last of its chunk adds the slabs in ascending order; the loss terms are added in fp64 in a fixed order: repeat launches give the
 * same bits.  A call with neither d_weight nor d_bias runs no such workgroup.
 *
 * Workspace: ranges * (CP K + CP) floats, CP = C rounded up to 32, + 2 floats per token + one double per tile + one counter per
 * chunk; at the training shape (B = 32, K = 70, C = 384, 28 x 28) 7,186,608 bytes, 0.19 of the 38.5 MB of feats.
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream` (capturable into a
 * HIP graph), STEGO_OK or an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_REC_H
#define STEGO_REC_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_REC_DIM = 140,        /* K outside [1, STEGO_REC_MAX_K] or C outside [1, STEGO_REC_MAX_C]                               */
    STEGO_ERR_REC_SIZE = 141        /* B outside [1, 65535], h or w outside [1, STEGO_REC_MAX_SIDE], or B h w > STEGO_REC_MAX_TOKENS */
};

#define STEGO_REC_MAX_K 128              /* code channels                                   */
#define STEGO_REC_MAX_C 1024             /* feature channels                                */
#define STEGO_REC_MAX_B 65535            /* images                                          */
#define STEGO_REC_MAX_SIDE 2048          /* rows / columns of the maps                      */
#define STEGO_REC_MAX_TOKENS (1 << 24)   /* B h w                                           */
#define STEGO_REC_TILE 32                /* tokens per tile                                 */
#define STEGO_REC_MAX_WORKGROUPS 64      /* token ranges of launch 2 = d_weight / d_bias slabs */
#define STEGO_REC_LAUNCHES 2

typedef struct StegoRecDesc {
    int32_t B;                   /* images (1 .. STEGO_REC_MAX_B)                    */
    int32_t K;                   /* code channels (1 .. STEGO_REC_MAX_K)             */
    int32_t C;                   /* feature channels (1 .. STEGO_REC_MAX_C)          */
    int32_t h, w;                /* rows, columns of both maps (1 .. STEGO_REC_MAX_SIDE) */
} StegoRecDesc;

/* Bytes of workspace stego_rec_loss needs for `desc` (the ranges' d_weight / d_bias slabs, the tokens' scalars and the tiles' loss terms); 0 for an
 * invalid descriptor. */
size_t stego_rec_loss_workspace_bytes(const StegoRecDesc* desc);

/* Host only: the LDS bytes of one workgroup and the number of workgroups of the two launches (tiles, finish) of a call with every
 * gradient.  Returns STEGO_OK, or the descriptor's error with both arrays zeroed.  Touches no device. */
int stego_rec_loss_plan(const StegoRecDesc* desc, size_t lds_bytes[STEGO_REC_LAUNCHES], int64_t workgroups[STEGO_REC_LAUNCHES]);

/* The loss and its gradients.
 *   code      : float32 [B, K, h, w] with arbitrary strides
 *   feats     : float32 [B, C, h, w] with arbitrary strides (the backbone's channels-last token view goes in without a copy; only
 *               stride_c == 1 is fast)
 *   weight    : float32 [C, K] contiguous (the 1 x 1 convolution's weight)
 *   bias      : float32 [C]
 *   loss      : float32 [1]
 *   d_code    : NULL, or float32 [B, K, h, w] described by its own four strides; `data` is written, every element
 *   d_weight  : NULL, or float32 [C, K] contiguous; written, not accumulated into
 *   d_bias    : NULL, or float32 [C]; written, not accumulated into
 *   workspace : at least stego_rec_loss_workspace_bytes(desc) bytes, 16-byte aligned; needs no initialisation
 * The gradients are those of a unit upstream.  The loss has the same bits whichever gradients are NULL.
 * Returns STEGO_ERR_NULL, STEGO_ERR_REC_DIM, STEGO_ERR_REC_SIZE, STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN (a float pointer not 4-byte
 * aligned, the workspace not 16-byte aligned). */
int stego_rec_loss(const StegoRecDesc* desc, const StegoMap* code, const StegoMap* feats, const float* weight, const float* bias,
                   float* loss, const StegoMap* d_code, float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes,
                   stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
