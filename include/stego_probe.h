/*
 * stego_probe.h - C ABI of the fused probe head of STEGO's inference tail, exported by the same libstego_corr.so.
 *
 * Replaces the chain demo_segmentation.py:62-78 and eval_segmentation.py:124-138 of the reference run over full-resolution tensors:
 *     code = (code1 + code2.flip(dims=[3])) / 2                                    [B, K, h, w]
 *     code = F.interpolate(code, (H, W), mode="bilinear", align_corners=False)      [B, K, H, W]
 *     linear  = log_softmax(W code + b, 1)                                          (the 1x1 linear probe)
 *     cluster = log_softmax(alpha * normalize(code, dim=1) . normalize(clusters, dim=1), 1)   (ClusterLookup, log_probs=True)
 * in one launch that reads the low-resolution code and writes, per probe, one of: the log-probabilities, the probabilities (the CRF's
 * input, crf.py:27-29) or the label index of the first maximum (torch.argmax).
 *
 * The resize is torch's upsample_bilinear2d with align_corners=False: scale = (float)in / out, src = max(scale * (dst + 0.5) - 0.5, 0),
 * i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, and the value h0 * (w0 * c00 + w1 * c01) + h1 * (w0 * c10 + w1 * c11).  The
 * interpolation weights sum to 1, so the kernel projects the flip-averaged low-resolution code onto both probes (W c + b and
 * c . centroid) and interpolates the projections; the norm of the cluster probe comes from the interpolated K-channel code itself, so
 * opposite neighbouring vectors do not cancel through a Gram form.  Results are fp32 and bitwise repeatable (no atomics).
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_PROBE_H
#define STEGO_PROBE_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_PROBE_DIM = 40,    /* K outside [1, STEGO_PROBE_MAX_K], or an active probe's n outside [1, STEGO_PROBE_MAX_N]            */
    STEGO_ERR_PROBE_SIZE = 41,   /* B outside [1, 65535], h or w outside [1, STEGO_PROBE_MAX_CODE], H or W outside [1, STEGO_PROBE_MAX_OUT] */
    STEGO_ERR_PROBE_OUTPUT = 42  /* an output kind outside the enum below, or both probes skipped                                    */
};

/* What a probe writes. */
enum {
    STEGO_PROBE_SKIP = 0,        /* nothing: the probe's n, weights and output are not read (any n, NULL pointers)                   */
    STEGO_PROBE_LOG_PROBS = 1,   /* float32 [B, n, H, W]: log_softmax over n                                                          */
    STEGO_PROBE_PROBS = 2,       /* float32 [B, n, H, W]: softmax over n (the dense CRF's `probs`, include/stego_crf.h)               */
    STEGO_PROBE_ARGMAX = 3       /* int64 [B, H, W]: index of the first maximum of the LOG_PROBS values over n (torch.argmax)         */
};

#define STEGO_PROBE_MAX_K 128        /* code channels (MAX_CODE_DIM)                        */
#define STEGO_PROBE_MAX_N 64         /* labels per probe (STEGO_CRF_MAX_C)                  */
#define STEGO_PROBE_MAX_OUT 2048     /* output rows / columns                               */
#define STEGO_PROBE_MAX_CODE 65535   /* code rows / columns                                 */

typedef struct StegoProbeDesc {
    int32_t B;                   /* images (1 .. 65535)                                                  */
    int32_t K;                   /* code channels (1 .. STEGO_PROBE_MAX_K)                               */
    int32_t h, w;                /* code rows, columns                                                   */
    int32_t H, W;                /* output rows, columns (any size: up- or downsampling)                 */
    int32_t n_lin, n_clu;        /* labels of the linear and the cluster probe (1 .. STEGO_PROBE_MAX_N)  */
    int32_t lin_kind, clu_kind;  /* STEGO_PROBE_*                                                        */
    float alpha;                 /* cluster logits = alpha * cosine (ClusterLookup(code, alpha = 2))     */
} StegoProbeDesc;

/* Both probes for B images.
 *   code      : float32 [B, K, h, w] with arbitrary strides (the head's channels-last view goes in without a copy)
 *   code_flip : the code of the horizontally flipped images, same shape, or NULL (no flip average)
 *   lin_w     : float32 [n_lin, K] contiguous, lin_b : float32 [n_lin]   (linear_probe.weight[:, :, 0, 0], linear_probe.bias)
 *   centroids : float32 [n_clu, K] contiguous, already L2-normalised (F.normalize(cluster_probe.clusters, dim=1))
 *   lin_out, clu_out : contiguous outputs of the kind the descriptor names (float32 [B, n, H, W] or int64 [B, H, W]); every element
 *               is written, offsets are 64-bit
 * Returns STEGO_ERR_NULL (desc, code, an active probe's weights or output), STEGO_ERR_PROBE_DIM, STEGO_ERR_PROBE_SIZE,
 * STEGO_ERR_PROBE_OUTPUT, STEGO_ERR_ALIGN (a float pointer not 4-byte aligned, an ARGMAX output not 8-byte aligned). */
int stego_probe_head(const StegoProbeDesc* desc, const StegoMap* code, const StegoMap* code_flip, const float* lin_w, const float* lin_b,
                     const float* centroids, void* lin_out, void* clu_out, stego_stream_t stream);

/* Host only: the dynamic LDS bytes one workgroup of stego_probe_head uses for `desc` (0 for an invalid descriptor), and the output
 * tile (rows, columns) it was planned for.  Touches no device. */
size_t stego_probe_head_plan(const StegoProbeDesc* desc, int32_t* tile_rows, int32_t* tile_cols);

#ifdef __cplusplus
}
#endif

#endif
