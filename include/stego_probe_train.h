/*
 * stego_probe_train.h - C ABI of the fused training tail of STEGO's two probes, exported by the same libstego_corr.so.
 *
 * Replaces the chain train_segmentation.py:199-224 of the reference runs on the detached code every training step:
 *     logits = F.interpolate(linear_probe(code), label.shape[-2:], mode="bilinear", align_corners=False)     [B, n_lin, H, W]
 *     linear_loss  = cross_entropy over the pixels with 0 <= label < n_lin (mean)
 *     cluster_loss = ClusterLookup(code, None)[0] = -mean_p max_n normalize(code)_p . normalize(clusters)_n  (at code resolution)
 * and their backward to linear_probe.weight, linear_probe.bias and cluster_probe.clusters, in one call of two launches that writes no
 * [B, n, H, W] tensor: the main kernel and a fixed-order reduction of its per-workgroup partial sums.
 *
 * Linear probe.  The interpolation weights sum to 1, so the logits of a pixel are the four-tap interpolation (the rule of
 * stego_probe.h, any ratio) of the low-resolution projections W c + b.  With g(p) = (softmax(logits_p) - onehot(label_p)) / n_valid on
 * the valid pixels and 0 elsewhere: loss = mean over the valid pixels of logsumexp(logits_p) - logits_p[label_p], d_lin_b = sum_p g(p),
 * d_lin_w = sum_p g(p) (x) code_interp(p).  No valid pixel at all: loss NaN and zero gradients (F.cross_entropy with ignore_index).
 *
 * Cluster probe.  x^ = code_p / max(|code_p|, 1e-12), c^ = clusters_n / max(|clusters_n|, 1e-12), a(p) the FIRST maximum of x^_p . c^_n
 * (torch.argmax), loss = -mean_p x^_p . c^_a(p).  The one-hot carries no gradient: dL/dc^_n = -(1/P) sum_{a(p) = n} x^_p, and through
 * the normalisation d_clusters_n = (dc^_n - (dc^_n . c^_n) c^_n) / max(|clusters_n|, 1e-12).
 *
 * All products are fp32 FMAs; the partial sums of the workgroups are added in a fixed order (in fp64, by the second launch).  No atomics:
 * repeat launches give the same bits.  Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work
 * enqueued on `stream` (capturable into a HIP graph), STEGO_OK or an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_PROBE_TRAIN_H
#define STEGO_PROBE_TRAIN_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_PTRAIN_DIM = 60,     /* K outside [1, STEGO_PTRAIN_MAX_K], or an active probe's n outside [1, STEGO_PTRAIN_MAX_N]          */
    STEGO_ERR_PTRAIN_SIZE = 61,    /* B outside [1, 65535], h or w outside [1, STEGO_PTRAIN_MAX_CODE], H or W outside [1, STEGO_PTRAIN_MAX_OUT] */
    STEGO_ERR_PTRAIN_PROBES = 62   /* n_lin == 0 and n_clu == 0: nothing to do                                                        */
};

#define STEGO_PTRAIN_MAX_K 128        /* code channels                                       */
#define STEGO_PTRAIN_MAX_N 64         /* labels per probe                                    */
#define STEGO_PTRAIN_MAX_OUT 2048     /* label rows / columns                                */
#define STEGO_PTRAIN_MAX_CODE 65535   /* code rows / columns                                 */

typedef struct StegoProbeTrainDesc {
    int32_t B;                   /* images (1 .. 65535)                                                                    */
    int32_t K;                   /* code channels (1 .. STEGO_PTRAIN_MAX_K)                                                */
    int32_t h, w;                /* code rows, columns                                                                     */
    int32_t H, W;                /* label rows, columns (any size: up- or downsampling; unused when n_lin == 0 but checked) */
    int32_t n_lin, n_clu;        /* labels of the linear and the cluster probe (1 .. STEGO_PTRAIN_MAX_N); 0 skips the probe */
} StegoProbeTrainDesc;

/* Bytes of workspace stego_probe_train needs for `desc` (the per-workgroup partial sums); 0 for an invalid descriptor. */
size_t stego_probe_train_workspace_bytes(const StegoProbeTrainDesc* desc);

/* Both probes' losses and parameter gradients for B images.
 *   code      : float32 [B, K, h, w] with arbitrary strides (the head's channels-last view goes in without a copy)
 *   label     : int64 [B, H, W] contiguous; a pixel counts iff 0 <= label < n_lin
 *   lin_w     : float32 [n_lin, K] contiguous, lin_b : float32 [n_lin]   (linear_probe.weight[:, :, 0, 0], linear_probe.bias)
 *   clusters  : float32 [n_clu, K] contiguous, NOT normalised (cluster_probe.clusters)
 *   losses    : float32 [2]: the linear loss, the cluster loss; the slot of a skipped probe is left untouched
 *   n_valid   : int64 [1]: the number of valid pixels (0 when the linear probe is skipped)
 *   d_lin_w [n_lin, K], d_lin_b [n_lin], d_clusters [n_clu, K] : float32, every element written
 *   workspace : at least stego_probe_train_workspace_bytes(desc) bytes, 8-byte aligned; needs no initialisation
 * A skipped probe's pointers (and `label` without the linear probe) may be NULL.
 * Returns STEGO_ERR_NULL, STEGO_ERR_PTRAIN_DIM, STEGO_ERR_PTRAIN_SIZE, STEGO_ERR_PTRAIN_PROBES, STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN
 * (a float pointer not 4-byte aligned; label, n_valid or the workspace not 8-byte aligned). */
int stego_probe_train(const StegoProbeTrainDesc* desc, const StegoMap* code, const int64_t* label, const float* lin_w, const float* lin_b,
                      const float* clusters, float* losses, int64_t* n_valid, float* d_lin_w, float* d_lin_b, float* d_clusters,
                      void* workspace, size_t workspace_bytes, stego_stream_t stream);

/* Host only: the dynamic LDS bytes one workgroup of the main kernel uses for `desc` (0 for an invalid descriptor) and the number of
 * workgroups it launches.  Touches no device. */
size_t stego_probe_train_plan(const StegoProbeTrainDesc* desc, int32_t* workgroups);

#ifdef __cplusplus
}
#endif

#endif
