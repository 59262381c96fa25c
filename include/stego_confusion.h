/*
 * stego_confusion.h - C ABI of the device-side confusion matrices behind mIoU and accuracy, exported by the same libstego_corr.so.
 *
 * Replaces the scoring chain of validation and evaluation (train_segmentation.py:247-262, eval_segmentation.py:124-144 and
 * UnsupervisedMetrics.update, utils.py:215-228 of the reference): resize the code to the label's resolution, run both probes, take the
 * argmax, mask the ignored labels, bincount and copy the histogram to the host, per probe and per batch.  Here one launch goes from the
 * low-resolution code to both confusion matrices: no per-pixel tensor is written and nothing is copied to the host.
 *
 * A confusion matrix is int64 [n, n_classes]: rows are predictions, columns are actual labels (the layout of UnsupervisedMetrics.stats).
 * Every entry point ADDS onto the matrices it is given; the caller zeroes them once per epoch.  A pixel whose label lies outside
 * [0, n_classes) counts nothing.  The counts are integers summed with integer atomics (32-bit in LDS per workgroup, 64-bit in global
 * memory), so they are exact and the same from run to run.
 *
 * Conventions as in stego_probe.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_CONFUSION_H
#define STEGO_CONFUSION_H

#include "stego_probe.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_CONF_DIM = 100,     /* K outside [1, STEGO_PROBE_MAX_K], an active probe's n or n_classes outside [1, STEGO_CONF_MAX_N]        */
    STEGO_ERR_CONF_SIZE = 101,    /* B, h, w, H or W out of range (stego_probe_confusion: the probe head's limits; stego_confusion: B, H, W
                                     < 1 or B * H * W >= 2^40)                                                                             */
    STEGO_ERR_CONF_PROBES = 102,  /* lin_on or clu_on neither 0 nor 1, or both probes skipped                                              */
    STEGO_ERR_CONF_KIND = 103     /* stego_confusion: pred_kind outside the enum below                                                     */
};

/* What stego_confusion's `pred` holds. */
enum {
    STEGO_CONF_LABELS = 0,        /* int64 [B, H, W] contiguous: label maps                                                               */
    STEGO_CONF_SCORES = 1         /* float32 [B, n, H, W] contiguous: scores; the prediction is the index of the first maximum over n     */
};

#define STEGO_CONF_MAX_N 64                    /* rows and columns of a confusion matrix (STEGO_PROBE_MAX_N) */
#define STEGO_CONF_MAX_PIXELS (1ll << 40)      /* B * H * W of stego_confusion stays below this              */

typedef struct StegoProbeConfusionDesc {
    int32_t B;                   /* images (1 .. 65535)                                                               */
    int32_t K;                   /* code channels (1 .. STEGO_PROBE_MAX_K)                                            */
    int32_t h, w;                /* code rows, columns (1 .. STEGO_PROBE_MAX_CODE)                                    */
    int32_t H, W;                /* label rows, columns (1 .. STEGO_PROBE_MAX_OUT; up- or downsampling)               */
    int32_t n_lin, n_clu;        /* labels of the linear and the cluster probe (1 .. STEGO_CONF_MAX_N)                */
    int32_t lin_on, clu_on;      /* 1: count this probe; 0: skip it (its n, weights and counts are never read)        */
    float alpha;                 /* cluster logits = alpha * cosine                                                   */
    int32_t n_classes;           /* columns of both matrices (1 .. STEGO_CONF_MAX_N)                                  */
} StegoProbeConfusionDesc;

/* The fused probe head with the confusion matrices as its only output.  Per label pixel the arithmetic is that of stego_probe_head
 * with STEGO_PROBE_ARGMAX (flip average, align_corners=False footprint, projections of the footprint pixels, four-tap interpolation,
 * the norm of the interpolated code for the cluster probe, first maximum of the log-softmax values), so the prediction equals that
 * kind's output bit for bit; then bin [prediction, labels[b, Y, X]] of the probe's matrix counts one when the label is in
 * [0, n_classes).
 *   code, code_flip, lin_w, lin_b, centroids : as stego_probe_head
 *   labels     : int64 [B, H, W] contiguous (required)
 *   lin_counts : int64 [n_lin, n_classes] contiguous, clu_counts : int64 [n_clu, n_classes] contiguous; added onto
 * Returns STEGO_ERR_NULL (desc, code, labels, an active probe's weights or counts), STEGO_ERR_CONF_PROBES, STEGO_ERR_CONF_DIM,
 * STEGO_ERR_CONF_SIZE, STEGO_ERR_ALIGN (a float pointer not 4-byte aligned; labels or counts not 8-byte aligned). */
int stego_probe_confusion(const StegoProbeConfusionDesc* desc, const StegoMap* code, const StegoMap* code_flip, const float* lin_w,
                          const float* lin_b, const float* centroids, const int64_t* labels, int64_t* lin_counts, int64_t* clu_counts,
                          stego_stream_t stream);

/* Host only: the dynamic LDS bytes one workgroup of stego_probe_confusion uses for `desc`, the per-workgroup histograms included
 * (0 for an invalid descriptor), and the label tile (rows, columns) it was planned for.  Touches no device. */
size_t stego_probe_confusion_plan(const StegoProbeConfusionDesc* desc, int32_t* tile_rows, int32_t* tile_cols);

typedef struct StegoConfusionDesc {
    int32_t B;                   /* images (>= 1)                                                                     */
    int32_t n;                   /* rows of the matrix: predictions (1 .. STEGO_CONF_MAX_N); the planes of SCORES     */
    int32_t H, W;                /* rows, columns (>= 1); B * H * W < STEGO_CONF_MAX_PIXELS, offsets are 64-bit       */
    int32_t n_classes;           /* columns of the matrix (1 .. STEGO_CONF_MAX_N)                                     */
    int32_t pred_kind;           /* STEGO_CONF_LABELS or STEGO_CONF_SCORES                                            */
} StegoConfusionDesc;

/* The same counting for predictions made elsewhere (the dense CRF's output, label maps).
 *   pred   : what desc->pred_kind names.  For SCORES the prediction is the index of the first maximum over n, which is torch.argmax
 *            for finite inputs; non-finite scores (NaN, +-inf) are unsupported: what they count is unspecified.
 *   labels : int64 [B, H, W] contiguous
 *   counts : int64 [n, n_classes] contiguous; added onto
 * A prediction outside [0, n) or a label outside [0, n_classes) counts nothing.
 * Returns STEGO_ERR_NULL, STEGO_ERR_CONF_KIND, STEGO_ERR_CONF_DIM, STEGO_ERR_CONF_SIZE, STEGO_ERR_ALIGN (SCORES not 4-byte aligned;
 * LABELS, labels or counts not 8-byte aligned). */
int stego_confusion(const StegoConfusionDesc* desc, const void* pred, const int64_t* labels, int64_t* counts, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
