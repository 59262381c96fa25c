/*
 * stego_pr.h - C ABI of the label co-occurrence precision / recall histogram of feature correspondences, exported by the same
 * libstego_corr.so.
 *
 * Replaces the per-batch chain of the reference's src/plot_pr_curves.py:108-121 (get_net_fd) and :160-166 (plot_pr):
 *     fd = tensor_correlation(norm(sample(feats1, coords1)), norm(sample(feats2, coords2)))          [B, S, S, S, S]
 *     ld = tensor_correlation(sample(one_hot(label1 + 1), coords1), sample(one_hot(label2 + 1), coords2))
 *     precision_recall_curve(ld.to(int64), rescaled fd)
 * by one launch that samples, normalises, contracts, tests the labels and counts: the result is a histogram of the scores over
 * fixed bins of [-1, 1], one column for the negative and one for the positive pairs.  No correlation tensor is written.  The
 * reference rescales the scores by their global minimum and maximum before scikit-learn sees them; that map is increasing and
 * affine, so precision, recall and average precision do not depend on it and one pass over the data suffices.
 *
 * Per image i, point p of coords1 and point q of coords2 (j = index_b ? index_b[i] : i):
 *   score   fd = <norm(sample(a_i, p)), norm(sample(b_j, q))>, sample / norm as in the loss kernels (bilinear, border padding,
 *           align_corners=True, F.normalize with eps = 1e-10).  The order of the points does not matter to a histogram, so the
 *           reference's coords.permute(0, 2, 1, 3) needs no counterpart: pass coords.reshape(B, S * S, 2).
 *           With STEGO_PR_RAW the normalisation is skipped and the raw dot product is clamped to [-1, 1] before it is binned.
 *   bin     min(n_bins - 1, max(0, floor((fd + 1) / 2 * n_bins)))
 *   target  positive iff every bilinear tap with a non-zero weight at p and at q carries one and the same class, where the class of a
 *           label l is l + 1 for 0 <= l < n_classes and 0 ("unlabeled") otherwise, as in one_hot(label + 1, n_classes + 1).  That is
 *           the reference's `ld == 1` in exact arithmetic.  It is computed from the integer labels.  The reference truncates an fp32
 *           sum (ld.to(int64)), so there a pure pair whose four fp32 weights sum to 0.99999994 becomes a negative; here it stays
 *           a positive.
 *           With STEGO_PR_SKIP_UNLABELED every pair in which a non-zero tap of p or q is unlabeled is left out of both columns.
 *   count   hist[bin][target] += 1 on top of what hist holds: one histogram collects a whole validation set over many calls.
 *           Counters are integers (per-workgroup counting in LDS, one flush per workgroup with 64-bit vector atomic adds), so the
 *           result does not depend on arrival order and is bitwise repeatable.
 *
 * Conventions as in stego_corr.h / stego_probe.h: device pointers, nothing allocated / freed / synchronised, work enqueued on
 * `stream`, STEGO_OK or an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_PR_H
#define STEGO_PR_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_PR_DIM = 50,       /* C outside [1, STEGO_PR_MAX_C]                                                            */
    STEGO_ERR_PR_POINTS = 51,    /* N1 or N2 outside [1, STEGO_PR_MAX_POINTS]                                                */
    STEGO_ERR_PR_BINS = 52,      /* n_bins outside [STEGO_PR_MIN_BINS, STEGO_PR_MAX_BINS]                                    */
    STEGO_ERR_PR_CLASSES = 53,   /* n_classes outside [1, STEGO_PR_MAX_CLASSES]                                              */
    STEGO_ERR_PR_SIZE = 54,      /* B outside [1, 65535], or h, w, HL, WL outside [1, STEGO_PR_MAX_SIDE]                     */
    STEGO_ERR_PR_FLAGS = 55      /* a flag bit outside STEGO_PR_RAW | STEGO_PR_SKIP_UNLABELED                                */
};

/* StegoPrDesc.flags */
enum {
    STEGO_PR_RAW = 1,            /* no normalisation: raw dot products, clamped to [-1, 1] for binning                       */
    STEGO_PR_SKIP_UNLABELED = 2  /* leave pairs with an unlabeled tap out of both columns                                    */
};

#define STEGO_PR_MAX_C 768
#define STEGO_PR_MAX_POINTS 4096
#define STEGO_PR_MIN_BINS 64
#define STEGO_PR_MAX_BINS 8192
#define STEGO_PR_MAX_CLASSES 255
#define STEGO_PR_MAX_SIDE 16384

typedef struct StegoPrDesc {
    int32_t B;                   /* images (1 .. 65535)                                                   */
    int32_t C;                   /* channels of both maps (1 .. STEGO_PR_MAX_C, any value)                */
    int32_t h, w;                /* rows, columns of both maps                                            */
    int32_t HL, WL;              /* rows, columns of both label maps (independent of h, w)                */
    int32_t N1, N2;              /* points per image of coords1 / coords2 (1 .. STEGO_PR_MAX_POINTS)      */
    int32_t n_bins;              /* score bins over [-1, 1]                                               */
    int32_t n_classes;           /* labels in [0, n_classes) are classes, everything else is "unlabeled"  */
    int32_t flags;               /* STEGO_PR_*                                                            */
} StegoPrDesc;

/* Adds the pairs of B images to `hist`.
 *   a, b       : float32 [B, C, h, w] with arbitrary strides (64-bit offsets)
 *   labels_a/b : int64 [B, HL, WL] contiguous
 *   index_b    : int64 [B] or NULL: the image of b / labels_b paired with image i of a (values are clamped to [0, B))
 *   coords1/2  : float32 [B, N1, 2] / [B, N2, 2] contiguous, (x, y) in [-1, 1] (anything outside is border-clamped)
 *   hist       : uint64 [n_bins, 2] contiguous, 8-byte aligned: (negatives, positives) per bin; only ever added to
 * Returns STEGO_ERR_NULL (desc, a map or its data, labels, coordinates, hist), STEGO_ERR_PR_*, STEGO_ERR_ALIGN (a float pointer
 * not 4-byte aligned; labels, index_b or hist not 8-byte aligned). */
int stego_pr_accumulate(const StegoPrDesc* desc, const StegoMap* a, const StegoMap* b, const int64_t* labels_a, const int64_t* labels_b,
                        const int64_t* index_b, const float* coords1, const float* coords2, uint64_t* hist, stego_stream_t stream);

/* Host only: the dynamic LDS bytes one workgroup of stego_pr_accumulate uses for `desc` (0 for an invalid descriptor) and the grid
 * of 128 x 128 point tiles per image it launches.  Touches no device. */
size_t stego_pr_plan(const StegoPrDesc* desc, int32_t* tiles1, int32_t* tiles2);

#ifdef __cplusplus
}
#endif

#endif
