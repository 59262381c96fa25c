/*
 * stego_kmeans.h - C ABI of the cluster refit: spherical (cosine) k-means over a resident tensor of segmentation codes, exported by the
 * same libstego_corr.so.
 *
 * The cluster probe (ClusterLookup) is trained by minibatch gradient steps for a count fixed at training time.  These entry points refit
 * it for any count n <= STEGO_PROBE_MAX_N from the codes of a whole dataset, with ClusterLookup's own definitions, so a refitted probe
 * means what a trained one means:
 *     x^ = x / max(|x|, 1e-12),  c^ = c / max(|c|, 1e-12),  a(p) = the FIRST maximum over n of x^_p . c^_n  (torch.argmax)
 *
 * The codes are one float32 map [B, K, h, w] with arbitrary element strides (the channels-last store of a dataset's low-resolution codes
 * is the fast case); a token is one (b, y, x), token p = (b h + y) w + x, T = B h w tokens.
 *
 * stego_kmeans_step: one Lloyd iteration, two launches, no float atomics anywhere: repeat calls are bitwise equal.
 *   main    persistent workgroups, each a contiguous slab of 128-token tiles.  c^ is staged in LDS once per workgroup (its norm in
 *           fp64).  Per tile the tokens are staged, normalised in LDS (the squared norm in fp64, the division in fp32), scored against
 *           the centroids on the exact fp32 matrix instruction (32x32x2: a k-ordered fmaf chain over the channels), and the first
 *           maximum is taken (ties to the lowest index).  The per-cluster sums of x^ are a second product on the same instruction,
 *           one-hot x x^, whose products are exact; an fp32 accumulator takes at most STEGO_KMEANS_FOLD tokens before it is added to
 *           an fp64 one.  Each workgroup writes one partial: [n, K] fp64 sums, n int64 counts, the fp64 sum of the winning
 *           similarities - and, when `labels` is given, the uint8 label of every token.
 *   finish  one workgroup per cluster adds the partials in workgroup order; centroids_out[n] = sums_n / |sums_n|, a cluster with count
 *           0 or a zero sum keeps its old row, normalised.  The workgroup that finishes last (an integer ticket) writes
 *           stats = {objective = sum_p max_n x^_p . c^_n, clusters that kept their row, shift = 1 - min_n c^old_n . c^new_n, T}.
 *   centroids_out == NULL is assignment only: labels, counts, stats = {objective, 0, 0, T}; the sums are not formed.
 *   centroids_in and centroids_out may be the same pointer.  A zero-norm token has x^ = 0: it goes to cluster 0, counts there and
 *   adds nothing, as in ClusterLookup.  NaNs in the codes are not supported (no fault; the label is unspecified).
 *
 * stego_kmeans_seed: k-means++ on the device, two small launches per round.  The n uniform numbers u are the caller's (its draw
 * stream stays its own) and are read on the HOST, when the call is made: `u` is a host pointer.
 *   round 0      the weight of a token is 1 if its norm is > 0, else 0
 *   round r >= 1 best_p = max(best_p, x^_p . c^_{r-1}) is kept as float32 [T] in the workspace; the weight is max(0, 1 - best_p), and
 *                0 for zero-norm tokens.  If the round's total weight is 0, round 0's weights are used.
 *   the pick     the first token whose inclusive cumulative weight exceeds u_r * total; totals and the cumulative sum are fp64 in token
 *                order: per-workgroup partials first, then a scan inside the one slab that holds the target.
 *   centroids[r] = x^ of the picked token, picks[r] = its index.  With no token of positive norm at all, token 0 is picked.
 *
 * Workspace.  The step keeps one partial per workgroup of the main launch - at most STEGO_KMEANS_MAX_WORKGROUPS = 512 of them, each a
 * contiguous slab of tiles: 512 * (n K + n + 1) * 8 bytes at the most, 33.8 MB at n = 64, K = 128.  The seeding keeps best_p, 4 T
 * bytes, and two fp64 totals per slab (at most 1024 slabs).  stego_kmeans_workspace_bytes is the larger of the two.
 *
 * Conventions as in stego_corr.h: device pointers (but `u`), nothing allocated / freed / synchronised, work enqueued on `stream`,
 * capturable into a HIP graph, STEGO_OK or an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_KMEANS_H
#define STEGO_KMEANS_H

#include "stego_probe.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_KMEANS_DIM = 180,     /* K outside [1, STEGO_KMEANS_MAX_K] or n outside [1, STEGO_KMEANS_MAX_N]                        */
    STEGO_ERR_KMEANS_SIZE = 181,    /* B outside [1, 65535], h or w < 1, or B * h * w > 2^31 - 1                                     */
    STEGO_ERR_KMEANS_DRAW = 182     /* a u outside [0, 1)                                                                            */
};

#define STEGO_KMEANS_MAX_K 128
#define STEGO_KMEANS_MAX_N 64
#define STEGO_KMEANS_FOLD 1024
#define STEGO_KMEANS_TILE 128
#define STEGO_KMEANS_MAX_WORKGROUPS 512

typedef struct StegoKmeansDesc {
    int32_t B, K, h, w;             /* the codes: images (1 .. 65535), channels (1 .. 128), rows, columns; B h w <= 2^31 - 1 */
    int32_t n;                      /* clusters (1 .. 64 = STEGO_PROBE_MAX_N)                                                 */
} StegoKmeansDesc;

/* Bytes of workspace stego_kmeans_step and stego_kmeans_seed need for `desc` (the larger of the two); 0 for an invalid descriptor.
 * Host only. */
size_t stego_kmeans_workspace_bytes(const StegoKmeansDesc* desc);

/* The LDS bytes of the main launch of stego_kmeans_step and, in *workgroups (may be NULL), its grid; 0 (and 0 workgroups) for an
 * invalid descriptor.  Host only: no device is touched. */
size_t stego_kmeans_plan(const StegoKmeansDesc* desc, int32_t* workgroups);

/* One Lloyd iteration: two launches.
 *   codes         : float32 [B, K, h, w] with arbitrary strides
 *   centroids_in  : float32 [n, K], dense (any scale: rows are normalised)
 *   centroids_out : float32 [n, K], dense, unit rows; NULL: assignment only; may equal centroids_in
 *   labels        : uint8 [B, h, w], dense; NULL: not written
 *   counts        : int64 [n]
 *   stats         : float64 [4] = {objective, clusters that kept their row, shift, T}
 *   workspace     : at least stego_kmeans_workspace_bytes(desc) bytes, 16-byte aligned, needs no initialisation
 * Returns STEGO_ERR_KMEANS_DIM / _SIZE, STEGO_ERR_NULL, STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN (codes or centroids not 4-byte aligned,
 * counts or stats not 8-byte, the workspace not 16-byte aligned). */
int stego_kmeans_step(const StegoKmeansDesc* desc, const StegoMap* codes, const float* centroids_in, float* centroids_out, uint8_t* labels,
                      int64_t* counts, double* stats, void* workspace, size_t workspace_bytes, stego_stream_t stream);

/* k-means++ seeding: 2 n launches.
 *   u         : float64 [n] in [0, 1), HOST memory, read before the call returns
 *   centroids : float32 [n, K], dense: x^ of the picked tokens
 *   picks     : int64 [n]: their token indices
 * Returns as stego_kmeans_step, and STEGO_ERR_KMEANS_DRAW (checked last). */
int stego_kmeans_seed(const StegoKmeansDesc* desc, const StegoMap* codes, const double* u, float* centroids, int64_t* picks, void* workspace,
                      size_t workspace_bytes, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
