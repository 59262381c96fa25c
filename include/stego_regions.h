/*
 * stego_regions.h - C ABI of the segments as objects: connected regions of a label map, their table, and the cleanup of small regions,
 * exported by the same libstego_corr.so.
 *
 * Definitions (INTEGRATION.md "Regions" has them in full; the kernels, the CPU chain of stego_amd/regions.py and the oracle of
 * tests/regions_oracle.py implement exactly these):
 *   input       labels [B, H, W], int64, int32 or uint8, dense.  Every image is on its own.
 *   region      a maximal set of pixels with the same label >= 0, connected under `connectivity` 4 or 8.  A pixel with a negative label
 *               belongs to no region: its id and its root are -1.
 *   first pixel the pixel of a region with the smallest raster index y W + x.
 *   region id   the regions of an image are numbered 0 .. n - 1 in increasing order of their first pixel.
 *   table       integer columns, a row per region: label, area, y0, x0, y1, x1 (an inclusive box), first, sum_y, sum_x.  No float sums:
 *               every output is independent of the order of the adds, two calls are bitwise equal.
 *   cleanup     one round, min_area >= 1, n_labels <= 256: a region is small when area < min_area.  votes[r][c] of a small region r counts
 *               the ordered pairs of 4-neighbours (p, q) with p in r, q in a region that is not small, label(q) = c (always 4-neighbours,
 *               whatever the connectivity of the regions is; a label >= n_labels casts no vote).  r takes the class with the most votes, the
 *               smallest class on a tie; with no votes it keeps its label.  Every small region is relabelled from the round's input state.
 *
 * stego_regions_label: six launches, no workgroup ever waits for another (the phases are launches):
 *   tile     a workgroup per STEGO_REGIONS_TILE^2 tile: union-find over the tile in LDS, the larger root is hung below the smaller, so a
 *            root is the first pixel of its piece; the piece's root goes to `root` as a raster index of the image.
 *   seam     a thread per pixel pair across a tile border: the same union on `root`, with atomicMin.
 *   flatten  root[p] = the root of p, and the number of roots of every STEGO_REGIONS_CHUNK pixels.
 *   scan     a workgroup per image: the exclusive sums of the chunks' counts in raster order, n_regions.
 *   number   ids of the roots: the chunk's offset + the rank inside the chunk.   spread   ids[p] = ids[root[p]].
 *   Every find loop walks strictly decreasing indices (root[p] <= p always holds, atomicMin only lowers a word); a union loop goes round
 *   again only after atomicMin answered with a parent smaller than the one it hung: both end on any input.
 * stego_regions_table: three launches (reset, add, finish).  Integer atomics only: add, min, max, a 64-bit add for the coordinate sums.
 *   The lanes of a wave that hold a run of one id along a row are combined first: one lane adds the run in closed form.
 * stego_regions_votes: two launches (reset, count).  stego_regions_relabel: one launch.
 *
 * Limits, all checked on the host before anything is enqueued: B in [1, 65535]; H, W >= 1 and H * W < 2^31 (raster indices are int32;
 * every byte offset into a [B, H, W] array is 64-bit); connectivity 4 or 8; label_dtype one of STEGO_REGIONS_*; n_labels in [1, 256] and
 * min_area >= 1 where they are used.  Pointers are aligned to their element (labels: 8 / 4 / 1 bytes; int32 arrays 4; int64 arrays 8;
 * the workspace 16).
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, capturable into a
 * HIP graph, STEGO_OK or an error code.
 */
#ifndef STEGO_REGIONS_H
#define STEGO_REGIONS_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_REGIONS_SIZE = 190,   /* B outside [1, 65535], H or W < 1, or H * W >= 2^31                                            */
    STEGO_ERR_REGIONS_CONN = 191,   /* connectivity neither 4 nor 8                                                                  */
    STEGO_ERR_REGIONS_DTYPE = 192,  /* label_dtype none of STEGO_REGIONS_I64, _I32, _U8                                              */
    STEGO_ERR_REGIONS_LABELS = 193, /* n_labels outside [1, STEGO_REGIONS_MAX_LABELS]                                                */
    STEGO_ERR_REGIONS_RANGE = 194   /* capacity < 0, lo < 0, hi < lo, or hi - lo rows of votes beyond 2^31 - 1 words                 */
};

enum { STEGO_REGIONS_I64 = 0, STEGO_REGIONS_I32 = 1, STEGO_REGIONS_U8 = 2 };

#define STEGO_REGIONS_TILE 32
#define STEGO_REGIONS_CHUNK 2048
#define STEGO_REGIONS_MAX_LABELS 256
#define STEGO_REGIONS_LAUNCHES 6

typedef struct StegoRegionsDesc {
    int32_t B, H, W;                /* images (1 .. 65535), rows, columns; H * W < 2^31   */
    int32_t connectivity;           /* 4 or 8                                             */
    int32_t label_dtype;            /* STEGO_REGIONS_I64 / _I32 / _U8                     */
} StegoRegionsDesc;

/* The columns of the table: `cols32` is int32 [STEGO_REGIONS_COLS32, capacity], `cols64` int64 [STEGO_REGIONS_COLS64, capacity]. */
enum { STEGO_REGIONS_AREA = 0, STEGO_REGIONS_Y0, STEGO_REGIONS_X0, STEGO_REGIONS_Y1, STEGO_REGIONS_X1, STEGO_REGIONS_FIRST,
       STEGO_REGIONS_COLS32 };
enum { STEGO_REGIONS_LABEL = 0, STEGO_REGIONS_SUM_Y, STEGO_REGIONS_SUM_X, STEGO_REGIONS_COLS64 };

/* Bytes of workspace stego_regions_label needs; 0 for an invalid descriptor.  Host only. */
size_t stego_regions_workspace_bytes(const StegoRegionsDesc* desc);

/* The launches of stego_regions_label in order (tile, seam, flatten, scan, number, spread): their static + dynamic LDS bytes and their
 * workgroups, STEGO_REGIONS_LAUNCHES of each (either may be NULL), and the tile edge in *tile (may be NULL).  Returns the descriptor's
 * code; zeros for an invalid one.  Host only: no device is touched. */
int stego_regions_plan(const StegoRegionsDesc* desc, int32_t* tile, size_t* lds_bytes, int64_t* workgroups);

/* labels -> ids, n_regions, root.
 *   labels    : [B, H, W] of desc->label_dtype, dense
 *   ids       : int32 [B, H, W]: the region id, -1 where the label is negative
 *   n_regions : int32 [B]
 *   root      : int32 [B, H, W]: the raster index y W + x of the first pixel of the pixel's region, -1 where the label is negative
 *   workspace : at least stego_regions_workspace_bytes(desc) bytes, 16-byte aligned, needs no initialisation
 * Returns STEGO_ERR_REGIONS_SIZE / _CONN / _DTYPE, STEGO_ERR_NULL, STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN. */
int stego_regions_label(const StegoRegionsDesc* desc, const void* labels, int32_t* ids, int32_t* n_regions, int32_t* root, void* workspace,
                        size_t workspace_bytes, stego_stream_t stream);

/* ids + labels -> the table.  The row of region `id` of image b is row_offset[b] + id; rows at or beyond `capacity` are left out.
 *   row_offset : int64 [B]: the first row of every image (the exclusive sums of n_regions)
 *   cols32     : int32 [STEGO_REGIONS_COLS32, capacity]: area, y0, x0, y1, x1, first
 *   cols64     : int64 [STEGO_REGIONS_COLS64, capacity]: label, sum_y, sum_x
 * capacity 0 is legal and does nothing.  Returns as above, and STEGO_ERR_REGIONS_RANGE. */
int stego_regions_table(const StegoRegionsDesc* desc, const void* labels, const int32_t* ids, const int64_t* row_offset, int64_t capacity,
                        int32_t* cols32, int64_t* cols64, stego_stream_t stream);

/* The votes of the small regions whose rank among the small ones lies in [lo, hi).
 *   small_rank : int32 [capacity]: per table row, the rank of the region among the small ones, or -1 for a region that is not small
 *   votes      : int32 [hi - lo, n_labels], reset here
 * Returns as above, and STEGO_ERR_REGIONS_LABELS / _RANGE. */
int stego_regions_votes(const StegoRegionsDesc* desc, const void* labels, const int32_t* ids, const int64_t* row_offset, int64_t capacity,
                        const int32_t* small_rank, int64_t lo, int64_t hi, int32_t n_labels, int32_t* votes, stego_stream_t stream);

/* Rewrites the pixels of the small regions of ranks [lo, hi): the first maximum of the region's vote row, nothing without a vote.
 *   labels_in  : the round's input state;  labels_out : the same dtype, another array that starts as a copy of labels_in
 *   first      : int32 [capacity]: the table's column (a region is counted by its first pixel)
 *   changed    : int32 [1]: += the regions whose label changed (the caller resets it once per round)
 * Returns as stego_regions_votes. */
int stego_regions_relabel(const StegoRegionsDesc* desc, const void* labels_in, void* labels_out, const int32_t* ids, const int64_t* row_offset,
                          int64_t capacity, const int32_t* small_rank, const int32_t* first, int64_t lo, int64_t hi, int32_t n_labels,
                          const int32_t* votes, int32_t* changed, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
