/*
 * stego_region_pool.h - C ABI of the region descriptors: the mean of a low-resolution map over every full-resolution region of an id map,
 * exported by the same libstego_corr.so.
 *
 * Definitions (INTEGRATION.md "Region descriptors" has them in full; the kernels, the CPU chain of stego_amd/region_descriptors.py and
 * the oracle of tests/region_pool_oracle.py implement exactly these):
 *   inputs      map [B, C, h, w] float32, any element strides (StegoMap), finite values; ids int32 [B, H, W] dense, as
 *               stego_regions_label writes it: -1 or a region id of its image; row_offset int64 [B], the first row of every image;
 *               area int32 [capacity], the table's column; a row range [lo, hi).
 *   pixel value v(b, Y, X, c) = F.interpolate(map, (H, W), mode="bilinear", align_corners=False), evaluated in float32: the taps
 *               (i0, i1, l1) of src_index (csrc/probe_common.h) for the scales h / H and w / W, every operation of the source index
 *               rounded on its own (no fused multiply-add: what numpy and torch's CPU path compute), l0 = 1 - l1, and the value as
 *               probe_phases.h's tap4 writes it, h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d), as
 *               fma(h0, fma(w0, a, w1 * b), h1 * fma(w0, c, w1 * d)).  With h == H and w == W the taps are the pixel itself
 *               (l1 = 0): the mean colours of an image, C = 3.
 *   scale       M = max |map| over the whole map of the call, found on the device (no host read).  M == 0: every descriptor is 0.
 *               Otherwise e with 2^(e-1) <= M < 2^e (e = -126 for a subnormal M) and s = 30 - e.
 *   quantised   q = (int64) rint(v * 2^s), round to nearest even; the scaling is exact.  The interpolation is convex, so |q| <= 2^30.
 *   sum         S[r][c] = the sum of q over the pixels with row_offset[b] + ids[b, Y, X] == r, in int64.  H * W < 2^31, so
 *               |S| < 2^61: no overflow.  Every add is an integer add.
 *   descriptor  out[r - lo][c] = float32((double) S[r][c] * 2^(-s) / area[r]) for r in [lo, hi); 0 where area[r] <= 0.  Pixels with
 *               id -1 and pixels of rows outside the range add nothing.
 * Consequence: the result is independent of the order of the adds, of the launch geometry and of how the rows are cut into ranges.
 * Two calls are bitwise equal, and so are two partitions of the rows.
 *
 * stego_region_pool: three launches, no workgroup waits for another.
 *   range    resets the sums and leaves the largest |map| of every workgroup in the workspace (at most STEGO_REGION_POOL_PARTIALS).
 *   pool     a wave owns one segment of one row of one image and one block of STEGO_REGION_POOL_CB channels; its lanes are channels
 *            (lane and lane + 64 of the block).  For C <= 32 the wave is cut into 64 / G groups of G = 2^ceil(log2 C) lanes, group g
 *            takes every (64 / G)-th pixel of the segment, and the segment is longer.  A group walks its pixels in order with the
 *            quantised values summed in int64 registers, and flushes them with one 64-bit integer atomic add per lane when the id
 *            changes or the segment ends.  The low-resolution cells stay in registers while the taps do not move.
 *   finish   converts, divides by the area and writes `out`.
 *
 * Limits, all checked on the host before anything is enqueued: B in [1, 65535]; H, W >= 1 and H * W < 2^31; h, w >= 1 and h * w < 2^31; C in
 * [1, STEGO_REGION_POOL_MAX_C]; 0 <= lo <= hi <= capacity; (hi - lo) * C < 2^31.  Pointers are aligned to their element (float32 and
 * int32 arrays 4, row_offset 8), the workspace to 16.  Every byte offset is 64-bit.  hi == lo is legal and does nothing.
 *
 * Conventions as in stego_regions.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, capturable
 * into a HIP graph, STEGO_OK or an error code.
 */
#ifndef STEGO_REGION_POOL_H
#define STEGO_REGION_POOL_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_REGION_POOL_SIZE = 200,   /* B outside [1, 65535], H, W, h or w < 1, or H * W or h * w >= 2^31                          */
    STEGO_ERR_REGION_POOL_DIM = 201,    /* C outside [1, STEGO_REGION_POOL_MAX_C]                                                    */
    STEGO_ERR_REGION_POOL_RANGE = 202   /* rows < 0; lo < 0, hi < lo or hi > capacity; (hi - lo) * C >= 2^31                         */
};

#define STEGO_REGION_POOL_MAX_C 2048
#define STEGO_REGION_POOL_CB 128
#define STEGO_REGION_POOL_PARTIALS 1024
#define STEGO_REGION_POOL_LAUNCHES 3

typedef struct StegoRegionPoolDesc {
    int32_t B, C, h, w;             /* the map: images (1 .. 65535), channels (1 .. 2048), rows, columns                 */
    int32_t H, W;                   /* the id map; H * W < 2^31                                                           */
    int64_t rows;                   /* the most rows (hi - lo) of one call: sizes the workspace; rows * C < 2^31          */
} StegoRegionPoolDesc;

/* Bytes of workspace a call of up to desc->rows rows needs: STEGO_REGION_POOL_PARTIALS floats and the int64 sums [rows, C].  0 for an
 * invalid descriptor.  Host only. */
size_t stego_region_pool_workspace_bytes(const StegoRegionPoolDesc* desc);

/* The launches in order (range, pool, finish; the finish for desc->rows rows): their LDS bytes and workgroups,
 * STEGO_REGION_POOL_LAUNCHES of each (either may be NULL); *segment: the pixels of the row segment one wave walks; *channel_block: the
 * channels of one wave (both may be NULL).  Returns the descriptor's code; zeros for an invalid one.  Host only: no device is touched. */
int stego_region_pool_plan(const StegoRegionPoolDesc* desc, int32_t* segment, int32_t* channel_block, size_t* lds_bytes,
                           int64_t* workgroups);

/* map, ids -> the descriptors of the rows [lo, hi).
 *   map        : [B, C, h, w] float32, element strides
 *   ids        : int32 [B, H, W] dense
 *   row_offset : int64 [B]
 *   area       : int32 [capacity]
 *   out        : float32 [hi - lo, C]
 *   workspace  : at least STEGO_REGION_POOL_PARTIALS * 4 + (hi - lo) * C * 8 bytes (stego_region_pool_workspace_bytes with
 *                rows >= hi - lo), 16-byte aligned; the call resets it, no memset is expected
 * Returns STEGO_ERR_REGION_POOL_SIZE / _DIM / _RANGE, STEGO_ERR_NULL, STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN. */
int stego_region_pool(const StegoRegionPoolDesc* desc, const StegoMap* map, const int32_t* ids, const int64_t* row_offset,
                      const int32_t* area, int64_t capacity, int64_t lo, int64_t hi, float* out, void* workspace, size_t workspace_bytes,
                      stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
