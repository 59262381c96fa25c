/*
 * stego_heat.h - C ABI of the query-point correspondence heatmaps, exported by the same libstego_corr.so.
 *
 * Replaces the chain of the reference's src/plot_dino_correspondence.py:39-58 (get_heatmaps), per target map:
 *     s    = sample(feats1, q)                                          bilinear, border, align_corners=True; q = (x, y)
 *     attn = einsum("nchw,ncij->nhwij", F.normalize(s, dim=1), F.normalize(feats_t, dim=1))        eps = 1e-12
 *     attn -= attn.mean([3, 4], keepdims=True);  attn = attn.clamp(0)
 *     heat = F.interpolate(attn, (H, W), mode="bilinear", align_corners=True)
 * by one call of two launches.  The only large tensor that is written is the result.
 *
 * Per image i (j = index_t ? index_t[i] : i), query n and cell (y, x) of the target map:
 *   low     r[n, y, x] = <s_n, t_yx> / (max(||s_n||, 1e-12) * max(||t_yx||, 1e-12)), s_n the bilinear sample of src_i at point n
 *           (a point outside [-1, 1] is border-clamped), t_yx the channel vector of tgt_j.  fp32 products and sums.
 *   centre  m[n] = mean of r[n] over the h * w cells, unless STEGO_HEAT_NO_CENTER (then m = 0).  The cells are added per chunk of
 *           128 cells in float64 and the chunks in a fixed order: no atomics, repeat launches are bitwise equal.
 *   clamp   a = max(r - m, 0), unless STEGO_HEAT_NO_CLAMP (then a = r - m).
 *   heat    the bilinear resize of a to H x W with align_corners=True in torch's arithmetic (upsample_bilinear2d): the source
 *           coordinate of output row Y is Y * (h - 1) / (H - 1), 0 for H == 1, so a side of size 1 takes source index 0; an output
 *           of the map's own size is an exact copy of a.  The weights and the three fused multiply-adds of a pixel are rounded in
 *           one fixed sequence, so the 16-byte and the 4-byte store paths (an output that is not 16-byte aligned, a row length that
 *           is no multiple of 4) give the same bits.
 *   peak    max of a[n] over the cells;  best  the (x, y) in [-1, 1] of the first cell in row-major order that holds it
 *           (x = 2 * col / (w - 1) - 1, 0 for w == 1; y likewise).  When the clamp leaves no positive cell that is cell 0.
 *           The maximum is located on r: subtracting m and clamping keep the order, so two cells whose r differ by less than an
 *           fp32 rounding of the subtraction may swap against a search on a.
 *
 * Workspace layout (stego_heat_workspace_bytes; needs no initialisation, fully rewritten by every call), NCH = ceil(h * w / 128):
 *     double  psum[B][N][NCH]      sum of r over the cells of chunk k
 *     float   low [B][N][h * w]    r itself
 *     float   pmax[B][N][NCH]      maximum of r in chunk k
 *     int32   pidx[B][N][NCH]      first cell that holds it
 *
 * Conventions as in stego_pr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_HEAT_H
#define STEGO_HEAT_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_HEAT_DIM = 70,     /* C outside [1, STEGO_HEAT_MAX_C]                                                          */
    STEGO_ERR_HEAT_POINTS = 71,  /* N outside [1, STEGO_HEAT_MAX_POINTS]                                                     */
    STEGO_ERR_HEAT_SIZE = 72,    /* B outside [1, 65535], hs or ws outside [1, STEGO_HEAT_MAX_SIDE], h or w < 1, or
                                    h * w > STEGO_HEAT_MAX_CELLS                                                             */
    STEGO_ERR_HEAT_OUTPUT = 73,  /* H or W outside [1, STEGO_HEAT_MAX_OUT]                                                   */
    STEGO_ERR_HEAT_FLAGS = 74    /* a flag bit outside STEGO_HEAT_NO_CENTER | STEGO_HEAT_NO_CLAMP                            */
};

/* StegoHeatDesc.flags (independent) */
enum {
    STEGO_HEAT_NO_CENTER = 1,    /* keep the mean: with NO_CLAMP the raw cosine map                                          */
    STEGO_HEAT_NO_CLAMP = 2      /* keep the negative part: with centring the signed map plot_heatmap(symmetric=True) shows  */
};

#define STEGO_HEAT_MAX_C 768
#define STEGO_HEAT_MAX_POINTS 4096
#define STEGO_HEAT_MAX_SIDE 16384
#define STEGO_HEAT_MAX_CELLS 16384
#define STEGO_HEAT_MAX_OUT 2048

typedef struct StegoHeatDesc {
    int32_t B;                   /* images (1 .. 65535)                                                   */
    int32_t C;                   /* channels of both maps (1 .. STEGO_HEAT_MAX_C, any value)              */
    int32_t hs, ws;              /* rows, columns of the source map (the one the points sample)           */
    int32_t h, w;                /* rows, columns of the target map (h * w <= STEGO_HEAT_MAX_CELLS)       */
    int32_t N;                   /* query points per image (1 .. STEGO_HEAT_MAX_POINTS)                   */
    int32_t H, W;                /* rows, columns of every heatmap (1 .. STEGO_HEAT_MAX_OUT)              */
    int32_t flags;               /* STEGO_HEAT_*                                                          */
} StegoHeatDesc;

/* Bytes of workspace stego_corr_heatmaps needs for `desc`; 0 for an invalid descriptor.  Host only. */
size_t stego_heat_workspace_bytes(const StegoHeatDesc* desc);

/* Host only: the launch plan for `desc`.  Returns the dynamic LDS bytes of a workgroup of the first launch (0 for an invalid
 * descriptor) and fills, where the pointer is not NULL,
 *   grid1[3]   (chunks of 128 target cells, tiles of 128 queries, B)
 *   grid2[3]   (blocks of out_rows output rows, N, B)
 *   lds2       dynamic LDS bytes of a workgroup of the second launch (the source rows a block of output rows reads)
 *   out_rows   output rows per workgroup of the second launch
 * Touches no device. */
size_t stego_heat_plan(const StegoHeatDesc* desc, int32_t* grid1, int32_t* grid2, size_t* lds2, int32_t* out_rows);

/* The heatmaps of N query points per image.
 *   src       : float32 [B, C, hs, ws], tgt: float32 [B, C, h, w]; arbitrary strides (64-bit offsets)
 *   index_t   : int64 [B] or NULL: the image of tgt paired with image i of src (values are clamped to [0, B))
 *   points    : float32 [B, N, 2] contiguous, (x, y) in [-1, 1] (anything outside is border-clamped)
 *   heat      : float32 [B, N, H, W] contiguous (may exceed 2^32 bytes)
 *   peak      : float32 [B, N] or NULL;  best: float32 [B, N, 2] or NULL
 *   workspace : at least stego_heat_workspace_bytes(desc) bytes, 8-byte aligned
 * Returns STEGO_ERR_NULL (desc, a map or its data, points, heat, workspace), STEGO_ERR_HEAT_*, STEGO_ERR_WORKSPACE,
 * STEGO_ERR_ALIGN (a float pointer not 4-byte aligned; index_t or workspace not 8-byte aligned). */
int stego_corr_heatmaps(const StegoHeatDesc* desc, const StegoMap* src, const StegoMap* tgt, const int64_t* index_t, const float* points,
                        float* heat, float* peak, float* best, void* workspace, size_t workspace_bytes, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
