/*
 * stego_stitch.h - C ABI of sliding-window segmentation of images of any size, exported by the same libstego_corr.so.
 *
 * The reference segments a large scene window by window (plot_potsdam.py: 15 x 15 windows of 320 of a 4800 x 4800 scene, each run
 * through the model and tiled back in Python, its full-resolution log-probabilities written, copied and re-read).  Here the windows
 * may overlap, and one launch reads every window's low-resolution code, blends the overlapping windows per canvas pixel and writes
 * only the canvas.
 *
 * Window layout, the same closed form on the host and on the device.  Along an axis of length L, with window side `win` and stride
 * s, L >= win and win <= 2 s <= 2 win:
 *     n   = 1 + ceil((L - win) / s)            windows
 *     o_i = min(i s, L - win)                  their origins: the last window is shifted back so that it ends at the image's edge
 * Nothing is padded and nothing dropped.  A pixel is covered by at most 3 windows per axis (two regular ones and the shifted last
 * one), 9 in all.  Windows are numbered t = iy * nx + ix.
 *
 * Blend.  Window t weighs a pixel at its window-local offset (y, x) with a = tent(y) * tent(x), tent(u) = min(u + 1, win - u): an
 * integer, exact in fp32.  The normalised weight is a^ = a / sum of a over the covering windows; one covering window gets exactly 1.
 * Per canvas pixel and probe:
 *     1. logits_t = what stego_probe_head computes for window t at size (win, win) before its softmax (W c + b of the resized code;
 *        alpha * cosine with the norm of that window's interpolated code);
 *     2. L = sum_t a^_t logits_t over the covering windows in ascending t, accumulated as acc = fmaf(a^, l, acc) from 0;
 *     3. the label mask is added (after the blend: no 0 * inf), then softmax, log_softmax or the first-maximum argmax, once.
 * For the linear probe this is the probe of the blended code; for the cluster probe the renormalised geometric mean of the windows'
 * distributions.  With one covering window the result is stego_probe_head's, bit for bit.  No atomics: repeat launches are
 * bitwise equal.
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_STITCH_H
#define STEGO_STITCH_H

#include "stego_probe.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_STITCH_DIM = 120,     /* K outside [1, STEGO_PROBE_MAX_K], or an active probe's n outside [1, STEGO_PROBE_MAX_N]          */
    STEGO_ERR_STITCH_SIZE = 121,    /* H or W outside [1, STEGO_STITCH_MAX_SIDE], win outside [1, STEGO_PROBE_MAX_OUT], hc or wc outside
                                       [1, STEGO_PROBE_MAX_CODE]                                                                        */
    STEGO_ERR_STITCH_LAYOUT = 122,  /* win > H, win > W, 2 * stride < win, or stride > win                                              */
    STEGO_ERR_STITCH_WINDOWS = 123, /* stego_stitch_probe: T != ny * nx of the layout                                                   */
    STEGO_ERR_STITCH_OUTPUT = 124,  /* an output kind outside STEGO_PROBE_*, or both probes skipped                                     */
    STEGO_ERR_STITCH_RANGE = 125    /* stego_window_gather: t0 < 0, n outside [1, 65535], or t0 + n > ny * nx                           */
};

#define STEGO_STITCH_MAX_SIDE 32768  /* canvas rows / columns */

/* The window layout of a canvas. */
typedef struct StegoWindowLayout {
    int32_t H, W;                /* canvas rows, columns (win .. STEGO_STITCH_MAX_SIDE)                  */
    int32_t win;                 /* window side (1 .. STEGO_PROBE_MAX_OUT)                               */
    int32_t stride;              /* window stride, win <= 2 * stride <= 2 * win                          */
} StegoWindowLayout;

typedef struct StegoStitchDesc {
    StegoWindowLayout layout;
    int32_t T;                   /* windows: ny * nx of the layout                                       */
    int32_t K;                   /* code channels (1 .. STEGO_PROBE_MAX_K)                               */
    int32_t hc, wc;              /* code rows, columns of one window                                     */
    int32_t n_lin, n_clu;        /* labels of the linear and the cluster probe (1 .. STEGO_PROBE_MAX_N)  */
    int32_t lin_kind, clu_kind;  /* STEGO_PROBE_*                                                        */
    float alpha;                 /* cluster logits = alpha * cosine                                      */
} StegoStitchDesc;

/* Both probes on the canvas, from the codes of its windows.
 *   code      : float32 [T, K, hc, wc] with arbitrary strides (the head's channels-last view goes in without a copy), window t's code
 *               at index t
 *   code_flip : the codes of the horizontally mirrored windows, same shape, or NULL; flip-averaged per window as in stego_probe_head
 *   lin_w, lin_b, centroids : as for stego_probe_head
 *   lin_out, clu_out : contiguous outputs on the canvas: float32 [n, H, W] (LOG_PROBS, PROBS) or int64 [H, W] (ARGMAX); every
 *               element is written, offsets are 64-bit.  A skipped probe's n, weights and output are not read (any n, NULL).
 * Returns STEGO_ERR_NULL, STEGO_ERR_STITCH_OUTPUT, STEGO_ERR_STITCH_DIM, STEGO_ERR_STITCH_SIZE, STEGO_ERR_STITCH_LAYOUT,
 * STEGO_ERR_STITCH_WINDOWS, STEGO_ERR_ALIGN (a float pointer not 4-byte aligned, an ARGMAX output not 8-byte aligned). */
int stego_stitch_probe(const StegoStitchDesc* desc, const StegoMap* code, const StegoMap* code_flip, const float* lin_w,
                       const float* lin_b, const float* centroids, void* lin_out, void* clu_out, stego_stream_t stream);

/* Host only: the dynamic LDS bytes one workgroup of stego_stitch_probe uses for `desc` (0 for an invalid descriptor; desc->T is not
 * checked), the canvas tile (rows, columns) it was planned for, and the layout's window counts.  Touches no device. */
size_t stego_stitch_probe_plan(const StegoStitchDesc* desc, int32_t* tile_rows, int32_t* tile_cols, int32_t* ny, int32_t* nx);

/* Windows [t0, t0 + n) of an image, as the backbone's input.
 *   img      : float32 [3, H, W] with arbitrary strides (stride_n is not read)
 *   out      : float32 [n, 3, win, win] contiguous: out[i] = img[:, oy : oy + win, ox : ox + win] of window t0 + i
 *   out_flip : the same windows mirrored horizontally (out[i].flip(2)), written in the same launch, or NULL
 * Returns STEGO_ERR_NULL, STEGO_ERR_STITCH_SIZE, STEGO_ERR_STITCH_LAYOUT, STEGO_ERR_STITCH_RANGE, STEGO_ERR_ALIGN. */
int stego_window_gather(const StegoWindowLayout* layout, const StegoMap* img, int32_t t0, int32_t n, float* out, float* out_flip,
                        stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
