/*
 * stego_render.h - C ABI of the coloured segmentation pictures, exported by the same libstego_corr.so.
 *
 * Replaces, per pixel and on the device, what the reference draws on the host (src/eval_segmentation.py:181-193,
 * src/utils.py:23-32 prep_for_plot):
 *     plot_img   = (prep_for_plot(img) * 255).astype(np.uint8)        un-normalise, rescale to the image's own range, truncate
 *     plot_label = label_cmap[label].astype(np.uint8)                 a table look-up; numpy wraps label -1 to the last entry
 * by one launch that writes packed uint8 RGB, into a tensor of its own or into a panel of a larger sheet.
 *
 * Un-normalisation of channel c:  v = x * std[c] + mean[c], a rounded multiply and then a rounded add (the reference's mul_ then
 * add_): never a fused multiply-add.  stego_image_range gives (lo, hi) = (min, max) of v over the three channels of an image.
 *
 * Per pixel (y, x) of image b, with l its label:
 *   labels only   rgb = lut[l] if 0 <= l < n_lut, else ignore_rgb.  Exact.
 *   EDGES         a pixel whose label differs from the label of its right neighbour (x + 1 < W) or of its lower neighbour
 *                 (y + 1 < H) gets edge_rgb instead.  The labels are compared as they are stored, before the range test.  The
 *                 neighbours come from the workgroup's label tile, which has a one-pixel halo.
 *   image only    u8 = (uint8) (v' * 255.f), truncated, per channel.  With RESCALE v' = (v - lo) / (hi - lo) with the image's
 *                 (lo, hi) of `range`, and 0 where hi == lo (the reference divides 0 by 0 there); without it v' = min(max(v, 0), 1).
 *                 The product is clamped to [0, 255] before the conversion, a NaN gives 0.
 *   BLEND         f = (1 - alpha) * v' + alpha * (rgb / 255.f), every operation rounded to fp32 on its own, then the same
 *                 truncation.  rgb is the labels-only colour, with EDGES the edge colour.  alpha = 0 gives the image-only bytes,
 *                 alpha = 1 the labels-only bytes.
 *
 * The output target is a base pointer with a byte stride per image and per row; a pixel is 3 consecutive bytes (R, G, B), a row
 * 3 * W consecutive bytes.  The base and the strides need no alignment.  Exactly the B * H * (3 * W) bytes of the panel are
 * written: the body of a row leaves as 16-byte stores of 16-byte aligned addresses, staged through LDS, and only the bytes of a
 * row in front of its first and behind its last aligned 16 bytes leave as byte stores.  Rows that overlap are the caller's error.
 * No atomics: repeat launches are bitwise equal.
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_RENDER_H
#define STEGO_RENDER_H

#include "stego_stitch.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_RENDER_SIZE = 150,    /* B outside [1, 65535], H or W outside [1, STEGO_STITCH_MAX_SIDE]                              */
    STEGO_ERR_RENDER_LUT = 151,     /* labels selected and n_lut outside [1, STEGO_RENDER_MAX_LUT]                                  */
    STEGO_ERR_RENDER_DTYPE = 152,   /* labels selected and label_dtype outside STEGO_RENDER_I64 / I32 / U8                          */
    STEGO_ERR_RENDER_FLAGS = 153,   /* a flag bit outside STEGO_RENDER_*                                                            */
    STEGO_ERR_RENDER_PARAM = 154,   /* alpha outside [0, 1] or not finite; a mean or std that is not finite                         */
    STEGO_ERR_RENDER_SELECT = 155   /* neither IMAGE nor LABELS; BLEND without both; EDGES without LABELS; RESCALE without IMAGE    */
};

/* StegoRenderDesc.flags */
enum {
    STEGO_RENDER_IMAGE = 1,         /* `image` is read                                                                              */
    STEGO_RENDER_LABELS = 2,        /* `labels` and `lut` are read                                                                  */
    STEGO_RENDER_EDGES = 4,         /* label boundaries in edge_rgb (needs LABELS)                                                  */
    STEGO_RENDER_BLEND = 8,         /* image under the label colours (needs IMAGE and LABELS); without it IMAGE and LABELS together
                                       are an error                                                                                 */
    STEGO_RENDER_RESCALE = 16       /* the image's own range from `range` (needs IMAGE); without it v is clamped to [0, 1]          */
};

/* StegoRenderDesc.label_dtype */
enum { STEGO_RENDER_I64 = 0, STEGO_RENDER_I32 = 1, STEGO_RENDER_U8 = 2 };

#define STEGO_RENDER_MAX_LUT 512

typedef struct StegoRenderDesc {
    int32_t B, H, W;                /* images (1 .. 65535), rows, columns (1 .. STEGO_STITCH_MAX_SIDE)              */
    int32_t n_lut;                  /* entries of the colour table (1 .. STEGO_RENDER_MAX_LUT)                      */
    int32_t label_dtype;            /* STEGO_RENDER_I64 / I32 / U8                                                  */
    int32_t flags;                  /* STEGO_RENDER_*                                                               */
    float alpha;                    /* BLEND: weight of the label colour (0 .. 1)                                   */
    float mean[3], std[3];          /* un-normalisation per channel                                                 */
    uint8_t ignore_rgb[4];          /* colour of a label outside [0, n_lut); byte 3 is not read                     */
    uint8_t edge_rgb[4];            /* colour of a label boundary; byte 3 is not read                               */
    int64_t label_stride_n, label_stride_h, label_stride_w;   /* of `labels`, in elements                           */
    int64_t out_stride_n, out_stride_h;                       /* of `out`, in bytes                                 */
} StegoRenderDesc;

/* Bytes of workspace stego_image_range needs for `desc` (B, H, W, mean and std are read); 0 for an invalid descriptor.  Host only. */
size_t stego_image_range_workspace_bytes(const StegoRenderDesc* desc);

/* range[b] = (lo, hi), the minimum and the maximum of the un-normalised image b over its three channels.
 *   image     : float32 [B, 3, H, W] with arbitrary strides; NaNs are passed over
 *   range     : float32 [B, 2]
 *   workspace : at least stego_image_range_workspace_bytes(desc) bytes, 4-byte aligned, needs no initialisation: every workgroup
 *               of the first launch leaves its (lo, hi), a second launch of B workgroups reduces them.  Minimum and maximum do
 *               not depend on the order: the result is exact and repeatable.
 * Of the descriptor B, H, W, mean and std are read.  Returns STEGO_ERR_NULL, STEGO_ERR_RENDER_SIZE, STEGO_ERR_RENDER_PARAM,
 * STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN. */
int stego_image_range(const StegoRenderDesc* desc, const StegoMap* image, float* range, void* workspace, size_t workspace_bytes,
                      stego_stream_t stream);

/* The picture, one launch.
 *   image  : float32 [B, 3, H, W] with arbitrary strides (IMAGE), else not read
 *   labels : [B, H, W] of label_dtype with the descriptor's element strides (LABELS), else not read
 *   lut    : n_lut packed RGB entries, 3 * n_lut bytes (LABELS), else not read; kept in LDS
 *   range  : float32 [B, 2] of stego_image_range (RESCALE), else not read
 *   out    : the target, B * H * 3 * W bytes at out + b * out_stride_n + y * out_stride_h + 3 * x
 * Returns STEGO_ERR_NULL (desc, out, or an input the flags select), STEGO_ERR_RENDER_*, STEGO_ERR_ALIGN (image or range not 4-byte
 * aligned, labels not aligned to their element). */
int stego_render(const StegoRenderDesc* desc, const StegoMap* image, const void* labels, const uint8_t* lut, const float* range,
                 uint8_t* out, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
