/*
 * stego_aug.h - C ABI of the device-side augmented view (stego_augment) and of the fused aug-alignment loss (stego_aug_align),
 * exported by the same libstego_corr.so.
 *
 * The reference makes the view per item on CPU workers with torchvision (data.py:556-563, train_segmentation.py:408-416):
 *     RandomHorizontalFlip -> RandomResizedCrop(res, scale=(0.8, 1)) -> ColorJitter(.3, .3, .3, .1) -> RandomGrayscale(.2) ->
 *     RandomApply([GaussianBlur((5, 5))])
 * and replays the geometric part on a coordinate image.  Here the random draws are made on the host (one record per image,
 * StegoAugParams) and one call turns a float batch into img_aug and coord_aug.  The operators are torchvision's tensor operators,
 * restated; all arithmetic is fp32 and the kernel does not care what range it is given (the reference applies them, clamps to [0, 1]
 * and all, to the NORMALISED image: a quirk that is kept).
 *
 * Geometry (F.resized_crop after hflip; bilinear, align_corners=False, no antialias): for output row y of R,
 *     src = max((float)ch / R * (y + 0.5) - 0.5, 0), y0 = (int)src, y1 = y0 + (y0 < ch - 1), l = src - y0   (the rule of stego_probe.h)
 * columns alike with cw; source row = top + y0/1; source column = left + x0/1, or W - 1 - (left + x0/1) with flip: the crop is given
 * in the coordinates of the flipped image.  value = (1 - ly) ((1 - lx) p00 + lx p01) + ly ((1 - lx) p10 + lx p11).
 * coord_aug[b, y, x, :] is the same transform of the coordinate image: channel 0 = linspace(-1, 1, H)[row] (the ROW ramp,
 * torch.meshgrid's "ij"), channel 1 = linspace(-1, 1, W)[column].
 *
 * Photometric operators on the pixel x = (r, g, b) after the geometry, the four entries of `order` in turn:
 *     gray(x) = 0.2989 r + 0.587 g + 0.114 b;  blend(a, b, f) = clamp(f a + (1 - f) b, 0, 1)
 *     0 brightness  blend(x, 0, f)
 *     1 contrast    blend(x, m, f), m = the mean of gray over the whole R x R image as it is after the operators before contrast
 *     2 saturation  blend(x, gray(x), f)
 *     3 hue         rgb -> hsv (maxc, minc, eqc = maxc == minc, s = cr / where(eqc, 1, maxc), rc, gc, bc over where(eqc, 1, cr),
 *                   h = fmod((hr + hg + hb) / 6 + 1, 1)), h = (h + f) mod 1, hsv -> rgb (i = floor(6 h), f' = 6 h - i, p, q, t clamped
 *                   to [0, 1]).  Hue applied first, to values outside [0, 1], is defined (it divides by maxc: whatever the formulas
 *                   give) but is outside the tested ground; after brightness, contrast or saturation the values are in [0, 1].
 *     4 none
 * then gray (all three channels = gray(x)), then the blur: separable 5 taps k_i ~ exp(-0.5 (i / sigma)^2), i = -2 .. 2, normalised,
 * reflect padding of 2 (index -1 -> 1, -2 -> 2, R -> R - 2, R + 1 -> R - 3), the same sigma on both axes.
 *
 * The aug-alignment loss (train_segmentation.py:189-198 of the reference):
 *     coord = resize(coord_aug.permute(0, 3, 1, 2), S).permute(0, 2, 3, 1)
 *     loss  = -einsum("bkhw,bkhw->bhw", norm(sample(code, coord)), norm(code_aug)).mean()
 * as one call: ds[b, p, q, :] = coord resized to S x S (bilinear, align_corners=False); a[b, :, p, q] = code[b] sampled bilinearly
 * (align_corners=True, border padding) at x = ds[b, q, p, 0], y = ds[b, q, p, 1] (the swapped indices of modules.sample);
 * loss = -(1 / (B S^2)) sum <a / max(|a|, 1e-10), c / max(|c|, 1e-10)>, c = code_aug[b, :, p, q].  Backward for a unit upstream:
 * through both normalisations (d v = (d v^ - (d v^ . v^) v^) / max(|v|, 1e-10); for |v| < 1e-10, as torch's clamp, d v^ / 1e-10
 * without the projection); d_code is the transpose of the four taps; coord gets no gradient.  Neither ds nor a is written to memory.
 * A reference quirk that is reproduced: channel 0 of coord_aug is the row ramp and sample reads channel 0 as x; with the swapped
 * indices the identity transform round-trips, but a horizontally flipped view looks `code` up VERTICALLY flipped.
 *
 * No float atomics: the loss terms are added in a fixed order in fp64, every code cell's taps in ascending (pixel, tap) order, so
 * repeat launches give the same bits.  The transpose gives every code cell to one wave that scans the image's S^2 tap records: its
 * time grows with h w S^2 / 64, and a cell that every pixel touches is summed by one wave alone (S^2 rows, one after the other):
 * hence the limits on the sides below.
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream` (capturable into a
 * HIP graph), STEGO_OK or an error code; every check is on the host, before anything is enqueued.
 */
#ifndef STEGO_AUG_H
#define STEGO_AUG_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_AUG_SIZE = 90,        /* B outside [1, 65535], H or W outside [1, STEGO_AUG_MAX_SIDE], R outside [3, STEGO_AUG_MAX_SIDE]   */
    STEGO_ERR_AUG_PARAM = 91,       /* a record of the parameter table is invalid (the rules at StegoAugParams)                          */
    STEGO_ERR_AUGALIGN_DIM = 92,    /* K outside [1, STEGO_AUGALIGN_MAX_K]                                                               */
    STEGO_ERR_AUGALIGN_SIZE = 93    /* B outside [1, 65535], h, w or S outside [1, STEGO_AUGALIGN_MAX_SIDE], Rh or Rw outside
                                       [1, STEGO_AUG_MAX_SIDE]                                                                           */
};

enum { STEGO_AUG_BRIGHTNESS = 0, STEGO_AUG_CONTRAST = 1, STEGO_AUG_SATURATION = 2, STEGO_AUG_HUE = 3, STEGO_AUG_NONE = 4 };

#define STEGO_AUG_MAX_SIDE 2048        /* rows / columns of the source, the view and the coordinate map        */
#define STEGO_AUG_MIN_RES 3            /* the reflect padding of 2 needs three rows                            */
#define STEGO_AUG_LAUNCHES 2
#define STEGO_AUGALIGN_MAX_K 128       /* code channels                                                        */
#define STEGO_AUGALIGN_MAX_SIDE 256    /* rows / columns of code and code_aug                                  */
#define STEGO_AUGALIGN_LAUNCHES 2

/* One image's draws: 64 bytes (sizeof(StegoAugParams) == 64).  Valid when flip and gray are 0 or 1; 1 <= ch <= H, 1 <= cw <= W,
 * 0 <= top <= H - ch, 0 <= left <= W - cw; every order entry is in [0, 4] and no operator other than STEGO_AUG_NONE occurs twice;
 * the four factors are finite, those of brightness, contrast and saturation >= 0, that of hue in [-0.5, 0.5]; blur_sigma is finite
 * and >= 0 (0 = no blur); reserved is 0. */
typedef struct StegoAugParams {
    int32_t flip;                /* 1: the view is taken from the horizontally flipped image              */
    int32_t top, left, ch, cw;   /* the crop, in the coordinates of the (possibly flipped) image          */
    int32_t order[4];            /* STEGO_AUG_* in the order they are applied                             */
    float factor[4];             /* indexed by operator: brightness, contrast, saturation, hue            */
    int32_t gray;                /* 1: all three channels become gray(x) after the four operators         */
    float blur_sigma;            /* 0: no blur                                                            */
    int32_t reserved;
} StegoAugParams;

typedef struct StegoAugDesc {
    int32_t B;                   /* images (1 .. 65535)                                   */
    int32_t H, W;                /* source rows, columns (1 .. STEGO_AUG_MAX_SIDE)        */
    int32_t R;                   /* side of the view (3 .. STEGO_AUG_MAX_SIDE)            */
} StegoAugDesc;

typedef struct StegoAugAlignDesc {
    int32_t B;                   /* images (1 .. 65535)                                   */
    int32_t K;                   /* code channels (1 .. STEGO_AUGALIGN_MAX_K)             */
    int32_t h, w;                /* rows, columns of code (1 .. STEGO_AUGALIGN_MAX_SIDE)  */
    int32_t S;                   /* side of code_aug (1 .. STEGO_AUGALIGN_MAX_SIDE)       */
    int32_t Rh, Rw;              /* rows, columns of coord (1 .. STEGO_AUG_MAX_SIDE)      */
} StegoAugAlignDesc;

/* Host only: checks the B records at `params_host`.  Returns STEGO_OK, the descriptor's error, STEGO_ERR_NULL, or
 * STEGO_ERR_AUG_PARAM with the index of the first bad record in *bad_record (if given; -1 otherwise).  *any_contrast (if given)
 * tells whether a record applies contrast, that is, whether stego_augment will run its mean pass. */
int stego_augment_check_params(const StegoAugDesc* desc, const StegoAugParams* params_host, int64_t* bad_record, int32_t* any_contrast);

/* Bytes of workspace stego_augment needs for `desc` (the partial sums of the contrast mean); 0 for an invalid descriptor. */
size_t stego_augment_workspace_bytes(const StegoAugDesc* desc);

/* Host only: the LDS bytes of one workgroup and the number of workgroups of the two launches (contrast mean, apply).  Returns
 * STEGO_OK, or the descriptor's error with both arrays zeroed.  Touches no device. */
int stego_augment_plan(const StegoAugDesc* desc, size_t lds_bytes[STEGO_AUG_LAUNCHES], int64_t workgroups[STEGO_AUG_LAUNCHES]);

/* img_aug and coord_aug of B images, in at most two launches (the mean pass is skipped when no record applies contrast).
 *   img         : float32 [B, 3, H, W] with arbitrary strides
 *   params_host : [B] StegoAugParams in host memory: checked here as stego_augment_check_params does, read during the call only
 *   params      : the same B records in device memory (one small copy made by the caller, on `stream` or before it)
 *   img_aug     : float32 [B, 3, R, R] contiguous, 16-byte aligned
 *   coord_aug   : float32 [B, R, R, 2] contiguous, 16-byte aligned
 *   workspace   : at least stego_augment_workspace_bytes(desc) bytes, 16-byte aligned; needs no initialisation
 * Returns STEGO_ERR_NULL, STEGO_ERR_AUG_SIZE, STEGO_ERR_AUG_PARAM, STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN (img not 4-byte aligned,
 * params not 4-byte aligned, an output or the workspace not 16-byte aligned). */
int stego_augment(const StegoAugDesc* desc, const StegoMap* img, const StegoAugParams* params_host, const StegoAugParams* params,
                  float* img_aug, float* coord_aug, void* workspace, size_t workspace_bytes, stego_stream_t stream);

/* Bytes of workspace stego_aug_align needs for `desc` (the loss terms, the gradient rows of the sampled vectors and their tap
 * records); 0 for an invalid descriptor. */
size_t stego_aug_align_workspace_bytes(const StegoAugAlignDesc* desc);

/* Host only: as stego_augment_plan for the two launches of stego_aug_align (pixels, finish) of a call with both gradients. */
int stego_aug_align_plan(const StegoAugAlignDesc* desc, size_t lds_bytes[STEGO_AUGALIGN_LAUNCHES],
                         int64_t workgroups[STEGO_AUGALIGN_LAUNCHES]);

/* The loss and its gradients.
 *   code       : float32 [B, K, h, w] with arbitrary strides
 *   code_aug   : float32 [B, K, S, S] with arbitrary strides
 *   coord      : float32 [B, Rh, Rw, 2] contiguous (coord_aug of stego_augment); values outside [-1, 1] take the border
 *   loss       : float32 [1]
 *   d_code     : NULL, or float32 [B, K, h, w] described by its own four strides; `data` is written, every element (cells no tap
 *                touches get 0); d loss / d code for a unit upstream
 *   d_code_aug : NULL, or float32 [B, K, S, S] likewise
 *   workspace  : at least stego_aug_align_workspace_bytes(desc) bytes, 16-byte aligned; needs no initialisation
 * With either or both gradients NULL the loss has the same bits.
 * Returns STEGO_ERR_NULL, STEGO_ERR_AUGALIGN_DIM, STEGO_ERR_AUGALIGN_SIZE, STEGO_ERR_WORKSPACE, STEGO_ERR_ALIGN (a float pointer
 * not 4-byte aligned, the workspace not 16-byte aligned). */
int stego_aug_align(const StegoAugAlignDesc* desc, const StegoMap* code, const StegoMap* code_aug, const float* coord, float* loss,
                    const StegoMap* d_code, const StegoMap* d_code_aug, void* workspace, size_t workspace_bytes, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
