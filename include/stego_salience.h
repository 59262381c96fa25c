/*
 * stego_salience.h - C ABI of the salience-guided coordinate draws of the loss (cfg.use_salience), exported by the same
 * libstego_corr.so.
 *
 * The reference (modules.py:298-311, 355-365) draws, per image and side, S * S sample points among the nonzero pixels of a salience
 * mask: torch.nonzero, then a Python loop over the batch with boolean indexing and a host randint per image.  Here both sides of the
 * whole batch come out of ONE launch from uniform numbers the caller draws on the device.  For side w in {1, 2}, image b and sample
 * j < S * S, with c the number of nonzeros of mask_w[b] ("nonzero" is torch's: -0.0 is zero, NaN is not):
 *     c > 0 :  r = min((int)(u[w, b, j, 0] * (float)c), c - 1)            (fp32);  (y, x) = the r-th nonzero in row-major order
 *     c == 0:  y = min((int)(u[w, b, j, 1] * (float)H), H - 1),  x = min((int)(u[w, b, j, 2] * (float)H), H - 1)
 *              (both from H: the reference draws randint(t.shape[1]) for both coordinates)
 *     nz = ((float)x / (float)H * 2 - 1, (float)y / (float)H * 2 - 1)     (the flip to (x, y), and the division by H for both)
 *     coords_w[b, j] = u_mix[b, j] > 0.1f ? nz : reg_w[b, j]              (one mix mask for both sides)
 * One workgroup per (side, image): a ballot / popcount pass over the flat mask in 64-pixel chunks, a two-level exclusive scan of the
 * chunk counts in LDS (per chunk inside its block of 64 chunks, and over the blocks), a binary search of every sample's rank over both
 * levels, and the k-th set bit of the chunk's ballot, which is re-read.  No atomics, no workspace, nothing read back: deterministic,
 * and legal under stream capture.
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; everything is validated on the host before anything is enqueued.
 */
#ifndef STEGO_SALIENCE_H
#define STEGO_SALIENCE_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_SALIENCE_SIZE = 130,      /* B outside [1, 65535], H or W < 1, or H * W > STEGO_SALIENCE_MAX_PIXELS */
    STEGO_ERR_SALIENCE_SAMPLES = 131,   /* S outside [1, 16]                                                      */
    STEGO_ERR_SALIENCE_DTYPE = 132      /* mask_dtype neither STEGO_SALIENCE_U8 nor STEGO_SALIENCE_F32            */
};

#define STEGO_SALIENCE_MAX_PIXELS (1 << 20)
#define STEGO_SALIENCE_MAX_S 16
#define STEGO_SALIENCE_MAX_B 65535

enum { STEGO_SALIENCE_U8 = 0 /* uint8 / bool, one byte per pixel */, STEGO_SALIENCE_F32 = 1 };

typedef struct StegoSalienceDesc {
    int32_t B, H, W;             /* masks [B, H, W], contiguous                   */
    int32_t S;                   /* S * S samples per image and side              */
    int32_t mask_dtype;          /* STEGO_SALIENCE_U8 / STEGO_SALIENCE_F32        */
} StegoSalienceDesc;

/*   mask1, mask2     : [B, H, W] of mask_dtype (device)
 *   u                : float32 [2, B, S * S, 3] uniform in [0, 1);  u_mix : float32 [B, S * S]
 *   reg1, reg2       : float32 [B, S * S, 2], the coordinates kept where u_mix <= 0.1
 *   coords1, coords2 : float32 [B, S * S, 2] (out)
 * Returns STEGO_ERR_NULL, STEGO_ERR_SALIENCE_SAMPLES / _SIZE / _DTYPE, STEGO_ERR_ALIGN (a float32 buffer not 4-byte aligned), all
 * before anything is enqueued. */
int stego_salience_coords(const StegoSalienceDesc* desc, const void* mask1, const void* mask2, const float* u, const float* u_mix,
                          const float* reg1, const float* reg2, float* coords1, float* coords2, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
