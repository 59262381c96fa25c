/*
 * stego_data.h - C ABI of the batch preparation of a device-resident image store, exported by the same libstego_corr.so.
 *
 * A whole cropped split (crop_datasets.py's tree) is decoded once on the host and kept on the device as two byte arenas: RGB HWC
 * images and their stored labels (PNG value = label + 1).  One call turns N dataset indices into a training batch at resolution R,
 * what the reference's get_transform(R, _, "center" | "random") + ToTensor + Normalize and CroppedDataset's "target - 1",
 * "mask = target == -1" do per item on the CPU:
 *     img[n, c, y, x] = lut[c * 256 + rgb[row_map[top + y], col_map[left + x], c]]
 *     label[n, y, x]  = lab[row_map[top + y], col_map[left + x]] - 1        (int64)
 *     mask[n, 0, y, x] = label[n, y, x] == -1                               (bool, one byte)
 * The row / column maps are PIL's NEAREST resize of the item to (nh, nw), built on the host (a 1 x src int32 ramp resized to
 * 1 x dst gives the source index of every output column); `lut` is the float32 (u8 / 255 - mean_c) / std_c table computed with the
 * host's numpy, so the result is bitwise what the CPU transform produces.  Deterministic: no atomics, repeat launches give the same
 * bytes.
 *
 * Conventions as in stego_corr.h: device pointers, nothing allocated / freed / synchronised, work enqueued on `stream`, STEGO_OK or
 * an error code; the descriptor is validated on the host before anything is enqueued.
 */
#ifndef STEGO_DATA_H
#define STEGO_DATA_H

#include "stego_corr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    STEGO_ERR_DATA_RES = 30,     /* R outside [1, STEGO_DATA_MAX_RES]                                                        */
    STEGO_ERR_DATA_COUNT = 31,   /* N outside [1, STEGO_DATA_MAX_N], or n_items outside [1, 2^31)                            */
    STEGO_ERR_DATA_ITEM = 32,    /* a table record with h or w < 1, nh or nw < R, or a centre origin outside the resized image */
    STEGO_ERR_DATA_RANGE = 33,   /* a record's arena bytes or index maps outside their arena / map pool                      */
    STEGO_ERR_DATA_ORIGIN = 34   /* an explicit crop origin outside [0, nh - R] x [0, nw - R]                                 */
};

#define STEGO_DATA_MAX_RES 2048          /* output side R                                  */
#define STEGO_DATA_MAX_N 65535           /* items per launch (anchors and positives)       */

/* One stored crop (48 bytes, 8-byte aligned). */
typedef struct StegoDataItem {
    int64_t img_offset;          /* byte offset of its h * w * 3 RGB bytes in the image arena            */
    int64_t label_offset;        /* byte offset of its h * w label bytes in the label arena              */
    int32_t h, w;                /* stored size (>= 1)                                                   */
    int32_t nh, nw;              /* size after the resize (short side R; >= R)                           */
    int32_t row_map, col_map;    /* offsets into the map pool of its nh row / nw column source indices  */
    int32_t center_top, center_left;   /* CenterCrop(R)'s origin: int(round((n - R) / 2)), round half to even */
} StegoDataItem;

typedef struct StegoDataDesc {
    int32_t N;                   /* items of this launch (1 .. STEGO_DATA_MAX_N)                          */
    int32_t R;                   /* output side (1 .. STEGO_DATA_MAX_RES)                                 */
    int64_t n_items;             /* records of the table                                                  */
    int64_t img_arena_bytes;     /* size of the image arena                                               */
    int64_t label_arena_bytes;   /* size of the label arena                                               */
    int64_t map_pool_len;        /* int32 entries of the map pool                                         */
} StegoDataDesc;

/* Host check of a table (host copy of the records the device table holds) against `desc` (R, n_items and the arena / pool sizes):
 * returns STEGO_OK, or STEGO_ERR_DATA_ITEM / STEGO_ERR_DATA_RANGE and the first bad record's index in *bad_item.  Touches no device.
 * A table that passes it keeps every read of stego_data_prepare inside the arenas and the pool. */
int stego_data_check_items(const StegoDataDesc* desc, const StegoDataItem* items_host, int64_t* bad_item);

/* The batch of `desc.N` items:
 *   items   : [n_items] StegoDataItem (device), checked with stego_data_check_items when it was built
 *   img_arena, label_arena : uint8 (device); map_pool : int32 [map_pool_len] (device); lut : float32 [3 * 256] (device)
 *   index   : int64 [N] dataset indices (device)
 *   origin  : int32 [N, 2] (top, left) in resized coordinates (device), or NULL for every record's centre origin
 *   img     : float32 [N, 3, R, R];  label : int64 [N, R, R];  mask : bool [N, 1, R, R]   (device, contiguous)
 * Returns STEGO_ERR_NULL, STEGO_ERR_ALIGN (img / label / lut / map_pool / index / origin / items not aligned to their element),
 * STEGO_ERR_DATA_RES, STEGO_ERR_DATA_COUNT, all before anything is enqueued.  Indices and origins live on the device and are not
 * checked there: an index outside [0, n_items) or an origin outside the resized image is clamped into range (reads stay inside the
 * arenas; the batch is then not what was asked for).  The host wrapper rejects both before the launch when they are known. */
int stego_data_prepare(const StegoDataDesc* desc, const StegoDataItem* items, const uint8_t* img_arena, const uint8_t* label_arena,
                       const int32_t* map_pool, const float* lut, const int64_t* index, const int32_t* origin, float* img,
                       int64_t* label, uint8_t* mask, stego_stream_t stream);

/* The same batch for a directory store (the user's own image folder, data.py DirectoryDataset): descriptor, records, maps, lut, index
 * and origin as for stego_data_prepare, with the directory dataset's label rule:
 *     label[n, y, x]   = lab[row_map[top + y], col_map[left + x]]          (int64: the stored byte itself, no "- 1")
 *     mask[n, 0, y, x] = label[n, y, x] > 0 ? 1.0f : 0.0f                  (float32: the salience mask of cfg.use_salience)
 * `label_arena` may be NULL - a folder without labels: label is -1 everywhere and mask 0; the records' label_offset and
 * desc.label_arena_bytes are then not used.  mask : float32 [N, 1, R, R].  The same host checks and error codes, with the float mask
 * aligned like img (16 bytes when R % 4 == 0, else 4), all before anything is enqueued.  Deterministic, no atomics. */
int stego_data_prepare_dir(const StegoDataDesc* desc, const StegoDataItem* items, const uint8_t* img_arena, const uint8_t* label_arena,
                           const int32_t* map_pool, const float* lut, const int64_t* index, const int32_t* origin, float* img,
                           int64_t* label, float* mask, stego_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
