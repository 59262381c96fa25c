// Batch preparation of the device-resident image store (include/stego_data.h): N dataset indices -> img float32 [N,3,R,R],
// label int64 [N,R,R], mask bool [N,1,R,R] in one launch.
//
// Grid: (units of one item / 256 threads, N items).  A thread owns V consecutive output pixels of one item in raster order (V = 16
// when R % 4 == 0, so that R * R is a multiple of 16 and every plane of every item starts 64-byte aligned; V = 1 otherwise).  Per
// pixel: the row and column maps give the source pixel, its three RGB bytes and its label byte are read from the arenas (the rows of
// one output row are contiguous in the source, so neighbouring lanes hit the same cache lines), and the normalisation is a lookup in
// the 3 x 256 float32 table held in LDS.  With V = 16 every plane is written with four 16-byte stores per lane, the labels with eight
// and the mask with one: the outputs (21 bytes per pixel) are nearly all of the traffic.  No atomics: the bytes are a pure function of
// the inputs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/stego_data.h"
#include "host_util.h"

namespace {

constexpr int TPB = 256;

struct PrepParams {
    const StegoDataItem* items;
    const uint8_t* img_arena;
    const uint8_t* label_arena;
    const int32_t* map_pool;
    const float* lut;
    const int64_t* index;
    const int32_t* origin;
    float* img;
    int64_t* label;
    uint8_t* mask;
    int64_t n_items;
    int32_t R;
};

template <int V>
__global__ __launch_bounds__(TPB) void batch_prep_kernel(PrepParams p)
{
    __shared__ float lut[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += TPB) lut[i] = p.lut[i];

    const int n = blockIdx.y;
    const int R = p.R;
    int64_t ind = p.index[n];
    ind = ind < 0 ? 0 : (ind >= p.n_items ? p.n_items - 1 : ind);       // memory safety only: the wrapper rejects bad indices
    const StegoDataItem it = p.items[ind];
    int top = it.center_top, left = it.center_left;
    if (p.origin) {
        top = min(max(p.origin[2 * n], 0), it.nh - R);
        left = min(max(p.origin[2 * n + 1], 0), it.nw - R);
    }
    __syncthreads();

    const int64_t P = (int64_t)R * R;
    const int64_t p0 = ((int64_t)blockIdx.x * TPB + threadIdx.x) * V;
    if (p0 >= P) return;
    const int32_t* rmap = p.map_pool + it.row_map + top;
    const int32_t* cmap = p.map_pool + it.col_map + left;
    const uint8_t* src = p.img_arena + it.img_offset;
    const uint8_t* lsrc = p.label_arena + it.label_offset;

    float f0[V], f1[V], f2[V];
    int64_t lab[V];
    uint8_t msk[V];
    int y = (int)(p0 / R), x = (int)(p0 - (int64_t)y * R);
    int sy = min(rmap[y], it.h - 1);
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int sx = min(cmap[x], it.w - 1);
        const int64_t o = (int64_t)sy * it.w + sx;
        const uint8_t* px = src + o * 3;
        f0[v] = lut[px[0]];
        f1[v] = lut[256 + px[1]];
        f2[v] = lut[512 + px[2]];
        const int l = lsrc[o];
        lab[v] = (int64_t)l - 1;
        msk[v] = l == 0;
        if (V > 1 && ++x == R && v + 1 < V) {
            x = 0;
            sy = min(rmap[++y], it.h - 1);
        }
    }

    float* o0 = p.img + ((int64_t)n * 3) * P + p0;
    int64_t* ol = p.label + (int64_t)n * P + p0;
    uint8_t* om = p.mask + (int64_t)n * P + p0;
    if constexpr (V == 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            reinterpret_cast<float4*>(o0)[q] = make_float4(f0[4 * q], f0[4 * q + 1], f0[4 * q + 2], f0[4 * q + 3]);
            reinterpret_cast<float4*>(o0 + P)[q] = make_float4(f1[4 * q], f1[4 * q + 1], f1[4 * q + 2], f1[4 * q + 3]);
            reinterpret_cast<float4*>(o0 + 2 * P)[q] = make_float4(f2[4 * q], f2[4 * q + 1], f2[4 * q + 2], f2[4 * q + 3]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            reinterpret_cast<longlong2*>(ol)[q] = make_longlong2(lab[2 * q], lab[2 * q + 1]);
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            w[q] = (uint32_t)msk[4 * q] | ((uint32_t)msk[4 * q + 1] << 8) | ((uint32_t)msk[4 * q + 2] << 16) | ((uint32_t)msk[4 * q + 3] << 24);
        *reinterpret_cast<uint4*>(om) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        o0[0] = f0[0];
        o0[P] = f1[0];
        o0[2 * P] = f2[0];
        ol[0] = lab[0];
        om[0] = msk[0];
    }
}

using stego::aligned;
using stego::hip_rc;

int check_desc(const StegoDataDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->R < 1 || d->R > STEGO_DATA_MAX_RES) return STEGO_ERR_DATA_RES;
    if (d->N < 1 || d->N > STEGO_DATA_MAX_N || d->n_items < 1 || d->n_items > INT32_MAX) return STEGO_ERR_DATA_COUNT;
    if (d->img_arena_bytes < 0 || d->label_arena_bytes < 0 || d->map_pool_len < 0) return STEGO_ERR_DATA_RANGE;
    return STEGO_OK;
}

}  // namespace

extern "C" int stego_data_check_items(const StegoDataDesc* desc, const StegoDataItem* items, int64_t* bad_item)
{
    if (!desc || !items) return STEGO_ERR_NULL;
    if (desc->R < 1 || desc->R > STEGO_DATA_MAX_RES) return STEGO_ERR_DATA_RES;
    if (desc->n_items < 1 || desc->n_items > INT32_MAX) return STEGO_ERR_DATA_COUNT;
    const int64_t R = desc->R;
    for (int64_t i = 0; i < desc->n_items; ++i) {
        const StegoDataItem& it = items[i];
        int rc = STEGO_OK;
        if (it.h < 1 || it.w < 1 || it.nh < R || it.nw < R || it.center_top < 0 || it.center_top > it.nh - R || it.center_left < 0 ||
            it.center_left > it.nw - R)
            rc = STEGO_ERR_DATA_ITEM;
        else if (it.img_offset < 0 || it.label_offset < 0 || it.row_map < 0 || it.col_map < 0 ||
                 it.img_offset > desc->img_arena_bytes - (int64_t)it.h * it.w * 3 ||
                 it.label_offset > desc->label_arena_bytes - (int64_t)it.h * it.w || (int64_t)it.row_map + it.nh > desc->map_pool_len ||
                 (int64_t)it.col_map + it.nw > desc->map_pool_len)
            rc = STEGO_ERR_DATA_RANGE;
        if (rc != STEGO_OK) {
            if (bad_item) *bad_item = i;
            return rc;
        }
    }
    return STEGO_OK;
}

extern "C" int stego_data_prepare(const StegoDataDesc* desc, const StegoDataItem* items, const uint8_t* img_arena, const uint8_t* label_arena,
                                  const int32_t* map_pool, const float* lut, const int64_t* index, const int32_t* origin, float* img,
                                  int64_t* label, uint8_t* mask, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!items || !img_arena || !label_arena || !map_pool || !lut || !index || !img || !label || !mask) return STEGO_ERR_NULL;
    const bool vec = desc->R % 4 == 0;
    if (!aligned(items, 8) || !aligned(map_pool, 4) || !aligned(lut, 4) || !aligned(index, 8) || (origin && !aligned(origin, 4)) ||
        !aligned(img, vec ? 16 : 4) || !aligned(label, vec ? 16 : 8) || (vec && !aligned(mask, 16)))
        return STEGO_ERR_ALIGN;
    PrepParams p{items, img_arena, label_arena, map_pool, lut, index, origin, img, label, mask, desc->n_items, desc->R};
    const int64_t P = (int64_t)desc->R * desc->R;
    const int V = vec ? 16 : 1;
    const dim3 grid((unsigned)((P / V + TPB - 1) / TPB), (unsigned)desc->N);
    (void)hipGetLastError();
    if (vec)
        batch_prep_kernel<16><<<grid, TPB, 0, static_cast<hipStream_t>(stream)>>>(p);
    else
        batch_prep_kernel<1><<<grid, TPB, 0, static_cast<hipStream_t>(stream)>>>(p);
    return hip_rc(hipGetLastError());
}
