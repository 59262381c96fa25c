// Batch preparation of a directory store (include/stego_data.h, stego_data_prepare_dir): N dataset indices -> img float32 [N,3,R,R],
// label int64 [N,R,R], mask float32 [N,1,R,R] in one launch.  The layout of csrc/batch_prep.hip's kernel - grid (units of one item /
// 256 threads, N items), a thread owns V consecutive output pixels of one item in raster order (V = 16 when R % 4 == 0, V = 1
// otherwise), the normalisation table in LDS - with the directory dataset's label rule: label = the stored byte (no "- 1"), or -1
// everywhere when the store has no label arena, and mask = 1.0f where label > 0.  With V = 16 a lane writes each image plane and the
// float mask with four 16-byte stores and the labels with eight: 24 output bytes per pixel.  No atomics: the bytes are a pure function
// of the inputs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/stego_data.h"
#include "host_util.h"

namespace {

constexpr int TPB = 256;

struct DirPrepParams {
    const StegoDataItem* items;
    const uint8_t* img_arena;
    const uint8_t* label_arena;      // nullptr: no labels
    const int32_t* map_pool;
    const float* lut;
    const int64_t* index;
    const int32_t* origin;
    float* img;
    int64_t* label;
    float* mask;
    int64_t n_items;
    int32_t R;
};

template <int V>
__global__ __launch_bounds__(TPB) void dir_prep_kernel(DirPrepParams p)
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
    const bool labelled = p.label_arena != nullptr;
    const uint8_t* lsrc = labelled ? p.label_arena + it.label_offset : nullptr;

    float f0[V], f1[V], f2[V], msk[V];
    int64_t lab[V];
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
        const int l = labelled ? (int)lsrc[o] : -1;
        lab[v] = (int64_t)l;
        msk[v] = l > 0 ? 1.0f : 0.0f;
        if (V > 1 && ++x == R && v + 1 < V) {
            x = 0;
            sy = min(rmap[++y], it.h - 1);
        }
    }

    float* o0 = p.img + ((int64_t)n * 3) * P + p0;
    int64_t* ol = p.label + (int64_t)n * P + p0;
    float* om = p.mask + (int64_t)n * P + p0;
    if constexpr (V == 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            reinterpret_cast<float4*>(o0)[q] = make_float4(f0[4 * q], f0[4 * q + 1], f0[4 * q + 2], f0[4 * q + 3]);
            reinterpret_cast<float4*>(o0 + P)[q] = make_float4(f1[4 * q], f1[4 * q + 1], f1[4 * q + 2], f1[4 * q + 3]);
            reinterpret_cast<float4*>(o0 + 2 * P)[q] = make_float4(f2[4 * q], f2[4 * q + 1], f2[4 * q + 2], f2[4 * q + 3]);
            reinterpret_cast<float4*>(om)[q] = make_float4(msk[4 * q], msk[4 * q + 1], msk[4 * q + 2], msk[4 * q + 3]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            reinterpret_cast<longlong2*>(ol)[q] = make_longlong2(lab[2 * q], lab[2 * q + 1]);
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

}  // namespace

extern "C" int stego_data_prepare_dir(const StegoDataDesc* desc, const StegoDataItem* items, const uint8_t* img_arena,
                                      const uint8_t* label_arena, const int32_t* map_pool, const float* lut, const int64_t* index,
                                      const int32_t* origin, float* img, int64_t* label, float* mask, stego_stream_t stream)
{
    if (!desc) return STEGO_ERR_NULL;
    if (desc->R < 1 || desc->R > STEGO_DATA_MAX_RES) return STEGO_ERR_DATA_RES;
    if (desc->N < 1 || desc->N > STEGO_DATA_MAX_N || desc->n_items < 1 || desc->n_items > INT32_MAX) return STEGO_ERR_DATA_COUNT;
    if (desc->img_arena_bytes < 0 || desc->label_arena_bytes < 0 || desc->map_pool_len < 0) return STEGO_ERR_DATA_RANGE;
    if (!items || !img_arena || !map_pool || !lut || !index || !img || !label || !mask) return STEGO_ERR_NULL;
    const bool vec = desc->R % 4 == 0;
    if (!aligned(items, 8) || !aligned(map_pool, 4) || !aligned(lut, 4) || !aligned(index, 8) || (origin && !aligned(origin, 4)) ||
        !aligned(img, vec ? 16 : 4) || !aligned(label, vec ? 16 : 8) || !aligned(mask, vec ? 16 : 4))
        return STEGO_ERR_ALIGN;
    DirPrepParams p{items, img_arena, label_arena, map_pool, lut, index, origin, img, label, mask, desc->n_items, desc->R};
    const int64_t P = (int64_t)desc->R * desc->R;
    const int V = vec ? 16 : 1;
    const dim3 grid((unsigned)((P / V + TPB - 1) / TPB), (unsigned)desc->N);
    (void)hipGetLastError();
    if (vec)
        dir_prep_kernel<16><<<grid, TPB, 0, static_cast<hipStream_t>(stream)>>>(p);
    else
        dir_prep_kernel<1><<<grid, TPB, 0, static_cast<hipStream_t>(stream)>>>(p);
    return hip_rc(hipGetLastError());
}
