// Region descriptors (include/stego_region_pool.h): the mean of a low-resolution map over every full-resolution region of an id map.
//
//   range    a grid-stride pass over the map in its own memory order (the host picks channels or columns as the fastest index from the
//            strides): the largest |value| of every workgroup goes to the workspace as float bits, which order like the magnitudes.  The
//            same launch resets the int64 sums with 16-byte stores.  The later launches reduce the at most 1024 partials themselves (four
//            loads a thread, one barrier), so no workgroup waits for another and nothing needs a reset in front of the call.
//   pool     a wave per (image, row, segment, channel block).  Lanes are channels: lane and lane + 64 of a block of 128, so the loads of a
//            channels-last map and the flush are contiguous across the wave.  For C <= 32 the wave is cut into groups of G = 2^ceil(log2 C)
//            lanes and group g takes the pixels g, g + 64 / G, ... of the segment: neighbouring groups read neighbouring pixels, and a
//            group goes on summing while the id it sees stays the same - the pixels between belong to the other groups, and the sum does
//            not depend on who adds what.  With one group (C > 32) whether a pixel starts a new run is wave-uniform.
//            A lane keeps the four cells of its taps in registers until the left column moves; the right column and the lower row are
//            loaded only where their weight is not zero (0 * finite adds nothing), so the identity case costs one load a pixel.
//            Values are quantised at the pixel and summed in int64 registers; a run costs one 64-bit integer atomic add per lane.
//   finish   four outputs a thread: (double) S * 2^-s / area, a 16-byte store where `out` allows it.
//
// Bounds: X < W and Y < H index ids; the taps are clamped to [0, h - 1] x [0, w - 1] by construction; a row key is used only when
// lo <= row_offset[b] + id < hi, so an id the table does not know adds nothing and nothing is written outside the workspace.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/stego_region_pool.h"
#include "host_util.h"
#include "ws_layout.h"

using namespace stego;

// The header's arithmetic is a sequence of individually rounded operations plus the fused multiply-adds it names: contraction is off for
// the whole unit (as in render.hip) and the fused ones are written out.
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int CB = STEGO_REGION_POOL_CB;
constexpr int MAX_PARTIALS = STEGO_REGION_POOL_PARTIALS;
constexpr int RANGE_PER_THREAD = 16;          // map elements of a thread the range grid is sized for
constexpr int BASE_SEGMENT = 64;              // pixels of a segment with one group a wave
constexpr int MAX_SEGMENT_GROUPS = 8;         // ... times min(groups, 8) with more
constexpr size_t RED_LDS = WAVES * sizeof(uint32_t);

struct PoolParams {
    StegoMap map;
    const int32_t* ids;
    const int64_t* row_offset;
    const int32_t* area;
    float* out;
    int64_t* sums;                            // [hi - lo][C]
    uint32_t* partial;                        // [n_partial]: float bits of a workgroup's largest |map|
    int64_t hw, lo, hi, n_sums, n_map;
    int64_t d1, d2, d3, s0, s1, s2, s3;       // the range's index order: (B, d1, d2, d3) with d3 the fastest, and their strides
    float scale_h, scale_w;
    int C, h, w, H, W;
    int n_partial, gl, seg, nseg, out_wide;
};

// src_index of probe_common.h with every operation rounded on its own
__device__ __forceinline__ void taps(int dst, float scale, int in, int& i0, int& i1, float& l1)
{
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

__device__ __forceinline__ float tap4(float h0, float h1, float w0, float w1, float a, float b, float c, float d)
{
    return __builtin_fmaf(h0, __builtin_fmaf(w0, a, w1 * b), h1 * __builtin_fmaf(w0, c, w1 * d));
}

__device__ __forceinline__ int64_t quantise(float v, int s) { return (int64_t)(int)rintf(ldexpf(v, s)); }     // |v * 2^s| <= 2^30

__device__ __forceinline__ uint32_t wave_max(uint32_t m)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    return m;
}

// every thread of the workgroup calls it: the float bits of M
__device__ __forceinline__ uint32_t block_max_bits(const PoolParams& p, uint32_t* red)
{
    uint32_t m = 0;
    for (int k = threadIdx.x; k < p.n_partial; k += TPB) m = max(m, p.partial[k]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    return max(max(red[0], red[1]), max(red[2], red[3]));
}

template <class I>
__device__ __forceinline__ uint32_t abs_bits_at(const PoolParams& p, I i)
{
    const I d1 = (I)p.d1, d2 = (I)p.d2, d3 = (I)p.d3;
    const I q3 = i / d3, i3 = i - q3 * d3;
    const I q2 = q3 / d2, i2 = q3 - q2 * d2;
    const I q1 = q2 / d1, i1 = q2 - q1 * d1;
    const float v = p.map.data[(int64_t)q1 * p.s0 + (int64_t)i1 * p.s1 + (int64_t)i2 * p.s2 + (int64_t)i3 * p.s3];
    return __float_as_uint(v) & 0x7fffffffu;
}

template <class I>
__device__ __forceinline__ uint32_t range_scan(const PoolParams& p, int64_t t, int64_t nt)
{
    uint32_t m = 0;
    for (int64_t i = t; i < p.n_map; i += 4 * nt) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i + k * nt < p.n_map ? abs_bits_at<I>(p, (I)(i + k * nt)) : 0u;
        m = max(max(m, max(v[0], v[1])), max(v[2], v[3]));
    }
    return m;
}

__global__ __launch_bounds__(TPB) void region_pool_range_kernel(const PoolParams p)
{
    __shared__ uint32_t red[WAVES];
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x, nt = (int64_t)gridDim.x * TPB;
    longlong2* pairs = reinterpret_cast<longlong2*>(p.sums);
    for (int64_t i = t; i < (p.n_sums >> 1); i += nt) pairs[i] = make_longlong2(0, 0);
    if (t == 0 && (p.n_sums & 1)) p.sums[p.n_sums - 1] = 0;
    uint32_t m = p.n_map <= (int64_t)INT32_MAX ? range_scan<uint32_t>(p, t, nt) : range_scan<int64_t>(p, t, nt);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) p.partial[blockIdx.x] = max(max(red[0], red[1]), max(red[2], red[3]));
}

__device__ __forceinline__ void flush(const PoolParams& p, int64_t key, int c, int64_t acc)
{
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(&p.sums[key * p.C + c]), (unsigned long long)acc, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(TPB) void region_pool_kernel(const PoolParams p)
{
    __shared__ uint32_t red[WAVES];
    const uint32_t mbits = block_max_bits(p, red);
    if (mbits == 0) return;                                              // M == 0: the sums stay zero
    const int s = 156 - (int)(mbits >> 23);                              // 30 - e
    const int lane = threadIdx.x & 63;
    const int64_t seg_id = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (seg_id >= (int64_t)p.H * p.nseg) return;
    const int Y = (int)(seg_id / p.nseg), sx = (int)(seg_id - (int64_t)Y * p.nseg);
    const int b = blockIdx.z;
    const int g = lane >> p.gl, ng = 64 >> p.gl;                         // the lane's group, the groups of the wave
    const int c0 = blockIdx.y * CB + (lane & ((1 << p.gl) - 1));         // the lane's channels: c0 and, with one group, c0 + 64
    if (c0 >= p.C) return;
    const bool two = p.gl == 6 && c0 + 64 < p.C;

    int y0, y1;
    float h1;
    taps(Y, p.scale_h, p.h, y0, y1, h1);
    const float h0 = 1.f - h1;
    const bool tall = h1 != 0.f;
    const float* m0 = p.map.data + (int64_t)b * p.map.stride_n + (int64_t)c0 * p.map.stride_c;
    const float* m1 = m0 + 64 * p.map.stride_c;
    const int64_t r0 = (int64_t)y0 * p.map.stride_h, r1 = (int64_t)y1 * p.map.stride_h;

    const int x_begin = sx * p.seg, x_end = x_begin + min(p.seg, p.W - x_begin);
    const int32_t* idrow = p.ids + (int64_t)b * p.hw + (int64_t)Y * p.W;
    const int64_t off = p.row_offset[b];

    int64_t cur = -1, acc0 = 0, acc1 = 0;
    int cx0 = -1;
    bool have_right = false;
    float a0 = 0.f, b0 = 0.f, c0v = 0.f, d0 = 0.f, a1 = 0.f, b1 = 0.f, c1v = 0.f, d1 = 0.f;
    int X = x_begin + g;
    int next_id = X < x_end ? idrow[X] : -1;
    for (; X < x_end; X += ng) {
        const int id = next_id;
        next_id = x_end - X > ng ? idrow[X + ng] : -1;
        const int64_t row = off + id;
        const int64_t key = id >= 0 && row >= p.lo && row < p.hi ? row - p.lo : -1;
        if (key != cur) {
            if (cur >= 0) {
                flush(p, cur, c0, acc0);
                if (two) flush(p, cur, c0 + 64, acc1);
            }
            cur = key;
            acc0 = acc1 = 0;
        }
        if (key < 0) continue;
        int x0, x1;
        float w1;
        taps(X, p.scale_w, p.w, x0, x1, w1);
        const bool right = w1 != 0.f;
        if (x0 != cx0 || (right && !have_right)) {
            const int64_t q0 = (int64_t)x0 * p.map.stride_w, q1 = (int64_t)x1 * p.map.stride_w;
            a0 = m0[r0 + q0];
            if (right) b0 = m0[r0 + q1];
            if (tall) {
                c0v = m0[r1 + q0];
                if (right) d0 = m0[r1 + q1];
            }
            if (two) {
                a1 = m1[r0 + q0];
                if (right) b1 = m1[r0 + q1];
                if (tall) {
                    c1v = m1[r1 + q0];
                    if (right) d1 = m1[r1 + q1];
                }
            }
            cx0 = x0;
            have_right = right;
        }
        const float w0 = 1.f - w1;
        acc0 += quantise(tap4(h0, h1, w0, w1, a0, b0, c0v, d0), s);
        if (two) acc1 += quantise(tap4(h0, h1, w0, w1, a1, b1, c1v, d1), s);
    }
    if (cur >= 0) {
        flush(p, cur, c0, acc0);
        if (two) flush(p, cur, c0 + 64, acc1);
    }
}

__global__ __launch_bounds__(TPB) void region_pool_finish_kernel(const PoolParams p)
{
    __shared__ uint32_t red[WAVES];
    const uint32_t mbits = block_max_bits(p, red);
    const int s = 156 - (int)(mbits >> 23);
    const int64_t i0 = ((int64_t)blockIdx.x * TPB + threadIdx.x) * 4;
    if (i0 >= p.n_sums) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k >= p.n_sums) break;
        const int a = p.area[p.lo + (int)(i0 + k) / p.C];
        if (a > 0) v[k] = (float)(ldexp((double)p.sums[i0 + k], -s) / (double)a);
    }
    if (p.out_wide && i0 + 4 <= p.n_sums) {
        *reinterpret_cast<float4*>(p.out + i0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int k = 0; k < 4 && i0 + k < p.n_sums; ++k) p.out[i0 + k] = v[k];
    }
}

// ---- host
int check_desc(const StegoRegionPoolDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->B < 1 || d->B > 65535 || d->H < 1 || d->W < 1 || (int64_t)d->H * d->W > (int64_t)INT32_MAX || d->h < 1 || d->w < 1 ||
        (int64_t)d->h * d->w > (int64_t)INT32_MAX)
        return STEGO_ERR_REGION_POOL_SIZE;
    if (d->C < 1 || d->C > STEGO_REGION_POOL_MAX_C) return STEGO_ERR_REGION_POOL_DIM;
    if (d->rows < 0 || d->rows * d->C > (int64_t)INT32_MAX) return STEGO_ERR_REGION_POOL_RANGE;
    return STEGO_OK;
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct Plan {
    int gl, seg, nseg, n_partial;
    int64_t n_map, pool_x;
    size_t partial, sums;
};

Plan plan(const StegoRegionPoolDesc* d)
{
    Plan pl{};
    pl.gl = 6;
    if (d->C <= 32)
        for (pl.gl = 0; (1 << pl.gl) < d->C; ++pl.gl) {}
    const int groups = 64 >> pl.gl;
    pl.seg = BASE_SEGMENT * (groups < MAX_SEGMENT_GROUPS ? groups : MAX_SEGMENT_GROUPS);
    pl.nseg = (int)ceil_div(d->W, pl.seg);
    pl.pool_x = ceil_div((int64_t)d->H * pl.nseg, WAVES);
    pl.n_map = (int64_t)d->B * d->C * d->h * d->w;
    const int64_t want = ceil_div(pl.n_map, (int64_t)TPB * RANGE_PER_THREAD);
    pl.n_partial = (int)(want < MAX_PARTIALS ? want : MAX_PARTIALS);
    WsLayout ws;
    pl.partial = ws.take((size_t)MAX_PARTIALS * sizeof(uint32_t), 16);
    pl.sums = ws.take(0, 16);
    return pl;
}

size_t bytes_for(const Plan& pl, int64_t rows, int C) { return WsLayout::round_up(pl.sums + (size_t)rows * C * sizeof(int64_t), 16); }

}  // namespace

extern "C" size_t stego_region_pool_workspace_bytes(const StegoRegionPoolDesc* desc)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    return bytes_for(plan(desc), desc->rows, desc->C);
}

extern "C" int stego_region_pool_plan(const StegoRegionPoolDesc* desc, int32_t* segment, int32_t* channel_block, size_t* lds_bytes,
                                      int64_t* workgroups)
{
    const int rc = check_desc(desc);
    size_t lds[STEGO_REGION_POOL_LAUNCHES] = {RED_LDS, RED_LDS, RED_LDS};
    int64_t wgs[STEGO_REGION_POOL_LAUNCHES] = {};
    if (segment) *segment = 0;
    if (channel_block) *channel_block = 0;
    if (rc == STEGO_OK) {
        const Plan pl = plan(desc);
        if (segment) *segment = pl.seg;
        if (channel_block) *channel_block = CB;
        wgs[0] = pl.n_partial;
        wgs[1] = pl.pool_x * ceil_div(desc->C, CB) * desc->B;
        wgs[2] = ceil_div(desc->rows * desc->C, 4 * TPB);
    }
    return report_plan(rc, STEGO_REGION_POOL_LAUNCHES, lds, wgs, lds_bytes, workgroups);
}

extern "C" int stego_region_pool(const StegoRegionPoolDesc* desc, const StegoMap* map, const int32_t* ids, const int64_t* row_offset,
                                 const int32_t* area, int64_t capacity, int64_t lo, int64_t hi, float* out, void* workspace,
                                 size_t workspace_bytes, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (lo < 0 || hi < lo || hi > capacity || (hi - lo) * desc->C > (int64_t)INT32_MAX) return STEGO_ERR_REGION_POOL_RANGE;
    if (hi == lo) return STEGO_OK;
    if (!map || !map->data || !ids || !row_offset || !area || !out || !workspace) return STEGO_ERR_NULL;
    const Plan pl = plan(desc);
    if (workspace_bytes < bytes_for(pl, hi - lo, desc->C)) return STEGO_ERR_WORKSPACE;
    if (!aligned(map->data, 4) || !aligned(ids, 4) || !aligned(row_offset, 8) || !aligned(area, 4) || !aligned(out, 4) ||
        !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;
    PoolParams p{};
    p.map = *map;
    p.ids = ids;
    p.row_offset = row_offset;
    p.area = area;
    p.out = out;
    p.partial = at<uint32_t>(workspace, pl.partial);
    p.sums = at<int64_t>(workspace, pl.sums);
    p.hw = (int64_t)desc->H * desc->W;
    p.lo = lo;
    p.hi = hi;
    p.n_sums = (hi - lo) * desc->C;
    p.n_map = pl.n_map;
    // the range walks the map with its smaller-stride index innermost: channels of a channels-last map, else columns
    const int64_t sc = map->stride_c < 0 ? -map->stride_c : map->stride_c, sw = map->stride_w < 0 ? -map->stride_w : map->stride_w;
    p.s0 = map->stride_n;
    if (sc < sw) {
        p.d1 = desc->h, p.d2 = desc->w, p.d3 = desc->C;
        p.s1 = map->stride_h, p.s2 = map->stride_w, p.s3 = map->stride_c;
    } else {
        p.d1 = desc->C, p.d2 = desc->h, p.d3 = desc->w;
        p.s1 = map->stride_c, p.s2 = map->stride_h, p.s3 = map->stride_w;
    }
    p.scale_h = (float)desc->h / (float)desc->H;
    p.scale_w = (float)desc->w / (float)desc->W;
    p.C = desc->C;
    p.h = desc->h;
    p.w = desc->w;
    p.H = desc->H;
    p.W = desc->W;
    p.n_partial = pl.n_partial;
    p.gl = pl.gl;
    p.seg = pl.seg;
    p.nseg = pl.nseg;
    p.out_wide = aligned(out, 16);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_first<region_pool_range_kernel>(dim3((unsigned)pl.n_partial), TPB, 0, s, p);
    if (e == hipSuccess)
        e = launch_next<region_pool_kernel>(dim3((unsigned)pl.pool_x, (unsigned)ceil_div(desc->C, CB), (unsigned)desc->B), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<region_pool_finish_kernel>(dim3((unsigned)ceil_div(p.n_sums, 4 * TPB)), TPB, 0, s, p);
    return hip_rc(e);
}
