// Segments as objects (include/stego_regions.h): connected regions of a label map, their table, the cleanup of small regions.
//
//   tile     a workgroup per 32 x 32 tile, four pixels a thread.  Labels and parents sit in LDS; a pixel is united with its left and upper
//            neighbours (and the two upper diagonals at connectivity 8) of the same label.  The larger root is hung below the smaller with
//            atomicMin, and inside a tile the local order (ly, lx) is the raster order of the image, so a root is its piece's first pixel.
//   seam     a thread per pixel on the far side of a tile border: the same union on the int32 root array of the image.
//   flatten  root[p] = find(p); the roots of every 2048 pixels are counted.   scan: the chunks' exclusive sums, a workgroup per image.
//   number   the roots get their ids (a thread takes 8 consecutive pixels, so the ranks inside a chunk are in raster order); spread hands
//            them to the other pixels.
//   table    a lane per pixel: the lanes of a wave that hold a run of one id along a row are found with one ballot, and the run's first
//            lane adds area, box and coordinate sums in closed form.  `first` is an atomicMin; y0 and the label follow from it per row.
//   votes / relabel   a thread per pixel; only the pixels of the small regions of the slab do anything.
//
// Termination: root[p] <= p holds from the start and atomicMin only lowers a word, so find() walks strictly decreasing indices; unite()
// goes round again only when atomicMin answered with a parent below the root it meant to hang.  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/stego_regions.h"
#include "host_util.h"
#include "ws_layout.h"

using namespace stego;

namespace {

constexpr int TPB = 256;
constexpr int T = STEGO_REGIONS_TILE;
constexpr int TT = T * T;
constexpr int PPT = TT / TPB;                 // pixels of a thread in the tile launch
constexpr int CH = STEGO_REGIONS_CHUNK;
constexpr int CPT = CH / TPB;                 // pixels of a thread in the chunked launches
constexpr size_t TILE_LDS = TT * (sizeof(int64_t) + sizeof(int));
constexpr size_t RED_LDS = TPB * sizeof(int);

struct LabelParams {
    const void* labels;
    int32_t* ids;
    int32_t* n_regions;
    int32_t* root;
    int32_t* partial;                         // [B][chunks]: roots of a chunk, then their exclusive sums
    int64_t hw, seam_v, seam_h;
    int H, W, ntx, nty, chunks, conn8, dt;
};

struct TableParams {
    const void* labels;
    const int32_t* ids;
    const int64_t* row_offset;
    const int32_t* small_rank;
    const int32_t* first;
    const int32_t* votes_in;
    int32_t* cols32;
    int64_t* cols64;
    int32_t* votes;
    int32_t* changed;
    void* labels_out;
    int64_t hw, cap, lo, hi;
    int H, W, B, n_labels, dt;
};

__device__ __forceinline__ int64_t load_label(const void* p, int dt, int64_t i)
{
    if (dt == STEGO_REGIONS_I64) return static_cast<const int64_t*>(p)[i];
    if (dt == STEGO_REGIONS_I32) return (int64_t) static_cast<const int32_t*>(p)[i];
    return (int64_t) static_cast<const uint8_t*>(p)[i];
}

__device__ __forceinline__ void store_label(void* p, int dt, int64_t i, int v)
{
    if (dt == STEGO_REGIONS_I64) static_cast<int64_t*>(p)[i] = (int64_t)v;
    else if (dt == STEGO_REGIONS_I32) static_cast<int32_t*>(p)[i] = v;
    else static_cast<uint8_t*>(p)[i] = (uint8_t)v;
}

// ---- union-find: SCOPE is the memory scope of the parent array (LDS: workgroup, the image's root array: agent)
template <int SCOPE>
__device__ __forceinline__ int find_root(int* par, int i)
{
    int p;
    while ((p = __hip_atomic_load(&par[i], __ATOMIC_RELAXED, SCOPE)) != i) i = p;        // p < i: strictly down
    return i;
}

template <int SCOPE>
__device__ __forceinline__ void unite(int* par, int a, int b)
{
    for (;;) {
        a = find_root<SCOPE>(par, a);
        b = find_root<SCOPE>(par, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = __hip_atomic_fetch_min(&par[a], b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;                 // a was a root and hangs below b now
        a = old;                              // old < a: someone hung a first; its former parent and b are still to be joined
    }
}

__global__ __launch_bounds__(TPB) void regions_tile_kernel(const LabelParams p)
{
    __shared__ int64_t lab[TT];
    __shared__ int par[TT];
    const int t = threadIdx.x;
    const int ty = blockIdx.x / p.ntx, tx = blockIdx.x - ty * p.ntx;
    const int64_t base = (int64_t)blockIdx.y * p.hw;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int li = t + k * TPB, y = ty * T + (li >> 5), x = tx * T + (li & 31);
        const bool in = y < p.H && x < p.W;
        const int64_t L = in ? load_label(p.labels, p.dt, base + (int64_t)y * p.W + x) : -1;
        lab[li] = L < 0 ? -1 : L;
        par[li] = li;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int li = t + k * TPB, ly = li >> 5, lx = li & 31;
        const int64_t L = lab[li];
        if (L < 0) continue;
        if (lx > 0 && lab[li - 1] == L) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, li, li - 1);
        if (ly > 0 && lab[li - T] == L) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, li, li - T);
        if (p.conn8 && ly > 0) {
            if (lx > 0 && lab[li - T - 1] == L) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, li, li - T - 1);
            if (lx < T - 1 && lab[li - T + 1] == L) unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, li, li - T + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int li = t + k * TPB, y = ty * T + (li >> 5), x = tx * T + (li & 31);
        if (y < p.H && x < p.W) {
            int r = -1;
            if (lab[li] >= 0) {
                const int l = find_root<__HIP_MEMORY_SCOPE_WORKGROUP>(par, li);
                r = (ty * T + (l >> 5)) * p.W + tx * T + (l & 31);
            }
            p.root[base + (int64_t)y * p.W + x] = r;
        }
    }
}

__device__ __forceinline__ void seam_pair(const LabelParams& p, int64_t base, int* par, int y, int x, int64_t L, int qy, int qx)
{
    if (qy < 0 || qy >= p.H || qx < 0 || qx >= p.W) return;
    if (load_label(p.labels, p.dt, base + (int64_t)qy * p.W + qx) != L) return;
    unite<__HIP_MEMORY_SCOPE_AGENT>(par, y * p.W + x, qy * p.W + qx);
}

__global__ __launch_bounds__(TPB) void regions_seam_kernel(const LabelParams p)
{
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= p.seam_v + p.seam_h) return;
    const int64_t base = (int64_t)blockIdx.y * p.hw;
    int* par = p.root + base;
    if (i < p.seam_v) {                       // the first column of a tile against the last column of the tile to its left
        const int s = (int)(i / p.H), y = (int)(i - (int64_t)s * p.H), x = (s + 1) * T;
        const int64_t L = load_label(p.labels, p.dt, base + (int64_t)y * p.W + x);
        if (L < 0) return;
        seam_pair(p, base, par, y, x, L, y, x - 1);
        if (p.conn8) {
            seam_pair(p, base, par, y, x, L, y - 1, x - 1);
            seam_pair(p, base, par, y, x, L, y + 1, x - 1);
        }
    } else {                                  // the first row of a tile against the last row of the tile above
        const int64_t j = i - p.seam_v;
        const int s = (int)(j / p.W), x = (int)(j - (int64_t)s * p.W), y = (s + 1) * T;
        const int64_t L = load_label(p.labels, p.dt, base + (int64_t)y * p.W + x);
        if (L < 0) return;
        seam_pair(p, base, par, y, x, L, y - 1, x);
        if (p.conn8) {
            seam_pair(p, base, par, y, x, L, y - 1, x - 1);
            seam_pair(p, base, par, y, x, L, y - 1, x + 1);
        }
    }
}

// the sum of one int per thread over the workgroup, valid in every thread
__device__ __forceinline__ int block_count(int v, int* red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int m = TPB / 2; m > 0; m >>= 1) {
        if (t < m) red[t] += red[t + m];
        __syncthreads();
    }
    return red[0];
}

// the inclusive sums of one int per thread in thread order; red[TPB - 1] is the total
__device__ __forceinline__ int block_scan(int v, int* red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int d = 1; d < TPB; d <<= 1) {
        const int u = t >= d ? red[t - d] : 0;
        __syncthreads();
        red[t] += u;
        __syncthreads();
    }
    return red[t];
}

__global__ __launch_bounds__(TPB) void regions_flatten_kernel(const LabelParams p)
{
    __shared__ int red[TPB];
    const int t = threadIdx.x;
    int* par = p.root + (int64_t)blockIdx.y * p.hw;
    int roots = 0;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int64_t px = (int64_t)blockIdx.x * CH + k * TPB + t;
        if (px < p.hw) {
            const int i = (int)px;
            if (__hip_atomic_load(&par[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) {
                const int r = find_root<__HIP_MEMORY_SCOPE_AGENT>(par, i);
                __hip_atomic_store(&par[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // a root of the same piece, <= i
                roots += r == i;
            }
        }
    }
    roots = block_count(roots, red);
    if (t == 0) p.partial[(int64_t)blockIdx.y * p.chunks + blockIdx.x] = roots;
}

__global__ __launch_bounds__(TPB) void regions_scan_kernel(const LabelParams p)
{
    __shared__ int red[TPB];
    const int t = threadIdx.x;
    int32_t* part = p.partial + (int64_t)blockIdx.x * p.chunks;
    int running = 0;
    for (int c0 = 0; c0 < p.chunks; c0 += TPB) {
        const int c = c0 + t;
        const int v = c < p.chunks ? part[c] : 0;
        const int incl = block_scan(v, red);
        if (c < p.chunks) part[c] = running + incl - v;
        running += red[TPB - 1];
        __syncthreads();
    }
    if (t == 0) p.n_regions[blockIdx.x] = running;
}

__global__ __launch_bounds__(TPB) void regions_number_kernel(const LabelParams p)
{
    __shared__ int red[TPB];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.y * p.hw;
    const int64_t px0 = (int64_t)blockIdx.x * CH + t * CPT;
    int r[CPT], mine = 0;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int64_t px = px0 + k;
        r[k] = px < p.hw ? p.root[base + px] : -1;
        mine += r[k] == (int)px && px < p.hw;
    }
    int rank = p.partial[(int64_t)blockIdx.y * p.chunks + blockIdx.x] + block_scan(mine, red) - mine;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int64_t px = px0 + k;
        if (px < p.hw && r[k] == (int)px) p.ids[base + px] = rank++;
    }
}

__global__ __launch_bounds__(TPB) void regions_spread_kernel(const LabelParams p)
{
    const int64_t base = (int64_t)blockIdx.y * p.hw;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int64_t px = (int64_t)blockIdx.x * CH + k * TPB + threadIdx.x;
        if (px < p.hw) {
            const int r = p.root[base + px];
            if (r < 0) p.ids[base + px] = -1;
            else if (r != (int)px) p.ids[base + px] = p.ids[base + r];       // the roots' ids are the last launch's
        }
    }
}

// ---- the table
__global__ __launch_bounds__(TPB) void regions_table_reset_kernel(const TableParams p)
{
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= p.cap) return;
    p.cols32[STEGO_REGIONS_AREA * p.cap + r] = 0;
    p.cols32[STEGO_REGIONS_Y0 * p.cap + r] = 0;
    p.cols32[STEGO_REGIONS_X0 * p.cap + r] = INT_MAX;
    p.cols32[STEGO_REGIONS_Y1 * p.cap + r] = -1;
    p.cols32[STEGO_REGIONS_X1 * p.cap + r] = -1;
    p.cols32[STEGO_REGIONS_FIRST * p.cap + r] = INT_MAX;
    p.cols64[STEGO_REGIONS_LABEL * p.cap + r] = 0;
    p.cols64[STEGO_REGIONS_SUM_Y * p.cap + r] = 0;
    p.cols64[STEGO_REGIONS_SUM_X * p.cap + r] = 0;
}

__global__ __launch_bounds__(TPB) void regions_table_add_kernel(const TableParams p)
{
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.y * p.hw;
    const int64_t off = p.row_offset[blockIdx.y];
#pragma unroll 2
    for (int k = 0; k < CPT; ++k) {
        const int64_t px = (int64_t)blockIdx.x * CH + k * TPB + threadIdx.x;       // a wave: 64 consecutive pixels
        const bool in = px < p.hw;
        const int id = in ? p.ids[base + px] : -1;
        const int y = in ? (int)(px / p.W) : -1, x = in ? (int)(px - (int64_t)y * p.W) : 0;
        const int pid = __shfl_up(id, 1), py = __shfl_up(y, 1);
        const bool brk = lane == 0 || pid != id || py != y;                         // a run of one id in one row starts here
        const unsigned long long starts = __ballot(brk);
        if (brk && id >= 0) {
            const unsigned long long rest = lane == 63 ? 0ull : starts >> (lane + 1);
            const int len = rest ? __ffsll((long long)rest) : 64 - lane;            // up to the next start, or the end of the wave
            const int64_t row = off + id;
            if (row < p.cap) {
                atomicAdd(&p.cols32[STEGO_REGIONS_AREA * p.cap + row], len);
                atomicMin(&p.cols32[STEGO_REGIONS_X0 * p.cap + row], x);
                atomicMax(&p.cols32[STEGO_REGIONS_X1 * p.cap + row], x + len - 1);
                atomicMax(&p.cols32[STEGO_REGIONS_Y1 * p.cap + row], y);
                atomicMin(&p.cols32[STEGO_REGIONS_FIRST * p.cap + row], (int)px);
                atomicAdd(reinterpret_cast<unsigned long long*>(&p.cols64[STEGO_REGIONS_SUM_Y * p.cap + row]),
                          (unsigned long long)y * (unsigned long long)len);
                atomicAdd(reinterpret_cast<unsigned long long*>(&p.cols64[STEGO_REGIONS_SUM_X * p.cap + row]),
                          (unsigned long long)x * (unsigned long long)len + (unsigned long long)len * (unsigned long long)(len - 1) / 2ull);
            }
        }
    }
}

// per row: the image that owns it (the last one whose first row is not beyond it), then y0 and the label from the first pixel
__global__ __launch_bounds__(TPB) void regions_table_finish_kernel(const TableParams p)
{
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= p.cap) return;
    const int first = p.cols32[STEGO_REGIONS_FIRST * p.cap + r];
    if (first == INT_MAX) return;             // a row no pixel belongs to
    int lo = 0, hi = p.B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.row_offset[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    p.cols32[STEGO_REGIONS_Y0 * p.cap + r] = first / p.W;
    p.cols64[STEGO_REGIONS_LABEL * p.cap + r] = load_label(p.labels, p.dt, (int64_t)lo * p.hw + first);
}

// ---- the cleanup
__global__ __launch_bounds__(TPB) void regions_votes_reset_kernel(const TableParams p)
{
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < (p.hi - p.lo) * p.n_labels) p.votes[i] = 0;
}

// the rank among the small regions of the region of pixel px, or -1: not small, no region, or a row beyond the table
__device__ __forceinline__ int small_rank_of(const TableParams& p, int64_t base, int64_t off, int64_t px)
{
    const int id = p.ids[base + px];
    if (id < 0) return -1;
    const int64_t row = off + id;
    return row < p.cap ? p.small_rank[row] : -1;
}

__device__ __forceinline__ void vote(const TableParams& p, int64_t base, int64_t off, int64_t q, int32_t* mine)
{
    const int id = p.ids[base + q];
    if (id < 0) return;
    const int64_t row = off + id;
    if (row >= p.cap || p.small_rank[row] >= 0) return;                  // only regions that are not small vote
    const int64_t c = load_label(p.labels, p.dt, base + q);
    if (c >= 0 && c < p.n_labels) atomicAdd(&mine[c], 1);
}

__global__ __launch_bounds__(TPB) void regions_votes_kernel(const TableParams p)
{
    const int64_t base = (int64_t)blockIdx.y * p.hw;
    const int64_t off = p.row_offset[blockIdx.y];
#pragma unroll 2
    for (int k = 0; k < CPT; ++k) {
        const int64_t px = (int64_t)blockIdx.x * CH + k * TPB + threadIdx.x;
        if (px >= p.hw) continue;
        const int64_t rk = small_rank_of(p, base, off, px);
        if (rk < p.lo || rk >= p.hi) continue;
        int32_t* mine = p.votes + (rk - p.lo) * p.n_labels;
        const int y = (int)(px / p.W), x = (int)(px - (int64_t)y * p.W);
        if (y > 0) vote(p, base, off, px - p.W, mine);
        if (x > 0) vote(p, base, off, px - 1, mine);
        if (x < p.W - 1) vote(p, base, off, px + 1, mine);
        if (y < p.H - 1) vote(p, base, off, px + p.W, mine);
    }
}

__global__ __launch_bounds__(TPB) void regions_relabel_kernel(const TableParams p)
{
    const int64_t base = (int64_t)blockIdx.y * p.hw;
    const int64_t off = p.row_offset[blockIdx.y];
#pragma unroll 2
    for (int k = 0; k < CPT; ++k) {
        const int64_t px = (int64_t)blockIdx.x * CH + k * TPB + threadIdx.x;
        if (px >= p.hw) continue;
        const int64_t rk = small_rank_of(p, base, off, px);
        if (rk < p.lo || rk >= p.hi) continue;
        const int32_t* row = p.votes_in + (rk - p.lo) * p.n_labels;
        int best = 0, cls = -1;
        for (int c = 0; c < p.n_labels; ++c) {                            // the first maximum
            const int v = row[c];
            if (v > best) {
                best = v;
                cls = c;
            }
        }
        if (cls < 0 || (int64_t)cls == load_label(p.labels, p.dt, base + px)) continue;
        store_label(p.labels_out, p.dt, base + px, cls);
        if (p.first[off + p.ids[base + px]] == (int)px) atomicAdd(p.changed, 1);       // once per region
    }
}

// ---- host
int check_desc(const StegoRegionsDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->B < 1 || d->B > 65535 || d->H < 1 || d->W < 1 || (int64_t)d->H * d->W > (int64_t)INT32_MAX) return STEGO_ERR_REGIONS_SIZE;
    if (d->connectivity != 4 && d->connectivity != 8) return STEGO_ERR_REGIONS_CONN;
    if (d->label_dtype != STEGO_REGIONS_I64 && d->label_dtype != STEGO_REGIONS_I32 && d->label_dtype != STEGO_REGIONS_U8)
        return STEGO_ERR_REGIONS_DTYPE;
    return STEGO_OK;
}

size_t label_align(int dt) { return dt == STEGO_REGIONS_I64 ? 8 : dt == STEGO_REGIONS_I32 ? 4 : 1; }

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct Plan {
    int64_t hw, seam_v, seam_h;
    int ntx, nty, chunks;
    size_t partial, total;
};

Plan plan(const StegoRegionsDesc* d)
{
    Plan pl{};
    pl.hw = (int64_t)d->H * d->W;
    pl.ntx = (int)ceil_div(d->W, T);
    pl.nty = (int)ceil_div(d->H, T);
    pl.seam_v = (int64_t)(pl.ntx - 1) * d->H;
    pl.seam_h = (int64_t)(pl.nty - 1) * d->W;
    pl.chunks = (int)ceil_div(pl.hw, CH);
    WsLayout ws;
    pl.partial = ws.take((size_t)d->B * pl.chunks * sizeof(int32_t), 16);
    pl.total = ws.total(16);
    return pl;
}

// the checks stego_regions_table, _votes and _relabel share
int check_table_call(const StegoRegionsDesc* d, const void* labels, const int32_t* ids, const int64_t* row_offset, int64_t capacity)
{
    const int rc = check_desc(d);
    if (rc != STEGO_OK) return rc;
    if (capacity < 0) return STEGO_ERR_REGIONS_RANGE;
    if (!labels || !ids || !row_offset) return STEGO_ERR_NULL;
    if (!aligned(labels, label_align(d->label_dtype)) || !aligned(ids, 4) || !aligned(row_offset, 8)) return STEGO_ERR_ALIGN;
    return STEGO_OK;
}

int check_slab(int64_t lo, int64_t hi, int32_t n_labels)
{
    if (n_labels < 1 || n_labels > STEGO_REGIONS_MAX_LABELS) return STEGO_ERR_REGIONS_LABELS;
    if (lo < 0 || hi < lo || (hi - lo) * n_labels > (int64_t)INT32_MAX) return STEGO_ERR_REGIONS_RANGE;
    return STEGO_OK;
}

TableParams table_params(const StegoRegionsDesc* d, const void* labels, const int32_t* ids, const int64_t* row_offset, int64_t capacity)
{
    TableParams p{};
    p.labels = labels;
    p.ids = ids;
    p.row_offset = row_offset;
    p.hw = (int64_t)d->H * d->W;
    p.cap = capacity;
    p.H = d->H;
    p.W = d->W;
    p.B = d->B;
    p.dt = d->label_dtype;
    return p;
}

dim3 pixel_grid(const StegoRegionsDesc* d) { return dim3((unsigned)ceil_div((int64_t)d->H * d->W, CH), (unsigned)d->B); }

}  // namespace

extern "C" size_t stego_regions_workspace_bytes(const StegoRegionsDesc* desc)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    return plan(desc).total;
}

extern "C" int stego_regions_plan(const StegoRegionsDesc* desc, int32_t* tile, size_t* lds_bytes, int64_t* workgroups)
{
    const int rc = check_desc(desc);
    if (tile) *tile = rc == STEGO_OK ? T : 0;
    size_t lds[STEGO_REGIONS_LAUNCHES] = {TILE_LDS, 0, RED_LDS, RED_LDS, RED_LDS, 0};
    int64_t wgs[STEGO_REGIONS_LAUNCHES] = {};
    if (rc == STEGO_OK) {
        const Plan pl = plan(desc);
        const int64_t px = (int64_t)pl.chunks * desc->B;
        wgs[0] = (int64_t)pl.ntx * pl.nty * desc->B;
        wgs[1] = ceil_div(pl.seam_v + pl.seam_h, TPB) * desc->B;
        wgs[2] = px;
        wgs[3] = desc->B;
        wgs[4] = px;
        wgs[5] = px;
    }
    return report_plan(rc, STEGO_REGIONS_LAUNCHES, lds, wgs, lds_bytes, workgroups);
}

extern "C" int stego_regions_label(const StegoRegionsDesc* desc, const void* labels, int32_t* ids, int32_t* n_regions, int32_t* root,
                                   void* workspace, size_t workspace_bytes, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!labels || !ids || !n_regions || !root || !workspace) return STEGO_ERR_NULL;
    const Plan pl = plan(desc);
    if (workspace_bytes < pl.total) return STEGO_ERR_WORKSPACE;
    if (!aligned(labels, label_align(desc->label_dtype)) || !aligned(ids, 4) || !aligned(n_regions, 4) || !aligned(root, 4) ||
        !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;
    LabelParams p{};
    p.labels = labels;
    p.ids = ids;
    p.n_regions = n_regions;
    p.root = root;
    p.partial = at<int32_t>(workspace, pl.partial);
    p.hw = pl.hw;
    p.seam_v = pl.seam_v;
    p.seam_h = pl.seam_h;
    p.H = desc->H;
    p.W = desc->W;
    p.ntx = pl.ntx;
    p.nty = pl.nty;
    p.chunks = pl.chunks;
    p.conn8 = desc->connectivity == 8;
    p.dt = desc->label_dtype;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned B = (unsigned)desc->B;
    const dim3 px((unsigned)pl.chunks, B);
    hipError_t e = launch_first<regions_tile_kernel>(dim3((unsigned)(pl.ntx * pl.nty), B), TPB, 0, s, p);
    const int64_t seams = pl.seam_v + pl.seam_h;
    if (e == hipSuccess && seams > 0) e = launch_next<regions_seam_kernel>(dim3((unsigned)ceil_div(seams, TPB), B), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<regions_flatten_kernel>(px, TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<regions_scan_kernel>(dim3(B), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<regions_number_kernel>(px, TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<regions_spread_kernel>(px, TPB, 0, s, p);
    return hip_rc(e);
}

extern "C" int stego_regions_table(const StegoRegionsDesc* desc, const void* labels, const int32_t* ids, const int64_t* row_offset,
                                   int64_t capacity, int32_t* cols32, int64_t* cols64, stego_stream_t stream)
{
    const int rc = check_table_call(desc, labels, ids, row_offset, capacity);
    if (rc != STEGO_OK) return rc;
    if (ceil_div(capacity, TPB) > (int64_t)INT32_MAX) return STEGO_ERR_REGIONS_RANGE;
    if (capacity == 0) return STEGO_OK;
    if (!cols32 || !cols64) return STEGO_ERR_NULL;
    if (!aligned(cols32, 4) || !aligned(cols64, 8)) return STEGO_ERR_ALIGN;
    TableParams p = table_params(desc, labels, ids, row_offset, capacity);
    p.cols32 = cols32;
    p.cols64 = cols64;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 rows((unsigned)ceil_div(capacity, TPB));
    hipError_t e = launch_first<regions_table_reset_kernel>(rows, TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<regions_table_add_kernel>(pixel_grid(desc), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<regions_table_finish_kernel>(rows, TPB, 0, s, p);
    return hip_rc(e);
}

extern "C" int stego_regions_votes(const StegoRegionsDesc* desc, const void* labels, const int32_t* ids, const int64_t* row_offset,
                                   int64_t capacity, const int32_t* small_rank, int64_t lo, int64_t hi, int32_t n_labels, int32_t* votes,
                                   stego_stream_t stream)
{
    int rc = check_table_call(desc, labels, ids, row_offset, capacity);
    if (rc == STEGO_OK) rc = check_slab(lo, hi, n_labels);
    if (rc != STEGO_OK) return rc;
    if (hi == lo || capacity == 0) return STEGO_OK;
    if (!small_rank || !votes) return STEGO_ERR_NULL;
    if (!aligned(small_rank, 4) || !aligned(votes, 4)) return STEGO_ERR_ALIGN;
    TableParams p = table_params(desc, labels, ids, row_offset, capacity);
    p.small_rank = small_rank;
    p.votes = votes;
    p.lo = lo;
    p.hi = hi;
    p.n_labels = n_labels;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_first<regions_votes_reset_kernel>(dim3((unsigned)ceil_div((hi - lo) * n_labels, TPB)), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<regions_votes_kernel>(pixel_grid(desc), TPB, 0, s, p);
    return hip_rc(e);
}

extern "C" int stego_regions_relabel(const StegoRegionsDesc* desc, const void* labels_in, void* labels_out, const int32_t* ids,
                                     const int64_t* row_offset, int64_t capacity, const int32_t* small_rank, const int32_t* first, int64_t lo,
                                     int64_t hi, int32_t n_labels, const int32_t* votes, int32_t* changed, stego_stream_t stream)
{
    int rc = check_table_call(desc, labels_in, ids, row_offset, capacity);
    if (rc == STEGO_OK) rc = check_slab(lo, hi, n_labels);
    if (rc != STEGO_OK) return rc;
    if (hi == lo || capacity == 0) return STEGO_OK;
    if (!labels_out || !small_rank || !first || !votes || !changed) return STEGO_ERR_NULL;
    if (!aligned(labels_out, label_align(desc->label_dtype)) || !aligned(small_rank, 4) || !aligned(first, 4) || !aligned(votes, 4) ||
        !aligned(changed, 4))
        return STEGO_ERR_ALIGN;
    TableParams p = table_params(desc, labels_in, ids, row_offset, capacity);
    p.labels_out = labels_out;
    p.small_rank = small_rank;
    p.first = first;
    p.votes_in = votes;
    p.changed = changed;
    p.lo = lo;
    p.hi = hi;
    p.n_labels = n_labels;
    return hip_rc(launch_first<regions_relabel_kernel>(pixel_grid(desc), TPB, 0, static_cast<hipStream_t>(stream), p));
}
