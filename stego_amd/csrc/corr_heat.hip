// Query-point correspondence heatmaps (include/stego_heat.h): bilinear sampling of the source map at the query points, L2
// normalisation of both sides, the channel contraction against every cell of the target map, the centring over a query's whole
// map, the clamp and the align_corners=True upsample, in one call of two launches.
//
// Launch 1, heat_low_kernel.  Grid: (chunks of 128 target cells, tiles of 128 queries, B); 256 threads (4 waves) own the 128 x 128
// tile (query, cell) of one image pair:
//   1. thread t < 128 prepares query t of the tile (the bilinear taps of the source map: element offset of the north-west tap and
//      the steps to its neighbours, 64-bit; four weights), thread 128 + t the element offset of cell t of the chunk;
//   2. per 64-channel chunk the four waves stage both operands in LDS as fp32 images [128][LDA] (corr_tile.h's mma_chunk_f32;
//      channels beyond C are zero): the queries with 64 lanes = 64 channels of one point, the cells either the same way (a map
//      whose channel stride is the smallest: channels-last) or with 64 lanes = 64 cells of one channel (NCHW), so that both
//      layouts are read in whole rows; every thread adds the squares of one operand row to its squared norm; each wave runs its
//      64 x 64 quadrant on v_mfma_f32_32x32x2_f32 (exact fp32 products);
//   3. epilogue: the operand stages are dead, the tile takes their place in LDS, scaled by the two inverse norms.  It is written
//      to the workspace in rows of 512 bytes, and thread t < 128 walks row t in cell order: the float64 sum of the chunk and its
//      first maximum.  One partial per (query, chunk): nothing is accumulated across workgroups.
// Launch 2, heat_write_kernel.  Grid: (blocks of output rows, N, B); every wave adds the query's partial sums with one fixed
// butterfly (bitwise repeatable), the workgroup stages the source rows its output rows read - centred and clamped - in LDS and
// writes the interpolated rows with 16-byte non-temporal stores (4-byte stores when W is no multiple of 4).  The first block of a
// query also reduces the partial maxima to `peak` / `best`.  The number of output rows per workgroup comes from the host plan: as
// many as keep about eight workgroups per compute unit in flight, at least one full pass of the workgroup, at most what the LDS
// holds of source rows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/stego_heat.h"
#include "addon_device.h"
#include "corr_tile.h"
#include "host_util.h"

namespace {

using namespace stego;

constexpr int CELLS = TP;                           // target cells per chunk
constexpr int OUT_ROWS_MAX = 16;                    // output rows per workgroup of the second launch, at most
constexpr int WG_TARGET = 2048;                     // workgroups the second launch aims for (8 per compute unit)
constexpr int LOW_LDS_FLOATS = 16384;               // second launch: source rows staged per workgroup, at most (64 KB)

// LDS carve of the first launch (bytes)
constexpr int SH_TAPO = 0;                          // int64 tapo[128][3]: offset of the north-west tap, step to east, step to south
constexpr int SH_TAPW = SH_TAPO + TP * 24;          // float4 tapw[128]: nw, ne, sw, se
constexpr int SH_CELL = SH_TAPW + TP * 16;          // int64 cello[128]: element offset of the cell in the target image
constexpr int SH_INV = SH_CELL + TP * 8;            // float inv[256]: 1 / max(||.||, 1e-12), queries then cells
constexpr int SH_BIG = SH_INV + 2 * TP * 4;         // two operand stages, then the result tile [128][LDT]
constexpr int SH_STAGES = 2 * FEAT_SIDE_F32;
static_assert(SH_BIG % 16 == 0, "operand stages are read with ds_read_b128");
static_assert(TP * LDT * 4 <= SH_STAGES, "the result tile aliases the operand stages");
constexpr size_t LOW_LDS_BYTES = SH_BIG + SH_STAGES;
static_assert(2 * LOW_LDS_BYTES <= 160 * 1024, "two workgroups per CU");

struct LowParams {
    StegoMap src, tgt;
    const int64_t* index_t;
    const float* points;
    double* psum;
    float* low;
    float* pmax;
    int32_t* pidx;
    int32_t B, C, hs, ws, w, hw, N, NCH, NKC, cell_fast;
};

struct WriteParams {
    const double* psum;
    const float* low;
    const float* pmax;
    const int32_t* pidx;
    float* heat;
    float* peak;
    float* best;
    float sy, sx;
    int32_t h, w, hw, N, NCH, H, W, RB, flags, cap_rows;
};

__global__ __launch_bounds__(NTHREADS) void heat_low_kernel(LowParams p)
{
    extern __shared__ float4 smem4[];
    unsigned char* const smem = reinterpret_cast<unsigned char*>(smem4);
    long long* const tapo = reinterpret_cast<long long*>(smem + SH_TAPO);
    float4* const tapw = reinterpret_cast<float4*>(smem + SH_TAPW);
    long long* const cello = reinterpret_cast<long long*>(smem + SH_CELL);
    float* const inv = reinterpret_cast<float*>(smem + SH_INV);
    float* const As = reinterpret_cast<float*>(smem + SH_BIG);
    float* const Bs = As + TP * LDA;
    float* const T = reinterpret_cast<float*>(smem + SH_BIG);

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t img_s = blockIdx.z;
    int64_t img_t = p.index_t ? p.index_t[img_s] : img_s;
    img_t = img_t < 0 ? 0 : (img_t > p.B - 1 ? p.B - 1 : img_t);         // memory safety only
    const int q0 = blockIdx.y * TP, c0 = blockIdx.x * CELLS;
    const int nq = min(TP, p.N - q0), nc = min(CELLS, p.hw - c0);        // both >= 1 by the grid

    // 1. this thread's query or cell
    if (tid < TP) {
        const bool valid = tid < nq;
        float x = 0.f, y = 0.f;
        if (valid) {
            const float* c = p.points + (img_s * p.N + q0 + tid) * 2;
            x = c[0];
            y = c[1];
        }
        const Taps f = bilinear_taps(x, y, p.hs, p.ws);
        tapo[tid * 3 + 0] = (long long)f.y0 * p.src.stride_h + (long long)f.x0 * p.src.stride_w;
        tapo[tid * 3 + 1] = (long long)(f.x1 - f.x0) * p.src.stride_w;
        tapo[tid * 3 + 2] = (long long)(f.y1 - f.y0) * p.src.stride_h;
        tapw[tid] = make_float4(f.wx0 * f.wy0, f.wx1 * f.wy0, f.wx0 * f.wy1, f.wx1 * f.wy1);
    } else {
        const int i = tid - TP;
        const int cell = c0 + (i < nc ? i : 0);
        cello[i] = (long long)(cell / p.w) * p.tgt.stride_h + (long long)(cell % p.w) * p.tgt.stride_w;
    }
    if (nq < TP || nc < CELLS) {                                         // rows nobody stages stay zero
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < SH_STAGES / 16; i += NTHREADS) reinterpret_cast<f32x4*>(As)[i] = z;
    }

    // 2. the contraction, 64 channels at a time
    f32x16 acc[2][2];
    zero_acc(acc);
    float ss = 0.f;                                                      // squared norm of operand row `tid` (queries, then cells)
    const float* const base_s = p.src.data + img_s * p.src.stride_n;
    const float* const base_t = p.tgt.data + img_t * p.tgt.stride_n;
    for (int ch = 0; ch < p.NKC; ++ch) {
        __syncthreads();                                                 // taps published / the previous chunk's MFMAs have read the stages
        {
            const int c = ch * KC + lane;
            const bool chok = c < p.C;
            const int64_t cc = chok ? c : p.C - 1;
            const float* const lane_s = base_s + cc * p.src.stride_c;
#pragma unroll 4
            for (int q = wave; q < nq; q += 4) {
                const long long o = tapo[3 * q], dx = tapo[3 * q + 1], dy = tapo[3 * q + 2];
                const float4 wt = tapw[q];
                const float* g = lane_s + o;
                const float t0 = g[0], t1 = g[dx], t2 = g[dy], t3 = g[dx + dy];
                const float r = wt.x * t0 + wt.y * t1 + wt.z * t2 + wt.w * t3;
                As[q * LDA + lane] = chok ? r : 0.f;
            }
            if (!p.cell_fast) {
                const float* const lane_t = base_t + cc * p.tgt.stride_c;
#pragma unroll 8
                for (int j = wave; j < nc; j += 4) {
                    const float v = lane_t[cello[j]];
                    Bs[j * LDA + lane] = chok ? v : 0.f;
                }
            }
        }
        if (p.cell_fast) {
            const int j = tid & (CELLS - 1), sub = tid >> 7;
            if (j < nc) {
                const float* const cell_t = base_t + cello[j];
#pragma unroll 8
                for (int k = 0; k < KC / 2; ++k) {
                    const int c = ch * KC + 2 * k + sub;
                    const bool chok = c < p.C;
                    const float v = cell_t[(int64_t)(chok ? c : p.C - 1) * p.tgt.stride_c];
                    Bs[j * LDA + 2 * k + sub] = chok ? v : 0.f;
                }
            }
        }
        __syncthreads();
        {
            const f32x4* row = reinterpret_cast<const f32x4*>(As + tid * LDA);   // Bs follows As: row tid of both
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < KC / 4; ++k) {
                const f32x4 v = row[k];
                s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
            }
            ss += s;
        }
        mma_chunk_f32(As, Bs, acc, lane, wr, wc);
    }
    inv[tid] = 1.f / fmaxf(sqrtf(ss), 1e-12f);                           // F.normalize's eps
    __syncthreads();                                                     // the stages are dead: the result tile takes their place

    // 3. the tile: scale, park, write, reduce
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int col = 64 * wc + 32 * ni + (lane & 31);
        const float ib = inv[TP + col];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 64 * wr + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                T[row * LDT + col] = (acc[mi][ni][r] * inv[row]) * ib;
            }
    }
    __syncthreads();
    const int64_t qrow = img_s * p.N + q0;                               // first (image, query) row of the tile
    {
        const int col = tid & (CELLS - 1);
        if (col < nc)
            for (int row = tid >> 7; row < nq; row += 2) p.low[(qrow + row) * p.hw + c0 + col] = T[row * LDT + col];
    }
    if (tid < nq) {
        const float* t = T + tid * LDT;
        double sum = 0.0;
        float m = t[0];
        int at = 0;
        for (int j = 0; j < nc; ++j) {
            const float v = t[j];
            sum += (double)v;
            if (v > m) { m = v; at = j; }
        }
        const int64_t o = (qrow + tid) * p.NCH + blockIdx.x;
        p.psum[o] = sum;
        p.pmax[o] = m;
        p.pidx[o] = c0 + at;
    }
}

// torch's upsample_bilinear2d source index under align_corners=True: i0 = (int)(scale * I), the weight of i0 + 1
__device__ __forceinline__ int src_index(float scale, int I, int n, float& l1)
{
#pragma clang fp contract(off)                                           // the product is rounded, as torch's: no fma with the subtraction below
    const float r = scale * (float)I;
    int i0 = (int)r;
    i0 = i0 > n - 1 ? n - 1 : i0;                                        // memory safety only
    l1 = r - (float)i0;
    return i0;
}

__device__ __forceinline__ float lerp2(float lx0, float lx1, float ly0, float ly1, float v00, float v01, float v10, float v11)
{
#pragma clang fp contract(off)                                           // the three fmas below and no others
    const float top = __builtin_fmaf(lx1, v01, lx0 * v00), bot = __builtin_fmaf(lx1, v11, lx0 * v10);
    return __builtin_fmaf(ly1, bot, ly0 * top);
}

template <int V>
__global__ __launch_bounds__(NTHREADS) void heat_write_kernel(WriteParams p)
{
    extern __shared__ float4 smem4[];
    float* const L = reinterpret_cast<float*>(smem4);
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t row = (int64_t)blockIdx.z * p.N + blockIdx.y;
    const int Y0 = blockIdx.x * p.RB, Y1 = min(Y0 + p.RB, p.H);
    const bool center = !(p.flags & STEGO_HEAT_NO_CENTER), clamp = !(p.flags & STEGO_HEAT_NO_CLAMP);

    // the query's mean: the same butterfly in every wave of every workgroup of the query
    float mean = 0.f;
    if (center) {
        const double* ps = p.psum + row * p.NCH;
        double s = (lane < p.NCH ? ps[lane] : 0.0) + (lane + 64 < p.NCH ? ps[lane + 64] : 0.0);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        mean = (float)(s / (double)p.hw);
    }

    if (blockIdx.x == 0 && tid < 64 && (p.peak || p.best)) {
        const float* pm = p.pmax + row * p.NCH;
        const int32_t* pi = p.pidx + row * p.NCH;
        float m = pm[lane < p.NCH ? lane : 0];
        int at = pi[lane < p.NCH ? lane : 0];
        if (lane + 64 < p.NCH) {
            const float m2 = pm[lane + 64];
            if (m2 > m) { m = m2; at = pi[lane + 64]; }                  // (a later chunk: wins only when greater)
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float mo = __shfl_xor(m, d, 64);
            const int ao = __shfl_xor(at, d, 64);
            if (mo > m || (mo == m && ao < at)) { m = mo; at = ao; }
        }
        if (lane == 0) {
            float v = m - mean;
            if (clamp && !(v > 0.f)) { v = 0.f; at = 0; }                // no positive cell: every cell is 0, the first one wins
            if (p.peak) p.peak[row] = v;
            if (p.best) {
                const int cx = at % p.w, cy = at / p.w;
                p.best[2 * row + 0] = p.w > 1 ? 2.f * (float)cx / (float)(p.w - 1) - 1.f : 0.f;
                p.best[2 * row + 1] = p.h > 1 ? 2.f * (float)cy / (float)(p.h - 1) - 1.f : 0.f;
            }
        }
    }

    // the source rows of this block, centred and clamped
    float dummy;
    const int ylo = src_index(p.sy, Y0, p.h, dummy);
    const int yhi = min(src_index(p.sy, Y1 - 1, p.h, dummy) + 1, p.h - 1);
    const int nrows = min(yhi - ylo + 1, p.cap_rows);                    // (the host plan sized cap_rows for every block)
    {
        const float* lo = p.low + row * p.hw + (int64_t)ylo * p.w;
        for (int i = tid; i < nrows * p.w; i += NTHREADS) {
            const float v = lo[i] - mean;
            L[i] = clamp ? fmaxf(v, 0.f) : v;
        }
    }
    __syncthreads();

    // output: items of V pixels; thread tid takes items tid, tid + 256, ... of the block's rows
    const int WV = p.W / V;
    const int step_y = NTHREADS / WV, step_x = NTHREADS % WV;
    int Y = Y0 + tid / WV, xi = tid % WV;
    float* const out = p.heat + row * p.H * p.W;
    while (Y < Y1) {
        float ly1;
        const int y0 = src_index(p.sy, Y, p.h, ly1);
        const int y0r = min(y0 - ylo, nrows - 1), y1r = min(y0r + (y0 < p.h - 1 ? 1 : 0), nrows - 1);
        const float ly0 = 1.f - ly1;
        const float* r0 = L + y0r * p.w;
        const float* r1 = L + y1r * p.w;
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float lx1;
            const int x0 = src_index(p.sx, xi * V + k, p.w, lx1);
            const int x1 = x0 + (x0 < p.w - 1 ? 1 : 0);
            const float lx0 = 1.f - lx1;
            // one fixed sequence of roundings: both store widths give the same bits (weights 0 and 1 still copy exactly)
            o[k] = lerp2(lx0, lx1, ly0, ly1, r0[x0], r0[x1], r1[x0], r1[x1]);
        }
        float* dst = out + (int64_t)Y * p.W + xi * V;
        if constexpr (V == 4) {
            const f32x4 v = {o[0], o[1], o[2], o[3]};
            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst));
        } else {
            __builtin_nontemporal_store(o[0], dst);
        }
        Y += step_y;
        xi += step_x;
        if (xi >= WV) { xi -= WV; ++Y; }
    }
}

int check_desc(const StegoHeatDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->flags & ~(STEGO_HEAT_NO_CENTER | STEGO_HEAT_NO_CLAMP)) return STEGO_ERR_HEAT_FLAGS;
    if (d->C < 1 || d->C > STEGO_HEAT_MAX_C) return STEGO_ERR_HEAT_DIM;
    if (d->N < 1 || d->N > STEGO_HEAT_MAX_POINTS) return STEGO_ERR_HEAT_POINTS;
    if (d->B < 1 || d->B > 65535 || d->hs < 1 || d->hs > STEGO_HEAT_MAX_SIDE || d->ws < 1 || d->ws > STEGO_HEAT_MAX_SIDE) return STEGO_ERR_HEAT_SIZE;
    if (d->h < 1 || d->w < 1 || (int64_t)d->h * d->w > STEGO_HEAT_MAX_CELLS) return STEGO_ERR_HEAT_SIZE;
    if (d->H < 1 || d->H > STEGO_HEAT_MAX_OUT || d->W < 1 || d->W > STEGO_HEAT_MAX_OUT) return STEGO_ERR_HEAT_OUTPUT;
    return STEGO_OK;
}

struct Plan {
    int NCH, NT, RB, blocks, span, V;
    float sy, sx;
    size_t off_psum, off_low, off_pmax, off_pidx, ws_bytes, lds2;
};

// torch's area_pixel_compute_scale under align_corners=True
inline float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// the most source rows a block of RB output rows reads, with the kernel's own fp32 arithmetic
int max_span(const StegoHeatDesc* d, float sy, int RB)
{
    int span = 1;
    for (int Y0 = 0; Y0 < d->H; Y0 += RB) {
        const int Y1 = Y0 + RB < d->H ? Y0 + RB : d->H;
        int lo = (int)(sy * (float)Y0), hi = (int)(sy * (float)(Y1 - 1));
        lo = lo > d->h - 1 ? d->h - 1 : lo;
        hi = hi > d->h - 1 ? d->h - 1 : hi;
        hi = hi + 1 < d->h - 1 ? hi + 1 : d->h - 1;
        span = hi - lo + 1 > span ? hi - lo + 1 : span;
    }
    return span;
}

Plan plan(const StegoHeatDesc* d, bool vec_ok)
{
    Plan pl{};
    const int64_t hw = (int64_t)d->h * d->w, rows = (int64_t)d->B * d->N;
    pl.NCH = (int)((hw + CELLS - 1) / CELLS);
    pl.NT = (d->N + TP - 1) / TP;
    pl.sy = ac_scale(d->h, d->H);
    pl.sx = ac_scale(d->w, d->W);
    pl.V = (vec_ok && d->W % 4 == 0) ? 4 : 1;
    // one full pass of the workgroup at least (with 16-byte stores: the plan does not depend on the alignment of `heat`)
    const int per_pass = NTHREADS * (d->W % 4 == 0 ? 4 : 1);
    int lo = (per_pass + d->W - 1) / d->W;
    int64_t rb = rows * d->H / WG_TARGET;
    rb = rb > OUT_ROWS_MAX ? OUT_ROWS_MAX : rb;
    rb = rb < lo ? lo : rb;
    rb = rb > d->H ? d->H : rb;
    pl.RB = (int)rb;
    while (pl.RB > 1 && (int64_t)max_span(d, pl.sy, pl.RB) * d->w > LOW_LDS_FLOATS) --pl.RB;
    pl.span = max_span(d, pl.sy, pl.RB);             // RB == 1: at most two rows, and 2 * w <= h * w <= 16384 when h >= 2
    pl.blocks = (d->H + pl.RB - 1) / pl.RB;
    pl.lds2 = (size_t)pl.span * d->w * 4;
    WsLayout ws;                                     // packed tight: the fp64 sums come first, everything after them is 4-byte data
    pl.off_psum = ws.take((size_t)rows * pl.NCH * 8, 1);
    pl.off_low = ws.take((size_t)rows * hw * 4, 1);
    pl.off_pmax = ws.take((size_t)rows * pl.NCH * 4, 1);
    pl.off_pidx = ws.take((size_t)rows * pl.NCH * 4, 1);
    pl.ws_bytes = ws.total(8);
    return pl;
}

}  // namespace

extern "C" size_t stego_heat_workspace_bytes(const StegoHeatDesc* desc)
{
    return check_desc(desc) == STEGO_OK ? plan(desc, true).ws_bytes : 0;
}

extern "C" size_t stego_heat_plan(const StegoHeatDesc* desc, int32_t* grid1, int32_t* grid2, size_t* lds2, int32_t* out_rows)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    const Plan pl = plan(desc, true);
    if (grid1) { grid1[0] = pl.NCH; grid1[1] = pl.NT; grid1[2] = desc->B; }
    if (grid2) { grid2[0] = pl.blocks; grid2[1] = desc->N; grid2[2] = desc->B; }
    if (lds2) *lds2 = pl.lds2;
    if (out_rows) *out_rows = pl.RB;
    return LOW_LDS_BYTES;
}

extern "C" int stego_corr_heatmaps(const StegoHeatDesc* desc, const StegoMap* src, const StegoMap* tgt, const int64_t* index_t,
                                   const float* points, float* heat, float* peak, float* best, void* workspace, size_t workspace_bytes,
                                   stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!src || !src->data || !tgt || !tgt->data || !points || !heat || !workspace) return STEGO_ERR_NULL;
    const Plan pl = plan(desc, aligned(heat, 16));
    if (workspace_bytes < pl.ws_bytes) return STEGO_ERR_WORKSPACE;
    if (!aligned(src->data, 4) || !aligned(tgt->data, 4) || !aligned(points, 4) || !aligned(heat, 4) || !aligned(peak, 4) || !aligned(best, 4))
        return STEGO_ERR_ALIGN;
    if (!aligned(index_t, 8) || !aligned(workspace, 8)) return STEGO_ERR_ALIGN;

    LowParams lp{};
    lp.src = *src;
    lp.tgt = *tgt;
    lp.index_t = index_t;
    lp.points = points;
    lp.psum = at<double>(workspace, pl.off_psum);
    lp.low = at<float>(workspace, pl.off_low);
    lp.pmax = at<float>(workspace, pl.off_pmax);
    lp.pidx = at<int32_t>(workspace, pl.off_pidx);
    lp.B = desc->B;
    lp.C = desc->C;
    lp.hs = desc->hs;
    lp.ws = desc->ws;
    lp.w = desc->w;
    lp.hw = desc->h * desc->w;
    lp.N = desc->N;
    lp.NCH = pl.NCH;
    lp.NKC = (desc->C + KC - 1) / KC;
    const int64_t sc = tgt->stride_c < 0 ? -tgt->stride_c : tgt->stride_c, sw = tgt->stride_w < 0 ? -tgt->stride_w : tgt->stride_w;
    lp.cell_fast = sw < sc ? 1 : 0;

    WriteParams wp{};
    wp.psum = lp.psum;
    wp.low = lp.low;
    wp.pmax = lp.pmax;
    wp.pidx = lp.pidx;
    wp.heat = heat;
    wp.peak = peak;
    wp.best = best;
    wp.sy = pl.sy;
    wp.sx = pl.sx;
    wp.h = desc->h;
    wp.w = desc->w;
    wp.hw = lp.hw;
    wp.N = desc->N;
    wp.NCH = pl.NCH;
    wp.H = desc->H;
    wp.W = desc->W;
    wp.RB = pl.RB;
    wp.flags = desc->flags;
    wp.cap_rows = pl.span;

    const hipStream_t s = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    const hipError_t e = launch<heat_low_kernel>(dim3((unsigned)pl.NCH, (unsigned)pl.NT, (unsigned)desc->B), dim3(NTHREADS), (int)LOW_LDS_BYTES, s, lp);
    if (e != hipSuccess) return hip_rc(e);
    const dim3 grid2((unsigned)pl.blocks, (unsigned)desc->N, (unsigned)desc->B);
    return hip_rc(with_const<4, 1>(pl.V, [&](auto V) { return launch_next<heat_write_kernel<V()>>(grid2, NTHREADS, pl.lds2, s, wp); }));
}
