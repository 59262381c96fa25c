// dense_crf.hip - the fully-connected CRF of the reference's evaluation (src/crf.py:22-45, pydensecrf's DenseCRF2D) on the device:
// include/stego_crf.h has the mathematics and the ABI.
//
// Construction, once per image for the bilateral lattice (d = 5) and once per call for the Gaussian one (d = 2: it depends on H, W
// and pos_xy_std only, one structure serves the batch):
//   crf_embed_kernel       one thread per pixel: densecrf's embedding in fp32, in its operation order, FP contraction off (the keys
//                          and barycentric weights equal tests/crf_oracle.py's bit for bit); d+1 (packed key, entry, weight) records
//   rocprim radix sort     stable sort of the records by key: the unique keys are the vertices, and every vertex's records end up
//                          contiguous and in pixel order - a CSR list of its contributions, no hash table
//   crf_count / scan / emit   head flags -> vertex ids (exclusive scans), the entry -> vertex map for the slice, and the splat's
//                          pieces: a vertex's segment cut at every multiple of PIECE sorted positions, so that one group never sums
//                          more than PIECE records (a flat-colour region sends most of an image to a handful of bilateral vertices)
//   crf_neighbors_kernel   the 2 (d+1) blur neighbours of every vertex by binary search in the sorted keys (-1 = absent)
//   s = 1 / sqrt(L(1) + 1e-20)   one filtering pass of ones
// Per mean-field iteration, both lattices and all images of the batch in the same launches (blockIdx.y = image):
//   crf_splat_kernel       one group of G lanes per piece, a float4 of channels per lane: the weighted sum of s*Q over its records
//   crf_blur_kernel        d+1 ping-pong passes v' = v + (v[n1] + v[n2]) / 2 over [M, C_pad] rows; the first pass adds up each
//                          vertex's pieces as it reads it
//   crf_combine_kernel     per pixel: slice both lattices, -U + pos_w K_g + bi_w K_b, softmax over C (group shuffles); writes the next
//                          s_g * Q and s_b * Q, and Q itself ([B, C, H, W]) after the last iteration.  Once before the loop
//                          with `first` set: Q0 = softmax(-U) of what crf_unary_kernel wrote
// The softmax and the unary's log are evaluated in double and rounded once; everything else is fp32 in the oracle's order.
// No float atomics and no order that depends on scheduling: the result is bitwise identical run to run.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/stego_crf.h"
#include "host_util.h"

namespace stego_crf {

constexpr int TPB = 256;
constexpr int PIECE = 64;                    // most records one group sums in the splat
constexpr int SCAN_ITEMS = 4;                // sorted positions per thread in the vertex scan
constexpr int SCAN_BLOCK = TPB * SCAN_ITEMS;
constexpr int MAX_D = 5;

// one lattice of the workspace: image b's structure (records, vertices, neighbours, s) at base + b * stride + o_*, its value buffers
// at vbase + b * vstride + o_P / o_V.  The Gaussian lattice depends on H, W and pos_xy_std only: one structure (stride 0) serves
// every image of the batch.
struct Lat {
    char* base;
    size_t stride;
    char* vbase;
    size_t vstride;
    size_t o_psorted, o_wsorted, o_ventry, o_bary, o_pbeg, o_fpiece, o_nbr, o_counts, o_s, o_vkey, o_P, o_V;
    int E;                                   // records per image: N * (d + 1)
    int shared;                              // stride == 0: built once, for image 0
};

// per-pixel state of the iteration: -U, s_g * Q, s_b * Q as [N, C_pad]
struct Pix {
    char* base;
    size_t stride;
    size_t o_negu, o_sqg, o_sqb;
};

template <class T>
__host__ __device__ inline T* at(const Lat& L, size_t off, int b) { return reinterpret_cast<T*>(L.base + (size_t)b * L.stride + off); }
template <class T>
__host__ __device__ inline T* val(const Lat& L, size_t off, int b) { return reinterpret_cast<T*>(L.vbase + (size_t)b * L.vstride + off); }
template <class T>
__host__ __device__ inline T* at(const Pix& P, size_t off, int b) { return reinterpret_cast<T*>(P.base + (size_t)b * P.stride + off); }

__device__ inline float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ inline float4 add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline float4 mul(float w, float4 a) { return make_float4(w * a.x, w * a.y, w * a.z, w * a.w); }

template <int D>
__host__ __device__ constexpr int key_bits() { return D <= 2 ? 32 : 12; }

struct Scales { float v[MAX_D]; };

// ---------------------------------------------------------------------------------------------------------------- construction
template <int D>
__global__ __launch_bounds__(TPB) void crf_embed_kernel(const uint8_t* __restrict__ bgr, int H, int W, float sxy, float srgb, Scales sc,
                                                        uint64_t* __restrict__ keys, int* __restrict__ vals, float* __restrict__ bary)
{
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= H * W) return;
    float f[D];
    f[0] = (float)(k % W) / sxy;
    f[1] = (float)(k / W) / sxy;
    if constexpr (D == 5) {
        const uint8_t* p = bgr + (size_t)k * 3;
        f[2] = (float)p[0] / srgb;
        f[3] = (float)p[1] / srgb;
        f[4] = (float)p[2] / srgb;
    }
    float el[D + 1];
    float sm = 0.f;
#pragma unroll
    for (int j = D; j > 0; --j) {
        const float cf = f[j - 1] * sc.v[j - 1];
        el[j] = sm - (float)j * cf;
        sm += cf;
    }
    el[0] = sm;
    const float down = 1.0f / (float)(D + 1), up = (float)(D + 1);
    int rem0[D + 1];
    int sum = 0;
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        const float v = down * el[i];
        const float hi = ceilf(v) * up, lo = floorf(v) * up;
        rem0[i] = (hi - el[i] < el[i] - lo) ? (int)hi : (int)lo;       // a tie goes down
        sum += rem0[i];
    }
    sum /= (D + 1);
    int rank[D + 1];
#pragma unroll
    for (int i = 0; i <= D; ++i) rank[i] = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const float di = el[i] - (float)rem0[i];
#pragma unroll
        for (int j = i + 1; j <= D; ++j) {
            if (di < el[j] - (float)rem0[j]) rank[i]++;
            else rank[j]++;
        }
    }
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        rank[i] += sum;
        if (rank[i] < 0) { rank[i] += D + 1; rem0[i] += D + 1; }
        else if (rank[i] > D) { rank[i] -= D + 1; rem0[i] -= D + 1; }
    }
    float bc[D + 2];
#pragma unroll
    for (int t = 0; t < D + 2; ++t) bc[t] = 0.f;
#pragma unroll
    for (int i = 0; i <= D; ++i) {
        const float v = (el[i] - (float)rem0[i]) * down;
#pragma unroll
        for (int t = 0; t <= D; ++t)            // bc[D - rank[i]] += v; bc[D - rank[i] + 1] -= v  (unrolled: no private-memory indexing)
            if (t == D - rank[i]) { bc[t] += v; bc[t + 1] -= v; }
    }
    bc[0] = (float)((double)bc[0] + (1.0 + (double)bc[D + 1]));   // densecrf: float += 1.0 (a double) + float
    constexpr int bits = key_bits<D>();
    constexpr uint64_t mask = (bits == 32) ? 0xffffffffull : ((1ull << bits) - 1);
#pragma unroll
    for (int r = 0; r <= D; ++r) {
        uint64_t key = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const int c = rem0[i] + (rank[i] <= D - r ? r : r - (D + 1));      // canonical[r][rank[i]]
            key |= (uint64_t)(((uint32_t)c + (1u << (bits - 1))) & (uint32_t)mask) << (i * bits);     // biased, in unsigned arithmetic
        }
        const int e = k * (D + 1) + r;
        keys[e] = key;
        vals[e] = e;
        bary[e] = bc[r];
    }
}

__device__ inline int2 wave_incl_scan(int2 v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(v.x, o, 64), b = __shfl_up(v.y, o, 64);
        if (lane >= o) { v.x += a; v.y += b; }
    }
    return v;
}

// exclusive scan over the 256 threads of the block; *total = the block's sum
__device__ inline int2 block_excl_scan(int2 v, int2* total)
{
    __shared__ int2 wsum[TPB / 64];
    const int2 inc = wave_incl_scan(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wsum[w] = inc;
    __syncthreads();
    int2 off = make_int2(0, 0), tot = make_int2(0, 0);
#pragma unroll
    for (int i = 0; i < TPB / 64; ++i) {
        if (i < w) { off.x += wsum[i].x; off.y += wsum[i].y; }
        tot.x += wsum[i].x;
        tot.y += wsum[i].y;
    }
    __syncthreads();
    *total = tot;
    return make_int2(off.x + inc.x - v.x, off.y + inc.y - v.y);
}

// (heads, piece starts) of one thread's SCAN_ITEMS consecutive sorted positions
__device__ inline int2 flags_of(const uint64_t* keys, int i, int E, int* h, int* p)
{
    int2 c = make_int2(0, 0);
#pragma unroll
    for (int t = 0; t < SCAN_ITEMS; ++t) {
        const int q = i + t;
        h[t] = q < E && (q == 0 || keys[q] != keys[q - 1]);
        p[t] = q < E && (h[t] || q % PIECE == 0);
        c.x += h[t];
        c.y += p[t];
    }
    return c;
}

__global__ __launch_bounds__(TPB) void crf_count_kernel(const uint64_t* __restrict__ keys, int E, int2* __restrict__ blk)
{
    int h[SCAN_ITEMS], p[SCAN_ITEMS];
    const int2 c = flags_of(keys, blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS, E, h, p);
    int2 tot;
    block_excl_scan(c, &tot);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// one workgroup: exclusive scan of the block counts in place; the vertex and piece totals and the CSR sentinels
__global__ __launch_bounds__(TPB) void crf_scan_blocks_kernel(int2* __restrict__ blk, int nblk, int E, int* __restrict__ counts,
                                                              int* __restrict__ fpiece, int* __restrict__ pbeg)
{
    int2 carry = make_int2(0, 0);
    for (int i0 = 0; i0 < nblk; i0 += TPB) {
        const int i = i0 + threadIdx.x;
        const int2 v = i < nblk ? blk[i] : make_int2(0, 0);
        int2 tot;
        const int2 ex = block_excl_scan(v, &tot);
        if (i < nblk) blk[i] = make_int2(carry.x + ex.x, carry.y + ex.y);
        carry.x += tot.x;
        carry.y += tot.y;
    }
    if (threadIdx.x == 0) {
        counts[0] = carry.x;         // M: vertices
        counts[1] = carry.y;         // pieces
        fpiece[carry.x] = carry.y;
        pbeg[carry.y] = E;
    }
}

template <int D>
__global__ __launch_bounds__(TPB) void crf_emit_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals, const int2* __restrict__ blk,
                                                       int E, Lat L, int b)
{
    int h[SCAN_ITEMS], p[SCAN_ITEMS];
    const int i0 = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    const int2 c = flags_of(keys, i0, E, h, p);
    int2 tot;
    const int2 ex = block_excl_scan(c, &tot);
    int hv = blk[blockIdx.x].x + ex.x, pv = blk[blockIdx.x].y + ex.y;
    int* psorted = at<int>(L, L.o_psorted, b);
    float* wsorted = at<float>(L, L.o_wsorted, b);
    int* ventry = at<int>(L, L.o_ventry, b);
    const float* bary = at<float>(L, L.o_bary, b);
    int* pbeg = at<int>(L, L.o_pbeg, b);
    int* fpiece = at<int>(L, L.o_fpiece, b);
    uint64_t* vkey = at<uint64_t>(L, L.o_vkey, b);
#pragma unroll
    for (int t = 0; t < SCAN_ITEMS; ++t) {
        const int i = i0 + t;
        if (i >= E) break;
        hv += h[t];
        pv += p[t];
        const int vid = hv - 1, pid = pv - 1, e = vals[i];
        psorted[i] = e / (D + 1);
        wsorted[i] = bary[e];
        ventry[e] = vid;
        if (h[t]) { vkey[vid] = keys[i]; fpiece[vid] = pid; }
        if (p[t]) pbeg[pid] = i;
    }
}

template <int D>
__global__ __launch_bounds__(TPB) void crf_neighbors_kernel(Lat L, int b)
{
    constexpr int bits = key_bits<D>();
    constexpr uint64_t mask = (bits == 32) ? 0xffffffffull : ((1ull << bits) - 1);
    const int M = at<int>(L, L.o_counts, b)[0];
    const uint64_t* vkey = at<uint64_t>(L, L.o_vkey, b);
    int2* nbr = at<int2>(L, L.o_nbr, b);
    for (int v = blockIdx.x * TPB + threadIdx.x; v < M; v += gridDim.x * TPB) {
        const uint64_t key = vkey[v];
        int c[D];
#pragma unroll
        for (int i = 0; i < D; ++i) c[i] = (int)((uint32_t)((key >> (i * bits)) & mask) - (1u << (bits - 1)));
#pragma unroll
        for (int j = 0; j <= D; ++j) {
            int r[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int dir = s == 0 ? -1 : 1;                 // n1 = key - 1, n2 = key + 1; coordinate j: + d, - d
                uint64_t q = 0;
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const int ci = c[i] + (i == j ? -dir * D : dir);
                    q |= (uint64_t)(((uint32_t)ci + (1u << (bits - 1))) & (uint32_t)mask) << (i * bits);
                }
                int lo = 0, hi = M;                                  // lower bound of q in vkey[0, M)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (vkey[mid] < q) lo = mid + 1;
                    else hi = mid;
                }
                r[s] = (lo < M && vkey[lo] == q) ? lo : -1;
            }
            nbr[(size_t)j * L.E + v] = make_int2(r[0], r[1]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- filtering
// One group of G lanes per row; lane l holds channels 4l .. 4l+3 of a row of cq float4 (lanes >= cq idle).
// `in` = NULL: the input is 1 in channel 0 (the normalisation pass).
template <int G>
__global__ __launch_bounds__(TPB) void crf_splat_kernel(Lat L, const char* in_base, size_t in_stride, int cq)
{
    const int b = blockIdx.y;
    const int npieces = at<int>(L, L.o_counts, b)[1];
    const int* pbeg = at<int>(L, L.o_pbeg, b);
    const int* psorted = at<int>(L, L.o_psorted, b);
    const float* wsorted = at<float>(L, L.o_wsorted, b);
    float4* P = val<float4>(L, L.o_P, b);
    const float4* in = in_base ? reinterpret_cast<const float4*>(in_base + (size_t)b * in_stride) : nullptr;
    const int lane = threadIdx.x % G;
    const int ngrp = gridDim.x * (TPB / G);
    for (int p = blockIdx.x * (TPB / G) + threadIdx.x / G; p < npieces; p += ngrp) {
        if (lane >= cq) continue;
        const int i0 = pbeg[p], i1 = pbeg[p + 1];
        float4 acc = f4(0.f);
        int i = i0;
        for (; i + 4 <= i1; i += 4) {
            int px[4];
            float w[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { px[t] = psorted[i + t]; w[t] = wsorted[i + t]; }
            float4 x[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) x[t] = in ? in[(size_t)px[t] * cq + lane] : make_float4(1.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = add(acc, mul(w[t], x[t]));
        }
        for (; i < i1; ++i) {
            const float4 x = in ? in[(size_t)psorted[i] * cq + lane] : make_float4(1.f, 0.f, 0.f, 0.f);
            acc = add(acc, mul(wsorted[i], x));
        }
        P[(size_t)p * cq + lane] = acc;
    }
}

// pass j: out[v] = in[v] + (in[n1] + in[n2]) / 2.  FIRST: `in` holds pieces, a vertex is the sum of its pieces fpiece[v] .. fpiece[v+1]-1.
template <int G, bool FIRST>
__global__ __launch_bounds__(TPB) void crf_blur_kernel(Lat L, int j, int cq, size_t o_in, size_t o_out)
{
    const int b = blockIdx.y;
    const int M = at<int>(L, L.o_counts, b)[0];
    const int2* nbr = at<int2>(L, L.o_nbr, b) + (size_t)j * L.E;
    const int* fp = at<int>(L, L.o_fpiece, b);
    const float4* in = val<float4>(L, o_in, b);
    float4* out = val<float4>(L, o_out, b);
    const int lane = threadIdx.x % G;
    const int ngrp = gridDim.x * (TPB / G);
    auto row = [&](int x) {
        if (!FIRST) return in[(size_t)x * cq + lane];
        const int p0 = fp[x], p1 = fp[x + 1];
        float4 s = in[(size_t)p0 * cq + lane];
        for (int p = p0 + 1; p < p1; ++p) s = add(s, in[(size_t)p * cq + lane]);
        return s;
    };
    for (int v = blockIdx.x * (TPB / G) + threadIdx.x / G; v < M; v += ngrp) {
        if (lane >= cq) continue;
        const int2 n = nbr[v];
        const float4 a = row(v);
        const float4 x = n.x >= 0 ? row(n.x) : f4(0.f);
        const float4 y = n.y >= 0 ? row(n.y) : f4(0.f);
        out[(size_t)v * cq + lane] = add(a, mul(0.5f, add(x, y)));
    }
}

// s = 1 / sqrt(L(1) + 1e-20) per pixel (densecrf computes it in double); `fin` = the buffer the last blur pass wrote (cq = 1)
template <int D>
__global__ __launch_bounds__(TPB) void crf_norm_kernel(Lat L, int N, size_t o_fin)
{
    const int b = blockIdx.y;
    const int* ventry = at<int>(L, L.o_ventry, b);
    const float* bary = at<float>(L, L.o_bary, b);
    const float4* V = val<float4>(L, o_fin, b);
    float* s = at<float>(L, L.o_s, b);
    for (int k = blockIdx.x * TPB + threadIdx.x; k < N; k += gridDim.x * TPB) {
        float n = 0.f;
#pragma unroll
        for (int r = 0; r <= D; ++r) {
            const int e = k * (D + 1) + r;
            n += bary[e] * V[ventry[e]].x;
        }
        s[k] = (float)(1.0 / sqrt((double)n + 1e-20));
    }
}

template <int G>
__device__ inline float group_max(float v)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

template <int G>
__device__ inline double group_sum(double v)
{
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// softmax over the C valid channels of a pixel held by G lanes (channel 4 lane + t); invalid channels come out 0.  Evaluated in
// double on the float logits and rounded once: Q is the correctly rounded softmax of its input, whatever the group width and
// the order of the sum.  expf's ulp, the float sum and the float division were the kernels' largest rounding per iteration, and
// the mean-field multiplies what each iteration adds (about 2 x per iteration on colour noise)
template <int G>
__device__ inline float4 group_softmax(float4 x, int lane, int C)
{
    float v[4] = {x.x, x.y, x.z, x.w};
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (4 * lane + t < C) m = fmaxf(m, v[t]);
    m = group_max<G>(m);
    double e[4], s = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        e[t] = (4 * lane + t < C) ? exp((double)v[t] - (double)m) : 0.0;
        s += e[t];
    }
    s = group_sum<G>(s);
    return make_float4((float)(e[0] / s), (float)(e[1] / s), (float)(e[2] / s), (float)(e[3] / s));
}

struct CombineParams {
    Lat g, bl;
    Pix px;
    size_t og_fin, ob_fin;   // where the last blur pass of each lattice wrote
    int N, C, cq;
    int first;               // crf_combine_kernel: Q0 = softmax(-U), no lattice is read
    float pos_w, bi_w;
    float* q_out;            // [B, C, H, W], written when not NULL
    const float* probs;      // crf_unary_kernel: [B, C, H, W]
};

template <int D>
__device__ inline float4 slice(const Lat& L, size_t o_fin, int b, int k, int cq, int lane)
{
    const int* ventry = at<int>(L, L.o_ventry, b);
    const float* bary = at<float>(L, L.o_bary, b);
    const float4* V = val<float4>(L, o_fin, b);
    float4 acc = f4(0.f);
#pragma unroll
    for (int r = 0; r <= D; ++r) {
        const int e = k * (D + 1) + r;
        acc = add(acc, mul(bary[e], V[(size_t)ventry[e] * cq + lane]));
    }
    return acc;
}

template <int G>
__device__ inline void store_state(const CombineParams& p, int b, int k, int lane, float4 q)
{
    const float sg = at<float>(p.g, p.g.o_s, b)[k], sb = at<float>(p.bl, p.bl.o_s, b)[k];
    if (lane < p.cq) {
        at<float4>(p.px, p.px.o_sqg, b)[(size_t)k * p.cq + lane] = mul(sg, q);
        at<float4>(p.px, p.px.o_sqb, b)[(size_t)k * p.cq + lane] = mul(sb, q);
    }
    if (p.q_out) {
        const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = 4 * lane + t;
            if (c < p.C) p.q_out[((size_t)b * p.C + c) * p.N + k] = v[t];
        }
    }
}

// -U = log(clip(p, 1e-5, 1)), the log in double and rounded once.  Q0 = softmax(-U) is the combine kernel's, with p.first set: the
// double log and the double softmax in one kernel would not fit 8 waves per SIMD
template <int G>
__global__ __launch_bounds__(TPB) void crf_unary_kernel(CombineParams p)
{
    const int b = blockIdx.y, lane = threadIdx.x % G;
    const int ngrp = gridDim.x * (TPB / G);
    for (int k = blockIdx.x * (TPB / G) + threadIdx.x / G; k < p.N; k += ngrp) {
        float v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = 4 * lane + t;
            v[t] = c < p.C ? (float)log((double)fminf(fmaxf(p.probs[((size_t)b * p.C + c) * p.N + k], 1e-5f), 1.0f)) : 0.f;     // rounded once
        }
        const float4 nu = make_float4(v[0], v[1], v[2], v[3]);
        if (lane < p.cq) at<float4>(p.px, p.px.o_negu, b)[(size_t)k * p.cq + lane] = nu;
    }
}

template <int G>
__global__ __launch_bounds__(TPB) void crf_combine_kernel(CombineParams p)
{
    const int b = blockIdx.y, lane = threadIdx.x % G;
    const int ngrp = gridDim.x * (TPB / G);
    for (int k = blockIdx.x * (TPB / G) + threadIdx.x / G; k < p.N; k += ngrp) {
        float4 x = f4(0.f);
        if (lane < p.cq && p.first) {
            x = at<float4>(p.px, p.px.o_negu, b)[(size_t)k * p.cq + lane];
        } else if (lane < p.cq) {
            const float sg = at<float>(p.g, p.g.o_s, b)[k], sb = at<float>(p.bl, p.bl.o_s, b)[k];
            const float4 kg = mul(sg, slice<2>(p.g, p.og_fin, b, k, p.cq, lane));
            const float4 kb = mul(sb, slice<5>(p.bl, p.ob_fin, b, k, p.cq, lane));
            const float4 nu = at<float4>(p.px, p.px.o_negu, b)[(size_t)k * p.cq + lane];
            x = add(add(nu, mul(p.pos_w, kg)), mul(p.bi_w, kb));
        }
        store_state<G>(p, b, k, lane, group_softmax<G>(x, lane, p.C));
    }
}

// ---------------------------------------------------------------------------------------------------------------- host side
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Geom {
    int N, Cp, cq, G;
    Lat lat[2];                  // 0: Gaussian (d = 2), 1: bilateral (d = 5)
    Pix pix;
    size_t o_lat[2], o_val[2], o_pix, o_keys0, o_keys1, o_vals0, o_vals1, o_blk, o_sort;
    size_t sort_bytes, total;
};

inline int dims(int l) { return l == 0 ? 2 : 5; }

Geom geometry(const StegoCrfDesc* d)
{
    Geom g{};
    g.N = d->H * d->W;
    g.Cp = (d->C + 3) & ~3;
    g.cq = g.Cp / 4;
    g.G = 1;
    while (g.G < g.cq) g.G <<= 1;
    size_t off = 0;
    for (int l = 0; l < 2; ++l) {
        const int D = dims(l);
        const size_t E = (size_t)g.N * (D + 1);
        Lat& L = g.lat[l];
        L.E = (int)E;
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t r = o; o += align256(bytes); return r; };
        L.o_psorted = take(E * 4);
        L.o_wsorted = take(E * 4);
        L.o_ventry = take(E * 4);
        L.o_bary = take(E * 4);
        L.o_pbeg = take((E + 1) * 4);
        L.o_fpiece = take((E + 1) * 4);
        L.o_nbr = take(E * (D + 1) * 8);
        L.o_counts = take(16);
        L.o_s = take((size_t)g.N * 4);
        L.o_vkey = take(E * 8);
        L.shared = l == 0;
        L.stride = L.shared ? 0 : o;
        g.o_lat[l] = off;
        off += o * (L.shared ? 1 : d->B);
        o = 0;
        L.o_P = take(E * g.Cp * 4);             // pieces (<= E rows), then the odd blur passes
        L.o_V = take(E * g.Cp * 4);             // the even blur passes (M <= E rows)
        L.vstride = o;
        g.o_val[l] = off;
        off += o * d->B;
    }
    {
        size_t o = 0;
        auto take = [&](size_t bytes) { const size_t r = o; o += align256(bytes); return r; };
        g.pix.o_negu = take((size_t)g.N * g.Cp * 4);
        g.pix.o_sqg = take((size_t)g.N * g.Cp * 4);
        g.pix.o_sqb = take((size_t)g.N * g.Cp * 4);
        g.pix.stride = o;
        g.o_pix = off;
        off += o * d->B;
    }
    const size_t Emax = (size_t)g.N * 6;       // construction scratch, reused by every (image, lattice)
    auto take = [&](size_t bytes) { const size_t r = off; off += align256(bytes); return r; };
    g.o_keys0 = take(Emax * 8);
    g.o_keys1 = take(Emax * 8);
    g.o_vals0 = take(Emax * 4);
    g.o_vals1 = take(Emax * 4);
    g.o_blk = take((Emax / SCAN_BLOCK + 1) * 8);
    g.sort_bytes = ((size_t)4 << 20) + Emax * 8;   // rocprim's onesweep needs far less (checked at every call)
    g.o_sort = take(g.sort_bytes);
    g.total = off;
    return g;
}

// float scale factors as densecrf computes them (Permutohedral::init)
Scales scales(int D)
{
    Scales s{};
    const float inv = (float)(std::sqrt(2.0 / 3.0) * (D + 1));
    for (int i = 0; i < D; ++i) s.v[i] = (float)(1.0 / std::sqrt((double)((i + 1) * (i + 2))) * (double)inv);
    return s;
}

// |elevated| <= max_j (sum_{i >= j} cf_i + j cf_{j-1}); rounding, the rank shift, the canonical offset and a blur neighbour add at
// most 4 (d + 1): every key of the image and its neighbours then fits the packed field
bool lattice_fits(int D, int H, int W, float sxy, float srgb)
{
    const Scales sc = scales(D);
    double cf[MAX_D];
    for (int i = 0; i < D; ++i) {
        const double fmax = i == 0 ? (W - 1) / (double)sxy : i == 1 ? (H - 1) / (double)sxy : 255.0 / (double)srgb;
        cf[i] = fmax * sc.v[i] * (1.0 + 1e-5) + 1e-5;
    }
    double bound = 0;
    for (int j = 0; j <= D; ++j) {
        double s = 0;
        for (int i = j; i < D; ++i) s += cf[i];
        if (j > 0) s += j * cf[j - 1];
        bound = std::fmax(bound, s);
    }
    const int bits = D <= 2 ? 32 : 12;
    double limit = std::ldexp(1.0, bits - 1) - 1 - 4 * (D + 1);
    if (D <= 2) limit = std::fmin(limit, std::ldexp(1.0, 22));     // fp32 rounding to multiples of d+1 stays exact
    return bound < limit;
}

int check(const StegoCrfDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->n_iter < 0 || d->B > 65535) return STEGO_ERR_SHAPE;
    const float st[3] = {d->pos_xy_std, d->bi_xy_std, d->bi_rgb_std};
    for (float s : st)
        if (!(s > 0.f) || !std::isfinite(s)) return STEGO_ERR_SHAPE;
    if (!std::isfinite(d->pos_w) || !std::isfinite(d->bi_w)) return STEGO_ERR_SHAPE;
    if (d->C < 1 || d->C > STEGO_CRF_MAX_C) return STEGO_ERR_CRF_LIMITS;
    if ((int64_t)d->H * d->W * 6 >= ((int64_t)1 << 31)) return STEGO_ERR_CRF_LIMITS;
    if (!lattice_fits(2, d->H, d->W, d->pos_xy_std, 1.f) || !lattice_fits(5, d->H, d->W, d->bi_xy_std, d->bi_rgb_std)) return STEGO_ERR_CRF_RANGE;
    return STEGO_OK;
}

using stego::hip_rc;

inline dim3 grid(size_t work_items, int per_block, int B)
{
    const size_t cap = std::max<size_t>(1, 4096 / (size_t)B);
    const size_t n = (work_items + per_block - 1) / per_block;
    return dim3((unsigned)std::max<size_t>(1, std::min(n, cap)), (unsigned)B);
}

template <int D>
int build_lattice(const StegoCrfDesc* d, const Geom& g, int l, char* ws, const uint8_t* bgr, float sxy, float srgb, hipStream_t st)
{
    const Lat& L = g.lat[l];
    const int E = L.E, N = g.N;
    uint64_t* k0 = reinterpret_cast<uint64_t*>(ws + g.o_keys0);
    uint64_t* k1 = reinterpret_cast<uint64_t*>(ws + g.o_keys1);
    int* v0 = reinterpret_cast<int*>(ws + g.o_vals0);
    int* v1 = reinterpret_cast<int*>(ws + g.o_vals1);
    int2* blk = reinterpret_cast<int2*>(ws + g.o_blk);
    const int nblk = (E + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const Scales sc = scales(D);
    const unsigned end_bit = D <= 2 ? 64 : 12 * D;
    for (int b = 0; b < (L.shared ? 1 : d->B); ++b) {
        crf_embed_kernel<D><<<(N + TPB - 1) / TPB, TPB, 0, st>>>(bgr + (size_t)b * N * 3, d->H, d->W, sxy, srgb, sc, k0, v0,
                                                                 at<float>(L, L.o_bary, b));
        rocprim::double_buffer<uint64_t> kb(k0, k1);
        rocprim::double_buffer<int> vb(v0, v1);
        size_t need = 0;
        hipError_t e = rocprim::radix_sort_pairs(nullptr, need, kb, vb, E, 0, end_bit, st);
        if (e != hipSuccess) return hip_rc(e);
        if (need > g.sort_bytes) return STEGO_ERR_WORKSPACE;
        e = rocprim::radix_sort_pairs(ws + g.o_sort, need, kb, vb, E, 0, end_bit, st);
        if (e != hipSuccess) return hip_rc(e);
        crf_count_kernel<<<nblk, TPB, 0, st>>>(kb.current(), E, blk);
        crf_scan_blocks_kernel<<<1, TPB, 0, st>>>(blk, nblk, E, at<int>(L, L.o_counts, b), at<int>(L, L.o_fpiece, b), at<int>(L, L.o_pbeg, b));
        crf_emit_kernel<D><<<nblk, TPB, 0, st>>>(kb.current(), vb.current(), blk, E, L, b);
        crf_neighbors_kernel<D><<<(unsigned)std::min<size_t>(((size_t)E + TPB - 1) / TPB, 2048), TPB, 0, st>>>(L, b);
    }
    return hip_rc(hipGetLastError());
}

template <int G>
void filter_launches(const Geom& g, int l, int B, const char* in_base, size_t in_stride, int cq, hipStream_t st)
{
    const Lat& L = g.lat[l];
    const int D = dims(l);
    const dim3 gr = grid((size_t)L.E, TPB / G, B);
    crf_splat_kernel<G><<<gr, TPB, 0, st>>>(L, in_base, in_stride, cq);
    for (int j = 0; j <= D; ++j) {
        const size_t o_in = j == 0 ? L.o_P : (j & 1) ? L.o_V : L.o_P;
        const size_t o_out = (j & 1) ? L.o_P : L.o_V;
        if (j == 0) crf_blur_kernel<G, true><<<gr, TPB, 0, st>>>(L, j, cq, o_in, o_out);
        else crf_blur_kernel<G, false><<<gr, TPB, 0, st>>>(L, j, cq, o_in, o_out);
    }
}

inline size_t final_buffer(const Lat& L, int D) { return (D & 1) ? L.o_P : L.o_V; }     // pass D wrote P when D is odd

template <int G>
int iterate(const StegoCrfDesc* d, const Geom& g, char* ws, const float* probs, float* q_out, hipStream_t st)
{
    const int B = d->B;
    CombineParams p{};
    p.g = g.lat[0];
    p.bl = g.lat[1];
    p.px = g.pix;
    p.og_fin = final_buffer(g.lat[0], 2);
    p.ob_fin = final_buffer(g.lat[1], 5);
    p.N = g.N;
    p.C = d->C;
    p.cq = g.cq;
    p.pos_w = d->pos_w;
    p.bi_w = d->bi_w;
    p.probs = probs;
    p.q_out = d->n_iter == 0 ? q_out : nullptr;
    const dim3 gp = grid((size_t)g.N, TPB / G, B);
    crf_unary_kernel<G><<<gp, TPB, 0, st>>>(p);
    p.first = 1;
    crf_combine_kernel<G><<<gp, TPB, 0, st>>>(p);
    p.first = 0;
    const char* sqg = g.pix.base + g.pix.o_sqg;
    const char* sqb = g.pix.base + g.pix.o_sqb;
    for (int it = 0; it < d->n_iter; ++it) {
        filter_launches<G>(g, 0, B, sqg, g.pix.stride, g.cq, st);
        filter_launches<G>(g, 1, B, sqb, g.pix.stride, g.cq, st);
        p.q_out = it == d->n_iter - 1 ? q_out : nullptr;
        crf_combine_kernel<G><<<gp, TPB, 0, st>>>(p);
    }
    return hip_rc(hipGetLastError());
}

}  // namespace stego_crf

using namespace stego_crf;

extern "C" size_t stego_crf_workspace_bytes(const StegoCrfDesc* desc)
{
    if (check(desc) != STEGO_OK) return 0;
    return geometry(desc).total;
}

// crf.py:22-45 (see include/stego_crf.h)
extern "C" int stego_crf_run(const StegoCrfDesc* desc, const uint8_t* bgr_u8, const float* probs, float* q_out, void* workspace,
                             size_t workspace_bytes, stego_stream_t stream)
{
    const int rc = check(desc);
    if (rc != STEGO_OK) return rc;
    if (!bgr_u8 || !probs || !q_out || !workspace) return STEGO_ERR_NULL;
    if ((reinterpret_cast<uintptr_t>(probs) & 3) || (reinterpret_cast<uintptr_t>(q_out) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return STEGO_ERR_ALIGN;
    Geom g = geometry(desc);
    if (workspace_bytes < g.total) return STEGO_ERR_WORKSPACE;
    char* ws = static_cast<char*>(workspace);
    for (int l = 0; l < 2; ++l) {
        g.lat[l].base = ws + g.o_lat[l];
        g.lat[l].vbase = ws + g.o_val[l];
    }
    g.pix.base = ws + g.o_pix;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int r = build_lattice<2>(desc, g, 0, ws, bgr_u8, desc->pos_xy_std, 1.f, st);
    if (r == STEGO_OK) r = build_lattice<5>(desc, g, 1, ws, bgr_u8, desc->bi_xy_std, desc->bi_rgb_std, st);
    if (r != STEGO_OK) return r;
    for (int l = 0; l < 2; ++l) {                 // s = 1 / sqrt(L(1) + 1e-20): one pass of ones, one channel
        const Lat& L = g.lat[l];
        const int nb = L.shared ? 1 : desc->B;
        filter_launches<1>(g, l, nb, nullptr, 0, 1, st);
        const dim3 gr = grid((size_t)g.N, TPB, nb);
        if (l == 0) crf_norm_kernel<2><<<gr, TPB, 0, st>>>(L, g.N, final_buffer(L, 2));
        else crf_norm_kernel<5><<<gr, TPB, 0, st>>>(L, g.N, final_buffer(L, 5));
    }
    switch (g.G) {
        case 1: return iterate<1>(desc, g, ws, probs, q_out, st);
        case 2: return iterate<2>(desc, g, ws, probs, q_out, st);
        case 4: return iterate<4>(desc, g, ws, probs, q_out, st);
        case 8: return iterate<8>(desc, g, ws, probs, q_out, st);
        default: return iterate<16>(desc, g, ws, probs, q_out, st);
    }
}

extern "C" int stego_crf_lattice_info(const StegoCrfDesc* desc, const void* workspace, size_t workspace_bytes, int32_t b, int32_t which,
                                      int32_t* n_vertices, uint64_t* keys, int32_t max_keys, stego_stream_t stream)
{
    const int rc = check(desc);
    if (rc != STEGO_OK) return rc;
    if (!workspace || !n_vertices) return STEGO_ERR_NULL;
    if (b < 0 || b >= desc->B || (which != 0 && which != 1) || max_keys < 0) return STEGO_ERR_SHAPE;
    Geom g = geometry(desc);
    if (workspace_bytes < g.total) return STEGO_ERR_WORKSPACE;
    Lat L = g.lat[which];
    L.base = const_cast<char*>(static_cast<const char*>(workspace)) + g.o_lat[which];
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t M = 0;
    hipError_t e = hipMemcpyAsync(&M, at<int>(L, L.o_counts, b), 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_rc(e);
    *n_vertices = M;
    const int n = std::min(M, max_keys);
    if (keys && n > 0) {
        e = hipMemcpyAsync(keys, at<uint64_t>(L, L.o_vkey, b), (size_t)n * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hip_rc(e);
    }
    return STEGO_OK;
}
