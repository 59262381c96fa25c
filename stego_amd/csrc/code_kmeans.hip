// Cluster refit (include/stego_kmeans.h): spherical k-means over a resident [B, K, h, w] map of segmentation codes.
//
//   assign<NT, CT, DENSE>  the main launch of a Lloyd step.  A persistent workgroup (4 waves) owns a contiguous slab of 128-token tiles.  LDS
//                    holds c^ as [channel][centroid] and the tile's x^ as [channel][token], so that every operand read of the 32x32x2
//                    fp32 matrix instruction has its 32 lanes on consecutive words (the scores: A = centroids, B = tokens) or on an odd
//                    stride (the sums: B = channels).  Scores D[centroid][token]: a lane holds 16 of the 32 centroids of a tile for
//                    its token, so the first maximum is taken in registers and finished with one exchange between the lane halves.
//                    Sums D[centroid][channel] = one-hot[centroid][token] x^[token][channel]: the NT x CT output tiles are dealt to the
//                    four waves, fp32 accumulators folded into fp64 every 1024 tokens.  NT = ceil(n / 32), CT = ceil(K / 32).
//   finish           one workgroup per cluster: the partials in workgroup order, the new row, and behind an integer ticket the stats.
//   seed_weigh       a round of k-means++: best_p and the per-slab fp64 totals of the weights.
//   seed_pick        one workgroup: the slab that holds u * total, a scan inside it, the picked token's x^.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/stego_kmeans.h"
#include "addon_device.h"
#include "host_util.h"
#include "launchers.h"
#include "ws_layout.h"

using namespace stego;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAX_K = STEGO_KMEANS_MAX_K;
constexpr int MAX_N = STEGO_KMEANS_MAX_N;
constexpr int TT = STEGO_KMEANS_TILE;    // tokens of a tile: 32 per wave
constexpr int XT = TT + 1;               // floats of a staged channel row of x^ (odd: the sums' B operand strides over rows)
constexpr int CS = MAX_N;                // floats of a staged channel row of c^
constexpr int SEED_SLABS = 1024;         // slabs of a seeding round at the most
constexpr int SEED_TOKENS = 256;         // ... and tokens of a slab at the least
constexpr float ZERO_NORM = 2.f;         // best_p of a zero-norm token: its weight max(0, 1 - best_p) is 0 in every round
constexpr float UNSEEN = -2.f;           // best_p before the first centroid is there

struct StepParams {
    StegoMap map;
    const float* cin;
    float* cout;
    uint8_t* labels;
    int64_t* counts;
    double* stats;
    double* psum;                        // [G][n][K]
    int64_t* pcnt;                       // [G][n]
    double* pobj;                        // [G]
    double* rowstat;                     // [n][2]: c^old . c^new, kept
    unsigned* ticket;
    int64_t T, tiles, tiles_per;
    int K, KP, n, hw, w, G, chan_major, dense;
};

struct SeedParams {
    StegoMap map;
    float* cent;
    int64_t* picks;
    float* best;                         // [T]
    double* part;                        // [G]: the round's weights per slab
    double* part0;                       // [G]: round 0's
    int64_t T, slab;
    int K, n, hw, w, G, chan_major, round;
    double u;
};

// element offset of token tk (channel 0)
__device__ __forceinline__ int64_t token_offset(const StegoMap& m, int64_t tk, int hw, int w)
{
    const unsigned b = (unsigned)tk / (unsigned)hw;
    const unsigned pix = (unsigned)tk - b * (unsigned)hw;
    const unsigned y = pix / (unsigned)w, x = pix - y * (unsigned)w;
    return (int64_t)b * m.stride_n + (int64_t)y * m.stride_h + (int64_t)x * m.stride_w;
}

__device__ __forceinline__ double load_shared_f64(const double* p)
{
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}

__device__ __forceinline__ void store_shared_f64(double* p, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the Lloyd step
// A dense channels-last map is one flat array of T * K floats: a tile's 128 * K floats are read as float4, 256 at a time, into
// registers, all of them in flight at once, and scattered to xs[channel][token].  R4 float4 per thread.  Only a whole tile goes this
// way: the ragged last one takes the strided path.
template <int R4>
__device__ __forceinline__ void dense_prefetch(float4 (&pre)[R4], const float* src, int K, int t)
{
    asm volatile("" : "+v"(t));                                         // per call: the offsets are cheaper computed than kept
#pragma unroll
    for (int i = 0; i < R4; ++i) {
        const int e = 4 * (i * TPB + t);                                // 128 K is a multiple of 4: a float4 is inside the tile or not
        pre[i] = e < TT * K ? *reinterpret_cast<const float4*>(src + e) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

template <int R4>
__device__ __forceinline__ void dense_scatter(const float4 (&pre)[R4], float* xs, int K, float inv_k, int t)
{
    asm volatile("" : "+v"(t));                                         // per call: R4 * 4 LDS addresses are cheaper computed than kept
#pragma unroll
    for (int i = 0; i < R4; ++i) {
        const int e = 4 * (i * TPB + t);
        const float v[4] = {pre[i].x, pre[i].y, pre[i].z, pre[i].w};
        if (e < TT * K) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ee = e + j;
                const int k = (int)(((float)ee + 0.5f) * inv_k);        // ee / K, exact: ee < 2^14 and the quotient is 0.5 / K off an integer
                xs[(ee - k * K) * XT + k] = v[j];
            }
        }
        __builtin_amdgcn_sched_barrier(0);                              // one float4 at a time: its four addresses die with it
    }
}

constexpr size_t ASSIGN_FIXED = TPB * sizeof(double) + TT * sizeof(int) + MAX_N * sizeof(int);     // red, lab, cnt

template <int NT, int CT, bool DENSE>
__global__ __launch_bounds__(TPB) void kmeans_assign_kernel(const StepParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* red = reinterpret_cast<double*>(smem);                      // [TPB]
    int* lab = reinterpret_cast<int*>(red + TPB);                       // [TT]: the tile's labels, 255 beyond T
    int* cnt = lab + TT;                                                // [MAX_N]
    float* cs = reinterpret_cast<float*>(cnt + MAX_N);                  // [KP][CS]
    float* xs = cs + p.KP * CS;                                         // [KP][XT]
    constexpr int TILES = NT * CT, TPW = (TILES + WAVES - 1) / WAVES;   // output tiles of the sums, and of a wave
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 31, hf = lane >> 5;
    const int K = p.K, KP = p.KP, n = p.n;
    const bool sums = p.cout != nullptr;

    if (blockIdx.x == 0 && t == 0) *p.ticket = 0u;                      // the finish launch counts its workgroups here
    if (t < MAX_N) {
        cnt[t] = 0;
        double s = 0.0;
        if (t < n)
            for (int c = 0; c < K; ++c) {
                const double v = (double)p.cin[(int64_t)t * K + c];
                s = fma(v, v, s);
            }
        red[t] = fmax(sqrt(s), 1e-12);
    }
    __syncthreads();
    // The columns beyond n repeat centroid 0 instead of a test of the index per score: their scores are bitwise those of centroid 0, and
    // a tie always goes to the lower index, so none of them is ever the first maximum.
    for (int e = t; e < KP * CS; e += TPB) {
        const int c = e / CS, j = e - c * CS, src = j < n ? j : 0;
        cs[e] = c < K ? p.cin[(int64_t)src * K + c] / (float)red[src] : 0.f;
    }

    f32x16 acc[TPW];
    double acc64[TPW][16];
#pragma unroll
    for (int s = 0; s < TPW; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[s][r] = 0.f;
            acc64[s][r] = 0.0;
        }
    double obj = 0.0;
    int staged = 0;
    const int64_t tile0 = (int64_t)blockIdx.x * p.tiles_per;
    const int64_t tile1 = tile0 + p.tiles_per < p.tiles ? tile0 + p.tiles_per : p.tiles;
    constexpr int R4 = 4 * CT;                                          // 1024 R4 floats >= 128 K
    const float inv_k = 1.f / (float)K;
    if (DENSE && KP > K)
        for (int k = t; k < TT; k += TPB) xs[K * XT + k] = 0.f;         // the row that makes K even: never written again
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t base = tile * TT;
        __syncthreads();                                                // the last tile is read (the first time: cs is written)
        // the raw tokens -> xs[channel][token]; rows K .. KP - 1 and tokens beyond T are zero
        if (DENSE && base + TT <= p.T) {
            float4 pre[R4];
            dense_prefetch<R4>(pre, p.map.data + base * K, K, t);      // every load of the tile in flight at once; the registers are
            dense_scatter<R4>(pre, xs, K, inv_k, t);                    // free again for the products (the compute unit's other
                                                                        // workgroup computes meanwhile)
        } else if (DENSE || p.chan_major) {                                             // a lane per channel, a token per wave and step
#pragma unroll 4
            for (int k = wave; k < TT; k += WAVES) {
                const int64_t tk = base + k;
                const bool in = tk < p.T;
                const float* src = p.map.data + (in ? token_offset(p.map, tk, p.hw, p.w) : 0);
                for (int c = lane; c < KP; c += 64) xs[c * XT + k] = (in && c < K) ? src[(int64_t)c * p.map.stride_c] : 0.f;
            }
        } else {                                                        // a lane per token, two channels per step
            const int k = t & (TT - 1);
            const int64_t tk = base + k;
            const bool in = tk < p.T;
            const float* src = p.map.data + (in ? token_offset(p.map, tk, p.hw, p.w) : 0);
#pragma unroll 8
            for (int c = t >> 7; c < KP; c += TPB / TT) xs[c * XT + k] = (in && c < K) ? src[(int64_t)c * p.map.stride_c] : 0.f;
        }
        __syncthreads();
        {   // x^ = x / max(|x|, 1e-12): two threads per token, half of the channels each
            const int k = t & (TT - 1), c0 = (t >> 7) ? KP / 2 : 0, c1 = (t >> 7) ? KP : KP / 2;
            double s = 0.0;
            for (int c = c0; c < c1; ++c) {
                const double v = (double)xs[c * XT + k];
                s = fma(v, v, s);
            }
            red[t] = s;
            __syncthreads();
            const float d = (float)fmax(sqrt(red[k] + red[k + TT]), 1e-12);
            for (int c = c0; c < c1; ++c) xs[c * XT + k] = xs[c * XT + k] / d;
        }
        __syncthreads();
        // scores D[centroid][token] of the wave's 32 tokens
        f32x16 sc[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[i][r] = 0.f;
        {
            const float* ca = cs + hf * CS + li;                        // A[i = centroid li][k = channel 2 kk + hf]
            const float* xb = xs + hf * XT + wave * 32 + li;            // B[k = channel 2 kk + hf][j = token li]
            for (int kk = 0; kk < KP / 2; ++kk) {
                const float b = xb[2 * kk * XT];
#pragma unroll
                for (int i = 0; i < NT; ++i) sc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[2 * kk * CS + 32 * i], b, sc[i], 0, 0, 0);
            }
        }
        // the first maximum: ascending over the lane's own centroids, then between the two lane halves
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (sc[i][r] > bv) {
                    bv = sc[i][r];
                    bi = 32 * i + acc_row(r, hf);
                }
            }
        {
            const float ov = __shfl_xor(bv, 32);
            const int oi = __shfl_xor(bi, 32);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (bi >= n) {                                                  // nothing compared greater (NaNs): stay inside the tables
            bi = 0;
            bv = 0.f;
        }
        if (hf == 0) {
            const int k = wave * 32 + li;
            const int64_t tk = base + k;
            const bool in = tk < p.T;
            lab[k] = in ? bi : 255;
            if (in) {
                obj += (double)bv;
                atomicAdd(&cnt[bi], 1);                                 // an integer count in LDS
                if (p.labels) p.labels[tk] = (uint8_t)bi;
            }
        }
        __syncthreads();
        if (sums) {
#pragma unroll
            for (int s = 0; s < TPW; ++s) {
                const int id = wave + WAVES * s;                        // the same for the whole wave
                if (id < TILES) {
                    const int i = id % NT, ct = id / NT;
                    const int cl = 32 * i + li, ch = 32 * ct + li;
                    const bool ch_in = ch < KP;
                    const float* xr = xs + (ch_in ? ch : 0) * XT + hf;  // B[k = token 2 kk + hf][j = channel ch]
#pragma unroll 8
                    for (int kk = 0; kk < TT / 2; ++kk) {
                        const float a = lab[2 * kk + hf] == cl ? 1.f : 0.f;         // A[i = centroid cl][k = token 2 kk + hf]
                        const float b = ch_in ? xr[2 * kk] : 0.f;
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[s], 0, 0, 0);
                    }
                }
            }
            staged += TT;
            if (staged == STEGO_KMEANS_FOLD) {
#pragma unroll
                for (int s = 0; s < TPW; ++s)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        acc64[s][r] += (double)acc[s][r];
                        acc[s][r] = 0.f;
                    }
                staged = 0;
            }
        }
    }
    __syncthreads();
    const int g = blockIdx.x;
    if (sums) {
#pragma unroll
        for (int s = 0; s < TPW; ++s) {
            const int id = wave + WAVES * s;
            if (id < TILES) {
                const int i = id % NT, ct = id / NT, ch = 32 * ct + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = 32 * i + acc_row(r, hf);
                    if (row < n && ch < K) p.psum[((int64_t)g * n + row) * K + ch] = acc64[s][r] + (double)acc[s][r];
                }
            }
        }
    }
    if (t < n) p.pcnt[(int64_t)g * n + t] = (int64_t)cnt[t];
    obj = block_sum<TPB>(obj, red);
    if (t == 0) p.pobj[g] = obj;
}

__global__ __launch_bounds__(TPB) void kmeans_finish_kernel(const StepParams p)
{
    __shared__ double red[TPB];
    __shared__ long long ired[TPB];
    __shared__ int is_last;
    const int t = threadIdx.x, row = blockIdx.x, K = p.K, n = p.n;
    long long cn = 0;
    for (int g = t; g < p.G; g += TPB) cn += p.pcnt[(int64_t)g * n + row];
    ired[t] = cn;
    __syncthreads();
    for (int m = TPB / 2; m > 0; m >>= 1) {
        if (t < m) ired[t] += ired[t + m];
        __syncthreads();
    }
    const long long count = ired[0];
    if (t == 0) p.counts[row] = count;
    if (p.cout) {
        double s = 0.0;
        if (t < K) {
            const double* src = p.psum + (int64_t)row * K + t;
#pragma unroll 8
            for (int g = 0; g < p.G; ++g) s += src[(int64_t)g * n * K];           // in workgroup order
        }
        const double old = t < K ? (double)p.cin[(int64_t)row * K + t] : 0.0;
        const double nn = block_sum<TPB>(s * s, red);
        __syncthreads();
        const double on = block_sum<TPB>(old * old, red);
        __syncthreads();
        const bool kept = count == 0 || !(nn > 0.0);
        const double oh = old / fmax(sqrt(on), 1e-12);
        const float nf = (float)(kept ? oh : s / sqrt(nn));
        const double dot = block_sum<TPB>(oh * (double)nf, red);
        if (t < K) p.cout[(int64_t)row * K + t] = nf;
        if (t == 0) {
            store_shared_f64(p.rowstat + 2 * row, dot);
            store_shared_f64(p.rowstat + 2 * row + 1, kept ? 1.0 : 0.0);
        }
    }
    // the workgroup that takes the last ticket has every other one's counts and row statistics behind it
    __threadfence();
    __syncthreads();
    if (t == 0) is_last = atomicAdd(p.ticket, 1u) == (unsigned)(n - 1);
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    double o = 0.0;
    for (int g = t; g < p.G; g += TPB) o += p.pobj[g];
    o = block_sum<TPB>(o, red);
    if (t == 0) {
        double kept = 0.0, lo = 1.0;
        if (p.cout) {
            lo = INFINITY;
            for (int j = 0; j < n; ++j) {
                lo = fmin(lo, load_shared_f64(p.rowstat + 2 * j));
                kept += load_shared_f64(p.rowstat + 2 * j + 1);
            }
        }
        p.stats[0] = o;
        p.stats[1] = kept;
        p.stats[2] = 1.0 - lo;
        p.stats[3] = (double)p.T;
    }
}

// ---- k-means++
// x . c and |x|^2 of one token in fp64 by a wave (a lane per channel): valid in every lane
__device__ __forceinline__ void wave_dot(const float* src, int64_t sc, const float* c, int K, int lane, double& dot, double& ss)
{
    dot = 0.0;
    ss = 0.0;
    for (int ch = lane; ch < K; ch += 64) {
        const double v = (double)src[(int64_t)ch * sc];
        dot = fma(v, (double)c[ch], dot);
        ss = fma(v, v, ss);
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        dot += __shfl_xor(dot, m);
        ss += __shfl_xor(ss, m);
    }
}

__device__ __forceinline__ float seed_best(float before, double dot, double ss, bool first)
{
    if (first) return ss > 0.0 ? UNSEEN : ZERO_NORM;
    if (before == ZERO_NORM) return ZERO_NORM;
    return fmaxf(before, (float)(dot / fmax(sqrt(ss), 1e-12)));
}

__device__ __forceinline__ double seed_weight(float best, bool first)
{
    if (first) return best == ZERO_NORM ? 0.0 : 1.0;
    return fmax(0.0, 1.0 - (double)best);
}

__global__ __launch_bounds__(TPB) void kmeans_seed_weigh_kernel(const SeedParams p)
{
    __shared__ float c[MAX_K];
    __shared__ double red[TPB];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, g = blockIdx.x, K = p.K;
    const bool first = p.round == 0;
    if (t < MAX_K) c[t] = (!first && t < K) ? p.cent[(int64_t)(p.round - 1) * K + t] : 0.f;
    __syncthreads();
    const int64_t t0 = (int64_t)g * p.slab, t1 = t0 + p.slab < p.T ? t0 + p.slab : p.T;
    double wsum = 0.0;
    if (p.chan_major) {                                                 // a wave per token, a lane per channel
        for (int64_t tk = t0 + wave; tk < t1; tk += WAVES) {
            double dot, ss;
            wave_dot(p.map.data + token_offset(p.map, tk, p.hw, p.w), p.map.stride_c, c, K, lane, dot, ss);
            const float b = seed_best(first ? 0.f : p.best[tk], dot, ss, first);
            if (lane == 0) {
                p.best[tk] = b;
                wsum += seed_weight(b, first);
            }
        }
    } else {                                                            // a thread per token
        for (int64_t tk = t0 + t; tk < t1; tk += TPB) {
            const float* src = p.map.data + token_offset(p.map, tk, p.hw, p.w);
            double dot = 0.0, ss = 0.0;
#pragma unroll 4
            for (int ch = 0; ch < K; ++ch) {
                const double v = (double)src[(int64_t)ch * p.map.stride_c];
                dot = fma(v, (double)c[ch], dot);
                ss = fma(v, v, ss);
            }
            const float b = seed_best(first ? 0.f : p.best[tk], dot, ss, first);
            p.best[tk] = b;
            wsum += seed_weight(b, first);
        }
    }
    wsum = block_sum<TPB>(wsum, red);
    if (t == 0) {
        p.part[g] = wsum;
        if (first) p.part0[g] = wsum;
    }
}

__global__ __launch_bounds__(TPB) void kmeans_seed_pick_kernel(const SeedParams p)
{
    __shared__ double pl[SEED_SLABS];
    __shared__ double scan[TPB];
    __shared__ double sh_cum, sh_target;
    __shared__ int sh_slab, sh_first, sh_found, sh_last;
    const int t = threadIdx.x, K = p.K;
    const bool round0 = p.round == 0;
    for (int i = t; i < p.G; i += TPB) pl[i] = p.part[i];
    __syncthreads();
    if (t == 0) {
        double tot = 0.0;
        for (int i = 0; i < p.G; ++i) tot += pl[i];
        sh_first = (round0 || !(tot > 0.0)) ? 1 : 0;                    // no weight left: round 0's weights
    }
    __syncthreads();
    const bool first = sh_first != 0;
    if (first && !round0) {
        for (int i = t; i < p.G; i += TPB) pl[i] = p.part0[i];
        __syncthreads();
    }
    if (t == 0) {
        double tot = 0.0;
        for (int i = 0; i < p.G; ++i) tot += pl[i];
        const double target = p.u * tot;
        double cum = 0.0, before = 0.0;
        int slab = -1, last = 0;
        for (int i = 0; i < p.G; ++i) {
            if (pl[i] > 0.0) {
                last = i;
                before = cum;
            }
            if (cum + pl[i] > target) {
                slab = i;
                break;
            }
            cum += pl[i];
        }
        if (slab < 0) {                                                 // rounding: the last slab with any weight
            slab = last;
            cum = before;
        }
        sh_slab = slab;
        sh_cum = cum;
        sh_target = target;
        sh_found = 0x7fffffff;
        sh_last = -1;
    }
    __syncthreads();
    const int64_t t0 = (int64_t)sh_slab * p.slab, t1 = t0 + p.slab < p.T ? t0 + p.slab : p.T;
    const double target = sh_target;
    double running = sh_cum;
    for (int64_t cb = t0; cb < t1; cb += TPB) {
        const int64_t tk = cb + t;
        double w = 0.0;
        if (tk < t1) w = seed_weight(p.best[tk], first);
        scan[t] = w;
        __syncthreads();
        for (int d = 1; d < TPB; d <<= 1) {                             // the inclusive sums of the chunk
            const double v = t >= d ? scan[t - d] : 0.0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        if (w > 0.0) {
            if (running + scan[t] > target) atomicMin(&sh_found, (int)(tk - t0));
            atomicMax(&sh_last, (int)(tk - t0));
        }
        running += scan[TPB - 1];
        __syncthreads();
        if (sh_found != 0x7fffffff) break;
    }
    const int64_t pick = sh_found != 0x7fffffff ? t0 + sh_found : sh_last >= 0 ? t0 + sh_last : 0;
    const float v = t < K ? p.map.data[token_offset(p.map, pick, p.hw, p.w) + (int64_t)t * p.map.stride_c] : 0.f;
    __syncthreads();
    const double ss = block_sum<TPB>((double)v * (double)v, scan);
    if (t < K) p.cent[(int64_t)p.round * K + t] = v / (float)fmax(sqrt(ss), 1e-12);
    if (t == 0) p.picks[p.round] = pick;
}

// ---- host
int check_desc(const StegoKmeansDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->K < 1 || d->K > MAX_K || d->n < 1 || d->n > MAX_N) return STEGO_ERR_KMEANS_DIM;
    if (d->B < 1 || d->B > 65535 || d->h < 1 || d->w < 1) return STEGO_ERR_KMEANS_SIZE;
    const int64_t hw = (int64_t)d->h * d->w;
    if (hw > INT32_MAX || (int64_t)d->B * hw > INT32_MAX) return STEGO_ERR_KMEANS_SIZE;
    return STEGO_OK;
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// lanes run over the channels where those are the closer together in memory (the channels-last view), else over the tokens
int channel_major(const StegoMap* m)
{
    const int64_t sc = m->stride_c < 0 ? -m->stride_c : m->stride_c, sw = m->stride_w < 0 ? -m->stride_w : m->stride_w;
    return sc <= sw;
}

struct Plan {
    int64_t T, tiles, tiles_per, seed_slab;
    int G, KP, seed_G;
    size_t lds, psum, pcnt, pobj, rowstat, ticket, best, part, part0, total;
};

Plan plan(const StegoKmeansDesc* d)
{
    Plan pl{};
    pl.T = (int64_t)d->B * d->h * d->w;
    pl.tiles = ceil_div(pl.T, TT);
    pl.tiles_per = ceil_div(pl.tiles, STEGO_KMEANS_MAX_WORKGROUPS);
    pl.G = (int)ceil_div(pl.tiles, pl.tiles_per);
    pl.KP = (d->K + 1) & ~1;
    pl.lds = ASSIGN_FIXED + (size_t)pl.KP * (CS + XT) * sizeof(float);
    const int64_t slabs = ceil_div(pl.T, SEED_TOKENS);
    pl.seed_slab = ceil_div(pl.T, slabs < SEED_SLABS ? slabs : SEED_SLABS);
    pl.seed_G = (int)ceil_div(pl.T, pl.seed_slab);
    WsLayout ws;
    pl.psum = ws.take((size_t)pl.G * d->n * d->K * sizeof(double), 16);
    pl.pcnt = ws.take((size_t)pl.G * d->n * sizeof(int64_t), 16);
    pl.pobj = ws.take((size_t)pl.G * sizeof(double), 16);
    pl.rowstat = ws.take((size_t)2 * d->n * sizeof(double), 16);
    pl.ticket = ws.take(16, 16);
    const size_t step = ws.total(16);
    WsLayout ws2;                                                       // the seeding has the workspace to itself
    pl.best = ws2.take((size_t)pl.T * sizeof(float), 16);
    pl.part = ws2.take((size_t)pl.seed_G * sizeof(double), 16);
    pl.part0 = ws2.take((size_t)pl.seed_G * sizeof(double), 16);
    const size_t seed = ws2.total(16);
    pl.total = step > seed ? step : seed;
    return pl;
}

template <int NT, int CT>
hipError_t launch_assign(int G, size_t lds, hipStream_t s, const StepParams& p)
{
    if (p.dense) return launch_first<kmeans_assign_kernel<NT, CT, true>>(dim3((unsigned)G), TPB, lds, s, p);
    return launch_first<kmeans_assign_kernel<NT, CT, false>>(dim3((unsigned)G), TPB, lds, s, p);
}

hipError_t dispatch_assign(int nt, int ct, int G, size_t lds, hipStream_t s, const StepParams& p)
{
    switch (4 * (nt - 1) + ct - 1) {
        case 0: return launch_assign<1, 1>(G, lds, s, p);
        case 1: return launch_assign<1, 2>(G, lds, s, p);
        case 2: return launch_assign<1, 3>(G, lds, s, p);
        case 3: return launch_assign<1, 4>(G, lds, s, p);
        case 4: return launch_assign<2, 1>(G, lds, s, p);
        case 5: return launch_assign<2, 2>(G, lds, s, p);
        case 6: return launch_assign<2, 3>(G, lds, s, p);
        case 7: return launch_assign<2, 4>(G, lds, s, p);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

extern "C" size_t stego_kmeans_workspace_bytes(const StegoKmeansDesc* desc)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    return plan(desc).total;
}

extern "C" size_t stego_kmeans_plan(const StegoKmeansDesc* desc, int32_t* workgroups)
{
    const bool ok = check_desc(desc) == STEGO_OK;
    const Plan pl = ok ? plan(desc) : Plan{};
    if (workgroups) *workgroups = ok ? pl.G : 0;
    return ok ? pl.lds : 0;
}

extern "C" int stego_kmeans_step(const StegoKmeansDesc* desc, const StegoMap* codes, const float* centroids_in, float* centroids_out,
                                 uint8_t* labels, int64_t* counts, double* stats, void* workspace, size_t workspace_bytes,
                                 stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!codes || !codes->data || !centroids_in || !counts || !stats || !workspace) return STEGO_ERR_NULL;
    const Plan pl = plan(desc);
    if (workspace_bytes < pl.total) return STEGO_ERR_WORKSPACE;
    if (!aligned(codes->data, 4) || !aligned(centroids_in, 4) || !aligned(centroids_out, 4) || !aligned(counts, 8) || !aligned(stats, 8) ||
        !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;
    StepParams p{};
    p.map = *codes;
    p.cin = centroids_in;
    p.cout = centroids_out;
    p.labels = labels;
    p.counts = counts;
    p.stats = stats;
    p.psum = at<double>(workspace, pl.psum);
    p.pcnt = at<int64_t>(workspace, pl.pcnt);
    p.pobj = at<double>(workspace, pl.pobj);
    p.rowstat = at<double>(workspace, pl.rowstat);
    p.ticket = at<unsigned>(workspace, pl.ticket);
    p.T = pl.T;
    p.tiles = pl.tiles;
    p.tiles_per = pl.tiles_per;
    p.K = desc->K;
    p.KP = pl.KP;
    p.n = desc->n;
    p.hw = desc->h * desc->w;
    p.w = desc->w;
    p.G = pl.G;
    p.chan_major = channel_major(codes);
    // one flat [T][K] array (the strides of a dimension of size 1 say nothing): float4 reads, a tile ahead
    p.dense = codes->stride_c == 1 && (desc->w == 1 || codes->stride_w == desc->K) &&
              (desc->h == 1 || codes->stride_h == (int64_t)desc->w * desc->K) &&
              (desc->B == 1 || codes->stride_n == (int64_t)desc->h * desc->w * desc->K) && aligned(codes->data, 16);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = dispatch_assign((desc->n + 31) / 32, (desc->K + 31) / 32, pl.G, pl.lds, s, p);
    if (e == hipSuccess) e = launch_next<kmeans_finish_kernel>(dim3((unsigned)desc->n), TPB, 0, s, p);
    return hip_rc(e);
}

extern "C" int stego_kmeans_seed(const StegoKmeansDesc* desc, const StegoMap* codes, const double* u, float* centroids, int64_t* picks,
                                 void* workspace, size_t workspace_bytes, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!codes || !codes->data || !u || !centroids || !picks || !workspace) return STEGO_ERR_NULL;
    const Plan pl = plan(desc);
    if (workspace_bytes < pl.total) return STEGO_ERR_WORKSPACE;
    if (!aligned(codes->data, 4) || !aligned(centroids, 4) || !aligned(picks, 8) || !aligned(u, 8) || !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;
    for (int r = 0; r < desc->n; ++r)
        if (!(u[r] >= 0.0 && u[r] < 1.0)) return STEGO_ERR_KMEANS_DRAW;
    SeedParams p{};
    p.map = *codes;
    p.cent = centroids;
    p.picks = picks;
    p.best = at<float>(workspace, pl.best);
    p.part = at<double>(workspace, pl.part);
    p.part0 = at<double>(workspace, pl.part0);
    p.T = pl.T;
    p.slab = pl.seed_slab;
    p.K = desc->K;
    p.n = desc->n;
    p.hw = desc->h * desc->w;
    p.w = desc->w;
    p.G = pl.seed_G;
    p.chan_major = channel_major(codes);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    for (int r = 0; r < desc->n && e == hipSuccess; ++r) {
        p.round = r;
        p.u = u[r];
        e = r == 0 ? launch_first<kmeans_seed_weigh_kernel>(dim3((unsigned)pl.seed_G), TPB, 0, s, p)
                   : launch_next<kmeans_seed_weigh_kernel>(dim3((unsigned)pl.seed_G), TPB, 0, s, p);
        if (e == hipSuccess) e = launch_next<kmeans_seed_pick_kernel>(dim3(1), TPB, 0, s, p);
    }
    return hip_rc(e);
}
