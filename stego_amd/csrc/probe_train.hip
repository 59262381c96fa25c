// Fused training tail of the two probes (include/stego_probe_train.h): the linear probe's cross-entropy at label resolution, the
// cluster probe's cosine k-means loss at code resolution and their gradients to the three parameters, in two launches that write no
// [B, n, H, W] tensor.
//
// Launch 1, probe_train_kernel: g_lin + g_clu workgroups of 256 threads; both counts depend on the descriptor alone.
//   The last g_lin workgroups walk the output tiles t = index, index + g_lin, ... of the linear probe.  Per tile (planned as in
//   probe_head.hip, TY x TX <= 256 label pixels of one image):
//     1. the tile's source footprint of the code goes to LDS, with a channel K that holds 1 (the bias' "code"), and the tile's
//        interpolation weights as two small dense matrices wy[footprint row][tile row], wx[footprint column][tile column];
//     2. every footprint pixel is projected onto the probe (W c + b, one wave per four labels, the weight rows wave-uniform);
//     3. every thread takes one label pixel: the four-tap interpolation of the projections, the softmax, its loss term, and the
//        logit gradient softmax - onehot (0 for an invalid pixel) into LDS;
//     4. gather form of the interpolation's adjoint: every (footprint pixel, label) sums wy * wx * gradient over the tile pixels that
//        touch it, in a fixed order - the footprint-resolution logit gradient G;
//     5. acc[label, channel] += sum over the footprint of G * code: a register tile per thread that lives across all tiles.
//   The first g_clu workgroups walk chunks of 64 code pixels of the cluster probe: normalise the pixels in LDS, project them
//   onto the clusters, take the first maximum, turn it into a one-hot "G" and run the same step 5 on the normalised code.
//   Each workgroup writes ONE partial: its [n, K (+ 1)] sums, its loss sum and (linear) its count of valid pixels.
// Launch 2, probe_train_reduce: one workgroup per parameter row adds the partials in a fixed order (fp64: contiguous slices of the workgroups, then the slices), divides by n_valid / P and
//   applies the adjoint of the clusters' normalisation; one more workgroup writes the two losses and n_valid.
// No atomics anywhere: repeat launches give the same bits.  Every pixel offset is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/stego_probe_train.h"
#include "host_util.h"
#include "probe_common.h"

namespace {

constexpr int TPB = 256;
constexpr int JB = 4;                           // label rows a wave projects at a time (independent FMA chains)
constexpr int LOADS = 4;                        // global loads a thread keeps in flight while a footprint / chunk is staged
constexpr int CP = 64;                          // code pixels per chunk of the cluster probe
constexpr int MAX_LIN_WG = 768, MAX_CLU_WG = 256;   // 256 compute units x 3 resident workgroups; the cluster chunks are short
constexpr size_t FOOT_BUDGET = 48 * 1024;       // LDS of a tile's footprint (code, projections, weight matrices)
constexpr int RED_FLOATS = 3 * TPB;             // block-reduction scratch at the LDS base: 256 int64 + 256 float

struct TrainParams {
    StegoMap code;
    const int64_t* label;
    const float* lin_w;
    const float* lin_b;
    const float* clusters;
    float* part_lin;                 // [g_lin][n_lin][K + 1]
    float* loss_lin;                 // [g_lin]
    long long* cnt_lin;              // [g_lin]
    float* part_clu;                 // [g_clu][n_clu][K]
    float* loss_clu;                 // [g_clu]
    int32_t K, h, w, H, W, n_lin, n_clu;
    float scale_h, scale_w;
    int32_t TY, TX, max_nr, max_nc;  // output tile, footprint capacity (rows, columns)
    int32_t KS, NPS, NG;             // LDS floats per pixel: code (odd, > K), projections, logit gradient (odd)
    int32_t tiles_x, tiles_y, g_lin, g_clu;
    int64_t n_tiles, P, n_chunks;    // P = B h w code pixels
};

// The register tile of step 5: thread t owns labels tj + JT a (a < A) and channels tk + KT b (b < BM, 129 channels at the most).
template <int NMAX>
struct Own {
    static constexpr int JT = NMAX < 16 ? NMAX : 16, A = NMAX / JT, KT = TPB / JT, BM = (STEGO_PTRAIN_MAX_K + 1 + KT - 1) / KT;
};

// acc[label][channel] += sum_q G[q][label] * cs[q][channel] over the first npx pixels, channels [0, kdim)
template <int NMAX>
__device__ inline void accumulate(float (&acc)[Own<NMAX>::A][Own<NMAX>::BM], const float* G, const float* cs, int npx, int kdim, int NPS,
                                  int KS)
{
    using O = Own<NMAX>;
    const int tj = threadIdx.x % O::JT, tk = threadIdx.x / O::JT;
    for (int q = 0; q < npx; ++q) {
        float gv[O::A];
#pragma unroll
        for (int a = 0; a < O::A; ++a) gv[a] = G[q * NPS + tj + O::JT * a];
#pragma unroll
        for (int b = 0; b < O::BM; ++b) {
            const int k = tk + O::KT * b;
            if (O::KT * b < kdim) {
                const float c = cs[q * KS + min(k, KS - 1)];   // channels past kdim: sums that write_partial drops
#pragma unroll
                for (int a = 0; a < O::A; ++a) acc[a][b] = fmaf(gv[a], c, acc[a][b]);
            }
        }
    }
}

template <int NMAX>
__device__ inline void write_partial(const float (&acc)[Own<NMAX>::A][Own<NMAX>::BM], float* part, int n, int kdim)
{
    using O = Own<NMAX>;
    const int tj = threadIdx.x % O::JT, tk = threadIdx.x / O::JT;
#pragma unroll
    for (int a = 0; a < O::A; ++a)
#pragma unroll
        for (int b = 0; b < O::BM; ++b) {
            const int j = tj + O::JT * a, k = tk + O::KT * b;
            if (j < n && k < kdim) part[(size_t)j * kdim + k] = acc[a][b];
        }
}

// Sum of one float and one count per thread over the workgroup, in a fixed tree; the result is valid in thread 0.
__device__ inline void block_sum(float& v, long long& c, float* red)
{
    long long* rc = reinterpret_cast<long long*>(red);
    float* rf = red + 2 * TPB;
    __syncthreads();
    rf[threadIdx.x] = v;
    rc[threadIdx.x] = c;
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            rf[threadIdx.x] += rf[threadIdx.x + s];
            rc[threadIdx.x] += rc[threadIdx.x + s];
        }
        __syncthreads();
    }
    v = rf[0];
    c = rc[0];
}

// (pixel, channel) of element i of a load of npx pixels: channels run fastest for a channels-last map, pixels for any other
__device__ inline void load_order(bool channels_last, int i, int npx, int K, int& px, int& k)
{
    if (channels_last) {
        px = i / K;
        k = i - px * K;
    } else {
        k = i / npx;
        px = i - k * npx;
    }
}

// The kernel's argument, read where it is used: every phase of the kernel takes the fields it needs from the kernel-argument segment
// again (scalar loads the compiler cannot move across the `asm`), so that the ~60 scalar registers of the argument and the loop
// invariants derived from them are not all live across the whole tile loop - kept live they spill.
// (The explicit arguments of a kernel start at offset 0 of its kernel-argument segment, hidden arguments follow them: AMDGPU code
// object ABI.  Every GPU parity test reads all fields this way; tests/test_probe_train_resources.py pins the 0 spills it buys.)
typedef const TrainParams __attribute__((address_space(4))) * KernArg;
// The probes' parameters are not written while the kernel runs: read through the constant address space, a wave-uniform row is
// fetched with scalar loads (through a plain pointer taken from the re-read argument the compiler issues one vector load per element).
typedef const float __attribute__((address_space(4))) * ConstRow;
__device__ inline KernArg kernarg()
{
    KernArg a = (KernArg)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return a;
}
__device__ inline StegoMap code_map(KernArg a)
{
    return StegoMap{a->code.data, a->code.stride_n, a->code.stride_c, a->code.stride_h, a->code.stride_w};
}

// The workgroup's dynamic LDS, carved from the plan in the kernel argument (recomputed per phase like the argument itself)
struct Lds {
    float *red, *cs, *ps, *gs, *wy, *wx, *small;     // small [NMAX]: the label mask (linear) / max(|cluster row|, eps) (cluster)
    int *ylo, *yhi, *xlo, *xhi;
};
template <int NMAX>
__device__ inline Lds carve(KernArg a, bool cluster = false)
{
    extern __shared__ float4 smem4[];
    Lds L;
    L.red = reinterpret_cast<float*>(smem4);
    L.cs = L.red + RED_FLOATS;
    if (cluster) {                               // a chunk's code and cosines, then `small`; nothing else is used
        L.ps = L.cs + CP * a->KS;
        L.gs = L.wy = L.wx = nullptr;
        L.small = L.ps + CP * a->NPS;
        L.ylo = L.yhi = L.xlo = L.xhi = nullptr;
        return L;
    }
    const int cap = a->max_nr * a->max_nc;
    L.ps = L.cs + cap * a->KS;
    L.gs = L.ps + cap * a->NPS;
    L.wy = L.gs + a->TY * a->TX * a->NG;
    L.wx = L.wy + a->max_nr * a->TY;
    L.small = L.wx + a->max_nc * a->TX;
    L.ylo = reinterpret_cast<int*>(L.small + NMAX);
    L.yhi = L.ylo + a->max_nr;
    L.xlo = L.yhi + a->max_nr;
    L.xhi = L.xlo + a->max_nc;
    return L;
}

template <int NMAX>
__global__ __launch_bounds__(TPB) void probe_train_kernel(TrainParams)
{
    using O = Own<NMAX>;
    const auto& p = *kernarg();
    const Lds L = carve<NMAX>(&p, (int)blockIdx.x < p.g_clu);
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    float acc[O::A][O::BM];
#pragma unroll
    for (int a = 0; a < O::A; ++a)
#pragma unroll
        for (int b = 0; b < O::BM; ++b) acc[a][b] = 0.f;
    float loss = 0.f;
    long long count = 0;

    if ((int)blockIdx.x >= p.g_clu) {            // (the cluster workgroups come first: short, they make room for the rest)
        const int wg = blockIdx.x - p.g_clu;
        // ---------------------------------------------------------------- the linear probe
        if (t < NMAX) L.small[t] = t < p.n_lin ? 0.f : -INFINITY;
        for (int64_t tile = wg; tile < kernarg()->n_tiles; tile += kernarg()->g_lin) {
            const auto& p = *kernarg();
            const Lds L = carve<NMAX>(&p);
            const int tiles_per_image = p.tiles_x * p.tiles_y;
            const int64_t b = tile / tiles_per_image;
            const int trem = (int)(tile - b * tiles_per_image);
            const int Y0 = (trem / p.tiles_x) * p.TY, X0 = (trem % p.tiles_x) * p.TX;
            const int Y1 = min(Y0 + p.TY, p.H), X1 = min(X0 + p.TX, p.W);
            const Footprint f = tile_footprint(Y0, Y1, X0, X1, p.scale_h, p.scale_w, p.h, p.w, p.max_nr, p.max_nc);
            const int ya = f.ya, xa = f.xa, nr = f.nr, nc = f.nc, npx = f.npx;
            long long lab = -1;                  // this thread's label pixel, asked for now and used in step 3
            if (t < p.TY * p.TX) {
                const int Y = Y0 + t / p.TX, X = X0 + t % p.TX;
                if (Y < Y1 && X < X1) lab = p.label[(b * p.H + Y) * (int64_t)p.W + X];
            }
            for (int f = t; f < nc + nr; f += TPB) {     // (ranges: last read in the previous tile's step 4, a barrier ago; a strongly
                (f < nc ? L.xlo : L.ylo)[f < nc ? f : f - nc] = INT32_MAX;   //  downsampled tile has more than 256 footprint columns)
                (f < nc ? L.xhi : L.yhi)[f < nc ? f : f - nc] = -1;
            }
            __syncthreads();                     // the previous tile's step 5 has read the code and G

            // 1. the footprint's code, a 1 in channel K, the weight matrices and the range of tile pixels that touch each footprint row /
            //    column (the mapping is monotone, so they are a range)
            {
                const auto& p = *kernarg();
                const Lds L = carve<NMAX>(&p);
                const StegoMap code = code_map(&p);
                for (int i0 = t; i0 < npx * p.K; i0 += LOADS * TPB) {       // LOADS global loads in flight per thread
                    float v[LOADS];
                    int at[LOADS];
#pragma unroll
                    for (int u = 0; u < LOADS; ++u) {
                        const int i = i0 + u * TPB;
                        at[u] = -1;
                        if (i < npx * p.K) {
                            int px, k;
                            load_order(code.stride_c == 1, i, npx, p.K, px, k);
                            at[u] = px * p.KS + k;
                            v[u] = load_code(code, b, k, ya + px / nc, xa + px % nc);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < LOADS; ++u)
                        if (at[u] >= 0) L.cs[at[u]] = v[u];
                }
                for (int px = t; px < npx; px += TPB) L.cs[px * p.KS + p.K] = 1.f;
            }
            for (int i = t; i < nc * p.TX; i += TPB) {
                const int c = i / p.TX, xx = i - c * p.TX;
                float v = 0.f;
                if (X0 + xx < X1) {
                    int x0, x1;
                    float w1;
                    src_index(X0 + xx, p.scale_w, p.w, x0, x1, w1);
                    const int c0 = max(min(x0 - xa, nc - 1), 0), c1 = max(min(x1 - xa, nc - 1), 0);
                    v = (c0 == c ? 1.f - w1 : 0.f) + (c1 == c ? w1 : 0.f);
                    if (c0 == c || c1 == c) {    // (integer min / max: the order does not matter)
                        atomicMin(&L.xlo[c], xx);
                        atomicMax(&L.xhi[c], xx);
                    }
                }
                L.wx[i] = v;
            }
            for (int i = t; i < nr * p.TY; i += TPB) {
                const int r = i / p.TY, yy = i - r * p.TY;
                float v = 0.f;
                if (Y0 + yy < Y1) {
                    int y0, y1;
                    float h1;
                    src_index(Y0 + yy, p.scale_h, p.h, y0, y1, h1);
                    const int r0 = max(min(y0 - ya, nr - 1), 0), r1 = max(min(y1 - ya, nr - 1), 0);
                    v = (r0 == r ? 1.f - h1 : 0.f) + (r1 == r ? h1 : 0.f);
                    if (r0 == r || r1 == r) {
                        atomicMin(&L.ylo[r], yy);
                        atomicMax(&L.yhi[r], yy);
                    }
                }
                L.wy[i] = v;
            }
            __syncthreads();

            // 2. projections of the footprint pixels, one wave per label slot (pad slots hold 0; the mask makes them -inf later)
            for (int j0 = wave * JB; j0 < NMAX; j0 += (TPB / 64) * JB) {
                const auto& p = *kernarg();
                const Lds L = carve<NMAX>(&p);
                ConstRow row[JB];
                float bias[JB];
#pragma unroll
                for (int u = 0; u < JB; ++u) {   // (a pad slot projects onto row 0 and is zeroed below)
                    row[u] = (ConstRow)p.lin_w + (size_t)(j0 + u < p.n_lin ? j0 + u : 0) * p.K;
                    bias[u] = ((ConstRow)p.lin_b)[j0 + u < p.n_lin ? j0 + u : 0];
                }
                for (int px = lane; px < npx; px += 64) {
                    const float* c = L.cs + px * p.KS;
                    float a[JB];
#pragma unroll
                    for (int u = 0; u < JB; ++u) a[u] = 0.f;
                    for (int k = 0; k < p.K; ++k) {
                        const float cv = c[k];
#pragma unroll
                        for (int u = 0; u < JB; ++u) a[u] = fmaf(row[u][k], cv, a[u]);
                    }
#pragma unroll
                    for (int u = 0; u < JB; ++u) L.ps[px * p.NPS + j0 + u] = j0 + u < p.n_lin ? a[u] + bias[u] : 0.f;
                }
            }
            __syncthreads();

            // 3. one label pixel per thread: loss term and logit gradient
            if (t < kernarg()->TY * kernarg()->TX) {
                const auto& p = *kernarg();
                const Lds L = carve<NMAX>(&p);
                const int yy = t / p.TX, xx = t - yy * p.TX;
                const int Y = Y0 + yy, X = X0 + xx;
                float* g = L.gs + t * p.NG;
                if (lab >= 0 && lab < p.n_lin) {
                    int y0, y1, x0, x1;
                    float h1, w1;
                    src_index(Y, p.scale_h, p.h, y0, y1, h1);
                    src_index(X, p.scale_w, p.w, x0, x1, w1);
                    const float h0 = 1.f - h1, w0 = 1.f - w1;
                    const int r0 = max(min(y0 - ya, nr - 1), 0), r1 = max(min(y1 - ya, nr - 1), 0);
                    const int c0 = max(min(x0 - xa, nc - 1), 0), c1 = max(min(x1 - xa, nc - 1), 0);
                    const float* q00 = L.ps + (r0 * nc + c0) * p.NPS;
                    const float* q01 = L.ps + (r0 * nc + c1) * p.NPS;
                    const float* q10 = L.ps + (r1 * nc + c0) * p.NPS;
                    const float* q11 = L.ps + (r1 * nc + c1) * p.NPS;
                    float l[NMAX];
#pragma unroll
                    for (int j = 0; j < NMAX; ++j)
                        l[j] = (h0 * (w0 * q00[j] + w1 * q01[j]) + h1 * (w0 * q10[j] + w1 * q11[j])) + L.small[j];
                    float m = l[0];
#pragma unroll
                    for (int j = 1; j < NMAX; ++j) m = fmaxf(m, l[j]);
                    // (the label's logit from LDS again, the same expression: selecting it from l[] would keep NMAX lane masks live)
                    const int jl = (int)lab;
                    const float at_label = h0 * (w0 * q00[jl] + w1 * q01[jl]) + h1 * (w0 * q10[jl] + w1 * q11[jl]);
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < NMAX; ++j) {
                        l[j] = expf(l[j] - m);
                        s += l[j];
                    }
                    loss += (m + logf(s)) - at_label;
                    count += 1;
                    const float inv = 1.f / s;
#pragma unroll
                    for (int j = 0; j < NMAX; ++j) g[j] = l[j] * inv - (j == (int)lab ? 1.f : 0.f);
                } else {
#pragma unroll
                    for (int j = 0; j < NMAX; ++j) g[j] = 0.f;
                }
            }
            __syncthreads();

            // 4. G[footprint pixel][label] = sum over the tile pixels that touch it of wy * wx * g, into the projections' place
            for (int i = t; i < npx * (NMAX / JB); i += TPB) {
                const auto& p = *kernarg();
                const Lds L = carve<NMAX>(&p);
                const int j0 = (i % (NMAX / JB)) * JB, q = i / (NMAX / JB);
                const int r = q / nc, c = q - r * nc;
                const int x_lo = L.xlo[c], x_hi = L.xhi[c];
                float s[JB];
#pragma unroll
                for (int u = 0; u < JB; ++u) s[u] = 0.f;
                for (int yy = L.ylo[r]; yy <= L.yhi[r]; ++yy) {
                    float rs[JB];
#pragma unroll
                    for (int u = 0; u < JB; ++u) rs[u] = 0.f;
                    for (int xx = x_lo; xx <= x_hi; ++xx) {
                        const float wv = L.wx[c * p.TX + xx];
                        const float* g = L.gs + (yy * p.TX + xx) * p.NG + j0;
#pragma unroll
                        for (int u = 0; u < JB; ++u) rs[u] = fmaf(wv, g[u], rs[u]);
                    }
                    const float wv = L.wy[r * p.TY + yy];
#pragma unroll
                    for (int u = 0; u < JB; ++u) s[u] = fmaf(wv, rs[u], s[u]);
                }
#pragma unroll
                for (int u = 0; u < JB; ++u) L.ps[q * p.NPS + j0 + u] = s[u];
            }
            __syncthreads();

            // 5. the parameter gradient's share of this tile
            accumulate<NMAX>(acc, L.ps, L.cs, npx, kernarg()->K + 1, kernarg()->NPS, kernarg()->KS);
        }
        block_sum(loss, count, L.red);
        const auto& p = *kernarg();
        if (t == 0) {
            p.loss_lin[wg] = loss;
            p.cnt_lin[wg] = count;
        }
        write_partial<NMAX>(acc, p.part_lin + (size_t)wg * p.n_lin * (p.K + 1), p.n_lin, p.K + 1);
        return;
    }

    // -------------------------------------------------------------------- the cluster probe
    const int wg = blockIdx.x;
    for (int j = wave; j < p.n_clu; j += TPB / 64) {         // max(|cluster row|, eps), one wave per row
        float s = 0.f;
        for (int k = lane; k < p.K; k += 64) {
            const float v = p.clusters[(size_t)j * p.K + k];
            s = fmaf(v, v, s);
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) L.small[j] = fmaxf(sqrtf(s), 1e-12f);
    }
    const int64_t hw = (int64_t)p.h * p.w;
    for (int64_t chunk = wg; chunk < kernarg()->n_chunks; chunk += kernarg()->g_clu) {
        const auto& p = *kernarg();
        const Lds L = carve<NMAX>(&p, true);
        const StegoMap code = code_map(&p);
        const int64_t p0 = chunk * CP;
        __syncthreads();                         // the previous chunk's accumulation has read the code and the cosines (and `small` is written)
        for (int i0 = t; i0 < CP * p.K; i0 += LOADS * TPB) {
            float v[LOADS];
            int at[LOADS];
#pragma unroll
            for (int u = 0; u < LOADS; ++u) {
                const int i = i0 + u * TPB;
                at[u] = -1;
                if (i < CP * p.K) {
                    int px, k;
                    load_order(code.stride_c == 1, i, CP, p.K, px, k);
                    at[u] = px * p.KS + k;
                    v[u] = 0.f;
                    if (p0 + px < p.P) {
                        const int64_t b = (p0 + px) / hw;
                        const unsigned rem = (unsigned)((p0 + px) - b * hw);       // h w < 2^32
                        v[u] = load_code(code, b, k, (int)(rem / (unsigned)p.w), (int)(rem % (unsigned)p.w));
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < LOADS; ++u)
                if (at[u] >= 0) L.cs[at[u]] = v[u];
        }
        __syncthreads();
        {   // F.normalize in place: four threads per pixel, each the channels k = part (mod 4)
            const int px = t >> 2, part = t & 3;
            float* c = L.cs + px * p.KS;
            float s = 0.f;
            for (int k = part; k < p.K; k += 4) s = fmaf(c[k], c[k], s);
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            const float den = fmaxf(sqrtf(s), 1e-12f);
            for (int k = part; k < p.K; k += 4) c[k] = c[k] / den;
        }
        __syncthreads();
        for (int j = wave; j < p.n_clu; j += TPB / 64) {     // cosines, one wave per cluster
            const ConstRow row = (ConstRow)p.clusters + (size_t)j * p.K;
            const float* c = L.cs + lane * p.KS;
            float a = 0.f;
            for (int k = 0; k < p.K; ++k) a = fmaf(row[k], c[k], a);
            L.ps[lane * p.NPS + j] = a / L.small[j];
        }
        __syncthreads();
        if (t < CP) {                            // the first maximum -> loss term and the one-hot "G"
            float* q = L.ps + t * p.NPS;
            int best = -1;
            if (p0 + t < p.P) {
                best = 0;
                float bv = q[0];
                for (int j = 1; j < p.n_clu; ++j) {
                    const float v = q[j];
                    best = v > bv ? j : best;
                    bv = v > bv ? v : bv;
                }
                loss += bv;
            }
            for (int j = 0; j < NMAX; ++j) q[j] = j == best ? 1.f : 0.f;
        }
        __syncthreads();
        accumulate<NMAX>(acc, L.ps, L.cs, CP, p.K, p.NPS, p.KS);
    }
    block_sum(loss, count, L.red);
    if (t == 0) p.loss_clu[wg] = loss;
    write_partial<NMAX>(acc, p.part_clu + (size_t)wg * p.n_clu * p.K, p.n_clu, p.K);
}

struct ReduceParams {
    const float* part_lin;
    const float* loss_lin;
    const long long* cnt_lin;
    const float* part_clu;
    const float* loss_clu;
    const float* clusters;
    float* losses;
    long long* n_valid;
    float* d_lin_w;
    float* d_lin_b;
    float* d_clusters;
    int32_t K, n_lin, n_clu, g_lin, g_clu;
    int64_t P;
};

__device__ inline double block_sum_f64(double v, double* red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// Element k of row `row` of the partials [g][n][kdim], summed over g in index order: the workgroup's threads split g into
// 256 / kdim contiguous slices, then the slices are added in order.  Valid in the threads t < kdim.
__device__ inline double row_sum(const float* part, int g, int n, int kdim, int row, double* red)
{
    const int t = threadIdx.x, S = TPB / kdim, s = t / kdim, k = t - s * kdim;
    double v = 0.0;
    if (s < S) {
#pragma unroll 8
        for (int i = (int)((int64_t)g * s / S), e = (int)((int64_t)g * (s + 1) / S); i < e; ++i)     // (unrolled: eight loads in flight)
            v += (double)part[((size_t)i * n + row) * kdim + k];
    }
    __syncthreads();
    red[t] = v;
    __syncthreads();
    v = 0.0;
    if (t < kdim)
        for (int i = 0; i < S; ++i) v += red[i * kdim + t];
    return v;
}

__global__ __launch_bounds__(TPB) void probe_train_reduce(ReduceParams p)
{
    __shared__ double red[TPB];
    const int t = threadIdx.x, blk = blockIdx.x;
    if (blk < p.n_lin + (p.n_lin ? 1 : 0)) {
        double c = 0.0;                          // counts below 2^53: exact in fp64
        for (int i = t; i < p.g_lin; i += TPB) c += (double)p.cnt_lin[i];
        const double nv = block_sum_f64(c, red);
        if (blk < p.n_lin) {
            const double v = row_sum(p.part_lin, p.g_lin, p.n_lin, p.K + 1, blk, red);
            const float o = nv > 0.0 ? (float)(v / nv) : 0.f;
            if (t < p.K)
                p.d_lin_w[(size_t)blk * p.K + t] = o;
            else if (t == p.K)
                p.d_lin_b[blk] = o;
            return;
        }
        double l = 0.0;                          // thread t adds the workgroups t, t + 256, ...; then the fixed tree
        for (int i = t; i < p.g_lin; i += TPB) l += (double)p.loss_lin[i];
        l = block_sum_f64(l, red);
        if (t == 0) {
            p.losses[0] = (float)(l / nv);       // 0 / 0 = NaN without a valid pixel, as F.cross_entropy
            *p.n_valid = (long long)nv;
        }
        return;
    }
    const int row = blk - p.n_lin - (p.n_lin ? 1 : 0);
    if (row < p.n_clu) {
        const double s = row_sum(p.part_clu, p.g_clu, p.n_clu, p.K, row, red);
        const double c = t < p.K ? (double)p.clusters[(size_t)row * p.K + t] : 0.0;
        const double cn = fmax(sqrt(block_sum_f64(c * c, red)), 1e-12);
        const double ch = c / cn, dch = t < p.K ? -s / (double)p.P : 0.0;
        const double dot = block_sum_f64(dch * ch, red);
        if (t < p.K) p.d_clusters[(size_t)row * p.K + t] = (float)((dch - dot * ch) / cn);
        return;
    }
    double l = 0.0;
    for (int i = t; i < p.g_clu; i += TPB) l += (double)p.loss_clu[i];
    l = block_sum_f64(l, red);
    if (t == 0) {
        p.losses[1] = (float)(-l / (double)p.P);
        if (!p.n_lin) *p.n_valid = 0;
    }
}

using stego::aligned;
using stego::hip_rc;

int check_desc(const StegoProbeTrainDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->n_lin == 0 && d->n_clu == 0) return STEGO_ERR_PTRAIN_PROBES;
    if (d->K < 1 || d->K > STEGO_PTRAIN_MAX_K || d->n_lin < 0 || d->n_lin > STEGO_PTRAIN_MAX_N || d->n_clu < 0 ||
        d->n_clu > STEGO_PTRAIN_MAX_N)
        return STEGO_ERR_PTRAIN_DIM;
    if (d->B < 1 || d->B > 65535 || d->h < 1 || d->h > STEGO_PTRAIN_MAX_CODE || d->w < 1 || d->w > STEGO_PTRAIN_MAX_CODE || d->H < 1 ||
        d->H > STEGO_PTRAIN_MAX_OUT || d->W < 1 || d->W > STEGO_PTRAIN_MAX_OUT)
        return STEGO_ERR_PTRAIN_SIZE;
    return STEGO_OK;
}

struct Plan {
    int TY, TX, max_nr, max_nc, KS, NMAX, NPS, NG, tiles_x, tiles_y, g_lin, g_clu;
    int64_t n_tiles, P, n_chunks;
    float scale_h, scale_w;
    size_t lds;
    size_t off_cnt, off_part_lin, off_loss_lin, off_part_clu, off_loss_clu, ws_bytes;   // the workspace's regions
};

Plan plan(const StegoProbeTrainDesc* d)
{
    Plan pl{};
    pl.scale_h = (float)d->h / (float)d->H;
    pl.scale_w = (float)d->w / (float)d->W;
    pl.KS = (d->K + 1) | 1;
    const int n = std::max(d->n_lin, d->n_clu);
    pl.NMAX = label_slots(n);
    pl.NPS = pl.NMAX + 4;
    pl.NG = pl.NMAX + 1;
    pl.TX = d->W < 64 ? d->W : 64;
    pl.TY = TPB / pl.TX;
    pl.TY = pl.TY < d->H ? pl.TY : d->H;
    if (d->n_lin) {
        for (;;) {
            pl.max_nr = max_span(d->H, d->h, pl.scale_h, pl.TY);
            pl.max_nc = max_span(d->W, d->w, pl.scale_w, pl.TX);
            const size_t foot = ((size_t)pl.max_nr * pl.max_nc * (pl.KS + pl.NPS) + (size_t)pl.max_nr * pl.TY + (size_t)pl.max_nc * pl.TX) * 4;
            if (foot <= FOOT_BUDGET || (pl.TY == 1 && pl.TX == 1)) break;
            if (pl.TY > 1)
                pl.TY = (pl.TY + 1) / 2;
            else
                pl.TX = (pl.TX + 1) / 2;
        }
        pl.tiles_x = (d->W + pl.TX - 1) / pl.TX;
        pl.tiles_y = (d->H + pl.TY - 1) / pl.TY;
        pl.n_tiles = (int64_t)d->B * pl.tiles_x * pl.tiles_y;
        pl.g_lin = (int)std::min<int64_t>(pl.n_tiles, MAX_LIN_WG);
    } else {
        pl.TY = pl.TX = pl.max_nr = pl.max_nc = 1;
    }
    pl.P = (int64_t)d->B * d->h * d->w;
    if (d->n_clu) {
        pl.n_chunks = (pl.P + CP - 1) / CP;
        pl.g_clu = (int)std::min<int64_t>(pl.n_chunks, MAX_CLU_WG);
    }
    const size_t lin_floats = d->n_lin ? (size_t)pl.max_nr * pl.max_nc * (pl.KS + pl.NPS) + (size_t)pl.TY * pl.TX * pl.NG +
                                             (size_t)pl.max_nr * pl.TY + (size_t)pl.max_nc * pl.TX + pl.NMAX + 2 * ((size_t)pl.max_nr + pl.max_nc)
                                       : 0;
    const size_t clu_floats = d->n_clu ? (size_t)CP * (pl.KS + pl.NPS) + pl.NMAX : 0;
    pl.lds = ((size_t)RED_FLOATS + std::max(lin_floats, clu_floats)) * 4;
    pl.lds = (pl.lds + 15) & ~(size_t)15;
    stego::WsLayout ws;                          // packed tight: the 8-byte counts come first, everything after them is 4-byte data
    pl.off_cnt = ws.take((size_t)pl.g_lin * 8, 1);
    pl.off_part_lin = ws.take((size_t)pl.g_lin * d->n_lin * (d->K + 1) * 4, 1);
    pl.off_loss_lin = ws.take((size_t)pl.g_lin * 4, 1);
    pl.off_part_clu = ws.take((size_t)pl.g_clu * d->n_clu * d->K * 4, 1);
    pl.off_loss_clu = ws.take((size_t)pl.g_clu * 4, 1);
    pl.ws_bytes = ws.total(8);
    return pl;
}

}  // namespace

extern "C" size_t stego_probe_train_workspace_bytes(const StegoProbeTrainDesc* desc)
{
    return check_desc(desc) == STEGO_OK ? plan(desc).ws_bytes : 0;
}

extern "C" size_t stego_probe_train_plan(const StegoProbeTrainDesc* desc, int32_t* workgroups)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    const Plan pl = plan(desc);
    if (workgroups) *workgroups = pl.g_lin + pl.g_clu;
    return pl.lds;
}

extern "C" int stego_probe_train(const StegoProbeTrainDesc* desc, const StegoMap* code, const int64_t* label, const float* lin_w,
                                 const float* lin_b, const float* clusters, float* losses, int64_t* n_valid, float* d_lin_w, float* d_lin_b,
                                 float* d_clusters, void* workspace, size_t workspace_bytes, stego_stream_t stream)
{
    int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    const bool lin = desc->n_lin > 0, clu = desc->n_clu > 0;
    if (!code || !code->data || !losses || !n_valid || !workspace) return STEGO_ERR_NULL;
    if ((lin && (!label || !lin_w || !lin_b || !d_lin_w || !d_lin_b)) || (clu && (!clusters || !d_clusters))) return STEGO_ERR_NULL;
    const Plan pl = plan(desc);
    if (workspace_bytes < pl.ws_bytes) return STEGO_ERR_WORKSPACE;
    if (!aligned(code->data, 4) || !aligned(losses, 4) || !aligned(n_valid, 8) || !aligned(workspace, 8)) return STEGO_ERR_ALIGN;
    if (lin && (!aligned(label, 8) || !aligned(lin_w, 4) || !aligned(lin_b, 4) || !aligned(d_lin_w, 4) || !aligned(d_lin_b, 4)))
        return STEGO_ERR_ALIGN;
    if (clu && (!aligned(clusters, 4) || !aligned(d_clusters, 4))) return STEGO_ERR_ALIGN;

    using stego::at;
    TrainParams p{};
    p.code = *code;
    p.label = label;
    p.lin_w = lin_w;
    p.lin_b = lin_b;
    p.clusters = clusters;
    p.cnt_lin = at<long long>(workspace, pl.off_cnt);
    p.part_lin = at<float>(workspace, pl.off_part_lin);
    p.loss_lin = at<float>(workspace, pl.off_loss_lin);
    p.part_clu = at<float>(workspace, pl.off_part_clu);
    p.loss_clu = at<float>(workspace, pl.off_loss_clu);
    p.K = desc->K;
    p.h = desc->h;
    p.w = desc->w;
    p.H = desc->H;
    p.W = desc->W;
    p.n_lin = desc->n_lin;
    p.n_clu = desc->n_clu;
    p.scale_h = pl.scale_h;
    p.scale_w = pl.scale_w;
    p.TY = pl.TY;
    p.TX = pl.TX;
    p.max_nr = pl.max_nr;
    p.max_nc = pl.max_nc;
    p.KS = pl.KS;
    p.NPS = pl.NPS;
    p.NG = pl.NG;
    p.tiles_x = pl.tiles_x;
    p.tiles_y = pl.tiles_y;
    p.g_lin = pl.g_lin;
    p.g_clu = pl.g_clu;
    p.n_tiles = pl.n_tiles;
    p.P = pl.P;
    p.n_chunks = pl.n_chunks;

    ReduceParams r{};
    r.part_lin = p.part_lin;
    r.loss_lin = p.loss_lin;
    r.cnt_lin = p.cnt_lin;
    r.part_clu = p.part_clu;
    r.loss_clu = p.loss_clu;
    r.clusters = clusters;
    r.losses = losses;
    r.n_valid = reinterpret_cast<long long*>(n_valid);
    r.d_lin_w = d_lin_w;
    r.d_lin_b = d_lin_b;
    r.d_clusters = d_clusters;
    r.K = desc->K;
    r.n_lin = desc->n_lin;
    r.n_clu = desc->n_clu;
    r.g_lin = pl.g_lin;
    r.g_clu = pl.g_clu;
    r.P = pl.P;

    const hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)(pl.g_lin + pl.g_clu);
    const hipError_t e = stego::with_const<8, 16, 32, 64>(pl.NMAX, [&](auto N) { return stego::launch_first<probe_train_kernel<N()>>(grid, TPB, pl.lds, s, p); });
    if (e != hipSuccess) return hip_rc(e);
    // rows of the linear probe, its loss, rows of the cluster probe, its loss
    const unsigned rgrid = (unsigned)(desc->n_lin + (lin ? 1 : 0) + desc->n_clu + (clu ? 1 : 0));
    return hip_rc(stego::launch_next<probe_train_reduce>(rgrid, TPB, 0, s, r));
}
