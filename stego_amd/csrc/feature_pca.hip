// Feature pictures (include/stego_pca.h): the three-principal-component false colouring of a [B, C, h, w] map.
//
//   mean_partial / mean_final   (a) fp64 channel sums per slab of tokens, a wave per token and a lane per channel (the channels-last
//                               view is read in whole rows); the slabs are added in slab order.
//   gram / gram_final           (b) a workgroup owns a 64 x 64 block (I <= J) of the centred second moments over one slab of tokens: 64
//                               tokens x 64 channels of each side staged through LDS with the mean subtracted, each wave one 32 x 32
//                               tile on the fp32-input 32x32x2 matrix instruction (tiles under the diagonal are skipped), the fp32
//                               accumulator folded into fp64 every 1024 tokens.  gram_final adds the slabs' tiles in slab order,
//                               divides by n - 1 and writes both halves of cov.
//   eigen                       (c) one workgroup per group, fp64: a thread owns up to three rows of Q (8 columns) in registers; cov is
//                               read by rows of its symmetric half so that the threads' loads are consecutive, Q broadcast from LDS.
//   scores / score_range        (d) a wave per token (channels-last) or a thread per token (any other strides), mean and basis in LDS.
//   paint                       (e) stego_render's target and row packing (rgb_rows.h): 16 rows x 768 bytes per workgroup.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/stego_pca.h"
#include "addon_device.h"
#include "host_util.h"
#include "rgb_rows.h"

using namespace stego;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAX_C = STEGO_PCA_MAX_C;
constexpr int LANE_CH = MAX_C / 64;      // channels of a lane of the mean kernel
constexpr int MEAN_TOKENS = 256;         // tokens of a mean slab at the least
constexpr int MEAN_SLABS = 256;          // ... and mean slabs of all groups together, beyond one per group
constexpr int GRAM_SLABS = 16;           // second-moment slabs of all groups together, beyond one per group
constexpr int GB = 64;                   // channels of a block side
constexpr int GT = 64;                   // tokens of a stage
constexpr int GS = GB + 4;               // floats of a staged token row
constexpr int EC = 8;                    // columns of the subspace iteration
constexpr int RPT = MAX_C / TPB;         // rows of Q per thread
constexpr int RANGE_MAX_WG = 1024;       // workgroups per image of the scores launch at the most ...
constexpr int RANGE_ALL_WG = 8192;       // ... and of all images together, beyond one per image

struct FitParams {
    StegoMap map;
    float* mean;
    double* cov;
    float* basis;
    float* stats;
    double* msum;                        // [G][MS][C]
    double* tiles;                       // [G][S][ntiles][32 * 32]
    int64_t n, mslab, slab;              // tokens of a group, of a mean slab, of a second-moment slab
    int B, C, h, w, T, G, joint, MS, S, nt, nb, ntiles, n_iter, chan_major;
};

struct ScoreParams {
    StegoMap map;
    const float* mean;
    const float* basis;
    float* scores;
    float* partial;                      // [B][nwg][3][2]
    float* range;
    int B, C, h, w, T, G, joint, nwg, chunk, chan_major;
};

struct PaintParams {
    const float* scores;
    const float* range;
    uint8_t* out;
    int64_t osn, osh;
    int B, h, w, H, W, joint, nearest, rescale;
    float scale_h, scale_w;
};

// element offset of token tg of group g (channel 0)
__device__ __forceinline__ int64_t token_offset(const StegoMap& m, int joint, int g, int64_t tg, int T, int w)
{
    const int b = joint ? (int)(tg / T) : g;
    const int pix = (int)(tg - (joint ? (int64_t)b * T : 0));
    const int y = pix / w, x = pix - y * w;
    return (int64_t)b * m.stride_n + (int64_t)y * m.stride_h + (int64_t)x * m.stride_w;
}

// ---- (a)
__global__ __launch_bounds__(TPB) void mean_partial_kernel(const FitParams p)
{
    __shared__ double red[WAVES * MAX_C];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int s = blockIdx.x, g = blockIdx.y;
    const int64_t t0 = (int64_t)s * p.mslab, t1 = t0 + p.mslab < p.n ? t0 + p.mslab : p.n;
    double acc[LANE_CH];
#pragma unroll
    for (int i = 0; i < LANE_CH; ++i) acc[i] = 0.0;
    for (int64_t tk = t0 + wave; tk < t1; tk += WAVES) {
        const float* src = p.map.data + token_offset(p.map, p.joint, g, tk, p.T, p.w);
        float v[LANE_CH];
#pragma unroll
        for (int i = 0; i < LANE_CH; ++i) {
            const int c = lane + 64 * i;
            v[i] = c < p.C ? src[(int64_t)c * p.map.stride_c] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < LANE_CH; ++i) acc[i] += (double)v[i];
    }
#pragma unroll
    for (int i = 0; i < LANE_CH; ++i) red[wave * MAX_C + lane + 64 * i] = acc[i];
    __syncthreads();
    double* dst = p.msum + ((int64_t)g * p.MS + s) * p.C;
    for (int c = t; c < p.C; c += TPB) dst[c] = ((red[c] + red[MAX_C + c]) + red[2 * MAX_C + c]) + red[3 * MAX_C + c];
}

__global__ __launch_bounds__(TPB) void mean_final_kernel(const FitParams p)
{
    const int g = blockIdx.y, c = blockIdx.x * TPB + threadIdx.x;
    if (c >= p.C) return;
    const double* src = p.msum + (int64_t)g * p.MS * p.C + c;
    double sum = 0.0;
    for (int s = 0; s < p.MS; ++s) sum += src[(int64_t)s * p.C];
    p.mean[(int64_t)g * p.C + c] = (float)(sum / (double)p.n);
}

// ---- (b)
__device__ __forceinline__ int tile_id(int ti, int tj, int nt) { return ti * nt - ti * (ti - 1) / 2 + (tj - ti); }

__global__ __launch_bounds__(TPB) void gram_kernel(const FitParams p)
{
    __shared__ __attribute__((aligned(16))) float xs[2][GT * GS];
    __shared__ float ms[2][GB];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 31, hf = lane >> 5;
    int idx = blockIdx.x, I = 0;
    while (idx >= p.nb - I) {
        idx -= p.nb - I;
        ++I;
    }
    const int J = I + idx;
    const int s = blockIdx.y, g = blockIdx.z;
    const bool diag = I == J;
    const int sides = diag ? 1 : 2;
    if (t < 2 * GB) {
        const int c = ((t >> 6) ? J : I) * GB + lane;
        ms[t >> 6][lane] = c < p.C ? p.mean[(int64_t)g * p.C + c] : 0.f;
    }
    const int wi = wave >> 1, wj = wave & 1;
    const int ti = 2 * I + wi, tj = 2 * J + wj;
    const bool active = ti < p.nt && tj < p.nt && tj >= ti;
    const float* xa = xs[0] + hf * GS + wi * 32 + li;                   // A[i = channel li of tile ti][k = token 2 kk + hf]
    const float* xb = xs[diag ? 0 : 1] + hf * GS + wj * 32 + li;        // B[k = token 2 kk + hf][j = channel li of tile tj]
    f32x16 acc;
    double acc64[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc[r] = 0.f;
        acc64[r] = 0.0;
    }
    const int64_t t0 = (int64_t)s * p.slab, t1 = t0 + p.slab < p.n ? t0 + p.slab : p.n;
    int staged = 0;
    for (int64_t base = t0; base < t1; base += GT) {
        __syncthreads();                                                // the last stage is read (the first time: ms is written)
        for (int side = 0; side < sides; ++side) {
            const int cb = (side ? J : I) * GB;
            float* dst = xs[side];
            if (p.chan_major) {                                         // a lane per channel, a token per wave and step
                const int c = cb + lane;
                const bool in_c = c < p.C;
                const float m = ms[side][lane];
#pragma unroll 4
                for (int k = wave; k < GT; k += WAVES) {
                    const int64_t tk = base + k;
                    float v = 0.f;
                    if (in_c && tk < t1) v = p.map.data[token_offset(p.map, p.joint, g, tk, p.T, p.w) + (int64_t)c * p.map.stride_c] - m;
                    dst[k * GS + lane] = v;
                }
            } else {                                                    // a lane per token, a channel per wave and step
                const int64_t tk = base + lane;
                const bool in_t = tk < t1;
                const int64_t off = in_t ? token_offset(p.map, p.joint, g, tk, p.T, p.w) : 0;
#pragma unroll 4
                for (int cc = wave; cc < GB; cc += WAVES) {
                    const int c = cb + cc;
                    float v = 0.f;
                    if (in_t && c < p.C) v = p.map.data[off + (int64_t)c * p.map.stride_c] - ms[side][cc];
                    dst[lane * GS + cc] = v;
                }
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int kk = 0; kk < GT / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * kk * GS], xb[2 * kk * GS], acc, 0, 0, 0);
        }
        staged += GT;
        if (staged == STEGO_PCA_FOLD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc64[r] += (double)acc[r];
                acc[r] = 0.f;
            }
            staged = 0;
        }
    }
    if (!active) return;
    double* dst = p.tiles + ((((int64_t)g * p.S + s) * p.ntiles + tile_id(ti, tj, p.nt)) << 10);
#pragma unroll
    for (int r = 0; r < 16; ++r) dst[acc_row(r, hf) * 32 + li] = acc64[r] + (double)acc[r];
}

__global__ __launch_bounds__(TPB) void gram_final_kernel(const FitParams p)
{
    int idx = blockIdx.x, ti = 0;
    while (idx >= p.nt - ti) {
        idx -= p.nt - ti;
        ++ti;
    }
    const int tj = ti + idx, g = blockIdx.y;
    const double* src = p.tiles + (((int64_t)g * p.S * p.ntiles + blockIdx.x) << 10);
    double* cov = p.cov + (int64_t)g * p.C * p.C;
    const double inv = 1.0 / (double)(p.n - 1);
    for (int e = threadIdx.x; e < 1024; e += TPB) {
        const int row = e >> 5, col = e & 31;
        const int ci = ti * 32 + row, cj = tj * 32 + col;
        if (ci >= p.C || cj >= p.C || (ti == tj && row > col)) continue;
        double sum = 0.0;
        for (int s = 0; s < p.S; ++s) sum += src[((int64_t)s * p.ntiles << 10) + e];
        sum *= inv;
        cov[(int64_t)ci * p.C + cj] = sum;
        cov[(int64_t)cj * p.C + ci] = sum;
    }
}

// ---- (c)
// the sums of 8 values per thread over the workgroup, in one fixed tree: valid in every thread
__device__ __forceinline__ void block_sum8(double (&v)[EC], double* red)
{
#pragma unroll
    for (int j = 0; j < EC; ++j)
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) v[j] += __shfl_xor(v[j], m);
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                                    // the last sums are read
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < EC; ++j) red[wave * EC + j] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < EC; ++j) v[j] = ((red[j] + red[EC + j]) + red[2 * EC + j]) + red[3 * EC + j];
}

// z = cov Q for the thread's rows: cov[k][row] stands for cov[row][k], so the threads of a wave read consecutive doubles
__device__ __forceinline__ void cov_times_q(const double* A, const double* Q, int C, double (&z)[RPT][EC])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < RPT; ++i)
#pragma unroll
        for (int j = 0; j < EC; ++j) z[i][j] = 0.0;
    // KB rows of cov in flight per thread before the first is used: one compute unit reads the whole matrix, and what it gets is its
    // loads in flight over the latency
    constexpr int KB = 16;
    int k = 0;
    for (; k + KB <= C; k += KB) {
        double a[KB][RPT];
#pragma unroll
        for (int u = 0; u < KB; ++u)
#pragma unroll
            for (int i = 0; i < RPT; ++i) a[u][i] = t + TPB * i < C ? A[(int64_t)(k + u) * C + t + TPB * i] : 0.0;
#pragma unroll
        for (int u = 0; u < KB; ++u)
#pragma unroll
            for (int j = 0; j < EC; ++j) {
                const double q = Q[(k + u) * EC + j];
#pragma unroll
                for (int i = 0; i < RPT; ++i) z[i][j] = fma(a[u][i], q, z[i][j]);
            }
    }
    for (; k < C; ++k) {
        double a[RPT];
#pragma unroll
        for (int i = 0; i < RPT; ++i) a[i] = t + TPB * i < C ? A[(int64_t)k * C + t + TPB * i] : 0.0;
#pragma unroll
        for (int j = 0; j < EC; ++j) {
            const double q = Q[k * EC + j];
#pragma unroll
            for (int i = 0; i < RPT; ++i) z[i][j] = fma(a[i], q, z[i][j]);
        }
    }
}

// One pass of modified Gram-Schmidt over the columns, row-oriented: column c is measured against itself and every later column in
// one sum, the later columns lose their share of it, and it is scaled to length 1.  A column whose squared length fell below 1e-24
// of what it was before the pass depends on the columns in front of it: it becomes a zero column (and stays one).
__device__ __forceinline__ void mgs_pass(double (&z)[RPT][EC], double* red)
{
    double n0[EC];
#pragma unroll
    for (int j = 0; j < EC; ++j) {
        n0[j] = 0.0;
#pragma unroll
        for (int i = 0; i < RPT; ++i) n0[j] = fma(z[i][j], z[i][j], n0[j]);
    }
    block_sum8(n0, red);
#pragma unroll
    for (int c = 0; c < EC; ++c) {
        double d[EC];
#pragma unroll
        for (int j = 0; j < EC; ++j) {
            d[j] = 0.0;
            if (j >= c)
#pragma unroll
                for (int i = 0; i < RPT; ++i) d[j] = fma(z[i][c], z[i][j], d[j]);
        }
        block_sum8(d, red);
        const double rcc = d[c];
        if (!(rcc > 1e-24 * n0[c])) {
#pragma unroll
            for (int i = 0; i < RPT; ++i) z[i][c] = 0.0;
        } else {
            const double inv = 1.0 / rcc, sc = 1.0 / sqrt(rcc);
#pragma unroll
            for (int j = 0; j < EC; ++j)
                if (j > c) {
                    const double f = d[j] * inv;
#pragma unroll
                    for (int i = 0; i < RPT; ++i) z[i][j] = fma(-f, z[i][c], z[i][j]);
                }
#pragma unroll
            for (int i = 0; i < RPT; ++i) z[i][c] *= sc;
        }
    }
}

__device__ __forceinline__ void store_rows(double* Q, int C, const double (&z)[RPT][EC])
{
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = threadIdx.x + TPB * i;
        if (r < C)
#pragma unroll
            for (int j = 0; j < EC; ++j) Q[r * EC + j] = z[i][j];
    }
}

// the start of the iteration: an integer hash of (channel, column) in [-0.5, 0.5)
__device__ __forceinline__ double start_value(int c, int j)
{
    uint32_t u = (uint32_t)c * 0x9E3779B1u + (uint32_t)(j + 1) * 0x85EBCA77u;
    u ^= u >> 15;
    u *= 0x2C1B3C6Du;
    u ^= u >> 12;
    return (double)(u >> 8) * (1.0 / 16777216.0) - 0.5;
}

// cyclic Jacobi on the symmetric 8 x 8 matrix T (one thread): T's diagonal becomes the eigenvalues, V's columns the eigenvectors
__device__ void jacobi8(double* T, double* V)
{
    for (int i = 0; i < EC * EC; ++i) V[i] = (i / EC == i % EC) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int a = 0; a < EC; ++a) {
            dia += T[a * EC + a] * T[a * EC + a];
            for (int b = a + 1; b < EC; ++b) off += T[a * EC + b] * T[a * EC + b];
        }
        if (!(off > 1e-40 * dia)) break;
        for (int a = 0; a < EC - 1; ++a)
            for (int b = a + 1; b < EC; ++b) {
                const double apq = T[a * EC + b];
                if (apq == 0.0) continue;
                const double theta = (T[b * EC + b] - T[a * EC + a]) / (2.0 * apq);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < EC; ++k) {
                    const double kp = T[k * EC + a], kq = T[k * EC + b];
                    T[k * EC + a] = c * kp - s * kq;
                    T[k * EC + b] = s * kp + c * kq;
                }
                for (int k = 0; k < EC; ++k) {
                    const double pk = T[a * EC + k], qk = T[b * EC + k];
                    T[a * EC + k] = c * pk - s * qk;
                    T[b * EC + k] = s * pk + c * qk;
                }
                for (int k = 0; k < EC; ++k) {
                    const double kp = V[k * EC + a], kq = V[k * EC + b];
                    V[k * EC + a] = c * kp - s * kq;
                    V[k * EC + b] = s * kp + c * kq;
                }
            }
    }
}

__global__ __launch_bounds__(TPB) void eigen_kernel(const FitParams p)
{
    __shared__ double Q[MAX_C * EC];
    __shared__ double red[WAVES * EC];
    __shared__ double Tm[EC * EC], Vm[EC * EC];
    __shared__ double bestv[TPB];
    __shared__ int besti[TPB];
    __shared__ int order[3];
    const int t = threadIdx.x, g = blockIdx.x, C = p.C;
    const double* A = p.cov + (int64_t)g * C * C;
    const int ncol = C < EC ? C : EC;
    double z[RPT][EC];
#pragma unroll
    for (int i = 0; i < RPT; ++i)
#pragma unroll
        for (int j = 0; j < EC; ++j) z[i][j] = (t + TPB * i < C && j < ncol) ? start_value(t + TPB * i, j) : 0.0;
    store_rows(Q, C, z);
    __syncthreads();
    for (int it = 0; it < p.n_iter; ++it) {
        cov_times_q(A, Q, C, z);
        mgs_pass(z, red);               // (its first barrier is behind every thread's last read of Q)
        mgs_pass(z, red);
        store_rows(Q, C, z);
        __syncthreads();
    }
    // Rayleigh-Ritz: T = Q^T (cov Q)
    cov_times_q(A, Q, C, z);
#pragma unroll
    for (int a = 0; a < EC; ++a) {
        double d[EC];
#pragma unroll
        for (int j = 0; j < EC; ++j) {
            d[j] = 0.0;
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const int r = t + TPB * i;
                if (r < C) d[j] = fma(Q[r * EC + a], z[i][j], d[j]);
            }
        }
        block_sum8(d, red);
        if (t == 0)
#pragma unroll
            for (int j = 0; j < EC; ++j) Tm[a * EC + j] = d[j];
    }
    __syncthreads();
    if (t == 0) {
        for (int a = 0; a < EC; ++a)
            for (int b = a + 1; b < EC; ++b) Tm[a * EC + b] = Tm[b * EC + a] = 0.5 * (Tm[a * EC + b] + Tm[b * EC + a]);
        jacobi8(Tm, Vm);
        unsigned used = 0;
        for (int k = 0; k < 3; ++k) {                                   // descending, ties to the lower column
            int best = -1;
            for (int a = 0; a < EC; ++a)
                if (!((used >> a) & 1u) && (best < 0 || Tm[a * EC + a] > Tm[best * EC + best])) best = a;
            used |= 1u << best;
            order[k] = best;
        }
    }
    __syncthreads();
    double lam[3];
    double v[RPT][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int o = order[k];
        lam[k] = Tm[o * EC + o];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int r = t + TPB * i;
            double sum = 0.0;
            if (r < C)
                for (int j = 0; j < EC; ++j) sum = fma(Q[r * EC + j], Vm[j * EC + o], sum);
            v[i][k] = sum;
        }
    }
    // the sign: the loading of largest magnitude is positive, ties to the lowest channel
    double sign[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double bv = -1.0;
        int bi = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int r = t + TPB * i;
            if (r < C && fabs(v[i][k]) > bv) {
                bv = fabs(v[i][k]);
                bi = r;
            }
        }
        __syncthreads();
        bestv[t] = bv;
        besti[t] = bi;
        __syncthreads();
        for (int m = TPB / 2; m > 0; m >>= 1) {
            if (t < m && (bestv[t + m] > bestv[t] || (bestv[t + m] == bestv[t] && besti[t + m] < besti[t]))) {
                bestv[t] = bestv[t + m];
                besti[t] = besti[t + m];
            }
            __syncthreads();
        }
        const int at = besti[0];
        double mine = 0.0;
#pragma unroll
        for (int i = 0; i < RPT; ++i)
            if (t + TPB * i == at) mine = v[i][k];
        __syncthreads();
        if (at % TPB == t) bestv[0] = mine;
        __syncthreads();
        sign[k] = bestv[0] < 0.0 ? -1.0 : 1.0;
    }
    // the residual |cov v - lambda v| and the trace: the components take the first three columns of Q
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = t + TPB * i;
        if (r < C)
#pragma unroll
            for (int k = 0; k < 3; ++k) Q[r * EC + k] = v[i][k];
    }
    __syncthreads();
    cov_times_q(A, Q, C, z);
    double d[EC];
#pragma unroll
    for (int j = 0; j < EC; ++j) d[j] = 0.0;
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const int r = t + TPB * i;
        if (r < C) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double e = z[i][k] - lam[k] * v[i][k];
                d[k] = fma(e, e, d[k]);
            }
            d[3] += A[(int64_t)r * C + r];
        }
    }
    block_sum8(d, red);
    const double trace = d[3];
    float* basis = p.basis + (int64_t)g * 3 * C;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool keep = lam[k] > trace * (1.0 / 1048576.0);
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int r = t + TPB * i;
            if (r < C) basis[(int64_t)k * C + r] = keep ? (float)(sign[k] * v[i][k]) : 0.f;
        }
        if (t == 0) {
            float* st = p.stats + (int64_t)g * 9 + 3 * k;
            st[0] = keep ? (float)lam[k] : 0.f;
            st[1] = keep ? (float)(lam[k] / trace) : 0.f;
            st[2] = keep ? (float)(sqrt(d[k]) / lam[0]) : 0.f;
        }
    }
}

// ---- (d)
__device__ __forceinline__ void fold_min_max(float (&lo)[3], float (&hi)[3], const float (&s)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        lo[i] = fminf(lo[i], s[i]);
        hi[i] = fmaxf(hi[i], s[i]);
    }
}

// the minimum and maximum of three (lo, hi) per thread over the workgroup, valid in thread 0
__device__ __forceinline__ void block_min_max3(float (&lo)[3], float (&hi)[3], float* red)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            lo[i] = fminf(lo[i], __shfl_xor(lo[i], m));
            hi[i] = fmaxf(hi[i], __shfl_xor(hi[i], m));
        }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            red[6 * wave + 2 * i] = lo[i];
            red[6 * wave + 2 * i + 1] = hi[i];
        }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int wv = 1; wv < WAVES; ++wv)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                lo[i] = fminf(lo[i], red[6 * wv + 2 * i]);
                hi[i] = fmaxf(hi[i], red[6 * wv + 2 * i + 1]);
            }
}

__global__ __launch_bounds__(TPB) void scores_kernel(const ScoreParams p)
{
    __shared__ float mb[4 * MAX_C];                                     // the group's mean and its three basis rows
    __shared__ float red[6 * WAVES];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int b = blockIdx.y, g = p.joint ? 0 : b, C = p.C;
    for (int c = t; c < C; c += TPB) {
        mb[c] = p.mean[(int64_t)g * C + c];
#pragma unroll
        for (int i = 0; i < 3; ++i) mb[(i + 1) * MAX_C + c] = p.basis[((int64_t)g * 3 + i) * C + c];
    }
    __syncthreads();
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    const float* img = p.map.data + (int64_t)b * p.map.stride_n;
    float* out = p.scores + (int64_t)b * p.T * 3;
    for (int base = blockIdx.x * p.chunk; base < p.T; base += p.nwg * p.chunk) {
        if (p.chan_major) {                                             // a wave per token, a lane per channel
            for (int k = wave; k < p.chunk; k += WAVES) {
                const int pix = base + k;
                if (pix >= p.T) break;
                const int y = pix / p.w, x = pix - y * p.w;
                const float* src = img + (int64_t)y * p.map.stride_h + (int64_t)x * p.map.stride_w;
                float s[3] = {0.f, 0.f, 0.f};
#pragma unroll 4
                for (int c = lane; c < C; c += 64) {
                    const float v = src[(int64_t)c * p.map.stride_c] - mb[c];
#pragma unroll
                    for (int i = 0; i < 3; ++i) s[i] = fmaf(v, mb[(i + 1) * MAX_C + c], s[i]);
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) s[i] = wave_sum(s[i]);
                if (lane < 3) out[(int64_t)pix * 3 + lane] = lane == 0 ? s[0] : lane == 1 ? s[1] : s[2];
                fold_min_max(lo, hi, s);
            }
        } else {                                                        // a thread per token
            const int pix = base + t;
            if (pix < p.T) {
                const int y = pix / p.w, x = pix - y * p.w;
                const float* src = img + (int64_t)y * p.map.stride_h + (int64_t)x * p.map.stride_w;
                float s[3] = {0.f, 0.f, 0.f};
#pragma unroll 4
                for (int c = 0; c < C; ++c) {
                    const float v = src[(int64_t)c * p.map.stride_c] - mb[c];
#pragma unroll
                    for (int i = 0; i < 3; ++i) s[i] = fmaf(v, mb[(i + 1) * MAX_C + c], s[i]);
                }
#pragma unroll
                for (int i = 0; i < 3; ++i) out[(int64_t)pix * 3 + i] = s[i];
                fold_min_max(lo, hi, s);
            }
        }
    }
    block_min_max3(lo, hi, red);
    if (t == 0) {
        float* dst = p.partial + 6 * ((int64_t)b * p.nwg + blockIdx.x);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dst[2 * i] = lo[i];
            dst[2 * i + 1] = hi[i];
        }
    }
}

__global__ __launch_bounds__(TPB) void score_range_kernel(const ScoreParams p)
{
    __shared__ float red[6 * WAVES];
    const int g = blockIdx.x;
    const int64_t count = (int64_t)(p.joint ? p.B : 1) * p.nwg;
    const float* src = p.partial + 6 * (int64_t)(p.joint ? 0 : g) * p.nwg;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = threadIdx.x; i < count; i += TPB)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], src[6 * i + 2 * k]);
            hi[k] = fmaxf(hi[k], src[6 * i + 2 * k + 1]);
        }
    block_min_max3(lo, hi, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            p.range[6 * g + 2 * k] = lo[k];
            p.range[6 * g + 2 * k + 1] = hi[k];
        }
}

// ---- (e)
// ATen's area_pixel_compute_source_index (align_corners=False) and upsample_bilinear2d's taps
__device__ __forceinline__ void src_taps(int dst, float scale, int in, int& i0, int& i1, float& l1)
{
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

__global__ __launch_bounds__(TPB) void paint_kernel(const PaintParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[ROWS * CHUNK];
    const int t = threadIdx.x;
    const int c = blockIdx.x, y0 = blockIdx.y * ROWS, b = blockIdx.z;
    float lo[3] = {0.f, 0.f, 0.f}, span[3] = {0.f, 0.f, 0.f};
    if (p.rescale) {
        const float* rg = p.range + 6 * (p.joint ? 0 : b);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            lo[i] = rg[2 * i];
            span[i] = rg[2 * i + 1] - lo[i];
        }
    }
    const float* sc = p.scores + (int64_t)b * p.h * p.w * 3;
    uint8_t* const out_b = p.out + (int64_t)b * p.osn;
    const int pix_x0 = c * CPIX - PIX_BACK;
    constexpr int N_PIX = ROWS * PIX_SPAN;
    for (int i = t; i < N_PIX; i += TPB) {
        const int r = i / PIX_SPAN, x = pix_x0 + (i - r * PIX_SPAN), y = y0 + r;
        if (y >= p.H || x < 0 || x >= p.W) continue;
        const int at = pixel_place(out_b + (int64_t)y * p.osh, x, c);
        if (at + 2 < 0 || at >= CHUNK) continue;
        float s[3];
        if (p.nearest) {
            const int ys = min((int)floorf((float)y * p.scale_h), p.h - 1), xs = min((int)floorf((float)x * p.scale_w), p.w - 1);
            const float* q = sc + ((int64_t)ys * p.w + xs) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = q[k];
        } else {
            int ya, yb, xa, xb;
            float ly, lx;
            src_taps(y, p.scale_h, p.h, ya, yb, ly);
            src_taps(x, p.scale_w, p.w, xa, xb, lx);
            const float wy0 = 1.f - ly, wx0 = 1.f - lx;
            const float* q00 = sc + ((int64_t)ya * p.w + xa) * 3;
            const float* q01 = sc + ((int64_t)ya * p.w + xb) * 3;
            const float* q10 = sc + ((int64_t)yb * p.w + xa) * 3;
            const float* q11 = sc + ((int64_t)yb * p.w + xb) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] = wy0 * (wx0 * q00[k] + lx * q01[k]) + ly * (wx0 * q10[k] + lx * q11[k]);
        }
        uint32_t px = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v;
            if (p.rescale)
                v = span[k] == 0.f ? 0.f : (s[k] - lo[k]) / span[k];
            else
                v = (s[k] + 1.f) / 2.f;
            px |= to_level(v) << (8 * k);
        }
        put_pixel(stage + r * CHUNK, at, px);
    }
    __syncthreads();
    store_rows<TPB>(out_b, p.osh, stage, c, y0, p.H, p.W);
}

// ---- host
int check_desc(const StegoPcaDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->C < 3 || d->C > STEGO_PCA_MAX_C) return STEGO_ERR_PCA_DIM;
    if (d->B < 1 || d->B > 65535 || d->h < 1 || d->h > STEGO_PCA_MAX_SIDE || d->w < 1 || d->w > STEGO_PCA_MAX_SIDE) return STEGO_ERR_PCA_SIZE;
    if ((int64_t)d->B * d->h * d->w > STEGO_PCA_MAX_TOKENS) return STEGO_ERR_PCA_SIZE;
    if (d->H < 1 || d->H > STEGO_STITCH_MAX_SIDE || d->W < 1 || d->W > STEGO_STITCH_MAX_SIDE) return STEGO_ERR_PCA_SIZE;
    if ((d->group != STEGO_PCA_PER_IMAGE && d->group != STEGO_PCA_JOINT) || (d->resize != STEGO_PCA_BILINEAR && d->resize != STEGO_PCA_NEAREST) ||
        (d->scale != STEGO_PCA_UNIT && d->scale != STEGO_PCA_RANGE))
        return STEGO_ERR_PCA_MODE;
    if ((int64_t)d->h * d->w * (d->group == STEGO_PCA_JOINT ? d->B : 1) < 4) return STEGO_ERR_PCA_SIZE;
    if (d->n_iter < 1 || d->n_iter > STEGO_PCA_MAX_ITER) return STEGO_ERR_PCA_ITER;
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
    int G, joint, T, MS, S, nt, nb, ntiles, score_wg_cm, score_wg_tm;
    int64_t n, mslab, slab;
    size_t msum, tiles, partial, total;
};

Plan plan(const StegoPcaDesc* d)
{
    Plan pl{};
    pl.joint = d->group == STEGO_PCA_JOINT;
    pl.G = pl.joint ? 1 : d->B;
    pl.T = d->h * d->w;
    pl.n = (int64_t)pl.T * (pl.joint ? d->B : 1);
    const int64_t ms_cap = MEAN_SLABS / pl.G > 1 ? MEAN_SLABS / pl.G : 1, ms = ceil_div(pl.n, MEAN_TOKENS);
    pl.mslab = ceil_div(pl.n, ms < ms_cap ? ms : ms_cap);
    pl.MS = (int)ceil_div(pl.n, pl.mslab);
    const int64_t s_cap = GRAM_SLABS / pl.G > 1 ? GRAM_SLABS / pl.G : 1, s = ceil_div(pl.n, STEGO_PCA_FOLD);
    pl.slab = ceil_div(ceil_div(pl.n, s < s_cap ? s : s_cap), STEGO_PCA_FOLD) * STEGO_PCA_FOLD;
    pl.S = (int)ceil_div(pl.n, pl.slab);
    pl.nt = (d->C + 31) / 32;
    pl.nb = (d->C + GB - 1) / GB;
    pl.ntiles = pl.nt * (pl.nt + 1) / 2;
    const int64_t cm = ceil_div(pl.T, 64), tm = ceil_div(pl.T, TPB);
    const int64_t wg_cap = RANGE_ALL_WG / d->B < 1 ? 1 : (RANGE_ALL_WG / d->B < RANGE_MAX_WG ? RANGE_ALL_WG / d->B : RANGE_MAX_WG);
    pl.score_wg_cm = (int)(cm < wg_cap ? cm : wg_cap);
    pl.score_wg_tm = (int)(tm < wg_cap ? tm : wg_cap);
    WsLayout ws;
    pl.msum = ws.take((size_t)pl.G * pl.MS * d->C * sizeof(double), 16);
    pl.tiles = ws.take(((size_t)pl.G * pl.S * pl.ntiles << 10) * sizeof(double), 16);
    const size_t fit = ws.total(16);
    WsLayout ws2;                                                       // stage (d) has the workspace to itself
    pl.partial = ws2.take((size_t)d->B * pl.score_wg_cm * 6 * sizeof(float), 16);
    const size_t sco = ws2.total(16);
    pl.total = fit > sco ? fit : sco;
    return pl;
}

}  // namespace

extern "C" size_t stego_pca_workspace_bytes(const StegoPcaDesc* desc)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    return plan(desc).total;
}

extern "C" int stego_pca_fit(const StegoPcaDesc* desc, const StegoMap* map, float* mean, double* cov, float* basis, float* stats,
                             void* workspace, size_t workspace_bytes, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!map || !map->data || !mean || !cov || !basis || !stats || !workspace) return STEGO_ERR_NULL;
    const Plan pl = plan(desc);
    if (workspace_bytes < pl.total) return STEGO_ERR_WORKSPACE;
    if (!aligned(map->data, 4) || !aligned(mean, 4) || !aligned(basis, 4) || !aligned(stats, 4) || !aligned(cov, 8) || !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;
    FitParams p{};
    p.map = *map;
    p.mean = mean;
    p.cov = cov;
    p.basis = basis;
    p.stats = stats;
    p.msum = at<double>(workspace, pl.msum);
    p.tiles = at<double>(workspace, pl.tiles);
    p.n = pl.n;
    p.mslab = pl.mslab;
    p.slab = pl.slab;
    p.B = desc->B;
    p.C = desc->C;
    p.h = desc->h;
    p.w = desc->w;
    p.T = pl.T;
    p.G = pl.G;
    p.joint = pl.joint;
    p.MS = pl.MS;
    p.S = pl.S;
    p.nt = pl.nt;
    p.nb = pl.nb;
    p.ntiles = pl.ntiles;
    p.n_iter = desc->n_iter;
    p.chan_major = channel_major(map);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned G = (unsigned)pl.G;
    hipError_t e = launch_first<mean_partial_kernel>(dim3((unsigned)pl.MS, G), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<mean_final_kernel>(dim3((unsigned)((p.C + TPB - 1) / TPB), G), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<gram_kernel>(dim3((unsigned)(pl.nb * (pl.nb + 1) / 2), (unsigned)pl.S, G), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<gram_final_kernel>(dim3((unsigned)pl.ntiles, G), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<eigen_kernel>(dim3(G), TPB, 0, s, p);
    return hip_rc(e);
}

extern "C" int stego_pca_scores(const StegoPcaDesc* desc, const StegoMap* map, const float* mean, const float* basis, float* scores,
                                float* range, void* workspace, size_t workspace_bytes, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!map || !map->data || !mean || !basis || !scores || !range || !workspace) return STEGO_ERR_NULL;
    const Plan pl = plan(desc);
    if (workspace_bytes < pl.total) return STEGO_ERR_WORKSPACE;
    if (!aligned(map->data, 4) || !aligned(mean, 4) || !aligned(basis, 4) || !aligned(scores, 4) || !aligned(range, 4) || !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;
    ScoreParams p{};
    p.map = *map;
    p.mean = mean;
    p.basis = basis;
    p.scores = scores;
    p.partial = at<float>(workspace, pl.partial);
    p.range = range;
    p.B = desc->B;
    p.C = desc->C;
    p.h = desc->h;
    p.w = desc->w;
    p.T = pl.T;
    p.G = pl.G;
    p.joint = pl.joint;
    p.chan_major = channel_major(map);
    p.nwg = p.chan_major ? pl.score_wg_cm : pl.score_wg_tm;
    p.chunk = p.chan_major ? 64 : TPB;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_first<scores_kernel>(dim3((unsigned)p.nwg, (unsigned)p.B), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<score_range_kernel>(dim3((unsigned)pl.G), TPB, 0, s, p);
    return hip_rc(e);
}

extern "C" int stego_pca_paint(const StegoPcaDesc* desc, const float* scores, const float* range, uint8_t* out, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    const bool rescale = desc->scale == STEGO_PCA_RANGE;
    if (!scores || !out || (rescale && !range)) return STEGO_ERR_NULL;
    if (!aligned(scores, 4) || (rescale && !aligned(range, 4))) return STEGO_ERR_ALIGN;
    PaintParams p{};
    p.scores = scores;
    p.range = rescale ? range : nullptr;
    p.out = out;
    p.osn = desc->out_stride_n;
    p.osh = desc->out_stride_h;
    p.B = desc->B;
    p.h = desc->h;
    p.w = desc->w;
    p.H = desc->H;
    p.W = desc->W;
    p.joint = desc->group == STEGO_PCA_JOINT;
    p.nearest = desc->resize == STEGO_PCA_NEAREST;
    p.rescale = rescale;
    p.scale_h = (float)desc->h / (float)desc->H;
    p.scale_w = (float)desc->w / (float)desc->W;
    // a row's bytes start up to 15 bytes behind its aligned address: chunks of 3 W + 15 bytes at the most
    const dim3 grid((unsigned)((3 * desc->W + 15 + CHUNK - 1) / CHUNK), (unsigned)((desc->H + ROWS - 1) / ROWS), (unsigned)desc->B);
    return hip_rc(launch_first<paint_kernel>(grid, TPB, 0, static_cast<hipStream_t>(stream), p));
}
