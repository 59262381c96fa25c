// Fused ContrastiveCRFLoss, forward and backward (include/stego_crf_loss.h), in three launches that write no [B, N, N] tensor.
//
// Launch 1, crf_prepare: one workgroup of 1024 threads per (image, 64 points), 16 lanes per point: the four-tap samples of the code
//   and the guidance and the normalisation.  Writes x^ [B, Np, KP] (Np = N rounded up to 128, KP = K rounded up to 32; the padding rows
//   and channels are zero, so no later launch checks a bound), 1 / max(|x|, eps) and the projection switch [B, Np, 2], and one record
//   (row, column, g[8]) per point [B, Np, 10].  With a gradient one more workgroup sorts the 4 N taps of the unsample by code cell
//   (bitonic sort of 64-bit keys cell << 16 | tap in LDS, at most 16 k keys = 128 KiB) and writes the keys and the taps' weights.
// Launch 2, crf_pairs<NT, BWD>: one workgroup of four waves per (image, 64 rows a).  It walks the columns b in stages of 128 rows of
//   x^ (and their records) in LDS; wave (rw, cw) owns rows 32 rw .. + 31 and the two 32-column tiles 2 cw, 2 cw + 1 of every stage:
//     T = x^_b x^_a^T on v_mfma_f32_32x32x2_f32, the stage's rows as the A operand from LDS, the wave's own rows as the B operand
//       from registers: the accumulator then has a on the lane and b in the 16 registers;
//     k in that layout (2 exponentials per element), the loss partial sum k T;
//     P_a += k x^_b on the same instruction: register r of the k tile is the A operand of k-step r (k is symmetric, so k^T = k), the
//       B operand is row b(r, lane half) of the stage - a permuted but consistent summation order, no transpose through LDS.
//   Epilogue: the two column halves' P are added through LDS (cw = 0 + cw = 1), then dx = (P - (P . x^) x^) / max(|x|, eps) scaled by
//   -2 / (B N^2) replaces P [B, Np, KP]; one fp64 loss partial per workgroup.  The full matrix is walked: the symmetry of k is not
//   used to skip the lower-triangle tiles.
// Launch 3, crf_finish: one workgroup per 16 code cells and image (beyond 2^18 such units the workgroups walk them with the grid's
//   stride, so the grid stays inside the launch limits at every size): 17 threads find the cells' ranges in the sorted keys, every wave
//   takes four cells and sums weight * dx over a cell's taps in sorted order, lanes over the channels; every element of d_code is
//   written.  One more workgroup adds the loss partials in a fixed order in fp64 and writes loss and per_image.
// No float atomics anywhere: repeat launches give the same bits.  Every offset into a map or the workspace is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/stego_crf_loss.h"
#include "addon_device.h"
#include "host_util.h"
#include "probe_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PREP_TPB = 1024, PREP_PTS = 64, PREP_LANES = 16;
constexpr int PAIR_TPB = 256, ROWS_WG = 64, CB = 128;     // pairs: rows a per workgroup, rows b per LDS stage
constexpr int PS = 10, GMAX = STEGO_CRFLOSS_MAX_G;         // floats per point record: row, column, g[8]
constexpr int FIN_TPB = 256, FIN_CELLS = 16, FIN_MAX_WG = 1 << 18;   // finish: a bounded grid walks the (image, 16 cells) units
constexpr float EPS = 1e-10f;

struct CrfParams {
    StegoMap code, guid, dcode;
    const int64_t* coords;
    float *xh, *nrm, *pt, *P, *tw;
    double* part;
    unsigned long long* keys;
    float *loss, *per_image;
    int32_t B, K, G, h, w, hg, wg, H, W, N, Np, KP, T4p, normalize, n_rowblk;
    float sh, sw, shg, swg;              // in / out of the two resizes
    float ia, ib, ig, w1, w2, shift;     // 1 / (2 alpha), 1 / (2 beta), 1 / (2 gamma)
    float gscale;                        // -2 / (B N^2)
};

__device__ inline int clampi(long long v, int hi) { return v < 0 ? 0 : v > hi ? hi : (int)v; }

__device__ inline float tap4(const StegoMap& m, int64_t b, int k, int y0, int y1, int x0, int x1, float ly, float lx)
{
    const float c00 = load_code(m, b, k, y0, x0), c01 = load_code(m, b, k, y0, x1);
    const float c10 = load_code(m, b, k, y1, x0), c11 = load_code(m, b, k, y1, x1);
    return (1.f - ly) * ((1.f - lx) * c00 + lx * c01) + ly * ((1.f - lx) * c10 + lx * c11);
}

__global__ __launch_bounds__(PREP_TPB) void crf_prepare(CrfParams p)
{
    extern __shared__ unsigned long long skeys[];
    const int t = threadIdx.x;
    const int n_prep = p.B * (p.Np / PREP_PTS);
    if ((int)blockIdx.x >= n_prep) {                    // the sort workgroup (launched only with a gradient)
        const int n4 = 4 * p.N;
        for (int i = t; i < p.T4p; i += PREP_TPB) {
            unsigned long long key = ~0ull;
            if (i < n4) {
                const int n = i >> 2;
                const int r = clampi(p.coords[n], p.H - 1), c = clampi(p.coords[p.N + n], p.W - 1);
                int y0, y1, x0, x1;
                float ly, lx;
                src_index(r, p.sh, p.h, y0, y1, ly);
                src_index(c, p.sw, p.w, x0, x1, lx);
                const int y = (i & 2) ? y1 : y0, x = (i & 1) ? x1 : x0;
                p.tw[i] = ((i & 2) ? ly : 1.f - ly) * ((i & 1) ? lx : 1.f - lx);
                key = ((unsigned long long)(y * p.w + x) << 16) | (unsigned)i;
            }
            skeys[i] = key;
        }
        __syncthreads();
        for (int k2 = 2; k2 <= p.T4p; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = t; i < p.T4p; i += PREP_TPB) {
                    const int o = i ^ j;
                    if (o > i) {
                        const unsigned long long a = skeys[i], b = skeys[o];
                        if ((a > b) == ((i & k2) == 0)) {
                            skeys[i] = b;
                            skeys[o] = a;
                        }
                    }
                }
                __syncthreads();
            }
        for (int i = t; i < p.T4p; i += PREP_TPB) p.keys[i] = skeys[i];
        return;
    }
    const int per_img = p.Np / PREP_PTS;
    const int b = blockIdx.x / per_img;
    const int n = (blockIdx.x - b * per_img) * PREP_PTS + t / PREP_LANES, s = t % PREP_LANES;
    const size_t row = (size_t)b * p.Np + n;
    float* xo = p.xh + row * p.KP;
    float* po = p.pt + row * PS;
    if (n >= p.N) {                                     // padding rows: zero vectors at point (0, 0) with zero guidance
        for (int k = s; k < p.KP; k += PREP_LANES) xo[k] = 0.f;
        if (s < PS) po[s] = 0.f;
        if (s < 2) p.nrm[row * 2 + s] = 0.f;
        return;
    }
    const int r = clampi(p.coords[n], p.H - 1), c = clampi(p.coords[p.N + n], p.W - 1);
    int y0, y1, x0, x1;
    float ly, lx;
    src_index(r, p.sh, p.h, y0, y1, ly);
    src_index(c, p.sw, p.w, x0, x1, lx);
    float v[STEGO_CRFLOSS_MAX_K / PREP_LANES];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < STEGO_CRFLOSS_MAX_K / PREP_LANES; ++i) {
        const int k = s + PREP_LANES * i;
        v[i] = k < p.K ? tap4(p.code, b, k, y0, y1, x0, x1, ly, lx) : 0.f;
        ss = fmaf(v[i], v[i], ss);
    }
#pragma unroll
    for (int m = PREP_LANES / 2; m > 0; m >>= 1) ss += __shfl_xor(ss, m);      // the same tree in all 16 lanes
    const float nv = sqrtf(ss), den = fmaxf(nv, EPS);
#pragma unroll
    for (int i = 0; i < STEGO_CRFLOSS_MAX_K / PREP_LANES; ++i) {
        const int k = s + PREP_LANES * i;
        if (k < p.KP) xo[k] = p.normalize ? v[i] / den : v[i];
    }
    if (s == 0) {
        p.nrm[row * 2] = p.normalize ? 1.f / den : 1.f;
        p.nrm[row * 2 + 1] = (p.normalize && nv >= EPS) ? 1.f : 0.f;
        po[0] = (float)r;
        po[1] = (float)c;
    }
    if (s < GMAX) {
        float g = 0.f;
        if (s < p.G) {
            src_index(r, p.shg, p.hg, y0, y1, ly);
            src_index(c, p.swg, p.wg, x0, x1, lx);
            g = tap4(p.guid, b, s, y0, y1, x0, x1, ly, lx);
        }
        po[2 + s] = g;
    }
}

template <int NT, bool BWD>
__global__ __launch_bounds__(PAIR_TPB, 2) void crf_pairs(CrfParams p)
{
    constexpr int KP = 32 * NT, KS = KP + 1;            // odd LDS row stride: the 32 lanes of a ds_read_b32 group hit 32 banks
    extern __shared__ float4 smem4[];
    float* xs = reinterpret_cast<float*>(smem4);        // [CB][KS]
    float* ps = xs + CB * KS;                           // [CB][PS]
    double* red = reinterpret_cast<double*>(ps + CB * PS);   // [PAIR_TPB] (CB * KS + CB * PS is even: 8-byte aligned)
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, li = lane & 31, hf = lane >> 5;
    const int rw = wave & 1, cw = wave >> 1;
    const int b = blockIdx.x / p.n_rowblk, rb = blockIdx.x - b * p.n_rowblk;
    const size_t img = (size_t)b * p.Np;
    const int a0 = rb * ROWS_WG + rw * 32;

    float xa[KP / 2];                                   // the wave's rows as the B operand: B[k = 2 kk + hf][j = li]
    {
        const float* xr = p.xh + (img + a0 + li) * KP + hf;
#pragma unroll
        for (int kk = 0; kk < KP / 2; ++kk) xa[kk] = xr[2 * kk];
    }
    float ra, ca, ga[GMAX];
    {
        const float* q = p.pt + (img + a0 + li) * PS;
        ra = q[0];
        ca = q[1];
#pragma unroll
        for (int c = 0; c < GMAX; ++c) ga[c] = q[2 + c];
    }
    f32x16 pacc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) pacc[nt][r] = 0.f;
    double lsum = 0.0;

    for (int col0 = 0; col0 < p.Np; col0 += CB) {
        __syncthreads();
        {
            const float4* src = reinterpret_cast<const float4*>(p.xh + (img + col0) * KP);
            for (int i = t; i < CB * KP / 4; i += PAIR_TPB) {
                const float4 v = src[i];
                const int row = (4 * i) / KP, k = (4 * i) - row * KP;
                float* d = xs + row * KS + k;
                d[0] = v.x;
                d[1] = v.y;
                d[2] = v.z;
                d[3] = v.w;
            }
            const float* q = p.pt + (img + col0) * PS;
            for (int i = t; i < CB * PS; i += PAIR_TPB) ps[i] = q[i];
        }
        __syncthreads();
#pragma unroll 1
        for (int sub = 2 * cw; sub < 2 * cw + 2; ++sub) {
            f32x16 tacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) tacc[r] = 0.f;
            const float* xsub = xs + (sub * 32 + li) * KS + hf;         // A[i = li][k = 2 kk + hf]
#pragma unroll
            for (int kk = 0; kk < KP / 2; ++kk) tacc = __builtin_amdgcn_mfma_f32_32x32x2f32(xsub[2 * kk], xa[kk], tacc, 0, 0, 0);
            float tsum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* q = ps + (sub * 32 + acc_row(r, hf)) * PS;
                const float dr = q[0] - ra, dc = q[1] - ca;
                const float d2 = dr * dr + dc * dc;
                float dg = 0.f;
#pragma unroll
                for (int c = 0; c < GMAX; ++c)
                    if (c < p.G) {
                        const float e = q[2 + c] - ga[c];
                        dg = fmaf(e, e, dg);
                    }
                const float kv = p.w1 * __expf(-d2 * p.ia - dg * p.ib) + p.w2 * __expf(-d2 * p.ig) - p.shift;
                tsum = fmaf(kv, tacc[r], tsum);
                tacc[r] = kv;
            }
            lsum += (double)tsum;
            if (BWD) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float* xr = xs + (sub * 32 + acc_row(r, hf)) * KS + li;   // B[k-step r, half hf][j = li]
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) pacc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(tacc[r], xr[32 * nt], pacc[nt], 0, 0, 0);
                }
            }
        }
    }

    __syncthreads();                                    // every wave is past its last read of the stage
    if (BWD && cw == 1) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) xs[(rw * 32 + acc_row(r, hf)) * KP + nt * 32 + li] = pacc[nt][r];
    }
    const double wg_sum = block_sum<PAIR_TPB>(lsum, red);
    if (t == 0) p.part[blockIdx.x] = wg_sum;
    if (!BWD || cw == 1) return;

    float dot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ar = acc_row(r, hf);
        const float* xr = p.xh + (img + a0 + ar) * KP + li;
        float d = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            pacc[nt][r] += xs[(rw * 32 + ar) * KP + nt * 32 + li];
            d = fmaf(pacc[nt][r], xr[32 * nt], d);
        }
        dot[r] = d;
    }
#pragma unroll
    for (int m = 16; m > 0; m >>= 1)
#pragma unroll
        for (int r = 0; r < 16; ++r) dot[r] += __shfl_xor(dot[r], m);          // within the lane half: the channels of one row
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const size_t row = img + a0 + acc_row(r, hf);
        const float inv = p.nrm[row * 2], pd = p.nrm[row * 2 + 1] * dot[r];
        const float* xr = p.xh + row * KP + li;
        float* out = p.P + row * KP + li;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) out[32 * nt] = (pacc[nt][r] - pd * xr[32 * nt]) * inv * p.gscale;
    }
}

// first index in the ascending keys [0, n) whose key is >= key
__device__ inline int lower_bound(const unsigned long long* keys, int n, unsigned long long key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(FIN_TPB) void crf_finish(CrfParams p, int cell_blocks, int workers)
{
    __shared__ int start[FIN_CELLS + 1];
    __shared__ double red[FIN_TPB];
    const int t = threadIdx.x;
    if ((int)blockIdx.x >= workers) {                   // the loss: the last block of the grid
        const double n2 = (double)p.N * (double)p.N;
        double tot = 0.0;
        for (int b = t; b < p.B; b += FIN_TPB) {
            double s = 0.0;
            for (int i = 0; i < p.n_rowblk; ++i) s += p.part[(size_t)b * p.n_rowblk + i];
            if (p.per_image) p.per_image[b] = (float)(-s / n2);
            tot += s;
        }
        tot = block_sum<FIN_TPB>(tot, red);
        if (t == 0) p.loss[0] = (float)(-tot / (n2 * (double)p.B));
        return;
    }
    // the (image, block of 16 cells) units, image-major, walked with the stride of the bounded grid
    const int cells = p.h * p.w;
    const int wave = t >> 6, lane = t & 63;
    const long long units = (long long)cell_blocks * p.B;
    for (long long u = blockIdx.x; u < units; u += workers) {
        const int b = (int)(u / cell_blocks), cell0 = (int)(u - (long long)b * cell_blocks) * FIN_CELLS;
        __syncthreads();                                // the previous unit's ranges have been read
        if (t <= FIN_CELLS) start[t] = lower_bound(p.keys, p.T4p, (unsigned long long)(cell0 + t) << 16);
        __syncthreads();
        float* dd = const_cast<float*>(p.dcode.data) + (int64_t)b * p.dcode.stride_n;
        const size_t img = (size_t)b * p.Np;
        for (int j = 0; j < FIN_CELLS / 4; ++j) {
            const int ci = wave * (FIN_CELLS / 4) + j, cell = cell0 + ci;
            if (cell >= cells) break;
            const int e0 = start[ci], e1 = start[ci + 1];
            const int y = cell / p.w, x = cell - y * p.w;
            for (int k = lane; k < p.K; k += 64) {
                float acc = 0.f;
                for (int e = e0; e < e1; ++e) {
                    const unsigned tap = (unsigned)(p.keys[e] & 0xffffu);
                    acc = fmaf(p.tw[tap], p.P[(img + (tap >> 2)) * p.KP + k], acc);
                }
                dd[(int64_t)k * p.dcode.stride_c + (int64_t)y * p.dcode.stride_h + (int64_t)x * p.dcode.stride_w] = acc;
            }
        }
    }
}

using stego::aligned;
using stego::hip_rc;

inline bool side_ok(int v) { return v >= 1 && v <= STEGO_CRFLOSS_MAX_SIDE; }

int check_desc(const StegoCrfLossDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->flags & ~STEGO_CRFLOSS_NORMALIZE) return STEGO_ERR_CRFLOSS_FLAGS;
    if (d->K < 1 || d->K > STEGO_CRFLOSS_MAX_K || d->G < 1 || d->G > STEGO_CRFLOSS_MAX_G) return STEGO_ERR_CRFLOSS_DIM;
    if (d->N < 1 || d->N > STEGO_CRFLOSS_MAX_POINTS) return STEGO_ERR_CRFLOSS_POINTS;
    if (d->B < 1 || d->B > 65535 || !side_ok(d->h) || !side_ok(d->w) || !side_ok(d->hg) || !side_ok(d->wg) || !side_ok(d->H) || !side_ok(d->W))
        return STEGO_ERR_CRFLOSS_SIZE;
    if (!(std::isfinite(d->alpha) && d->alpha > 0.f && std::isfinite(d->beta) && d->beta > 0.f && std::isfinite(d->gamma) && d->gamma > 0.f &&
          std::isfinite(d->w1) && std::isfinite(d->w2) && std::isfinite(d->shift)))
        return STEGO_ERR_CRFLOSS_PARAM;
    return STEGO_OK;
}

struct Plan {
    int Np, KP, NT, T4p, n_rowblk, cell_blocks, fin_workers;
    size_t lds[STEGO_CRFLOSS_LAUNCHES];
    int64_t wgs[STEGO_CRFLOSS_LAUNCHES];
    size_t off_keys, off_tw, off_part, off_xh, off_P, off_pt, off_nrm, ws_bytes;
};

Plan plan(const StegoCrfLossDesc* d)
{
    Plan pl{};
    pl.Np = (d->N + CB - 1) / CB * CB;
    pl.NT = (d->K + 31) / 32;
    pl.KP = 32 * pl.NT;
    pl.T4p = 4;
    while (pl.T4p < 4 * d->N) pl.T4p <<= 1;
    pl.n_rowblk = pl.Np / ROWS_WG;
    pl.cell_blocks = (d->h * d->w + FIN_CELLS - 1) / FIN_CELLS;
    pl.lds[0] = (size_t)pl.T4p * 8;
    pl.wgs[0] = (int64_t)d->B * (pl.Np / PREP_PTS) + 1;
    pl.lds[1] = ((size_t)CB * (pl.KP + 1) + (size_t)CB * PS) * 4 + (size_t)PAIR_TPB * 8;
    pl.wgs[1] = (int64_t)d->B * pl.n_rowblk;
    pl.lds[2] = (FIN_CELLS + 1) * 4 + 4 + (size_t)FIN_TPB * 8;
    pl.fin_workers = (int)std::min<int64_t>((int64_t)pl.cell_blocks * d->B, FIN_MAX_WG);
    pl.wgs[2] = pl.fin_workers + 1;
    const size_t rows = (size_t)d->B * pl.Np;
    stego::WsLayout ws;
    pl.off_keys = ws.take((size_t)pl.T4p * 8, 16);
    pl.off_tw = ws.take((size_t)4 * d->N * 4, 16);
    pl.off_part = ws.take((size_t)d->B * pl.n_rowblk * 8, 16);
    pl.off_xh = ws.take(rows * pl.KP * 4, 16);
    pl.off_P = ws.take(rows * pl.KP * 4, 16);
    pl.off_pt = ws.take(rows * PS * 4, 16);
    pl.off_nrm = ws.take(rows * 2 * 4, 16);
    pl.ws_bytes = ws.total(16);
    return pl;
}

template <bool BWD>
hipError_t launch_pairs(int NT, const CrfParams& p, unsigned grid, size_t lds, hipStream_t s)
{
    return stego::with_const<1, 2, 3, 4>(NT, [&](auto N) { return stego::launch_first<crf_pairs<N(), BWD>>(grid, PAIR_TPB, lds, s, p); });      // (anything else: 4)
}

}  // namespace

extern "C" size_t stego_crf_loss_workspace_bytes(const StegoCrfLossDesc* desc)
{
    return check_desc(desc) == STEGO_OK ? plan(desc).ws_bytes : 0;
}

extern "C" int stego_crf_loss_plan(const StegoCrfLossDesc* desc, size_t lds_bytes[STEGO_CRFLOSS_LAUNCHES],
                                   int64_t workgroups[STEGO_CRFLOSS_LAUNCHES])
{
    const int rc = check_desc(desc);
    Plan pl{};
    if (rc == STEGO_OK) pl = plan(desc);
    return stego::report_plan(rc, STEGO_CRFLOSS_LAUNCHES, pl.lds, pl.wgs, lds_bytes, workgroups);
}

extern "C" int stego_crf_loss(const StegoCrfLossDesc* desc, const StegoMap* guidance, const StegoMap* code, const int64_t* coords,
                              float* loss, float* per_image, const StegoMap* d_code, void* workspace, size_t workspace_bytes,
                              stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!guidance || !guidance->data || !code || !code->data || !coords || !loss || !workspace || (d_code && !d_code->data))
        return STEGO_ERR_NULL;
    const Plan pl = plan(desc);
    if (workspace_bytes < pl.ws_bytes) return STEGO_ERR_WORKSPACE;
    if (!aligned(guidance->data, 4) || !aligned(code->data, 4) || !aligned(coords, 8) || !aligned(loss, 4) || !aligned(per_image, 4) ||
        (d_code && !aligned(d_code->data, 4)) || !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;

    using stego::at;
    CrfParams p{};
    p.code = *code;
    p.guid = *guidance;
    if (d_code) p.dcode = *d_code;
    p.coords = coords;
    p.keys = at<unsigned long long>(workspace, pl.off_keys);
    p.tw = at<float>(workspace, pl.off_tw);
    p.part = at<double>(workspace, pl.off_part);
    p.xh = at<float>(workspace, pl.off_xh);
    p.P = at<float>(workspace, pl.off_P);
    p.pt = at<float>(workspace, pl.off_pt);
    p.nrm = at<float>(workspace, pl.off_nrm);
    p.loss = loss;
    p.per_image = per_image;
    p.B = desc->B;
    p.K = desc->K;
    p.G = desc->G;
    p.h = desc->h;
    p.w = desc->w;
    p.hg = desc->hg;
    p.wg = desc->wg;
    p.H = desc->H;
    p.W = desc->W;
    p.N = desc->N;
    p.Np = pl.Np;
    p.KP = pl.KP;
    p.T4p = pl.T4p;
    p.normalize = (desc->flags & STEGO_CRFLOSS_NORMALIZE) ? 1 : 0;
    p.n_rowblk = pl.n_rowblk;
    p.sh = (float)desc->h / (float)desc->H;
    p.sw = (float)desc->w / (float)desc->W;
    p.shg = (float)desc->hg / (float)desc->H;
    p.swg = (float)desc->wg / (float)desc->W;
    p.ia = 1.f / (2.f * desc->alpha);
    p.ib = 1.f / (2.f * desc->beta);
    p.ig = 1.f / (2.f * desc->gamma);
    p.w1 = desc->w1;
    p.w2 = desc->w2;
    p.shift = desc->shift;
    p.gscale = (float)(-2.0 / ((double)desc->B * (double)desc->N * (double)desc->N));

    const hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t lds0 = d_code ? pl.lds[0] : 0;
    hipError_t e = stego::launch_first<crf_prepare>((unsigned)(pl.wgs[0] - (d_code ? 0 : 1)), PREP_TPB, lds0, s, p);
    if (e != hipSuccess) return hip_rc(e);
    e = d_code ? launch_pairs<true>(pl.NT, p, (unsigned)pl.wgs[1], pl.lds[1], s) : launch_pairs<false>(pl.NT, p, (unsigned)pl.wgs[1], pl.lds[1], s);
    if (e != hipSuccess) return hip_rc(e);
    // the (image, 16 cells) units of the unsample on a bounded grid (none without a gradient), and one more block for the loss
    const int workers = d_code ? pl.fin_workers : 0;
    return hip_rc(stego::launch_next<crf_finish>((unsigned)workers + 1, FIN_TPB, 0, s, p, pl.cell_blocks, workers));
}
