// Fused probe head (include/stego_probe.h): flip average, bilinear resize (align_corners=False), linear probe, cluster probe and a
// softmax / log_softmax / argmax per probe, from the low-resolution code straight to the full-resolution outputs in one launch.
//
// Grid: (output column tiles, output row tiles, B).  A workgroup of 256 threads owns a TY x TX tile of output pixels of one image:
//   1. it loads the source footprint of the tile (the code rows / columns its pixels interpolate from) into LDS, flip-averaged in the
//      reference's order ((code + code_flip[.., w-1-x]) / 2), K channels per pixel padded to a multiple of 4 plus 4 (bank spread);
//   2. it projects every footprint pixel onto both probes: W c + b for the linear probe, c . centroid for the cluster probe (one wave
//      per label row, so the weight row is wave-uniform and read with scalar loads; the lanes run over the footprint pixels);
//   3. every thread then takes one output pixel: torch's source index and weights, the four-tap interpolation of the projections (the
//      weights sum to 1, so this is the probe of the interpolated code), and for the cluster probe the norm of the interpolated
//      K-channel code (four taps from LDS, no Gram form that could cancel), then the per-probe softmax and its store.
// The tile is planned on the host so that the largest footprint fits 64 KiB of LDS (4 x 64 pixels, one per thread, at 8x upsampling;
// smaller tiles for strong downsampling); every output offset is 64-bit.  No atomics: repeat launches give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/stego_probe.h"
#include "probe_common.h"

namespace {

constexpr int TPB = 256;
constexpr size_t LDS_BUDGET = 64 * 1024;

struct ProbeParams {
    StegoMap code, flip;             // flip.data == nullptr: no flip average
    const float* lin_w;
    const float* lin_b;
    const float* cent;
    void* lin_out;
    void* clu_out;
    int32_t K, h, w, H, W;
    int32_t n_lin, n_clu, lin_kind, clu_kind;
    float alpha, scale_h, scale_w;
    int32_t TY, TX, max_nr, max_nc;  // output tile, footprint capacity (rows, columns)
    int32_t K4, KS;                  // K rounded up to 4; LDS floats per footprint pixel of code
    int32_t NPS;                     // LDS floats per footprint pixel of projections: 2 * NMAX label slots + 4
};

// The softmax of one probe at one pixel: l[0, n) are the logits, l[n, NMAX) are -inf (the label mask), so the max, the sums
// (exp(-inf - m) adds +0) and the argmax over all NMAX slots are those over [0, n) with no per-label test; only the stores test
// `j < n`.
template <int NMAX>
__device__ inline void finish(const float (&l)[NMAX], int n, int kind, void* out, int64_t b, int64_t HW, int64_t pix)
{
    float m = l[0];
#pragma unroll
    for (int j = 1; j < NMAX; ++j) m = fmaxf(m, l[j]);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) s += expf(l[j] - m);
    if (kind == STEGO_PROBE_PROBS) {
        float* o = static_cast<float*>(out) + b * n * HW + pix;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            if (j < n) *o = expf(l[j] - m) / s;
            o += HW;
        }
        return;
    }
    const float ls = logf(s);
    if (kind == STEGO_PROBE_LOG_PROBS) {
        float* o = static_cast<float*>(out) + b * n * HW + pix;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            if (j < n) *o = (l[j] - m) - ls;
            o += HW;
        }
        return;
    }
    // ARGMAX: the first maximum of the very values LOG_PROBS writes (rounding can tie two distinct logits there); -inf never wins
    int best = 0;
    float bv = (l[0] - m) - ls;
#pragma unroll
    for (int j = 1; j < NMAX; ++j) {
        const float v = (l[j] - m) - ls;
        best = v > bv ? j : best;
        bv = v > bv ? v : bv;
    }
    static_cast<int64_t*>(out)[b * HW + pix] = best;
}

template <int NMAX>
__global__ __launch_bounds__(TPB) void probe_head_kernel(ProbeParams p)
{
    extern __shared__ float4 smem4[];
    float* const cs = reinterpret_cast<float*>(smem4);
    float* const ps = cs + (size_t)p.max_nr * p.max_nc * p.KS;
    float* const mask = ps + (size_t)p.max_nr * p.max_nc * p.NPS;   // [2 * NMAX]: 0 for a label of the probe, -inf for a pad slot

    const int64_t b = blockIdx.z;
    const int Y0 = blockIdx.y * p.TY, X0 = blockIdx.x * p.TX;
    const int Y1 = min(Y0 + p.TY, p.H), X1 = min(X0 + p.TX, p.W);
    int ya, yb, xa, xb, t0;
    float tl;
    src_index(Y0, p.scale_h, p.h, ya, t0, tl);
    src_index(Y1 - 1, p.scale_h, p.h, t0, yb, tl);
    src_index(X0, p.scale_w, p.w, xa, t0, tl);
    src_index(X1 - 1, p.scale_w, p.w, t0, xb, tl);
    const int nr = min(yb - ya + 1, p.max_nr), nc = min(xb - xa + 1, p.max_nc);
    const int npx = nr * nc;

    // 1. the footprint's code, flip-averaged, channels K .. K4 zeroed
    for (int i = threadIdx.x; i < npx * p.K4; i += TPB) {
        const int k = i % p.K4, px = i / p.K4;
        const int y = ya + px / nc, x = xa + px % nc;
        float v = 0.f;
        if (k < p.K) {
            v = load_code(p.code, b, k, y, x);
            if (p.flip.data) v = (v + load_code(p.flip, b, k, y, p.w - 1 - x)) * 0.5f;
        }
        cs[px * p.KS + k] = v;
    }
    __syncthreads();

    // 2. projections: label slot j of both probes (linear slots [0, NMAX), cluster slots [NMAX, 2 NMAX)), one wave per slot
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (threadIdx.x < 2 * NMAX) {
        const int j = threadIdx.x;
        mask[j] = (j < NMAX ? j < p.n_lin : j - NMAX < p.n_clu) ? 0.f : -INFINITY;
    }
    for (int j = wave; j < 2 * NMAX; j += TPB / 64) {
        const bool lin = j < NMAX;
        const int jj = lin ? j : j - NMAX;
        const bool live = lin ? jj < p.n_lin : jj < p.n_clu;
        const float* row = live ? (lin ? p.lin_w : p.cent) + (size_t)jj * p.K : nullptr;
        const float bias = live && lin ? p.lin_b[jj] : 0.f;
        for (int px = lane; px < npx; px += 64) {
            float acc = 0.f;
            if (live) {
                const float* c = cs + px * p.KS;
                for (int k = 0; k < p.K; ++k) acc = fmaf(row[k], c[k], acc);
                acc += bias;
            }
            ps[px * p.NPS + j] = acc;
        }
    }
    __syncthreads();

    // 3. output pixels
    const int64_t HW = (int64_t)p.H * p.W;
    const float4* cs4 = reinterpret_cast<const float4*>(cs);
    const float4* ps4 = reinterpret_cast<const float4*>(ps);
    const float4* mask4 = reinterpret_cast<const float4*>(mask);
    const int KS4 = p.KS >> 2, NPS4 = p.NPS >> 2;
    {   // one output pixel per thread (TY * TX <= 256; a loop here would let the compiler hoist the label loops' tests and spill)
        const int i = threadIdx.x;
        const int Y = Y0 + i / p.TX, X = X0 + i % p.TX;
        if (i >= p.TY * p.TX || Y >= Y1 || X >= X1) return;
        int y0, y1, x0, x1;
        float h1, w1;
        src_index(Y, p.scale_h, p.h, y0, y1, h1);
        src_index(X, p.scale_w, p.w, x0, x1, w1);
        const float h0 = 1.f - h1, w0 = 1.f - w1;
        // (clamps: memory safety only - the footprint covers every tap, the host plan one row / column more)
        const int r0 = max(min(y0 - ya, nr - 1), 0), r1 = max(min(y1 - ya, nr - 1), 0);
        const int c0 = max(min(x0 - xa, nc - 1), 0), c1 = max(min(x1 - xa, nc - 1), 0);
        const int q00 = r0 * nc + c0, q01 = r0 * nc + c1, q10 = r1 * nc + c0, q11 = r1 * nc + c1;
        const int64_t pix = (int64_t)Y * p.W + X;

        if (p.lin_kind != STEGO_PROBE_SKIP) {
            float l[NMAX];
#pragma unroll
            for (int g = 0; g < NMAX / 4; ++g) {
                const float4 a = ps4[q00 * NPS4 + g], bq = ps4[q01 * NPS4 + g], c = ps4[q10 * NPS4 + g], d = ps4[q11 * NPS4 + g];
                const float4 mk = mask4[g];
                l[4 * g + 0] = (h0 * (w0 * a.x + w1 * bq.x) + h1 * (w0 * c.x + w1 * d.x)) + mk.x;
                l[4 * g + 1] = (h0 * (w0 * a.y + w1 * bq.y) + h1 * (w0 * c.y + w1 * d.y)) + mk.y;
                l[4 * g + 2] = (h0 * (w0 * a.z + w1 * bq.z) + h1 * (w0 * c.z + w1 * d.z)) + mk.z;
                l[4 * g + 3] = (h0 * (w0 * a.w + w1 * bq.w) + h1 * (w0 * c.w + w1 * d.w)) + mk.w;
            }
            finish<NMAX>(l, p.n_lin, p.lin_kind, p.lin_out, b, HW, pix);
        }
        if (p.clu_kind != STEGO_PROBE_SKIP) {
            // F.normalize's denominator: the norm of the interpolated code, clamped at 1e-12
            float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k4 = 0; k4 < (p.K4 >> 2); ++k4) {
                const float4 a = cs4[q00 * KS4 + k4], bq = cs4[q01 * KS4 + k4], c = cs4[q10 * KS4 + k4], d = cs4[q11 * KS4 + k4];
                const float vx = h0 * (w0 * a.x + w1 * bq.x) + h1 * (w0 * c.x + w1 * d.x);
                const float vy = h0 * (w0 * a.y + w1 * bq.y) + h1 * (w0 * c.y + w1 * d.y);
                const float vz = h0 * (w0 * a.z + w1 * bq.z) + h1 * (w0 * c.z + w1 * d.z);
                const float vw = h0 * (w0 * a.w + w1 * bq.w) + h1 * (w0 * c.w + w1 * d.w);
                n4.x = fmaf(vx, vx, n4.x);
                n4.y = fmaf(vy, vy, n4.y);
                n4.z = fmaf(vz, vz, n4.z);
                n4.w = fmaf(vw, vw, n4.w);
            }
            const float den = fmaxf(sqrtf((n4.x + n4.y) + (n4.z + n4.w)), 1e-12f);
            float l[NMAX];
#pragma unroll
            for (int g = 0; g < NMAX / 4; ++g) {
                const int o = NMAX / 4 + g;
                const float4 a = ps4[q00 * NPS4 + o], bq = ps4[q01 * NPS4 + o], c = ps4[q10 * NPS4 + o], d = ps4[q11 * NPS4 + o];
                const float4 mk = mask4[o];
                l[4 * g + 0] = (h0 * (w0 * a.x + w1 * bq.x) + h1 * (w0 * c.x + w1 * d.x)) / den * p.alpha + mk.x;
                l[4 * g + 1] = (h0 * (w0 * a.y + w1 * bq.y) + h1 * (w0 * c.y + w1 * d.y)) / den * p.alpha + mk.y;
                l[4 * g + 2] = (h0 * (w0 * a.z + w1 * bq.z) + h1 * (w0 * c.z + w1 * d.z)) / den * p.alpha + mk.z;
                l[4 * g + 3] = (h0 * (w0 * a.w + w1 * bq.w) + h1 * (w0 * c.w + w1 * d.w)) / den * p.alpha + mk.w;
            }
            finish<NMAX>(l, p.n_clu, p.clu_kind, p.clu_out, b, HW, pix);
        }
    }
}

inline int hip_rc(hipError_t e) { return e == hipSuccess ? STEGO_OK : STEGO_ERR_HIP + (int)e; }

inline bool aligned(const void* ptr, size_t a) { return (reinterpret_cast<uintptr_t>(ptr) % a) == 0; }

inline bool kind_ok(int k) { return k >= STEGO_PROBE_SKIP && k <= STEGO_PROBE_ARGMAX; }

int check_desc(const StegoProbeDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (!kind_ok(d->lin_kind) || !kind_ok(d->clu_kind) || (d->lin_kind == STEGO_PROBE_SKIP && d->clu_kind == STEGO_PROBE_SKIP))
        return STEGO_ERR_PROBE_OUTPUT;
    if (d->K < 1 || d->K > STEGO_PROBE_MAX_K) return STEGO_ERR_PROBE_DIM;
    if (d->lin_kind != STEGO_PROBE_SKIP && (d->n_lin < 1 || d->n_lin > STEGO_PROBE_MAX_N)) return STEGO_ERR_PROBE_DIM;
    if (d->clu_kind != STEGO_PROBE_SKIP && (d->n_clu < 1 || d->n_clu > STEGO_PROBE_MAX_N)) return STEGO_ERR_PROBE_DIM;
    if (d->B < 1 || d->B > 65535 || d->h < 1 || d->h > STEGO_PROBE_MAX_CODE || d->w < 1 || d->w > STEGO_PROBE_MAX_CODE || d->H < 1 ||
        d->H > STEGO_PROBE_MAX_OUT || d->W < 1 || d->W > STEGO_PROBE_MAX_OUT)
        return STEGO_ERR_PROBE_SIZE;
    return STEGO_OK;
}

struct Plan {
    int TY, TX, max_nr, max_nc, K4, KS, NMAX, NPS;
    float scale_h, scale_w;
    size_t lds;
};

Plan plan(const StegoProbeDesc* d)
{
    Plan pl{};
    pl.scale_h = (float)d->h / (float)d->H;
    pl.scale_w = (float)d->w / (float)d->W;
    pl.K4 = round4(d->K);
    pl.KS = pl.K4 + 4;
    const int n = std::max(d->lin_kind != STEGO_PROBE_SKIP ? d->n_lin : 0, d->clu_kind != STEGO_PROBE_SKIP ? d->n_clu : 0);
    pl.NMAX = n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64;
    pl.NPS = 2 * pl.NMAX + 4;
    pl.TX = d->W < 64 ? d->W : 64;
    pl.TY = TPB / pl.TX;
    pl.TY = pl.TY < d->H ? pl.TY : d->H;
    for (;;) {
        pl.max_nr = max_span(d->H, d->h, pl.scale_h, pl.TY);
        pl.max_nc = max_span(d->W, d->w, pl.scale_w, pl.TX);
        pl.lds = ((size_t)pl.max_nr * pl.max_nc * (pl.KS + pl.NPS) + 2 * pl.NMAX) * sizeof(float);
        if (pl.lds <= LDS_BUDGET || (pl.TY == 1 && pl.TX == 1)) break;
        if (pl.TY > 1)
            pl.TY = (pl.TY + 1) / 2;
        else
            pl.TX = (pl.TX + 1) / 2;
    }
    return pl;
}

}  // namespace

extern "C" size_t stego_probe_head_plan(const StegoProbeDesc* desc, int32_t* tile_rows, int32_t* tile_cols)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    const Plan pl = plan(desc);
    if (tile_rows) *tile_rows = pl.TY;
    if (tile_cols) *tile_cols = pl.TX;
    return pl.lds;
}

extern "C" int stego_probe_head(const StegoProbeDesc* desc, const StegoMap* code, const StegoMap* code_flip, const float* lin_w,
                                const float* lin_b, const float* centroids, void* lin_out, void* clu_out, stego_stream_t stream)
{
    int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    const bool lin = desc->lin_kind != STEGO_PROBE_SKIP, clu = desc->clu_kind != STEGO_PROBE_SKIP;
    if (!code || !code->data || (code_flip && !code_flip->data)) return STEGO_ERR_NULL;
    if ((lin && (!lin_w || !lin_b || !lin_out)) || (clu && (!centroids || !clu_out))) return STEGO_ERR_NULL;
    if (!aligned(code->data, 4) || (code_flip && !aligned(code_flip->data, 4))) return STEGO_ERR_ALIGN;
    if (lin && (!aligned(lin_w, 4) || !aligned(lin_b, 4) || !aligned(lin_out, desc->lin_kind == STEGO_PROBE_ARGMAX ? 8 : 4)))
        return STEGO_ERR_ALIGN;
    if (clu && (!aligned(centroids, 4) || !aligned(clu_out, desc->clu_kind == STEGO_PROBE_ARGMAX ? 8 : 4))) return STEGO_ERR_ALIGN;

    const Plan pl = plan(desc);
    ProbeParams p{};
    p.code = *code;
    p.flip = code_flip ? *code_flip : StegoMap{nullptr, 0, 0, 0, 0};
    p.lin_w = lin_w;
    p.lin_b = lin_b;
    p.cent = centroids;
    p.lin_out = lin_out;
    p.clu_out = clu_out;
    p.K = desc->K;
    p.h = desc->h;
    p.w = desc->w;
    p.H = desc->H;
    p.W = desc->W;
    p.n_lin = lin ? desc->n_lin : 0;      // a skipped probe has no live label slot: its n, weights and output are never read
    p.n_clu = clu ? desc->n_clu : 0;
    p.lin_kind = desc->lin_kind;
    p.clu_kind = desc->clu_kind;
    p.alpha = desc->alpha;
    p.scale_h = pl.scale_h;
    p.scale_w = pl.scale_w;
    p.TY = pl.TY;
    p.TX = pl.TX;
    p.max_nr = pl.max_nr;
    p.max_nc = pl.max_nc;
    p.K4 = pl.K4;
    p.KS = pl.KS;
    p.NPS = pl.NPS;
    const dim3 grid((unsigned)((desc->W + pl.TX - 1) / pl.TX), (unsigned)((desc->H + pl.TY - 1) / pl.TY), (unsigned)desc->B);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    (void)hipGetLastError();
    if (pl.NMAX == 8)
        probe_head_kernel<8><<<grid, TPB, pl.lds, s>>>(p);
    else if (pl.NMAX == 16)
        probe_head_kernel<16><<<grid, TPB, pl.lds, s>>>(p);
    else if (pl.NMAX == 32)
        probe_head_kernel<32><<<grid, TPB, pl.lds, s>>>(p);
    else
        probe_head_kernel<64><<<grid, TPB, pl.lds, s>>>(p);
    return hip_rc(hipGetLastError());
}
