// The phases of the fused probe head, stated once for the kernels built from them: probe_head.hip's (softmax, log-softmax or argmax
// maps as the sink) and confusion.hip's (two confusion matrices).  The FMA order, the contraction and the four-tap expression decide
// the last bit of every prediction, so both kernels take them from here and predict the same labels by construction.
// Every phase is a forced-inline function (a template on NMAX, the label slots per probe) that takes plain values: each kernel keeps
// its own parameter struct, reads the values from where it holds them, and places its own barriers between the phases.
// LDS: cs [footprint pixel][KS] the code, ps [footprint pixel][NPS] the projections (linear slots [0, NMAX), cluster slots
// [NMAX, 2 NMAX)), mask [2 NMAX].  KS and NPS are multiples of 4: phase 3 reads both as float4.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/stego_probe.h"
#include "probe_common.h"

namespace {

// 1. the footprint's code, flip-averaged in the reference's order ((code + code_flip[.., w-1-x]) / 2), channels K .. K4 zeroed
__device__ __forceinline__ void load_footprint(float* cs, const StegoMap& code, const StegoMap& flip, bool has_flip, int64_t b,
                                               const Footprint& f, int K, int K4, int KS, int w)
{
    for (int i = threadIdx.x; i < f.npx * K4; i += PROBE_TPB) {
        const int k = i % K4, px = i / K4;
        const int y = f.ya + px / f.nc, x = f.xa + px % f.nc;
        float v = 0.f;
        if (k < K) {
            v = load_code(code, b, k, y, x);
            if (has_flip) v = (v + load_code(flip, b, k, y, w - 1 - x)) * 0.5f;
        }
        cs[px * KS + k] = v;
    }
}

// The label mask: 0 for a label of the probe, -inf for a pad slot.  With it l[n, NMAX) are -inf, so the max, the sums (exp(-inf - m)
// adds +0) and the argmax over all NMAX slots are those over [0, n) with no per-label test.
template <int NMAX>
__device__ __forceinline__ void init_mask(float* mask, int n_lin, int n_clu)
{
    if (threadIdx.x < 2 * NMAX) {
        const int j = threadIdx.x;
        mask[j] = (j < NMAX ? j < n_lin : j - NMAX < n_clu) ? 0.f : -INFINITY;
    }
}

// 2. projections of every footprint pixel onto label slot j of both probes: W c + b for the linear probe, c . centroid for the cluster
//    probe.  One wave per slot, so the weight row is wave-uniform and read with scalar loads; the lanes run over the pixels.
template <int NMAX>
__device__ __forceinline__ void project(float* ps, const float* cs, const float* lin_w, const float* lin_b, const float* cent, int n_lin,
                                        int n_clu, int K, int KS, int NPS, int npx, int wave, int lane)
{
    for (int j = wave; j < 2 * NMAX; j += PROBE_TPB / 64) {
        const bool lin = j < NMAX;
        const int jj = lin ? j : j - NMAX;
        const bool live = lin ? jj < n_lin : jj < n_clu;
        const float* row = live ? (lin ? lin_w : cent) + (size_t)jj * K : nullptr;
        const float bias = live && lin ? lin_b[jj] : 0.f;
        for (int px = lane; px < npx; px += 64) {
            float acc = 0.f;
            if (live) {
                const float* c = cs + px * KS;
                for (int k = 0; k < K; ++k) acc = fmaf(row[k], c[k], acc);
                acc += bias;
            }
            ps[px * NPS + j] = acc;
        }
    }
}

// 3. the taps of one output pixel: torch's weights and the four footprint pixels they apply to
struct Taps { float h0, h1, w0, w1; int q00, q01, q10, q11; };

__device__ __forceinline__ Taps pixel_taps(int Y, int X, float scale_h, float scale_w, int h, int w, const Footprint& f)
{
    int y0, y1, x0, x1;
    float h1, w1;
    src_index(Y, scale_h, h, y0, y1, h1);
    src_index(X, scale_w, w, x0, x1, w1);
    const float h0 = 1.f - h1, w0 = 1.f - w1;
    // (clamps: memory safety only - the footprint covers every tap, the host plan one row / column more)
    const int r0 = max(min(y0 - f.ya, f.nr - 1), 0), r1 = max(min(y1 - f.ya, f.nr - 1), 0);
    const int c0 = max(min(x0 - f.xa, f.nc - 1), 0), c1 = max(min(x1 - f.xa, f.nc - 1), 0);
    return Taps{h0, h1, w0, w1, r0 * f.nc + c0, r0 * f.nc + c1, r1 * f.nc + c0, r1 * f.nc + c1};
}

// the four-tap interpolation; the weights sum to 1, so the interpolated projection is the probe of the interpolated code
__device__ __forceinline__ float tap4(const Taps& t, float a, float b, float c, float d)
{
    return t.h0 * (t.w0 * a + t.w1 * b) + t.h1 * (t.w0 * c + t.w1 * d);
}

// the linear probe's logits of the pixel
template <int NMAX>
__device__ __forceinline__ void linear_logits(float (&l)[NMAX], const float4* ps4, const float4* mask4, int NPS4, const Taps& t)
{
#pragma unroll
    for (int g = 0; g < NMAX / 4; ++g) {
        const float4 a = ps4[t.q00 * NPS4 + g], bq = ps4[t.q01 * NPS4 + g], c = ps4[t.q10 * NPS4 + g], d = ps4[t.q11 * NPS4 + g];
        const float4 mk = mask4[g];
        l[4 * g + 0] = tap4(t, a.x, bq.x, c.x, d.x) + mk.x;
        l[4 * g + 1] = tap4(t, a.y, bq.y, c.y, d.y) + mk.y;
        l[4 * g + 2] = tap4(t, a.z, bq.z, c.z, d.z) + mk.z;
        l[4 * g + 3] = tap4(t, a.w, bq.w, c.w, d.w) + mk.w;
    }
}

// F.normalize's denominator: the norm of the interpolated K-channel code (four taps from LDS, no Gram form that could cancel),
// clamped at 1e-12
__device__ __forceinline__ float code_norm(const float4* cs4, int KS4, int K4, const Taps& t)
{
    float4 n4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k4 = 0; k4 < (K4 >> 2); ++k4) {
        const float4 a = cs4[t.q00 * KS4 + k4], bq = cs4[t.q01 * KS4 + k4], c = cs4[t.q10 * KS4 + k4], d = cs4[t.q11 * KS4 + k4];
        const float vx = tap4(t, a.x, bq.x, c.x, d.x);
        const float vy = tap4(t, a.y, bq.y, c.y, d.y);
        const float vz = tap4(t, a.z, bq.z, c.z, d.z);
        const float vw = tap4(t, a.w, bq.w, c.w, d.w);
        n4.x = fmaf(vx, vx, n4.x);
        n4.y = fmaf(vy, vy, n4.y);
        n4.z = fmaf(vz, vz, n4.z);
        n4.w = fmaf(vw, vw, n4.w);
    }
    return fmaxf(sqrtf((n4.x + n4.y) + (n4.z + n4.w)), 1e-12f);
}

// the cluster probe's logits of the pixel: alpha times the cosine to every centroid; den is code_norm()
template <int NMAX>
__device__ __forceinline__ void cluster_logits(float (&l)[NMAX], const float4* ps4, const float4* mask4, int NPS4, const Taps& t,
                                               float den, float alpha)
{
#pragma unroll
    for (int g = 0; g < NMAX / 4; ++g) {
        const int o = NMAX / 4 + g;
        const float4 a = ps4[t.q00 * NPS4 + o], bq = ps4[t.q01 * NPS4 + o], c = ps4[t.q10 * NPS4 + o], d = ps4[t.q11 * NPS4 + o];
        const float4 mk = mask4[o];
        l[4 * g + 0] = tap4(t, a.x, bq.x, c.x, d.x) / den * alpha + mk.x;
        l[4 * g + 1] = tap4(t, a.y, bq.y, c.y, d.y) / den * alpha + mk.y;
        l[4 * g + 2] = tap4(t, a.z, bq.z, c.z, d.z) / den * alpha + mk.z;
        l[4 * g + 3] = tap4(t, a.w, bq.w, c.w, d.w) / den * alpha + mk.w;
    }
}

// the softmax's statistics over all NMAX slots: the maximum and the sum of exp(l - m); log_softmax is (l[j] - m) - logf(s)
template <int NMAX>
__device__ __forceinline__ void softmax_stats(const float (&l)[NMAX], float& m, float& s)
{
    m = l[0];
#pragma unroll
    for (int j = 1; j < NMAX; ++j) m = fmaxf(m, l[j]);
    s = 0.f;
#pragma unroll
    for (int j = 0; j < NMAX; ++j) s += expf(l[j] - m);
}

// The predicted label: the first maximum of the very values log_softmax gives (rounding can tie two distinct logits there); -inf
// never wins.  ls = logf(s).
template <int NMAX>
__device__ __forceinline__ int first_max(const float (&l)[NMAX], float m, float ls)
{
    int best = 0;
    float bv = (l[0] - m) - ls;
#pragma unroll
    for (int j = 1; j < NMAX; ++j) {
        const float v = (l[j] - m) - ls;
        best = v > bv ? j : best;
        bv = v > bv ? v : bv;
    }
    return best;
}

template <int NMAX>
__device__ __forceinline__ int first_max(const float (&l)[NMAX])
{
    float m, s;
    softmax_stats<NMAX>(l, m, s);
    return first_max<NMAX>(l, m, logf(s));
}

// The softmax of one probe at one pixel and its store (probe_head.hip's and stitch_probe.hip's sink; `kind` is a STEGO_PROBE_*): l[0, n) are the logits, l[n, NMAX) are -inf (the label mask); only the stores
// test `j < n`.
template <int NMAX>
__device__ inline void finish(const float (&l)[NMAX], int n, int kind, void* out, int64_t b, int64_t HW, int64_t pix)
{
    float m, s;
    softmax_stats<NMAX>(l, m, s);
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
    static_cast<int64_t*>(out)[b * HW + pix] = first_max<NMAX>(l, m, ls);      // ARGMAX
}

}  // namespace
