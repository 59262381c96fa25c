// The device-side augmented view and the fused aug-alignment loss (include/stego_aug.h).
//
// stego_augment, at most two launches:
//   aug_mean   (only when a record applies contrast): one workgroup per (image, 8 output rows).  Every thread recomputes the geometry
//              and the operators that precede contrast for its pixels and adds their gray values in index order; an LDS tree adds the
//              256 thread sums in fp64: one partial per workgroup, [B, ceil(R / 8)].  Images without contrast return at once.
//   aug_apply  one workgroup per (image, 16 x 64 output tile).  The first wave adds the image's partials in a fixed order (the mean);
//              the tile with a halo of 2, reflected at the image border, is recomputed into LDS (geometry, the four operators, gray);
//              the 5-tap blur runs separably from LDS (rows into a second LDS tile, then columns); every thread owns four neighbouring
//              pixels of one row and writes them with 16-byte stores when R % 4 == 0, and the same thread writes their coord_aug.
//              Images without blur compute no halo.
// stego_aug_align, two launches:
//   align_pixels  one wave per output pixel (b, p, q), lanes over the K <= 128 channels: the resized coordinate, the four taps of
//              `code`, both normalisations, the cosine term (a float per pixel), d_code_aug of the pixel, and for d_code the gradient
//              row of the sampled vector [B S^2, K] with its four (cell, weight) tap records.
//   align_finish  the transpose of the taps without atomics: one wave per four code cells scans the image's tap records 64 pixels at
//              a time (one 16-byte load per lane, ballots against its cells) and adds weight * row over the matches in ascending
//              (pixel, tap) order; every element of d_code is written.  One more workgroup adds the loss terms in a fixed order in fp64.
// No float atomics anywhere: repeat launches give the same bits.  Offsets into maps and the workspace are 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/stego_aug.h"
#include "addon_device.h"
#include "host_util.h"
#include "probe_common.h"

namespace {

constexpr int TPB = 256;
constexpr int MEAN_ROWS = 8;                                   // output rows per workgroup of aug_mean
constexpr int TH = 16, TW = 64, HALO = 2;                      // aug_apply: output tile and blur halo
constexpr int HH = TH + 2 * HALO, HW = TW + 2 * HALO;
constexpr int FIN_CELLS = 16, FIN_MAX_WG = 1 << 18;            // align_finish: cells per workgroup (four per wave), grid bound
constexpr float EPS = 1e-10f;

struct AugP {
    StegoMap img;
    const StegoAugParams* params;
    float *img_aug, *coord_aug;
    double* part;
    int32_t B, H, W, R, nblk;
};

__device__ inline int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
__device__ inline float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ inline float gray3(const float v[3]) { return 0.2989f * v[0] + 0.587f * v[1] + 0.114f * v[2]; }

// The pixel of the resized crop of the (flipped) image at output (y, x): F.resized_crop after hflip, bilinear, align_corners=False.
// The record was checked on the host; the indices are clamped all the same, so a device table that differs from it reads no foreign memory.
__device__ inline void fetch(const AugP& p, const StegoAugParams& rec, int b, float sy, float sx, int y, int x, float v[3])
{
    int y0, y1, x0, x1;
    float ly, lx;
    src_index(y, sy, rec.ch, y0, y1, ly);
    src_index(x, sx, rec.cw, x0, x1, lx);
    const int r0 = clampi(rec.top + y0, p.H - 1), r1 = clampi(rec.top + y1, p.H - 1);
    int c0 = rec.left + x0, c1 = rec.left + x1;
    if (rec.flip) {
        c0 = p.W - 1 - c0;
        c1 = p.W - 1 - c1;
    }
    c0 = clampi(c0, p.W - 1);
    c1 = clampi(c1, p.W - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float p00 = load_code(p.img, b, c, r0, c0), p01 = load_code(p.img, b, c, r0, c1);
        const float p10 = load_code(p.img, b, c, r1, c0), p11 = load_code(p.img, b, c, r1, c1);
        v[c] = (1.f - ly) * ((1.f - lx) * p00 + lx * p01) + ly * ((1.f - lx) * p10 + lx * p11);
    }
}

// torchvision's adjust_hue on one pixel: _rgb2hsv, h = (h + f) mod 1, _hsv2rgb
__device__ inline void hue(float v[3], float f)
{
    const float r = v[0], g = v[1], b = v[2];
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float div = eqc ? 1.f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    const float hr = (maxc == r) ? bc - gc : 0.f;
    const float hg = (maxc == g && maxc != r) ? 2.f + rc - bc : 0.f;
    const float hb = (maxc != g && maxc != r) ? 4.f + gc - rc : 0.f;
    float h = fmodf((hr + hg + hb) / 6.f + 1.f, 1.f);
    h += f;
    h -= floorf(h);
    const float h6 = h * 6.f, fl = floorf(h6), ff = h6 - fl;
    int i = (int)fl % 6;
    if (i < 0) i += 6;
    const float val = maxc;
    const float pp = clamp01(val * (1.f - s)), q = clamp01(val * (1.f - s * ff)), t = clamp01(val * (1.f - s * (1.f - ff)));
    switch (i) {
        case 0: v[0] = val; v[1] = t; v[2] = pp; break;
        case 1: v[0] = q; v[1] = val; v[2] = pp; break;
        case 2: v[0] = pp; v[1] = val; v[2] = t; break;
        case 3: v[0] = pp; v[1] = q; v[2] = val; break;
        case 4: v[0] = t; v[1] = pp; v[2] = val; break;
        default: v[0] = val; v[1] = pp; v[2] = q; break;
    }
}

// the first `count` entries of the record's order on one pixel; `mean` is what contrast blends with
__device__ inline void apply_ops(float v[3], const StegoAugParams& rec, int count, float mean)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i >= count) break;
        const int op = rec.order[i];
        if (op == STEGO_AUG_BRIGHTNESS) {
            const float f = rec.factor[0];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = clamp01(f * v[c] + (1.f - f) * 0.f);
        } else if (op == STEGO_AUG_CONTRAST) {
            const float f = rec.factor[1];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = clamp01(f * v[c] + (1.f - f) * mean);
        } else if (op == STEGO_AUG_SATURATION) {
            const float f = rec.factor[2], g = gray3(v);
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = clamp01(f * v[c] + (1.f - f) * g);
        } else if (op == STEGO_AUG_HUE) {
            hue(v, rec.factor[3]);
        }
    }
}

__device__ inline int contrast_index(const StegoAugParams& rec)
{
    int ci = -1;
#pragma unroll
    for (int i = 3; i >= 0; --i)
        if (rec.order[i] == STEGO_AUG_CONTRAST) ci = i;
    return ci;
}

__global__ __launch_bounds__(TPB) void aug_mean(AugP p)
{
    __shared__ double red[TPB];
    const int t = threadIdx.x, blk = blockIdx.x, b = blockIdx.y;
    const StegoAugParams rec = p.params[b];
    const int ci = contrast_index(rec);
    if (ci < 0) return;                                  // the whole workgroup: this image has no contrast
    const float sy = (float)rec.ch / (float)p.R, sx = (float)rec.cw / (float)p.R;
    const int y0 = blk * MEAN_ROWS;
    const int n = min(MEAN_ROWS, p.R - y0) * p.R;
    float s = 0.f;
    for (int idx = t; idx < n; idx += TPB) {
        const int dy = idx / p.R;
        float v[3];
        fetch(p, rec, b, sy, sx, y0 + dy, idx - dy * p.R, v);
        apply_ops(v, rec, ci, 0.f);
        s += gray3(v);
    }
    const double sum = block_sum<TPB>((double)s, red);
    if (t == 0) p.part[(size_t)b * p.nblk + blk] = sum;
}

// index -1 -> 1, -2 -> 2, R -> R - 2, R + 1 -> R - 3; positions further out (tile rows past the image) are never used: clamped
__device__ inline int reflect(int i, int R)
{
    if (i < 0) i = -i;
    if (i >= R) i = 2 * (R - 1) - i;
    return clampi(i, R - 1);
}

// torch.linspace(-1, 1, n)[i] in fp32: from the start in the lower half, from the end in the upper one
__device__ inline float ramp(int i, int n)
{
    if (n <= 1) return -1.f;
    const float step = 2.f / (float)(n - 1);
    return i < n / 2 ? -1.f + step * (float)i : 1.f - step * (float)(n - 1 - i);
}

__global__ __launch_bounds__(TPB) void aug_apply(AugP p, int vec4)
{
    __shared__ float s0[3][HH][HW];                      // the tile with its halo after the operators and gray
    __shared__ float s1[3][HH][TW];                      // ... after the blur along the rows
    __shared__ float smean;
    const int t = threadIdx.x, b = blockIdx.z;
    const int ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TW;
    const int R = p.R;
    const StegoAugParams rec = p.params[b];
    const float sy = (float)rec.ch / (float)R, sx = (float)rec.cw / (float)R;
    const bool blur = rec.blur_sigma > 0.f;
    float mean = 0.f;
    if (contrast_index(rec) >= 0) {                      // the whole workgroup
        if (t < 64) {
            double s = 0.0;
            for (int i = t; i < p.nblk; i += 64) s += p.part[(size_t)b * p.nblk + i];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
            if (t == 0) smean = (float)(s / ((double)R * (double)R));
        }
        __syncthreads();
        mean = smean;
    }
    for (int idx = t; idx < HH * HW; idx += TPB) {
        const int i = idx / HW, j = idx - i * HW;
        if (!blur && (i < HALO || i >= HH - HALO || j < HALO || j >= HW - HALO)) continue;
        float v[3];
        fetch(p, rec, b, sy, sx, reflect(ty0 - HALO + i, R), reflect(tx0 - HALO + j, R), v);
        apply_ops(v, rec, 4, mean);
        if (rec.gray) v[0] = v[1] = v[2] = gray3(v);
        s0[0][i][j] = v[0];
        s0[1][i][j] = v[1];
        s0[2][i][j] = v[2];
    }
    __syncthreads();
    float k0 = 1.f, k1 = 0.f, k2 = 0.f;
    if (blur) {                                          // the whole workgroup
        const float e1 = expf(-0.5f * (1.f / rec.blur_sigma) * (1.f / rec.blur_sigma));
        const float e2 = expf(-0.5f * (2.f / rec.blur_sigma) * (2.f / rec.blur_sigma));
        const float sum = e2 + e1 + 1.f + e1 + e2;
        k0 = 1.f / sum;
        k1 = e1 / sum;
        k2 = e2 / sum;
        for (int idx = t; idx < 3 * HH * TW; idx += TPB) {
            const int c = idx / (HH * TW), r = idx - c * (HH * TW), i = r / TW, j = r - i * TW;
            const float* q = &s0[c][i][j];
            s1[c][i][j] = k2 * q[0] + k1 * q[1] + k0 * q[2] + k1 * q[3] + k2 * q[4];
        }
        __syncthreads();
    }
    const int row = t >> 4, xq = (t & 15) * 4;
    const int y = ty0 + row, x = tx0 + xq;
    if (y >= R || x >= R) return;
    float out[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            out[c][e] = blur ? k2 * s1[c][row][xq + e] + k1 * s1[c][row + 1][xq + e] + k0 * s1[c][row + 2][xq + e] +
                                   k1 * s1[c][row + 3][xq + e] + k2 * s1[c][row + 4][xq + e]
                             : s0[c][row + HALO][xq + HALO + e];
    // coord_aug: the same geometry on the row ramp (channel 0) and the column ramp (channel 1)
    float co[8];
    {
        int y0, y1;
        float ly;
        src_index(y, sy, rec.ch, y0, y1, ly);
        const float cy = (1.f - ly) * ramp(clampi(rec.top + y0, p.H - 1), p.H) + ly * ramp(clampi(rec.top + y1, p.H - 1), p.H);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int x0, x1;
            float lx;
            src_index(min(x + e, R - 1), sx, rec.cw, x0, x1, lx);
            int c0 = rec.left + x0, c1 = rec.left + x1;
            if (rec.flip) {
                c0 = p.W - 1 - c0;
                c1 = p.W - 1 - c1;
            }
            co[2 * e] = cy;
            co[2 * e + 1] = (1.f - lx) * ramp(clampi(c0, p.W - 1), p.W) + lx * ramp(clampi(c1, p.W - 1), p.W);
        }
    }
    const size_t plane = (size_t)R * R;
    float* io = p.img_aug + (size_t)b * 3 * plane + (size_t)y * R + x;
    float* cp = p.coord_aug + ((size_t)b * plane + (size_t)y * R + x) * 2;
    if (vec4) {                                          // R % 4 == 0: the four pixels are inside and every address is 16-byte aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(io + c * plane) = make_float4(out[c][0], out[c][1], out[c][2], out[c][3]);
        *reinterpret_cast<float4*>(cp) = make_float4(co[0], co[1], co[2], co[3]);
        *reinterpret_cast<float4*>(cp + 4) = make_float4(co[4], co[5], co[6], co[7]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x + e < R) {
#pragma unroll
                for (int c = 0; c < 3; ++c) io[c * plane + e] = out[c][e];
                cp[2 * e] = co[2 * e];
                cp[2 * e + 1] = co[2 * e + 1];
            }
    }
}

// ---- the aug-alignment loss
struct AlignP {
    StegoMap code, caug, dcode, dcaug;
    const float* coord;
    float *loss, *part, *dA, *tw;
    int* tcell;
    int32_t B, K, h, w, S, Rh, Rw, has_dcode, has_dcaug;
    float sr, sc, gscale;                               // Rh / S, Rw / S, -1 / (B S^2)
    long long npix;
};

__global__ __launch_bounds__(TPB) void align_pixels(AlignP p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n = (long long)blockIdx.x * (TPB / 64) + wave;
    if (n >= p.npix) return;                             // (no barrier in this kernel)
    const int S2 = p.S * p.S;
    const int b = (int)(n / S2), rem = (int)(n - (long long)b * S2);
    const int pp = rem / p.S, q = rem - pp * p.S;
    // ds[b, q, pp, :]: row q, column pp of the coordinate map resized to S x S
    float gx, gy;
    {
        int y0, y1, x0, x1;
        float ly, lx;
        src_index(q, p.sr, p.Rh, y0, y1, ly);
        src_index(pp, p.sc, p.Rw, x0, x1, lx);
        const float* cb = p.coord + (size_t)b * p.Rh * p.Rw * 2;
        const float2 c00 = *reinterpret_cast<const float2*>(cb + ((size_t)y0 * p.Rw + x0) * 2);
        const float2 c01 = *reinterpret_cast<const float2*>(cb + ((size_t)y0 * p.Rw + x1) * 2);
        const float2 c10 = *reinterpret_cast<const float2*>(cb + ((size_t)y1 * p.Rw + x0) * 2);
        const float2 c11 = *reinterpret_cast<const float2*>(cb + ((size_t)y1 * p.Rw + x1) * 2);
        gx = (1.f - ly) * ((1.f - lx) * c00.x + lx * c01.x) + ly * ((1.f - lx) * c10.x + lx * c11.x);
        gy = (1.f - ly) * ((1.f - lx) * c00.y + lx * c01.y) + ly * ((1.f - lx) * c10.y + lx * c11.y);
    }
    // grid_sample, align_corners=True, border padding: unnormalise, clip, the four taps nw, ne, sw, se
    const float ix = fminf(fmaxf(((gx + 1.f) / 2.f) * (float)(p.w - 1), 0.f), (float)(p.w - 1));
    const float iy = fminf(fmaxf(((gy + 1.f) / 2.f) * (float)(p.h - 1), 0.f), (float)(p.h - 1));
    const int xi = clampi((int)floorf(ix), p.w - 1), yi = clampi((int)floorf(iy), p.h - 1);
    const float wx1 = ix - (float)xi, wx0 = (float)(xi + 1) - ix, wy1 = iy - (float)yi, wy0 = (float)(yi + 1) - iy;
    const bool vx = xi + 1 <= p.w - 1, vy = yi + 1 <= p.h - 1;      // a tap outside the map has weight 0 and is dropped
    const float wt[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
    const int cell[4] = {yi * p.w + xi, vx ? yi * p.w + xi + 1 : -1, vy ? (yi + 1) * p.w + xi : -1, (vx && vy) ? (yi + 1) * p.w + xi + 1 : -1};
    float a[2], c[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int k = lane + 64 * i;
        a[i] = c[i] = 0.f;
        if (k < p.K) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (cell[j] >= 0) a[i] += wt[j] * load_code(p.code, b, k, yi + (j >> 1), xi + (j & 1));
            c[i] = load_code(p.caug, b, k, pp, q);
        }
    }
    const float na = sqrtf(wave_sum(a[0] * a[0] + a[1] * a[1])), nc = sqrtf(wave_sum(c[0] * c[0] + c[1] * c[1]));
    const float da = fmaxf(na, EPS), dc = fmaxf(nc, EPS);
    const float ah[2] = {a[0] / da, a[1] / da}, ch[2] = {c[0] / dc, c[1] / dc};
    const float dot = wave_sum(ah[0] * ch[0] + ah[1] * ch[1]);
    if (lane == 0) p.part[n] = dot;
    const float pa = na >= EPS ? dot : 0.f, pc = nc >= EPS ? dot : 0.f;       // torch's clamp: no projection below eps
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int k = lane + 64 * i;
        if (k >= p.K) continue;
        if (p.has_dcaug)
            const_cast<float*>(p.dcaug.data)[(int64_t)b * p.dcaug.stride_n + (int64_t)k * p.dcaug.stride_c + (int64_t)pp * p.dcaug.stride_h +
                                             (int64_t)q * p.dcaug.stride_w] = p.gscale * (ah[i] - pc * ch[i]) / dc;
        if (p.has_dcode) p.dA[(size_t)n * p.K + k] = p.gscale * (ch[i] - pa * ah[i]) / da;
    }
    if (p.has_dcode && lane < 4) {
        p.tcell[(size_t)n * 4 + lane] = lane == 0 ? cell[0] : lane == 1 ? cell[1] : lane == 2 ? cell[2] : cell[3];
        p.tw[(size_t)n * 4 + lane] = lane == 0 ? wt[0] : lane == 1 ? wt[1] : lane == 2 ? wt[2] : wt[3];
    }
}

__global__ __launch_bounds__(TPB) void align_finish(AlignP p, int cell_blocks, int workers)
{
    __shared__ double red[TPB];
    const int t = threadIdx.x;
    if ((int)blockIdx.x >= workers) {                    // the loss: the last block of the grid
        double s = 0.0;
        for (long long i = t; i < p.npix; i += TPB) s += (double)p.part[i];
        s = block_sum<TPB>(s, red);
        if (t == 0) p.loss[0] = (float)(-s / (double)p.npix);
        return;
    }
    // the (image, block of 16 cells) units, image-major, walked with the stride of the bounded grid; four cells per wave
    const int lane = t & 63, wave = t >> 6;
    const int cells = p.h * p.w, S2 = p.S * p.S;
    const long long units = (long long)cell_blocks * p.B;
    const int4* recs = reinterpret_cast<const int4*>(p.tcell);
    for (long long u = blockIdx.x; u < units; u += workers) {
        const int b = (int)(u / cell_blocks), cell0 = (int)(u - (long long)b * cell_blocks) * FIN_CELLS + wave * (FIN_CELLS / 4);
        if (cell0 >= cells) continue;
        const size_t pix0 = (size_t)b * S2;
        float acc[4][2];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) acc[ci][0] = acc[ci][1] = 0.f;
        for (int base = 0; base < S2; base += 64) {
            const int4 cs = base + lane < S2 ? recs[pix0 + base + lane] : make_int4(-1, -1, -1, -1);
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) {
                const int cell = cell0 + ci;
                const unsigned long long m0 = __ballot(cs.x == cell), m1 = __ballot(cs.y == cell), m2 = __ballot(cs.z == cell),
                                         m3 = __ballot(cs.w == cell);
                unsigned long long any = m0 | m1 | m2 | m3;
                while (any) {                            // the matching pixels in ascending order, their taps in tap order
                    const int l = __builtin_ctzll(any);
                    any &= any - 1;
                    const size_t row = pix0 + base + l;
                    const float* dr = p.dA + row * p.K;
                    const float v0 = lane < p.K ? dr[lane] : 0.f, v1 = lane + 64 < p.K ? dr[lane + 64] : 0.f;
                    const float* w4 = p.tw + row * 4;
                    if ((m0 >> l) & 1) { acc[ci][0] = fmaf(w4[0], v0, acc[ci][0]); acc[ci][1] = fmaf(w4[0], v1, acc[ci][1]); }
                    if ((m1 >> l) & 1) { acc[ci][0] = fmaf(w4[1], v0, acc[ci][0]); acc[ci][1] = fmaf(w4[1], v1, acc[ci][1]); }
                    if ((m2 >> l) & 1) { acc[ci][0] = fmaf(w4[2], v0, acc[ci][0]); acc[ci][1] = fmaf(w4[2], v1, acc[ci][1]); }
                    if ((m3 >> l) & 1) { acc[ci][0] = fmaf(w4[3], v0, acc[ci][0]); acc[ci][1] = fmaf(w4[3], v1, acc[ci][1]); }
                }
            }
        }
        float* dd = const_cast<float*>(p.dcode.data) + (int64_t)b * p.dcode.stride_n;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
            const int cell = cell0 + ci;
            if (cell >= cells) break;
            const int y = cell / p.w, x = cell - y * p.w;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int k = lane + 64 * i;
                if (k < p.K) dd[(int64_t)k * p.dcode.stride_c + (int64_t)y * p.dcode.stride_h + (int64_t)x * p.dcode.stride_w] = acc[ci][i];
            }
        }
    }
}

using stego::aligned;
using stego::hip_rc;

int check_aug(const StegoAugDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->B < 1 || d->B > 65535 || d->H < 1 || d->H > STEGO_AUG_MAX_SIDE || d->W < 1 || d->W > STEGO_AUG_MAX_SIDE ||
        d->R < STEGO_AUG_MIN_RES || d->R > STEGO_AUG_MAX_SIDE)
        return STEGO_ERR_AUG_SIZE;
    return STEGO_OK;
}

bool record_ok(const StegoAugDesc* d, const StegoAugParams& r, bool& contrast)
{
    if ((r.flip != 0 && r.flip != 1) || (r.gray != 0 && r.gray != 1) || r.reserved != 0) return false;
    if (r.ch < 1 || r.ch > d->H || r.cw < 1 || r.cw > d->W || r.top < 0 || r.top > d->H - r.ch || r.left < 0 || r.left > d->W - r.cw) return false;
    int seen = 0;
    for (int i = 0; i < 4; ++i) {
        const int op = r.order[i];
        if (op < 0 || op > STEGO_AUG_NONE) return false;
        if (op == STEGO_AUG_NONE) continue;
        if (seen & (1 << op)) return false;
        seen |= 1 << op;
    }
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(r.factor[i])) return false;
    if (r.factor[0] < 0.f || r.factor[1] < 0.f || r.factor[2] < 0.f || r.factor[3] < -0.5f || r.factor[3] > 0.5f) return false;
    if (!std::isfinite(r.blur_sigma) || r.blur_sigma < 0.f) return false;
    contrast = (seen & (1 << STEGO_AUG_CONTRAST)) != 0;
    return true;
}

int check_records(const StegoAugDesc* d, const StegoAugParams* recs, int64_t* bad, int32_t* any_contrast)
{
    if (bad) *bad = -1;
    if (any_contrast) *any_contrast = 0;
    const int rc = check_aug(d);
    if (rc != STEGO_OK) return rc;
    if (!recs) return STEGO_ERR_NULL;
    int any = 0;
    for (int i = 0; i < d->B; ++i) {
        bool contrast = false;
        if (!record_ok(d, recs[i], contrast)) {
            if (bad) *bad = i;
            return STEGO_ERR_AUG_PARAM;
        }
        any |= contrast ? 1 : 0;
    }
    if (any_contrast) *any_contrast = any;
    return STEGO_OK;
}

struct AugPlan {
    int nblk, tiles_x, tiles_y;
    size_t lds[STEGO_AUG_LAUNCHES];
    int64_t wgs[STEGO_AUG_LAUNCHES];
    size_t off_part, ws_bytes;
};

AugPlan aug_plan(const StegoAugDesc* d)
{
    AugPlan pl{};
    pl.nblk = (d->R + MEAN_ROWS - 1) / MEAN_ROWS;
    pl.tiles_x = (d->R + TW - 1) / TW;
    pl.tiles_y = (d->R + TH - 1) / TH;
    pl.lds[0] = TPB * sizeof(double);
    pl.wgs[0] = (int64_t)d->B * pl.nblk;
    pl.lds[1] = (size_t)(3 * HH * HW + 3 * HH * TW + 1) * sizeof(float);
    pl.wgs[1] = (int64_t)d->B * pl.tiles_x * pl.tiles_y;
    stego::WsLayout ws;
    pl.off_part = ws.take((size_t)d->B * pl.nblk * sizeof(double), 16);
    pl.ws_bytes = ws.total(16);
    return pl;
}

int check_align(const StegoAugAlignDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->K < 1 || d->K > STEGO_AUGALIGN_MAX_K) return STEGO_ERR_AUGALIGN_DIM;
    const auto side = [](int v, int hi) { return v >= 1 && v <= hi; };
    if (d->B < 1 || d->B > 65535 || !side(d->h, STEGO_AUGALIGN_MAX_SIDE) || !side(d->w, STEGO_AUGALIGN_MAX_SIDE) ||
        !side(d->S, STEGO_AUGALIGN_MAX_SIDE) || !side(d->Rh, STEGO_AUG_MAX_SIDE) || !side(d->Rw, STEGO_AUG_MAX_SIDE))
        return STEGO_ERR_AUGALIGN_SIZE;
    return STEGO_OK;
}

struct AlignPlan {
    long long npix;
    int cell_blocks, workers;
    size_t lds[STEGO_AUGALIGN_LAUNCHES];
    int64_t wgs[STEGO_AUGALIGN_LAUNCHES];
    size_t off_part, off_tcell, off_tw, off_dA, ws_bytes;
};

AlignPlan align_plan(const StegoAugAlignDesc* d)
{
    AlignPlan pl{};
    pl.npix = (long long)d->B * d->S * d->S;
    pl.cell_blocks = (d->h * d->w + FIN_CELLS - 1) / FIN_CELLS;
    pl.workers = (int)std::min<long long>((long long)pl.cell_blocks * d->B, FIN_MAX_WG);
    pl.wgs[0] = (pl.npix + TPB / 64 - 1) / (TPB / 64);
    pl.lds[1] = TPB * sizeof(double);
    pl.wgs[1] = (int64_t)pl.workers + 1;
    stego::WsLayout ws;
    pl.off_part = ws.take((size_t)pl.npix * 4, 16);
    pl.off_tcell = ws.take((size_t)pl.npix * 16, 16);
    pl.off_tw = ws.take((size_t)pl.npix * 16, 16);
    pl.off_dA = ws.take((size_t)pl.npix * d->K * 4, 16);
    pl.ws_bytes = ws.total(16);
    return pl;
}

}  // namespace

extern "C" int stego_augment_check_params(const StegoAugDesc* desc, const StegoAugParams* params_host, int64_t* bad_record,
                                          int32_t* any_contrast)
{
    return check_records(desc, params_host, bad_record, any_contrast);
}

extern "C" size_t stego_augment_workspace_bytes(const StegoAugDesc* desc)
{
    return check_aug(desc) == STEGO_OK ? aug_plan(desc).ws_bytes : 0;
}

extern "C" int stego_augment_plan(const StegoAugDesc* desc, size_t lds_bytes[STEGO_AUG_LAUNCHES], int64_t workgroups[STEGO_AUG_LAUNCHES])
{
    const int rc = check_aug(desc);
    AugPlan pl{};
    if (rc == STEGO_OK) pl = aug_plan(desc);
    return stego::report_plan(rc, STEGO_AUG_LAUNCHES, pl.lds, pl.wgs, lds_bytes, workgroups);
}

extern "C" int stego_augment(const StegoAugDesc* desc, const StegoMap* img, const StegoAugParams* params_host, const StegoAugParams* params,
                             float* img_aug, float* coord_aug, void* workspace, size_t workspace_bytes, stego_stream_t stream)
{
    int rc = check_aug(desc);
    if (rc != STEGO_OK) return rc;
    if (!img || !img->data || !params_host || !params || !img_aug || !coord_aug || !workspace) return STEGO_ERR_NULL;
    int32_t any_contrast = 0;
    rc = check_records(desc, params_host, nullptr, &any_contrast);
    if (rc != STEGO_OK) return rc;
    const AugPlan pl = aug_plan(desc);
    if (workspace_bytes < pl.ws_bytes) return STEGO_ERR_WORKSPACE;
    if (!aligned(img->data, 4) || !aligned(params, 4) || !aligned(img_aug, 16) || !aligned(coord_aug, 16) || !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;

    AugP p{};
    p.img = *img;
    p.params = params;
    p.img_aug = img_aug;
    p.coord_aug = coord_aug;
    p.part = stego::at<double>(workspace, pl.off_part);
    p.B = desc->B;
    p.H = desc->H;
    p.W = desc->W;
    p.R = desc->R;
    p.nblk = pl.nblk;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 tiles((unsigned)pl.tiles_x, (unsigned)pl.tiles_y, (unsigned)desc->B);
    const int vec4 = desc->R % 4 == 0 ? 1 : 0;
    if (!any_contrast) return hip_rc(stego::launch_first<aug_apply>(tiles, TPB, 0, s, p, vec4));
    const hipError_t e = stego::launch_first<aug_mean>(dim3((unsigned)pl.nblk, (unsigned)desc->B), TPB, 0, s, p);
    if (e != hipSuccess) return hip_rc(e);
    return hip_rc(stego::launch_next<aug_apply>(tiles, TPB, 0, s, p, vec4));
}

extern "C" size_t stego_aug_align_workspace_bytes(const StegoAugAlignDesc* desc)
{
    return check_align(desc) == STEGO_OK ? align_plan(desc).ws_bytes : 0;
}

extern "C" int stego_aug_align_plan(const StegoAugAlignDesc* desc, size_t lds_bytes[STEGO_AUGALIGN_LAUNCHES],
                                    int64_t workgroups[STEGO_AUGALIGN_LAUNCHES])
{
    const int rc = check_align(desc);
    AlignPlan pl{};
    if (rc == STEGO_OK) pl = align_plan(desc);
    return stego::report_plan(rc, STEGO_AUGALIGN_LAUNCHES, pl.lds, pl.wgs, lds_bytes, workgroups);
}

extern "C" int stego_aug_align(const StegoAugAlignDesc* desc, const StegoMap* code, const StegoMap* code_aug, const float* coord,
                               float* loss, const StegoMap* d_code, const StegoMap* d_code_aug, void* workspace, size_t workspace_bytes,
                               stego_stream_t stream)
{
    const int rc = check_align(desc);
    if (rc != STEGO_OK) return rc;
    if (!code || !code->data || !code_aug || !code_aug->data || !coord || !loss || !workspace || (d_code && !d_code->data) ||
        (d_code_aug && !d_code_aug->data))
        return STEGO_ERR_NULL;
    const AlignPlan pl = align_plan(desc);
    if (workspace_bytes < pl.ws_bytes) return STEGO_ERR_WORKSPACE;
    if (!aligned(code->data, 4) || !aligned(code_aug->data, 4) || !aligned(coord, 4) || !aligned(loss, 4) ||
        (d_code && !aligned(d_code->data, 4)) || (d_code_aug && !aligned(d_code_aug->data, 4)) || !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;

    using stego::at;
    AlignP p{};
    p.code = *code;
    p.caug = *code_aug;
    if (d_code) p.dcode = *d_code;
    if (d_code_aug) p.dcaug = *d_code_aug;
    p.coord = coord;
    p.loss = loss;
    p.part = at<float>(workspace, pl.off_part);
    p.tcell = at<int>(workspace, pl.off_tcell);
    p.tw = at<float>(workspace, pl.off_tw);
    p.dA = at<float>(workspace, pl.off_dA);
    p.B = desc->B;
    p.K = desc->K;
    p.h = desc->h;
    p.w = desc->w;
    p.S = desc->S;
    p.Rh = desc->Rh;
    p.Rw = desc->Rw;
    p.has_dcode = d_code ? 1 : 0;
    p.has_dcaug = d_code_aug ? 1 : 0;
    p.sr = (float)desc->Rh / (float)desc->S;
    p.sc = (float)desc->Rw / (float)desc->S;
    p.gscale = (float)(-1.0 / (double)pl.npix);
    p.npix = pl.npix;

    const hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = stego::launch_first<align_pixels>((unsigned)pl.wgs[0], TPB, 0, s, p);
    if (e != hipSuccess) return hip_rc(e);
    // the (image, 16 cells) units of the transpose on a bounded grid (none without d_code), and one more block for the loss
    const int workers = d_code ? pl.workers : 0;
    return hip_rc(stego::launch_next<align_finish>((unsigned)workers + 1, TPB, 0, s, p, pl.cell_blocks, workers));
}
