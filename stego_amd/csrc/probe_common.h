// What the fused probe kernels share (probe_head.hip, confusion.hip, probe_train.hip): torch's bilinear source index on the device and
// on the host, the strided code load, an output tile's source footprint on the device and its largest extent on the host, the host's
// tile plan of the probe head and the probe-confusion kernel, and the pointer checks their launchers share.  The device phases those two kernels are built from: probe_phases.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/stego_corr.h"
#include "host_util.h"

namespace {

constexpr int PROBE_TPB = 256;       // threads of a probe workgroup: one output pixel each

inline __host__ __device__ int round4(int x) { return (x + 3) & ~3; }

// torch's area_pixel_compute_source_index (align_corners=False, linear) and upsample_bilinear2d's taps: i0, i1 = i0 + (i0 < in - 1),
// lambda of the i1 tap.  The expression is written as torch writes it, so the device compiler contracts it the way torch's is.
__device__ inline void src_index(int dst, float scale, int in, int& i0, int& i1, float& l1)
{
    float s = scale * (dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

__device__ inline float load_code(const StegoMap& m, int64_t b, int k, int y, int x)
{
    return m.data[b * m.stride_n + (int64_t)k * m.stride_c + (int64_t)y * m.stride_h + (int64_t)x * m.stride_w];
}

// The source footprint of the output tile [Y0, Y1) x [X0, X1): first code row / column, rows and columns (no more than the host
// planned room for), pixels.
struct Footprint { int ya, xa, nr, nc, npx; };

__device__ __forceinline__ Footprint tile_footprint(int Y0, int Y1, int X0, int X1, float scale_h, float scale_w, int h, int w, int max_nr,
                                                    int max_nc)
{
    int ya, yb, xa, xb, t0;
    float tl;
    src_index(Y0, scale_h, h, ya, t0, tl);
    src_index(Y1 - 1, scale_h, h, t0, yb, tl);
    src_index(X0, scale_w, w, xa, t0, tl);
    src_index(X1 - 1, scale_w, w, t0, xb, tl);
    const int nr = min(yb - ya + 1, max_nr), nc = min(xb - xa + 1, max_nc);
    return Footprint{ya, xa, nr, nc, nr * nc};
}

// Host mirror of src_index (plain float arithmetic); plan() adds one row / column of margin for a contraction the device may apply.
void host_src(int dst, float scale, int in, int& i0, int& i1)
{
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s < in - 1 ? (int)s : in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
}

int max_span(int out, int in, float scale, int T)
{
    int best = 1;
    for (int t0 = 0; t0 < out; t0 += T) {
        const int t1 = (t0 + T < out ? t0 + T : out) - 1;
        int a, b, u;
        host_src(t0, scale, in, a, u);
        host_src(t1, scale, in, u, b);
        best = b - a + 1 > best ? b - a + 1 : best;
    }
    return best + 1 < in ? best + 1 : in;
}

// The pointer checks the probe head, the stitched probe head and the probe-confusion kernel share, in the order every one of them
// keeps: the code maps, then a live probe's weights and output - all for NULL, then all for alignment (the output's alignment depends
// on what is written there, so the caller names it).  STEGO_OK, STEGO_ERR_NULL or STEGO_ERR_ALIGN.
inline int check_probe_ptrs(const StegoMap* code, const StegoMap* code_flip, bool lin, const float* lin_w, const float* lin_b,
                            const void* lin_out, size_t lin_out_align, bool clu, const float* centroids, const void* clu_out,
                            size_t clu_out_align)
{
    using stego::aligned;
    if (!code || !code->data || (code_flip && !code_flip->data)) return STEGO_ERR_NULL;
    if ((lin && (!lin_w || !lin_b || !lin_out)) || (clu && (!centroids || !clu_out))) return STEGO_ERR_NULL;
    if (!aligned(code->data, 4) || (code_flip && !aligned(code_flip->data, 4))) return STEGO_ERR_ALIGN;
    if (lin && (!aligned(lin_w, 4) || !aligned(lin_b, 4) || !aligned(lin_out, lin_out_align))) return STEGO_ERR_ALIGN;
    if (clu && (!aligned(centroids, 4) || !aligned(clu_out, clu_out_align))) return STEGO_ERR_ALIGN;
    return STEGO_OK;
}

// Label slots of a kernel instantiation: the probes' larger live label count n, rounded up to 8, 16, 32 or 64.
inline int label_slots(int n) { return n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }

// The tile of the probe head and the probe-confusion kernel: TY x TX <= PROBE_TPB output pixels, halved (rows first) until the largest
// footprint - KS floats of code and NPS of projections per pixel - and the caller's `extra` bytes of LDS fit `budget` together.
struct TilePlan {
    int TY, TX, max_nr, max_nc, K4, KS, NMAX, NPS;
    float scale_h, scale_w;
    size_t lds;
};

TilePlan plan_tile(int K, int h, int w, int H, int W, int n, size_t extra, size_t budget)
{
    TilePlan pl{};
    pl.scale_h = (float)h / (float)H;
    pl.scale_w = (float)w / (float)W;
    pl.K4 = round4(K);
    pl.KS = pl.K4 + 4;
    pl.NMAX = label_slots(n);
    pl.NPS = 2 * pl.NMAX + 4;
    pl.TX = W < 64 ? W : 64;
    pl.TY = PROBE_TPB / pl.TX;
    pl.TY = pl.TY < H ? pl.TY : H;
    for (;;) {
        pl.max_nr = max_span(H, h, pl.scale_h, pl.TY);
        pl.max_nc = max_span(W, w, pl.scale_w, pl.TX);
        pl.lds = (size_t)pl.max_nr * pl.max_nc * (pl.KS + pl.NPS) * sizeof(float) + extra;
        if (pl.lds <= budget || (pl.TY == 1 && pl.TX == 1)) break;
        if (pl.TY > 1)
            pl.TY = (pl.TY + 1) / 2;
        else
            pl.TX = (pl.TX + 1) / 2;
    }
    return pl;
}

}  // namespace
