// What the fused probe kernels share (probe_head.hip, probe_train.hip): torch's bilinear source index on the device and on the host,
// the strided code load, and the largest source footprint of an output tile.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/stego_corr.h"

namespace {

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

}  // namespace
