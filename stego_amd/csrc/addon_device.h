// Small device helpers the add-on units share (crf_loss.hip, rec_loss.hip, augment.hip, corr_pr.hip, corr_heat.hip): the taps of a
// bilinear grid sample, the row of a 32 x 32 accumulator register, the sum over a wave and the fp64 sum over a workgroup.  Like
// probe_common.h, everything sits in the including unit's anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// ATen grid_sampler_2d (bilinear, border, align_corners=True) as corr_common.h's make_taps computes it, with the factors of the four
// weights kept apart (corr_pr.hip's label test needs to know which taps have a non-zero weight) and no 16-bit packing of the pixel.
struct Taps {
    int x0, y0, x1, y1;
    float wx0, wx1, wy0, wy1;
};

__device__ __forceinline__ Taps bilinear_taps(float x, float y, int H, int W)
{
    float ix = ((x + 1.f) * 0.5f) * (float)(W - 1);
    float iy = ((y + 1.f) * 0.5f) * (float)(H - 1);
    ix = fminf((float)(W - 1), fmaxf(ix, 0.f));
    iy = fminf((float)(H - 1), fmaxf(iy, 0.f));
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    Taps t;
    t.x0 = (int)fx0;
    t.y0 = (int)fy0;
    t.x1 = t.x0 + 1;
    t.y1 = t.y0 + 1;
    t.wx1 = ix - fx0;
    t.wx0 = (fx0 + 1.f) - ix;
    t.wy1 = iy - fy0;
    t.wy0 = (fy0 + 1.f) - iy;
    if (t.x1 > W - 1) { t.wx1 = 0.f; t.x1 = t.x0; }      // out-of-range taps contribute zero
    if (t.y1 > H - 1) { t.wy1 = 0.f; t.y1 = t.y0; }
    return t;
}

// row of a 32 x 32 accumulator tile that register r of lane half hf holds (the C / D layout of the 32x32 matrix instructions)
__device__ inline int acc_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

__device__ inline float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);        // the same tree in all 64 lanes
    return v;
}

// The sum of one fp64 value per thread over a workgroup of TPB threads, in one fixed tree through red[TPB] in LDS: valid in every
// thread after the last barrier.  Whatever else the caller stores to LDS before the call is published by the first barrier too.
template <int TPB>
__device__ inline double block_sum(double v, double* red)
{
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int m = TPB / 2; m > 0; m >>= 1) {
        if (t < m) red[t] += red[t + m];
        __syncthreads();
    }
    return red[0];
}

}  // namespace
