// Salience-guided coordinate draws (include/stego_salience.h): both sides of the whole batch in one launch.
//
// Grid (B images, 2 sides), 1024 threads = 16 waves per workgroup.  Pass 1: a wave takes a block of 64 chunks of 64 pixels at a time;
// per chunk every lane tests one pixel (coalesced), __ballot gives the chunk's 64-bit mask and its popcount is kept by the lane
// of the chunk's number; a wave scan of those counts leaves the chunk's exclusive prefix inside its block (16 bits in LDS) and the
// block's total.  Wave 0 then scans the block totals (at most 256).  Pass 2: thread j < S * S resolves its sample - a binary search
// of its rank over the block prefix, then over the chunk prefix of that block - and leaves (chunk, k) in LDS; pass 3: the waves take
// the samples in turn, re-read the sample's chunk, ballot again, and the lane that holds the k-th set bit writes the coordinate.
// No atomics: the result is a pure function of the inputs.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/stego_salience.h"
#include "host_util.h"

namespace {

constexpr int TPB = 1024;
constexpr int WAVES = TPB / 64;
constexpr int MAX_CHUNKS = STEGO_SALIENCE_MAX_PIXELS / 64;       // 16384
constexpr int MAX_BLOCKS = MAX_CHUNKS / 64;                      // 256
constexpr int MAX_SAMPLES = STEGO_SALIENCE_MAX_S * STEGO_SALIENCE_MAX_S;

struct SalParams {
    const void* mask[2];
    const float* u;
    const float* u_mix;
    const float* reg[2];
    float* coords[2];
    int32_t B, H, W, SS;
};

template <bool F32>
__device__ __forceinline__ bool nonzero_at(const void* m, int64_t i)
{
    if constexpr (F32)
        return static_cast<const float*>(m)[i] != 0.0f;           // -0.0 is zero, NaN is not: torch.nonzero's rule
    else
        return static_cast<const uint8_t*>(m)[i] != 0;
}

template <bool F32>
__global__ __launch_bounds__(TPB) void salience_draw_kernel(SalParams p)
{
    __shared__ uint16_t chunk_pre[MAX_CHUNKS];      // exclusive prefix of the chunk counts inside their block of 64 chunks
    __shared__ uint32_t block_pre[MAX_BLOCKS + 1];  // block totals, then their exclusive prefix; [n_blocks] = c
    __shared__ int32_t sel_chunk[MAX_SAMPLES];      // per sample: its chunk, or -1 when the sample is already written
    __shared__ int32_t sel_k[MAX_SAMPLES];          // per sample: which set bit of that chunk's ballot

    const int b = blockIdx.x, side = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = p.H * p.W;
    const int n_chunks = (n + 63) >> 6;
    const int n_blocks = (n_chunks + 63) >> 6;
    const void* mask = p.mask[side];
    const int64_t base = (int64_t)b * n;

    // ---- pass 1: chunk counts and their prefix inside each block of 64 chunks
    for (int blk = wave; blk < n_blocks; blk += WAVES) {
        uint32_t mine = 0;
        const int c0 = blk << 6;
#pragma unroll 8
        for (int i = 0; i < 64; ++i) {
            const int px = ((c0 + i) << 6) + lane;
            const bool nz = px < n && nonzero_at<F32>(mask, base + px);
            const uint32_t cnt = (uint32_t)__popcll(__ballot(nz));
            if (lane == i) mine = cnt;
        }
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (c0 + lane < n_chunks) chunk_pre[c0 + lane] = (uint16_t)(incl - mine);
        if (lane == 63) block_pre[blk] = incl;
    }
    __syncthreads();

    // ---- exclusive scan of the block totals (wave 0: four blocks per lane)
    if (wave == 0) {
        uint32_t v[4], s = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = lane * 4 + q;
            v[q] = i < n_blocks ? block_pre[i] : 0u;
            s += v[q];
        }
        uint32_t incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        uint32_t run = incl - s;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = lane * 4 + q;
            if (i < n_blocks) block_pre[i] = run;
            run += v[q];
        }
        if (lane == 63) block_pre[n_blocks] = incl;
    }
    __syncthreads();

    // ---- pass 2: every sample's rank -> (chunk, bit); samples that need no pixel are written here
    const int SS = p.SS;
    const int H = p.H;
    const float fH = (float)H;
    const int c = (int)block_pre[n_blocks];
    if ((int)threadIdx.x < SS) {
        const int j = threadIdx.x;
        const int64_t bj = (int64_t)b * SS + j;
        int chunk = -1, k = 0;
        if (!(p.u_mix[bj] > 0.1f)) {
            p.coords[side][2 * bj] = p.reg[side][2 * bj];
            p.coords[side][2 * bj + 1] = p.reg[side][2 * bj + 1];
        } else {
            const float* u = p.u + (((int64_t)side * p.B + b) * SS + j) * 3;
            if (c == 0) {
                const int y = min((int)(u[1] * fH), H - 1);
                const int x = min((int)(u[2] * fH), H - 1);
                p.coords[side][2 * bj] = (float)x / fH * 2.0f - 1.0f;
                p.coords[side][2 * bj + 1] = (float)y / fH * 2.0f - 1.0f;
            } else {
                const uint32_t r = (uint32_t)min((int)(u[0] * (float)c), c - 1);
                int lo = 0, hi = n_blocks - 1;                 // the last block whose prefix is <= r: it holds rank r
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (block_pre[mid] <= r) lo = mid; else hi = mid - 1;
                }
                const uint32_t rem = r - block_pre[lo];
                int clo = lo << 6, chi = min(clo + 63, n_chunks - 1);
                while (clo < chi) {
                    const int mid = (clo + chi + 1) >> 1;
                    if (chunk_pre[mid] <= rem) clo = mid; else chi = mid - 1;
                }
                chunk = clo;
                k = (int)(rem - chunk_pre[clo]);
            }
        }
        sel_chunk[j] = chunk;
        sel_k[j] = k;
    }
    __syncthreads();

    // ---- pass 3: the k-th set bit of the sample's chunk
    const int W = p.W;
    for (int j = wave; j < SS; j += WAVES) {
        const int chunk = sel_chunk[j];
        if (chunk < 0) continue;                               // wave-uniform
        const int k = sel_k[j];
        const int px = (chunk << 6) + lane;
        const bool nz = px < n && nonzero_at<F32>(mask, base + px);
        const uint64_t bits = __ballot(nz);
        const int below = __popcll(bits & ((1ull << lane) - 1ull));
        if (nz && below == k) {
            const int y = px / W, x = px - y * W;
            const int64_t bj = (int64_t)b * SS + j;
            p.coords[side][2 * bj] = (float)x / fH * 2.0f - 1.0f;
            p.coords[side][2 * bj + 1] = (float)y / fH * 2.0f - 1.0f;
        }
    }
}

using stego::aligned;
using stego::hip_rc;

}  // namespace

extern "C" int stego_salience_coords(const StegoSalienceDesc* desc, const void* mask1, const void* mask2, const float* u, const float* u_mix,
                                     const float* reg1, const float* reg2, float* coords1, float* coords2, stego_stream_t stream)
{
    if (!desc) return STEGO_ERR_NULL;
    if (desc->S < 1 || desc->S > STEGO_SALIENCE_MAX_S) return STEGO_ERR_SALIENCE_SAMPLES;
    if (desc->B < 1 || desc->B > STEGO_SALIENCE_MAX_B || desc->H < 1 || desc->W < 1 ||
        (int64_t)desc->H * desc->W > STEGO_SALIENCE_MAX_PIXELS)
        return STEGO_ERR_SALIENCE_SIZE;
    if (desc->mask_dtype != STEGO_SALIENCE_U8 && desc->mask_dtype != STEGO_SALIENCE_F32) return STEGO_ERR_SALIENCE_DTYPE;
    if (!mask1 || !mask2 || !u || !u_mix || !reg1 || !reg2 || !coords1 || !coords2) return STEGO_ERR_NULL;
    const bool f32 = desc->mask_dtype == STEGO_SALIENCE_F32;
    if ((f32 && (!aligned(mask1, 4) || !aligned(mask2, 4))) || !aligned(u, 4) || !aligned(u_mix, 4) || !aligned(reg1, 4) ||
        !aligned(reg2, 4) || !aligned(coords1, 4) || !aligned(coords2, 4))
        return STEGO_ERR_ALIGN;
    SalParams p{{mask1, mask2}, u, u_mix, {reg1, reg2}, {coords1, coords2}, desc->B, desc->H, desc->W, desc->S * desc->S};
    const dim3 grid((unsigned)desc->B, 2u);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (f32) return hip_rc(stego::launch_first<salience_draw_kernel<true>>(grid, TPB, 0, s, p));
    return hip_rc(stego::launch_first<salience_draw_kernel<false>>(grid, TPB, 0, s, p));
}
