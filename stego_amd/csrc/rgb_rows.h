// Packed RGB rows at a byte-strided target, shared by render.hip and feature_pca.hip.  A workgroup of 256 threads owns RGB_ROWS rows of
// one image times one chunk: RGB_CHUNK bytes of every row counted from the row's own 16-byte aligned address A_r = row address & ~15,
// so chunk c of row r is the aligned global range [A_r + 768 c, A_r + 768 (c + 1)).  The pixels of a row that a chunk holds shift by up
// to 15 bytes from row to row (the target's strides have byte alignment only), and a pixel that straddles two chunks is computed by both.
// The kernel puts each pixel's three bytes into the row's stage in LDS (put_pixel at pixel_place); after a barrier store_rows sends the
// stage out as 16-byte stores of aligned addresses, and a 16-byte piece that the row covers only in part - the row's head and tail - as
// byte stores of the covered bytes.  Nothing outside the B x H x 3W panel bytes is written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));       // 16 bytes of a lane

constexpr int ROWS = 16;                 // rows of a workgroup
constexpr int CHUNK = 768;               // bytes of a row per workgroup: 48 pieces of 16 bytes, 256 pixels
constexpr int PIECES = CHUNK / 16;
constexpr int CPIX = CHUNK / 3;          // 256
constexpr int PIX_BACK = 5;              // a chunk's first pixel is at most (15 + 2) / 3 pixels in front of 256 c
constexpr int PIX_SPAN = CPIX + PIX_BACK;

__device__ __forceinline__ uint32_t to_level(float f)
{
    const float p = f * 255.f;
    return (uint32_t)(int)fminf(fmaxf(p, 0.f), 255.f);       // fmaxf(NaN, 0) = 0; the conversion truncates
}

// the first byte of pixel x of the row at `row` in chunk c; the pixel has bytes in the chunk when -2 <= at < CHUNK
__device__ __forceinline__ int pixel_place(const uint8_t* row, int x, int c)
{
    return 3 * x + (int)(reinterpret_cast<uintptr_t>(row) & 15) - c * CHUNK;
}

// R | G << 8 | B << 16 into the row's stage at `at`
__device__ __forceinline__ void put_pixel(uint8_t* stage_row, int at, uint32_t px)
{
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (at + k >= 0 && at + k < CHUNK) stage_row[at + k] = (uint8_t)(px >> (8 * k));
}

// the stage [ROWS][CHUNK] of chunk c of rows y0 .. y0 + ROWS of the image at out_b, by TPB threads
template <int TPB>
__device__ __forceinline__ void store_rows(uint8_t* out_b, int64_t osh, const uint8_t* stage, int c, int y0, int H, int W)
{
    const int row_bytes = 3 * W;
    for (int i = threadIdx.x; i < ROWS * PIECES; i += TPB) {
        const int r = i / PIECES, s = i - r * PIECES, y = y0 + r;
        if (y >= H) continue;
        uint8_t* const row = out_b + (int64_t)y * osh;
        const int a = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        const int q = c * CHUNK + 16 * s;                                // the piece, in bytes from the row's aligned address
        const int from = q > a ? q : a, to = q + 16 < a + row_bytes ? q + 16 : a + row_bytes;
        if (from >= to) continue;
        uint8_t* const g = row - a + q;                                  // 16-byte aligned
        const uint8_t* const l = stage + r * CHUNK + 16 * s;
        if (to - from == 16) {
            *reinterpret_cast<u32x4*>(g) = *reinterpret_cast<const u32x4*>(l);
        } else {
            for (int k = from - q; k < to - q; ++k) {
                g[k] = l[k];
                asm volatile("" ::: "memory");            // byte stores as written: no wide copy of an unaligned run
            }
        }
    }
}

}  // namespace
