// Dense feature correspondence, streaming form (round 6)  out[n,h,w,i,j] = sum_c a[n,c,h,w] * b[n,c,i,j]  (gfx950).
//
//   reference: tensor_correlation() src/modules.py:283-284 = einsum("nchw,ncij->nhwij") on norm()'ed maps (:275-276); the full-resolution
//              callers are plot_dino_correspondence.py:39-58 / plot_pr_curves.py:108-121.  SURVEY.md 8(f) rank 3.
//
// dense_corr.hip's row-block kernel (round 4 / 5) reads B operands that a prep launch wrote (read 38.5 MB, write 43 MB: 28 us at
// [32,784,784] C = 384), streams them with LDS-DMA behind one barrier per chunk, every wave reading its fragments and multiplying in
// lockstep, and drains its stores after every block: 93 us.  This kernel keeps its decomposition - one workgroup of four 512-register
// waves per (image, 128-pixel block of A), the A block as split-fp16 MFMA fragments in registers (192 VGPRs), wave w owns rows
// 32 w .. 32 w + 31 against all 128 columns of a B block - and changes the stream:
//   * B is read as it lies (fp32, channels-last): lane (q, s) holds 16 bytes of eight rows of the chunk on its way, scales them by the
//     row's 1 / ||b|| x power of two (the only thing a small launch in front computes: dense_stats_kernel, two floats per pixel), splits
//     into fp16 hi / lo, stores a row pair into one of TWO LDS stages behind each k-step's MFMAs and reloads its registers with the chunk
//     after next at once (one register set, a whole chunk of latency).  No operand image in memory at all.
//   * the A block comes in the same way, every chunk in flight at once, branch-free, and passes through the two stages into fragments;
//   * ONE set of B fragments (32 registers) is reloaded as it dies, the order pinned by sched_barrier (the scheduler, short of registers,
//     otherwise sinks every read to just in front of its MFMA; two sets in flight spill inside the loop);
//   * the whole-block chunk is ONE basic block (what varies is compile-time; the stream runs one chunk past its end on clamped addresses);
//   * the 32 x 128 slab of a wave is parked in a region of its own right after the block's last MFMA and leaves in sixteen 16-byte
//     stores per lane DURING the next block's first chunk (two whole 512-byte rows per instruction); nothing waits for a store.
// Same arithmetic as the row-block kernel: hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16, fp32 accumulate, the rows' power-of-two
// staging scales divided out at the park.  Measured 122 -> 98 us; where a chunk's 1.7 us go, and the four other forms that were built
// and measured no faster: DESIGN.md 4.6c, profiles/r06_dense_attempts.txt (the conversion's ~150 VALU instructions per chunk do NOT
// hide behind the MFMAs: a SIMD has room for ~4 plain / 2 packed VALU instructions per MFMA, tools/ubench/mfma_beside.hip).
#include "corr_common.h"
#include "host_util.h"
#include "launchers.h"
#include <type_traits>

namespace stego {

struct DenseStreamParams {
    MapV a, b;                  // [B,C,H1,W1], [B,C,H2,W2], channels-last (sc == 1), 16-byte aligned pixels
    float* out;                 // [B][M][N]
    float* invB;                // [B][nbB*128]  multiplier of a B row in front of the split: 1 / max(||b||, eps) (or 1) x power of two (0 behind the map)
    float* rsB;                 // [B][nbB*128]  1 / that power of two
    int B, C, M, N, W1, W2, nbA, nbB, normalize;
    int dbg;                    // (tools: bit 16 - every workgroup leaves its phase stamps over the first floats of its first output row)
};

#ifndef DS_ABL
#define DS_ABL 0                                    // (tools/ubench/dense_stream_bench.hip: compile-time timing ablations of the whole-block chunk)
#endif
constexpr int DS_STAGE = 2 * TP * LDH * 2;          // bytes of one LDS stage: hi[128][72] + lo[128][72] fp16
constexpr int DS_PKS = 132;                         // floats per parked row (528 B: conflict-free 16-byte reads along a row)
constexpr int DS_PARK = 32 * DS_PKS * 4;            // one wave's parked 32 x 128 slab
constexpr int DS_LDS = 2 * DS_STAGE + 4 * DS_PARK + TP * 4;              // + 1 / row scale of the A block

// one half-wave per pixel of b, four pixels in flight per half-wave: invB / rsB as dense_prep_kernel computes them (same sums in the same order)
__global__ void __launch_bounds__(NTHREADS) dense_stats_kernel(const DenseStreamParams prm)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int hl = lane & 31, hw = tid >> 5;
    const int rows_pad = prm.nbB * TP;
    const long long total = (long long)prm.B * rows_pad;
    constexpr int RPH = 4;                           // rows per half-wave
    const long long r0 = ((long long)blockIdx.x * 8 + hw) * RPH;
    constexpr int MAXJ = 3;                          // C <= 384
    f32x4 v[RPH][MAXJ];
    bool rv[RPH];
#pragma unroll
    for (int q = 0; q < RPH; ++q) {
        const long long row = r0 + q;
        const int n = (int)(row / rows_pad), pix = (int)(row - (long long)n * rows_pad);
        rv[q] = row < total && pix < prm.N;
        const int hh = rv[q] ? pix / prm.W2 : 0, ww = rv[q] ? pix - hh * prm.W2 : 0;
        const float* x = prm.b.p + (long long)(rv[q] ? n : 0) * prm.b.sn + (long long)hh * prm.b.sh + (long long)ww * prm.b.sw;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            const int c = 128 * j + 4 * hl;
            v[q][j] = (rv[q] && c < prm.C) ? *reinterpret_cast<const f32x4*>(x + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int q = 0; q < RPH; ++q) {
        float ss = 0.f, mx = 0.f;
#pragma unroll
        for (int j = 0; j < MAXJ; ++j) {
            ss += v[q][j][0] * v[q][j][0] + v[q][j][1] * v[q][j][1] + v[q][j][2] * v[q][j][2] + v[q][j][3] * v[q][j][3];
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v[q][j][0]), fabsf(v[q][j][1])), fmaxf(fabsf(v[q][j][2]), fabsf(v[q][j][3]))));
        }
#pragma unroll
        for (int s2 = 16; s2 >= 1; s2 >>= 1) { ss += __shfl_xor(ss, s2, 64); mx = fmaxf(mx, __shfl_xor(mx, s2, 64)); }
        float inv = prm.normalize ? 1.f / fmaxf(sqrtf(ss), 1e-10f) : 1.f;              // norm(), modules.py:276
        const float rs = mx * inv > 0.f ? __builtin_ldexpf(1.f, -__builtin_amdgcn_frexp_expf(mx * inv)) : 1.f;
        const long long row = r0 + q;
        if (hl == 0 && row < total) {
            prm.invB[row] = rv[q] ? inv * rs : 0.f;
            prm.rsB[row] = 1.f / rs;
        }
    }
}

// grid = ceil(B / 8) * 8 * nbA, block = 256 (4 waves, 512 registers each); image n on XCD n % 8 (its workgroups stream the same B map)
template <int NCH>
__global__ void __launch_bounds__(NTHREADS) dense_stream_kernel(const DenseStreamParams prm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* ra_s = reinterpret_cast<float*>(smem + 2 * DS_STAGE + 4 * DS_PARK);        // [128] 1 / row scale of the A block
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = prm.C;
    const int x = blockIdx.x & 7, sl = blockIdx.x >> 3;
    const int n = (sl / prm.nbA) * 8 + x, mi = sl % prm.nbA;
    if (n >= prm.B) return;
    const int r = lane & 31, half = lane >> 5;
    unsigned long long ts[8];
    ts[0] = __builtin_amdgcn_s_memrealtime();

    // ---- the B stream: chunk g = nj * NCH + c.  Lane (q = lane >> 4, s = lane & 15) of wave w converts, for i = 0..7, channels 4 s .. 4 s + 3
    // of the chunk of row 32 w + 4 i + q of the block: a wave instruction reads four whole 256-byte runs.  Everything here is branch-free:
    // pixels beyond N and channels beyond C are read from a clamped address and multiplied by zero (invB is 0 behind the map's last pixel).
    const int q4 = lane >> 4, s16 = lane & 15;
    const int G = prm.nbB * NCH;
    const float* bimg = prm.b.p + (long long)n * prm.b.sn;                 // (dense pixel stride: pixel p lies at p * sw - dense_corr_kernel: b.sh == W2 * b.sw)
    const unsigned bsw4 = 4u * (unsigned)prm.b.sw;
    const float* invn = prm.invB + (size_t)n * prm.nbB * TP + 32 * wave + q4;
    float binv[8];                                   // multipliers of my eight pixels, for the block being CONVERTED (dense_stats_kernel; 0 behind the map)
    auto block_scales = [&](int nj) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) binv[i] = invn[nj * TP + 4 * i];
    };
    f32x4 raw[8];                                    // my eight 16-byte pieces of the chunk on its way: a row pair is reloaded (chunk g + 2) right
                                                     // after it was converted (chunk g + 1) - one register set, a whole chunk of latency
    auto load_rows = [&](int nj, int c, int i0, int i1) __attribute__((always_inline)) {
        // (uniform base + 32-bit UNSIGNED lane offset - no 64-bit lane pointers to keep alive.  dense_corr_kernel sends a map here only if
        // (N - 1) * 4 sw + 4 C <= 2^32: the clamp comes before the product, so no offset is beyond the last pixel's last channel)
        const unsigned cho = 4u * (unsigned)min(64 * c + 4 * s16, C - 4);
        const int p0 = nj * TP + 32 * wave + q4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < i0 || i >= i1) continue;
            const unsigned off = (unsigned)min(p0 + 4 * i, prm.N - 1) * bsw4 + cho;
            raw[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(bimg) + off);
        }
    };
    // rows 4 i + q of my wave's 32, i in [i0, i1), of chunk cn of a block: scale, split, two 8-byte LDS stores per row
    auto convert_rows = [&](unsigned char* stage, int i0, int i1, int nb, int cn) __attribute__((always_inline)) {
        (void)nb;
        const float chmask = (cn == NCH - 1 && 64 * cn + 4 * s16 >= C) ? 0.f : 1.f;       // channels beyond C (the last chunk only)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < i0 || i >= i1) continue;
            const float sc = cn == NCH - 1 ? binv[i] * chmask : binv[i];
            unsigned h0, l0, h1, l1;
            split_f16_pair(raw[i][0] * sc, raw[i][1] * sc, h0, l0);
            split_f16_pair(raw[i][2] * sc, raw[i][3] * sc, h1, l1);
            half_t* dh = reinterpret_cast<half_t*>(stage) + (32 * wave + 4 * i + q4) * LDH + 4 * s16;
            *reinterpret_cast<u32x2*>(dh) = u32x2{h0, h1};
            *reinterpret_cast<u32x2*>(dh + TP * LDH) = u32x2{l0, l1};
        }
    };

    float* outn = prm.out + (size_t)n * prm.M * prm.N;
    float* park = reinterpret_cast<float*>(smem + 2 * DS_STAGE) + wave * (32 * DS_PKS);
    const bool live = mi * TP + 32 * wave < prm.M;                // (a wave whose rows are all beyond M converts and keeps the barriers)
    const bool rows_full = mi * TP + 32 * wave + 32 <= prm.M;
    const bool v4 = (prm.N & 3) == 0;
    constexpr int LO = TP * LDH;
    const float* prd = park + half * DS_PKS + 4 * r;              // my 16 bytes of row pair k: prd + 2 k DS_PKS
    const unsigned ordo = 4u * ((unsigned)(mi * TP + 32 * wave + half) * (unsigned)prm.N + 4u * r);      // byte offset of my piece of row pair 0 (dense_corr_kernel: an image's output is <= 2^32 bytes; rows beyond M may wrap, they are never stored)
    const unsigned rowp = 8u * (unsigned)prm.N;                  // bytes between row pairs

    // row pairs [k0, k1) of the sixteen of the parked slab of block njp: row 2 k + half, columns 4 r .. 4 r + 3 (one 512-byte run per half-wave)
    auto store_rows = [&](int njp, int k0, int k1, bool full) __attribute__((always_inline)) {
        if (full) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < k0 || k >= k1) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(prd + 2 * k * DS_PKS);
                __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(reinterpret_cast<char*>(outn) + (ordo + k * rowp + 4u * (unsigned)(njp * TP))));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < k0 || k >= k1) continue;
                const int row = mi * TP + 32 * wave + 2 * k + half, col = njp * TP + 4 * r;
                const f32x4 v = *reinterpret_cast<const f32x4*>(prd + 2 * k * DS_PKS);
                if (row < prm.M) {
                    float* o = reinterpret_cast<float*>(reinterpret_cast<char*>(outn) + (ordo + k * rowp + 4u * (unsigned)(njp * TP)));
                    if (v4) {
                        if (col < prm.N) __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(o));
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (col + e < prm.N) __builtin_nontemporal_store(v[e], o + e);
                    }
                }
            }
        }
    };

    // ---- the A block -> MFMA fragments in registers (lane (r, half) holds channels 16 ks + 8 half .. + 7 of every 64-channel chunk of row
    // 32 w + r).  The block comes in the way the B chunks do - lane (q, s) reads 16 bytes of eight rows per chunk, four whole 256-byte runs
    // per wave instruction, all NCH chunks in flight at once -, gets its row statistics by shuffles inside the 16-lane groups, and passes
    // through the two LDS stages in the split-fp16 chunk layout, from which every lane takes its fragments with conflict-free 16-byte reads.
    // (The row-block kernel had each lane read its own row in 32-byte pieces, twice, behind a branch and a full wait per piece: ~25
    // serialized cold round trips + every line pulled into the L1 four times: 40 us of its 93.)
    f16x8 Ah[NCH][KC / 16], Al[NCH][KC / 16];
    block_scales(0);
    load_rows(0, 0, 0, 8);                           // B's first chunk rides along
    {
        const float* aimg = prm.a.p + (long long)n * prm.a.sn;
        f32x4 ar[NCH][8];
        const float* arow[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int pc = min(mi * TP + 32 * wave + 4 * i + q4, prm.M - 1);
            const int hh = pc / prm.W1, ww = pc - hh * prm.W1;
            arow[i] = aimg + (long long)hh * prm.a.sh + (long long)ww * prm.a.sw;
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int ch = min(64 * c + 4 * s16, C - 4);
#pragma unroll
            for (int i = 0; i < 8; ++i) ar[c][i] = *reinterpret_cast<const f32x4*>(arow[i] + ch);
        }
        const float lastmask = (64 * (NCH - 1) + 4 * s16 >= C) ? 0.f : 1.f;       // channels beyond C (the last chunk only)
        float ainv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float ss = 0.f, mx = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const f32x4 v = ar[c][i];
                const float s4 = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
                const float m4 = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
                ss += c == NCH - 1 ? s4 * lastmask : s4;
                mx = fmaxf(mx, c == NCH - 1 ? m4 * lastmask : m4);
            }
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) { ss += __shfl_xor(ss, m, 64); mx = fmaxf(mx, __shfl_xor(mx, m, 64)); }
            float inv = prm.normalize ? 1.f / fmaxf(sqrtf(ss), 1e-10f) : 1.f;        // norm(), modules.py:276
            const float rs = mx * inv > 0.f ? __builtin_ldexpf(1.f, -__builtin_amdgcn_frexp_expf(mx * inv)) : 1.f;
            const int rl = 32 * wave + 4 * i + q4;
            ainv[i] = mi * TP + rl < prm.M ? inv * rs : 0.f;                       // (rows beyond M: the map's last pixel times zero)
            if (s16 == 0) ra_s[rl] = 1.f / rs;
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            unsigned char* stage = smem + (c & 1) * DS_STAGE;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float sc = c == NCH - 1 ? ainv[i] * lastmask : ainv[i];
                unsigned h0, l0, h1, l1;
                split_f16_pair(ar[c][i][0] * sc, ar[c][i][1] * sc, h0, l0);
                split_f16_pair(ar[c][i][2] * sc, ar[c][i][3] * sc, h1, l1);
                half_t* dh = reinterpret_cast<half_t*>(stage) + (32 * wave + 4 * i + q4) * LDH + 4 * s16;
                *reinterpret_cast<u32x2*>(dh) = u32x2{h0, h1};
                *reinterpret_cast<u32x2*>(dh + TP * LDH) = u32x2{l0, l1};
            }
            __syncthreads();                         // the chunk is whole (and everybody has read the stage's previous tenant: see above)
            const half_t* ap = reinterpret_cast<const half_t*>(stage) + (32 * wave + r) * LDH + 8 * half;
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                Ah[c][ks] = *reinterpret_cast<const f16x8*>(ap + 16 * ks);
                Al[c][ks] = *reinterpret_cast<const f16x8*>(ap + TP * LDH + 16 * ks);
            }
        }
    }
    __syncthreads();                                 // the stages are free; ra_s
    ts[1] = __builtin_amdgcn_s_memrealtime();
    convert_rows(smem, 0, 8, 0, 0);                  // B's chunk 0 into stage 0
    load_rows(0, 1, 0, 8);                           // chunk 1 on its way
    __syncthreads();

    int pending = -1;                                // block whose slab is parked and not yet stored
    bool pending_full = false;
    float rbv[4];                                    // 1 / staging scale of my four columns of the block being multiplied
    int g = 0;
    // One chunk of a WHOLE block (all four 32-column groups exist: every block in front of the map's last, partial one).  The body is one
    // basic block - no run-time condition inside - so that the scheduler can put the conversion's VALU work, the LDS traffic and the
    // previous slab's stores between the MFMAs (a wave issues in order: what stands behind the last MFMA of a k-step waits for all of
    // them): chunk g + 2 is ALWAYS loaded and chunk g + 1 ALWAYS converted (behind the stream's end: clamped addresses, a stage nobody
    // reads), whether the previous slab is stored (every block but the first) and whether my 32 rows all exist are compile-time flags.
    auto fast_chunk = [&](auto firstc, auto fullc, const int nj, const int c, f32x16 (&acc)[4]) __attribute__((always_inline)) {
        constexpr bool FIRST = decltype(firstc)::value, ROWS_FULL = decltype(fullc)::value;
        unsigned char* Sg = smem + (g & 1) * DS_STAGE;
        unsigned char* Sn = smem + ((g + 1) & 1) * DS_STAGE;
        if (!(FIRST && c == 0)) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();            // stage g & 1 is complete, the other one has been read
            asm volatile("" ::: "memory");
        }
        const int cn = (c + 1) % NCH;                // the place of chunk g + 1 in its block (unrolled: a constant)
        const int nb = c + 1 == NCH ? nj + 1 : nj;   // and its block
        if (c + 1 == NCH) block_scales(nj + 1);      // (behind the map's last block: the words in front of rsB - never multiplied)
        if (c == 0) {
            const float* rb = prm.rsB + ((size_t)n * prm.nbB + nj) * TP;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) rbv[ni] = rb[32 * ni + r];
        }
        const half_t* bp = reinterpret_cast<const half_t*>(Sg) + r * LDH + 8 * half;
        // ONE set of fragments (32 registers), reloaded as it dies: per k-step the eight MFMAs that need the hi fragments of B run first, the
        // next k-step's hi fragments are read into their registers under the four MFMAs that need the lo fragments, and those are re-read
        // right behind them.  sched_barrier pins that order (left alone, the scheduler - short of registers - sinks every read to just in
        // front of its MFMA: an LDS round trip exposed per MFMA, 1.9 us per chunk; two full sets in flight made it spill inside the loop).
        f16x8 bh[4], bl[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) bh[ni] = *reinterpret_cast<const f16x8*>(bp + ni * 32 * LDH);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) bl[ni] = *reinterpret_cast<const f16x8*>(bp + ni * 32 * LDH + LO);
#pragma unroll
        for (int ks = 0; ks < KC / 16; ++ks) {
            __builtin_amdgcn_sched_barrier(0);
            if (!(DS_ABL & 4)) {
                if (c == 0 && ks == 0) {
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[c][ks], bh[ni], f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                } else {
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[c][ks], bh[ni], acc[ni], 0, 0, 0);
                }
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al[c][ks], bh[ni], acc[ni], 0, 0, 0);
            }
            if (!(DS_ABL & (2 | 64))) convert_rows(Sn, 2 * ks, 2 * ks + 1, nb, cn);
            if (!(DS_ABL & (2 | 32))) load_rows(c + 2 >= NCH ? nj + 1 : nj, (c + 2) % NCH, 2 * ks, 2 * ks + 1);
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 1 < KC / 16 && !(DS_ABL & 1)) {
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) bh[ni] = *reinterpret_cast<const f16x8*>(bp + ni * 32 * LDH + 16 * (ks + 1));
            }
            __builtin_amdgcn_sched_barrier(0);
            if (!(DS_ABL & 4)) {
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[c][ks], bl[ni], acc[ni], 0, 0, 0);
            }
            if (!(DS_ABL & (2 | 64))) convert_rows(Sn, 2 * ks + 1, 2 * ks + 2, nb, cn);
            if (!(DS_ABL & (2 | 32))) load_rows(c + 2 >= NCH ? nj + 1 : nj, (c + 2) % NCH, 2 * ks + 1, 2 * ks + 2);
            if (c == 0 && !FIRST && !(DS_ABL & 8)) {
                if constexpr (ROWS_FULL) store_rows(nj - 1, 4 * ks, 4 * ks + 4, true);
                else if (pending >= 0) store_rows(nj - 1, 4 * ks, 4 * ks + 4, false);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (ks + 1 < KC / 16 && !(DS_ABL & 1)) {
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) bl[ni] = *reinterpret_cast<const f16x8*>(bp + ni * 32 * LDH + LO + 16 * (ks + 1));
            }
        }
        if (c == 0) pending = -1;
        ++g;
    };
    // One chunk of the map's last, partial block: the nlive groups that exist, one after the other (accumulators of its own: sharing them
    // with the whole blocks' form made the compiler copy all 64 registers between the two allocations in every chunk).
    auto tail_chunk = [&](const int nj, const int c, f32x16 (&acc)[4], const int nlive) __attribute__((always_inline)) {
        unsigned char* Sg = smem + (g & 1) * DS_STAGE;
        unsigned char* Sn = smem + ((g + 1) & 1) * DS_STAGE;
        if (g > 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        // (only the rows of the block that exist are converted: the waves behind them have nothing to do but the barriers)
        const bool conv = g + 1 < G && nj * TP + 32 * wave < prm.N;
        const int cn = (c + 1) % NCH;
        if (c == 0) {
            const float* rb = prm.rsB + ((size_t)n * prm.nbB + nj) * TP;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) rbv[ni] = rb[32 * ni + r];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[ni][e] = 0.f;
        }
        const half_t* bp = reinterpret_cast<const half_t*>(Sg) + r * LDH + 8 * half;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            if (ni < nlive) {
#pragma unroll
                for (int ks = 0; ks < KC / 16; ++ks) {
                    const f16x8 bh = *reinterpret_cast<const f16x8*>(bp + ni * 32 * LDH + 16 * ks);
                    const f16x8 bl = *reinterpret_cast<const f16x8*>(bp + ni * 32 * LDH + LO + 16 * ks);
                    acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al[c][ks], bh, acc[ni], 0, 0, 0);
                    acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[c][ks], bl, acc[ni], 0, 0, 0);
                    acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[c][ks], bh, acc[ni], 0, 0, 0);
                }
            }
        }
        if (conv) convert_rows(Sn, 0, 8, nj, cn);
        if (g + 2 < G && nj * TP + 32 * wave < prm.N) load_rows(c + 2 >= NCH ? nj + 1 : nj, (c + 2) % NCH, 0, 8);
        if (c == 0 && pending >= 0) store_rows(pending, 0, 16, pending_full);
        if (c == 0) pending = -1;
        ++g;
    };
    // park my 32 x 128 slab.  C/D layout: col = lane & 31 (+ 32 ni), row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    auto park_slab = [&](const int nj, const f32x16 (&acc)[4], const int nlive) __attribute__((always_inline)) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            if (ni < nlive) {
                const float sb = rbv[ni];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int rl = (e & 3) + 8 * (e >> 2) + 4 * half;
                    park[rl * DS_PKS + 32 * ni + r] = acc[ni][e] * (ra_s[32 * wave + rl] * sb);
                }
            }
        }
        pending = nj;
        pending_full = rows_full && v4 && nj * TP + TP <= prm.N;
    };

    const int nfull = prm.N / TP;                    // whole 128-pixel blocks of B
    // the whole blocks, for a wave whose 32 rows all exist (unguarded 16-byte stores; needs N % 4 == 0) or not
    auto whole_blocks = [&](auto fullc) __attribute__((always_inline)) {
        constexpr bool ROWS_FULL = decltype(fullc)::value;
        f32x16 acc[4];
        auto full_block = [&](auto firstc, const int nj) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) fast_chunk(firstc, fullc, nj, c, acc);
            if (ROWS_FULL || live) park_slab(nj, acc, 4);         // (a wave whose rows are all beyond M multiplied zeros)
        };
        if (nfull > 0) full_block(std::true_type{}, 0);
        ts[2] = __builtin_amdgcn_s_memrealtime();
        for (int nj = 1; nj < nfull; ++nj) full_block(std::false_type{}, nj);
    };
    if (rows_full && v4) whole_blocks(std::true_type{}); else whole_blocks(std::false_type{});
    ts[3] = ts[2];
    ts[4] = __builtin_amdgcn_s_memrealtime();
    if (nfull < prm.nbB) {                           // the map's last pixels
        f32x16 acc[4];
        const int nlive = live ? (prm.N - nfull * TP + 31) >> 5 : 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) tail_chunk(nfull, c, acc, nlive);
        if (nlive > 0) park_slab(nfull, acc, nlive);
    }
    ts[5] = __builtin_amdgcn_s_memrealtime();
    if (pending >= 0) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        store_rows(pending, 0, 16, pending_full);
    }
    if (prm.dbg & 16) {                              // (tools: this workgroup's stamps over the first floats of its first output row)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ts[6] = __builtin_amdgcn_s_memrealtime();
        __syncthreads();
        if (tid == 0) {
            unsigned* o = reinterpret_cast<unsigned*>(outn + (size_t)(mi * TP) * prm.N);
            o[0] = (unsigned)ts[0];
#pragma unroll
            for (int k = 1; k < 7; ++k) o[k] = (unsigned)(ts[k] - ts[0]);
        }
    }
}

size_t dense_stream_workspace_bytes(int B, int N)
{
    return (size_t)2 * B * ((N + TP - 1) / TP) * TP * sizeof(float) + 512;
}

// the caller (launch_dense_corr) has asked dense_corr_kernel: channels-last maps, 16-byte aligned pixels, C % 8 == 0, 64 < C <= 384, B's pixels
// at a dense stride, and the two 32-bit offset limits of dense_stream_kernel (output bytes per image, B's largest byte offset)
hipError_t launch_dense_stream(const MapV& a, const MapV& b, int B, int C, int H1, int W1, int H2, int W2, int normalize, float* out, void* ws,
                               hipStream_t stream)
{
    DenseStreamParams prm{};
    prm.a = a; prm.b = b; prm.out = out;
    prm.B = B; prm.C = C; prm.M = H1 * W1; prm.N = H2 * W2; prm.W1 = W1; prm.W2 = W2;
    prm.nbA = (prm.M + TP - 1) / TP; prm.nbB = (prm.N + TP - 1) / TP;
    prm.normalize = normalize;
    prm.dbg = (knob(KNOB_DEBUG) >> 22) & 31;
    unsigned char* w = static_cast<unsigned char*>(ws);
    w += (256 - (reinterpret_cast<uintptr_t>(w) & 255)) & 255;
    prm.invB = reinterpret_cast<float*>(w);
    prm.rsB = prm.invB + (size_t)B * prm.nbB * TP;
    const long long rows = (long long)B * prm.nbB * TP;
    hipLaunchKernelGGL(dense_stats_kernel, dim3((unsigned)((rows + 31) / 32)), dim3(NTHREADS), 0, stream, prm);
    const int NCH = (C + KC - 1) / KC;
    const dim3 grid((unsigned)(((B + 7) / 8) * 8 * prm.nbA));
    auto go = [&](auto N) { return launch<dense_stream_kernel<N()>>(grid, dim3(NTHREADS), DS_LDS, stream, prm); };
#ifndef DS_ONLY6
    return with_const_strict<2, 3, 4, 5, 6>(NCH, go);
#else
    return with_const_strict<6>(NCH, go);
#endif
}

}  // namespace stego
