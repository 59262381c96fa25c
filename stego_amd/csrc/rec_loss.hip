// Fused reconstruction loss, forward and backward (include/stego_rec.h), in two launches that write no [T, C] tensor.
//
// Launch 1, rec_tiles<NT>: one workgroup of four waves per tile of 32 tokens (beyond 2048 tiles they walk them with the grid's stride).
//   A tile's codes xs [32][KP + 1] and features fs [CP][33] (channel-major) are put into LDS (KP, CP = K, C rounded up to 32, the padding
//   is zero; lanes run over the channels: coalesced when stride_c == 1), then, the 32-channel chunks of C dealt to the waves in turn:
//     pass 1: R = X W_chunk^T + b on v_mfma_f32_32x32x2_f32, the tile's codes as the A operand from LDS, the chunk's rows of W as the B
//       operand from registers (read once per chunk from the cached weight): the accumulator has the channel on the lane and the 32
//       tokens in its registers.  |r|^2, r . f and |f|^2 are summed per register, then over the lanes and the waves in a fixed order:
//       per token alpha = -1 / (T nf nr), beta = [|r| >= eps] c / (T nr^2), so that g = alpha f + beta r.  One fp64 loss term per tile;
//       with d_weight or d_bias asked for, alpha and beta of every token go to the workspace.
//     pass 2 (with d_code): R again, bit for bit, G = alpha F + beta R over F in LDS, element by element, by the lane that read it.
//     d_code tile = G W: wave nt < NT owns 32 code channels, G from LDS as the A operand (token on the lane), rows of W as the B
//       operand (coalesced, from the cache); written with d_code's own strides.
// Launch 2, rec_finish<NT>: d_weight / d_bias by workgroups (token range of 64, 32-channel chunk) whose accumulators stay in registers
//   over all their tiles, the ranges' partials added in ascending order by the workgroup that finishes a chunk last (described at the
//   kernel); one more workgroup adds the tiles' loss terms in a fixed order in fp64.
// No float atomics anywhere: repeat launches give the same bits.  Every offset into a map or the workspace is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/stego_rec.h"
#include "addon_device.h"
#include "host_util.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TILE = STEGO_REC_TILE, TPB = 256, WAVES = TPB / 64, FIN_TPB = 256;
constexpr float EPS = 1e-10f;
constexpr int TILES_MAX_WG = 2048;          // workgroups of launch 1: one per tile up to here, then the grid's stride

struct RecParams {
    StegoMap code, feats, dcode;         // dcode.data == nullptr: no d_code
    const float *weight, *bias;
    float *slabs, *gscal, *loss, *d_weight, *d_bias;   // gscal [T][2]: alpha, beta of every token (written with d_weight / d_bias)
    double* tile_part;
    unsigned* counters;                  // [CP / 32]: the ranges of a chunk that have written their partial; zeroed by launch 1
    int32_t B, K, C, h, w, T, CP, n_tiles, n_wg, n_rg, wgrad;
    float inv_t;
};

// A value the tile loop needs once per tile, moved to a vector register: the loop's scalar registers are for what its inner loops use.
template <class V>
__device__ inline V cold(V v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// what token_offset needs of a map
struct TokenStrides { int64_t n, h, w; };

__device__ inline TokenStrides cold_strides(const StegoMap& m) { return {cold(m.stride_n), cold(m.stride_h), cold(m.stride_w)}; }

__device__ inline int64_t token_offset(const TokenStrides& m, int tg, int hw, int w)
{
    const int b = tg / hw, rem = tg - b * hw, y = rem / w, x = rem - y * w;
    return (int64_t)b * m.n + (int64_t)y * m.h + (int64_t)x * m.w;
}

// a tile of a map into LDS, element (token, channel) at token * ts + channel * cs; channels [0, n) from memory, [n, np) and the tokens
// from T on zero.  The lanes run over the channels: coalesced for stride_c == 1, correct for every other layout.
__device__ inline void load_tile(const float* data, int64_t stride_c, const long long* base, float* dst, int ts, int cs, int n, int np, int valid, int t)
{
    constexpr int ROWS = TILE / WAVES;                   // a wave's tokens: their loads are all in flight before the first store
    const int wave = t >> 6, lane = t & 63;
    const float* src[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) src[j] = data + base[wave + WAVES * j];
    for (int c = lane; c < np; c += 64) {
        float v[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; ++j) v[j] = (wave + WAVES * j < valid && c < n) ? src[j][(int64_t)c * stride_c] : 0.f;
#pragma unroll
        for (int j = 0; j < ROWS; ++j) dst[(wave + WAVES * j) * ts + c * cs] = v[j];
    }
}

template <int NT>
__device__ inline f32x16 r_chunk(const float* xa, const float (&wreg)[16 * NT], float bias_c)
{
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = bias_c;
#pragma unroll
    for (int kk = 0; kk < 16 * NT; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * kk], wreg[kk], acc, 0, 0, 0);
    return acc;
}

// The weight through a buffer descriptor of its C K floats: a read beyond the end gives 0, so rows from C on are zero rows with no test.
// A read beyond a row's K lands in the next row, where the other operand is the zero padding of xs / the result is never stored.  A
// non-finite weight there would reach this row through 0 * inf - in a call whose every output is NaN already: each token's |r| takes
// every row of W, and the loss and all three gradients take every token's |r|.
__device__ inline float load_w(const __amdgpu_buffer_rsrc_t& rsrc, int elem)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, elem * 4, 0, 0));
}

// the B operand of R = X W_chunk^T: B[k = 2 kk + hf][j = li] = W[c][2 kk + hf]
template <int NT>
__device__ inline void load_w_rows(const __amdgpu_buffer_rsrc_t& rsrc, int row_elem, float (&wreg)[16 * NT])
{
#pragma unroll
    for (int kk = 0; kk < 16 * NT; ++kk) wreg[kk] = load_w(rsrc, row_elem + 2 * kk);
}

template <int NT>
__global__ __launch_bounds__(TPB) void rec_tiles(RecParams p)
{
    constexpr int KP = 32 * NT, KS = KP + 1, FS = TILE + 1;     // odd LDS row strides: the 32 lanes of a ds_read_b32 group hit 32 banks
    extern __shared__ float4 smem4[];
    long long* cbase = reinterpret_cast<long long*>(smem4);    // [TILE] offsets of the tile's tokens in code, feats and d_code
    long long* fbase = cbase + TILE;
    long long* dbase = fbase + TILE;
    float* xs = reinterpret_cast<float*>(dbase + TILE);        // [TILE][KS]
    float* part = xs + TILE * KS;                       // [WAVES][TILE][3]
    float* scal = part + WAVES * TILE * 3;              // [TILE][2]: alpha, beta
    float* ct = scal + TILE * 2;                        // [TILE]: c_t
    float* fs = ct + TILE;                              // [CP][FS]: channel-major, every offset of a token a constant; the one
                                                        // array of a run-time size comes last, so every other address is a constant

    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, li = lane & 31, hf = lane >> 5;
    const int n_chunks = p.CP / 32;
    const int hw = cold(p.h * p.w), wd = cold(p.w);
    const TokenStrides code_s = cold_strides(p.code), feats_s = cold_strides(p.feats), dcode_s = cold_strides(p.dcode);
    const bool want_dcode = p.dcode.data != nullptr;
    double* tile_part = cold(p.tile_part);
    float* gscal = cold(p.gscal);
    if (blockIdx.x == 0 && p.wgrad && t < n_chunks) p.counters[t] = 0u;
    // this lane's column of d_code in the last stage: code channel 32 wave + li
    float* dcode_col = const_cast<float*>(p.dcode.data) + (int64_t)(wave * 32 + li) * p.dcode.stride_c;
    const float* code_data = cold(p.code.data);
    const float* feats_data = cold(p.feats.data);
    const int64_t code_sc = cold(p.code.stride_c), feats_sc = cold(p.feats.stride_c);
    const float* bias = cold(p.bias);
    const float inv_t = cold(p.inv_t);
    const int n_tok = cold(p.T);
    const float* xa = xs + li * KS + hf;                // A[i = li][k = 2 kk + hf]
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.weight), 0, p.C * p.K * 4, 0x00020000);

    for (int tile = blockIdx.x; tile < p.n_tiles; tile += p.n_wg) {
        const int t0 = tile * TILE, valid = __builtin_amdgcn_readfirstlane(min(TILE, n_tok - t0));
        __syncthreads();                                // the previous tile's LDS has been read
        if (t < TILE) {
            const int tg = min(t0 + t, n_tok - 1);
            cbase[t] = token_offset(code_s, tg, hw, wd);
            fbase[t] = token_offset(feats_s, tg, hw, wd);
            dbase[t] = token_offset(dcode_s, tg, hw, wd);
        }
        __syncthreads();
        load_tile(code_data, code_sc, cbase, xs, KS, 1, p.K, KP, valid, t);
        load_tile(feats_data, feats_sc, fbase, fs, 1, FS, p.C, p.CP, valid, t);
        __syncthreads();

        // ---- pass 1: the three sums of every token
        float rr[16], rf[16], ff[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) rr[r] = rf[r] = ff[r] = 0.f;
#pragma unroll 1
        for (int ch = wave; ch < n_chunks; ch += WAVES) {
            const int c = ch * 32 + li;
            float wreg[16 * NT];
            load_w_rows<NT>(w_rsrc, c * p.K + hf, wreg);
            const f32x16 acc = r_chunk<NT>(xa, wreg, c < p.C ? bias[c] : 0.f);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float f = fs[c * FS + acc_row(r, hf)];
                rr[r] = fmaf(acc[r], acc[r], rr[r]);
                rf[r] = fmaf(acc[r], f, rf[r]);
                ff[r] = fmaf(f, f, ff[r]);
            }
        }
#pragma unroll
        for (int m = 16; m > 0; m >>= 1)
#pragma unroll
            for (int r = 0; r < 16; ++r) {              // within the lane half: the channels of one token
                rr[r] += __shfl_xor(rr[r], m);
                rf[r] += __shfl_xor(rf[r], m);
                ff[r] += __shfl_xor(ff[r], m);
            }
        if (li == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float* q = part + (wave * TILE + acc_row(r, hf)) * 3;
                q[0] = rr[r];
                q[1] = rf[r];
                q[2] = ff[r];
            }
        }
        __syncthreads();
        if (t < TILE) {
            float s_rr = 0.f, s_rf = 0.f, s_ff = 0.f;
#pragma unroll
            for (int wv = 0; wv < WAVES; ++wv) {
                const float* q = part + (wv * TILE + t) * 3;
                s_rr += q[0];
                s_rf += q[1];
                s_ff += q[2];
            }
            const float nrv = sqrtf(s_rr), nr = fmaxf(nrv, EPS), nf = fmaxf(sqrtf(s_ff), EPS);
            const float c = s_rf / (nr * nf);
            const bool live = t < valid;
            scal[2 * t] = live ? -inv_t / (nf * nr) : 0.f;
            scal[2 * t + 1] = (live && nrv >= EPS) ? inv_t * c / (nr * nr) : 0.f;
            ct[t] = live ? c : 0.f;
            if (live && p.wgrad) {
                gscal[2 * (int64_t)(t0 + t)] = scal[2 * t];
                gscal[2 * (int64_t)(t0 + t) + 1] = scal[2 * t + 1];
            }
        }
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int i = 0; i < TILE; ++i) s += (double)ct[i];
            tile_part[tile] = s;
        }
        if (!want_dcode) continue;

        // ---- pass 2: G = alpha F + beta R chunk by chunk, over F in LDS
#pragma unroll 1
        for (int ch = wave; ch < n_chunks; ch += WAVES) {
            const int c = ch * 32 + li;
            float wreg[16 * NT];
            load_w_rows<NT>(w_rsrc, c * p.K + hf, wreg);
            const f32x16 r2 = r_chunk<NT>(xa, wreg, c < p.C ? bias[c] : 0.f);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tok = acc_row(r, hf);
                float* fp = fs + c * FS + tok;
                *fp = fmaf(scal[2 * tok], *fp, scal[2 * tok + 1] * r2[r]);
            }
        }
        __syncthreads();                                // G of every chunk is in LDS

        // ---- d_code tile = G W: wave nt owns the code channels 32 nt .. + 31
        if (wave < NT) {
            const int k = wave * 32 + li;
            const bool in_k = k < p.K;
            const float* ga = fs + hf * FS + li;        // A[i = token li][k = channel 2 kk + hf]
            f32x16 dc;
#pragma unroll
            for (int r = 0; r < 16; ++r) dc[r] = 0.f;
            for (int k16 = 0; k16 < 16 * n_chunks; k16 += 16) {         // a chunk's 16 weight loads in flight together
#pragma unroll
                for (int kk = k16; kk < k16 + 16; ++kk)
                    dc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[2 * kk * FS], load_w(w_rsrc, (2 * kk + hf) * p.K + k), dc, 0, 0, 0);
            }
            if (in_k) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int tok = acc_row(r, hf);
                    if (tok < valid) dcode_col[dbase[tok]] = dc[r];
                }
            }
        }
    }
}

// d_weight / d_bias and the loss.  Workgroup (range rg, chunk ch) of the first n_rg * n_chunks: its four waves take the tiles
// rg, rg + n_rg, ... in turn, each wave on its own: R = X W_chunk^T + b again (bit for bit the R of launch 1), G = alpha F + beta R with
// the stored scalars, d_weight chunk += G^T X in NT accumulators that live in registers over all its tiles; codes and features come
// through a per-wave LDS tile, the features straight from memory in the accumulator layout (the second read of both, served from the
// caches: launch 1 has just read them).  The
// waves' accumulators are added in wave order through LDS and written as the range's partial; the workgroup that finds itself the last
// of its chunk (a counter that launch 1 zeroed) adds the n_rg partials in ascending order and writes the chunk of d_weight / d_bias.
// Whichever workgroup that is, the order of the sum is the same.
template <int NT>
__global__ __launch_bounds__(FIN_TPB) void rec_finish(RecParams p, int elem_blocks)
{
    __shared__ double red[FIN_TPB];
    constexpr int KP = 32 * NT, KS = KP + 1;
    constexpr int SUM_LEN = (WAVES - 1) * (NT * 16 + 1) * 64, XS_LEN = WAVES * TILE * KS;
    __shared__ float lds[SUM_LEN > XS_LEN ? SUM_LEN : XS_LEN];      // the waves' code tiles in the loop, their sums after it
    float* wsum = lds;
    __shared__ int is_last;
    const int t = threadIdx.x;
    if ((int)blockIdx.x >= elem_blocks) {               // the loss: the last block of the grid
        double s = 0.0;
        for (int i = t; i < p.n_tiles; i += FIN_TPB) s += p.tile_part[i];
        s = block_sum<FIN_TPB>(s, red);
        if (t == 0) p.loss[0] = (float)(-s / (double)p.T);
        return;
    }
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, li = lane & 31, hf = lane >> 5;
    const int n_chunks = p.CP / 32;
    const int rg = blockIdx.x / n_chunks, ch = blockIdx.x - rg * n_chunks, c0 = ch * 32, c = c0 + li;
    const int hw = p.h * p.w;
    const TokenStrides code_s = {p.code.stride_n, p.code.stride_h, p.code.stride_w};
    const TokenStrides feats_s = {p.feats.stride_n, p.feats.stride_h, p.feats.stride_w};
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.weight), 0, p.C * p.K * 4, 0x00020000);
    float wreg[16 * NT];
    load_w_rows<NT>(w_rsrc, c * p.K + hf, wreg);
    const bool in_c = c < p.C;
    const float bias_c = in_c ? p.bias[c] : 0.f;
    f32x16 dw[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dw[nt][r] = 0.f;
    float gsum = 0.f;

    float* xs = lds + wave * TILE * KS;                 // this wave's codes [TILE][KS], zero beyond K and T
    const float* xa = xs + li * KS + hf;                // A[i = token li][k = 2 kk + hf]
    // the same trip count in every wave (the barriers order a wave's LDS stores and the other lanes' loads); a wave past its last
    // tile works on zeros
#pragma unroll 1
    for (int first = rg; first < p.n_tiles; first += p.n_rg * WAVES) {
        const int tile = first + p.n_rg * wave;
        const int t0 = tile < p.n_tiles ? tile * TILE : p.T;
        // lane li: the offsets and the scalars of token t0 + li; the other lanes fetch theirs from it
        const bool live = t0 + li < p.T;
        const int tg = min(t0 + li, p.T - 1);
        const long long co = token_offset(code_s, tg, hw, p.w), fo = token_offset(feats_s, tg, hw, p.w);
        const float al = live ? p.gscal[2 * (int64_t)tg] : 0.f, be = live ? p.gscal[2 * (int64_t)tg + 1] : 0.f;
        __syncthreads();                                // the previous tile's codes have been read
#pragma unroll 1
        for (int row0 = 0; row0 < TILE; row0 += 8) {    // eight rows' loads in flight before the first store
            const float* src[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) src[j] = p.code.data + __shfl(co, row0 + j);
            for (int k = lane; k < KP; k += 64) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (t0 + row0 + j < p.T && k < p.K) ? src[j][(int64_t)k * p.code.stride_c] : 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) xs[(row0 + j) * KS + k] = v[j];
            }
        }
        float f[16], ar[16], br[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int src = acc_row(r, hf);             // (lanes src and src + 32 hold the same token's values)
            const long long fr = __shfl(fo, src);       // a token from T on: the last token's features under alpha = beta = 0
            ar[r] = __shfl(al, src);
            br[r] = __shfl(be, src);
            f[r] = in_c ? p.feats.data[fr + (int64_t)c * p.feats.stride_c] : 0.f;
        }
        __syncthreads();                                // the codes are in LDS
        f32x16 g;
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = bias_c;
#pragma unroll
        for (int kk = 0; kk < 16 * NT; ++kk) g = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * kk], wreg[kk], g, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            g[r] = fmaf(ar[r], f[r], br[r] * g[r]);
            gsum += g[r];
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r)                // A[i = channel li][k = token(r, hf)], B[k = token(r, hf)][j = code channel li]
                dw[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], xs[acc_row(r, hf) * KS + nt * 32 + li], dw[nt], 0, 0, 0);
    }
    __syncthreads();                                    // every wave is past its last read of the codes: the region takes the sums

    // the waves' sums in wave order: waves 1 .. 3 through LDS, wave 0 adds
    gsum += __shfl_xor(gsum, 32);
    if (wave > 0) {
        float* q = wsum + (wave - 1) * (NT * 16 + 1) * 64 + lane;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) q[(nt * 16 + r) * 64] = dw[nt][r];
        q[NT * 16 * 64] = gsum;
    }
    __syncthreads();
    const int64_t slab_len = (int64_t)p.CP * p.K + p.CP;         // a partial: [CP][K], then [CP]
    if (wave == 0) {
#pragma unroll 1
        for (int wv = 0; wv < WAVES - 1; ++wv) {
            const float* q = wsum + wv * (NT * 16 + 1) * 64 + lane;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) dw[nt][r] += q[(nt * 16 + r) * 64];
            gsum += q[NT * 16 * 64];
        }
        float* slab = p.slabs + (int64_t)rg * slab_len;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            if (nt * 32 + li < p.K) {
#pragma unroll
                for (int r = 0; r < 16; ++r) slab[(int64_t)(c0 + acc_row(r, hf)) * p.K + nt * 32 + li] = dw[nt][r];
            }
        if (hf == 0) slab[(int64_t)p.CP * p.K + c] = gsum;
        __threadfence();                                // the partial is visible to the device before the counter says so
    }
    __syncthreads();
    if (t == 0) is_last = atomicAdd(&p.counters[ch], 1u) == (unsigned)(p.n_rg - 1);
    __syncthreads();
    if (!is_last) return;
    __threadfence();                                    // the other ranges' partials, as the device has them
    const int n_elem = 32 * p.K + 32;                   // the chunk's rows of d_weight, then its d_bias
    for (int e = t; e < n_elem; e += FIN_TPB) {
        const bool is_w = e < 32 * p.K;
        const int row = is_w ? e / p.K : e - 32 * p.K;
        if (c0 + row >= p.C) continue;
        const int64_t se = is_w ? (int64_t)c0 * p.K + e : (int64_t)p.CP * p.K + c0 + row;
        float s = 0.f;
        for (int i0 = 0; i0 < p.n_rg; i0 += 8) {        // eight partials in flight, added in ascending order
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                v[j] = i0 + j < p.n_rg ? __builtin_bit_cast(float, __hip_atomic_load(reinterpret_cast<const unsigned*>(
                                                                       p.slabs + (int64_t)(i0 + j) * slab_len + se),
                                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                                       : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (i0 + j < p.n_rg) s += v[j];
        }
        if (is_w) {
            if (p.d_weight) p.d_weight[(int64_t)c0 * p.K + e] = s;
        } else if (p.d_bias) {
            p.d_bias[c0 + row] = s;
        }
    }
}

using stego::aligned;
using stego::hip_rc;

inline bool side_ok(int v) { return v >= 1 && v <= STEGO_REC_MAX_SIDE; }

int check_desc(const StegoRecDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->K < 1 || d->K > STEGO_REC_MAX_K || d->C < 1 || d->C > STEGO_REC_MAX_C) return STEGO_ERR_REC_DIM;
    if (d->B < 1 || d->B > STEGO_REC_MAX_B || !side_ok(d->h) || !side_ok(d->w)) return STEGO_ERR_REC_SIZE;
    if ((int64_t)d->B * d->h * d->w > STEGO_REC_MAX_TOKENS) return STEGO_ERR_REC_SIZE;
    return STEGO_OK;
}

struct Plan {
    int T, NT, CP, n_tiles, n_wg, n_rg, elem_blocks;
    size_t lds[STEGO_REC_LAUNCHES];
    int64_t wgs[STEGO_REC_LAUNCHES];
    size_t off_slabs, off_part, off_scal, off_count, ws_bytes;
};

Plan plan(const StegoRecDesc* d)
{
    Plan pl{};
    pl.T = d->B * d->h * d->w;
    pl.NT = (d->K + 31) / 32;
    pl.CP = (d->C + 31) / 32 * 32;
    pl.n_tiles = (pl.T + TILE - 1) / TILE;
    pl.n_wg = std::min(pl.n_tiles, TILES_MAX_WG);
    pl.n_rg = std::min(pl.n_tiles, STEGO_REC_MAX_WORKGROUPS);
    const size_t slab_len = (size_t)pl.CP * d->K + pl.CP;
    pl.elem_blocks = pl.n_rg * (pl.CP / 32);
    pl.lds[0] = (size_t)3 * TILE * 8 + ((size_t)pl.CP * (TILE + 1) + (size_t)TILE * (32 * pl.NT + 1) + WAVES * TILE * 3 + TILE * 3) * 4;
    pl.wgs[0] = pl.n_wg;
    pl.lds[1] = (size_t)FIN_TPB * 8 + std::max((size_t)(WAVES - 1) * (pl.NT * 16 + 1) * 64, (size_t)WAVES * TILE * (32 * pl.NT + 1)) * 4 + 4;
    pl.wgs[1] = pl.elem_blocks + 1;
    stego::WsLayout ws;
    pl.off_slabs = ws.take((size_t)pl.n_rg * slab_len * 4, 16);
    pl.off_part = ws.take((size_t)pl.n_tiles * 8, 16);
    pl.off_scal = ws.take((size_t)pl.T * 2 * 4, 16);
    pl.off_count = ws.take((size_t)(pl.CP / 32) * 4, 16);
    pl.ws_bytes = ws.total(16);
    return pl;
}

}  // namespace

extern "C" size_t stego_rec_loss_workspace_bytes(const StegoRecDesc* desc)
{
    return check_desc(desc) == STEGO_OK ? plan(desc).ws_bytes : 0;
}

extern "C" int stego_rec_loss_plan(const StegoRecDesc* desc, size_t lds_bytes[STEGO_REC_LAUNCHES], int64_t workgroups[STEGO_REC_LAUNCHES])
{
    const int rc = check_desc(desc);
    Plan pl{};
    if (rc == STEGO_OK) pl = plan(desc);
    return stego::report_plan(rc, STEGO_REC_LAUNCHES, pl.lds, pl.wgs, lds_bytes, workgroups);
}

extern "C" int stego_rec_loss(const StegoRecDesc* desc, const StegoMap* code, const StegoMap* feats, const float* weight, const float* bias,
                              float* loss, const StegoMap* d_code, float* d_weight, float* d_bias, void* workspace,
                              size_t workspace_bytes, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!code || !code->data || !feats || !feats->data || !weight || !bias || !loss || !workspace || (d_code && !d_code->data))
        return STEGO_ERR_NULL;
    const Plan pl = plan(desc);
    if (workspace_bytes < pl.ws_bytes) return STEGO_ERR_WORKSPACE;
    if (!aligned(code->data, 4) || !aligned(feats->data, 4) || !aligned(weight, 4) || !aligned(bias, 4) || !aligned(loss, 4) ||
        (d_code && !aligned(d_code->data, 4)) || !aligned(d_weight, 4) || !aligned(d_bias, 4) || !aligned(workspace, 16))
        return STEGO_ERR_ALIGN;

    using stego::at;
    RecParams p{};
    p.code = *code;
    p.feats = *feats;
    if (d_code) p.dcode = *d_code;
    p.weight = weight;
    p.bias = bias;
    p.slabs = at<float>(workspace, pl.off_slabs);
    p.tile_part = at<double>(workspace, pl.off_part);
    p.loss = loss;
    p.d_weight = d_weight;
    p.d_bias = d_bias;
    p.B = desc->B;
    p.K = desc->K;
    p.C = desc->C;
    p.h = desc->h;
    p.w = desc->w;
    p.T = pl.T;
    p.CP = pl.CP;
    p.n_tiles = pl.n_tiles;
    p.n_wg = pl.n_wg;
    p.n_rg = pl.n_rg;
    p.gscal = at<float>(workspace, pl.off_scal);
    p.counters = at<unsigned>(workspace, pl.off_count);
    p.wgrad = (d_weight || d_bias) ? 1 : 0;
    p.inv_t = (float)(1.0 / (double)pl.T);

    const hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = stego::with_const<1, 2, 3, 4>(pl.NT, [&](auto N) { return stego::launch_first<rec_tiles<N()>>((unsigned)p.n_wg, TPB, pl.lds[0], s, p); });
    if (e != hipSuccess) return hip_rc(e);
    // the (range, chunk) workgroups of d_weight / d_bias (none without them), and one more block for the loss
    const int elem_blocks = p.wgrad ? pl.elem_blocks : 0;
    return hip_rc(stego::with_const<1, 2, 3, 4>(pl.NT, [&](auto N) {
        return stego::launch_first<rec_finish<N()>>((unsigned)elem_blocks + 1, FIN_TPB, 0, s, p, elem_blocks);
    }));
}
