// One (pair-set, image) tile of the loss backward, as device functions: the bodies that the plain tile kernels (corr_bwd.hip) and the
// tile role of the build kernels (corr_bwd_lists.hip) both run.
//      G[hw][ij]  = dL/dcd = g_cd + g_loss * (-(fd_final - shift)) * 1[cmin <= cd <= cmax]   (clamp/mul backward;
//                   fd_final - shift = saved w + old_mean, the clamp mask rides in the LSB of the saved w)
//      dAn = G . Bn          dBn = G^T . An          (the two bmm adjoints; An/Bn = normalised sampled codes,
//                                                      re-used from the forward's saved context: no re-gather)
//      dA  = (dAn - An <An,dAn>) / ||a||             (F.normalize backward), likewise dB
// Output: per (tile, side) the gradient w.r.t. the RAW sampled codes, DT[tile][side][128][LDK].
//   bwd_tile_body<NT>           GEMMs on v_mfma_f32_16x16x4_f32 (exact fp32), 256 threads, K <= 80
//   bwd_tile_h_body<NT, DENSE>  GEMMs as split-fp16 products on v_mfma_f32_16x16x32_f16, 512 threads, K <= 128
// LDS carve, workgroup sizes and debug bits: corr_bwd_plan.h.
#pragma once
#include "corr_bwd_plan.h"
#include "corr_common.h"

namespace stego {

// normalize-backward of one side's gradient held in MFMA 16x16 C/D layout and store to DT:
// d[mt][nt][reg] <-> point 32*wave + 16*mt + 4*(lane>>4) + reg, channel 16*nt + (lane&15).
template <int NT>
__device__ __forceinline__ void normalize_bwd_store(f32x4 (&d)[2][NT], const float* __restrict__ Cn, int ldk,
                                                    const float* __restrict__ nrm, float* __restrict__ dt_out,
                                                    int K, int KQ, int lane, int wave)
{
    const int cl = lane & 15, rg = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int pt = 32 * wave + 16 * mt + 4 * rg + reg;
            float cn[NT];
            float dot = 0.f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ch = 16 * nt + cl;
                cn[nt] = ch < K ? Cn[pt * ldk + ch] : 0.f;       // columns >= K hold padding / neighbours
                dot += cn[nt] * (ch < K ? d[mt][nt][reg] : 0.f);
            }
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) dot += __shfl_xor(dot, m, 64);
            const float nr = nrm[pt];
            const bool big = nr > 1e-10f;
            const float inv = 1.f / fmaxf(nr, 1e-10f);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ch = 16 * nt + cl;
                if (ch < KQ) {
                    const float dn = d[mt][nt][reg];
                    float v = big ? (dn - cn[nt] * dot) * inv : dn * inv;
                    if (ch >= K) v = 0.f;
                    dt_out[pt * ldk + ch] = v;
                }
            }
        }
    }
}

template <int NT>
__device__ __forceinline__ void bwd_tile_body(const BwdParams& prm, const int tile, unsigned char* smem)
{
    const int ldk = prm.LDK;
    const int cside = TP * ldk * 4;
    float* nrm = reinterpret_cast<float*>(smem + SMB_NRM);
    unsigned char* An_b = smem + SMB_AN;
    unsigned char* Bn_b = An_b + cside;
    float* An = reinterpret_cast<float*>(An_b);
    float* G = reinterpret_cast<float*>(Bn_b + cside);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = prm.B, P = prm.P, K = prm.K;
    const int b = tile % B, p = tile / B;
    const bool direct = prm.mode == 1;
    const bool sameAB = !direct && p == 0;
    const int sA = b;
    const int sB = direct ? B + b : (p == 0 ? b : p * B + b);
    const float* Bn = sameAB ? An : reinterpret_cast<const float*>(Bn_b);

    // debug bit 8: phase stamps (100 MHz global clock), 4 per tile, second half of the workspace tail
    unsigned long long* ts = reinterpret_cast<unsigned long long*>(prm.dt + (size_t)prm.n_sets * B * 2 * TP * ldk) + 4096 + (size_t)tile * 4;
    const bool stamp_on = (prm.debug & BWD_DBG_STAMPS) && tid == 0 && tile < 1024;
    if (stamp_on) ts[0] = __builtin_amdgcn_s_memrealtime();
    // ---- async copies of the normalised sampled codes (saved by the forward) + their norms
    {
        const unsigned char* srcA = reinterpret_cast<const unsigned char*>(prm.cs) + (size_t)sA * cside;
        const unsigned char* srcB = reinterpret_cast<const unsigned char*>(prm.cs) + (size_t)sB * cside;
        const int npieces = cside / 1024;
        for (int pc = wave; pc < npieces; pc += 4) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcA + (size_t)pc * 1024 + lane * 16),
                                             (__attribute__((address_space(3))) void*)(An_b + pc * 1024), 16, 0, 0);
            if (!sameAB)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcB + (size_t)pc * 1024 + lane * 16),
                                                 (__attribute__((address_space(3))) void*)(Bn_b + pc * 1024), 16, 0, 0);
        }
        nrm[tid] = prm.nrm[(size_t)(tid < TP ? sA : sB) * TP + (tid & (TP - 1))];
    }

    // ---- G tile: row-wise, branch-free, many loads in flight per lane.
    // Upstreams are folded into (pointer, index multiplier, scale) triples so that absent / broadcast
    // gradients need no branches: g = -(w + old_mean) * gl * 1[cmin<=cd<=cmax] + gc.
    {
        const int P2 = P * P;
        const size_t t0 = direct ? (size_t)b * P2 : (p < 2 ? (size_t)b * P2 : ((size_t)(p - 2) * B + b) * P2);
        const float* wp = prm.saved_w + ((size_t)p * B + b) * P2;
        const float inv_numel = 1.f / ((float)B * (float)P2);
        const float* glp = wp;      // dummy when there is no upstream (scale 0)
        int gl_mul = 0;
        float gl_scale = 0.f;
        if (direct || p >= 2) {
            if (prm.g_neg_loss) {
                const bool dense = direct || prm.g_neg_loss_stride > 0;
                glp = dense ? prm.g_neg_loss + t0 : prm.g_neg_loss;
                gl_mul = dense ? 1 : 0;
                // stride -1: the upstream of torch.cat(neg losses).mean(): one scalar, spread over n_neg B P^2 elements
                gl_scale = (!direct && prm.g_neg_loss_stride < 0) ? inv_numel / (float)prm.n_neg : 1.f;
            }
        } else {
            const float* gs = p == 0 ? prm.g_intra : prm.g_inter;     // .mean() backward (modules.py:393,395)
            if (gs) { glp = gs; gl_scale = inv_numel; }
        }
        const float* gcd = direct ? prm.g_neg_cd : (p == 0 ? prm.g_intra_cd : (p == 1 ? prm.g_inter_cd : prm.g_neg_cd));
        const float* gcp = gcd ? gcd + t0 : wp;
        const float om = prm.saved_mean[p];
        // absent / broadcast upstreams cost no loads (uniform branches around whole batches of loads)
        const bool has_gl = gl_mul != 0, has_gc = gcd != nullptr;
        const float gl_b = has_gl ? 0.f : glp[0] * gl_scale;
        constexpr int RB = 16;
        for (int i0 = 0; i0 < TP / 4; i0 += RB) {
            float wv[RB][2], glv[RB][2], gcv[RB][2];
#pragma unroll
            for (int j = 0; j < RB; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int r = wave + 4 * (i0 + j), c = lane + 64 * h;
                    wv[j][h] = wp[min(r, P - 1) * P + min(c, P - 1)];
                }
            if (has_gl) {
#pragma unroll
                for (int j = 0; j < RB; ++j)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int r = wave + 4 * (i0 + j), c = lane + 64 * h;
                        glv[j][h] = glp[min(r, P - 1) * P + min(c, P - 1)] * gl_scale;
                    }
            }
            if (has_gc) {
#pragma unroll
                for (int j = 0; j < RB; ++j)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int r = wave + 4 * (i0 + j), c = lane + 64 * h;
                        gcv[j][h] = gcp[min(r, P - 1) * P + min(c, P - 1)];
                    }
            }
#pragma unroll
            for (int j = 0; j < RB; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int r = wave + 4 * (i0 + j), c = lane + 64 * h;
                    // the forward left the clamp pass-mask 1[cmin <= cd <= cmax] in the mantissa LSB of w
                    const unsigned wb = __builtin_bit_cast(unsigned, wv[j][h]);
                    const float w = __builtin_bit_cast(float, wb & ~1u);
                    float g = (wb & 1u) ? -(w + om) * (has_gl ? glv[j][h] : gl_b) : 0.f;
                    if (has_gc) g += gcv[j][h];
                    G[r * LDG + c] = (r < P && c < P) ? g : 0.f;
                }
        }
    }
    sync_after_lds_dma();  // An/Bn landed, G complete
    if (stamp_on) ts[1] = __builtin_amdgcn_s_memrealtime();

    // ---- dAn = G . Bn  and  dBn = G^T . An   on v_mfma_f32_16x16x4_f32
    // operand lane map: A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15]
    f32x4 dA[2][NT], dB[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { dA[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f}; dB[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    // dA first, its normalize-backward + stores next (they drain while the second GEMM runs), then dB
    const int cl = lane & 15, kq = lane >> 4;
    const int row0 = 32 * wave + cl;
    const int kend = (prm.debug & BWD_DBG_NO_GEMM) ? 0 : TP;
    float* dtA = prm.dt + ((size_t)tile * 2 + 0) * TP * ldk;
    for (int kk = 0; kk < kend; kk += 4) {
        const int k = kk + kq;
        float ga[2], bn[NT];
        ga[0] = G[row0 * LDG + k];                 // G[i][k]
        ga[1] = G[(row0 + 16) * LDG + k];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bn[nt] = Bn[k * ldk + 16 * nt + cl];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            dA[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[0], bn[nt], dA[0][nt], 0, 0, 0);
            dA[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[1], bn[nt], dA[1][nt], 0, 0, 0);
        }
    }
    if (!sameAB) normalize_bwd_store<NT>(dA, An, ldk, nrm, dtA, K, prm.KQ, lane, wave);
    for (int kk = 0; kk < kend; kk += 4) {
        const int k = kk + kq;
        float gt[2], an[NT];
        gt[0] = G[k * LDG + row0];                 // G^T[i][k] = G[k][i]
        gt[1] = G[k * LDG + row0 + 16];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) an[nt] = An[k * ldk + 16 * nt + cl];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            dB[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gt[0], an[nt], dB[0][nt], 0, 0, 0);
            dB[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(gt[1], an[nt], dB[1][nt], 0, 0, 0);
        }
    }
    if (stamp_on) ts[2] = __builtin_amdgcn_s_memrealtime();
    // ---- normalize backward -> DT[tile][side]
    if (sameAB) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) dA[mt][nt] += dB[mt][nt];   // c1 is c2: both adjoints hit the same samples
        normalize_bwd_store<NT>(dA, An, ldk, nrm, dtA, K, prm.KQ, lane, wave);
    } else {
        normalize_bwd_store<NT>(dB, Bn, ldk, nrm + TP, dtA + (size_t)TP * ldk, K, prm.KQ, lane, wave);
    }
    if (stamp_on) ts[3] = __builtin_amdgcn_s_memrealtime();
}

// ------------------------------------------------------------------------------- tile kernel, split-fp16 GEMMs
// The same backward with the two code GEMMs on the fp16 matrix cores (forward() semantics: precision F16X3, and any mode once
// K > 80; the fp32 MFMA of the kernel above runs at the VALU rate on gfx950: 2 x 4.3 us per tile).  Every fp32 operand is
// split into fp16 hi + lo and a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation, as in
// the forward (the K = 32 form takes the time of the K = 16 form on gfx950: half the issues).  MFMA operands must be k-contiguous
// per lane, 8 halves each:
//   CT [side][hi|lo][channel][point]   the normalised sampled codes of both sides, TRANSPOSED on the way into LDS
//   Gh/Gl [row][col]                   G, row-major, times one power of two per tile
//   dAn^T = Bn^T . G^T    A operand = rows of CT(B), B operand = rows of G (k = column: 16-byte reads)
//   dBn^T = An^T . G      A operand = rows of CT(A) (k = anchor point), B operand = COLUMNS of G, gathered by two transposing
//                         8-byte reads per lane and step (a transposed copy of G does not fit next to CT: 157 KB are in use)
// Scale: G's entries are ~1e-7 (upstream 1 / (B P^2)).  One power of two per tile brings the largest |g| (scalar upstreams: the
// bound 4 |gl|; tensor upstreams, DENSE: the exact maximum, one wave reduction + 8 partials through LDS) into [0.5, 1); fp16
// hi + lo then resolve 2^-25 of that absolutely - fp32 accuracy relative to the largest entries, which is what a 128-term sum needs.
// Channel tiles beyond 5 (K > 80) are processed in two groups that share the G image.

// normalize-backward of the B side's gradient held TRANSPOSED in MFMA 16x16 C/D layout and store to DT:
// d[mc][np][reg] <-> channel 16 mc + 4 (lane >> 4) + reg, point 16 (NP wave + np) + (lane & 15).
constexpr int HW_NP = TP / (16 * HW_WAVES);           // 16-point tiles per wave
template <int NT>
__device__ __forceinline__ void normalize_bwd_store_t(f32x4 (&d)[NT][HW_NP], const float* __restrict__ Cn, int ldk,
                                                      const float* __restrict__ nrm, float* __restrict__ dt_out,
                                                      int K, int KQ, int lane, int wave, bool wt = false)
{
    const int cl = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int np = 0; np < HW_NP; ++np) {
        const int pt = 16 * (HW_NP * wave + np) + cl;
        f32x4 cn[NT];
        float dot = 0.f;
#pragma unroll
        for (int mc = 0; mc < NT; ++mc) {
            const int ch0 = 16 * mc + 4 * kq;
            cn[mc] = *reinterpret_cast<const f32x4*>(Cn + (size_t)pt * ldk + ch0);     // columns >= K hold padding / neighbours
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                if (ch0 + reg >= K) cn[mc][reg] = 0.f;
                dot += cn[mc][reg] * (ch0 + reg < K ? d[mc][np][reg] : 0.f);
            }
        }
        dot += __shfl_xor(dot, 16, 64);
        dot += __shfl_xor(dot, 32, 64);
        const float nr = nrm[pt];
        const bool big = nr > 1e-10f;
        const float inv = 1.f / fmaxf(nr, 1e-10f);
#pragma unroll
        for (int mc = 0; mc < NT; ++mc) {
            const int ch0 = 16 * mc + 4 * kq;
            if (ch0 < KQ) {                           // KQ is a multiple of 8: a 4-channel group is inside or outside
                f32x4 v;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const float dn = d[mc][np][reg];
                    v[reg] = big ? (dn - cn[mc][reg] * dot) * inv : dn * inv;
                    if (ch0 + reg >= K) v[reg] = 0.f;
                }
                float* dst = dt_out + (size_t)pt * ldk + ch0;
                // wt: written through (16-byte sc1 store, the cost of a plain one) instead of staying dirty in the L2 until the launch ends
                if (wt) asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(dst), "v"(v) : "memory");
                else *reinterpret_cast<f32x4*>(dst) = v;
            }
        }
    }
}

// One tile of the split-fp16 backward (the body of corr_bwd_tile_h_kernel and of the tile role of corr_bwd_tile_build_kernel).
template <int NT, bool DENSE>      // DENSE: some upstream gradient is a tensor (not the training case)
__device__ __forceinline__ void bwd_tile_h_body(const BwdParams& prm, const int tile, unsigned char* smem)
{
    // channel tiles are processed in groups whose operand images fit LDS next to G: all of them up to K = 80, two groups beyond
    constexpr int NTG = NT <= BWD_NT_F32_MAX ? NT : (NT + 1) / 2;      // (bwd_plan sizes the LDS by the same rule)
    constexpr int NG = (NT + NTG - 1) / NTG;
    constexpr int CTR = 16 * NTG;                     // channel rows per operand image
    float* nrm = reinterpret_cast<float*>(smem + SMH_NRM);
    float* red = nrm + 2 * TP;                        // [HW_WAVES] partial maxima of |g|
    half_t* CT = reinterpret_cast<half_t*>(smem + SMH_CT);                       // [side][hi|lo][CTR][HB_LDR]
    half_t* Gh = CT + 4 * CTR * HB_LDR;
    half_t* Gl = Gh + TP * HB_LDR;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = prm.B, P = prm.P, K = prm.K, ldk = prm.LDK;
    const int b = tile % B, p = tile / B;
    const bool sameAB = p == 0;
    const int sA = b;
    const int sB = p == 0 ? b : p * B + b;
    const float* csA = prm.cs + (size_t)sA * TP * ldk;
    const float* csB = prm.cs + (size_t)sB * TP * ldk;

    // debug bit 8: phase stamps (100 MHz global clock), 4 per tile, second half of the workspace tail
    unsigned long long* ts = reinterpret_cast<unsigned long long*>(prm.dt + (size_t)prm.n_sets * B * 2 * TP * ldk) + 4096 + (size_t)tile * 4;
    const bool stamp_on = (prm.debug & BWD_DBG_STAMPS) && tid == 0 && tile < 1024;
    if (stamp_on) ts[0] = __builtin_amdgcn_s_memrealtime();

    // ---- upstreams folded into (pointer, index multiplier, scale) triples: absent / broadcast gradients need no branches
    //      g = -(w + old_mean) * gl * 1[cmin <= cd <= cmax] + gc
    const int P2 = P * P;
    const size_t t0 = p < 2 ? (size_t)b * P2 : ((size_t)(p - 2) * B + b) * P2;
    const float* wp = prm.saved_w + ((size_t)p * B + b) * P2;
    const float* glp = wp;                            // dummy when there is no upstream (scale 0)
    bool has_gl = false;
    float gl_b = 0.f;                                 // broadcast / scalar upstream of the loss
    if (p >= 2) {
        if (prm.g_neg_loss) {
            if (DENSE && prm.g_neg_loss_stride > 0) { glp = prm.g_neg_loss + t0; has_gl = true; }
            else if (prm.g_neg_loss_stride < 0) gl_b = prm.g_neg_loss[0] * (1.f / ((float)B * (float)P2 * (float)prm.n_neg));   // mean upstream
            else gl_b = prm.g_neg_loss[0];
        }
    } else {
        const float* gs = p == 0 ? prm.g_intra : prm.g_inter;     // .mean() backward (modules.py:393,395)
        if (gs) gl_b = gs[0] * (1.f / ((float)B * (float)P2));
    }
    const float* gcd = !DENSE ? nullptr : (p == 0 ? prm.g_intra_cd : (p == 1 ? prm.g_inter_cd : prm.g_neg_cd));
    const bool has_gc = gcd != nullptr;
    const float* gcp = has_gc ? gcd + t0 : wp;
    const float om = prm.saved_mean[p];

    // ---- every global load of the first operands goes out first (one round trip: a wave has 512 registers here): the saved
    // w (and dense upstreams) of my 16 rows of G, and my share of the first group's code rows of both sides
    constexpr int RB = TP / HW_WAVES;                 // rows of G per wave
    constexpr int c4n = CTR / 4;                      // 4-channel groups per row of a group (reads past ldk stay inside the slack)
    constexpr int NIT = ((TP / 2) * c4n + HW_THREADS - 1) / HW_THREADS;
    float wv[RB][2], glv[RB][2], gcv[RB][2];
    f32x4 r0[2][NIT], r1[2][NIT];
    auto load_codes = [&](int grp) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const float* src = ((side == 0 || sameAB) ? csA : csB) + grp * CTR;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int i = (prm.debug & BWD_DBG_ONE_LOAD) ? 0 : min(tid + it * HW_THREADS, (TP / 2) * c4n - 1);    // (ablation 16: one element)
                const int pp = i / c4n, c4 = i - pp * c4n;
                r0[side][it] = *reinterpret_cast<const f32x4*>(src + (size_t)(2 * pp) * ldk + 4 * c4);
                r1[side][it] = *reinterpret_cast<const f32x4*>(src + (size_t)(2 * pp + 1) * ldk + 4 * c4);
            }
        }
    };
    // [point][channel] fp32 rows -> [channel][point] fp16 hi / lo images (two points per store)
    auto convert_codes = [&](int grp) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            if (side == 1 && sameAB) break;
            half_t* dh = CT + (size_t)(2 * side) * CTR * HB_LDR;
            half_t* dl = dh + CTR * HB_LDR;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int i = tid + it * HW_THREADS;
                if (i < (TP / 2) * c4n) {
                    const int pp = i / c4n, c4 = i - pp * c4n;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int ch = 4 * c4 + e;
                        const bool in = grp * CTR + ch < K;
                        unsigned h, l;
                        split_f16_pair(in ? r0[side][it][e] : 0.f, in ? r1[side][it][e] : 0.f, h, l);
                        // (4-point groups of a channel row XOR-swizzled by ch >> 4: the 20 channel groups of a wave's store
                        // otherwise fall into 4 banks - rows are 68 dwords apart - a 5-way conflict on each of the 48 stores per lane;
                        // ch >> 4 is the MFMA's channel tile mc, so the fragment reads below stay conflict-free)
                        const int col = (((pp >> 1) ^ (ch >> 4)) << 2) + 2 * (pp & 1);
                        *reinterpret_cast<unsigned*>(dh + ch * HB_LDR + col) = h;
                        *reinterpret_cast<unsigned*>(dl + ch * HB_LDR + col) = l;
                    }
                }
            }
        }
    };
    {
        const int c0 = min(2 * lane, P - 1), c1 = min(2 * lane + 1, P - 1);
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const int r = (prm.debug & BWD_DBG_ONE_ROW) ? 0 : min(wave + HW_WAVES * j, P - 1);       // (ablation 4: one row)
            wv[j][0] = wp[r * P + c0];
            wv[j][1] = wp[r * P + c1];
        }
        if (has_gl) {
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int r = min(wave + HW_WAVES * j, P - 1);
                glv[j][0] = glp[r * P + c0];
                glv[j][1] = glp[r * P + c1];
            }
        }
        if (has_gc) {
#pragma unroll
            for (int j = 0; j < RB; ++j) {
                const int r = min(wave + HW_WAVES * j, P - 1);
                gcv[j][0] = gcp[r * P + c0];
                gcv[j][1] = gcp[r * P + c1];
            }
        }
        load_codes(0);
    }
    if (tid < 2 * TP) nrm[tid] = prm.nrm[(size_t)(tid < TP ? sA : sB) * TP + (tid & (TP - 1))];
    // ---- G (rows r = wave + HW_WAVES j, columns 2 lane, 2 lane + 1) in registers; its largest entry picks the tile's scale
    float gmax = 0.f;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int r = wave + HW_WAVES * j;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // the forward left the clamp pass-mask 1[cmin <= cd <= cmax] in the mantissa LSB of w
            const unsigned wb = __builtin_bit_cast(unsigned, wv[j][h]);
            const float w = __builtin_bit_cast(float, wb & ~1u);
            float g = (wb & 1u) ? -(w + om) * (has_gl ? glv[j][h] : gl_b) : 0.f;
            if (has_gc) g += gcv[j][h];
            g = (r < P && 2 * lane + h < P) ? g : 0.f;
            wv[j][h] = g;
            gmax = fmaxf(gmax, fabsf(g));
        }
    }
    float tmax;
    if constexpr (DENSE) {
        // the exact largest |g| of the tile: one wave reduction + 8 partials through LDS
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) gmax = fmaxf(gmax, __shfl_xor(gmax, m, 64));
        if (lane == 0) red[wave] = gmax;
        __syncthreads();
        tmax = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < HW_WAVES; ++w2) tmax = fmaxf(tmax, red[w2]);
    } else {
        // scalar upstream: |g| = |gl| |w + old_mean| < 4 |gl| (w = a cosine - a row mean - a shift): a bound is as good as the
        // maximum here (it only has to keep |g| s below fp16's range and within a few bits of 1), and costs no barrier
        tmax = 4.f * fabsf(gl_b);
    }
    // one power of two per tile brings the largest |g| into [0.5, 1): fp16 hi + lo then resolve 2^-25 of it absolutely
    float sc_tile = 1.f, inv_tile = 1.f;
    if (tmax > 0.f && tmax < 3.0e38f) {
        const int e = __builtin_amdgcn_frexp_expf(tmax);
        sc_tile = __builtin_ldexpf(1.f, -e);
        inv_tile = __builtin_ldexpf(1.f, e);
    }
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        const int r = wave + HW_WAVES * j;
        unsigned hi, lo;
        split_f16_pair(wv[j][0] * sc_tile, wv[j][1] * sc_tile, hi, lo);
        *reinterpret_cast<unsigned*>(Gh + r * HB_LDR + 2 * lane) = hi;
        *reinterpret_cast<unsigned*>(Gl + r * HB_LDR + 2 * lane) = lo;
    }

    // lane map of v_mfma_f32_16x16x32_f16: A[i = lane & 15][k = 8 (lane >> 4) + 0..7], B[k = 8 (lane >> 4) + 0..7][j = lane & 15];
    // C/D as the K = 16 form's (column lane & 15, row 4 (lane >> 4) + reg): half the issues of that form for the same sum
    const int cl = lane & 15, kq = lane >> 4;
    // a lane's 8 points kk + 8 kq .. + 7 of channel row `row` (channel tile mc) of a code image: the 4-point groups 2 j and 2 j + 1,
    // j = kk / 8 + kq.  convert_codes put group g at g ^ mc, so the two sit at (2 j) ^ mc and ((2 j) ^ mc) ^ 1: ONE aligned 16-byte
    // block, (j ^ (mc >> 1)), with its 8-byte halves exchanged when mc is odd.  That exchange is a permutation of k inside the lane:
    // the product only needs both operands to run through k alike, so an odd tile is multiplied with a G fragment whose halves are
    // exchanged too (gemm_dB: the two transposed reads joined the other way round; gemm_dA: the 16 bytes of the row, halves exchanged) -
    // one extra copy of the G fragments per k step where exchanging the code fragments would take one per odd tile.
    // (Rows 272 B apart: the 16 lanes of a read hit 16 distinct 4-dword bank groups.)
    auto ct_frag = [&](const half_t* row, int kk, int mc) {
        return *reinterpret_cast<const f16x8*>(row + ((((kk >> 3) + kq) ^ (mc >> 1)) << 3));
    };
    auto join = [](const void* first, const void* second) {
        f16x8 v;
        __builtin_memcpy(&v, first, 8);
        __builtin_memcpy(reinterpret_cast<char*>(&v) + 8, second, 8);
        return v;
    };
    half_t* ATh = CT;                                 // side 0 = anchors
    half_t* ATl = CT + CTR * HB_LDR;
    half_t* BTh = sameAB ? ATh : CT + 2 * CTR * HB_LDR;
    half_t* BTl = sameAB ? ATl : CT + 3 * CTR * HB_LDR;
    float* dtA = prm.dt + ((size_t)tile * 2 + 0) * TP * ldk;
    const bool skip = (prm.debug & BWD_DBG_NO_GEMM) || tmax == 0.f; // (no upstream: G = 0, the gradients are zero)

    const bool early_dB = NG == 1 && !sameAB && !skip && !(prm.debug & BWD_DBG_LATE_DB);      // (debug 2048: both sides at the end, plain)
    f32x4 dAt[NT][HW_NP], dBt[NT][HW_NP];
#pragma unroll
    for (int mc = 0; mc < NT; ++mc)
#pragma unroll
        for (int np = 0; np < HW_NP; ++np) { dAt[mc][np] = f32x4{0.f, 0.f, 0.f, 0.f}; dBt[mc][np] = f32x4{0.f, 0.f, 0.f, 0.f}; }

#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
        if (grp > 0) {
            __syncthreads();                          // everyone is done with the previous group's images
            load_codes(grp);
        }
        convert_codes(grp);
        __syncthreads();                              // CT of this group (and, the first time, G) complete
        if (stamp_on && grp == 0) ts[1] = __builtin_amdgcn_s_memrealtime();
        if (skip) continue;
        auto gemm_dA = [&]() {
            // ---- dAn^T = Bn^T . G^T: channel rows of CT(B) (A operand) against the ROWS 16 (HW_NP wave + np) + j of G (B operand:
            // B[k][j] = G[j][k], k-contiguous in a row-major G)
            {
                const int ra = cl * HB_LDR;
                const int rg = (16 * HW_NP * wave + cl) * HB_LDR + 8 * kq;          // 8 contiguous halves of a row of G: one 16-byte read
#pragma unroll 2
                for (int kk = 0; kk < TP; kk += 32) {
                    f16x8 ah[NTG], al[NTG], bh[HW_NP][2], bl[HW_NP][2];           // b.[np][1]: halves exchanged, for the odd channel tiles
#pragma unroll
                    for (int mc = 0; mc < NTG; ++mc) {
                        ah[mc] = ct_frag(BTh + ra + 16 * mc * HB_LDR, kk, mc);
                        al[mc] = ct_frag(BTl + ra + 16 * mc * HB_LDR, kk, mc);
                    }
#pragma unroll
                    for (int np = 0; np < HW_NP; ++np) {
                        const half_t* gh = Gh + rg + 16 * np * HB_LDR + kk;
                        const half_t* gl = Gl + rg + 16 * np * HB_LDR + kk;
                        bh[np][0] = *reinterpret_cast<const f16x8*>(gh);
                        bl[np][0] = *reinterpret_cast<const f16x8*>(gl);
                        if (NTG > 1) {
                            bh[np][1] = join(gh + 4, gh);
                            bl[np][1] = join(gl + 4, gl);
                        }
                    }
                    // the three terms outermost: consecutive MFMAs never wait for each other's accumulator
#pragma unroll
                    for (int term = 0; term < 3; ++term)
#pragma unroll
                        for (int mc = 0; mc < NTG; ++mc)
#pragma unroll
                            for (int np = 0; np < HW_NP; ++np)
                                if (grp * NTG + mc < NT)
                                    dAt[grp * NTG + mc][np] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                                        term == 2 ? al[mc] : ah[mc], term == 1 ? bl[np][mc & 1] : bh[np][mc & 1], dAt[grp * NTG + mc][np], 0, 0, 0);
                }
            }
        };
        auto gemm_dB = [&]() {
            // ---- dBn^T = An^T . G: channel rows of CT(A) against the COLUMNS 16 (HW_NP wave + np) + j of G (k = anchor point),
            // gathered by the transposing LDS read
            {
                const int ra = cl * HB_LDR;                                   // CT(A): channel cl (+16 mc), k = kk + 8 kq ..
                // G: row kk + 8 kq + e, column 16 (HW_NP wave + np) + cl - eight ROWS of one column per lane: the LDS transposes
                // (ds_read_b64_tr_b16: lane p of a 16-lane group passes the address of row p >> 2, columns 4 (p & 3) .. + 3 of a
                // [4 rows][16 columns] block and receives column p, rows 0..3; two reads per fragment - rows + 0..3 and + 4..7 -
                // instead of eight 2-byte reads)
                const int gt = (8 * kq + (cl >> 2)) * HB_LDR + 16 * HW_NP * wave + 4 * (cl & 3);
                typedef __fp16 fp16x4v __attribute__((__vector_size__(4 * sizeof(__fp16))));
                typedef __attribute__((address_space(3))) fp16x4v* lds_tr_ptr;
#pragma unroll 2
                for (int kk = 0; kk < TP; kk += 32) {
                    f16x8 ah[NTG], al[NTG], bh[HW_NP][2], bl[HW_NP][2];
#pragma unroll
                    for (int mc = 0; mc < NTG; ++mc) {
                        ah[mc] = ct_frag(ATh + ra + 16 * mc * HB_LDR, kk, mc);
                        al[mc] = ct_frag(ATl + ra + 16 * mc * HB_LDR, kk, mc);
                    }
#pragma unroll
                    for (int np = 0; np < HW_NP; ++np) {
                        const fp16x4v th0 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_tr_ptr)(Gh + gt + kk * HB_LDR + 16 * np));
                        const fp16x4v th1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_tr_ptr)(Gh + gt + (kk + 4) * HB_LDR + 16 * np));
                        const fp16x4v tl0 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_tr_ptr)(Gl + gt + kk * HB_LDR + 16 * np));
                        const fp16x4v tl1 = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_tr_ptr)(Gl + gt + (kk + 4) * HB_LDR + 16 * np));
                        bh[np][0] = join(&th0, &th1);
                        bl[np][0] = join(&tl0, &tl1);
                        bh[np][1] = join(&th1, &th0);
                        bl[np][1] = join(&tl1, &tl0);
                    }
#pragma unroll
                    for (int term = 0; term < 3; ++term)
#pragma unroll
                        for (int mc = 0; mc < NTG; ++mc)
#pragma unroll
                            for (int np = 0; np < HW_NP; ++np)
                                if (grp * NTG + mc < NT)
                                    dBt[grp * NTG + mc][np] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                                        term == 2 ? al[mc] : ah[mc], term == 1 ? bl[np][mc & 1] : bh[np][mc & 1], dBt[grp * NTG + mc][np], 0, 0, 0);
                }
            }
        };
        if (early_dB) {
            // The B side first: its rows leave (normalised, written through) while the A side is multiplied, so half of the DT bytes are
            // out of the L2 before the launch ends - what is still dirty then is written back behind the last workgroup, in front of the
            // unsample launch.  The A-side rows stay plain: the unsample units of this anchor's image run on this XCD and hit them in L2.
            gemm_dB();
#pragma unroll
            for (int mc = 0; mc < NT; ++mc)
#pragma unroll
                for (int np = 0; np < HW_NP; ++np) dBt[mc][np] *= inv_tile;
            normalize_bwd_store_t<NT>(dBt, csB, ldk, nrm + TP, dtA + (size_t)TP * ldk, K, prm.KQ, lane, wave, true);
            gemm_dA();
        } else {
            gemm_dA();
            gemm_dB();
        }
    }
    if (stamp_on) ts[2] = __builtin_amdgcn_s_memrealtime();
#pragma unroll
    for (int mc = 0; mc < NT; ++mc)
#pragma unroll
        for (int np = 0; np < HW_NP; ++np) { dAt[mc][np] *= inv_tile; if (!early_dB) dBt[mc][np] *= inv_tile; }
    if (sameAB) {
        // c1 is c2: both adjoints hit the same samples (same register layout: just add)
#pragma unroll
        for (int mc = 0; mc < NT; ++mc)
#pragma unroll
            for (int np = 0; np < HW_NP; ++np) dAt[mc][np] += dBt[mc][np];
        normalize_bwd_store_t<NT>(dAt, csA, ldk, nrm, dtA, K, prm.KQ, lane, wave);
    } else {
        normalize_bwd_store_t<NT>(dAt, csA, ldk, nrm, dtA, K, prm.KQ, lane, wave);
        if (!early_dB) normalize_bwd_store_t<NT>(dBt, csB, ldk, nrm + TP, dtA + (size_t)TP * ldk, K, prm.KQ, lane, wave);
    }
    if (stamp_on) ts[3] = __builtin_amdgcn_s_memrealtime();
}

}  // namespace stego
