// The body of the backbone's GEMM kernels (vit_forward.hip: vit_gemm_kernel<EPI, X3> and vit_keys_kernel<X3>), included INSIDE each of
// them: one 256 x 192 tile of C = A W^T, then the epilogue EPI names.  In scope at the point of inclusion: `p` (GemmParams), `mtiles`,
// `ntiles`, the constants EPI and X3.  (Text, not a function: a __device__ function inlined into vit_gemm_kernel changed the
// instructions of the instantiations that exist - register allocation and schedule of the epilogues - and those are measured and pinned.)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int mt = xcd + 8 * (slot / ntiles), nt = slot % ntiles;
    if (mt >= mtiles) return;
    const unsigned char* Ap = p.A + (size_t)(2 * mt) * p.nkc * VP_BYTES;        // row panels 2mt, 2mt+1
    // the 192 W rows of column tile nt: rows [r0, 128) of panel p0, then the first 192 - (128 - r0) rows of panel p0 + 1.
    // EPI_KEYS computes the K third of a QKV weight only: its columns start at weight row D (a multiple of 64, so r0 stays 0 or 64);
    // p.bias and p.N are those of the third, column tile nt is local to it
    const int wrow0 = (EPI == EPI_KEYS ? p.D : 0) + GT_N * nt;
    const int p0 = wrow0 >> 7, r0 = wrow0 & 127;
    const unsigned char* W0 = p.W + (size_t)p0 * p.nkc * VP_BYTES + r0 * (VP_LD * 2);
    const unsigned char* W1 = p.W + (size_t)(p0 + 1) * p.nkc * VP_BYTES;
    const int w0_pieces = (128 - r0) * (VP_LD * 2) / 1024;                      // 18 or 9
    auto issue = [&](int c) {
        unsigned char* dst = smem;
        const size_t ko = (size_t)c * VP_BYTES;
        for (int pc = wave; pc < 63; pc += 8) {
            const unsigned char* src;
            if (pc < 18) src = Ap + ko + pc * 1024;
            else if (pc < 36) src = Ap + (size_t)p.nkc * VP_BYTES + ko + (pc - 18) * 1024;
            else if (pc - 36 < w0_pieces) src = W0 + ko + (pc - 36) * 1024;
            else src = W1 + ko + (pc - 36 - w0_pieces) * 1024;
            lds_copy_kib(src, dst + pc * 1024, lane);
        }
    };
    f32x16 acc[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int r = lane & 31, half = lane >> 5;
    for (int c = 0; c < p.nkc; ++c) {
        // One stage per workgroup and no prefetch inside it: the copies of a stage are hidden by the OTHER workgroup of
        // this CU, which is in its MFMAs or its epilogue meanwhile (two 63 KiB stages + the epilogue parks fit the LDS
        // only this way; a double-buffered single workgroup per CU left the CU idle during every epilogue).
        if (c > 0) __syncthreads();                        // everyone is done reading chunk c-1
        if (c == 0 || !(p.debug & 2)) issue(c);
        sync_after_lds_dma();                              // chunk c landed
        if (p.debug & 1) continue;
        const half_t* As = reinterpret_cast<const half_t*>(smem);
        const half_t* Bs = As + GT_M * VP_LD;
        const half_t* ap = As + (64 * wr + r) * VP_LD + 8 * half;
        const half_t* bp = Bs + (96 * wc + r) * VP_LD + 8 * half;
        if constexpr (X3) {
            // a chunk holds 32 k values: halves [kk, kk + 16) of a row are hi parts, 32 further their lo parts; lo*hi and hi*lo first,
            // one term at a time over the six accumulators (no MFMA waits for the one issued before it)
#pragma unroll
            for (int kk = 0; kk < 32; kk += 16) {
                const f16x8 a0h = *reinterpret_cast<const f16x8*>(ap + kk), a1h = *reinterpret_cast<const f16x8*>(ap + 32 * VP_LD + kk);
                const f16x8 a0l = *reinterpret_cast<const f16x8*>(ap + 32 + kk), a1l = *reinterpret_cast<const f16x8*>(ap + 32 * VP_LD + 32 + kk);
                const f16x8 b0h = *reinterpret_cast<const f16x8*>(bp + kk), b1h = *reinterpret_cast<const f16x8*>(bp + 32 * VP_LD + kk);
                const f16x8 b2h = *reinterpret_cast<const f16x8*>(bp + 64 * VP_LD + kk);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0l, b0h, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1l, b0h, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0l, b1h, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1l, b1h, acc[1][1], 0, 0, 0);
                acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0l, b2h, acc[0][2], 0, 0, 0);
                acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1l, b2h, acc[1][2], 0, 0, 0);
                const f16x8 b0l = *reinterpret_cast<const f16x8*>(bp + 32 + kk), b1l = *reinterpret_cast<const f16x8*>(bp + 32 * VP_LD + 32 + kk);
                const f16x8 b2l = *reinterpret_cast<const f16x8*>(bp + 64 * VP_LD + 32 + kk);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b0l, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b0l, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b1l, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b1l, acc[1][1], 0, 0, 0);
                acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b2l, acc[0][2], 0, 0, 0);
                acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b2l, acc[1][2], 0, 0, 0);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b0h, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b0h, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b1h, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b1h, acc[1][1], 0, 0, 0);
                acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0h, b2h, acc[0][2], 0, 0, 0);
                acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1h, b2h, acc[1][2], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < VP_KC; kk += 16) {
                const f16x8 a0 = *reinterpret_cast<const f16x8*>(ap + kk), a1 = *reinterpret_cast<const f16x8*>(ap + 32 * VP_LD + kk);
                const f16x8 b0 = *reinterpret_cast<const f16x8*>(bp + kk), b1 = *reinterpret_cast<const f16x8*>(bp + 32 * VP_LD + kk);
                const f16x8 b2 = *reinterpret_cast<const f16x8*>(bp + 64 * VP_LD + kk);
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, acc[1][1], 0, 0, 0);
                acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b2, acc[0][2], 0, 0, 0);
                acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b2, acc[1][2], 0, 0, 0);
            }
        }
    }
    // ---- epilogue.  C/D layout of the accumulators: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
    if ((p.debug & 4) && acc[0][0][0] != 12345.678f) return;
    // F16X3: the accumulators hold (16 x activation) . (2^s x weight): one exact power of two puts them back
    const float osc = X3 ? __builtin_ldexpf(1.f / VIT_ASCALE, amax_exp(*p.wamax) - 11) : 1.f;
    if constexpr (EPI == EPI_GELU || EPI == EPI_QKV) {
        // fp16 outputs go through LDS (the stage buffer is free now) and leave in the layout of their consumer with
        // wide, coalesced stores, 128 rows per pass.  Storing straight from the accumulators (a lane owns one column:
        // 2-byte stores, 64 B runs, or fully scattered for V^T) cost more than the whole k loop.
        // F16X3 has twice the bytes to park and the same LDS: four passes - GELU by column half (three 32-column chunk panels, hi |
        // lo in one row) in two balanced sets, QKV by plane (the hi values of all three 64-column groups, then the lo values into the lo arrays).
        half_t* T = reinterpret_cast<half_t*>(smem);
        constexpr int GRP = VP_ROWS * VP_LD;            // halves per 64-column group region of one pass (18 KiB)
        constexpr int LDV = VP_ROWS + 8;                // V^T rows: 128 tokens + pad
        // nn.GELU (exact form) with erf from Abramowitz-Stegun 7.1.26 (|err| < 1.5e-7: below the fp16 rounding of the F16 result
        // and - as an ABSOLUTE error of 0.75e-7 |v| on the product - inside the fp32 class of F16X3, tests/test_vit_native.py;
        // ocml erff is ~3x the instructions and was a third of this kernel's time).  (Finishing all 96 values of a wave before the
        // passes - so that no wave waits at a barrier while two compute - made the compiler spill 400 registers inside the k loop.)
        auto gelu = [](float v) {
            const float x = fabsf(v) * 0.70710678118654752f;
            const float t = __builtin_amdgcn_rcpf(1.f + 0.3275911f * x);
            const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
            const float erfa = 1.f - poly * __builtin_amdgcn_exp2f(-x * x * LOG2E);
            return 0.5f * v * (1.f + copysignf(erfa, v));
        };
        for (int pass = 0; pass < (X3 ? 4 : 2); ++pass) {
            const int rh = X3 ? pass >> 1 : pass;       // row half of the tile
            const int sub = pass & 1;                   // F16X3: column half (GELU) / plane (QKV)
            __syncthreads();                            // stage buffer / previous pass's park region is free
            if ((wr >> 1) == rh) {
#pragma unroll
                for (int ni = 0; ni < 3; ++ni) {
                    // F16X3 GELU: the six 32-column chunk panels of a row half leave three per pass, and all four waves of the row
                    // half work in both passes (two blocks and one, then one and two) - by column half only two of eight waves computed
                    // at a time.  Slot of (wc, ni) in its pass: sub 0 = {(0,0) (0,1) (1,0)}, sub 1 = {(0,2) (1,1) (1,2)}
                    const int gslot = sub == 0 ? (wc == 0 ? (ni < 2 ? ni : -1) : (ni == 0 ? 2 : -1)) : (wc == 0 ? (ni == 2 ? 0 : -1) : (ni >= 1 ? ni : -1));
                    if (X3 && EPI == EPI_GELU && gslot < 0) continue;
                    const int col = 96 * wc + 32 * ni + r, cg = col >> 6, cl = col & 63;
                    const int n = nt * GT_N + col;
                    const float bias = (p.bias && n < p.N) ? p.bias[n] : 0.f;
                    const int n0 = nt * GT_N + 64 * cg;     // first column of this lane's 64-column group (wave-uniform)
                    const int which = EPI == EPI_QKV ? n0 / p.D : 0;
                    const float oscale = which == 0 && EPI == EPI_QKV ? p.qscale : 1.f;
                    auto park = [&](auto transposed) {
#pragma unroll
                        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                            for (int e = 0; e < 16; ++e) {
                                const int lrow = 64 * (wr & 1) + 32 * mi + (e & 3) + 8 * (e >> 2) + 4 * half;
                                const float v = acc[mi][ni][e] * osc + bias;
                                if constexpr (EPI == EPI_GELU && X3) {
                                    const float g = x3_sat(gelu(v) * VIT_ASCALE);
                                    const half_t hi = (half_t)g;
                                    T[gslot * GRP + lrow * VP_LD + r] = hi;
                                    T[gslot * GRP + lrow * VP_LD + 32 + r] = (half_t)(g - (float)hi);
                                } else if constexpr (EPI == EPI_GELU) {
                                    T[cg * GRP + lrow * VP_LD + cl] = (half_t)gelu(v);
                                } else {
                                    const float w = v * oscale;
                                    half_t o = (half_t)w;
                                    if (X3 && sub) o = (half_t)(w - (float)o);
                                    if constexpr (decltype(transposed)::value) T[cg * GRP + cl * LDV + lrow] = o;       // V^T
                                    else T[cg * GRP + lrow * VP_LD + cl] = o;                                       // Q (pre-scaled), K
                                }
                            }
                    };
                    if (EPI == EPI_QKV && which == 2) park(std::true_type{});
                    else park(std::false_type{});
                }
            }
            __syncthreads();
            if constexpr (EPI == EPI_GELU) {
                // the three [128][72] images are panels already: linear 16-byte copies
                for (int cg = 0; cg < 3; ++cg) {
                    // (F16X3: slot cg of pass sub holds chunk 3 wc + ni of the tile, see the park above)
                    const int kc = X3 ? nt * 6 + (sub == 0 ? (cg < 2 ? cg : 3) : (cg == 0 ? 2 : 3 + cg)) : nt * 3 + cg;
                    if (kc >= p.out_nkc) continue;
                    unsigned char* dst = p.outp + ((size_t)(2 * mt + rh) * p.out_nkc + kc) * VP_BYTES;
                    const unsigned char* src = smem + cg * VP_BYTES;
                    for (int i = tid; i < VP_BYTES / 16; i += GT_THREADS)
                        *reinterpret_cast<f32x4*>(dst + i * 16) = *reinterpret_cast<const f32x4*>(src + i * 16);
                }
            } else {
                const size_t po = X3 && sub ? p.plane : 0;
                for (int cg = 0; cg < 3; ++cg) {
                    const int n0 = nt * GT_N + 64 * cg;
                    if (n0 >= p.N) continue;
                    const int which = n0 / p.D, head = (n0 - which * p.D) >> 6;
                    if (which < 2) {                     // Q / K: [b][head][token][64], one 128-byte row per token
                        half_t* dstb = (which == 0 ? p.q : p.k) + po;
                        for (int i = tid; i < VP_ROWS * 8; i += GT_THREADS) {
                            const int lrow = i >> 3, ch = i & 7;
                            const int m = mt * GT_M + 128 * rh + lrow;
                            if (m >= p.M) continue;
                            const int b = (int)(((float)m + 0.5f) * p.inv_ntok);
                            const int t = m - b * p.ntok;
                            half_t* dst = dstb + (((size_t)b * p.heads + head) * p.ntok_pad + t) * 64 + ch * 8;
                            *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(T + cg * GRP + lrow * VP_LD + ch * 8);
                        }
                    } else {                             // V^T: [b][head][64][token]; lanes run along the tokens
                        const int lrow = tid & (VP_ROWS - 1);
                        const int m = mt * GT_M + 128 * rh + lrow;
                        if (m < p.M) {
                            const int b = (int)(((float)m + 0.5f) * p.inv_ntok);
                            const int t = m - b * p.ntok;
                            half_t* dst = p.vt + po + (((size_t)b * p.heads + head) * 64) * p.ntok_pad + t;
                            for (int d = tid >> 7; d < 64; d += GT_THREADS / VP_ROWS)
                                dst[(size_t)d * p.ntok_pad] = T[cg * GRP + d * LDV + lrow];
                        }
                    }
                }
            }
        }
    } else {
        const size_t rbytes = (size_t)p.M * p.ldr * 4;
        const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(p.resid, 0, rbytes < 0xFFFFFFFFull ? (unsigned)rbytes : 0xFFFFFFFFu, 0x00020000);
        const unsigned rstride = (unsigned)p.ldr * 4u;
        constexpr int RB = 8;                         // read-modify-writes in flight per accumulator block (16: same time, 6 spilled registers)
#pragma unroll
        for (int ni = 0; ni < 3; ++ni) {
            const int n = nt * GT_N + 96 * wc + 32 * ni + r;
            if (n >= p.N) continue;
            const float bias = p.bias ? p.bias[n] : 0.f;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int mbase = mt * GT_M + 64 * wr + 32 * mi + 4 * half;
                if constexpr (EPI == EPI_RESID) {
                    // all 16 loads of an accumulator block first (interleaved read-modify-writes through one pointer would be serialised
                    // by the compiler: every load ordered behind the previous store, one memory round trip each), then the 16 stores.
                    // Buffer accesses: rows beyond M are out of the descriptor's range (loads return 0, stores are dropped) - no branch
                    // per element - and an address is ONE 32-bit register (round 4: B = 64 forward 14.27 -> 13.83 ms, F16 6.95 -> 6.53 ms
                    // same box against 64-bit pointers + a bounds branch per element)
                    const unsigned off0 = ((unsigned)mbase * (unsigned)p.ldr + (unsigned)n) * 4u;
#pragma unroll
                    for (int e0 = 0; e0 < 16; e0 += RB) {
                        float old[RB];
#pragma unroll
                        for (int e = 0; e < RB; ++e)
                            old[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrsrc, off0 + (unsigned)(((e0 + e) & 3) + 8 * ((e0 + e) >> 2)) * rstride, 0, 0));
#pragma unroll
                        for (int e = 0; e < RB; ++e)
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, old[e] + (acc[mi][ni][e0 + e] * osc + bias)), rrsrc,
                                                                  off0 + (unsigned)(((e0 + e) & 3) + 8 * ((e0 + e) >> 2)) * rstride, 0, 0);
                    }
                } else if constexpr (EPI == EPI_KEYS) {
                    // the keys of the last block leave the fp32 accumulators as they are (never parked as fp16): output row = GEMM row,
                    // the addressing of the residual epilogue without its load; rows beyond M are outside the descriptor and dropped.
                    // Columns n >= N of a partial last tile (products with V rows of the weight, or with its zero padding) were skipped above
                    const unsigned off0 = ((unsigned)mbase * (unsigned)p.ldr + (unsigned)n) * 4u;
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc[mi][ni][e] * osc + bias), rrsrc,
                                                              off0 + (unsigned)((e & 3) + 8 * (e >> 2)) * rstride, 0, 0);
                } else {                              // EPI_EMBED: patch rows -> token rows 1.. of their image, + pos_embed
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int m = mbase + (e & 3) + 8 * (e >> 2);
                        if (m >= p.M) continue;
                        const int b = (int)(((float)m + 0.5f) * p.inv_hw);
                        const int pi = m - b * p.hw;
                        p.resid[((size_t)b * p.ntok + 1 + pi) * p.ldr + n] = acc[mi][ni][e] * osc + bias + p.pos[(size_t)(1 + pi) * p.D + n];
                    }
                }
            }
        }
    }
