// Stage 1 of the forward: bilinear sampling + L2 normalisation of (i) the ANCHOR features, written as ready-made LDS
// operand images the tile kernel copies with global_load_lds, and (ii) the CODES of every (role, image) "set", the
// tap tables and the code norms = the saved context the backward re-uses.
//
//   reference: sample() modules.py:287-288 (grid_sample bilinear/border/align_corners) and
//              norm() :275-276, applied at :369-373 (anchor @coords1, positive @coords2) and
//              :384-385 (negatives: orig_feats[perm] / orig_code[perm] @coords2).
//
// Sets: s = role*B + b.  role 0 = anchor (feats/code[b] @ coords1[b]); role 1 = positive
// (feats_pos/code_pos[b] @ coords2[b]); role 2+i = negative i (feats/code[perm_i[b]] @ coords2[b]).
// helper mode: role 0 = (f1,c1), role 1 = (f2,c2), both taken pixel-for-pixel (already sampled).
//
// Only the anchor features are sampled here: they are the one feature set used by more than one tile (all 2+n_neg
// tiles of their image).  Every other set feeds exactly one tile, which gathers it straight from the source image
// (corr_fwd.hip); materialising them (second design) made this kernel HBM-bound at 43 us.
// Work assignment: block -> (16-point unit, set), unit-major, so that blockIdx % 8 = b % 8 (B % 8 == 0): the 8 units
// of an anchor set share an XCD L2 (observed dispatch order; it only affects speed).
//
// One half-wave (32 lanes) owns one sample point: lane hl holds channels 128*j + 4*hl .. +3, so a
// wave instruction is two coalesced 512 B runs; the row norm is a 5-step shuffle reduction.
#include "corr_common.h"
#include "host_util.h"
#include "launchers.h"

namespace stego {

struct PointTaps {
    int4 yx;
    float4 w;
    bool valid;
};

template <int PREC>
__device__ __forceinline__ void store_feat4(const SampleParams& prm, int s, int q, int c, f32x4 v)
{
    const int chunk = c >> 6, col = c & 63;
    if constexpr (PREC == PREC_F32) {
        float* d = static_cast<float*>(prm.fs) + (((size_t)s * prm.NCH + chunk) * TP + q) * LDA + col;
        *reinterpret_cast<f32x4*>(d) = v;
    } else {
        half_t* dh = static_cast<half_t*>(prm.fs) + ((((size_t)s * prm.NCH + chunk) * 2) * TP + q) * LDH + col;
        half_t* dl = dh + TP * LDH;
        unsigned h0, l0, h1, l1;
        split_f16_pair(v[0], v[1], h0, l0);
        split_f16_pair(v[2], v[3], h1, l1);
        *reinterpret_cast<u32x2*>(dh) = u32x2{h0, h1};
        *reinterpret_cast<u32x2*>(dl) = u32x2{l0, l1};
    }
}

template <int PREC>
__device__ __forceinline__ void store_feat1(const SampleParams& prm, int s, int q, int c, float v)
{
    const int chunk = c >> 6, col = c & 63;
    if constexpr (PREC == PREC_F32) {
        static_cast<float*>(prm.fs)[(((size_t)s * prm.NCH + chunk) * TP + q) * LDA + col] = v;
    } else {
        half_t* dh = static_cast<half_t*>(prm.fs) + ((((size_t)s * prm.NCH + chunk) * 2) * TP + q) * LDH + col;
        unsigned h0, l0;
        split_f16_pair(v, 0.f, h0, l0);
        *reinterpret_cast<unsigned short*>(dh) = (unsigned short)(h0 & 0xffffu);
        *reinterpret_cast<unsigned short*>(dh + TP * LDH) = (unsigned short)(l0 & 0xffffu);
    }
}

__device__ __forceinline__ float half_wave_sum(float v)
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);   // xor masks < 32 stay inside the half-wave
    return v;
}

// NJ > 0: channels-last, 16-byte aligned, C == 128*NJ: everything stays in registers.
// NJ == 0: any strides / any C: two gather passes (norm, then normalised write).
template <int NJ, int PREC, bool CCL>
__global__ void __launch_bounds__(NTHREADS) sample_norm_kernel(const SampleParams prm)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hl = lane & 31, hw = lane >> 5;
    const int B = prm.B, P = prm.P;
    const int nsets = prm.n_roles * B;
    const bool direct = prm.mode == 1;
    // Work assignment: block -> (unit qt of 16 points, set s), qt-major.  Consecutive blocks are consecutive sets,
    // so (observed dispatch order) block % 8 = s % 8 = b % 8 when B % 8 == 0: the 8 units of an anchor set - the
    // only role whose FEATURES are sampled here - run on one XCD and its image is fetched from HBM once.
    {
        {
            {
                {
                    const int qt = blockIdx.x / nsets;
                    const int s0 = blockIdx.x - qt * nsets;
                    const int role = s0 / B;
                    const int b = s0 - role * B;
                    // ---------------- one unit: set s = role*B + b, points [16*qt, 16*qt+16)
                    const int s = role * B + b;
                    const int src = (!direct && role >= 2) ? (int)prm.perms[(size_t)(role - 2) * B + b] : b;
                    const bool pos = role == 1;
                    const MapV mf = pos ? prm.feats_pos : prm.feats;
                    const MapV mc = pos ? prm.code_pos : prm.code;
                    const float* fimg = mf.p + (long long)src * mf.sn;
                    const float* cimg = mc.p + (long long)src * mc.sn;
                    const float* coords = direct ? nullptr : ((role == 0 ? prm.coords1 : prm.coords2) + (size_t)b * P * 2);
                // the 4 points this half-wave owns in the unit: fetch their coords up front
                int4 yxs[2];
                float4 ws[2];
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const int q = 16 * qt + 8 * it + 2 * wave + hw;
                    yxs[it] = make_int4(0, 0, 0, 0);
                    ws[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (q < P) {
                        const int hh = (q * prm.div_magic) >> 16, ww = q - hh * prm.div_by;   // q / S (or q / W), q < 128
                        if (direct) {
                            const int v = (hh << 16) | ww;
                            yxs[it] = make_int4(v, v, v, v);
                            ws[it] = make_float4(1.f, 0.f, 0.f, 0.f);
                        } else {
                            const f32x2 cxy = *reinterpret_cast<const f32x2*>(coords + (ww * prm.S + hh) * 2);
                            make_taps(cxy[0], cxy[1], prm.H, prm.W, yxs[it], ws[it]);
                        }
                    }
                }
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const int q = 16 * qt + 8 * it + 2 * wave + hw;
                    const int4 yx = yxs[it];
                    const float4 w = ws[it];
                    const bool valid = q < P;
                    if (hl == 0 && prm.tapyx) {
                        prm.tapyx[(size_t)s * TP + q] = yx;
                        prm.tapw[(size_t)s * TP + q] = w;
                    }
                    // ---- features (anchor role only: every other set is gathered by the one tile that uses it)
                    const int4 of = taps_to_offsets(yx, mf.sh, mf.sw);
                    if (role >= prm.feat_roles) {
                    } else if constexpr (NJ > 0) {
                        f32x4 v[NJ];
                        f32x4 t[NJ][4];
                        const char* fb = reinterpret_cast<const char*>(fimg);     // uniform base + 32-bit lane offset
                        const f32x4* p0 = reinterpret_cast<const f32x4*>(fb + (unsigned)((of.x + 4 * hl) * 4));
                        const f32x4* p1 = reinterpret_cast<const f32x4*>(fb + (unsigned)((of.y + 4 * hl) * 4));
                        const f32x4* p2 = reinterpret_cast<const f32x4*>(fb + (unsigned)((of.z + 4 * hl) * 4));
                        const f32x4* p3 = reinterpret_cast<const f32x4*>(fb + (unsigned)((of.w + 4 * hl) * 4));
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {       // +512 B per j: immediate offsets
                            if (prm.debug & 2) { t[j][0] = t[j][1] = t[j][2] = t[j][3] = f32x4{1.f, 2.f, 3.f, (float)hl}; continue; }
                            t[j][0] = p0[32 * j]; t[j][1] = p1[32 * j]; t[j][2] = p2[32 * j]; t[j][3] = p3[32 * j];
                        }
                        float ss = 0.f;
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float r = w.x * t[j][0][e] + w.y * t[j][1][e] + w.z * t[j][2][e] + w.w * t[j][3][e];
                                v[j][e] = r;
                                ss += r * r;
                            }
                        ss = half_wave_sum(ss);
                        // F.normalize eps (modules.py:276); padding points (zero taps) are written as zeros
                        const float inv = valid ? __builtin_amdgcn_rcpf(fmaxf(sqrtf(ss), 1e-10f)) : 0.f;
                        if (!(prm.debug & 1)) {
#pragma unroll
                            for (int j = 0; j < NJ; ++j) store_feat4<PREC>(prm, s, q, 128 * j + 4 * hl, v[j] * inv);
                        } else if (v[0][0] * inv == 123.456f) prm.nrm[0] = 1.f;
                    } else {
                        const int cpad = prm.NCH * 64;
                        float ss = 0.f;
                        for (int c = hl; c < prm.C; c += 32) {
                            const float* base = fimg + (long long)c * mf.sc;
                            const float r = w.x * base[of.x] + w.y * base[of.y] + w.z * base[of.z] + w.w * base[of.w];
                            ss += valid ? r * r : 0.f;
                        }
                        ss = half_wave_sum(ss);
                        const float inv = 1.f / fmaxf(sqrtf(ss), 1e-10f);
                        for (int c = hl; c < cpad; c += 32) {
                            float r = 0.f;
                            if (c < prm.C && valid) {
                                const float* base = fimg + (long long)c * mf.sc;
                                r = (w.x * base[of.x] + w.y * base[of.y] + w.z * base[of.z] + w.w * base[of.w]) * inv;
                            }
                            store_feat1<PREC>(prm, s, q, c, r);
                        }
                    }
                    // ---- code
                    if (!(prm.debug & 4)) {
                        const int4 oc = taps_to_offsets(yx, mc.sh, mc.sw);
                        float* crow = prm.cs + ((size_t)s * TP + q) * prm.LDK;
                        if constexpr (CCL) {
                            // channels-last, K even: lane hl holds channels 2*hl,2*hl+1 (+64 for the second group)
                            const bool g1 = 64 + 2 * hl < prm.KQ;                 // second group needed (K > 64)
                            const int c1 = (64 + 2 * hl < prm.K) ? 64 + 2 * hl : 0;
                            const int c0 = (2 * hl < prm.K) ? 2 * hl : 0;
                            f32x2 a[4], b2[4];
                            a[0] = *reinterpret_cast<const f32x2*>(cimg + oc.x + c0);
                            a[1] = *reinterpret_cast<const f32x2*>(cimg + oc.y + c0);
                            a[2] = *reinterpret_cast<const f32x2*>(cimg + oc.z + c0);
                            a[3] = *reinterpret_cast<const f32x2*>(cimg + oc.w + c0);
                            if (prm.K > 64) {
                                b2[0] = *reinterpret_cast<const f32x2*>(cimg + oc.x + c1);
                                b2[1] = *reinterpret_cast<const f32x2*>(cimg + oc.y + c1);
                                b2[2] = *reinterpret_cast<const f32x2*>(cimg + oc.z + c1);
                                b2[3] = *reinterpret_cast<const f32x2*>(cimg + oc.w + c1);
                            } else {
                                b2[0] = b2[1] = b2[2] = b2[3] = f32x2{0.f, 0.f};
                            }
                            f32x2 r0 = w.x * a[0] + w.y * a[1] + w.z * a[2] + w.w * a[3];
                            f32x2 r1 = w.x * b2[0] + w.y * b2[1] + w.z * b2[2] + w.w * b2[3];
                            if (2 * hl >= prm.K) r0 = f32x2{0.f, 0.f};
                            if (64 + 2 * hl >= prm.K) r1 = f32x2{0.f, 0.f};
                            float ss = r0[0] * r0[0] + r0[1] * r0[1] + r1[0] * r1[0] + r1[1] * r1[1];
                            ss = half_wave_sum(ss);
                            const float nr = valid ? sqrtf(ss) : 0.f;
                            const float inv = valid ? __builtin_amdgcn_rcpf(fmaxf(nr, 1e-10f)) : 0.f;
                            if (2 * hl < prm.KQ) *reinterpret_cast<f32x2*>(crow + 2 * hl) = r0 * inv;
                            if (g1) *reinterpret_cast<f32x2*>(crow + 64 + 2 * hl) = r1 * inv;
                            if (hl == 0) prm.nrm[(size_t)s * TP + q] = nr;
                        } else {
                            // generic strides: lane hl holds channels hl + 32*m
                            constexpr int MK = 3;           // K <= 72 (host-checked)
                            float cv[MK];
                            float ct[MK][4];
#pragma unroll
                            for (int m = 0; m < MK; ++m) {          // branch-free: out-of-range channels re-read channel 0
                                const int c = hl + 32 * m;
                                const float* base = cimg + (long long)(c < prm.K ? c : 0) * mc.sc;
                                if (32 * m < prm.K) {               // (wave-uniform) skip whole groups beyond K
                                    ct[m][0] = base[oc.x]; ct[m][1] = base[oc.y]; ct[m][2] = base[oc.z]; ct[m][3] = base[oc.w];
                                } else {
                                    ct[m][0] = ct[m][1] = ct[m][2] = ct[m][3] = 0.f;
                                }
                            }
                            float ss = 0.f;
#pragma unroll
                            for (int m = 0; m < MK; ++m) {
                                const int c = hl + 32 * m;
                                float r = w.x * ct[m][0] + w.y * ct[m][1] + w.z * ct[m][2] + w.w * ct[m][3];
                                r = (valid && c < prm.K) ? r : 0.f;
                                cv[m] = r;
                                ss += r * r;
                            }
                            ss = half_wave_sum(ss);
                            const float nr = sqrtf(ss);
                            const float inv = 1.f / fmaxf(nr, 1e-10f);
#pragma unroll
                            for (int m = 0; m < MK; ++m) {
                                const int c = hl + 32 * m;
                                if (c < prm.KQ) crow[c] = cv[m] * inv;
                            }
                            if (hl == 0) prm.nrm[(size_t)s * TP + q] = nr;
                        }
                    }
                    }      // it
                }
            }
        }
    }
}

hipError_t launch_corr_sample(const SampleParams& prm_in, int precision, hipStream_t stream)
{
    SampleParams prm = prm_in;
    auto cl = [&](const MapV& m, int v) {
        return m.sc == 1 && (m.sn % v) == 0 && (m.sh % v) == 0 && (m.sw % v) == 0 &&
               (reinterpret_cast<uintptr_t>(m.p) % (4 * v)) == 0;
    };
    int nj = 0;
    if (prm.C % 128 == 0 && prm.C <= 768 && cl(prm.feats, 4) && cl(prm.feats_pos, 4)) nj = prm.C / 128;
    const bool ccl = prm.K % 2 == 0 && cl(prm.code, 2) && cl(prm.code_pos, 2);
    prm.div_by = prm.mode == 1 ? prm.W : prm.S;
    prm.div_magic = 65536 / prm.div_by + 1;             // (q * magic) >> 16 == q / div_by for q < 128
    const dim3 grid(prm.n_roles * prm.B * 8), block(NTHREADS);      // 8 units of 16 points per set
    // three or six stages of 128 channels, anything else the generic kernel (0); PREC_F16X3 or else the fp32 kernel
    return with_const<3, 6, 0>(nj, [&](auto NJ) {
        return with_const<PREC_F16X3, PREC_F32>(precision, [&](auto PR) {
            return ccl ? launch<sample_norm_kernel<NJ(), PR(), true>>(grid, block, 0, stream, prm)
                       : launch<sample_norm_kernel<NJ(), PR(), false>>(grid, block, 0, stream, prm);
        });
    });
}

}  // namespace stego
