// Class-token attention maps and attention salience masks (include/stego_vit.h: stego_vit_forward_attn, stego_attn_salience).
// Reference: src/dino/vision_transformer.py:83-85 (attn = softmax(q k^T * scale)) and :239-246 (get_last_selfattention), row 0 only.
//
// vit_cls_attn_kernel reads what the last block's QKV GEMM left in the workspace of the forward (csrc/vit_forward.hip, EPI_QKV):
// Q and K as [b][head][token, padded to ntok_pad][64] halves, Q times log2(e) / 8, F16X3 as a hi and a lo plane.  Nothing after the
// last attention launch writes them, so the class token's attention row is one read-only pass over K: an M = 1 product, which the
// matrix cores have nothing to offer - plain fp32 FMAs on q = hi + lo and k = hi + lo (exact sums: 22 bits), lo * lo included.
// attn_salience_kernel turns the maps into a foreground mask: the smallest set of strongest patches that holds `keep` of the attention
// mass, by an order that needs no sort.
#include "../../include/stego_vit.h"
#include "corr_common.h"
#include "host_util.h"
#include "vit_cls_attn.h"

namespace stego {
namespace vit {

constexpr int CA_THREADS = 256;
constexpr int CA_LDS_TOK = 8192;          // logits kept in LDS (32 KiB); tokens beyond them are computed again in the later passes
constexpr int CA_UNROLL = 4;              // groups of 8 key rows a wave has in flight

// One workgroup per (image, head).  A key row is 128 bytes: 8 lanes x 16 bytes cover a row, a wave 8 consecutive rows per load
// instruction; the dot finishes with 3 exchanges inside the 8 lanes.  Tokens t < ntok only: the zeroed padding rows
// never enter the max or the sum.  Every reduction has a fixed order: the result depends on (image, head) alone.
template <bool X3>
__global__ void __launch_bounds__(CA_THREADS) vit_cls_attn_kernel(const half_t* __restrict__ q, const half_t* __restrict__ k, const size_t plane,
                                                                  const int ntok, const int ntok_pad, float* __restrict__ out)
{
    __shared__ float logit[CA_LDS_TOK];
    __shared__ float red[2][CA_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, sub = lane & 7, rw = lane >> 3;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t unit = blockIdx.x;
    const half_t* Kg = k + unit * ntok_pad * 64 + sub * 8;
    float* o = out + unit * ntok;
    float qf[8];
    {
        const half_t* qp = q + unit * ntok_pad * 64 + sub * 8;       // row 0: the class token's query
        const f16x8 h = *reinterpret_cast<const f16x8*>(qp);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[e] = (float)h[e];
        if constexpr (X3) {
            const f16x8 l = *reinterpret_cast<const f16x8*>(qp + plane);
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[e] += (float)l[e];
        }
    }
    // f(t, s) for every token t in [first, ntok), s = q . k_t (times log2(e) / 8) in all 8 lanes of the row's group
    // A wave takes CA_UNROLL groups of 8 rows per step and issues all their loads before the first product: the pass runs at the
    // latency of a load (192 workgroups at ViT-B/8, B = 16), and with one load per wave and step forward_tokens_attn cost 13 - 37 us
    // more than forward_tokens, with four 2 - 22 us.
    auto rows = [&](const int first, auto&& f) {
        for (int t0 = first + wave * (8 * CA_UNROLL); t0 < ntok; t0 += CA_THREADS / 8 * CA_UNROLL) {
            f16x8 h[CA_UNROLL], l[CA_UNROLL];
#pragma unroll
            for (int u = 0; u < CA_UNROLL; ++u) {
                const int t = t0 + 8 * u + rw;
#pragma unroll
                for (int e = 0; e < 8; ++e) h[u][e] = l[u][e] = (half_t)0.f;
                if (t < ntok) {
                    const half_t* kp = Kg + (size_t)t * 64;
                    h[u] = *reinterpret_cast<const f16x8*>(kp);
                    if constexpr (X3) l[u] = *reinterpret_cast<const f16x8*>(kp + plane);
                }
            }
#pragma unroll
            for (int u = 0; u < CA_UNROLL; ++u) {
                const int t = t0 + 8 * u + rw;
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) s = fmaf(qf[e], X3 ? (float)h[u][e] + (float)l[u][e] : (float)h[u][e], s);
                s += __shfl_xor(s, 1, 64);
                s += __shfl_xor(s, 2, 64);
                s += __shfl_xor(s, 4, 64);
                if (t < ntok) f(t, s);
            }
        }
    };
    auto block_reduce = [&](float v, const int slot, auto&& op) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
        if (lane == 0) red[slot][wave] = v;
        __syncthreads();
        float r = red[slot][0];
#pragma unroll
        for (int i = 1; i < CA_THREADS / 64; ++i) r = op(r, red[slot][i]);
        return r;
    };

    float m = -INFINITY;
    rows(0, [&](const int t, const float s) {
        if (sub == 0 && t < CA_LDS_TOK) logit[t] = s;
        m = fmaxf(m, s);
    });
    m = block_reduce(m, 0, [](float a, float b) { return fmaxf(a, b); });      // (its barrier publishes the logits)
    const int n_lds = ntok < CA_LDS_TOK ? ntok : CA_LDS_TOK;
    float sum = 0.f;
    for (int t = tid; t < n_lds; t += CA_THREADS) {
        const float e = __builtin_amdgcn_exp2f(logit[t] - m);
        logit[t] = e;                                                           // read back by this thread only
        sum += e;
    }
    if (ntok > CA_LDS_TOK)
        rows(CA_LDS_TOK, [&](const int, const float s) {
            if (sub == 0) sum += __builtin_amdgcn_exp2f(s - m);
        });
    sum = block_reduce(sum, 1, [](float a, float b) { return a + b; });
    for (int t = tid; t < n_lds; t += CA_THREADS) o[t] = logit[t] / sum;
    if (ntok > CA_LDS_TOK)
        rows(CA_LDS_TOK, [&](const int t, const float s) {
            if (sub == 0) o[t] = __builtin_amdgcn_exp2f(s - m) / sum;
        });
}

hipError_t launch_cls_attn(const _Float16* q, const _Float16* k, size_t plane, int ntok, int ntok_pad, int heads, int B, bool x3,
                           float* attn_out, hipStream_t stream)
{
    const dim3 grid((unsigned)(B * heads)), block(CA_THREADS);
    return x3 ? stego::launch<vit_cls_attn_kernel<true>>(grid, block, 0, stream, q, k, plane, ntok, ntok_pad, attn_out)
              : stego::launch<vit_cls_attn_kernel<false>>(grid, block, 0, stream, q, k, plane, ntok, ntok_pad, attn_out);
}

// ------------------------------------------------------------------------------------------------- salience
constexpr int SAL_THREADS = 256;
constexpr int SAL_MAX_PATCHES = 4096;

// patch rows one workgroup decides: about one patch per thread, whole rows (at least one)
inline int sal_rows(int w) { return w >= SAL_THREADS ? 1 : SAL_THREADS / w; }

// A workgroup per (image, slice of whole patch rows).  Every workgroup forms all m_i = sum over the heads of the class token's weight
// on patch i and T = sum m_i in fp64 (the same additions in the same order in every workgroup of an image: the same T), m staged in
// LDS, and decides the patches of its rows.  The order (m descending, index ascending on ties) needs no sort: a thread sums, for a
// patch it owns, the m_j of the patches that come before it - m_j > m_i, or equal and j < i - in fp64 in increasing j.
// kept_i = that sum < keep * T.  The mask of the slice - rows * patch pixel rows, a multiple of 64 bytes from the image's start - leaves
// as whole 16-byte stores over its flat bytes: a row of w * patch bytes is a multiple of 8, so each 8-byte half of a store lies in one
// patch (the two halves of a store are in different pixel rows when w is odd and patch is 8).
__global__ void __launch_bounds__(SAL_THREADS) attn_salience_kernel(const float* __restrict__ attn, const int heads, const int h, const int w,
                                                                    const int patch, const int rows, const double keep,
                                                                    float* __restrict__ soft, uint8_t* __restrict__ mask)
{
    __shared__ double m[SAL_MAX_PATCHES];
    __shared__ double red[SAL_THREADS / 64];
    __shared__ unsigned char kept[SAL_MAX_PATCHES];
    const int tid = threadIdx.x, n = h * w, ntok = n + 1;
    const size_t b = blockIdx.x;
    const int r0 = blockIdx.y * rows, r1 = min(r0 + rows, h);
    const float* a = attn + b * heads * ntok + 1;                   // the class column left out
    double part = 0.0;
    for (int i = tid; i < n; i += SAL_THREADS) {
        double s = 0.0;
        for (int hd = 0; hd < heads; ++hd) s += (double)a[(size_t)hd * ntok + i];
        m[i] = s;
        part += s;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    double T = red[0];
#pragma unroll
    for (int i = 1; i < SAL_THREADS / 64; ++i) T += red[i];
    const double limit = keep * T;
    for (int i = r0 * w + tid; i < r1 * w; i += SAL_THREADS) {
        const double mi = m[i];
        double ahead = 0.0;
        for (int j = 0; j < n; ++j) {
            const double mj = m[j];
            ahead += (mj > mi || (mj == mi && j < i)) ? mj : 0.0;
        }
        kept[i] = ahead < limit ? 1 : 0;
        if (soft) soft[b * n + i] = (float)(mi / T);
    }
    if (!mask) return;
    __syncthreads();
    const int W = w * patch;
    const int c0 = r0 * patch * W / 16, c1 = r1 * patch * W / 16;  // patch * W is a multiple of 64
    uint8_t* mb = mask + b * ((size_t)n * patch * patch);
    for (int c = c0 + tid; c < c1; c += SAL_THREADS) {
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        u32x4 v;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int pix = c * 16 + half * 8;
            const int y = pix / W, x = pix - y * W;
            const unsigned word = kept[(y / patch) * w + x / patch] ? 0x01010101u : 0u;
            v[2 * half] = word;
            v[2 * half + 1] = word;
        }
        *reinterpret_cast<u32x4*>(mb + (size_t)c * 16) = v;
    }
}

}  // namespace vit
}  // namespace stego

using namespace stego;
using namespace stego::vit;

extern "C" int stego_attn_salience(const float* attn, int32_t B, int32_t heads, int32_t h, int32_t w, int32_t patch, float keep, float* soft,
                                   uint8_t* mask, stego_stream_t stream)
{
    if (!attn) return STEGO_ERR_NULL;
    if (B <= 0 || heads <= 0 || h <= 0 || w <= 0) return STEGO_ERR_SHAPE;
    if (!(keep > 0.f && keep <= 1.f)) return STEGO_ERR_SHAPE;
    if (patch != 8 && patch != 16) return STEGO_ERR_UNSUPPORTED;
    if ((long long)h * w > SAL_MAX_PATCHES) return STEGO_ERR_UNSUPPORTED;
    if (!aligned(attn, 4) || !aligned(soft, 4) || !aligned(mask, 16)) return STEGO_ERR_ALIGN;
    if (!soft && !mask) return STEGO_OK;
    const int rows = sal_rows(w);
    return hip_rc(launch_first<attn_salience_kernel>(dim3((unsigned)B, (unsigned)((h + rows - 1) / rows)), dim3(SAL_THREADS), 0,
                                                     static_cast<hipStream_t>(stream), attn, (int)heads, (int)h, (int)w, (int)patch, rows,
                                                     (double)keep, soft, mask));
}
