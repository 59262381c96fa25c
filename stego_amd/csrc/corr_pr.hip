// Label co-occurrence precision / recall histogram of feature correspondences (include/stego_pr.h): bilinear sampling of two feature
// maps and two label maps, L2 normalisation, the channel contraction, the same-class test and the counting in one launch.
//
// Grid: (point tiles of coords2, point tiles of coords1, B).  A workgroup of 256 threads (4 waves) owns a 128 x 128 tile of pairs of
// one image pair:
//   1. thread t < 128 prepares point t of the coords1 tile, thread 128 + t point t of the coords2 tile: the bilinear taps of the
//      feature map (element offset of the north-west tap and the steps to its neighbours, 64-bit; four weights) and, from the up to
//      four label taps with a non-zero weight, the point's purity code: the class (0 = unlabeled, l + 1 otherwise) if they all agree,
//      "impure" (a value that differs between the two sides, so it never compares equal), or "skip" (padding point of the tile; with
//      STEGO_PR_SKIP_UNLABELED also a point with an unlabeled tap);
//   2. per 64-channel chunk: the four waves sample both sides into LDS (64 lanes = 64 channels of one point, so a channels-last map
//      is read in 256-byte rows; fp32 operand images [128][LDA] as corr_tile.h's mma_chunk_f32 expects them, channels beyond C
//      zero), every thread adds the squares of one operand row to its point's squared norm, and each wave runs the 64 x 64 quadrant
//      of the tile on v_mfma_f32_32x32x2_f32 (exact fp32 products: the 2e-5 score bar holds for C = 768 without a split);
//   3. epilogue: the operand stages are dead, so the histogram of the tile (uint32 [n_bins][2]) takes their place in LDS.  Every lane
//      scales its 64 accumulators by the two inverse norms, bins them and adds 1 to (bin, codes equal) with an LDS atomic unless one of
//      the codes says skip; then the non-zero counters are flushed with one 64-bit global atomic add each.
// Integer counters only: the result is independent of arrival order.  81408 bytes of LDS for every n_bins: two workgroups per CU, the
// sampling of one overlaps the MFMAs of the other.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/stego_pr.h"
#include "addon_device.h"
#include "corr_tile.h"
#include "host_util.h"

namespace {

using namespace stego;

constexpr int CODE_SKIP = 0xffff;          // bit 15: the pair is not counted
constexpr int CODE_IMPURE_A = 0x100;       // classes are 0 .. 255
constexpr int CODE_IMPURE_B = 0x200;

// LDS carve (bytes); side 0 = coords1 points, side 1 = coords2 points
constexpr int SP_TAPO = 0;                          // int64 tapo[2][128][3]: offset of the north-west tap, step to east, step to south
constexpr int SP_TAPW = SP_TAPO + 2 * TP * 24;      // float4 tapw[2][128]: nw, ne, sw, se
constexpr int SP_INV = SP_TAPW + 2 * TP * 16;       // float inv[2][128]: 1 / max(||x||, 1e-10)
constexpr int SP_CODE = SP_INV + 2 * TP * 4;        // unsigned short code[2][128]
constexpr int SP_BIG = SP_CODE + 2 * TP * 2;        // two operand stages, then the tile's histogram
constexpr int SP_STAGES = 2 * FEAT_SIDE_F32;
static_assert(SP_BIG % 16 == 0, "operand stages are read with ds_read_b128");
static_assert(STEGO_PR_MAX_BINS * 2 * 4 <= SP_STAGES, "the histogram aliases the operand stages");
constexpr size_t PR_LDS_BYTES = SP_BIG + SP_STAGES;
static_assert(2 * PR_LDS_BYTES <= 160 * 1024, "two workgroups per CU");

struct PrParams {
    StegoMap a, b;
    const int64_t* labels_a;
    const int64_t* labels_b;
    const int64_t* index_b;
    const float* coords1;
    const float* coords2;
    unsigned long long* hist;
    int32_t B, C, h, w, HL, WL, N1, N2, n_bins, n_classes, flags, NCH;
};

// One side's 64-channel chunk of 128 sampled points -> float stage[128][LDA].  Wave `wave` takes points wave, wave + 4, ...
__device__ __forceinline__ void sample_chunk(const float* __restrict__ lane_base, bool chok, const long long* __restrict__ tapo,
                                             const float4* __restrict__ tapw, float* __restrict__ stage, int wave, int lane)
{
#pragma unroll 8
    for (int p = wave; p < TP; p += 4) {
        const long long o = tapo[3 * p], dx = tapo[3 * p + 1], dy = tapo[3 * p + 2];
        const float4 wt = tapw[p];
        const float* q = lane_base + o;
        const float t0 = q[0], t1 = q[dx], t2 = q[dy], t3 = q[dx + dy];
        const float r = wt.x * t0 + wt.y * t1 + wt.z * t2 + wt.w * t3;
        stage[p * LDA + lane] = chok ? r : 0.f;
    }
}

__global__ __launch_bounds__(NTHREADS) void corr_pr_kernel(PrParams p)
{
    extern __shared__ float4 smem4[];
    unsigned char* const smem = reinterpret_cast<unsigned char*>(smem4);
    long long* const tapo = reinterpret_cast<long long*>(smem + SP_TAPO);
    float4* const tapw = reinterpret_cast<float4*>(smem + SP_TAPW);
    float* const inv = reinterpret_cast<float*>(smem + SP_INV);
    unsigned short* const code = reinterpret_cast<unsigned short*>(smem + SP_CODE);
    float* const As = reinterpret_cast<float*>(smem + SP_BIG);
    float* const Bs = As + TP * LDA;
    unsigned* const h32 = reinterpret_cast<unsigned*>(smem + SP_BIG);

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t img_a = blockIdx.z;
    int64_t img_b = p.index_b ? p.index_b[img_a] : img_a;
    img_b = img_b < 0 ? 0 : (img_b > p.B - 1 ? p.B - 1 : img_b);         // memory safety only

    // 1. this thread's point: feature taps and the purity code
    {
        const int side = tid >> 7, i = tid & (TP - 1);
        const int N = side ? p.N2 : p.N1;
        const int pt = (side ? blockIdx.x : blockIdx.y) * TP + i;
        const bool valid = pt < N;
        float x = 0.f, y = 0.f;
        if (valid) {
            const float* c = (side ? p.coords2 : p.coords1) + (img_a * N + pt) * 2;
            x = c[0];
            y = c[1];
        }
        const StegoMap& m = side ? p.b : p.a;
        const Taps f = bilinear_taps(x, y, p.h, p.w);
        tapo[(side * TP + i) * 3 + 0] = valid ? (long long)f.y0 * m.stride_h + (long long)f.x0 * m.stride_w : 0;
        tapo[(side * TP + i) * 3 + 1] = valid ? (long long)(f.x1 - f.x0) * m.stride_w : 0;
        tapo[(side * TP + i) * 3 + 2] = valid ? (long long)(f.y1 - f.y0) * m.stride_h : 0;
        tapw[side * TP + i] = valid ? make_float4(f.wx0 * f.wy0, f.wx1 * f.wy0, f.wx0 * f.wy1, f.wx1 * f.wy1) : make_float4(0.f, 0.f, 0.f, 0.f);

        int cd = CODE_SKIP;
        if (valid) {
            const Taps l = bilinear_taps(x, y, p.HL, p.WL);
            const int64_t* lab = (side ? p.labels_b : p.labels_a) + (side ? img_b : img_a) * p.HL * p.WL;
            const int ys[4] = {l.y0, l.y0, l.y1, l.y1}, xs[4] = {l.x0, l.x1, l.x0, l.x1};
            const bool on[4] = {l.wx0 > 0.f && l.wy0 > 0.f, l.wx1 > 0.f && l.wy0 > 0.f, l.wx0 > 0.f && l.wy1 > 0.f, l.wx1 > 0.f && l.wy1 > 0.f};
            int first = -1;
            bool pure = true, unlabeled = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t v = lab[(int64_t)ys[k] * p.WL + xs[k]];         // (a tap with weight 0 is still a pixel of the map)
                const int cls = (v >= 0 && v < p.n_classes) ? (int)v + 1 : 0;
                if (on[k]) {
                    unlabeled |= cls == 0;
                    pure &= first < 0 || cls == first;
                    first = first < 0 ? cls : first;
                }
            }
            cd = pure ? first : (side ? CODE_IMPURE_B : CODE_IMPURE_A);
            if (first < 0 || ((p.flags & STEGO_PR_SKIP_UNLABELED) && unlabeled)) cd = CODE_SKIP;
        }
        code[side * TP + i] = (unsigned short)cd;
    }

    // 2. the contraction, 64 channels at a time
    f32x16 acc[2][2];
    zero_acc(acc);
    float ss = 0.f;                                                      // squared norm of operand row `tid` (A rows, then B rows)
    const float* const base_a = p.a.data + img_a * p.a.stride_n;
    const float* const base_b = p.b.data + img_b * p.b.stride_n;
    for (int ch = 0; ch < p.NCH; ++ch) {
        __syncthreads();                                                 // taps published / the previous chunk's MFMAs have read the stages
        const int c = ch * KC + lane;
        const bool chok = c < p.C;
        const int64_t cc = chok ? c : p.C - 1;
        sample_chunk(base_a + cc * p.a.stride_c, chok, tapo, tapw, As, wave, lane);
        sample_chunk(base_b + cc * p.b.stride_c, chok, tapo + 3 * TP, tapw + TP, Bs, wave, lane);
        __syncthreads();
        {
            const f32x4* row = reinterpret_cast<const f32x4*>(As + tid * LDA);   // Bs follows As: row tid of both
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < KC / 4; ++k) {
                const f32x4 v = row[k];
                s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
            }
            ss += s;
        }
        mma_chunk_f32(As, Bs, acc, lane, wr, wc);
    }
    __syncthreads();                                                     // the stages are dead: the histogram takes their place

    // 3. count
    inv[tid] = (p.flags & STEGO_PR_RAW) ? 1.f : 1.f / fmaxf(sqrtf(ss), 1e-10f);
    for (int i = tid; i < 2 * p.n_bins; i += NTHREADS) h32[i] = 0u;
    __syncthreads();
    const float nb = (float)p.n_bins, top = (float)(p.n_bins - 1);
    const bool raw = (p.flags & STEGO_PR_RAW) != 0;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int col = 64 * wc + 32 * ni + (lane & 31);
        const int cb = code[TP + col];
        const float ib = inv[TP + col];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 64 * wr + 32 * mi + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int ca = code[row];
                float fd = (acc[mi][ni][r] * inv[row]) * ib;
                if (raw) fd = fminf(fmaxf(fd, -1.f), 1.f);
                const float t = fminf(fmaxf(floorf((fd + 1.f) * 0.5f * nb), 0.f), top);     // (NaN ends in bin 0)
                if (!((ca | cb) & 0x8000)) atomicAdd(&h32[2 * (int)t + (ca == cb ? 1 : 0)], 1u);
            }
    }
    __syncthreads();
    for (int i = tid; i < 2 * p.n_bins; i += NTHREADS) {
        const unsigned n = h32[i];
        if (n) atomicAdd(&p.hist[i], (unsigned long long)n);
    }
}

inline bool side_ok(int v) { return v >= 1 && v <= STEGO_PR_MAX_SIDE; }

int check_desc(const StegoPrDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->flags & ~(STEGO_PR_RAW | STEGO_PR_SKIP_UNLABELED)) return STEGO_ERR_PR_FLAGS;
    if (d->C < 1 || d->C > STEGO_PR_MAX_C) return STEGO_ERR_PR_DIM;
    if (d->N1 < 1 || d->N1 > STEGO_PR_MAX_POINTS || d->N2 < 1 || d->N2 > STEGO_PR_MAX_POINTS) return STEGO_ERR_PR_POINTS;
    if (d->n_bins < STEGO_PR_MIN_BINS || d->n_bins > STEGO_PR_MAX_BINS) return STEGO_ERR_PR_BINS;
    if (d->n_classes < 1 || d->n_classes > STEGO_PR_MAX_CLASSES) return STEGO_ERR_PR_CLASSES;
    if (d->B < 1 || d->B > 65535 || !side_ok(d->h) || !side_ok(d->w) || !side_ok(d->HL) || !side_ok(d->WL)) return STEGO_ERR_PR_SIZE;
    return STEGO_OK;
}

}  // namespace

extern "C" size_t stego_pr_plan(const StegoPrDesc* desc, int32_t* tiles1, int32_t* tiles2)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    if (tiles1) *tiles1 = (desc->N1 + TP - 1) / TP;
    if (tiles2) *tiles2 = (desc->N2 + TP - 1) / TP;
    return PR_LDS_BYTES;
}

extern "C" int stego_pr_accumulate(const StegoPrDesc* desc, const StegoMap* a, const StegoMap* b, const int64_t* labels_a,
                                   const int64_t* labels_b, const int64_t* index_b, const float* coords1, const float* coords2,
                                   uint64_t* hist, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    if (!a || !a->data || !b || !b->data || !labels_a || !labels_b || !coords1 || !coords2 || !hist) return STEGO_ERR_NULL;
    if (!aligned(a->data, 4) || !aligned(b->data, 4) || !aligned(coords1, 4) || !aligned(coords2, 4)) return STEGO_ERR_ALIGN;
    if (!aligned(labels_a, 8) || !aligned(labels_b, 8) || !aligned(index_b, 8) || !aligned(hist, 8)) return STEGO_ERR_ALIGN;

    PrParams p{};
    p.a = *a;
    p.b = *b;
    p.labels_a = labels_a;
    p.labels_b = labels_b;
    p.index_b = index_b;
    p.coords1 = coords1;
    p.coords2 = coords2;
    p.hist = reinterpret_cast<unsigned long long*>(hist);
    p.B = desc->B;
    p.C = desc->C;
    p.h = desc->h;
    p.w = desc->w;
    p.HL = desc->HL;
    p.WL = desc->WL;
    p.N1 = desc->N1;
    p.N2 = desc->N2;
    p.n_bins = desc->n_bins;
    p.n_classes = desc->n_classes;
    p.flags = desc->flags;
    p.NCH = (desc->C + KC - 1) / KC;
    const dim3 grid((unsigned)((desc->N2 + TP - 1) / TP), (unsigned)((desc->N1 + TP - 1) / TP), (unsigned)desc->B);
    (void)hipGetLastError();
    return hip_rc(launch<corr_pr_kernel>(grid, dim3(NTHREADS), (int)PR_LDS_BYTES, static_cast<hipStream_t>(stream), p));
}
