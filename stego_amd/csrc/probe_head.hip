// Fused probe head (include/stego_probe.h): flip average, bilinear resize (align_corners=False), linear probe, cluster probe and a
// softmax / log_softmax / argmax per probe, from the low-resolution code straight to the full-resolution outputs in one launch.
//
// Grid: (output column tiles, output row tiles, B).  A workgroup of 256 threads owns a TY x TX tile of output pixels of one image:
//   1. it loads the source footprint of the tile (the code rows / columns its pixels interpolate from) into LDS, flip-averaged in the
//      reference's order ((code + code_flip[.., w-1-x]) / 2), K channels per pixel padded to a multiple of 4 plus 4 (bank spread);
//   2. it projects every footprint pixel onto both probes: W c + b for the linear probe, c . centroid for the cluster probe (one wave
//      per label row, so the weight row is wave-uniform and read with scalar loads; the lanes run over the footprint pixels);
//   3. every thread then takes one output pixel: torch's source index and weights, the four-tap interpolation of the projections (the
//      weights sum to 1, so this is the probe of the interpolated code), and for the cluster probe the norm of the interpolated
//      K-channel code (four taps from LDS, no Gram form that could cancel), then the per-probe softmax and its store.
// The tile is planned on the host so that the largest footprint fits 64 KiB of LDS (4 x 64 pixels, one per thread, at 8x upsampling;
// smaller tiles for strong downsampling); every output offset is 64-bit.  No atomics: repeat launches give the same bits.
// The phases themselves are in probe_phases.h, shared with confusion.hip's and stitch_probe.hip's kernels; finish() and its three stores
// are there too, shared with stitch_probe.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/stego_probe.h"
#include "host_util.h"
#include "probe_phases.h"

namespace {

constexpr int TPB = PROBE_TPB;
constexpr size_t LDS_BUDGET = 64 * 1024;

struct ProbeParams {
    StegoMap code, flip;             // flip.data == nullptr: no flip average
    const float* lin_w;
    const float* lin_b;
    const float* cent;
    void* lin_out;
    void* clu_out;
    int32_t K, h, w, H, W;
    int32_t n_lin, n_clu, lin_kind, clu_kind;
    float alpha, scale_h, scale_w;
    int32_t TY, TX, max_nr, max_nc;  // output tile, footprint capacity (rows, columns)
    int32_t K4, KS;                  // K rounded up to 4; LDS floats per footprint pixel of code
    int32_t NPS;                     // LDS floats per footprint pixel of projections: 2 * NMAX label slots + 4
};

template <int NMAX>
__global__ __launch_bounds__(TPB) void probe_head_kernel(ProbeParams p)
{
    extern __shared__ float4 smem4[];
    float* const cs = reinterpret_cast<float*>(smem4);
    float* const ps = cs + (size_t)p.max_nr * p.max_nc * p.KS;
    float* const mask = ps + (size_t)p.max_nr * p.max_nc * p.NPS;   // [2 * NMAX]: 0 for a label of the probe, -inf for a pad slot

    const int64_t b = blockIdx.z;
    const int Y0 = blockIdx.y * p.TY, X0 = blockIdx.x * p.TX;
    const int Y1 = min(Y0 + p.TY, p.H), X1 = min(X0 + p.TX, p.W);
    const Footprint f = tile_footprint(Y0, Y1, X0, X1, p.scale_h, p.scale_w, p.h, p.w, p.max_nr, p.max_nc);

    // 1. the footprint's code
    load_footprint(cs, p.code, p.flip, p.flip.data != nullptr, b, f, p.K, p.K4, p.KS, p.w);
    __syncthreads();

    // 2. its projections onto both probes, and the label mask
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    init_mask<NMAX>(mask, p.n_lin, p.n_clu);
    project<NMAX>(ps, cs, p.lin_w, p.lin_b, p.cent, p.n_lin, p.n_clu, p.K, p.KS, p.NPS, f.npx, wave, lane);
    __syncthreads();

    // 3. output pixels
    const int64_t HW = (int64_t)p.H * p.W;
    const float4* cs4 = reinterpret_cast<const float4*>(cs);
    const float4* ps4 = reinterpret_cast<const float4*>(ps);
    const float4* mask4 = reinterpret_cast<const float4*>(mask);
    const int KS4 = p.KS >> 2, NPS4 = p.NPS >> 2;
    {   // one output pixel per thread (TY * TX <= 256; a loop here would let the compiler hoist the label loops' tests and spill)
        const int i = threadIdx.x;
        const int Y = Y0 + i / p.TX, X = X0 + i % p.TX;
        if (i >= p.TY * p.TX || Y >= Y1 || X >= X1) return;
        const Taps t = pixel_taps(Y, X, p.scale_h, p.scale_w, p.h, p.w, f);
        const int64_t pix = (int64_t)Y * p.W + X;

        if (p.lin_kind != STEGO_PROBE_SKIP) {
            float l[NMAX];
            linear_logits<NMAX>(l, ps4, mask4, NPS4, t);
            finish<NMAX>(l, p.n_lin, p.lin_kind, p.lin_out, b, HW, pix);
        }
        if (p.clu_kind != STEGO_PROBE_SKIP) {
            const float den = code_norm(cs4, KS4, p.K4, t);
            float l[NMAX];
            cluster_logits<NMAX>(l, ps4, mask4, NPS4, t, den, p.alpha);
            finish<NMAX>(l, p.n_clu, p.clu_kind, p.clu_out, b, HW, pix);
        }
    }
}

using stego::hip_rc;

inline bool kind_ok(int k) { return k >= STEGO_PROBE_SKIP && k <= STEGO_PROBE_ARGMAX; }

int check_desc(const StegoProbeDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (!kind_ok(d->lin_kind) || !kind_ok(d->clu_kind) || (d->lin_kind == STEGO_PROBE_SKIP && d->clu_kind == STEGO_PROBE_SKIP))
        return STEGO_ERR_PROBE_OUTPUT;
    if (d->K < 1 || d->K > STEGO_PROBE_MAX_K) return STEGO_ERR_PROBE_DIM;
    if (d->lin_kind != STEGO_PROBE_SKIP && (d->n_lin < 1 || d->n_lin > STEGO_PROBE_MAX_N)) return STEGO_ERR_PROBE_DIM;
    if (d->clu_kind != STEGO_PROBE_SKIP && (d->n_clu < 1 || d->n_clu > STEGO_PROBE_MAX_N)) return STEGO_ERR_PROBE_DIM;
    if (d->B < 1 || d->B > 65535 || d->h < 1 || d->h > STEGO_PROBE_MAX_CODE || d->w < 1 || d->w > STEGO_PROBE_MAX_CODE || d->H < 1 ||
        d->H > STEGO_PROBE_MAX_OUT || d->W < 1 || d->W > STEGO_PROBE_MAX_OUT)
        return STEGO_ERR_PROBE_SIZE;
    return STEGO_OK;
}

TilePlan plan(const StegoProbeDesc* d)
{
    const int n = std::max(d->lin_kind != STEGO_PROBE_SKIP ? d->n_lin : 0, d->clu_kind != STEGO_PROBE_SKIP ? d->n_clu : 0);
    return plan_tile(d->K, d->h, d->w, d->H, d->W, n, 2 * label_slots(n) * sizeof(float), LDS_BUDGET);     // + the label mask
}

}  // namespace

extern "C" size_t stego_probe_head_plan(const StegoProbeDesc* desc, int32_t* tile_rows, int32_t* tile_cols)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    const TilePlan pl = plan(desc);
    if (tile_rows) *tile_rows = pl.TY;
    if (tile_cols) *tile_cols = pl.TX;
    return pl.lds;
}

extern "C" int stego_probe_head(const StegoProbeDesc* desc, const StegoMap* code, const StegoMap* code_flip, const float* lin_w,
                                const float* lin_b, const float* centroids, void* lin_out, void* clu_out, stego_stream_t stream)
{
    int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    const bool lin = desc->lin_kind != STEGO_PROBE_SKIP, clu = desc->clu_kind != STEGO_PROBE_SKIP;
    rc = check_probe_ptrs(code, code_flip, lin, lin_w, lin_b, lin_out, desc->lin_kind == STEGO_PROBE_ARGMAX ? 8 : 4, clu, centroids, clu_out,
                          desc->clu_kind == STEGO_PROBE_ARGMAX ? 8 : 4);
    if (rc != STEGO_OK) return rc;

    const TilePlan pl = plan(desc);
    ProbeParams p{};
    p.code = *code;
    p.flip = code_flip ? *code_flip : StegoMap{nullptr, 0, 0, 0, 0};
    p.lin_w = lin_w;
    p.lin_b = lin_b;
    p.cent = centroids;
    p.lin_out = lin_out;
    p.clu_out = clu_out;
    p.K = desc->K;
    p.h = desc->h;
    p.w = desc->w;
    p.H = desc->H;
    p.W = desc->W;
    p.n_lin = lin ? desc->n_lin : 0;      // a skipped probe has no live label slot: its n, weights and output are never read
    p.n_clu = clu ? desc->n_clu : 0;
    p.lin_kind = desc->lin_kind;
    p.clu_kind = desc->clu_kind;
    p.alpha = desc->alpha;
    p.scale_h = pl.scale_h;
    p.scale_w = pl.scale_w;
    p.TY = pl.TY;
    p.TX = pl.TX;
    p.max_nr = pl.max_nr;
    p.max_nc = pl.max_nc;
    p.K4 = pl.K4;
    p.KS = pl.KS;
    p.NPS = pl.NPS;
    const dim3 grid((unsigned)((desc->W + pl.TX - 1) / pl.TX), (unsigned)((desc->H + pl.TY - 1) / pl.TY), (unsigned)desc->B);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    return hip_rc(stego::with_const<8, 16, 32, 64>(pl.NMAX, [&](auto N) { return stego::launch_first<probe_head_kernel<N()>>(grid, TPB, pl.lds, s, p); }));
}
