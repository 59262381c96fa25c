// Device-side confusion matrices (include/stego_confusion.h): the fused probe head with the two matrices as its only output, and the
// same counting for label maps and score planes made elsewhere.
//
// probe_confusion_kernel is probe_head.hip's kernel with another sink: both are built from the phases of probe_phases.h (footprint
// load, projections, taps, logits, the first maximum), so the label counted here is the label the head's ARGMAX kind writes, by
// construction; tests/test_confusion_gpu.py also holds the two equal bit for bit.  What is this kernel's own: the tile loop, the label
// read, the ConfMaps copy in LDS and the counting.
//
// Grid: sized from the compute units, not from the pixels.  A workgroup of 256 threads walks the label tiles (column tiles, row tiles,
// images; tile t, t + grid, ...) and keeps one uint32 histogram per active probe in LDS, [n, n_classes] as in global memory.  Per tile
// every thread has one label pixel and so one bin per probe.  Segmentation maps are piecewise constant: most lanes of a wave hold the
// same bin, so the wave adds per distinct bin, not per lane (wave_count: the first pending lane's bin goes to every lane, a ballot
// finds the lanes that hold it, that one lane adds their number with one LDS atomic; 1-4 rounds on real maps).  After its last tile the
// workgroup adds its non-zero bins onto the int64 matrices with 64-bit global atomics.  Integer adds commute: the counts are exact and
// repeat from run to run.  Nothing per pixel is written to global memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/stego_confusion.h"
#include "host_util.h"
#include "probe_phases.h"

namespace {

constexpr int TPB = PROBE_TPB;
constexpr size_t LDS_BUDGET = 64 * 1024;
constexpr int WGS_PER_CU = 4;
// a workgroup's uint32 bins must not wrap before it flushes them: the host sizes the grid so that none counts more pixels than this
constexpr int64_t MAX_WG_PIXELS = 1ll << 31;

// What only per-thread arithmetic reads.  The kernel copies it to LDS once and reads it from there: held in scalar registers for the
// whole tile loop, beside the loop's own state, these 29 dwords do not fit the scalar register file.
struct ConfMaps {
    StegoMap code, flip;             // flip.data == nullptr: no flip average
    const int64_t* labels;
    unsigned long long* lin_counts;
    unsigned long long* clu_counts;
    float alpha, scale_h, scale_w;
};
constexpr int MAPS_FLOATS = 32;      // sizeof(ConfMaps) = 120 bytes, rounded up to whole float4

struct ConfParams {
    ConfMaps maps;
    const float* lin_w;
    const float* lin_b;
    const float* cent;
    int32_t K, h, w, H, W;
    int32_t n_lin, n_clu, n_classes; // n_lin / n_clu == 0: the probe is skipped
    int32_t TY, TX, max_nr, max_nc;  // label tile, footprint capacity (rows, columns)
    int32_t K4, KS;                  // as in probe_head.hip; its NPS is 2 * NMAX + 4 here
    int32_t ntx, tpi, B;             // tiles per row of tiles, per image (< 2^23); images
    int32_t has_flip;
};

// One add per distinct bin of the wave.  Every lane of the wave calls this (converged); key < 0: the lane counts nothing.
__device__ inline void wave_count(unsigned* hist, int key, int lane)
{
    unsigned long long pending = __ballot(key >= 0);
    while (pending) {
        const int lead = __builtin_amdgcn_readfirstlane(__builtin_ctzll(pending));
        const int k = __builtin_amdgcn_readlane(key, lead);
        const unsigned long long same = __ballot(key == k);
        if (lane == lead) atomicAdd(hist + k, (unsigned)__popcll(same));
        pending &= ~same;
    }
}

// The workgroup's non-zero bins onto the global matrix.  Barriers: the caller's.
__device__ inline void flush(unsigned* hist, int bins, unsigned long long* counts)
{
    for (int i = threadIdx.x; i < bins; i += TPB) {
        const unsigned v = hist[i];
        if (v) atomicAdd(counts + i, (unsigned long long)v);
    }
}

template <int NMAX>
__global__ __launch_bounds__(TPB) void probe_confusion_kernel(ConfParams p)
{
    extern __shared__ float4 smem4[];
    ConfMaps* const maps = reinterpret_cast<ConfMaps*>(smem4);
    float* const cs = reinterpret_cast<float*>(smem4) + MAPS_FLOATS;
    float* const ps = cs + (size_t)p.max_nr * p.max_nc * p.KS;
    constexpr int NPS = 2 * NMAX + 4, NPS4 = NPS >> 2;
    float* const mask = ps + (size_t)p.max_nr * p.max_nc * NPS;   // [2 * NMAX]: 0 for a label of the probe, -inf for a pad slot
    unsigned* const lin_hist = reinterpret_cast<unsigned*>(mask + 2 * NMAX);
    const int lin_bins = p.n_lin * p.n_classes, clu_bins = p.n_clu * p.n_classes;
    unsigned* const clu_hist = lin_hist + lin_bins;

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    init_mask<NMAX>(mask, p.n_lin, p.n_clu);
    for (int i = threadIdx.x; i < lin_bins + clu_bins; i += TPB) lin_hist[i] = 0;
    if (threadIdx.x == 0) *maps = p.maps;

    const float4* cs4 = reinterpret_cast<const float4*>(cs);
    const float4* ps4 = reinterpret_cast<const float4*>(ps);
    const float4* mask4 = reinterpret_cast<const float4*>(mask);
    const int KS4 = p.KS >> 2;

    // tile ti of image b; the workgroup's next one is gridDim.x tiles on (32-bit: gridDim.x and tpi are both far below 2^30)
    int b = 0, ti = blockIdx.x;
    for (;; ti += gridDim.x) {
        while (ti >= p.tpi && b < p.B) {
            ti -= p.tpi;
            ++b;
        }
        if (b >= p.B) break;
        const int tx = ti % p.ntx, ty = ti / p.ntx;
        const int Y0 = ty * p.TY, X0 = tx * p.TX;
        const int Y1 = min(Y0 + p.TY, p.H), X1 = min(X0 + p.TX, p.W);
        __syncthreads();                                            // the tile before is done with cs / ps; the first: maps, mask, bins
        const float scale_h = maps->scale_h, scale_w = maps->scale_w;
        const Footprint f = tile_footprint(Y0, Y1, X0, X1, scale_h, scale_w, p.h, p.w, p.max_nr, p.max_nc);

        // phases 1 and 2 of the head (probe_phases.h): the footprint's code, then its projections onto both probes
        const StegoMap code = maps->code, flip = maps->flip;
        load_footprint(cs, code, flip, p.has_flip != 0, b, f, p.K, p.K4, p.KS, p.w);
        __syncthreads();
        project<NMAX>(ps, cs, p.lin_w, p.lin_b, p.cent, p.n_lin, p.n_clu, p.K, p.KS, NPS, f.npx, wave, lane);
        __syncthreads();

        // phase 3: one label pixel per thread (TY * TX <= 256); a thread without one keeps key -1 and stays for the wave's count
        const int i = threadIdx.x;
        const int Y = Y0 + i / p.TX, X = X0 + i % p.TX;
        const bool has = i < p.TY * p.TX && Y < Y1 && X < X1;
        int64_t label = -1;
        if (has) label = maps->labels[((int64_t)b * p.H + Y) * p.W + X];
        const bool counted = label >= 0 && label < p.n_classes;
        int lin_key = -1, clu_key = -1;
        if (counted) {
            const Taps t = pixel_taps(Y, X, scale_h, scale_w, p.h, p.w, f);
            if (p.n_lin) {
                float l[NMAX];
                linear_logits<NMAX>(l, ps4, mask4, NPS4, t);
                lin_key = first_max<NMAX>(l) * p.n_classes + (int)label;
            }
            if (p.n_clu) {
                const float den = code_norm(cs4, KS4, p.K4, t);
                float l[NMAX];
                cluster_logits<NMAX>(l, ps4, mask4, NPS4, t, den, maps->alpha);
                clu_key = first_max<NMAX>(l) * p.n_classes + (int)label;
            }
        }
        if (p.n_lin) wave_count(lin_hist, lin_key, lane);
        if (p.n_clu) wave_count(clu_hist, clu_key, lane);
    }
    __syncthreads();
    if (p.n_lin) flush(lin_hist, lin_bins, maps->lin_counts);
    if (p.n_clu) flush(clu_hist, clu_bins, maps->clu_counts);
}

struct CountParams {
    const void* pred;
    const int64_t* labels;
    unsigned long long* counts;
    int32_t n, n_classes;
    int64_t HW, total;               // H * W, B * H * W
};

// Grid-stride pass over the pixels, one per thread and round: lane i of a wave reads pixel base + i, so each of the n planes (and the
// labels) is read in whole rows of consecutive addresses.  SCORES: the running first maximum stays in registers.
template <bool SCORES>
__global__ __launch_bounds__(TPB) void confusion_count_kernel(CountParams p)
{
    __shared__ unsigned hist[STEGO_CONF_MAX_N * STEGO_CONF_MAX_N];
    const int bins = p.n * p.n_classes;
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < bins; i += TPB) hist[i] = 0;
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * TPB;
    for (int64_t base = (int64_t)blockIdx.x * TPB; base < p.total; base += step) {
        const int64_t px = base + threadIdx.x;
        int key = -1;
        if (px < p.total) {
            const int64_t label = p.labels[px];
            int64_t pred;
            if (SCORES) {
                const int64_t b = px / p.HW, q = px - b * p.HW;
                const float* s = static_cast<const float*>(p.pred) + b * p.n * p.HW + q;
                float bv = s[0];
                int best = 0;
#pragma unroll 8
                for (int j = 1; j < p.n; ++j) {
                    const float v = s[(int64_t)j * p.HW];
                    best = v > bv ? j : best;
                    bv = v > bv ? v : bv;
                }
                pred = best;
            } else {
                pred = static_cast<const int64_t*>(p.pred)[px];
            }
            if (label >= 0 && label < p.n_classes && pred >= 0 && pred < p.n) key = (int)pred * p.n_classes + (int)label;
        }
        wave_count(hist, key, lane);
    }
    __syncthreads();
    flush(hist, bins, p.counts);
}

using stego::aligned;
using stego::hip_rc;

int check_desc(const StegoProbeConfusionDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if ((d->lin_on != 0 && d->lin_on != 1) || (d->clu_on != 0 && d->clu_on != 1) || (!d->lin_on && !d->clu_on)) return STEGO_ERR_CONF_PROBES;
    if (d->K < 1 || d->K > STEGO_PROBE_MAX_K) return STEGO_ERR_CONF_DIM;
    if (d->lin_on && (d->n_lin < 1 || d->n_lin > STEGO_CONF_MAX_N)) return STEGO_ERR_CONF_DIM;
    if (d->clu_on && (d->n_clu < 1 || d->n_clu > STEGO_CONF_MAX_N)) return STEGO_ERR_CONF_DIM;
    if (d->n_classes < 1 || d->n_classes > STEGO_CONF_MAX_N) return STEGO_ERR_CONF_DIM;
    if (d->B < 1 || d->B > 65535 || d->h < 1 || d->h > STEGO_PROBE_MAX_CODE || d->w < 1 || d->w > STEGO_PROBE_MAX_CODE || d->H < 1 ||
        d->H > STEGO_PROBE_MAX_OUT || d->W < 1 || d->W > STEGO_PROBE_MAX_OUT)
        return STEGO_ERR_CONF_SIZE;
    return STEGO_OK;
}

static_assert(sizeof(ConfMaps) <= MAPS_FLOATS * sizeof(float), "ConfMaps outgrew its LDS slot");

// The tile shrinks until footprint and histograms fit the budget together.
TilePlan plan(const StegoProbeConfusionDesc* d)
{
    const int n_lin = d->lin_on ? d->n_lin : 0, n_clu = d->clu_on ? d->n_clu : 0;
    const int n = std::max(n_lin, n_clu);
    const size_t hist = (size_t)(n_lin + n_clu) * d->n_classes * sizeof(unsigned);
    return plan_tile(d->K, d->h, d->w, d->H, d->W, n, (2 * label_slots(n) + MAPS_FLOATS) * sizeof(float) + hist, LDS_BUDGET);
}

}  // namespace

extern "C" size_t stego_probe_confusion_plan(const StegoProbeConfusionDesc* desc, int32_t* tile_rows, int32_t* tile_cols)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    const TilePlan pl = plan(desc);
    if (tile_rows) *tile_rows = pl.TY;
    if (tile_cols) *tile_cols = pl.TX;
    return pl.lds;
}

extern "C" int stego_probe_confusion(const StegoProbeConfusionDesc* desc, const StegoMap* code, const StegoMap* code_flip,
                                     const float* lin_w, const float* lin_b, const float* centroids, const int64_t* labels,
                                     int64_t* lin_counts, int64_t* clu_counts, stego_stream_t stream)
{
    int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    const bool lin = desc->lin_on != 0, clu = desc->clu_on != 0;
    if (!labels) return STEGO_ERR_NULL;                 // (with the other NULL tests: a NULL anywhere comes before an alignment)
    rc = check_probe_ptrs(code, code_flip, lin, lin_w, lin_b, lin_counts, 8, clu, centroids, clu_counts, 8);
    if (rc != STEGO_OK) return rc;
    if (!aligned(labels, 8)) return STEGO_ERR_ALIGN;

    const TilePlan pl = plan(desc);
    if (pl.lds > LDS_BUDGET) return STEGO_ERR_UNSUPPORTED;          // (unreachable: a 1 x 1 tile's footprint and both histograms fit)
    ConfParams p{};
    p.maps.code = *code;
    p.maps.flip = code_flip ? *code_flip : StegoMap{nullptr, 0, 0, 0, 0};
    p.maps.labels = labels;
    p.has_flip = code_flip != nullptr;
    p.lin_w = lin_w;
    p.lin_b = lin_b;
    p.cent = centroids;
    p.maps.lin_counts = reinterpret_cast<unsigned long long*>(lin_counts);
    p.maps.clu_counts = reinterpret_cast<unsigned long long*>(clu_counts);
    p.K = desc->K;
    p.h = desc->h;
    p.w = desc->w;
    p.H = desc->H;
    p.W = desc->W;
    p.n_lin = lin ? desc->n_lin : 0;      // a skipped probe has no live label slot: its n, weights and counts are never read
    p.n_clu = clu ? desc->n_clu : 0;
    p.n_classes = desc->n_classes;
    p.maps.alpha = desc->alpha;
    p.maps.scale_h = pl.scale_h;
    p.maps.scale_w = pl.scale_w;
    p.TY = pl.TY;
    p.TX = pl.TX;
    p.max_nr = pl.max_nr;
    p.max_nc = pl.max_nc;
    p.K4 = pl.K4;
    p.KS = pl.KS;
    p.ntx = (desc->W + pl.TX - 1) / pl.TX;
    p.tpi = p.ntx * ((desc->H + pl.TY - 1) / pl.TY);
    p.B = desc->B;
    const int64_t tiles = (int64_t)p.tpi * desc->B;
    const unsigned grid = (unsigned)std::min(tiles, std::max((int64_t)stego::device_cu_count() * WGS_PER_CU, tiles * TPB / MAX_WG_PIXELS + 1));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    return hip_rc(stego::with_const<8, 16, 32, 64>(pl.NMAX, [&](auto N) { return stego::launch_first<probe_confusion_kernel<N()>>(grid, TPB, pl.lds, s, p); }));
}

extern "C" int stego_confusion(const StegoConfusionDesc* desc, const void* pred, const int64_t* labels, int64_t* counts,
                               stego_stream_t stream)
{
    if (!desc || !pred || !labels || !counts) return STEGO_ERR_NULL;
    if (desc->pred_kind != STEGO_CONF_LABELS && desc->pred_kind != STEGO_CONF_SCORES) return STEGO_ERR_CONF_KIND;
    if (desc->n < 1 || desc->n > STEGO_CONF_MAX_N || desc->n_classes < 1 || desc->n_classes > STEGO_CONF_MAX_N) return STEGO_ERR_CONF_DIM;
    if (desc->B < 1 || desc->H < 1 || desc->W < 1) return STEGO_ERR_CONF_SIZE;
    const int64_t HW = (int64_t)desc->H * desc->W;                  // < 2^62
    if (HW >= STEGO_CONF_MAX_PIXELS || desc->B >= (STEGO_CONF_MAX_PIXELS + HW - 1) / HW) return STEGO_ERR_CONF_SIZE;
    const bool scores = desc->pred_kind == STEGO_CONF_SCORES;
    if (!aligned(pred, scores ? 4 : 8) || !aligned(labels, 8) || !aligned(counts, 8)) return STEGO_ERR_ALIGN;

    CountParams p{};
    p.pred = pred;
    p.labels = labels;
    p.counts = reinterpret_cast<unsigned long long*>(counts);
    p.n = desc->n;
    p.n_classes = desc->n_classes;
    p.HW = HW;
    p.total = HW * desc->B;
    const int64_t rounds = (p.total + TPB - 1) / TPB;
    const unsigned grid = (unsigned)std::min(rounds, std::max((int64_t)stego::device_cu_count() * WGS_PER_CU, p.total / MAX_WG_PIXELS + 1));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (scores) return hip_rc(stego::launch_first<confusion_count_kernel<true>>(grid, TPB, 0, s, p));
    return hip_rc(stego::launch_first<confusion_count_kernel<false>>(grid, TPB, 0, s, p));
}
