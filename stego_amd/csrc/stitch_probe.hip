// Sliding-window segmentation of a canvas of any size (include/stego_stitch.h): the fused probe head over every window's
// low-resolution code, the overlapping windows blended per canvas pixel, in one launch that writes only the canvas; and the gather
// that cuts the windows (and their mirror images) out of the image for the backbone.
//
// stitch_probe_kernel.  Grid: (canvas column tiles, canvas row tiles).  A workgroup of 256 threads owns a TY x TX tile of canvas
// pixels, one per thread, and walks the windows that intersect it in ascending t = iy * nx + ix.  Per window it runs the probe head's
// phases (probe_phases.h, unchanged) on the part of the window under the tile, in window-local coordinates: the footprint's code,
// flip-averaged; its projections onto both probes; then every thread whose pixel lies inside the window takes the window's logits of
// its pixel and adds them, weighted, onto its register accumulators: acc = fmaf(a^, l, acc).  The phases get a mask of zeros; the label
// mask is added once after the last window, then finish() (softmax, log_softmax or argmax) stores the pixel.  A pixel under one window
// only (a^ = 1) is stored at once, by the head's own statements.  Windows come one after another, so the LDS need is the probe head's
// own plus the second mask and a copy of the kernel's parameters.  Window origins, the windows that reach a tile and the sum of the
// weights come from the layout's closed form: no origin arrays, nothing read but the codes and the weights.
//   With 64 label slots every probe has launches of its own: two 64-wide accumulators and the window's logits do not share the
// registers well, and finish() inside the window loop runs out of scalar registers there, so the pixels under one window get a
// launch without a loop (one workgroup per tile and window) and the pixels under several get the walk.  With fewer slots one walk
// serves both probes and every pixel.
//   The canvas tile lies anywhere in a window, unlike the head's tiles, so the plan takes the largest footprint over every start.
// No atomics, no workspace: repeat launches give the same bits.  Every output offset is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/stego_stitch.h"
#include "host_util.h"
#include "probe_phases.h"

namespace {

constexpr int TPB = PROBE_TPB;
constexpr size_t LDS_BUDGET = 64 * 1024;

// ---- the window layout's closed form, host and device
inline __host__ __device__ int axis_windows(int L, int win, int s) { return 1 + (L - win + s - 1) / s; }

// origin of window i: the last one is shifted back to end at the edge
inline __host__ __device__ int axis_origin(int i, int L, int win, int s) { return i * s < L - win ? i * s : L - win; }

// the first window that reaches position p: the smallest i with i * s + win > p (at most n - 1 for p < L)
inline __host__ __device__ int axis_first(int p, int win, int s) { return p < win ? 0 : (p - win) / s + 1; }

inline __host__ __device__ int tent(int u, int win) { return u + 1 < win - u ? u + 1 : win - u; }

// sum of tent over the windows that cover position p of the axis, and how many they are (at most 3)
__device__ inline int axis_tent_sum(int p, int L, int win, int s, int n, int& count)
{
    int sum = 0;
    count = 0;
    for (int i = axis_first(p, win, s); i < n; ++i) {
        const int o = axis_origin(i, L, win, s);
        if (o > p) break;
        sum += tent(p - o, win);
        ++count;
    }
    return sum;
}

// What finish() and the per-thread arithmetic read.
struct StitchMaps {
    StegoMap code, flip;             // flip.data == nullptr: no flip average
    void* lin_out;
    void* clu_out;
    int64_t HW;                      // canvas pixels
    float alpha, scale_h, scale_w;
    int32_t n_lin, n_clu, lin_kind, clu_kind;   // what finish() takes
};

// The kernel copies its parameters to LDS once and the window loop reads them from there, as confusion.hip does with its maps: held
// in scalar registers for the whole loop, beside the loop's own state and the NMAX comparison masks of an ARGMAX finish() inside
// the loop, they do not fit the scalar register file.  An LDS read cannot be hoisted over the loop's LDS stores, so each value is
// live only where it is used.
struct StitchParams {
    StitchMaps maps;
    const float* lin_w;
    const float* lin_b;
    const float* cent;
    int32_t K, hc, wc, H, W, win, stride, ny, nx;
    int32_t n_lin, n_clu;            // a skipped probe has n == 0
    int32_t has_flip;
    int32_t TY, TX, max_nr, max_nc;  // canvas tile, footprint capacity (rows, columns)
    int32_t K4, KS, NPS;             // as in probe_head.hip
    int32_t Y0, Y1, X0, X1;          // the workgroup's canvas tile: the kernel fills these in its LDS copy
};
constexpr int PARAMS_FLOATS = 64;    // sizeof(StitchParams) = 256 bytes: whole float4
static_assert(sizeof(StitchParams) <= PARAMS_FLOATS * sizeof(float) && PARAMS_FLOATS % 4 == 0, "StitchParams outgrew its LDS room");

// a pointer every lane holds alike, back in scalar registers: project() reads the weight rows with scalar loads
__device__ __forceinline__ const float* uniform_ptr(const float* ptr)
{
    const uint64_t v = reinterpret_cast<uint64_t>(ptr);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
}

// One sweep over the windows under the workgroup's tile [Y0, Y1) x [X0, X1) for the probes LIN / CLU name (and the descriptor has),
// then the stores.  Every thread of the workgroup runs the window loop (barriers); `has`: the thread has a canvas pixel.
// PASS: which pixels the sweep serves.  PASS_ALL: every pixel, in one walk over the windows.  With 64 label slots finish()'s first_max
// holds 63 comparison masks in scalar registers, which leaves no room for a loop's state around it, so the pixels under one window
// get a launch without a loop (PASS_SOLE: blockIdx.z names the one window of the tile the workgroup serves, out of at most
// SOLE_SLOTS per axis) and the pixels under several get the walk (PASS_BLEND).
enum { PASS_ALL = 0, PASS_SOLE = 1, PASS_BLEND = 2 };
// Windows over a tile per axis: indices from axis_first on while the origin is below the tile's end; the regular ones are fewer than
// (tile + win) / stride + 1 <= 2 * 2 + 1 (tile <= win <= 2 stride), the shifted last one adds one.
constexpr int SOLE_SLOTS = 6;

template <int NMAX, bool LIN, bool CLU, int PASS>
__device__ __forceinline__ void sweep(const StitchParams& p, float* cs, float* ps, const float* mask, const float* zero)
{
    const int Y0 = p.Y0, Y1 = p.Y1, X0 = p.X0, X1 = p.X1;
    const StitchMaps* const maps = &p.maps;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const float4* cs4 = reinterpret_cast<const float4*>(cs);
    const float4* ps4 = reinterpret_cast<const float4*>(ps);
    const float4* zero4 = reinterpret_cast<const float4*>(zero);
    const int KS4 = p.KS >> 2, NPS4 = p.NPS >> 2;
    const bool lin = LIN && p.n_lin != 0, clu = CLU && p.n_clu != 0;
    const int n_lin = lin ? p.n_lin : 0, n_clu = clu ? p.n_clu : 0;

    const int i = threadIdx.x;
    const int Y = Y0 + i / p.TX, X = X0 + i % p.TX;
    const bool has = i < p.TY * p.TX && Y < Y1 && X < X1;
    // the sum of a = tent(y) tent(x) over the covering windows is (sum of tent(y)) (sum of tent(x)): integers below 2^24, exact
    int cover_y = 1, cover_x = 1;
    const float total =
        has ? (float)(axis_tent_sum(Y, p.H, p.win, p.stride, p.ny, cover_y) * axis_tent_sum(X, p.W, p.win, p.stride, p.nx, cover_x))
            : 1.f;
    // One window over the pixel: a^ = 1, and acc = fmaf(1, l, 0) + mask is the probe head's own logits.  Such a pixel takes the head's
    // statement sequence as it stands (phases with the label mask, finish() at once), so that the compiler contracts the four-tap
    // expression as it does there and the stored bits are stego_probe_head's.
    const bool sole = cover_y * cover_x == 1;
    const int64_t pix = (int64_t)Y * p.W + X;
    const float4* mask4 = reinterpret_cast<const float4*>(mask);

    constexpr int NL = LIN && PASS != PASS_SOLE ? NMAX : 1, NC = CLU && PASS != PASS_SOLE ? NMAX : 1;
    float al[NL], ac[NC];
#pragma unroll
    for (int j = 0; j < NL; ++j) al[j] = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) ac[j] = 0.f;

    // window (iy, ix) with origin (oy, ox), which reaches the tile
    auto window = [&](int iy, int oy, int ix, int ox) __attribute__((always_inline)) {
        {
            const int ly0 = max(Y0 - oy, 0), ly1 = min(Y1 - oy, p.win);
            const int lx0 = max(X0 - ox, 0), lx1 = min(X1 - ox, p.win);
            const int64_t t = (int64_t)iy * p.nx + ix;
            __syncthreads();                                        // the window before is done with cs / ps; the first: the masks
            const float scale_h = maps->scale_h, scale_w = maps->scale_w;
            const Footprint f = tile_footprint(ly0, ly1, lx0, lx1, scale_h, scale_w, p.hc, p.wc, p.max_nr, p.max_nc);
            const StegoMap code = maps->code, flip = maps->flip;
            load_footprint(cs, code, flip, p.has_flip != 0, t, f, p.K, p.K4, p.KS, p.wc);
            __syncthreads();
            project<NMAX>(ps, cs, uniform_ptr(p.lin_w), uniform_ptr(p.lin_b), uniform_ptr(p.cent), n_lin, n_clu, p.K, p.KS, p.NPS,
                          f.npx, wave, lane);
            __syncthreads();

            const int y = Y - oy, x = X - ox;
            if (has && y >= 0 && y < p.win && x >= 0 && x < p.win) {
                const Taps tp = pixel_taps(y, x, scale_h, scale_w, p.hc, p.wc, f);
                if (sole) {
                    if constexpr (LIN && PASS != PASS_BLEND) {
                        if (lin) {
                            float l[NMAX];
                            linear_logits<NMAX>(l, ps4, mask4, NPS4, tp);
                            finish<NMAX>(l, maps->n_lin, maps->lin_kind, maps->lin_out, 0, maps->HW, pix);
                        }
                    }
                    if constexpr (CLU && PASS != PASS_BLEND) {
                        if (clu) {
                            const float den = code_norm(cs4, KS4, p.K4, tp);
                            float l[NMAX];
                            cluster_logits<NMAX>(l, ps4, mask4, NPS4, tp, den, maps->alpha);
                            finish<NMAX>(l, maps->n_clu, maps->clu_kind, maps->clu_out, 0, maps->HW, pix);
                        }
                    }
                } else {
                    const float a = (float)(tent(y, p.win) * tent(x, p.win)) / total;
                    if constexpr (LIN && PASS != PASS_SOLE) {
                        if (lin) {
                            float l[NMAX];
                            linear_logits<NMAX>(l, ps4, zero4, NPS4, tp);
#pragma unroll
                            for (int j = 0; j < NMAX; ++j) al[j] = fmaf(a, l[j], al[j]);
                        }
                    }
                    if constexpr (CLU && PASS != PASS_SOLE) {
                        if (clu) {
                            const float den = code_norm(cs4, KS4, p.K4, tp);
                            float l[NMAX];
                            cluster_logits<NMAX>(l, ps4, zero4, NPS4, tp, den, maps->alpha);
#pragma unroll
                            for (int j = 0; j < NMAX; ++j) ac[j] = fmaf(a, l[j], ac[j]);
                        }
                    }
                }
            }
        }
    };

    if constexpr (PASS == PASS_SOLE) {      // one window, named by blockIdx.z; the exits are the whole workgroup's
        const int iy = axis_first(Y0, p.win, p.stride) + (int)blockIdx.z / SOLE_SLOTS;
        const int ix = axis_first(X0, p.win, p.stride) + (int)blockIdx.z % SOLE_SLOTS;
        if (iy >= p.ny || ix >= p.nx) return;
        const int oy = axis_origin(iy, p.H, p.win, p.stride), ox = axis_origin(ix, p.W, p.win, p.stride);
        if (oy >= Y1 || ox >= X1) return;
        window(iy, oy, ix, ox);
        return;
    } else {
        for (int iy = axis_first(Y0, p.win, p.stride); iy < p.ny; ++iy) {
            const int oy = axis_origin(iy, p.H, p.win, p.stride);
            if (oy >= Y1) break;
            for (int ix = axis_first(X0, p.win, p.stride); ix < p.nx; ++ix) {
                const int ox = axis_origin(ix, p.W, p.win, p.stride);
                if (ox >= X1) break;
                window(iy, oy, ix, ox);
            }
        }
    }
    if (!has || sole) return;
    if constexpr (LIN && PASS != PASS_SOLE) {
        if (lin) {
#pragma unroll
            for (int j = 0; j < NMAX; ++j) al[j] += mask[j];
            finish<NMAX>(al, maps->n_lin, maps->lin_kind, maps->lin_out, 0, maps->HW, pix);
        }
    }
    if constexpr (CLU && PASS != PASS_SOLE) {
        if (clu) {
#pragma unroll
            for (int j = 0; j < NMAX; ++j) ac[j] += mask[NMAX + j];
            finish<NMAX>(ac, maps->n_clu, maps->clu_kind, maps->clu_out, 0, maps->HW, pix);
        }
    }
}

// LIN / CLU: the probes this instantiation can serve (the descriptor may still skip one of them); PASS: the pixels
template <int NMAX, bool LIN, bool CLU, int PASS>
__global__ __launch_bounds__(TPB) void stitch_probe_kernel(StitchParams prm)
{
    extern __shared__ float4 smem4[];
    StitchParams* const lp = reinterpret_cast<StitchParams*>(smem4);
    float* const cs = reinterpret_cast<float*>(smem4) + PARAMS_FLOATS;
    float* const ps = cs + (size_t)prm.max_nr * prm.max_nc * prm.KS;
    float* const mask = ps + (size_t)prm.max_nr * prm.max_nc * prm.NPS;   // [2 * NMAX]: 0 for a label of the probe, -inf for a pad slot
    float* const zero = mask + 2 * NMAX;                                  // [2 * NMAX] zeros: what the phases add to a window's logits

    init_mask<NMAX>(mask, prm.n_lin, prm.n_clu);
    if (threadIdx.x < 2 * NMAX) zero[threadIdx.x] = 0.f;
    if (threadIdx.x == 0) {
        *lp = prm;
        lp->Y0 = blockIdx.y * prm.TY;
        lp->X0 = blockIdx.x * prm.TX;
        lp->Y1 = min(lp->Y0 + prm.TY, prm.H);
        lp->X1 = min(lp->X0 + prm.TX, prm.W);
    }
    __syncthreads();
    sweep<NMAX, LIN, CLU, PASS>(*lp, cs, ps, mask, zero);
}

struct GatherParams {
    StegoMap img;
    float* out;
    float* out_flip;
    int32_t H, W, win, stride, nx, t0;
};

// Grid: (256-pixel pieces of a window plane, 3 channels, n windows); consecutive threads take consecutive columns of a row.
__global__ __launch_bounds__(TPB) void window_gather_kernel(GatherParams p)
{
    const int e = blockIdx.x * TPB + threadIdx.x;
    if (e >= p.win * p.win) return;
    const int y = e / p.win, x = e % p.win;
    const int c = blockIdx.y, t = p.t0 + (int)blockIdx.z;
    const int oy = axis_origin(t / p.nx, p.H, p.win, p.stride), ox = axis_origin(t % p.nx, p.W, p.win, p.stride);
    const float* row = p.img.data + (int64_t)c * p.img.stride_c + (int64_t)(oy + y) * p.img.stride_h + (int64_t)ox * p.img.stride_w;
    const int64_t o = (((int64_t)blockIdx.z * 3 + c) * p.win + y) * p.win + x;
    p.out[o] = row[(int64_t)x * p.img.stride_w];
    if (p.out_flip) p.out_flip[o] = row[(int64_t)(p.win - 1 - x) * p.img.stride_w];
}

using stego::aligned;
using stego::hip_rc;

inline bool kind_ok(int k) { return k >= STEGO_PROBE_SKIP && k <= STEGO_PROBE_ARGMAX; }

int check_layout(const StegoWindowLayout* l)
{
    if (l->H < 1 || l->H > STEGO_STITCH_MAX_SIDE || l->W < 1 || l->W > STEGO_STITCH_MAX_SIDE || l->win < 1 || l->win > STEGO_PROBE_MAX_OUT)
        return STEGO_ERR_STITCH_SIZE;
    if (l->win > l->H || l->win > l->W || l->stride > l->win || l->stride < 1 || 2 * l->stride < l->win) return STEGO_ERR_STITCH_LAYOUT;
    return STEGO_OK;
}

// everything but desc->T
int check_desc(const StegoStitchDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (!kind_ok(d->lin_kind) || !kind_ok(d->clu_kind) || (d->lin_kind == STEGO_PROBE_SKIP && d->clu_kind == STEGO_PROBE_SKIP))
        return STEGO_ERR_STITCH_OUTPUT;
    if (d->K < 1 || d->K > STEGO_PROBE_MAX_K) return STEGO_ERR_STITCH_DIM;
    if (d->lin_kind != STEGO_PROBE_SKIP && (d->n_lin < 1 || d->n_lin > STEGO_PROBE_MAX_N)) return STEGO_ERR_STITCH_DIM;
    if (d->clu_kind != STEGO_PROBE_SKIP && (d->n_clu < 1 || d->n_clu > STEGO_PROBE_MAX_N)) return STEGO_ERR_STITCH_DIM;
    if (d->hc < 1 || d->hc > STEGO_PROBE_MAX_CODE || d->wc < 1 || d->wc > STEGO_PROBE_MAX_CODE) return STEGO_ERR_STITCH_SIZE;
    return check_layout(&d->layout);
}

// max_span() of probe_common.h for a tile that starts anywhere in the window, not only at multiples of T
int max_span_any(int out, int in, float scale, int T)
{
    int best = 1;
    for (int t0 = 0; t0 < out; ++t0) {
        const int t1 = (t0 + T < out ? t0 + T : out) - 1;
        int a, b, u;
        host_src(t0, scale, in, a, u);
        host_src(t1, scale, in, u, b);
        best = b - a + 1 > best ? b - a + 1 : best;
    }
    return best + 1 < in ? best + 1 : in;
}

// The probe head's plan at the window's scale (plan_tile), its footprint capacity then widened to tiles at any offset and the tile
// halved further, by plan_tile's rule, should that no longer fit.
TilePlan plan(const StegoStitchDesc* d)
{
    const int n = std::max(d->lin_kind != STEGO_PROBE_SKIP ? d->n_lin : 0, d->clu_kind != STEGO_PROBE_SKIP ? d->n_clu : 0);
    const int win = d->layout.win;
    const size_t extra = (4 * label_slots(n) + PARAMS_FLOATS) * sizeof(float);    // the label mask, the mask of zeros, StitchParams
    TilePlan pl = plan_tile(d->K, d->hc, d->wc, win, win, n, extra, LDS_BUDGET);
    for (;;) {
        pl.max_nr = max_span_any(win, d->hc, pl.scale_h, pl.TY);
        pl.max_nc = max_span_any(win, d->wc, pl.scale_w, pl.TX);
        pl.lds = (size_t)pl.max_nr * pl.max_nc * (pl.KS + pl.NPS) * sizeof(float) + extra;
        if (pl.lds <= LDS_BUDGET || (pl.TY == 1 && pl.TX == 1)) break;
        if (pl.TY > 1)
            pl.TY = (pl.TY + 1) / 2;
        else
            pl.TX = (pl.TX + 1) / 2;
    }
    return pl;
}

}  // namespace

extern "C" size_t stego_stitch_probe_plan(const StegoStitchDesc* desc, int32_t* tile_rows, int32_t* tile_cols, int32_t* ny, int32_t* nx)
{
    if (check_desc(desc) != STEGO_OK) return 0;
    const TilePlan pl = plan(desc);
    const StegoWindowLayout& l = desc->layout;
    if (tile_rows) *tile_rows = pl.TY;
    if (tile_cols) *tile_cols = pl.TX;
    if (ny) *ny = axis_windows(l.H, l.win, l.stride);
    if (nx) *nx = axis_windows(l.W, l.win, l.stride);
    return pl.lds;
}

extern "C" int stego_stitch_probe(const StegoStitchDesc* desc, const StegoMap* code, const StegoMap* code_flip, const float* lin_w,
                                  const float* lin_b, const float* centroids, void* lin_out, void* clu_out, stego_stream_t stream)
{
    int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    const StegoWindowLayout& l = desc->layout;
    const int ny = axis_windows(l.H, l.win, l.stride), nx = axis_windows(l.W, l.win, l.stride);
    if ((int64_t)desc->T != (int64_t)ny * nx) return STEGO_ERR_STITCH_WINDOWS;
    const bool lin = desc->lin_kind != STEGO_PROBE_SKIP, clu = desc->clu_kind != STEGO_PROBE_SKIP;
    rc = check_probe_ptrs(code, code_flip, lin, lin_w, lin_b, lin_out, desc->lin_kind == STEGO_PROBE_ARGMAX ? 8 : 4, clu, centroids, clu_out,
                          desc->clu_kind == STEGO_PROBE_ARGMAX ? 8 : 4);
    if (rc != STEGO_OK) return rc;

    const TilePlan pl = plan(desc);
    if (pl.lds > LDS_BUDGET) return STEGO_ERR_UNSUPPORTED;          // (a 1 x 1 tile always fits: 4 footprint pixels at the most)
    StitchParams p{};
    p.maps.code = *code;
    p.maps.flip = code_flip ? *code_flip : StegoMap{nullptr, 0, 0, 0, 0};
    p.maps.lin_out = lin_out;
    p.maps.clu_out = clu_out;
    p.maps.alpha = desc->alpha;
    p.maps.scale_h = pl.scale_h;
    p.maps.scale_w = pl.scale_w;
    p.has_flip = code_flip ? 1 : 0;
    p.lin_w = lin_w;
    p.lin_b = lin_b;
    p.cent = centroids;
    p.K = desc->K;
    p.hc = desc->hc;
    p.wc = desc->wc;
    p.H = l.H;
    p.W = l.W;
    p.win = l.win;
    p.stride = l.stride;
    p.ny = ny;
    p.nx = nx;
    p.n_lin = lin ? desc->n_lin : 0;      // a skipped probe has no live label slot: its n, weights and output are never read
    p.n_clu = clu ? desc->n_clu : 0;
    p.maps.n_lin = p.n_lin;
    p.maps.n_clu = p.n_clu;
    p.maps.lin_kind = desc->lin_kind;
    p.maps.clu_kind = desc->clu_kind;
    p.maps.HW = (int64_t)l.H * l.W;
    p.TY = pl.TY;
    p.TX = pl.TX;
    p.max_nr = pl.max_nr;
    p.max_nc = pl.max_nc;
    p.K4 = pl.K4;
    p.KS = pl.KS;
    p.NPS = pl.NPS;
    const dim3 grid((unsigned)((l.W + pl.TX - 1) / pl.TX), (unsigned)((l.H + pl.TY - 1) / pl.TY));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (pl.NMAX < 64)                                   // (label_slots: 8, 16 or 32)
        return hip_rc(stego::with_const<8, 16, 32>(pl.NMAX, [&](auto N) {
            return stego::launch_first<stitch_probe_kernel<N(), true, true, PASS_ALL>>(grid, TPB, pl.lds, s, p);
        }));
    // 64 label slots: a probe at a time, the pixels one window covers first, then the blended ones
    const dim3 sole_grid(grid.x, grid.y, SOLE_SLOTS * SOLE_SLOTS);
    hipError_t e = hipSuccess;
    if (lin) {
        e = stego::launch_first<stitch_probe_kernel<64, true, false, PASS_SOLE>>(sole_grid, TPB, pl.lds, s, p);
        if (e == hipSuccess) e = stego::launch_next<stitch_probe_kernel<64, true, false, PASS_BLEND>>(grid, TPB, pl.lds, s, p);
    }
    if (clu && e == hipSuccess) {
        e = stego::launch_first<stitch_probe_kernel<64, false, true, PASS_SOLE>>(sole_grid, TPB, pl.lds, s, p);
        if (e == hipSuccess) e = stego::launch_next<stitch_probe_kernel<64, false, true, PASS_BLEND>>(grid, TPB, pl.lds, s, p);
    }
    return hip_rc(e);
}

extern "C" int stego_window_gather(const StegoWindowLayout* layout, const StegoMap* img, int32_t t0, int32_t n, float* out,
                                   float* out_flip, stego_stream_t stream)
{
    if (!layout) return STEGO_ERR_NULL;
    const int rc = check_layout(layout);
    if (rc != STEGO_OK) return rc;
    const int ny = axis_windows(layout->H, layout->win, layout->stride), nx = axis_windows(layout->W, layout->win, layout->stride);
    if (t0 < 0 || n < 1 || n > 65535 || (int64_t)t0 + n > (int64_t)ny * nx) return STEGO_ERR_STITCH_RANGE;
    if (!img || !img->data || !out) return STEGO_ERR_NULL;
    if (!aligned(img->data, 4) || !aligned(out, 4) || !aligned(out_flip, 4)) return STEGO_ERR_ALIGN;
    GatherParams p{};
    p.img = *img;
    p.out = out;
    p.out_flip = out_flip;
    p.H = layout->H;
    p.W = layout->W;
    p.win = layout->win;
    p.stride = layout->stride;
    p.nx = nx;
    p.t0 = t0;
    const dim3 grid((unsigned)((layout->win * layout->win + TPB - 1) / TPB), 3u, (unsigned)n);
    return hip_rc(stego::launch_first<window_gather_kernel>(grid, TPB, 0, static_cast<hipStream_t>(stream), p));
}
