// Backward of STEGO's ContrastiveCorrelationLoss w.r.t. orig_code / orig_code_pos (gfx950): the general path and the dispatch.
//
// Every backward is two launches, no global atomics, no memsets: a tile launch (corr_bwd_tile.h: per (pair-set, image) tile the
// gradient w.r.t. the raw sampled codes, DT[tile][side][128][LDK]) and an unsample launch (the adjoint of the bilinear sampling,
// grid_sampler_2d_backward, and of the orig_code[perm] gather, index_put, modules.py:385, as a GATHER per destination pixel).
// launch_corr_bwd() computes one plan (corr_bwd_plan.h: bwd_plan) and switches on it:
//
//   lists first   corr_bwd_tile_build_kernel / corr_bwd_tile32_build_kernel + corr_unsample_list_kernel (corr_bwd_lists.hip):
//                 training - forward() semantics, scalar upstreams, maps up to 64 x 64
//   tile + row    corr_bwd_tile_h_kernel (split-fp16) / corr_bwd_tile_kernel (fp32) + corr_unsample_row_kernel, this file: dense
//                 upstreams, helper(), maps taller than 64, STEGO_DEBUG_BWD 1024
//   tile + band   the same tile kernels + corr_unsample_kernel (rows in an LDS band, worklists, plain LDS read-modify-write), this
//                 file: maps wider than 64 pixels, STEGO_DEBUG_BWD 32
//
// The first version of this backward scattered with 15 M global fp32 atomics (93 of its 136 us).
//
// Reference: autograd through src/modules.py:335-347, 369-391.
#include "corr_bwd_plan.h"
#include "corr_bwd_tile.h"
#include "corr_common.h"
#include "host_util.h"
#include "launchers.h"

namespace stego {

template <int NT>
__global__ void __launch_bounds__(NTHREADS) corr_bwd_tile_kernel(const BwdParams prm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bwd_tile_body<NT>(prm, (int)blockIdx.x, smem);
}

template <int NT, bool DENSE>
__global__ void __launch_bounds__(HW_THREADS) corr_bwd_tile_h_kernel(const BwdParams prm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    bwd_tile_h_body<NT, DENSE>(prm, (int)blockIdx.x, smem);
}

// ------------------------------------------------------------------------------- unsample
// grid = n_dest(2) * B * n_bands ; block = 512 (8 waves); a band has RT <= 8 pixel rows and WAVE r OWNS ROW r.
// LDS: float acc[RT][W][K] | contribution table | per-row worklists | counters.
// Per round, 4 contributions x 128 points are tested lane-parallel; every tap row that falls in the band
// appends a 16-byte row-entry {DT row, x0|x1, w0, w1} to the list of that pixel row.  The owning wave then
// drains its list: 16 DT rows in flight per lane, plain LDS read-modify-write (LDS fp32 atomics measured
// ~1000 cycles per wave-instruction on gfx950, so they are used only on worklist overflow).
constexpr int UNS_SETS_PER_ROUND = UNS_THREADS / TP;      // 4

struct UnsRowEntry {        // UNS_ENTRY_BYTES
    int dtoff;              // float offset of the DT row
    int x01;                // x0 | x1 << 16
    float wa, wb;           // tap weights at (row, x0), (row, x1)
};
static_assert(sizeof(UnsRowEntry) == UNS_ENTRY_BYTES, "bwd_plan sizes the worklists");

__global__ void __launch_bounds__(UNS_THREADS) corr_unsample_kernel(const BwdParams prm, const int RT, const int n_bands,
                                                                   const int acc_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* acc = reinterpret_cast<float*>(smem);
    int* ctab = reinterpret_cast<int*>(smem + acc_bytes);                               // [UNS_MAX_CONTRIB]
    UnsRowEntry* wl = reinterpret_cast<UnsRowEntry*>(smem + acc_bytes + UNS_MAX_CONTRIB * 4);   // [UNS_MAX_RT][UNS_ROW_CAP]
    int* cnt = reinterpret_cast<int*>(smem + acc_bytes + UNS_MAX_CONTRIB * 4 + UNS_MAX_RT * UNS_ROW_CAP * (int)sizeof(UnsRowEntry));
    int& s_nc = cnt[UNS_MAX_RT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = prm.B, P = prm.P, K = prm.K, W = prm.W, H = prm.H, ldk = prm.LDK;
    const bool direct = prm.mode == 1;
    int bid = blockIdx.x;
    const int band = bid % n_bands; bid /= n_bands;
    const int j = bid % B;
    const int dest = bid / B;                        // 0: d_code (d_c1), 1: d_code_pos (d_c2)
    const int r0 = band * RT, r1 = min(H, r0 + RT);
    const int band_elems = (r1 - r0) * W * K;
    const int side_elems = TP * ldk;
    for (int e = tid; e < band_elems; e += UNS_THREADS) acc[e] = 0.f;

    // ---- contribution table: every contribution is (taps of sample set s, DT matrix (tile, side)).
    //   own role of image j, entries [0, n_own):
    //       dest 0: anchor set j with the A side of EVERY pair-set tile (p, j)      -> n_own = n_sets
    //       dest 1: positive set B+j with the B side of tile (1, j); helper: set dest*B+j, tile j, side dest
    //   then (dest 0 only) the negative sets (2+i)*B+b with perm_i[b] == j, B side of their own tile
    //   (the index_put of orig_code[perm], modules.py:385).   ctab[c] holds the set id of entry c >= n_own.
    const int n_own = (!direct && dest == 0) ? prm.n_sets : 1;
    if (wave == 0) {
        int nc = n_own;
        if (!direct && dest == 0) {
            for (int i = 0; i < prm.n_neg; ++i)
                for (int b0 = 0; b0 < B; b0 += 64) {
                    const int bb = b0 + lane;
                    const bool m = bb < B && (int)prm.perms[(size_t)i * B + bb] == j;
                    const unsigned long long mask = __ballot(m);
                    const int pre = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
                    if (m && nc + pre < UNS_MAX_CONTRIB) ctab[nc + pre] = (2 + i) * B + bb;
                    nc += __builtin_popcountll(mask);
                }
            if (nc > UNS_MAX_CONTRIB) nc = UNS_MAX_CONTRIB;        // (cannot happen: bwd_check)
        }
        if (lane == 0) s_nc = nc;
    }
    __syncthreads();
    const int NC = s_nc;
    

    for (int c0 = 0; c0 < NC; c0 += UNS_SETS_PER_ROUND) {
        if (tid < UNS_MAX_RT) cnt[tid] = 0;
        __syncthreads();
        // ---- phase 1: thread -> (contribution c0 + tid/128, point tid%128): band test, append row-entries
        {
            const int c = c0 + (tid >> 7), q = tid & (TP - 1);
            if (c < NC && q < P && !(prm.debug & BWD_DBG_NO_SCATTER)) {
                int s, tile0, side;
                if (c < n_own) {
                    if (direct) { s = dest * B + j; tile0 = j; side = dest; }
                    else if (dest == 1) { s = B + j; tile0 = B + j; side = 1; }
                    else { s = j; tile0 = c * B + j; side = 0; }
                } else { s = ctab[c]; tile0 = s; side = 1; }
                const int4 yx = prm.tapyx[(size_t)s * TP + q];
                const float4 w = prm.tapw[(size_t)s * TP + q];
                const int dtoff = (tile0 * 2 + side) * side_elems + q * ldk;
#pragma unroll
                for (int hrow = 0; hrow < 2; ++hrow) {
                    const int y = (hrow ? yx.z : yx.x) >> 16;
                    const float wa = hrow ? w.z : w.x, wb = hrow ? w.w : w.y;
                    if (y < r0 || y >= r1 || (wa == 0.f && wb == 0.f)) continue;
                    if (hrow == 1 && y == (yx.x >> 16)) continue;          // clamped second row: weights are 0 anyway
                    const int xa = (hrow ? yx.z : yx.x) & 0xffff, xb = (hrow ? yx.w : yx.y) & 0xffff;
                    const int row = y - r0;
                    const int slot = atomicAdd(&cnt[row], 1);
                    if (slot < UNS_ROW_CAP) {
                        UnsRowEntry e;
                        e.dtoff = dtoff; e.x01 = xa | (xb << 16); e.wa = wa; e.wb = wb;
                        wl[row * UNS_ROW_CAP + slot] = e;
                    } else {
                        // overflow (pathological coords, e.g. every point on one row): slow but correct path
                        for (int ch = 0; ch < K; ++ch) {
                            const float v = prm.dt[dtoff + ch];
                            if (wa != 0.f) atomicAdd(&acc[(row * W + xa) * K + ch], wa * v);
                            if (wb != 0.f) atomicAdd(&acc[(row * W + xb) * K + ch], wb * v);
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- phase 2: wave r drains the list of pixel row r (lanes = channels, second pass for channels >= 64)
        if (wave < r1 - r0) {
            const int count = min(cnt[wave], UNS_ROW_CAP);
            const UnsRowEntry* list = wl + wave * UNS_ROW_CAP;
            float* arow = acc + wave * W * K;
            constexpr int UB = 16;
            // branch-free: lanes without a channel (and clamped second taps) are redirected to a per-lane
            // dummy cell behind the band, so every load / read-modify-write is unconditional
            const int cA = min(lane, K - 1), cB = min(64 + lane, K - 1);
            const bool hasA = lane < K, hasB = 64 + lane < K;
            float* dummy = acc + (acc_bytes >> 2) - 4 * 64 + lane;
            for (int e0 = 0; e0 < count; e0 += UB) {
                float v0[UB], v1[UB], wa[UB], wb[UB];
                int x01[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const UnsRowEntry en = list[min(e0 + u, count - 1)];
                    const bool on = e0 + u < count;
                    x01[u] = en.x01; wa[u] = on ? en.wa : 0.f; wb[u] = on ? en.wb : 0.f;
                    v0[u] = prm.dt[en.dtoff + cA];
                    v1[u] = prm.dt[en.dtoff + cB];
                }
                if (!(prm.debug & BWD_DBG_ONE_LOAD)) {
#pragma unroll
                    for (int u = 0; u < UB; ++u) {
                        // the (up to) 4 cells of one row-entry are distinct: read all, then write all
                        const int xa = x01[u] & 0xffff, xb = x01[u] >> 16;
                        const bool two = xb != xa;                 // clamped tap (xb == xa) carries weight 0
                        float* pa0 = hasA ? arow + xa * K + lane : dummy;
                        float* pb0 = (hasA && two) ? arow + xb * K + lane : dummy + 64;
                        float* pa1 = hasB ? arow + xa * K + 64 + lane : dummy + 128;
                        float* pb1 = (hasB && two) ? arow + xb * K + 64 + lane : dummy + 192;
                        const float a0 = *pa0, b0 = *pb0, a1 = *pa1, b1 = *pb1;
                        *pa0 = a0 + wa[u] * v0[u];
                        *pb0 = b0 + wb[u] * v0[u];
                        *pa1 = a1 + wa[u] * v1[u];
                        *pb1 = b1 + wb[u] * v1[u];
                    }
                }
            }
        }
        __syncthreads();
    }
    float* out = (dest == 0 ? prm.d_code : prm.d_code_pos) + ((size_t)j * H + r0) * W * K;
    for (int e = tid; e < band_elems; e += UNS_THREADS) out[e] = acc[e];
}


// ------------------------------------------------------------------------------- unsample, row-owned
// The fast path (W <= 64): ONE PIXEL ROW of one destination image is owned by a wave (or by the 3 waves of a
// workgroup) and lives in REGISTERS as MFMA accumulators.  The bilinear adjoint of a row is a tiny sparse GEMM
//        row[x][ch] += sum_e  onehot_e[x] * DT_e[ch],      onehot_e[x] = wa_e (x == x0_e), wb_e (x == x0_e+1), 0
// and it is issued exactly like that on v_mfma_f32_16x16x4_f32 (M = 16 pixels, N = 16 channels, K = 4
// row-entries): no dynamic register indexing, no branches, no LDS read-modify-write chain (the LDS-band
// version measured ~500 cycles per entry; a wave-uniform switch over register accumulators made the
// structurizer emit 15 k accumulator copies).  No atomics, deterministic summation order.
//
// The kernel is bound by DEPENDENT LOAD ROUND TRIPS (~2 us each with 4 k waves in flight, measured with
// s_memrealtime stamps), neither by bytes nor by flops, so it is shaped to need three of them:
//   1. perms  -> items : the DT matrices that touch this image (anchor role: A side of every pair-set tile of
//                        the image; negatives: the (i,b) with perm_i[b] == image, found with ballots)
//   2. scan           : the (y0 << 16 | x0) word of every point of <= 6 items; points whose upper or lower
//                        tap row is MY row are compacted (ballot + mbcnt) into a 4-byte worklist in LDS
//   3. drain          : 40 entries per step; the 16 lanes of entry k = lane / 16 load its DT row (B operand,
//                        5 dwords per lane) AND its 32-byte tap record (one dword per lane, spread to the group
//                        with ds_bpermute) in the same round; the A operand is the one-hot weight of pixel lane % 16
// and every row has to be in flight at once (register budget: 128 VGPRs -> 4 waves per SIMD -> 4096 waves).
// Rows of the anchor image (forward mode, dest 0) collect ~12 items, the others one: a HEAVY row gets a
// workgroup whose 3 waves take every 3rd item and reduce-scatter their partial rows through LDS at the end;
// light rows are one wave each.
constexpr int UR_GROUP = 6;          // items scanned per step; a point hits a row at most once -> <= 6*128 entries
constexpr int UR_CAP = UR_GROUP * TP;
constexpr int UR_ITEMCAP = 96;       // a pass looks at 256 candidates; only heavy rows have > 1, split over 3 waves
// UR_NT (template): 16-channel tiles, 5 for K <= 80, 8 for K <= 128.  UR_EG: groups of 4 entries per drain step
// (NT = 5: 9 groups = 54 loads in flight per lane; NT = 8: 5 groups = 45)

template <int MT, int UR_NT>        // 16-pixel tiles per row: W <= 16 * MT; 16-channel tiles: K <= 16 * UR_NT
__global__ void __launch_bounds__(UR_WAVES * 64, (MT <= 2 && UR_NT <= 5) ? 4 : 2) corr_unsample_row_kernel(const BwdParams prm)
{
    constexpr int UR_EG = UR_NT <= 5 ? 9 : 5;
    constexpr int RED_BYTES = UR_WAVES * UR_NT * 64 * (int)sizeof(f32x4);          // reduction buffer, aliases the worklists
    constexpr int WL_BYTES = UR_WAVES * MT * UR_CAP * 4;      // one worklist per 16-pixel tile
    __shared__ __attribute__((aligned(16))) unsigned char wl_raw[RED_BYTES > WL_BYTES ? RED_BYTES : WL_BYTES];
    __shared__ __attribute__((aligned(8))) int2 items_s[UR_WAVES][UR_ITEMCAP];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int B = prm.B, P = prm.P, K = prm.K, W = prm.W, H = prm.H, ldk = prm.LDK;
    const bool direct = prm.mode == 1;
    const int n_heavy = direct ? 0 : B * H;                 // units are (dest, image j, row r); heavy dest 0 first
    const bool heavy = (int)blockIdx.x < n_heavy;
    const int unit = heavy ? (int)blockIdx.x : n_heavy + ((int)blockIdx.x - n_heavy) * UR_WAVES + wave;
    const int sub = heavy ? wave : 0, nsub = heavy ? UR_WAVES : 1;
    if (unit >= 2 * B * H) return;
    const int r = unit % H;
    const int j = (unit / H) % B;
    const int dest = unit / (H * B);
    int* wl = reinterpret_cast<int*>(wl_raw) + wave * MT * UR_CAP;
    int2* items = items_s[wave];
    const int side_elems = TP * ldk;
    const int n_own = (!direct && dest == 0) ? prm.n_sets : 1;
    const int n_cand = n_own + ((!direct && dest == 0) ? prm.n_neg * B : 0);
    const int l16 = lane & 15, k4 = lane >> 4;
    int cch[UR_NT];                                          // channel of this lane in each N tile, kept inside the DT row
#pragma unroll
    for (int nt = 0; nt < UR_NT; ++nt) cch[nt] = min(16 * nt + l16, ldk - 1);
    // word of the 32-byte tap record this lane fetches for its entry: lanes 0-3 the pixel words, 4-7 the weights
    // (32-bit offsets from uniform bases: one address VGPR per load instead of two)
    const int* tap_words = reinterpret_cast<const int*>(prm.tapyx);
    const unsigned meta_off = l16 < 4 ? (unsigned)l16
                                      : (unsigned)(reinterpret_cast<const int*>(prm.tapw) - tap_words) + (unsigned)(l16 & 3);
    const int grp_lane0 = lane & 48;

    f32x4 acc[MT][UR_NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < UR_NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // debug bit 8: start / end of every workgroup on the 100 MHz global clock (tools/stamps_bwd.py)
    unsigned long long* ts = reinterpret_cast<unsigned long long*>(prm.dt + (size_t)prm.n_sets * B * 2 * side_elems);
    const bool stamp_on = (prm.debug & BWD_DBG_STAMPS) && threadIdx.x == 0 && blockIdx.x < 4000;
    if (stamp_on) ts[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();

    int n_seen = 0;
    static_assert(UR_ITEMCAP * UR_WAVES >= 256 && UR_ITEMCAP <= 128, "item table vs candidate pass / 7-bit item index");
    for (int u0 = 0; u0 < n_cand; u0 += 256) {
        // ---- item table from the next 256 candidates (loads issued together)
        int n_items = 0;
        const int n_before = (n_seen + nsub - 1 - sub) / nsub;      // items this wave took in earlier passes
        {
            long long pv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = u0 + k * 64 + lane - n_own;
                pv[k] = (t >= 0 && t < n_cand - n_own) ? prm.perms[t] : -1;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int u = u0 + k * 64 + lane;
                bool m = false;
                int s = 0, tile0 = 0, side = 0;
                if (u < n_own) {
                    m = true;
                    if (direct) { s = dest * B + j; tile0 = j; side = dest; }
                    else if (dest == 1) { s = B + j; tile0 = B + j; side = 1; }
                    else { s = j; tile0 = u * B + j; side = 0; }
                } else if (u < n_cand) {
                    m = (int)pv[k] == j;                     // the index_put of orig_code[perm], modules.py:385
                    s = 2 * B + (u - n_own); tile0 = s; side = 1;
                }
                const unsigned long long mask = __ballot(m);
                const int ord = n_seen + lane_prefix(mask);          // this wave takes every nsub-th item
                if (m && ord % nsub == sub) items[ord / nsub - n_before] = make_int2(s, (tile0 * 2 + side) * side_elems);
                n_seen += __builtin_popcountll(mask);
            }
            n_items = (n_seen + nsub - 1 - sub) / nsub - n_before;
        }
        __builtin_amdgcn_wave_barrier();       // LDS is in-order per wave; this only pins the compiler

        for (int it_pos = 0; it_pos < n_items; it_pos += UR_GROUP) {
            // ---- scan a group of items: which points have a tap row on row r?  Only the (y0 << 16 | x0) word
            // of the tap record is read here; the lower row is y0 + 1 (a clamped lower row has zero weights).
            // An entry only feeds the 16-pixel tile(s) its two taps fall in, so entries are binned per tile
            // (x0 % 16 == 15 goes to two bins) and a group of 4 entries costs 5 MFMAs instead of 5 * MT: the
            // MFMA pipe is what this kernel saturates first (ablation: scan 7.6 us, + loads 12.5 us, + MFMA 25 us
            // before binning).
            int cnt[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) cnt[m] = 0;
            {
                int yx0[UR_GROUP][2];
#pragma unroll
                for (int g = 0; g < UR_GROUP; ++g) {
                    const int2 it = items[min(it_pos + g, n_items - 1)];
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        yx0[g][h] = reinterpret_cast<const int*>(prm.tapyx + (size_t)it.x * TP + h * 64 + lane)[0];
                }
#pragma unroll
                for (int g = 0; g < UR_GROUP; ++g) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int q = h * 64 + lane;
                        const int y0 = yx0[g][h] >> 16, x0 = yx0[g][h] & 0xffff;
                        const bool hit = it_pos + g < n_items && q < P && (y0 == r || y0 + 1 == r);
#pragma unroll
                        for (int m = 0; m < MT; ++m) {
                            const bool mine = hit && ((x0 >> 4) == m || x0 == 16 * m - 1);
                            const unsigned long long mask = __ballot(mine);
                            if (mine) wl[m * UR_CAP + cnt[m] + lane_prefix(mask)] = (it_pos + g) << 7 | q;
                            cnt[m] += __builtin_popcountll(mask);
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
            // virtual entry order: bin 0, padded to a multiple of 4, then bin 1, ...  (every group of 4 is one bin)
            int off[MT + 1];
            off[0] = 0;
#pragma unroll
            for (int m = 0; m < MT; ++m) off[m + 1] = off[m] + ((cnt[m] + 3) & ~3);
            int count = off[MT];

            // ---- drain: UR_EG groups of 4 entries per step, entry k = lane / 16 of each group
            if (prm.debug & BWD_DBG_ROW_NO_DRAIN) count = 0;                // ablation: no drain at all
            for (int e0 = 0; e0 < count; e0 += 4 * UR_EG) {
                float bv[UR_EG][UR_NT];
                int meta[UR_EG];
#pragma unroll
                for (int g = 0; g < UR_EG; ++g) {
                    const int eg = min(e0 + 4 * g, count - 4);               // group start (uniform), clamped
                    int m = 0;
#pragma unroll
                    for (int mm = 1; mm < MT; ++mm) m += eg >= off[mm] ? 1 : 0;
                    int base = 0, n = cnt[0], o = 0;
#pragma unroll
                    for (int mm = 1; mm < MT; ++mm) if (m == mm) { base = mm * UR_CAP; n = cnt[mm]; o = off[mm]; }
                    const int pk = wl[base + min(eg - o + k4, n - 1)];
                    const int2 it = items[pk >> 7];
                    const int q = pk & (TP - 1);
                    const unsigned rowoff = (unsigned)(it.y + q * ldk);
#pragma unroll
                    for (int nt = 0; nt < UR_NT; ++nt) bv[g][nt] = prm.dt[rowoff + (unsigned)cch[nt]];
                    meta[g] = tap_words[(unsigned)(it.x * TP + q) * 4u + meta_off];
                }
                __builtin_amdgcn_sched_barrier(0);          // every load is in flight before the first use waits
                if (prm.debug & BWD_DBG_ROW_LOADS_ONLY) {                        // ablation: loads only
                    float sum = 0.f;
#pragma unroll
                    for (int g = 0; g < UR_EG; ++g) {
                        sum += __builtin_bit_cast(float, meta[g]);
#pragma unroll
                        for (int nt = 0; nt < UR_NT; ++nt) sum += bv[g][nt];
                    }
                    acc[0][0][0] += sum;
                    continue;
                }
#pragma unroll
                for (int g = 0; g < UR_EG; ++g) {
                    const int eg = e0 + 4 * g;
                    if (eg < count) {                                          // uniform: skip the tail groups
                        int m = 0;
#pragma unroll
                        for (int mm = 1; mm < MT; ++mm) m += eg >= off[mm] ? 1 : 0;
                        int n = cnt[0], o = 0;
#pragma unroll
                        for (int mm = 1; mm < MT; ++mm) if (m == mm) { n = cnt[mm]; o = off[mm]; }
                        const int yx = __shfl(meta[g], grp_lane0, 64);
                        const int x0 = yx & 0xffff;
                        const int low = (yx >> 16) != r ? 2 : 0;       // my row is the lower tap row of this point
                        float wa = __builtin_bit_cast(float, __shfl(meta[g], grp_lane0 + 4 + low, 64));
                        float wb = __builtin_bit_cast(float, __shfl(meta[g], grp_lane0 + 5 + low, 64));
                        if (eg - o + k4 >= n) { wa = 0.f; wb = 0.f; }
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) {
                            if (m == mt) {                                     // uniform
                                const int dx = 16 * mt + l16 - x0;
                                const float a = dx == 0 ? wa : (dx == 1 ? wb : 0.f);
#pragma unroll
                                for (int nt = 0; nt < UR_NT; ++nt)
                                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[g][nt], acc[mt][nt], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }

    // ---- the row, once, from the accumulators: acc[mt][nt][reg] is pixel 16 mt + 4 (lane / 16) + reg,
    //      channel 16 nt + lane % 16
    float* out = (dest == 0 ? prm.d_code : prm.d_code_pos) + ((size_t)j * H + r) * W * K;
    if (!heavy) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int x = 16 * mt + 4 * k4 + reg;
#pragma unroll
                for (int nt = 0; nt < UR_NT; ++nt) {
                    const int ch = 16 * nt + l16;
                    if (x < W && ch < K) __builtin_nontemporal_store(acc[mt][nt][reg], out + (size_t)x * K + ch);
                }
            }
        return;
    }
    // heavy row: reduce-scatter the partial rows, one pixel tile (5 accumulator tiles) per round; wave w sums
    // and stores tiles w, w + 3.  The buffer aliases the (now idle) worklists.
    f32x4* red = reinterpret_cast<f32x4*>(wl_raw);             // [wave][5 tiles][64 lanes]
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < UR_NT; ++nt) red[(wave * UR_NT + nt) * 64 + lane] = acc[mt][nt];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < (UR_NT + UR_WAVES - 1) / UR_WAVES; ++t) {
            const int nt = wave + UR_WAVES * t;                // wave-uniform
            if (nt < UR_NT) {
                f32x4 v = red[nt * 64 + lane];
#pragma unroll
                for (int w2 = 1; w2 < UR_WAVES; ++w2) v += red[(w2 * UR_NT + nt) * 64 + lane];
                const int ch = 16 * nt + l16;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int x = 16 * mt + 4 * k4 + reg;
                    if (x < W && ch < K) __builtin_nontemporal_store(v[reg], out + (size_t)x * K + ch);
                }
            }
        }
    }
    if (stamp_on) ts[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
}

hipError_t launch_corr_bwd(const BwdParams& prm_in, hipStream_t stream)
{
    BwdParams prm = prm_in;
    const BwdShape shape{prm.B, prm.K, prm.H, prm.W, prm.S, prm.n_neg, prm.mode == 1, prm.precision};
    const bool dense = prm.g_intra_cd || prm.g_inter_cd || prm.g_neg_cd || (prm.g_neg_loss && prm.g_neg_loss_stride > 0);
    const BwdPlan pl = bwd_plan(shape, dense, prm.debug);
    prm.n_build = pl.n_build;
    if (pl.path == BwdPath::Invalid) return hipErrorInvalidValue;        // (helper() is limited to K <= 72 by check_desc)
    if (pl.path == BwdPath::Lists) return launch_corr_bwd_lists(prm, pl, stream);
    // ---- tile kernel.  Channel tiles of 16: 1 .. 5 (anything else: 5) in either precision; the split kernel alone goes on to 6, 7, 8 (anything beyond: 8)
    {
        const dim3 grid(pl.tile.grid), block(pl.tile.block);
        auto tile_h = [&](auto N) {
            return pl.dense ? launch<corr_bwd_tile_h_kernel<N(), true>>(grid, block, pl.tile.lds, stream, prm)
                            : launch<corr_bwd_tile_h_kernel<N(), false>>(grid, block, pl.tile.lds, stream, prm);
        };
        const hipError_t e = pl.nt > BWD_NT_F32_MAX ? with_const<6, 7, 8>(pl.nt, tile_h)
                             : pl.split ? with_const<1, 2, 3, 4, 5>(pl.nt, tile_h)
                                        : with_const<1, 2, 3, 4, 5>(pl.nt, [&](auto N) { return launch<corr_bwd_tile_kernel<N()>>(grid, block, pl.tile.lds, stream, prm); });
        if (e != hipSuccess) return e;
    }
    // ---- unsample
    const dim3 grid(pl.uns.grid), block(pl.uns.block);
    if (pl.path == BwdPath::TileBand) return launch<corr_unsample_kernel>(grid, block, pl.uns.lds, stream, prm, pl.rt, pl.n_bands, pl.acc_bytes);
    return with_const<2, 4>(pl.mt, [&](auto MT) {
        return with_const<5, 8>(pl.ur_nt, [&](auto NT) { return launch<corr_unsample_row_kernel<MT(), NT()>>(grid, block, pl.uns.lds, stream, prm); });
    });
}

}  // namespace stego
