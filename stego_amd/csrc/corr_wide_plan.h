// The wide loss path's one definition of its choices (corr_wide.hip, S * S > 128, and the building blocks the generic path reuses): the vector
// width of every point sampler, the prepared-operand GEMM a correlation takes, the code-channel windows of the backward's GEMM kernel, gather
// or scatter for the backward of the sampling, and the launch counts.  launch_sample_panels2 (sample_sets.hip), launch_dense_corr_panels_seg
// (dense_corr.hip), wide_geometry and launch_wide_bwd (corr_wide.hip) decide with these functions.  Plain C++17, no HIP include:
// tests/test_wide_variants_host.py compiles this header alone with g++ and walks tests/wide_variant_cases.py against it on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#include "corr_consts.h"

namespace stego {

// ---- what the width rules read of a map view: strides in floats and the address of element 0
struct MapFacts {
    long long sn, sc, sh, sw;
    uintptr_t addr;
};

// ---- sample_panels_kernel<VW1, VW2>: channels per lane and load of one side.  4: 16-byte loads (C % 4 == 0, C <= 1024), 2: 8-byte loads
// (C % 2 == 0, C <= 512), 0: any layout, scalar loads.  A vector width needs a dense channel axis, every other stride a multiple of it and
// the map (and the optional fp32 row output) aligned to the vector.  RowSampler holds PANEL_MAXJ vectors per lane: 64 * PANEL_MAXJ * vw channels.
constexpr int PANEL_MAXJ = 4;

constexpr bool panel_vw_ok(const MapFacts& m, int C, uintptr_t rows_out, int vw)
{
    return m.sc == 1 && C % vw == 0 && C <= 64 * PANEL_MAXJ * vw && m.sn % vw == 0 && m.sh % vw == 0 && m.sw % vw == 0 &&
           m.addr % (4 * (uintptr_t)vw) == 0 && rows_out % (4 * (uintptr_t)vw) == 0;        // (rows_out 0: no fp32 rows)
}

constexpr int panel_vw(const MapFacts& m, int C, uintptr_t rows_out)
{
    return panel_vw_ok(m, C, rows_out, 4) ? 4 : panel_vw_ok(m, C, rows_out, 2) ? 2 : 0;
}

// sample_gather_kernel<VEC> (stego_sample): 16-byte loads and stores along the channels, any C % 4 == 0 (the kernel loops over the row)
constexpr bool sample_gather_vec(const MapFacts& m, int C, uintptr_t out)
{
    return m.sc == 1 && C % 4 == 0 && m.sn % 4 == 0 && m.sh % 4 == 0 && m.sw % 4 == 0 && m.addr % 16 == 0 && out % 16 == 0;
}

// ---- the GEMM of two prepared operand sets (launch_dense_corr_panels_seg): images of 128-point blocks x PANEL_KC-channel chunks
constexpr int PANEL_KC = 64;          // channels per chunk (KC of corr_common.h)
constexpr int DR_MAXCH = 6;           // chunks the row-block kernel keeps of its A block in registers: C <= 384
constexpr int DR2_MAXCH = 2;          // chunks of the row-pair kernel (both row blocks of a pair in one workgroup): C <= 128

enum PanelDebug : int {               // STEGO_DEBUG bits the panel GEMM's dispatch reads
    PANEL_DBG_TILE = 8192,            // the tile kernel whatever the width
    PANEL_DBG_RING4 = 1 << 19,        // tools: the row-block kernel with four ring stages
    PANEL_DBG_NO_PAIR = 1 << 20,      // one row block per workgroup where the row-pair kernel would run
};

enum class PanelGemm { Invalid, RowPair, RowBlock, RowBlock4, Tile };      // Invalid: segmented outputs need a row kernel (hipErrorInvalidValue)

struct PanelGemmPlan {
    PanelGemm kernel;
    bool rowsum_launch;               // the tile kernel's workgroups see 128 columns: row sums take a launch of rowsum_kernel behind it
    int nbA, nbB, NCH;
    constexpr int launches() const { return kernel == PanelGemm::Invalid ? 0 : 1 + (rowsum_launch ? 1 : 0); }
};

constexpr PanelGemmPlan panel_gemm_plan(int C, int M, int N, bool segmented, bool want_rowsum, int debug)
{
    PanelGemmPlan p{};
    p.nbA = (M + TP - 1) / TP;
    p.nbB = (N + TP - 1) / TP;
    p.NCH = (C + PANEL_KC - 1) / PANEL_KC;
    if (p.NCH <= DR_MAXCH && !(debug & PANEL_DBG_TILE)) {
        if (p.nbA >= 2 && p.NCH <= DR2_MAXCH && !(debug & PANEL_DBG_NO_PAIR)) p.kernel = PanelGemm::RowPair;
        else p.kernel = (debug & PANEL_DBG_RING4) ? PanelGemm::RowBlock4 : PanelGemm::RowBlock;
        return p;                     // (the row kernels take the row sums on the way)
    }
    p.kernel = segmented ? PanelGemm::Invalid : PanelGemm::Tile;
    p.rowsum_launch = !segmented && want_rowsum;
    return p;
}

// ---- the backward's GEMM kernel (wide_bwd_kernel) takes the code channels in windows: both code tiles + G in 160 KB of LDS
constexpr int WB_MAXNB = 2;           // point blocks per side: S * S <= 256
constexpr int WB_MAXKB = 3;           // 32-channel blocks of one pass
constexpr int WB_WIN = 88;            // channels of one window at most (WB_MAXKB blocks hold 96; 88 is what the LDS holds)
constexpr int WIDE_MAX_K = 128;       // two windows

struct WideWindows {
    int nwin, Kc;                                         // Kc: channels of every window but the last, a multiple of 8
    constexpr int k0(int win) const { return win * Kc; }
    constexpr int kc(int win, int K) const { return K - k0(win) < Kc ? K - k0(win) : Kc; }
};

constexpr WideWindows wide_windows(int K)
{
    WideWindows w{};
    w.nwin = (K + WB_WIN - 1) / WB_WIN;
    w.Kc = (((K + w.nwin - 1) / w.nwin) + 7) & ~7;
    return w;
}

static_assert(WB_WIN <= 32 * WB_MAXKB && wide_windows(WIDE_MAX_K).nwin == 2 && wide_windows(WIDE_MAX_K).Kc <= WB_WIN, "K <= 128 in two windows");

// ---- the backward of norm() and of the sampling: a gather per destination pixel (lists built by a counting sort in LDS) for maps up to
// 4096 pixels whose list builder fits LDS, the one-wave-per-point scatter with fp32 atomics beyond
constexpr int WIDE_GATHER_MAX_HW = 4096;
constexpr int WIDE_LIST_THREADS = 512;
constexpr int WIDE_DBG_SCATTER = 1 << 20;             // STEGO_DEBUG_BWD: the scatter whatever the map
constexpr int WIDE_LDS_MAX_BYTES = 160 * 1024;

constexpr size_t wide_list_lds_bytes(int HW, int nnb)     // cnt[HW] | off[HW + 1] | srcs[n_neg B] | misc[2 + waves] (+ 4 spare words)
{
    return ((size_t)2 * HW + 1 + nnb + 2 + WIDE_LIST_THREADS / 64 + 4) * 4;
}

constexpr bool wide_gather(int B, int H, int W, int n_neg, int debug_bwd)
{
    return H * W <= WIDE_GATHER_MAX_HW && wide_list_lds_bytes(H * W, n_neg * B) <= (size_t)WIDE_LDS_MAX_BYTES - 1024 && !(debug_bwd & WIDE_DBG_SCATTER);
}

constexpr bool wide_supported_shape(int B, int C, int K, int S, int n_neg)
{
    const int P = S * S;
    return P > TP && P <= WB_MAXNB * TP && K <= WIDE_MAX_K && B >= 1 && C >= 1 && n_neg >= 0 && (long long)(2 + n_neg) * B <= 65535 &&
           (long long)(2 + n_neg) * B * P < (1ll << 31) / 4;
}

// ---- the whole path for one descriptor and the layout of its four maps
struct WideLayout {
    MapFacts feats, feats_pos, code, code_pos;
    uintptr_t ctx;                    // address of the saved context: the codes' normalised fp32 rows start there, image n at n * P * K floats
};

struct WidePlan {
    int vw[3][2];                     // sampler launch of source s (anchors | positives | negatives): sample_panels_kernel<vw[s][0], vw[s][1]>
    int n_sample;                     // sampler launches (the negatives' is dropped at n_neg == 0)
    PanelGemmPlan fd, cd;
    WideWindows win;
    bool gather;
    int fwd_launches, bwd_launches;
};

constexpr WidePlan wide_plan(int B, int C, int K, int H, int W, int S, int n_neg, bool pointwise, const WideLayout& l, int debug, int debug_bwd)
{
    WidePlan p{};
    const int P = S * S;
    const MapFacts* fm[3] = {&l.feats, &l.feats_pos, &l.feats};
    const MapFacts* cm[3] = {&l.code, &l.code_pos, &l.code};
    const int first[3] = {0, B, 2 * B};
    for (int s = 0; s < 3; ++s) {
        p.vw[s][0] = panel_vw(*fm[s], C, 0);              // (the fp32 rows of the features never exist)
        p.vw[s][1] = panel_vw(*cm[s], K, l.ctx + (uintptr_t)first[s] * P * K * 4);
    }
    p.n_sample = n_neg > 0 ? 3 : 2;
    p.fd = panel_gemm_plan(C, P, P, false, pointwise, debug);
    p.cd = panel_gemm_plan(K, P, P, true, false, debug);
    p.win = wide_windows(K);
    p.gather = wide_gather(B, H, W, n_neg, debug_bwd);
    p.fwd_launches = p.n_sample + p.fd.launches() + p.cd.launches() + 3;      // + set means, pointwise, loss means
    p.bwd_launches = 2 * p.win.nwin + (p.gather ? 2 : 2 + (n_neg > 0 ? 1 : 0));     // (tiles + GEMMs) per window; rows + gather, or the scatters
    return p;
}

}  // namespace stego
