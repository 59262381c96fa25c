// The loss backward's one definition of its workspace layout, its limits and its dispatch: which kernels run for a descriptor, with
// which grid, workgroup and LDS, and where in the workspace they find what.  c_api.hip sizes and carves the workspace from here, the
// launchers (corr_bwd.hip, corr_bwd_lists.hip) switch on the plan, the kernels index with the same constants.  Plain C++17, no HIP
// include: tests/test_bwd_plan_host.py compiles this header alone with g++ and walks it on the CPU.
#pragma once
#include <cstddef>

#include "../../include/stego_corr.h"
#include "corr_consts.h"

namespace stego {

// ---- STEGO_DEBUG_BWD (BwdParams::debug): measurement ablations and path overrides, one bit each
enum BwdDebug : int {
    BWD_DBG_NO_GEMM = 1,         // tile kernels: corr_bwd_tile_kernel runs no MFMA loop; the split-fp16 body skips both GEMMs (as it does for a zero upstream)
    BWD_DBG_NO_SCATTER = 2,      // corr_unsample_kernel (band): phase 1 appends no row-entries
    BWD_DBG_ONE_ROW = 4,         // split-fp16 tile body: every saved-w load reads row 0 (load ablation)
    BWD_DBG_STAMPS = 8,          // every kernel: s_memrealtime phase stamps into the BWD_STAMP_BYTES behind the DT rows (tools/stamps_bwd*.py)
    BWD_DBG_ONE_LOAD = 16,       // split-fp16 tile body: the code loads read one element; corr_unsample_kernel (band): lists are built, not drained
    BWD_DBG_BAND = 32,           // host: the LDS-band unsample where the row kernel would run (and no lists)
    BWD_DBG_ROW_LOADS_ONLY = 64, // corr_unsample_row_kernel: the drain's loads without its MFMAs
    BWD_DBG_ROW_NO_DRAIN = 128,  // corr_unsample_row_kernel: no drain at all
    BWD_DBG_F32_TILES = 512,     // host: the fp32-MFMA tile kernels in F16X3 mode as well (K <= 80 only: beyond, the launch is refused)
    BWD_DBG_NO_LISTS = 1024,     // host: tile + row kernels where lists first would run
    BWD_DBG_LATE_DB = 2048,      // split-fp16 tile body: both sides normalised and stored at the end (no early, written-through B side)
};

// ---- tile kernels: LDS carve (corr_bwd_tile.h)
constexpr int LDG = 130;                              // fp32 kernel: G row stride (floats)
constexpr int SMB_NRM = 0;                            // float nrm[2][128]
constexpr int SMB_AN = SMB_NRM + 2 * TP * 4;          // float An[128][LDK], then Bn[128][LDK], then G[128][LDG]
constexpr int HB_LDR = 136;                           // split kernel: halves per row of an operand image (272 B: conflict-free 8-byte reads)
constexpr int SMH_NRM = 0;                            // float nrm[2][128], red[8]
constexpr int SMH_CT = 1280;                          // half CT[side][hi|lo][16 ntg][HB_LDR], then Gh[128][HB_LDR], Gl[128][HB_LDR]
constexpr int HW_WAVES = 8;                           // waves of the split kernel (two per SIMD: the phases are latency chains)
constexpr int HW_THREADS = 64 * HW_WAVES;
constexpr int BWD_NT_F32_MAX = 5;                     // 16-channel tiles the fp32 kernel holds (K <= 80); the split kernel walks up to
constexpr int BWD_NT_MAX = 8;                         // 8 (K <= 128), beyond 5 in two groups that share the G image
constexpr int LDS_MAX_BYTES = 160 * 1024;             // what a gfx950 workgroup may ask for

// ---- unsample, LDS band (corr_unsample_kernel): maps wider than the row kernel's
constexpr int UNS_THREADS = 512;
constexpr int UNS_MAX_RT = 8;                         // pixel rows per band: one per wave
constexpr int UNS_ROW_CAP = 192;                      // row-entries per pixel row per round (expected ~35)
constexpr int UNS_ENTRY_BYTES = 16;                   // sizeof(UnsRowEntry)
constexpr int UNS_MAX_CONTRIB = 1024;                 // contribution table: n_sets + n_neg B entries at most (bwd_check)
constexpr int UNS_BAND_BYTES = 96 * 1024;             // fp32 accumulators of a band; one pixel row must fit (bwd_check)
constexpr int UNS_DUMMY_BYTES = 4 * 64 * 4 + 256;     // per-lane dummy cells behind the band
static_assert(UNS_MAX_RT == UNS_THREADS / 64, "wave r owns pixel row r of the band");

// ---- unsample, row-owned (corr_unsample_row_kernel<MT, UR_NT>)
constexpr int UR_WAVES = 3;
constexpr int BIN_W = 16;                             // pixels per bin: the M of the one-hot MFMA (row and list kernels)
constexpr int UR_MAX_MT = 4;                          // bins per row the row kernel holds in registers
constexpr int UR_MAX_W = BIN_W * UR_MAX_MT;

// ---- lists first (corr_bwd_lists.hip): builders' LDS and the list slots / overflow pool in the workspace
constexpr int BF_MAXH = 64;                           // maps up to BF_MAXH x (BIN_W BF_MAXMT)
constexpr int BF_MAXMT_LOG2 = 2, BF_MAXMT = 1 << BF_MAXMT_LOG2;       // a list key is (dest H + row) BF_MAXMT + bin
constexpr int BF_NKEY = 2 * BF_MAXH * BF_MAXMT;       // list keys of one image: (destination, pixel row, 16-pixel bin)
constexpr int BF_ITEM_CAP = 1032;                     // items of one destination image: n_sets + n_neg B, + 1 for dest 1's (bwd_check)
constexpr int UL_ENTRY_BYTES = 16;                    // a list entry {DT row (float index), x0, w_left, w_right}; a slot's header {count, overflow start}
constexpr int UL_CAP0 = 63, UL_CAP1 = 15;             // entries in the slot of a dest-0 / dest-1 unit, behind the header
constexpr int UL_SLOT0 = UL_ENTRY_BYTES * (UL_CAP0 + 1), UL_SLOT1 = UL_ENTRY_BYTES * (UL_CAP1 + 1);
constexpr int UL_POINT_ENTRIES = 4;                   // entries of one (item, point): two tap rows, at most two bins each
constexpr int UL_WAVES = 4;                           // corr_unsample_list_kernel: one wave per unit pair
constexpr int BFS_ITEMS = 0;                                          // int2[BF_ITEM_CAP]  {sample set, DT base (floats)}
constexpr int BFS_HIST = BFS_ITEMS + BF_ITEM_CAP * 8;                 // unsigned[HW_WAVES][BF_NKEY] counts, then running positions
constexpr int BFS_OVF = BFS_HIST + HW_WAVES * BF_NKEY * 4;            // unsigned[BF_NKEY] overflow start of every list (pool entries)
constexpr int BFS_SCAN = BFS_OVF + BF_NKEY * 4;                       // unsigned[HW_WAVES + 1] partial sums of the block scan
constexpr int BFS_MISC = BFS_SCAN + 64;                               // int[4]: items of dest 0, overflow slab of dest 0 / dest 1
constexpr int BF_LDS_BYTES = BFS_MISC + 64;
constexpr int BF_MAX_BUILDERS = 32;                   // builder workgroups in front of the tiles (B = 32: 224 tiles leave 32 CUs free)
constexpr size_t BWD_STAMP_BYTES = 65536;             // debug stamps behind the DT rows

static_assert(BF_NKEY % HW_THREADS == 0 && BF_NKEY % NTHREADS == 0, "whole keys per thread in the builders' prefix");
static_assert(UL_SLOT0 == 64 * UL_ENTRY_BYTES && UL_SLOT1 == 16 * UL_ENTRY_BYTES, "the list kernel reads a slot pair in one round: lane i of 64 / of 16 its header or entry i - 1");
static_assert((UL_CAP0 + 1) % 4 == 0 && (UL_CAP1 + 1) % 4 == 0, "groups of 4 entries per MFMA");
static_assert(BIN_W * BF_MAXMT <= UR_MAX_W, "whatever lists first covers, the row kernel covers too (debug 1024, dense upstreams)");
static_assert(BF_ITEM_CAP >= UNS_MAX_CONTRIB + 1, "items of dest 0 + the one of dest 1");
static_assert(BF_LDS_BYTES <= LDS_MAX_BYTES, "builders' tables");
static_assert(UNS_BAND_BYTES + UNS_DUMMY_BYTES + UNS_MAX_CONTRIB * 4 + UNS_MAX_RT * UNS_ROW_CAP * UNS_ENTRY_BYTES + 64 <= LDS_MAX_BYTES, "band kernel");
static_assert(SMH_CT >= SMH_NRM + (2 * TP + HW_WAVES) * 4, "nrm + red in front of the operand images");

// ---- what the rules read of a descriptor
struct BwdShape {
    int B, K, H, W, S, n_neg;      // (helper: S, n_neg unused)
    bool helper;                   // helper() on pre-sampled maps: one pair set, every pixel a point
    int precision;                 // PREC_*
    constexpr int n_sets() const { return helper ? 1 : 2 + n_neg; }
    constexpr int P() const { return helper ? H * W : S * S; }
    constexpr int KQ() const { return (K + 7) & ~7; }
    constexpr int LDK() const { return KQ() + 4; }
    constexpr int nt() const { return (KQ() + 15) / 16; }               // 16-channel tiles
    constexpr int bins() const { return (W + BIN_W - 1) / BIN_W; }      // 16-pixel bins per row
    constexpr size_t n_tiles() const { return (size_t)n_sets() * B; }
    constexpr size_t dt_elems() const { return n_tiles() * 2 * TP * LDK(); }
    constexpr size_t contributions() const { return (size_t)n_sets() + (helper ? 0 : (size_t)n_neg * B); }     // (tile, side) matrices that can land in one image
};

// ---- the workspace: DT rows | stamps | list slots | overflow pool
struct BwdWorkspace {
    size_t dt_bytes, stamp_bytes, slots_bytes, pool_bytes;     // slots / pool: 0 when the map is not the lists' (helper, H > BF_MAXH, W > BIN_W BF_MAXMT)
    size_t stamps_off, slots_off, pool_off, total;
    bool lists;                                                // slots and pool are there AND every buffer fits a 32-bit buffer resource
};

constexpr BwdWorkspace bwd_workspace(const BwdShape& s)
{
    BwdWorkspace w{};
    w.dt_bytes = round_up(s.dt_elems() * sizeof(float), 256);
    w.stamp_bytes = BWD_STAMP_BYTES;
    if (!s.helper && s.H <= BF_MAXH && s.W <= BIN_W * BF_MAXMT) {
        // a slot per (image, pixel row, 16-pixel bin) unit of orig_code and one per unit of orig_code_pos, and room for every entry
        // (at most UL_POINT_ENTRIES per (item, point)) in the overflow pool - an item is one (tile, side) whose gradient rows land in a
        // destination image: the anchors' A sides (n_sets B), the negatives' B sides (n_neg B), the positives' B sides (B)
        const size_t units = (size_t)s.B * s.H * s.bins();
        const size_t items = s.n_tiles() + (size_t)s.n_neg * s.B + s.B;
        w.slots_bytes = round_up(units * (UL_SLOT0 + UL_SLOT1), 256);
        w.pool_bytes = round_up((size_t)UL_POINT_ENTRIES * s.P() * items * UL_ENTRY_BYTES, 256);
    }
    w.stamps_off = w.dt_bytes;
    w.slots_off = w.stamps_off + w.stamp_bytes;
    w.pool_off = w.slots_off + w.slots_bytes;
    w.total = w.pool_off + w.pool_bytes;
    constexpr size_t rsrc_max = (size_t)1 << 32;
    w.lists = w.pool_bytes && w.dt_bytes < rsrc_max && w.pool_bytes < rsrc_max && w.slots_bytes < rsrc_max;
    return w;
}

// ---- limits beyond check_desc's: STEGO_OK or STEGO_ERR_UNSUPPORTED
constexpr int bwd_check(const BwdShape& s)
{
    if ((size_t)s.W * s.K * 4 > UNS_BAND_BYTES) return STEGO_ERR_UNSUPPORTED;          // one image row must fit the LDS band
    if (!s.helper && s.contributions() > UNS_MAX_CONTRIB) return STEGO_ERR_UNSUPPORTED;  // unsample contribution table, builders' item table
    return STEGO_OK;
}

// ---- the plan
enum class BwdPath { Invalid, Lists, TileRow, TileBand };      // Invalid: no kernel (hipErrorInvalidValue)

struct BwdLaunch { unsigned grid, block; int lds; };           // one-dimensional grids; lds = dynamic LDS bytes

struct BwdPlan {
    BwdPath path;
    // tile launch: Lists: corr_bwd_tile_build_kernel<nt> (split) / corr_bwd_tile32_build_kernel<nt>, n_build builder workgroups in front;
    //              otherwise corr_bwd_tile_h_kernel<nt, dense> (split) / corr_bwd_tile_kernel<nt>
    bool split, dense;
    int nt, n_build;
    BwdLaunch tile;
    // unsample launch
    BwdLaunch uns;
    int nq, tail;                  // Lists: corr_unsample_list_kernel<nq, tail>
    int mt, ur_nt, n_heavy;        // TileRow: corr_unsample_row_kernel<mt, ur_nt>; the first n_heavy workgroups are heavy rows
    int rt, n_bands, acc_bytes;    // TileBand: corr_unsample_kernel(rt, n_bands, acc_bytes)
};

// dense: some upstream gradient is a tensor (g_*_cd, or g_neg_loss with stride > 0) - not the training case
constexpr BwdPlan bwd_plan(const BwdShape& s, bool dense, int debug)
{
    BwdPlan p{};
    const int nt = s.nt(), ldk = s.LDK();
    // split-fp16 GEMMs in F16X3 mode and - whatever the mode - for code dimensions above 80, whose fp32 operand images no longer fit LDS
    // (the split kernel walks the channel tiles in two groups); helper() always takes the fp32 kernel (check_desc keeps it at K <= 72)
    p.split = !s.helper && !(debug & BWD_DBG_F32_TILES) && (s.precision == PREC_F16X3 || nt > BWD_NT_F32_MAX);
    p.dense = dense;
    p.nt = nt;
    if (nt > BWD_NT_F32_MAX && !p.split) return p;             // Invalid
    const int ntg = nt <= BWD_NT_F32_MAX ? nt : (nt + 1) / 2;  // channel tiles per operand group
    const int tile_lds = p.split ? SMH_CT + (4 * 16 * ntg + 2 * TP) * HB_LDR * 2 : SMB_AN + 2 * TP * ldk * 4 + TP * LDG * 4;
    const unsigned tile_block = p.split ? HW_THREADS : NTHREADS;
    const unsigned n_tiles = (unsigned)s.n_tiles();

    // lists first: forward() semantics on a map whose workspace carries lists (DT rows below 2^32 bytes: 32-bit byte offsets), scalar upstreams
    if (bwd_workspace(s).lists && !dense && !(debug & (BWD_DBG_BAND | BWD_DBG_NO_LISTS))) {
        p.path = BwdPath::Lists;
        p.n_build = s.B < BF_MAX_BUILDERS ? s.B : BF_MAX_BUILDERS;
        p.tile = BwdLaunch{(unsigned)p.n_build + n_tiles, tile_block, tile_lds < BF_LDS_BYTES ? BF_LDS_BYTES : tile_lds};
        // channels as nq x 64 (16-byte loads) + tail x 16 (4-byte loads)
        p.nq = s.K <= 80 ? 1 : 2;
        p.tail = s.K > 64 && s.K <= 80 ? 1 : 0;
        // every unit of image j on XCD j % 8: (B rounded up to 8) x (waves of an image's units, UL_WAVES per workgroup)
        const int upi = s.H * s.bins(), wpi = (upi + UL_WAVES - 1) / UL_WAVES;
        p.uns = BwdLaunch{(unsigned)(((s.B + 7) / 8) * 8 * wpi), 64 * UL_WAVES, 0};
        return p;
    }
    p.tile = BwdLaunch{n_tiles, tile_block, tile_lds};
    // row-owned register kernel for W <= UR_MAX_W (32-bit float offsets into DT), LDS band kernel beyond
    if (s.W <= UR_MAX_W && s.dt_elems() < ((size_t)1 << 31) && !(debug & BWD_DBG_BAND)) {
        p.path = BwdPath::TileRow;
        p.mt = s.W <= 2 * BIN_W ? 2 : UR_MAX_MT;
        p.ur_nt = s.KQ() > 16 * BWD_NT_F32_MAX ? BWD_NT_MAX : BWD_NT_F32_MAX;
        p.n_heavy = s.helper ? 0 : s.B * s.H;                  // units are (dest, image, row): the rows of dest 0 get a workgroup each,
        p.uns = BwdLaunch{(unsigned)(p.n_heavy + (2 * s.B * s.H - p.n_heavy + UR_WAVES - 1) / UR_WAVES), UR_WAVES * 64, 0};     // the others a wave
        return p;
    }
    // bands of rt <= UNS_MAX_RT rows (one per wave) with rt W K floats <= UNS_BAND_BYTES of LDS
    p.path = BwdPath::TileBand;
    const int row_bytes = s.W * s.K * 4;
    int rt = UNS_BAND_BYTES / row_bytes;
    if (rt > UNS_MAX_RT) rt = UNS_MAX_RT;
    if (rt < 1) rt = 1;
    if (rt > s.H) rt = s.H;
    p.n_bands = (s.H + rt - 1) / rt;
    p.rt = (s.H + p.n_bands - 1) / p.n_bands;                  // even bands
    p.acc_bytes = ((p.rt * row_bytes + 15) & ~15) + UNS_DUMMY_BYTES;
    p.uns = BwdLaunch{(unsigned)(2 * s.B * p.n_bands), UNS_THREADS,
                      p.acc_bytes + UNS_MAX_CONTRIB * 4 + UNS_MAX_RT * UNS_ROW_CAP * UNS_ENTRY_BYTES + 64};
    return p;
}

}  // namespace stego
