"""csrc/corr_bwd_plan.h is the loss backward's one definition of workspace layout, limits and dispatch (which kernels, grid, workgroup,
LDS).  The header is plain C++17, so a stand-alone g++ program - AddressSanitizer + UndefinedBehaviorSanitizer on, it is an ordinary
executable - walks it on the CPU: a table of expected plans, every boundary of the dispatch rules, and over a sweep of descriptors
the invariants the kernels call "host-checked".

The table's literals are what the commit BEFORE the plan header did: workspace totals from stego_corr_bwd_workspace_bytes /
stego_corr_helper_bwd_workspace_bytes of that library, kernel, grid and workgroup from a rocprofv3 kernel trace of
tests/test_bwd_fused.py and tests/test_parity_gpu.py on the MI355X (the trace reports threads; the table holds workgroups), dynamic LDS
from that commit's launch code (the trace reports static LDS only).  The two shapes one row / one column past the lists' map
(2, 32, 65, 16, ...) / (2, 32, 16, 65, ...) were not run by that commit's tests: their rows follow its rules by hand."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>

#include "corr_bwd_plan.h"

using namespace stego;

static int failures = 0;
#define CHECK(...) do { if (!(__VA_ARGS__)) { if (failures < 40) std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); ++failures; } } while (0)

constexpr int F32 = PREC_F32, F16 = PREC_F16X3;
constexpr BwdPath L = BwdPath::Lists, R = BwdPath::TileRow, D = BwdPath::TileBand, X = BwdPath::Invalid;

static BwdShape fwd(int B, int H, int W, int K, int S, int n_neg, int prec) { return BwdShape{B, K, H, W, S, n_neg, false, prec}; }

// what check_desc (c_api.hip) accepts of the fields the backward reads, one-tile path (S * S <= 128; beyond: corr_wide.hip's own backward)
static bool desc_ok(const BwdShape& s)
{
    if (s.B <= 0 || s.K <= 0 || s.H <= 0 || s.W <= 0 || s.H > 32767 || s.W > 32767) return false;
    if (s.helper) return s.K <= 72 && s.H * s.W <= TP;
    return s.K <= 128 && s.S > 0 && s.n_neg >= 0 && s.n_neg + 2 <= 256 && s.S * s.S <= TP;
}

struct Expect {
    BwdShape s; bool dense; int debug;
    size_t ws_total;
    BwdPath path; bool split; int nt, n_build;
    BwdLaunch tile, uns;
    int a, b, c;          // Lists: nq, tail, 0; TileRow: mt, ur_nt, n_heavy; TileBand: rt, n_bands, acc_bytes
};

static void expected_plans()
{
    const Expect table[] = {
        // BASELINE config 2 (test_bwd_fused: cfg-2 at full size, rotating contexts, the F32 case)
        {fwd(32, 28, 28, 70, 11, 5, F16), false, 0,    23013376, L, true,  5, 32, {256, 512, 157952}, {448, 256, 0}, 1, 1, 0},
        {fwd(32, 28, 28, 70, 11, 5, F16), false, 1024, 23013376, R, true,  5, 0,  {224, 512, 157952}, {1195, 192, 0}, 2, 5, 896},
        {fwd(32, 28, 28, 70, 11, 5, F32), false, 0,    23013376, L, false, 5, 32, {256, 256, 145408}, {448, 256, 0}, 1, 1, 0},
        {fwd(32, 28, 28, 70, 11, 5, F32), false, 1024, 23013376, R, false, 5, 0,  {224, 256, 145408}, {1195, 192, 0}, 2, 5, 896},
        // test_bwd_fused edge shapes (F16X3; those of the F32 test in both)
        {fwd(1, 8, 8, 8, 5, 0, F16), false, 0,    105216, L, true, 1, 1, {3, 512, 88320}, {16, 256, 0}, 1, 0, 0},
        {fwd(1, 8, 8, 8, 5, 0, F16), false, 1024, 105216, R, true, 1, 0, {2, 512, 88320}, {11, 192, 0}, 2, 5, 8},
        {fwd(3, 6, 9, 8, 5, 2, F16), false, 0,    269824, L, true,  1, 3, {15, 512, 88320}, {16, 256, 0}, 1, 0, 0},
        {fwd(3, 6, 9, 8, 5, 2, F16), false, 1024, 269824, R, true,  1, 0, {12, 512, 88320}, {24, 192, 0}, 2, 5, 18},
        {fwd(3, 6, 9, 8, 5, 2, F32), false, 0,    269824, L, false, 1, 3, {15, 256, 79872}, {16, 256, 0}, 1, 0, 0},
        {fwd(3, 6, 9, 8, 5, 2, F32), false, 1024, 269824, R, false, 1, 0, {12, 256, 79872}, {24, 192, 0}, 2, 5, 18},
        {fwd(4, 40, 40, 70, 11, 5, F16), false, 0,    3261696, L, true,  5, 4, {32, 512, 157952}, {240, 256, 0}, 1, 1, 0},
        {fwd(4, 40, 40, 70, 11, 5, F16), false, 1024, 3261696, R, true,  5, 0, {28, 512, 157952}, {214, 192, 0}, 4, 5, 160},
        {fwd(4, 40, 40, 70, 11, 5, F32), false, 0,    3261696, L, false, 5, 4, {32, 256, 145408}, {240, 256, 0}, 1, 1, 0},
        {fwd(4, 40, 40, 70, 11, 5, F32), false, 1024, 3261696, R, false, 5, 0, {28, 256, 145408}, {214, 192, 0}, 4, 5, 160},
        {fwd(2, 64, 64, 16, 7, 3, F16), false, 0,    982272, L, true, 1, 2, {12, 512, 88320}, {512, 256, 0}, 1, 0, 0},
        {fwd(2, 64, 64, 16, 7, 3, F16), false, 1024, 982272, R, true, 1, 0, {10, 512, 88320}, {171, 192, 0}, 4, 5, 128},
        {fwd(2, 12, 12, 100, 6, 2, F16), false, 0,    1013248, L, true, 7, 2, {10, 512, 140544}, {24, 256, 0}, 2, 0, 0},
        {fwd(2, 12, 12, 100, 6, 2, F16), false, 1024, 1013248, R, true, 7, 0, {8, 512, 140544}, {32, 192, 0}, 2, 8, 24},
        {fwd(5, 16, 16, 70, 11, 5, F16), false, 0,    3395328, L, true, 5, 5, {40, 512, 157952}, {32, 256, 0}, 1, 1, 0},
        {fwd(5, 16, 16, 70, 11, 5, F16), false, 1024, 3395328, R, true, 5, 0, {35, 512, 157952}, {107, 192, 0}, 2, 5, 80},
        {fwd(40, 8, 8, 24, 5, 5, F16), false, 0,    9335296, L, true,  2, 32, {312, 512, 105728}, {80, 256, 0}, 1, 0, 0},
        {fwd(40, 8, 8, 24, 5, 5, F16), false, 1024, 9335296, R, true,  2, 0,  {280, 512, 105728}, {427, 192, 0}, 2, 5, 320},
        {fwd(40, 8, 8, 24, 5, 5, F32), false, 0,    9335296, L, false, 2, 32, {312, 256, 96256}, {80, 256, 0}, 1, 0, 0},
        {fwd(40, 8, 8, 24, 5, 5, F32), false, 1024, 9335296, R, false, 2, 0,  {280, 256, 96256}, {427, 192, 0}, 2, 5, 320},
        // one row / one column past the lists' map: no slots in the workspace - the row kernel, the band kernel
        {fwd(2, 65, 16, 8, 5, 1, F16), false, 0,    139264, R, true, 1, 0, {6, 512, 88320}, {174, 192, 0}, 2, 5, 130},
        {fwd(2, 65, 16, 8, 5, 1, F16), false, 1024, 139264, R, true, 1, 0, {6, 512, 88320}, {174, 192, 0}, 2, 5, 130},
        {fwd(2, 16, 65, 8, 5, 1, F16), false, 0,    139264, D, true, 1, 0, {6, 512, 88320}, {8, 512, 46656}, 8, 2, 17920},
        {fwd(2, 16, 65, 8, 5, 1, F16), false, 1024, 139264, D, true, 1, 0, {6, 512, 88320}, {8, 512, 46656}, 8, 2, 17920},
        // test_bwd_fused: every negative from one image; linearity
        {fwd(16, 12, 20, 24, 7, 5, F16), false, 0,    4420608, L, true, 2, 16, {128, 512, 105728}, {96, 256, 0}, 1, 0, 0},
        {fwd(16, 12, 20, 24, 7, 5, F16), false, 1024, 4420608, R, true, 2, 0,  {112, 512, 105728}, {256, 192, 0}, 2, 5, 192},
        {fwd(4, 8, 8, 16, 5, 2, F16), false, 0, 478976, L, true, 1, 4, {20, 512, 88320}, {16, 256, 0}, 1, 0, 0},
        // test_parity_gpu edge shapes: W > 64 (band), 32 < W <= 64
        {fwd(2, 3, 70, 6, 4, 1, F32), false, 0, 139264, D, false, 1, 0, {6, 256, 79872}, {4, 512, 35056}, 3, 1, 6320},
        {fwd(2, 3, 70, 6, 4, 1, F16), false, 0, 139264, D, true,  1, 0, {6, 512, 88320}, {4, 512, 35056}, 3, 1, 6320},
        {fwd(2, 40, 40, 70, 11, 2, F32), false, 0, 1103872, L, false, 5, 2, {10, 256, 145408}, {240, 256, 0}, 1, 1, 0},
        {fwd(2, 40, 40, 70, 11, 2, F16), false, 0, 1103872, L, true,  5, 2, {10, 512, 157952}, {240, 256, 0}, 1, 1, 0},
        // helper() on [3, 10, 5, 7] codes (test_parity_gpu): dense upstreams, one pair set, every row light
        {BwdShape{3, 10, 5, 7, 7, 0, true, F32}, true, 0, 126976, R, false, 1, 0, {3, 256, 88064}, {10, 192, 0}, 2, 5, 0},
    };
    for (const Expect& e : table) {
        const BwdPlan p = bwd_plan(e.s, e.dense, e.debug);
        const bool ok = desc_ok(e.s) && bwd_check(e.s) == STEGO_OK && bwd_workspace(e.s).total == e.ws_total && p.path == e.path && p.split == e.split &&
            p.dense == e.dense && p.nt == e.nt && p.n_build == e.n_build && p.tile.grid == e.tile.grid && p.tile.block == e.tile.block &&
            p.tile.lds == e.tile.lds && p.uns.grid == e.uns.grid && p.uns.block == e.uns.block && p.uns.lds == e.uns.lds &&
            (e.path == L ? p.nq == e.a && p.tail == e.b : e.path == R ? p.mt == e.a && p.ur_nt == e.b && p.n_heavy == e.c
                                                                       : p.rt == e.a && p.n_bands == e.b && p.acc_bytes == e.c);
        if (!ok) std::printf("plan of row %d (B %d H %d W %d K %d debug %d): ws %zu path %d split %d nt %d n_build %d tile %u %u %d uns %u %u %d | %d %d | %d %d %d | %d %d %d\n",
                             (int)(&e - table), e.s.B, e.s.H, e.s.W, e.s.K, e.debug, bwd_workspace(e.s).total, (int)p.path, p.split, p.nt, p.n_build, p.tile.grid, p.tile.block,
                             p.tile.lds, p.uns.grid, p.uns.block, p.uns.lds, p.nq, p.tail, p.mt, p.ur_nt, p.n_heavy, p.rt, p.n_bands, p.acc_bytes);
        CHECK(ok);
    }
    // cfg-2's workspace, part by part
    const BwdWorkspace w = bwd_workspace(fwd(32, 28, 28, 70, 11, 5, F16));
    CHECK(w.dt_bytes == 17432576 && w.stamp_bytes == 65536 && w.slots_bytes == 2293760 && w.pool_bytes == 3221504 && w.lists);
    CHECK(w.stamps_off == 17432576 && w.slots_off == 17498112 && w.pool_off == 19791872);
}

static void boundaries()
{
    auto plan = [](int B, int H, int W, int K, int prec, int debug = 0, bool dense = false, int n_neg = 2) { return bwd_plan(fwd(B, H, W, K, 5, n_neg, prec), dense, debug); };
    // the list kernel's channel variant: <1, 0> to K = 64, <1, 1> to 80, <2, 0> beyond
    for (int K : {1, 64}) { const BwdPlan p = plan(4, 16, 16, K, F16); CHECK(p.path == L && p.nq == 1 && p.tail == 0); }
    for (int K : {65, 80}) { const BwdPlan p = plan(4, 16, 16, K, F16); CHECK(p.path == L && p.nq == 1 && p.tail == 1); }
    for (int K : {81, 128}) { const BwdPlan p = plan(4, 16, 16, K, F16); CHECK(p.path == L && p.nq == 2 && p.tail == 0); }
    // channel tiles 5 -> 6 at K 80 -> 81; F32 takes the split kernel beyond 80; the row kernel's UR_NT follows
    for (int prec : {F32, F16}) {
        const BwdPlan a = plan(4, 16, 16, 80, prec), b = plan(4, 16, 16, 81, prec), c = plan(4, 16, 16, 128, prec);
        CHECK(a.nt == 5 && a.split == (prec == F16) && a.tile.block == (prec == F16 ? 512u : 256u) && a.tile.lds == (prec == F16 ? 157952 : 153600));
        CHECK(b.nt == 6 && b.split && b.tile.block == 512 && b.tile.lds == 123136);
        CHECK(c.nt == 8 && c.split && c.tile.lds == 140544 && c.path == L);
        const BwdPlan ar = plan(4, 16, 16, 80, prec, 1024), br = plan(4, 16, 16, 81, prec, 1024), cr = plan(4, 16, 16, 128, prec, 1024);
        CHECK(ar.path == R && ar.ur_nt == 5 && br.path == R && br.ur_nt == 8 && cr.path == R && cr.ur_nt == 8 && cr.nt == 8);
    }
    // the row kernel's pixel tiles: MT = 2 to W = 32, 4 to 64
    CHECK(plan(4, 16, 32, 16, F16, 1024).mt == 2 && plan(4, 16, 33, 16, F16, 1024).mt == 4 && plan(4, 16, 64, 16, F16, 1024).mt == 4);
    // lists -> row past 64 rows, lists -> band past 64 columns; the workspace loses its slots with the lists
    {
        const BwdShape a = fwd(4, 64, 64, 16, 5, 2, F16), b = fwd(4, 65, 64, 16, 5, 2, F16), c = fwd(4, 64, 65, 16, 5, 2, F16);
        CHECK(bwd_plan(a, false, 0).path == L && bwd_workspace(a).lists && bwd_workspace(a).slots_bytes == 4 * 64 * 4 * (size_t)(UL_SLOT0 + UL_SLOT1));
        CHECK(bwd_plan(b, false, 0).path == R && !bwd_workspace(b).lists && bwd_workspace(b).slots_bytes == 0 && bwd_workspace(b).pool_bytes == 0);
        CHECK(bwd_plan(c, false, 0).path == D && !bwd_workspace(c).lists && bwd_workspace(c).total == bwd_workspace(c).dt_bytes + BWD_STAMP_BYTES);
    }
    // builders: one per image up to 32
    CHECK(plan(31, 8, 8, 16, F16).n_build == 31 && plan(32, 8, 8, 16, F16).n_build == 32 && plan(33, 8, 8, 16, F16).n_build == 32);
    CHECK(plan(33, 8, 8, 16, F16).tile.grid == 32 + 4 * 33);
    // a dense upstream: no lists, the DENSE tile kernel
    for (int prec : {F32, F16}) {
        const BwdPlan p = plan(4, 16, 16, 70, prec, 0, true);
        CHECK(p.path == R && p.dense && p.n_build == 0 && p.split == (prec == F16) && p.tile.grid == 16 && p.n_heavy == 64);
    }
    // helper(): never lists (no slots either), the fp32 tile kernel in either precision, no heavy rows
    for (int prec : {F32, F16}) {
        const BwdShape h{3, 72, 8, 16, 16, 0, true, prec};
        const BwdPlan p = bwd_plan(h, true, 0);
        CHECK(desc_ok(h) && p.path == R && !p.split && p.n_heavy == 0 && p.tile.grid == 3 && p.uns.grid == 16 && !bwd_workspace(h).lists && bwd_workspace(h).slots_bytes == 0);
    }
    // debug bits: 32 the band kernel, 512 the fp32 tiles (lists stay), 1024 tile + row; 512 beyond K = 80 has no kernel
    CHECK(plan(4, 16, 16, 70, F16, 32).path == D && plan(4, 16, 16, 70, F16, 32 | 1024).path == D);
    { const BwdPlan p = plan(4, 16, 16, 70, F16, 512); CHECK(p.path == L && !p.split && p.tile.block == 256 && p.tile.lds == 145408 && p.n_build == 4); }
    { const BwdPlan p = plan(4, 16, 16, 70, F16, 1024); CHECK(p.path == R && p.split && p.n_build == 0); }
    CHECK(plan(4, 16, 16, 81, F16, 512).path == X && plan(4, 16, 16, 81, F32, 512).path == X && plan(4, 16, 16, 81, F16, 512 | 1024).path == X);
    CHECK(plan(4, 16, 16, 80, F16, 512 | 1024).path == R);
    for (int bit : {1, 2, 4, 8, 16, 64, 128, 2048}) { const BwdPlan p = plan(4, 16, 16, 70, F16, bit); CHECK(p.path == L && p.split && p.tile.grid == 20); }      // kernel-side bits
    // the size guards: DT rows below 2^30 floats for the lists (32-bit byte offsets), below 2^31 for the row kernel (32-bit float offsets)
    CHECK(plan(15887, 8, 8, 128, F16, 0, false, 0).path == L && plan(15888, 8, 8, 128, F16, 0, false, 0).path == R);
    CHECK(plan(31775, 8, 8, 128, F16, 0, false, 0).path == R && plan(31776, 8, 8, 128, F16, 0, false, 0).path == D);
    CHECK(bwd_workspace(fwd(15887, 8, 8, 128, 5, 0, F16)).lists && !bwd_workspace(fwd(15888, 8, 8, 128, 5, 0, F16)).lists && bwd_workspace(fwd(15888, 8, 8, 128, 5, 0, F16)).slots_bytes > 0);
    // the two limits, last accepted and first refused: one pixel row in the LDS band; the contribution table
    CHECK(bwd_check(fwd(2, 8, 192, 128, 5, 2, F16)) == STEGO_OK && bwd_check(fwd(2, 8, 193, 128, 5, 2, F16)) == STEGO_ERR_UNSUPPORTED);
    CHECK(bwd_check(fwd(2, 8, 24576, 1, 5, 2, F16)) == STEGO_OK && bwd_check(fwd(2, 8, 24577, 1, 5, 2, F16)) == STEGO_ERR_UNSUPPORTED);
    CHECK(bwd_check(fwd(203, 8, 8, 16, 5, 5, F16)) == STEGO_OK && bwd_check(fwd(204, 8, 8, 16, 5, 5, F16)) == STEGO_ERR_UNSUPPORTED);
    CHECK(bwd_check(fwd(4, 8, 8, 16, 5, 204, F16)) == STEGO_OK && bwd_check(fwd(4, 8, 8, 16, 5, 205, F16)) == STEGO_ERR_UNSUPPORTED);
    CHECK(bwd_check(BwdShape{4096, 72, 8, 16, 16, 0, true, F32}) == STEGO_OK);      // helper(): no contribution table to fill
}

static void invariants()
{
    long accepted = 0, plans = 0;
    int Bs[42];
    for (int i = 0; i < 40; ++i) Bs[i] = i + 1;
    Bs[40] = 64; Bs[41] = 204;
    const size_t rsrc_max = (size_t)1 << 32;
    for (int B : Bs) for (int H : {1, 8, 16, 17, 28, 40, 64}) for (int W : {1, 8, 16, 17, 28, 40, 64}) for (int K : {1, 8, 64, 70, 80, 100, 128})
    for (int S : {1, 5, 11}) for (int n_neg : {0, 2, 5}) {
        const BwdShape s0 = fwd(B, H, W, K, S, n_neg, F16);
        if (!desc_ok(s0) || bwd_check(s0) != STEGO_OK) continue;
        ++accepted;
        const BwdWorkspace w = bwd_workspace(s0);
        // what the kernels call host-checked
        CHECK(s0.contributions() <= (size_t)UNS_MAX_CONTRIB);                          // contribution table of the band kernel
        CHECK(s0.contributions() + 1 <= (size_t)BF_ITEM_CAP);                          // builders' item table: dest 0's items + dest 1's one
        CHECK(w.total == w.dt_bytes + w.stamp_bytes + w.slots_bytes + w.pool_bytes);
        CHECK(w.stamps_off == w.dt_bytes && w.slots_off == w.stamps_off + w.stamp_bytes && w.pool_off == w.slots_off + w.slots_bytes);
        CHECK(w.dt_bytes % 256 == 0 && w.stamps_off % 256 == 0 && w.slots_off % 256 == 0 && w.pool_off % 256 == 0 && w.total % 256 == 0);
        CHECK(w.dt_bytes >= s0.dt_elems() * 4);
        CHECK(w.lists);                                                                // every map of this sweep is the lists'
        if (w.lists) {
            const size_t items = s0.n_tiles() + (size_t)n_neg * B + B;                 // (tile, side) matrices that land in some image
            CHECK(w.pool_bytes >= 4 * (size_t)s0.P() * items * 16);                    // 4 entries per (item, point) in the worst case
            CHECK(w.slots_bytes >= (size_t)B * H * s0.bins() * (UL_SLOT0 + UL_SLOT1));
            CHECK(w.dt_bytes < rsrc_max && w.slots_bytes < rsrc_max && w.pool_bytes < rsrc_max);       // buffer resources
            CHECK((size_t)2 * H * BF_MAXMT <= (size_t)BF_NKEY && s0.bins() <= BF_MAXMT);               // list keys of an image
        }
        for (int prec : {F32, F16}) for (int dense = 0; dense < 2; ++dense) for (int debug : {0, 32, 512, 1024}) {
            const BwdShape s = fwd(B, H, W, K, S, n_neg, prec);
            const BwdPlan p = bwd_plan(s, dense != 0, debug);
            ++plans;
            if (p.path == X) { CHECK((debug & 512) && p.nt > 5); continue; }
            CHECK(p.nt >= 1 && p.nt <= BWD_NT_MAX && 16 * p.nt >= K && (p.split || p.nt <= BWD_NT_F32_MAX));
            CHECK(p.tile.grid > 0 && p.uns.grid > 0 && p.tile.block == (p.split ? 512u : 256u));
            CHECK(p.tile.lds > 0 && p.tile.lds <= LDS_MAX_BYTES && p.uns.lds >= 0 && p.uns.lds <= LDS_MAX_BYTES);
            CHECK(p.tile.grid == (unsigned)p.n_build + s.n_tiles());
            if (p.path == L) {
                CHECK(w.lists && !dense && !(debug & (32 | 1024)) && p.tile.lds >= BF_LDS_BYTES && p.n_build >= 1 && p.n_build <= B && p.n_build <= BF_MAX_BUILDERS);
                CHECK(K <= 64 * p.nq + 16 * p.tail && p.uns.block == 64u * UL_WAVES && p.uns.lds == 0);
                CHECK((size_t)(p.uns.grid / 8) * UL_WAVES >= (size_t)((B + 7) / 8) * H * s.bins());   // a wave per unit pair on the image's XCD
            } else if (p.path == R) {
                CHECK(p.n_build == 0 && W <= BIN_W * p.mt && K <= 16 * p.ur_nt && s.dt_elems() < ((size_t)1 << 31) && p.uns.block == 64u * UR_WAVES);
                CHECK((size_t)p.n_heavy + ((size_t)p.uns.grid - p.n_heavy) * UR_WAVES >= (size_t)2 * B * H && p.n_heavy == B * H);
            } else {
                CHECK(p.n_build == 0 && p.rt >= 1 && p.rt <= UNS_MAX_RT && p.rt * p.n_bands >= H && p.uns.grid == 2u * B * p.n_bands);
                CHECK((size_t)p.rt * W * K * 4 + UNS_DUMMY_BYTES <= (size_t)p.acc_bytes && (size_t)p.rt * W * K * 4 <= (size_t)UNS_BAND_BYTES);
            }
        }
    }
    CHECK(accepted > 100000 && plans == accepted * 16);
    std::printf("accepted %ld descriptors, %ld plans\n", accepted, plans);
}

int main()
{
    expected_plans();
    boundaries();
    invariants();
    if (!failures) std::printf("bwd plan ok\n");
    return failures ? 1 : 0;
}
"""


@pytest.mark.skipif(GXX is None, reason="needs g++")
def test_backward_plan_workspace_and_limits(tmp_path):
    src = tmp_path / "bwd_plan_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "bwd_plan_main"
    cmd = [GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "stego_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "bwd plan ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
