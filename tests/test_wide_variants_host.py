"""tests/wide_variant_cases.py against csrc/corr_wide_plan.h, on the CPU: a stand-alone g++ program (AddressSanitizer +
UndefinedBehaviorSanitizer on, an ordinary executable, in the manner of tests/test_bwd_variants_host.py) generated from the table checks that
every row is a shape the wide path takes and that the variants a row names are the ones wide_plan() yields for its shape and layouts; the set
of variants the table reaches must then equal the set the launchers can emit - twelve sampler instantiations, three fd kernels, both window
counts, gather and scatter - so a variant added later without a row fails here, and so does the table with any one row deleted.  The other
tests assert the table's conditions on its inputs in the fp64 oracle: no cd element of a clamped row within CLAMP_MARGIN of a clamp bound
(the exact zeros of the zero-vector rows excepted), and every point's taps the same pixels in float32 and float64."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import wide_variant_cases as T
from stego_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")

# every row and stage case by name: a row that leaves the table, or joins it, does so here too - on purpose
ROWS = """
    vw42-C384-K70 vw42-C384-K70-dense vw44-C64-K24-S16 vw40-C384-K101 vw24-C70-K24 vw22-C134-K70 vw20-C70-K1 vw04-C192nchw-K88 vw02-C65-K70
    vw00-C128nchw-K89nchw vw0-C770-K8 vw0-C1028-K127 align1-C384of388-K70 align2-C384of388-K70 fd-C128-K8 fd-C392-K8 fd-C64-K8-nopointwise
    fd-C128-K8-nopointwise fd-C134-K8-nopointwise fd-C384-K8-nopointwise fd-C392-K8-nopointwise fd-C770-K8-nopointwise win-K8-stab win-K97-S16-dense
    win-K128 win-K128-B1 edge-nneg0 edge-nneg0-dense edge-B1 edge-image0 edge-H1 edge-W1 edge-1x1 edge-coords edge-coords-dense edge-zeros edge-zeros-dense
    edge-S13 scatter-65x64 scatter-65x64-dense
""".split()
STAGE_CASES = """
    one4-C64 one4-C128 one4-C384 one4-C392 one4-C1024 one2-C70 one2-C134 one2-C510 one2-slice2 one0-C65 one0-C770 one0-C1028 one0-nchw one0-slice1
""".split()

PROGRAM = r"""
#include <cstdio>
#include <set>
#include <string>

#include "corr_wide_plan.h"

using namespace stego;

static int failures = 0;
static const uintptr_t BASE = 0x7f0000000000ull;        // what an allocator hands out: 256-byte aligned

struct Row {
    const char* name;
    int B, C, H, W, K, S, n_neg;
    MapFacts f, c;                                       // both feature maps / both code maps (addr: bytes past BASE)
    bool pointwise;
    const char *pair, *fd, *win, *bwd;
};
struct Panel { const char* name; int C, H, W, S; MapFacts m; int vw; const char* gemm; };

static const Row rows[] = {
@ROWS@
};
static const Panel panels[] = {
@PANELS@
};

static MapFacts at_base(MapFacts m) { m.addr += BASE; return m; }

static std::string pair_name(int v1, int v2) { return "panels<" + std::to_string(v1) + "," + std::to_string(v2) + ">"; }
static std::string one_name(int v) { return "panels<" + std::to_string(v) + ">"; }
static std::string gemm_name(PanelGemm k)
{
    return k == PanelGemm::RowPair ? "rowpair" : k == PanelGemm::RowBlock ? "rowblock" : k == PanelGemm::Tile ? "tile" : "other";
}

int main()
{
    std::set<std::string> reached;
    for (const Row& r : rows) {
        const WideLayout l{at_base(r.f), at_base(r.f), at_base(r.c), at_base(r.c), BASE};
        const WidePlan p = wide_plan(r.B, r.C, r.K, r.H, r.W, r.S, r.n_neg, r.pointwise, l, 0, 0);
        bool ok = wide_supported_shape(r.B, r.C, r.K, r.S, r.n_neg) && r.H >= 1 && r.W >= 1 && r.H <= 32767 && r.W <= 32767;
        // the three sources sample maps of one layout: one pair per row
        for (int s = 0; s < p.n_sample; ++s) ok = ok && pair_name(p.vw[s][0], p.vw[s][1]) == r.pair;
        const std::string fd = "fd:" + gemm_name(p.fd.kernel), win = "win:" + std::to_string(p.win.nwin), bwd = p.gather ? "bwd:gather" : "bwd:scatter";
        ok = ok && fd == r.fd && win == r.win && bwd == r.bwd;
        // the code correlation of a wide shape is the row pair's whatever the row; its outputs are segmented
        ok = ok && p.cd.kernel == PanelGemm::RowPair && !p.cd.rowsum_launch;
        // row sums ride in the row kernels; the tile kernel takes a launch for them when the pointwise shift wants them
        ok = ok && p.fd.rowsum_launch == (p.fd.kernel == PanelGemm::Tile && r.pointwise);
        ok = ok && p.fwd_launches == p.n_sample + 5 + (p.fd.rowsum_launch ? 1 : 0);
        ok = ok && p.bwd_launches == 2 * p.win.nwin + (p.gather ? 2 : r.n_neg > 0 ? 3 : 2);
        // the windows cover [0, K) in order, each a multiple of 8 channels but the last, none wider than the kernel holds
        int covered = 0;
        for (int w = 0; w < p.win.nwin; ++w) {
            ok = ok && p.win.k0(w) == covered && p.win.kc(w, r.K) >= 1 && p.win.kc(w, r.K) <= WB_WIN && (w + 1 == p.win.nwin || p.win.kc(w, r.K) % 8 == 0);
            covered += p.win.kc(w, r.K);
        }
        ok = ok && covered == r.K;
        if (!ok) {
            std::printf("FAILED %s: plan (%s, %s, %s, %s) table (%s, %s, %s, %s) launches %d + %d\n", r.name, pair_name(p.vw[0][0], p.vw[0][1]).c_str(),
                        fd.c_str(), win.c_str(), bwd.c_str(), r.pair, r.fd, r.win, r.bwd, p.fwd_launches, p.bwd_launches);
            ++failures;
            continue;
        }
        std::printf("ROW %s kc", r.name);
        for (int w = 0; w < p.win.nwin; ++w) std::printf(" %d", p.win.kc(w, r.K));
        std::printf(" launches %d %d\n", p.fwd_launches, p.bwd_launches);
        for (const std::string& v : {std::string(r.pair), fd, win, bwd}) reached.insert(v);
    }
    for (const Panel& q : panels) {
        const int vw = panel_vw(at_base(q.m), q.C, 0);
        const PanelGemmPlan g = panel_gemm_plan(q.C, q.S * q.S, q.S * q.S, false, true, 0);
        if (vw != q.vw || gemm_name(g.kernel) != q.gemm) {
            std::printf("FAILED %s: plan (%d, %s) table (%d, %s)\n", q.name, vw, gemm_name(g.kernel).c_str(), q.vw, q.gemm);
            ++failures;
            continue;
        }
        reached.insert(one_name(vw));
        std::printf("PANEL %s %s\n", q.name, q.gemm);
    }
    // what the launchers can emit: with_const<4, 2, 0> x with_const<-1, 4, 2, 0> of launch_sample_panels2, the three kernels of
    // launch_dense_corr_panels_seg without a debug bit, wide_windows over K = 1 .. WIDE_MAX_K, both answers of wide_gather
    std::set<std::string> emitted;
    for (int v1 : {4, 2, 0}) {
        emitted.insert(one_name(v1));
        for (int v2 : {4, 2, 0}) emitted.insert(pair_name(v1, v2));
    }
    for (int C = 1; C <= 2048; ++C)
        for (int P : {129, 256}) emitted.insert("fd:" + gemm_name(panel_gemm_plan(C, P, P, false, true, 0).kernel));
    for (int K = 1; K <= WIDE_MAX_K; ++K) emitted.insert("win:" + std::to_string(wide_windows(K).nwin));
    emitted.insert(wide_gather(2, 64, 64, 1, 0) ? "bwd:gather" : "?");
    emitted.insert(wide_gather(2, 65, 64, 1, 0) ? "?" : "bwd:scatter");
    // every width rule has both answers among the maps a caller can hand over: the rule cannot emit a width outside {4, 2, 0}
    for (const std::string& v : emitted)
        if (!reached.count(v)) { std::printf("NOT REACHED %s\n", v.c_str()); ++failures; }
    for (const std::string& v : reached)
        if (!emitted.count(v)) { std::printf("NOT EMITTED %s\n", v.c_str()); ++failures; }
    for (const std::string& v : reached) std::printf("REACHED %s\n", v.c_str());
    std::printf("VARIANTS %d\n", (int)emitted.size());
    // the limits the table's shapes sit on
    if (wide_windows(88).nwin != 1 || wide_windows(89).nwin != 2 || wide_windows(97).Kc != 56 || wide_windows(97).kc(1, 97) != 41 ||
        wide_windows(128).Kc != 64 || !wide_gather(3, 64, 64, 5, 0) || wide_gather(3, 1, 4097, 5, 0) || wide_gather(3, 8, 8, 5, WIDE_DBG_SCATTER)) {
        std::printf("FAILED limits\n");
        ++failures;
    }
    if (!failures) std::printf("wide variants ok\n");
    return failures ? 1 : 0;
}
"""


def _facts_literal(layout, C, H, W):
    sn, sc, sh, sw, off = T.facts(layout, C, H, W)
    return "MapFacts{%d, %d, %d, %d, %d}" % (sn, sc, sh, sw, off)


def _program(cases, panels):
    rows = ",\n".join('    {"%s", %s, %s, %s, %s, "%s", "%s", "%s", "%s"}' % (
        c.name, ", ".join(str(v) for v in c.shape), _facts_literal(c.flayout, c.shape[1], c.shape[2], c.shape[3]),
        _facts_literal(c.clayout, c.shape[4], c.shape[2], c.shape[3]), "true" if c.pointwise else "false", *c.variants) for c in cases)
    B, H, W = T.PANEL_MAP
    pans = ",\n".join('    {"%s", %d, %d, %d, %d, %s, %d, "%s"}' % (q.name, q.C, H, W, q.S, _facts_literal(q.layout, q.C, H, W), q.vw, q.gemm) for q in panels)
    return PROGRAM.replace("@ROWS@", rows).replace("@PANELS@", pans)


def _build_and_run(tmp_path, cases, panels, tag="main"):
    src = tmp_path / ("wide_variants_%s.cpp" % tag)
    src.write_text(_program(cases, panels))
    exe = tmp_path / ("wide_variants_%s" % tag)
    cmd = [GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "stego_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_the_table_is_well_formed():
    names = [c.name for c in T.CASES] + [q.name for q in T.PANELS]
    assert len(set(names)) == len(names)
    assert [c.name for c in T.CASES] == ROWS and [q.name for q in T.PANELS] == STAGE_CASES
    for c in T.CASES:
        B, C, H, W, K, S, n_neg = c.shape
        assert c.flayout in T.LAYOUTS and c.clayout in T.LAYOUTS and c.recipe in T.RECIPES and c.cfg in T.CFGS, c
        assert B <= 3 and S in range(12, 17) and C <= 1028 and K <= 128, c
        assert (H <= 12 and W <= 12) or (c.variants[3] == "bwd:scatter" and H * W <= 4096 + 64), c
        assert c.recipe != "zeros" or (H >= 7 and W >= 9), c             # the zero blocks lie inside the map
        assert c.recipe != "image0" or (B >= 2 and n_neg >= 1), c
    shapes = {c.shape for c in T.CASES}
    assert {K for (_, _, _, _, K, _, _) in shapes} >= set(T.K_WINDOWS)
    assert {S for s in shapes for S in [s[5]]} >= {12, 16}
    assert {c.shape[1] for c in T.CASES if not c.pointwise} >= {64, 128, 134, 384, 392, 770}
    assert {c.shape[1] for c in T.CASES if c.pointwise} >= {64, 128, 134, 384, 392, 770, 1028}
    assert any(c.shape[6] == 0 for c in T.CASES) and any(c.shape[0] == 1 for c in T.CASES)
    assert {(c.shape[2] == 1, c.shape[3] == 1) for c in T.CASES} == {(False, False), (True, False), (False, True), (True, True)}
    for recipe in T.RECIPES:
        assert any(c.recipe == recipe and c.dense for c in T.CASES) or recipe == "image0"
        assert any(c.recipe == recipe and not c.dense for c in T.CASES)
    assert any(c.variants[3] == "bwd:scatter" and c.dense for c in T.CASES) and any(c.variants[3] == "bwd:scatter" and not c.dense for c in T.CASES)
    # the clamp mask stays under test: most rows clamp
    assert sum(c.cfg != "noclamp" for c in T.CASES) >= 2 * sum(c.cfg == "noclamp" for c in T.CASES)


@pytest.mark.skipif(GXX is None, reason="needs g++")
def test_every_row_names_the_plan_s_variants_and_the_table_reaches_every_variant(tmp_path):
    run = _build_and_run(tmp_path, T.CASES, T.PANELS)
    assert run.returncode == 0 and "wide variants ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    assert re.search(r"VARIANTS (\d+)", run.stdout).group(1) == str(12 + 3 + 2 + 2)
    rows = dict(m.groups() for m in re.finditer(r"ROW (\S+) kc ([\d ]+?) launches", run.stdout))
    assert rows["win-K97-S16-dense"] == "56 41" and rows["vw00-C128nchw-K89nchw"] == "48 41" and rows["vw04-C192nchw-K88"] == "88"
    launches = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"ROW (\S+) kc [\d ]+ launches (\d+) (\d+)", run.stdout)}
    assert launches["vw42-C384-K70"] == (8, 4)                        # what corr_wide.hip's header counts
    assert launches["vw0-C770-K8"] == (9, 4) and launches["fd-C770-K8-nopointwise"] == (8, 4)
    assert launches["edge-nneg0"] == (7, 4) and launches["scatter-65x64"] == (8, 5) and launches["win-K128"] == (8, 6)
    # the kernel a stage case names is the one the Python surface would get
    assert len(run.stdout.split("PANEL ")) - 1 == len(T.PANELS)


@pytest.mark.skipif(GXX is None or not _build.have_hipcc(), reason="needs g++ and hipcc")
def test_the_table_reaches_every_kernel_the_sampler_and_gemm_units_emit(tmp_path):
    """The instantiations hipcc emits for sample_sets.hip and dense_corr.hip, by their mangled names: every sample_panels_kernel<VW1, VW2>
    and every GEMM on prepared operands has a row or a stage case (the four-stage ring of the row-block kernel is a tool's, behind a debug bit;
    dense_prep_kernel and dense_rowblock_kernel<false> take maps, not prepared operands: tests/test_dense_corr.py)."""
    run = _build_and_run(tmp_path, T.CASES, T.PANELS)
    reached = {line.split(" ", 1)[1] for line in run.stdout.splitlines() if line.startswith("REACHED ")}
    emitted, others = set(), set()
    for unit in _build.kernel_resources_each(["sample_sets.hip", "dense_corr.hip"]):
        for mangled in unit:
            m = re.match(r"_ZN5stego(\d+)", mangled)
            assert m, mangled
            fn = mangled[m.end():m.end() + int(m.group(1))]
            args = [("-" if a[1] == "n" else "") + a[2] if a[0] == "i" else ("true" if a[2] == "1" else "false")
                    for a in re.findall(r"L([ib])(n?)(\d+)E", mangled[m.end() + int(m.group(1)):].split("EE")[0] + "E")]
            if fn == "sample_panels_kernel":
                emitted.add("panels<%s>" % ",".join(a for a in args if a != "-1"))
            elif (fn, args) in (("dense_rowpair_kernel", ["2"]), ("dense_rowblock_kernel", ["true", "2"]), ("dense_tile_kernel", [])):
                emitted.add("fd:" + fn[len("dense_"):-len("_kernel")])
            else:
                others.add(fn + "<" + ",".join(args) + ">")
    assert others == {"sample_gather_kernel<true>", "sample_gather_kernel<false>", "sample_scatter_kernel<>", "dense_prep_kernel<>",
                      "dense_rowblock_kernel<false,3>", "dense_rowblock_kernel<true,4>"}, sorted(others)
    assert len(emitted) == 15 and emitted == {v for v in reached if v.startswith(("panels<", "fd:"))}, (sorted(emitted), sorted(reached))


@pytest.mark.skipif(GXX is None, reason="needs g++")
def test_the_program_notices_a_variant_without_a_row(tmp_path):
    """Deleting the only rows of a variant fails the program (run here for one variant of two kinds).  Any other row that is deleted fails
    test_the_table_is_well_formed: its coverage conditions, or at the least the list of names."""
    only = {}
    for c in T.CASES:
        for v in c.variants:
            only.setdefault(v, []).append(c.name)
    for kind in ("panels<2,0>", "bwd:scatter"):
        gone = set(only[kind])
        run = _build_and_run(tmp_path, [c for c in T.CASES if c.name not in gone], T.PANELS, tag=re.sub(r"\W", "_", kind))
        assert run.returncode == 1 and "NOT REACHED " + kind in run.stdout, run.stdout[-2000:]


def test_no_clamped_row_has_a_cd_element_near_a_clamp_bound():
    """The distance of every cd element of the fp64 oracle to the clamp bounds of the row's cfg.  A condition on the table's inputs, not a
    measurement of the kernels."""
    seen = {}
    for c in T.CASES:
        if c.cfg == "noclamp":
            continue
        key = (c.shape[0],) + c.shape[2:] + (c.recipe, c.cfg, c.seed)      # (the code side does not see C)
        if key not in seen:
            seen[key] = T.cd_margin(c)
        assert seen[key] >= T.CLAMP_MARGIN, (c.name, seen[key])
    assert len(seen) >= 12


def test_every_point_has_the_same_taps_in_float32_and_float64():
    """make_taps (corr_common.h) in float32 and the oracle in float64 floor every unnormalised coordinate to the same pixel: the gradients'
    zero pattern is the oracle's.  The pixel centres of the "edges" recipe are exact in both."""
    f32 = np.float32
    exact = 0
    for c in T.CASES:
        B, C, H, W, K, S, n_neg = c.shape
        d = T.make_codes(c)
        for key in ("coords1", "coords2"):
            for axis, n in ((0, W), (1, H)):
                v = d[key][..., axis]
                i32 = np.minimum(f32(n - 1), np.maximum(((v + f32(1)) * f32(0.5)) * f32(n - 1), f32(0)))
                i64 = np.minimum(n - 1.0, np.maximum((v.astype(np.float64) + 1) / 2 * (n - 1), 0.0))
                assert i32.dtype == np.float32 and np.array_equal(np.floor(i32), np.floor(i64)), (c.name, key, axis)
                assert np.array_equal(i32 == np.floor(i32), i64 == np.floor(i64)), (c.name, key, axis)
                if c.recipe == "edges":
                    exact += int(np.count_nonzero((i64 == np.floor(i64)) & (np.abs(v) <= 1)))
                    assert (np.abs(v) > 1).any() and (np.abs(v) == 1).any(), (c.name, key, axis)
    assert exact > 100
