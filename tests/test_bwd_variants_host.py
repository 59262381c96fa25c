"""tests/bwd_variant_cases.py against csrc/corr_bwd_plan.h, on the CPU: a stand-alone g++ program (AddressSanitizer +
UndefinedBehaviorSanitizer on, an ordinary executable, in the manner of tests/test_bwd_plan_host.py) generated from the table checks that
every row is accepted (the refusal rows refused) and that the kernel pair a row names is the one bwd_plan() yields for its (shape, dense,
debug); the set of kernels the table reaches must then equal the set of __global__ functions corr_bwd.hip and corr_bwd_lists.hip emit, so a
future variant without a GPU case fails here.  The last test asserts the table's condition on its inputs: no cd element of a default-cfg row
within CLAMP_MARGIN of a clamp bound in the fp64 oracle."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bwd_variant_cases as T
from oracle import corr_oracle as O
from stego_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")

# short name in the table -> the __global__ function template
FUNCTIONS = {"tile_build": "corr_bwd_tile_build_kernel", "tile32_build": "corr_bwd_tile32_build_kernel", "tile_h": "corr_bwd_tile_h_kernel",
             "tile_kernel": "corr_bwd_tile_kernel", "list": "corr_unsample_list_kernel", "row": "corr_unsample_row_kernel",
             "unsample_kernel": "corr_unsample_kernel"}

PROGRAM = r"""
#include <cstdio>
#include <string>

#include "corr_bwd_plan.h"

using namespace stego;

static int failures = 0;

// what check_desc (c_api.hip) and plan_fwd accept of the fields the backward reads, one-tile path (S * S <= 128)
static bool desc_ok(const BwdShape& s, int C)
{
    if (s.B <= 0 || C <= 0 || s.K <= 0 || s.H <= 0 || s.W <= 0 || s.H > 32767 || s.W > 32767) return false;
    if (s.helper) return s.K <= 72 && s.H * s.W <= TP;
    if (s.K > 72 && !(C == 192 || C == 384 || C == 768)) return false;       // 72 < K <= 128: the fused forward's maps only
    return s.K <= 128 && s.S > 0 && s.S <= 16 && s.n_neg >= 0 && s.n_neg + 2 <= 256 && s.S * s.S <= TP;
}

// plan -> kernel names, written once; mirrors launch_corr_bwd_lists() and launch_corr_bwd()
static std::string tile_name(const BwdPlan& p)
{
    const std::string nt = std::to_string(p.nt);
    if (p.path == BwdPath::Lists) return (p.split ? "tile_build<" : "tile32_build<") + nt + ">";
    return p.split ? "tile_h<" + nt + (p.dense ? ",true>" : ",false>") : "tile_kernel<" + nt + ">";
}

static std::string uns_name(const BwdPlan& p)
{
    if (p.path == BwdPath::Lists) return "list<" + std::to_string(p.nq) + "," + std::to_string(p.tail) + ">";
    if (p.path == BwdPath::TileBand) return "unsample_kernel";
    return "row<" + std::to_string(p.mt) + "," + std::to_string(p.ur_nt) + ">";
}

struct Row { const char* name; BwdShape s; int C; bool dense; int debug; const char* tile; const char* uns; };
struct Ref { const char* name; BwdShape s; int C; int debug; bool by_check; };

static const Row rows[] = {
@ROWS@
};
static const Ref refusals[] = {
@REFUSALS@
};

int main()
{
    for (const Row& r : rows) {
        const BwdPlan p = bwd_plan(r.s, r.dense, r.debug);
        const bool ok = desc_ok(r.s, r.C) && bwd_check(r.s) == STEGO_OK && p.path != BwdPath::Invalid && tile_name(p) == r.tile && uns_name(p) == r.uns;
        if (!ok) {
            std::printf("FAILED %s: desc_ok %d bwd_check %d path %d plan (%s, %s) table (%s, %s)\n", r.name, (int)desc_ok(r.s, r.C), bwd_check(r.s), (int)p.path,
                        tile_name(p).c_str(), uns_name(p).c_str(), r.tile, r.uns);
            ++failures;
            continue;
        }
        std::printf("REACHED %s\nREACHED %s\n", tile_name(p).c_str(), uns_name(p).c_str());
        // what the band kernel's branches need of the shape is visible in the plan
        if (p.path == BwdPath::TileBand) std::printf("BAND %s rt %d n_bands %d H %d row_bytes %d\n", r.name, p.rt, p.n_bands, r.s.H, r.s.W * r.s.K * 4);
    }
    for (const Ref& r : refusals) {
        const BwdPlan p = bwd_plan(r.s, false, r.debug);
        // check_desc accepts all of them: the refusal is the backward's own
        const bool ok = desc_ok(r.s, r.C) && (r.by_check ? bwd_check(r.s) == STEGO_ERR_UNSUPPORTED : bwd_check(r.s) == STEGO_OK && p.path == BwdPath::Invalid);
        if (!ok) { std::printf("FAILED %s: desc_ok %d bwd_check %d path %d\n", r.name, (int)desc_ok(r.s, r.C), bwd_check(r.s), (int)p.path); ++failures; }
    }
    std::printf("LIMITS %d %d\n", UNS_BAND_BYTES, UNS_MAX_CONTRIB);
    if (!failures) std::printf("bwd variants ok\n");
    return failures ? 1 : 0;
}
"""


def _shape_literal(shape, mode, precision):
    B, C, H, W, K, S, n_neg = shape
    return "BwdShape{%d, %d, %d, %d, %d, %d, %s, %s}" % (B, K, H, W, S, n_neg, "true" if mode == "helper" else "false",
                                                         "PREC_F32" if precision == "f32" else "PREC_F16X3")


def _run_program(tmp_path):
    rows = ",\n".join('    {"%s", %s, %d, %s, %d, "%s", "%s"}' % (c.name, _shape_literal(c.shape, c.mode, c.precision), c.shape[1],
                                                                  "true" if c.dense else "false", c.debug, c.kernels[0], c.kernels[1])
                      for c in T.CASES)
    refs = ",\n".join('    {"%s", %s, %d, %d, %s}' % (r.name, _shape_literal(r.shape, "forward", r.precision), r.shape[1], r.debug,
                                                      "true" if r.why == "bwd_check" else "false") for r in T.REFUSALS)
    src = tmp_path / "bwd_variants_main.cpp"
    src.write_text(PROGRAM.replace("@ROWS@", rows).replace("@REFUSALS@", refs))
    exe = tmp_path / "bwd_variants_main"
    cmd = [GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "stego_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "bwd variants ok" in run.stdout, (run.stdout + run.stderr)[-3000:]
    return run.stdout


def test_the_table_is_well_formed():
    names = [c.name for c in T.CASES] + [r.name for r in T.REFUSALS]
    assert len(set(names)) == len(names)
    for c in T.CASES:
        B, C, H, W, K, S, n_neg = c.shape
        assert c.precision in ("f32", "f16x3") and c.mode in ("forward", "helper") and c.cfg in ("default", "noclamp") and c.recipe in T.RECIPES, c
        assert c.debug & ~T.ALLOWED_DEBUG_BITS == 0, c                # the ablation bits change results
        assert K <= 72 or C == 192, c                                # K > 72: the fused layout
        assert c.kernels[0].split("<")[0] in FUNCTIONS and c.kernels[1].split("<")[0] in FUNCTIONS, c
        assert c.mode == "forward" or (c.dense and c.recipe == "random" and n_neg == 0), c
    for c in T.CASES:                                                # an F32 twin is the same inputs on the same path
        t = T.twin(c)
        assert t is None or (t.shape, t.seed, t.recipe, t.dense, t.debug, t.cfg) == (c.shape, c.seed, c.recipe, c.dense, c.debug, c.cfg)
    assert sum(T.twin(c) is not None for c in T.CASES) >= 20
    assert any(c.name == T.AFTER_REFUSAL for c in T.CASES)


@pytest.mark.skipif(GXX is None or not _build.have_hipcc(), reason="needs g++ and hipcc")
def test_every_row_names_the_plan_s_kernels_and_the_table_reaches_every_emitted_kernel(tmp_path):
    out = _run_program(tmp_path)
    reached = {line.split(" ", 1)[1] for line in out.splitlines() if line.startswith("REACHED ")}
    # the band rows are at the shapes their branches need: rt = 2 with a partial last band; rt = 1 at the last accepted row size
    bands = {m.group(1): tuple(int(x) for x in m.groups()[1:]) for m in
             re.finditer(r"BAND (\S+) rt (\d+) n_bands (\d+) H (\d+) row_bytes (\d+)", out)}
    assert bands["band-f16x3-W66-K128"][:3] == (2, 3, 5) and bands["band-f16x3-W192-K128"] == (1, 3, 3, 98304), bands

    # the two units, compiled exactly as test_backward_kernels_do_not_spill compiles them
    by_function = {v: k for k, v in FUNCTIONS.items()}
    emitted = set()
    for unit in _build.kernel_resources_each(["corr_bwd.hip", "corr_bwd_lists.hip"]):
        for mangled in unit:
            m = re.match(r"_ZN5stego(\d+)", mangled)
            assert m, mangled
            fn = mangled[m.end():m.end() + int(m.group(1))]
            rest = mangled[m.end() + int(m.group(1)):]
            args = []
            if rest.startswith("I"):                                 # template arguments: Li<int>E / Lb<0|1>E ... E
                rest = rest[1:]
                while not rest.startswith("E"):
                    a = re.match(r"L([ib])(\d+)E", rest)
                    assert a, mangled
                    args.append(a.group(2) if a.group(1) == "i" else ("true" if a.group(2) == "1" else "false"))
                    rest = rest[a.end():]
            assert fn in by_function, "a backward kernel the case table has no name for: " + mangled
            emitted.add(by_function[fn] + ("<" + ",".join(args) + ">" if args else ""))
    # ContrastiveCorrelationLoss.fused_kernels_cover restates the two limits of bwd_check: the same numbers, the same boundaries
    from stego_amd import modules as M
    assert re.search(r"LIMITS (\d+) (\d+)", out).groups() == (str(M._BWD_BAND_BYTES), str(M._BWD_MAX_CONTRIB))
    cover = M.ContrastiveCorrelationLoss.fused_kernels_cover
    assert cover(203, 32, 16, 8, 8, 5, n_neg=5) and not cover(204, 32, 16, 8, 8, 5, n_neg=5) and cover(204, 32, 16, 8, 8, 5, n_neg=4)
    assert cover(2, 192, 128, 4, 192, 5, n_neg=1) and not cover(2, 192, 128, 4, 193, 5, n_neg=1) and cover(2, 192, 127, 4, 193, 5, n_neg=1)
    assert cover(250, 32, 16, 8, 8, 12, n_neg=5)                  # S * S > 128: corr_wide.hip's own backward, without these limits
    assert len(emitted) == 42, sorted(emitted)
    assert reached == emitted, ("kernels without a GPU case: %s; names no unit emits: %s" % (sorted(emitted - reached), sorted(reached - emitted)))


def _cd_margin(case):
    d = T.make_inputs(case)
    if case.mode == "helper":
        _, cd, _ = O.helper(*(d[k].astype(np.float64) for k in ("f1", "f2", "c1", "c2")), 0.31, O.CorrCfg())
        return float(np.abs(cd).min())
    S, n_neg = case.shape[5:]
    out = O.corr_loss_forward(d["feats"], d["feats_pos"], d["code"], d["code_pos"], d["coords1"], d["coords2"], d["perms"],
                              O.CorrCfg(feature_samples=S, neg_samples=n_neg))
    return min(float(np.abs(x).min()) for x in (out.pos_intra_cd, out.pos_inter_cd, out.neg_inter_cd) if x.size)


def test_no_default_cfg_row_has_a_cd_element_near_a_clamp_bound():
    """The default cfg clamps cd at 0 from below (no upper bound): the distance of every cd element of the fp64 oracle to 0.  A condition on
    the table's inputs, not a measurement of the kernels."""
    seen = {}
    for c in T.CASES + T.SURFACE:
        if c.cfg != "default":
            continue
        key = (c.shape, c.seed, c.recipe, c.mode)
        if key not in seen:
            seen[key] = _cd_margin(c)
        assert seen[key] >= T.CLAMP_MARGIN, (c.name, seen[key])
    assert len(seen) >= 20
