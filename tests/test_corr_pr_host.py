"""The label co-occurrence PR curves without a GPU: the float64 oracle (tests/corr_pr_oracle.py) against what the unmodified reference
computed (tests/golden/corr_pr_small.npz, tools/make_pr_golden.py), the curve arithmetic against scikit-learn, every host check of
stego_pr_accumulate (include/stego_pr.h), and the kernel's compiled resources."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import corr_pr_oracle as P
from conftest import load_golden
from stego_amd import _build, capi
from stego_amd.correspondence_pr import CorrespondencePR, pr_from_hist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000          # a 256-byte aligned stand-in address: the checks reject before any pointer is read


# ------------------------------------------------------------------ 1. oracle vs the reference
def test_oracle_matches_reference_golden():
    g = load_golden("corr_pr_small")
    n_classes = int(g["meta"][0])
    o = P.net_fd(g["feats1"], g["feats2"], g["label1"].astype(np.int64), g["label2"].astype(np.int64), g["coords1"], g["coords2"], n_classes)
    assert o["fd"].shape == g["fd"].shape == o["target"].shape
    np.testing.assert_allclose(o["fd"], g["fd"], rtol=1e-5, atol=1e-6)        # the bar of tests/test_oracle_golden.py:20
    # the reference's ld is fp32 arithmetic on label pixel coordinates up to 47 (ulp 2^-18 = 3.8e-6): each point's tap weights are off
    # by up to about two of those, a pair's ld by about four -> 2e-5 (a sanity bound on the golden; the separation below is the check)
    np.testing.assert_allclose(o["ld"], g["ld"], rtol=0, atol=2e-5)
    # no impure pair inside the band below 1 in exact arithmetic (the inputs were chosen so) ...
    assert not ((o["ld"] > 1 - 2e-3) & ~o["target"]).any()
    # ... so the reference's fp32 ld separates the pairs exactly as the integer test does
    assert np.array_equal(g["ld"] >= 1 - 1e-3, o["target"])
    assert 50 <= o["target"].sum() < o["target"].size // 2 and o["skip"].any() and not o["skip"].all()
    # the documented difference: the reference's ld.to(int64) turns some of these positives into negatives, never the reverse
    trunc = g["ld"].astype(np.int64)
    assert not (trunc[~o["target"]] != 0).any()
    assert (trunc[o["target"]] == 0).sum() == 3


def test_oracle_exact_target_is_ld_equal_one():
    """On label-aligned points (every weight 0 or 1) the float64 ld is exactly 0 or 1 and equals the integer target."""
    rng = np.random.default_rng(5)
    lab = rng.integers(-1, 3, (2, 9, 9))
    px = rng.integers(0, 9, (2, 6, 1, 2))
    coords = px / 4.0 - 1.0
    f = rng.standard_normal((2, 4, 3, 3))
    o = P.net_fd(f, f, lab, lab, coords, coords, 3)
    assert np.array_equal(o["ld"] == 1.0, o["target"]) and set(np.unique(o["ld"])) <= {0.0, 1.0}
    same = lab[np.arange(2)[:, None], px[:, :, 0, 1], px[:, :, 0, 0]]
    cls = np.where(same >= 0, same + 1, 0)
    assert np.array_equal(o["target"][:, 0, :, 0, :], cls[:, :, None] == cls[:, None, :])


# ------------------------------------------------------------------ 2. the curve arithmetic
def _expand(hist):
    scores = np.repeat(np.arange(hist.shape[0]), hist.sum(1))
    targets = np.concatenate([np.r_[np.zeros(n, dtype=np.int64), np.ones(p, dtype=np.int64)] for n, p in hist])
    return targets, scores


def _filled(hist):
    m = CorrespondencePR(n_classes=3, n_bins=hist.shape[0])
    m.hist = torch.from_numpy(np.ascontiguousarray(hist)).clone()           # hand-filled: compute() only reads it
    return m


@pytest.mark.parametrize("case", ["random", "ties", "single_bin", "sparse"])
def test_compute_equals_scikit_learn(case):
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(11)
    n_bins = 64
    hist = np.zeros((n_bins, 2), dtype=np.int64)
    if case == "random":
        hist[:] = rng.integers(0, 40, (n_bins, 2))
    elif case == "ties":
        hist[[3, 40, 41]] = [[5000, 20], [300, 7000], [1, 1]]
    elif case == "single_bin":
        hist[17] = [30, 12]
    else:
        hist[rng.choice(n_bins, 9, replace=False)] = rng.integers(0, 5, (9, 2))
        hist[63] = [0, 2]
    m = _filled(hist)
    res = m.compute()
    y, s = _expand(hist)
    precision, recall, thr = skm.precision_recall_curve(y, s)
    np.testing.assert_allclose(res["precision"], precision, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["recall"], recall, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["thresholds"], -1.0 + 2.0 * thr / n_bins, rtol=0, atol=1e-12)
    assert abs(res["average_precision"] - skm.average_precision_score(y, s)) <= 1e-12
    assert res["n_pos"] == int(y.sum()) and res["n_total"] == y.size
    # the oracle's loop gives the same curve
    po, ro, bo, ao = P.pr_from_hist(hist)
    np.testing.assert_allclose(po, precision, rtol=0, atol=1e-12)
    np.testing.assert_allclose(ro, recall, rtol=0, atol=1e-12)
    assert np.array_equal(bo, thr) and abs(ao - res["average_precision"]) <= 1e-12


def test_no_positives_gives_nan_without_warning():
    hist = np.zeros((64, 2), dtype=np.int64)
    hist[[2, 9], 0] = [4, 6]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = _filled(hist).compute()
        at = _filled(hist).at(0.1)
        empty = CorrespondencePR(n_classes=3, n_bins=64).compute()
        with np.errstate(all="raise"):
            pr_from_hist(hist)
    assert np.isnan(res["average_precision"]) and np.isnan(res["recall"][:-1]).all() and res["n_pos"] == 0 and res["n_total"] == 10
    assert np.array_equal(res["precision"], [0.0, 0.0, 1.0])
    assert np.isnan(at["recall"]) and np.isnan(at["precision"]) and at["share"] == 0.0
    assert np.isnan(empty["average_precision"]) and empty["n_total"] == 0 and np.isnan(P.pr_from_hist(hist)[3])


def test_at_reports_the_quantised_edge():
    hist = np.zeros((64, 2), dtype=np.int64)
    hist[10] = [6, 2]          # cosines in [-0.6875, -0.65625)
    hist[40] = [1, 3]          # [0.25, 0.28125)
    hist[50] = [0, 4]          # [0.5625, 0.59375)
    m = _filled(hist)
    a = m.at(0.26)             # lowest edge not below 0.26 is 0.28125 (bin 41)
    assert a["edge"] == 0.28125 and a["precision"] == 1.0 and a["recall"] == 4 / 9 and a["share"] == 4 / 16
    a = m.at(0.25)             # an edge itself
    assert a["edge"] == 0.25 and a["precision"] == 7 / 8 and a["recall"] == 7 / 9 and a["share"] == 8 / 16
    assert m.at(-1.0)["share"] == 1.0 and m.at(-1.0)["edge"] == -1.0
    assert m.at(1.0)["edge"] == 1.0 and m.at(1.0)["share"] == 0.0 and np.isnan(m.at(1.0)["precision"])


# ------------------------------------------------------------------ 3. host checks of the C ABI
def _desc(**kw):
    d = dict(B=2, C=70, h=40, w=40, HL=320, WL=320, N1=121, N2=121, n_bins=4096, n_classes=27, flags=0)
    d.update(kw)
    return capi.pr_desc(**d)


def _map(addr=A):
    return capi.StegoMap(addr, 70 * 1600, 1600, 40, 1)


def _rc(desc, a="map", b="map", la=A, lb=A, ib=None, c1=A, c2=A, hist=A):
    return capi.pr_accumulate_raw(desc, _map() if a == "map" else a, _map() if b == "map" else b, la, lb, ib, c1, c2, hist)


@pytest.mark.parametrize("kw,rc", [
    (dict(C=0), capi.PR_ERR_DIM), (dict(C=769), capi.PR_ERR_DIM), (dict(C=-3), capi.PR_ERR_DIM),
    (dict(N1=0), capi.PR_ERR_POINTS), (dict(N1=4097), capi.PR_ERR_POINTS), (dict(N2=0), capi.PR_ERR_POINTS), (dict(N2=4097), capi.PR_ERR_POINTS),
    (dict(n_bins=63), capi.PR_ERR_BINS), (dict(n_bins=8193), capi.PR_ERR_BINS), (dict(n_bins=0), capi.PR_ERR_BINS),
    (dict(n_classes=0), capi.PR_ERR_CLASSES), (dict(n_classes=256), capi.PR_ERR_CLASSES),
    (dict(B=0), capi.PR_ERR_SIZE), (dict(B=65536), capi.PR_ERR_SIZE), (dict(h=0), capi.PR_ERR_SIZE), (dict(w=16385), capi.PR_ERR_SIZE),
    (dict(HL=0), capi.PR_ERR_SIZE), (dict(WL=16385), capi.PR_ERR_SIZE),
    (dict(flags=4), capi.PR_ERR_FLAGS), (dict(flags=-1), capi.PR_ERR_FLAGS),
])
def test_descriptor_checks(kw, rc):
    assert _rc(_desc(**kw)) == rc
    assert capi.pr_plan(_desc(**kw))[0] == 0
    assert capi.load().stego_error_string(rc).decode().startswith("correspondence PR:")


def test_error_codes_are_distinct_and_free():
    codes = [capi.PR_ERR_DIM, capi.PR_ERR_POINTS, capi.PR_ERR_BINS, capi.PR_ERR_CLASSES, capi.PR_ERR_SIZE, capi.PR_ERR_FLAGS]
    taken = {1, 2, 3, 4, 5, capi.CRF_ERR_LIMITS, capi.CRF_ERR_RANGE, capi.DATA_ERR_RES, capi.DATA_ERR_COUNT, capi.DATA_ERR_ITEM, capi.DATA_ERR_RANGE,
             capi.DATA_ERR_ORIGIN, capi.PROBE_ERR_DIM, capi.PROBE_ERR_SIZE, capi.PROBE_ERR_OUTPUT}
    assert len(set(codes)) == len(codes) and not set(codes) & taken and max(codes) < 1000


@pytest.mark.parametrize("which", ["a", "b", "la", "lb", "c1", "c2", "hist"])
def test_null_and_misaligned_pointers(which):
    null = {which: _map(0) if which in ("a", "b") else None}
    assert _rc(_desc(), **null) == 1                                       # STEGO_ERR_NULL
    off = {which: _map(A + 2) if which in ("a", "b") else A + 2}
    assert _rc(_desc(), **off) == 5                                        # STEGO_ERR_ALIGN
    if which in ("la", "lb", "hist"):
        assert _rc(_desc(), **{which: A + 4}) == 5                          # 64-bit data
    if which in ("a", "b"):
        assert _rc(_desc(), **{which: None}) == 1


def test_null_descriptor_and_index_alignment():
    m = _map()
    assert capi.load().stego_pr_accumulate(None, ctypes.byref(m), ctypes.byref(m), A, A, None, A, A, A, None) == 1
    assert _rc(_desc(), ib=A + 4) == 5
    assert capi.load().stego_pr_plan(None, None, None) == 0


@pytest.mark.parametrize("n_bins", [64, 65, 1000, 4096, 8191, 8192])
@pytest.mark.parametrize("C,N1,N2", [(1, 1, 1), (27, 50, 333), (70, 121, 121), (384, 784, 784), (768, 1600, 1600), (768, 4096, 4096)])
def test_plan_fits_lds(n_bins, C, N1, N2):
    lds, t1, t2 = capi.pr_plan(_desc(n_bins=n_bins, C=C, N1=N1, N2=N2))
    assert n_bins * 2 * 4 < lds <= 160 * 1024, lds
    assert 2 * lds <= 160 * 1024, "two workgroups per CU (csrc/corr_pr.hip)"
    assert (t1, t2) == (-(-N1 // 128), -(-N2 // 128))


def test_symbols_exported_and_abi_unchanged():
    lib = capi.load()
    assert hasattr(lib, "stego_pr_accumulate") and hasattr(lib, "stego_pr_plan")
    assert "stego_pr_accumulate" in capi.SIGNATURES and "stego_pr_plan" in capi.SIGNATURES
    assert lib.stego_abi_version() == 7
    fields = [n for n, _ in capi.StegoPrDesc._fields_]
    assert fields == ["B", "C", "h", "w", "HL", "WL", "N1", "N2", "n_bins", "n_classes", "flags"]
    hdr = open(os.path.join(ROOT, "include", "stego_pr.h")).read()
    order = [hdr.index("int32_t %s" % n) for n in ("B;", "C;", "h, w;", "HL, WL;", "N1, N2;", "n_bins;", "n_classes;", "flags;")]
    assert order == sorted(order)


def test_python_surface_refuses_cpu_tensors():
    f = torch.zeros(1, 4, 5, 5)
    lab = torch.zeros(1, 8, 8, dtype=torch.int64)
    c = torch.zeros(1, 3, 2)
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.pr_accumulate(f, f, lab, lab, c, c, torch.zeros(64, 2, dtype=torch.int64), 3)
    with pytest.raises(RuntimeError, match="MI355X only"):
        CorrespondencePR(n_classes=3, n_bins=64).update(f, f, lab, lab, c, c)
    with pytest.raises(ValueError):
        CorrespondencePR(n_classes=3, n_bins=32)


# ------------------------------------------------------------------ 4. compiled resources
@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_corr_pr_kernel_has_no_spills():
    kernels = _build.kernel_resources("corr_pr.hip")
    pr = {k: v for k, v in kernels.items() if "corr_pr_kernel" in k}
    assert len(pr) == 1, sorted(kernels)                   # one instantiation: flags and shapes are run-time parameters
    for k, v in pr.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        # today: 102 VGPRs + 64 AGPRs (the 128 x 128 fp32 accumulator tile) = 3 waves per SIMD by registers; the 81408 bytes of LDS
        # allow two workgroups (2 waves per SIMD) per CU, which is what the kernel is planned for
        assert v["Occupancy [waves/SIMD]"] >= 2, (k, v)
