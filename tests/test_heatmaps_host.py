"""The query-point correspondence heatmaps without a GPU: the float64 oracle (tests/corr_heatmap_oracle.py) against what the
reference's chain computed (tests/golden/corr_heatmaps_small.npz, tools/make_heatmap_golden.py), every host check of
stego_corr_heatmaps (include/stego_heat.h), the host-only plan, and the pixel arithmetic of the figures."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import corr_heatmap_oracle as O
from conftest import load_golden
from stego_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 0x10000          # a 256-byte aligned stand-in address: the checks reject before any pointer is read
BIG = 1 << 40


# ------------------------------------------------------------------ 1. oracle vs the reference
def test_oracle_matches_reference_golden():
    g = load_golden("corr_heatmaps_small")
    pts = g["points"].reshape(1, -1, 2)
    assert g["feats1"].shape == (1, 24, 6, 5) and pts.shape == (1, 4, 2) and [tuple(s) for s in g["sizes"]] == [(17, 13), (6, 5), (1, 7)]
    for name, tgt in (("intra", g["feats1"]), ("inter", g["feats2"])):
        for H, W in g["sizes"]:
            want = g["%s_%dx%d" % (name, H, W)]
            o = O.heatmaps(g["feats1"], tgt, pts, (int(H), int(W)))
            assert want.shape == (4, H, W) and want.dtype == np.float32
            err = np.abs(o["heat"][0] - want).max()
            print("%s %dx%d: max |oracle - reference fp32| = %.3e" % (name, H, W, err))
            assert err <= 2e-5                                    # the bar tests/test_dense_corr.py holds unit-scale correlations to
    # what the inputs were built to contain: a query inside the zero region (a heatmap of zeros), one beyond the border (equal to
    # the clamped point), one on a corner (the corner cell's own vector: cosine 1 with itself before centring)
    o = O.heatmaps(g["feats1"], g["feats1"], pts, (6, 5))
    assert not o["heat"][0, 1].any() and o["heat"][0, 0].any() and not g["intra_17x13"][1].any()
    clamped = pts.copy()
    clamped[0, 2, 0] = 1.0
    assert np.array_equal(O.heatmaps(g["feats1"], g["feats1"], clamped, (6, 5))["heat"][0, 2], o["heat"][0, 2])
    assert abs(o["raw"][0, 3, 5, 0] - 1.0) < 1e-12 and o["cell"][0, 3] == 5 * 5 and tuple(o["best"][0, 3]) == (-1.0, 1.0)


@pytest.mark.parametrize("center,clamp", [(True, True), (True, False), (False, True), (False, False)])
def test_oracle_identity_size_is_the_low_resolution_map(center, clamp):
    rng = np.random.default_rng(3)
    f = rng.standard_normal((2, 7, 4, 9))
    pts = rng.random((2, 5, 2)) * 2.6 - 1.3
    o = O.heatmaps(f, f, pts, (4, 9), index_t=np.array([1, 1]), center=center, clamp=clamp)
    assert np.array_equal(o["heat"], o["low"])
    assert (o["low"].min() >= 0.0) == clamp
    assert (np.abs(o["low"].mean((2, 3))).max() < 1e-12) == (center and not clamp)
    assert np.array_equal(o["peak"], o["low"].max((2, 3)))
    # a side of size 1 takes source index 0
    one = O.heatmaps(f, f, pts, (1, 1), center=center, clamp=clamp)
    assert np.array_equal(one["heat"][..., 0, 0], one["low"][..., 0, 0])


# ------------------------------------------------------------------ 2. host checks of the C ABI
def _desc(**kw):
    d = dict(B=2, C=70, hs=40, ws=40, h=28, w=28, N=33, H=224, W=224, flags=0)
    d.update(kw)
    return capi.heat_desc(**d)


def _map(addr=A):
    return capi.StegoMap(addr, 70 * 1600, 1600, 40, 1)


def _rc(desc, src="map", tgt="map", it=None, pts=A, heat=A, peak=None, best=None, ws=A, ws_bytes=BIG):
    return capi.corr_heatmaps_raw(desc, _map() if src == "map" else src, _map() if tgt == "map" else tgt, it, pts, heat, peak, best, ws, ws_bytes)


def test_symbols_exported_and_abi_unchanged():
    lib = capi.load()
    for name in ("stego_corr_heatmaps", "stego_heat_workspace_bytes", "stego_heat_plan"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    assert lib.stego_abi_version() == 7
    fields = [n for n, _ in capi.StegoHeatDesc._fields_]
    assert fields == ["B", "C", "hs", "ws", "h", "w", "N", "H", "W", "flags"]
    hdr = open(os.path.join(ROOT, "include", "stego_heat.h")).read()
    order = [hdr.index("int32_t %s" % n) for n in ("B;", "C;", "hs, ws;", "h, w;", "N;", "H, W;", "flags;")]
    assert order == sorted(order)
    for name, value in (("STEGO_ERR_HEAT_DIM", capi.HEAT_ERR_DIM), ("STEGO_ERR_HEAT_POINTS", capi.HEAT_ERR_POINTS),
                        ("STEGO_ERR_HEAT_SIZE", capi.HEAT_ERR_SIZE), ("STEGO_ERR_HEAT_OUTPUT", capi.HEAT_ERR_OUTPUT),
                        ("STEGO_ERR_HEAT_FLAGS", capi.HEAT_ERR_FLAGS), ("STEGO_HEAT_NO_CENTER", capi.HEAT_NO_CENTER),
                        ("STEGO_HEAT_NO_CLAMP", capi.HEAT_NO_CLAMP)):
        assert "%s = %d" % (name, value) in hdr
    for name, value in (("MAX_C", capi.HEAT_MAX_C), ("MAX_POINTS", capi.HEAT_MAX_POINTS), ("MAX_SIDE", capi.HEAT_MAX_SIDE),
                        ("MAX_CELLS", capi.HEAT_MAX_CELLS), ("MAX_OUT", capi.HEAT_MAX_OUT)):
        assert "#define STEGO_HEAT_%s %d" % (name, value) in hdr


@pytest.mark.parametrize("kw,rc", [
    (dict(C=0), capi.HEAT_ERR_DIM), (dict(C=769), capi.HEAT_ERR_DIM), (dict(C=-3), capi.HEAT_ERR_DIM),
    (dict(N=0), capi.HEAT_ERR_POINTS), (dict(N=4097), capi.HEAT_ERR_POINTS), (dict(N=-1), capi.HEAT_ERR_POINTS),
    (dict(B=0), capi.HEAT_ERR_SIZE), (dict(B=65536), capi.HEAT_ERR_SIZE), (dict(hs=0), capi.HEAT_ERR_SIZE), (dict(ws=16385), capi.HEAT_ERR_SIZE),
    (dict(h=0), capi.HEAT_ERR_SIZE), (dict(w=-2), capi.HEAT_ERR_SIZE), (dict(h=129, w=128), capi.HEAT_ERR_SIZE),
    (dict(h=1, w=16385), capi.HEAT_ERR_SIZE), (dict(h=65536, w=65536), capi.HEAT_ERR_SIZE),
    (dict(H=0), capi.HEAT_ERR_OUTPUT), (dict(H=2049), capi.HEAT_ERR_OUTPUT), (dict(W=0), capi.HEAT_ERR_OUTPUT), (dict(W=2049), capi.HEAT_ERR_OUTPUT),
    (dict(flags=4), capi.HEAT_ERR_FLAGS), (dict(flags=-1), capi.HEAT_ERR_FLAGS),
])
def test_descriptor_checks(kw, rc):
    assert _rc(_desc(**kw)) == rc
    assert capi.heat_plan(_desc(**kw))[0] == 0
    assert capi.heat_workspace_bytes(_desc(**kw)) == 0
    assert capi.load().stego_error_string(rc).decode().startswith("correspondence heatmaps:")


def test_error_codes_are_distinct_and_free():
    codes = [capi.HEAT_ERR_DIM, capi.HEAT_ERR_POINTS, capi.HEAT_ERR_SIZE, capi.HEAT_ERR_OUTPUT, capi.HEAT_ERR_FLAGS]
    taken = {1, 2, 3, 4, 5, capi.CRF_ERR_LIMITS, capi.CRF_ERR_RANGE, capi.DATA_ERR_RES, capi.DATA_ERR_COUNT, capi.DATA_ERR_ITEM, capi.DATA_ERR_RANGE,
             capi.DATA_ERR_ORIGIN, capi.PROBE_ERR_DIM, capi.PROBE_ERR_SIZE, capi.PROBE_ERR_OUTPUT, capi.PR_ERR_DIM, capi.PR_ERR_POINTS,
             capi.PR_ERR_BINS, capi.PR_ERR_CLASSES, capi.PR_ERR_SIZE, capi.PR_ERR_FLAGS, capi.PTRAIN_ERR_DIM, capi.PTRAIN_ERR_SIZE,
             capi.PTRAIN_ERR_PROBES}
    assert len(set(codes)) == len(codes) and not set(codes) & taken and max(codes) < 1000


@pytest.mark.parametrize("which", ["src", "tgt", "pts", "heat", "ws"])
def test_null_and_misaligned_pointers(which):
    null = {which: _map(0) if which in ("src", "tgt") else None}
    assert _rc(_desc(), **null) == 1                                       # STEGO_ERR_NULL
    off = {which: _map(A + 2) if which in ("src", "tgt") else A + 2}
    assert _rc(_desc(), **off) == 5                                        # STEGO_ERR_ALIGN
    if which == "ws":
        assert _rc(_desc(), ws=A + 4) == 5                                  # it holds float64 partial sums
    if which in ("src", "tgt"):
        assert _rc(_desc(), **{which: None}) == 1


def test_optional_pointers_workspace_size_and_null_descriptor():
    m = _map()
    assert capi.load().stego_corr_heatmaps(None, ctypes.byref(m), ctypes.byref(m), None, A, A, None, None, A, BIG, None) == 1
    assert capi.load().stego_heat_plan(None, None, None, None, None) == 0 and capi.load().stego_heat_workspace_bytes(None) == 0
    assert _rc(_desc(), it=A + 4) == 5 and _rc(_desc(), peak=A + 2) == 5 and _rc(_desc(), best=A + 1) == 5
    n = capi.heat_workspace_bytes(_desc())
    assert n > 0 and _rc(_desc(), ws_bytes=n - 1) == 4 and _rc(_desc(), ws_bytes=0) == 4      # STEGO_ERR_WORKSPACE


@pytest.mark.parametrize("C,h,w,N,H,W", [
    (384, 64, 64, 280, 512, 512), (384, 64, 64, 3, 512, 512), (70, 64, 64, 1, 512, 512),            # the movie, the figure, interactive
    (1, 1, 1, 1, 1, 1), (768, 128, 128, 4096, 2048, 2048), (8, 4, 4, 1100, 1024, 1024),
    (24, 1, 16384, 2, 2048, 2048), (24, 16384, 1, 2, 2048, 2048), (24, 2, 8192, 1, 3, 2048), (24, 128, 128, 1, 1, 1),
    (24, 128, 128, 5, 3, 7), (3, 1, 9, 2, 4, 20), (192, 28, 28, 1, 10, 10), (384, 7, 11, 33, 50, 37),
])
def test_plan_covers_the_output_and_fits_the_lds(C, h, w, N, H, W):
    B = 2
    d = _desc(B=B, C=C, h=h, w=w, N=N, H=H, W=W)
    lds1, g1, g2, lds2, rows = capi.heat_plan(d)
    nch = -(-(h * w) // 128)
    assert 0 < lds1 and 2 * lds1 <= 160 * 1024, "two workgroups of the first launch per CU (csrc/corr_heat.hip)"
    assert g1 == (nch, -(-N // 128), B)
    assert rows >= 1 and g2 == (-(-H // rows), N, B) and all(0 < v <= 65535 for v in g1 + g2)
    # every block's source rows fit what it allocates: the span in float32 arithmetic, as the kernel computes it
    sy = np.float32(h - 1) / np.float32(H - 1) if H > 1 else np.float32(0)
    span = 1
    for y0 in range(0, H, rows):
        y1 = min(y0 + rows, H)
        lo, hi = min(int(sy * np.float32(y0)), h - 1), min(int(sy * np.float32(y1 - 1)), h - 1)
        span = max(span, min(hi + 1, h - 1) - lo + 1)
    assert lds2 == span * w * 4 and 4 <= lds2 <= 64 * 1024
    assert capi.heat_workspace_bytes(d) == (B * N * (nch * 16 + h * w * 4) + 7) // 8 * 8


def test_python_surface_refuses_cpu_tensors_and_batches():
    from stego_amd import correspondence_heatmaps as CH
    f = torch.zeros(1, 4, 5, 5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.corr_heatmaps(f, f, torch.zeros(1, 3, 2), (8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        CH.correspondence_heatmaps(f, f, torch.zeros(1, 3, 1, 2), (8, 8), want_best=True)

    def net(img):
        raise AssertionError("the batch check comes before the network runs")
    with pytest.raises(ValueError, match="correspondence_heatmaps"):
        CH.get_heatmaps(net, torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 1, 2))


# ------------------------------------------------------------------ 3. the figures
def test_render_overlay_by_hand():
    from stego_amd.correspondence_heatmaps import render_overlay
    img = np.array([[[255, 255, 255], [0, 0, 0]], [[255, 0, 0], [10, 200, 90]]], dtype=np.uint8)
    heat = np.array([[0.0, 2.0], [1.0, 0.5]])
    # grey * 0.8: white (0.2989 + 0.5870 + 0.1140) * 0.8 = 0.79992; black 0; red 0.2989 * 0.8 = 0.23912;
    # (10 * 0.2989 + 200 * 0.5870 + 90 * 0.1140) / 255 * 0.8 = 0.409870...
    # ramp index min(floor(heat / 2 * 255), 254): 0, 254, 127, 63 -> opacity 0.5 * i / 255: 0, 0.498039, 0.249020, 0.123529
    # red (1, 0, 0) over the grey g at opacity a: (g (1 - a) + a, g (1 - a), g (1 - a)), then round(255 x)
    want = np.array([[[204, 204, 204], [127, 0, 0]], [[109, 46, 46], [123, 92, 92]]], dtype=np.uint8)
    got = render_overlay(img, heat, (1, 0, 0))
    assert got.dtype == np.uint8 and np.array_equal(got, want), got
    # an explicit vmax of 4.1: ramp indices 0, 124, 62, 31 -> opacities 0, 62 / 255, 31 / 255, 15.5 / 255; yellow writes two channels
    want4 = np.array([[[204, 204, 204], [62, 62, 0]], [[85, 85, 54], [114, 114, 98]]], dtype=np.uint8)
    got4 = render_overlay(img, heat, (1, 1, 0), vmax=4.1)
    assert np.array_equal(got4, want4), got4
    # a map of zeros leaves the grey image; a wrong size is refused
    assert np.array_equal(render_overlay(img, np.zeros((2, 2)), (0, 1, 0)), np.array([[[204] * 3, [0] * 3], [[61] * 3, [105] * 3]], dtype=np.uint8))
    with pytest.raises(ValueError):
        render_overlay(img, np.zeros((3, 2)), (0, 1, 0))


def test_movie_path_is_the_references():
    from stego_amd.correspondence_heatmaps import COLOURS, movie_points
    pts = movie_points()
    assert len(pts) == 280 and pts[0] == [-.7, -.7] and pts[59] == [-.7, -.7] and pts[110] == [-.1, 0.0] and pts[279] == [.5, .8]
    assert pts[60] == [-.7, -.7] and pts[109] == [-.1, 0.0]                 # np.linspace includes both ends
    np.testing.assert_allclose(pts[61], [-.7 + .6 / 49, -.7 + .7 / 49], rtol=0, atol=1e-15)
    assert COLOURS == ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0))


def test_config_loads():
    from stego_amd.correspondence_heatmaps import PLOT_CONFIG, result_dir
    from stego_amd.train_segmentation import load_config
    cfg = load_config(PLOT_CONFIG, overrides=["output_root=/out", "movie_frames=4"])
    assert cfg.high_res == 512 and cfg.image_num == 6 and cfg.plot_correspondence is True and cfg.plot_movie is True
    assert cfg.query_points == [[-.1, 0.0], [.5, .8], [-.7, -.7]] and cfg.movie_frames == 4
    assert cfg.image is None and cfg.image_pos is None and cfg.result_dir is None
    assert (cfg.model_type, cfg.dino_patch_size, cfg.dim, cfg.arch, cfg.dataset_name, cfg.res) == ("vit_small", 8, 70, "dino", "cocostuff27", 224)
    assert result_dir(cfg) == os.path.join("/out", "results", "correspondence")
    assert result_dir(types.SimpleNamespace(result_dir="/r", output_root="/out")) == "/r"
