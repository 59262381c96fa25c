"""csrc/corr_heat.hip on the MI355X against the float64 oracle (tests/corr_heatmap_oracle.py) on the same fp32 inputs.

The bar (the one tests/test_probe_head_gpu.py uses): the kernel's max |error| against the oracle is at most twice the max |error| of
the torch fp32 chain of the reference (grid_sample, two F.normalize, einsum, mean, clamp, F.interpolate, run here on the device on
the same input) against that same oracle, plus 1e-6.  Every case prints both numbers.  `peak` is held to the same bar against the
chain's own low-resolution maximum.  `best` must equal the oracle's wherever the oracle's two largest cells differ by more than 1e-4
(the probe head's convention for an argmax); on the seeded random cases that is every query, asserted on the oracle side before the
kernel is looked at (the seeds were picked on the CPU for it).  What integers decide - repeatability, the copy at identity size,
a heatmap of zeros, full overwrite - is compared exactly."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import corr_heatmap_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GAP = 1e-4

# name: (B, C, (hs, ws), (h, w), N, (H, W), source layout, target layout, seed)
SHAPES = {
    "golden_shape": (2, 24, (6, 5), (6, 5), 4, (17, 13), "nchw", "nchw", 0),
    "one_row": (2, 3, (1, 9), (1, 9), 2, (4, 20), "nchw", "nchw", 1),
    "code_28": (2, 70, (28, 28), (28, 28), 9, (224, 224), "cl", "cl", 0),
    "two_sizes_nchw_cl": (2, 384, (13, 9), (7, 11), 33, (50, 37), "nchw", "cl", 10),
    "two_sizes_cl_nchw": (2, 384, (13, 9), (7, 11), 33, (50, 37), "cl", "nchw", 2),
    "downsample": (2, 192, (28, 28), (28, 28), 1, (10, 10), "cl", "cl", 0),
    "c768_n130": (2, 768, (16, 16), (16, 16), 130, (64, 64), "cl", "cl", 8),
    "out_h1": (2, 24, (6, 5), (6, 5), 4, (1, 13), "nchw", "nchw", 0),
    "out_w1": (2, 24, (6, 5), (6, 5), 4, (17, 1), "nchw", "cl", 0),
    "out_1x1": (2, 24, (6, 5), (6, 5), 4, (1, 1), "cl", "nchw", 0),
    "odd_width": (1, 40, (9, 9), (9, 9), 5, (31, 30), "cl", "cl", 0),          # W % 4 != 0: the 4-byte store path, more than one row block
}


def _features(rng, B, C, h, w):
    """Low-rank structure plus noise, so that the cosines spread over [-1, 1] instead of piling up around 0."""
    proto = rng.standard_normal((5, C))
    z = rng.standard_normal((B, 5, h, w))
    return (np.einsum("brhw,rc->bchw", z, proto) + 0.5 * rng.standard_normal((B, C, h, w))).astype(np.float32)


def _inputs(name):
    B, C, (hs, ws), (h, w), N, size, ls, lt, seed = SHAPES[name]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    src = _features(rng, B, C, hs, ws)
    tgt = src if (hs, ws) == (h, w) and name != "code_28" else _features(rng, B, C, h, w)      # self and cross targets
    pts = (rng.random((B, N, 2)) * 2 - 1).astype(np.float32)
    return src, tgt, pts, size, ls, lt


def _dev_map(f, layout):
    t = torch.from_numpy(f).to(DEV)
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if layout == "cl" else t


def _chain(src, tgt, pts, size, index_t=None, center=True, clamp=True):
    """plot_dino_correspondence.py:43-56 with a batch dimension, torch fp32 on the device -> (heat, low)."""
    B, N = pts.shape[:2]
    s = F.grid_sample(src, pts.reshape(B, N, 1, 2).permute(0, 2, 1, 3), padding_mode="border", align_corners=True)   # modules.sample
    t = tgt if index_t is None else tgt[index_t.clamp(0, B - 1)]
    attn = torch.einsum("nchw,ncij->nhwij", F.normalize(s, dim=1), F.normalize(t, dim=1))[:, 0]
    if center:
        attn = attn - attn.mean([2, 3], keepdim=True)
    if clamp:
        attn = attn.clamp(0)
    return F.interpolate(attn, size, mode="bilinear", align_corners=True), attn


def _err(t, ref):
    return float(np.abs(t.detach().cpu().numpy().astype(np.float64) - ref).max())


def _compare(tag, src, tgt, pts, size, ls="nchw", lt="nchw", index_t=None, center=True, clamp=True, all_best=False, best=True):
    """Runs oracle, chain and kernel on one input, prints the errors, asserts the bar; returns (oracle, kernel heat, peak, best)."""
    from stego_amd.correspondence_heatmaps import correspondence_heatmaps
    o = O.heatmaps(src, tgt, pts, size, index_t=index_t, center=center, clamp=clamp)
    sure = o["gap"] > GAP
    if all_best:
        assert sure.all(), "%s: pick another seed, top-2 gaps %s" % (tag, np.sort(o["gap"].ravel())[:3])
    ts = _dev_map(src, ls)
    tt = ts if (tgt is src and lt == ls) else _dev_map(tgt, lt)
    tp = torch.from_numpy(pts).to(DEV)
    ti = None if index_t is None else torch.from_numpy(np.asarray(index_t, dtype=np.int64)).to(DEV)
    c_heat, c_low = _chain(ts, tt, tp, size, ti, center, clamp)
    heat, peak, bst = correspondence_heatmaps(ts, tt, tp, size, center=center, clamp=clamp, index_t=ti, want_best=True)
    assert heat.shape == o["heat"].shape and heat.dtype == torch.float32 and heat.is_cuda and heat.is_contiguous()
    assert peak.shape == o["peak"].shape and bst.shape == o["best"].shape
    kerr, cerr = _err(heat, o["heat"]), _err(c_heat, o["heat"])
    kpeak, cpeak = _err(peak, o["peak"]), _err(c_low.flatten(2).amax(2), o["peak"])
    print("%-40s heat: kernel %.3e chain %.3e   peak: kernel %.3e chain %.3e   min top-2 gap %.2e" % (tag, kerr, cerr, kpeak, cpeak, o["gap"].min()))
    assert kerr <= 2 * cerr + 1e-6, (tag, kerr, cerr)
    assert kpeak <= 2 * cpeak + 1e-6, (tag, kpeak, cpeak)
    if best:
        got = bst.cpu().numpy().astype(np.float64)
        assert np.abs(got - o["best"])[sure].max(initial=0.0) <= 1e-6, (tag, got[sure], o["best"][sure])
    return o, heat, peak, bst


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes(name):
    src, tgt, pts, size, ls, lt = _inputs(name)
    _compare(name, src, tgt, pts, size, ls, lt, all_best=True)


@pytest.mark.parametrize("center,clamp", [(True, True), (True, False), (False, True), (False, False)])
def test_flags(center, clamp):
    for name in ("golden_shape", "two_sizes_nchw_cl"):
        src, tgt, pts, size, ls, lt = _inputs(name)
        o, heat, _, _ = _compare("%s center=%s clamp=%s" % (name, center, clamp), src, tgt, pts, size, ls, lt, center=center, clamp=clamp,
                                 all_best=True)
        assert (float(heat.min()) >= 0.0) == clamp


def test_identity_size_is_a_copy_of_the_workspace_map():
    """C = 1 at the map's own size: with both flags off the output is the workspace's low-resolution map bit for bit; with centring
    and the clamp it is max(low - mean, 0) of that map, the mean taken from the workspace's float64 partial sums."""
    from stego_amd import capi
    rng = np.random.default_rng(12)
    src = rng.standard_normal((2, 1, 5, 5)).astype(np.float32)
    pts = (rng.random((2, 3, 2)) * 2 - 1).astype(np.float32)
    ts, tp = torch.from_numpy(src).to(DEV), torch.from_numpy(pts).to(DEV)
    heat, desc, ws = capi.corr_heatmaps(ts, ts, tp, (5, 5), center=False, clamp=False, keep_workspace=True)
    torch.cuda.synchronize()
    psum, low, pmax, pidx = capi.heat_workspace_views(desc, ws)
    assert low.shape == heat.shape and torch.equal(heat, low)
    assert float((low.abs() - 1).abs().max()) <= 1e-6                          # cosines of scalars: +-1
    # one chunk of cells: its float64 sum of 25 floats is exact in any order; the first maximum in row-major order
    assert torch.equal(psum[..., 0], low.double().sum((2, 3))) and torch.equal(pmax[..., 0], low.flatten(2).amax(2))
    assert np.array_equal(pidx[..., 0].cpu().numpy(), low.flatten(2).cpu().numpy().argmax(2))
    heat2, desc2, ws2 = capi.corr_heatmaps(ts, ts, tp, (5, 5), keep_workspace=True)
    low2 = capi.heat_workspace_views(desc2, ws2)[1]
    mean = (low2.double().sum((2, 3), keepdim=True) / 25).float()
    assert torch.equal(low2, low) and torch.equal(heat2, (low2 - mean).clamp(min=0))
    _compare("c1_identity", src, src, pts, (5, 5), best=False)                  # (ties between equal cosines: `best` is not unique)


def _special_points(h, w):
    """On grid nodes, on +-1, at +-1.3 (beyond the border), two inside the zero region rows 2-5 x columns 0-2 (between nodes and on a node
    whose neighbours are zero too: a weight that rounding makes 1e-7 instead of 0 must not reach a non-zero vector, which the
    normalisation would blow up to full size), and two generic ones."""
    node = lambda i, n: 2.0 * i / (n - 1) - 1.0
    return np.array([[node(2, w), node(1, h)], [node(w - 2, w), node(h - 1, h)], [1.0, 1.0], [-1.0, -1.0], [1.0, -1.0], [1.3, -1.3],
                     [-1.3, 0.2], [0.4, 1.3], [node(0.5, w), node(3.5, h)], [node(1, w), node(4, h)], [0.13, -0.58], [-0.41, 0.77]], dtype=np.float32)


@pytest.mark.parametrize("layout", ["nchw", "cl"])
def test_points(layout):
    rng = np.random.default_rng(21)
    B, C, h, w = 2, 40, 8, 7
    src = _features(rng, B, C, h, w)
    src[:, :, 2:6, 0:3] = 0.0
    pts = np.repeat(_special_points(h, w)[None], B, 0)
    for tgt, tag in ((src, "self"), (_features(rng, B, C, h, w), "cross")):
        o, heat, peak, bst = _compare("points %s %s" % (layout, tag), src, tgt, pts, (19, 22), layout, layout)
        assert not o["heat"][:, 8:10].any() and not heat[:, 8:10].any()        # inside the zero region: a heatmap of zeros ...
        assert not peak[:, 8:10].any() and torch.equal(bst[:, 8:10], torch.full((B, 2, 2), -1.0, device=DEV))     # ... whose first cell wins
        if tag == "self":                                                      # a node sees itself: cosine 1 at its own cell
            assert np.allclose(o["best"][:, 0], pts[:, 0], atol=1e-6) and np.allclose(o["best"][:, 2], [1.0, 1.0])
        # beyond the border = on the border
        clamped = np.clip(pts, -1.0, 1.0)
        _, heat_c, _, _ = _compare("points %s %s clamped" % (layout, tag), src, tgt, clamped, (19, 22), layout, layout)
        assert torch.equal(heat_c, heat)


def test_zero_and_constant_targets():
    rng = np.random.default_rng(22)
    B, C, h, w, N = 2, 70, 9, 12, 6
    src = _features(rng, B, C, h, w)
    pts = (rng.random((B, N, 2)) * 2 - 1).astype(np.float32)
    tgt = _features(rng, B, C, h, w)
    tgt[0, :, 2:5, 3:9] = 0.0                                                  # zero vectors: cosine 0 with everything
    tgt[1, :, 0, 0] = 0.0
    o, heat, _, _ = _compare("zero cells in the target", src, tgt, pts, (30, 44), "cl", "cl")
    assert (o["raw"][0, :, 2:5, 3:9] == 0).all()
    const = np.repeat(np.repeat(rng.standard_normal((B, C, 1, 1)).astype(np.float32), h, 2), w, 3)
    for center in (True, False):
        o, heat, peak, _ = _compare("constant target center=%s" % center, src, const, pts, (30, 44), "cl", "nchw", center=center, best=False)
        if center:                                                              # every cell equals the mean
            assert float(heat.abs().max()) <= 1e-6 and float(peak.abs().max()) <= 1e-6


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_magnitudes(scale):
    for name in ("golden_shape", "two_sizes_nchw_cl"):
        src, tgt, pts, size, ls, lt = _inputs(name)
        s = np.float32(scale)
        ssrc = src * s
        stgt = ssrc if tgt is src else tgt * s
        o, heat, _, _ = _compare("%s x %g" % (name, scale), ssrc, stgt, pts, size, ls, lt, all_best=True)
        o1 = O.heatmaps(src, tgt, pts, size)
        assert np.abs(o["heat"] - o1["heat"]).max() <= 1e-6                    # the result is scale free


def test_index_t_permutation_with_a_repeat():
    rng = np.random.default_rng(23)
    B, C, N = 4, 70, 7
    src, tgt = _features(rng, B, C, 10, 10), _features(rng, B, C, 6, 8)
    pts = (rng.random((B, N, 2)) * 2 - 1).astype(np.float32)
    index_t = np.array([2, 0, 2, 1])
    o, heat, _, _ = _compare("index_t", src, tgt, pts, (21, 24), "cl", "cl", index_t=index_t, all_best=True)
    plain = O.heatmaps(src, tgt[index_t], pts, (21, 24))
    assert np.array_equal(o["heat"], plain["heat"]) and not np.array_equal(o["heat"], O.heatmaps(src, tgt, pts, (21, 24))["heat"])
    _compare("index_t out of range is clamped", src, tgt, pts, (21, 24), "cl", "cl", index_t=np.array([-5, 0, 9, 3]))


def _raw_call(ts, tt, tp, size, heat, peak=None, best=None):
    from stego_amd import capi
    B, C, hs, ws = ts.shape
    desc = capi.heat_desc(B, C, hs, ws, tt.shape[2], tt.shape[3], tp.shape[1], size[0], size[1])
    n = capi.heat_workspace_bytes(desc)
    wsb = torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)                  # NaN patterns: the workspace needs no initialisation
    rc = capi.corr_heatmaps_raw(desc, capi._map(ts), capi._map(tt), None, tp, heat, peak, best, wsb, n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return wsb


@pytest.mark.parametrize("name", ["code_28", "odd_width", "c768_n130"])
def test_repeat_launches_are_bitwise_equal_and_overwrite_everything(name):
    src, tgt, pts, size, ls, lt = _inputs(name)
    B, N = pts.shape[:2]
    ts, tt, tp = _dev_map(src, ls), _dev_map(tgt, lt), torch.from_numpy(pts).to(DEV)
    outs = []
    for _ in range(3):
        heat = torch.full((B, N) + tuple(size), float("nan"), device=DEV)
        peak = torch.full((B, N), float("nan"), device=DEV)
        best = torch.full((B, N, 2), float("nan"), device=DEV)
        _raw_call(ts, tt, tp, size, heat, peak, best)
        assert not torch.isnan(heat).any() and not torch.isnan(peak).any() and not torch.isnan(best).any()
        outs.append((heat, peak, best))
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
    # an unaligned output (a view one float into a larger buffer) takes the 4-byte store path: same values
    buf = torch.full((B * N * size[0] * size[1] + 1,), float("nan"), device=DEV)
    view = buf[1:].view(B, N, *size)
    _raw_call(ts, tt, tp, size, view)
    assert torch.equal(view, outs[0][0]) and torch.isnan(buf[0])


def test_offsets_beyond_4_gib():
    """B = 1, N = 1100 heatmaps of 1024 x 1024: 4.6 GB; heatmap 1024 starts exactly 2^32 bytes into the output."""
    from stego_amd.correspondence_heatmaps import correspondence_heatmaps
    rng = np.random.default_rng(24)
    C, N, size = 8, 1100, (1024, 1024)
    src = _features(rng, 1, C, 4, 4)
    pts = (rng.random((1, N, 2)) * 2 - 1).astype(np.float32)
    ts, tp = torch.from_numpy(src).to(DEV), torch.from_numpy(pts).to(DEV)
    heat = correspondence_heatmaps(ts, ts, tp, size)
    assert heat.numel() * 4 > 2 ** 32 and heat.shape == (1, N) + size
    pick = [0, 1023, 1024, 1099]
    o = O.heatmaps(src, src, pts[:, pick], size)
    c_heat, _ = _chain(ts, ts, tp[:, pick], size)
    kerr, cerr = _err(heat[:, pick], o["heat"]), _err(c_heat, o["heat"])
    print("beyond 2^32 bytes: kernel %.3e chain %.3e" % (kerr, cerr))
    assert kerr <= 2 * cerr + 1e-6
    assert torch.equal(heat[:, pick], correspondence_heatmaps(ts, ts, tp[:, pick].contiguous(), size))
    del heat
    torch.cuda.empty_cache()


def _tiny_net():
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=2", "dim=70", "dropout=False"])
    torch.manual_seed(0)
    return LitUnsupervisedSegmenter(27, cfg).to(DEV).eval().net


@pytest.mark.parametrize("which", ["feats", "code"])
def test_get_heatmaps_on_a_tiny_featurizer(which):
    from stego_amd.correspondence_heatmaps import get_heatmaps
    net = _tiny_net()
    g = torch.Generator().manual_seed(5)
    img, img_pos = torch.randn(1, 3, 64, 64, generator=g), torch.randn(1, 3, 64, 48, generator=g)
    q = torch.tensor([[-.1, 0.0], [.5, .8], [-.7, -.7], [1.0, -1.0]]).reshape(1, 4, 1, 2)
    intra, inter = get_heatmaps(net, img, img_pos, q, which)
    assert intra.shape == (4, 64, 64) and inter.shape == (4, 64, 48) and not intra.is_cuda and not inter.is_cuda
    assert intra.dtype == torch.float32 and float(intra.min()) >= 0.0 and float(intra.max()) > 0.0
    with torch.no_grad():
        m1 = dict(zip(("feats", "code"), net(img.to(DEV))))[which].float()
        m2 = dict(zip(("feats", "code"), net(img_pos.to(DEV))))[which].float()
    assert m1.shape[1] == (192 if which == "feats" else 70) and m1.shape[2:] == (4, 4) and m2.shape[2:] == (4, 3)
    pts = q.reshape(1, 4, 2).numpy()
    for got, tgt, size in ((intra, m1, (64, 64)), (inter, m2, (64, 48))):
        o = O.heatmaps(m1.cpu().numpy(), tgt.cpu().numpy(), pts, size)
        c_heat, _ = _chain(m1, tgt, q.reshape(1, 4, 2).to(DEV), size)
        kerr, cerr = _err(got[None], o["heat"]), _err(c_heat, o["heat"])
        print("get_heatmaps %s -> %s: kernel %.3e chain %.3e" % (which, size, kerr, cerr))
        assert kerr <= 2 * cerr + 1e-6
    with pytest.raises(ValueError, match="correspondence_heatmaps"):
        get_heatmaps(net, img.repeat(2, 1, 1, 1), img_pos.repeat(2, 1, 1, 1), q.repeat(2, 1, 1, 1))


def test_my_app_writes_the_figure_and_the_frames(tmp_path, capsys):
    from PIL import Image
    from stego_amd import correspondence_heatmaps as CH
    from stego_amd.train_segmentation import load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(CH.PLOT_CONFIG, overrides=["model_type=vit_tiny", "dino_patch_size=16", "high_res=64", "movie_frames=4", "dropout=False",
                                                 "result_dir=%s" % (tmp_path / "out"), "pytorch_data_dir=%s" % (tmp_path / "none"), "num_workers=0"])
    written = CH.my_app(cfg)
    assert "synthetic data" in capsys.readouterr().out
    out = str(tmp_path / "out")
    assert written == [os.path.join(out, "correspondence.png")] + [os.path.join(out, "attention_interp", "frame_%04d.png" % i) for i in range(4)]
    assert sorted(os.listdir(os.path.join(out, "attention_interp"))) == ["frame_%04d.png" % i for i in range(4)]
    for path in written:
        with Image.open(path) as im:
            assert im.size == (3 * 64 + 16, 64) and im.mode == "RGB"
    with Image.open(written[0]) as im:
        fig = np.asarray(im)
    # the left panel is the image with its coloured crosses; the other two are grey images with coloured overlays
    assert (fig[:, 72:136] != fig[:, 72:136, :1]).any() and (fig[:, 144:] != fig[:, 144:, :1]).any() and not fig[:, 64:72].any()
    cx, cy = int((-.1 + 1) / 2 * 64), int((0.0 + 1) / 2 * 64)
    assert (fig[cy - 2:cy + 3, cx - 2:cx + 3] == (255, 0, 0)).all(-1).any()     # the first point's red cross
    # two image files instead of the dataset
    rng = np.random.default_rng(3)
    Image.fromarray(rng.integers(0, 256, (80, 100, 3), dtype=np.uint8)).save(tmp_path / "a.png")
    Image.fromarray(rng.integers(0, 256, (70, 64), dtype=np.uint8), "L").save(tmp_path / "b.png")
    cfg2 = load_config(CH.PLOT_CONFIG, overrides=["model_type=vit_tiny", "dino_patch_size=16", "high_res=64", "plot_movie=False", "dropout=False",
                                                  "output_root=%s" % tmp_path, "image=%s" % (tmp_path / "a.png"), "image_pos=%s" % (tmp_path / "b.png"),
                                                  "map=code"])
    assert CH.my_app(cfg2) == [os.path.join(str(tmp_path), "results", "correspondence", "correspondence.png")]
    assert "synthetic" not in capsys.readouterr().out
