"""Coloured pictures on the MI355X (include/stego_render.h, csrc/render.hip, stego_amd.render).

The label paths are exact: they are compared bit for bit with a numpy restatement of the header's rules.  The image paths are
compared with a float64 restatement computed from the same fp32 inputs: every value within one level, and at most max(2, 1 %) of
the values different at all.  That cap is a condition on the arithmetic, not a measurement of it: the fp32 chain and float64
truncation part ways only where v' * 255 lies within an fp32 rounding of an integer (about 1e-4 of random values), while a rounded
conversion or a contracted multiply-add moves tens of percent.  Two kinds of input would make the true value an exact integer on
purpose and so decide the comparison by the last bit: a blend over clamped pixels (0.3 * k is an integer for every colour value k
that is a multiple of 10) - the blend images therefore stay inside (0, 1) after un-normalisation, and clamping is checked on the
image-only path, where 0 and 1 give 0 and 255 in either arithmetic - and the two pixels that hold an image's minimum and maximum
under RESCALE, which the cap's "2" allows for.

Shapes: the smallest where the packing can go wrong (one pixel, one row shorter and longer than a 16-byte piece, odd sizes over
more than one block of 16 rows), and one wider than the 256 pixels of a workgroup's chunk, so that pixels straddle chunks.
"""
import os
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

from stego_amd import capi, render

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(1, 1, 1), (1, 1, 17), (3, 37, 53), (2, 64, 64), (1, 5, 16), (1, 2, 15), (1, 18, 523)]
DTYPES = [torch.int64, torch.int32, torch.uint8]
EDGE = (255, 254, 253)


def _labels(shape, n_lut, dtype, seed=0):
    """Random labels in [0, n_lut) in patches (so that edges are neither everywhere nor nowhere), with n_lut - 1, and where the
    dtype holds them -1 and n_lut, sprinkled in."""
    rng = np.random.default_rng(seed)
    B, H, W = shape
    lab = rng.integers(0, n_lut, (B, (H + 2) // 3, (W + 3) // 4)).repeat(3, 1).repeat(4, 2)[:, :H, :W].copy()
    special = [n_lut - 1] + ([-1] if dtype != torch.uint8 else []) + ([n_lut] if dtype != torch.uint8 or n_lut < 256 else [])
    for i, v in enumerate(special * 3):
        lab[rng.integers(B), rng.integers(H), rng.integers(W)] = v
    lab[0, 0, 0] = special[-1]
    lab[-1, -1, -1] = special[0]
    return lab


def _cmap(n_lut, seed=1):
    if n_lut == 512:
        return render.pascal_label_colormap()
    return np.random.default_rng(seed).integers(0, 256, (n_lut, 3))


def np_colorize(lab, cmap, edges=False):
    """The header's rules in numpy: lut[l] inside [0, n_lut), cmap[-1] outside; with edges, EDGE where the label differs from the
    right or the lower neighbour inside the image."""
    n = cmap.shape[0]
    table = np.concatenate([cmap, cmap[-1:]], 0).astype(np.uint8)
    rgb = table[np.where((lab >= 0) & (lab < n), lab, n)]
    if edges:
        e = np.zeros(lab.shape, dtype=bool)
        e[:, :, :-1] |= lab[:, :, 1:] != lab[:, :, :-1]
        e[:, :-1, :] |= lab[:, 1:, :] != lab[:, :-1, :]
        rgb[e] = np.array(EDGE, np.uint8)
    return rgb


def np_unit64(img, rescale, mean, std):
    """v' of the header in float64 from the fp32 image [B, 3, H, W] -> [B, H, W, 3]."""
    m = np.asarray(mean, np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    s = np.asarray(std, np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    v = (img.astype(np.float64) * s + m).transpose(0, 2, 3, 1)
    if not rescale:
        return np.clip(v, 0, 1)
    lo, hi = v.min((1, 2, 3), keepdims=True), v.max((1, 2, 3), keepdims=True)
    return np.where(hi > lo, (v - lo) / np.where(hi > lo, hi - lo, 1), 0)


def np_levels64(f):
    return np.clip(np.floor(f * 255.0), 0, 255).astype(np.uint8)


def close_to_f64(got, want, what):
    """Within one level everywhere, and at most max(2, 1 %) of the values different; prints the observed count."""
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    n = int((diff > 0).sum())
    print("%s: %d of %d values differ from float64 truncation (cap %d), max %d level(s)"
          % (what, n, diff.size, max(2, diff.size // 100), int(diff.max())))
    assert diff.max() <= 1, what
    assert n <= max(2, diff.size // 100), what


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_labels_and_edges_are_exact(shape, dtype):
    for n_lut in (1, 27, 512):
        cmap = _cmap(n_lut)
        lab = _labels(shape, n_lut, dtype)
        t = torch.from_numpy(lab).to(dtype).to(DEV)
        lab = t.cpu().numpy().astype(np.int64)                       # what the dtype really holds
        got = render.colorize(t, cmap)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == shape + (3,)
        assert np.array_equal(got.cpu().numpy(), np_colorize(lab, cmap)), n_lut
        got = render.colorize(t, cmap, edges=True, edge_color=EDGE)
        assert np.array_equal(got.cpu().numpy(), np_colorize(lab, cmap, edges=True)), n_lut


def test_mapping_is_composed_into_the_table():
    cmap = render.cityscapes_colormap()
    mapping = np.array([3, -1, 0, 27, 5, 99, -1])
    lab = _labels((2, 19, 23), 7, torch.int64, seed=4)
    got = render.colorize(torch.from_numpy(lab).to(DEV), cmap, mapping=mapping).cpu().numpy()
    table = np.stack([cmap[3], cmap[-1], cmap[0], cmap[27], cmap[5], cmap[-1], cmap[-1]])
    assert np.array_equal(got, np_colorize(lab, table))              # the table's last entry is cmap[-1], the ignore colour
    assert np.array_equal(got, render.torch_colorize(torch.from_numpy(lab), cmap, mapping=mapping).numpy())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_strided_label_views(dtype):
    cmap = _cmap(27)
    full = torch.from_numpy(_labels((3, 40, 120), 27, dtype, seed=5)).to(dtype).to(DEV)
    for view in (full[:, 1:38, 3:109:2], full[::2, ::3, 7:60], full.permute(0, 2, 1)[:, 5:58, :37], full[:, :, 1:]):
        assert not view.is_contiguous()
        want = np_colorize(view.cpu().numpy().astype(np.int64), cmap, edges=True)
        assert np.array_equal(render.colorize(view, cmap, edges=True, edge_color=EDGE).cpu().numpy(), want)


def _image(shape, seed, lo=None, hi=None, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    B, H, W = shape
    if lo is None:
        return torch.randn(B, 3, H, W, generator=g) * scale
    return torch.rand(B, 3, H, W, generator=g) * (hi - lo) + lo


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_image_u8_against_float64(shape):
    img = _image(shape, 7)
    for rescale in (True, False):
        for mean, std in ((render.PLOT_MEAN, render.PLOT_STD), (render.IMAGENET_MEAN, render.IMAGENET_STD)):
            want = np_levels64(np_unit64(img.numpy(), rescale, mean, std))
            got = render.image_u8(img.to(DEV), rescale=rescale, mean=mean, std=std)
            close_to_f64(got.cpu().numpy(), want, "image_u8 %s rescale=%s" % (shape, rescale))
            cl = img.to(DEV).contiguous(memory_format=torch.channels_last)
            if shape[1] * shape[2] > 1:
                assert not cl.is_contiguous()
            assert torch.equal(render.image_u8(cl, rescale=rescale, mean=mean, std=std), got)     # channels-last: the same bits
    if shape[1] * shape[2] > 1:
        got = render.image_u8(img.to(DEV))
        per_image = got.reshape(shape[0], -1)
        assert (per_image.min(1).values == 0).all() and (per_image.max(1).values == 255).all()   # each image to its own range


@pytest.mark.parametrize("shape", [(3, 37, 53), (1, 2, 15), (1, 18, 523)], ids=lambda s: "x".join(map(str, s)))
def test_blend_against_float64(shape):
    cmap = render.cityscapes_colormap()
    lab = _labels(shape, 28, torch.int64, seed=8)
    img = _image(shape, 9, lo=-1.7, hi=2.0)             # un-normalised inside (0.02, 0.95): nothing clamps (module docstring)
    t, d = torch.from_numpy(lab).to(DEV), img.to(DEV)
    mean, std = render.IMAGENET_MEAN, render.IMAGENET_STD
    for edges in (False, True):
        rgb = np_colorize(lab, cmap, edges=edges)
        solid = render.colorize(t, cmap, edges=edges, edge_color=EDGE)
        assert np.array_equal(solid.cpu().numpy(), rgb)
        for rescale in (False, True):
            unit = np_unit64(img.numpy(), rescale, mean, std)
            for alpha in (0.0, 0.3, 1.0):
                a = float(np.float32(alpha))
                want = np_levels64((1.0 - a) * unit + a * (rgb.astype(np.float64) / 255.0))
                got = render.colorize(t, cmap, image=d, alpha=alpha, edges=edges, rescale=rescale, edge_color=EDGE)
                close_to_f64(got.cpu().numpy(), want, "blend %s alpha=%s edges=%s rescale=%s" % (shape, alpha, edges, rescale))
                if alpha == 0.0:
                    assert torch.equal(got, render.image_u8(d, rescale=rescale, mean=mean, std=std))
                if alpha == 1.0:
                    assert torch.equal(got, solid)


def test_strided_target_touches_only_its_panel():
    """A 37 x 53 panel inside a 45 x 200 sheet of sentinels at x = 0, 1, 2, 3, 5: the sheet's rows are 600 bytes, so the panel's rows
    start at every alignment modulo 4 (and at 8 different ones modulo 16); then two panels side by side through the image stride."""
    cmap = _cmap(27)
    lab = torch.from_numpy(_labels((2, 37, 53), 27, torch.int64, seed=10)).to(DEV)
    img = _image((2, 37, 53), 11).to(DEV)
    for kind in ("labels", "image", "overlay"):
        def draw(l, i, out=None):
            if kind == "labels":
                return render.colorize(l, cmap, edges=True, out=out)
            if kind == "image":
                return render.image_u8(i, out=out)
            return render.colorize(l, cmap, image=i, alpha=0.4, edges=True, out=out)
        want = draw(lab, img)
        for x in (0, 1, 2, 3, 5):
            sheet = torch.full((45, 200, 3), 0xA5, dtype=torch.uint8, device=DEV)
            view = sheet[4:41, x:x + 53]
            assert draw(lab[0], img[0], out=view) is view
            assert torch.equal(view, want[0]), (kind, x)
            mask = torch.ones(45, 200, dtype=torch.bool, device=DEV)
            mask[4:41, x:x + 53] = False
            assert (sheet[mask] == 0xA5).all(), (kind, x)
        for x in (1, 6):
            sheet = torch.full((45, 200, 3), 0xA5, dtype=torch.uint8, device=DEV)
            view = torch.as_strided(sheet, (2, 37, 53, 3), (61 * 3, 600, 3, 1), (3 * 200 + x) * 3)       # panels 61 pixels apart
            draw(lab, img, out=view)
            mask = torch.ones(45, 200, dtype=torch.bool, device=DEV)
            for b in range(2):
                assert torch.equal(sheet[3:40, x + 61 * b:x + 61 * b + 53], want[b]), (kind, x, b)
                mask[3:40, x + 61 * b:x + 61 * b + 53] = False
            assert (sheet[mask] == 0xA5).all(), (kind, x)


def test_wide_strided_target():
    """Rows wider than one chunk at an odd address and an odd row stride: pixels that straddle chunks, heads and tails."""
    cmap = _cmap(27)
    lab = torch.from_numpy(_labels((1, 18, 523), 27, torch.int32, seed=12)).to(torch.int32).to(DEV)
    want = render.colorize(lab, cmap, edges=True)
    buf = torch.full((20 * 1601 + 7,), 0x5A, dtype=torch.uint8, device=DEV)
    view = torch.as_strided(buf, (1, 18, 523, 3), (0, 1601, 3, 1), 1601 + 7)
    render.colorize(lab, cmap, edges=True, out=view)
    assert torch.equal(view, want)
    mask = torch.ones_like(buf, dtype=torch.bool)
    for y in range(18):
        mask[1601 * (y + 1) + 7:1601 * (y + 1) + 7 + 3 * 523] = False
    assert (buf[mask] == 0x5A).all()


def test_image_range_is_exact():
    for shape in ((1, 1, 1), (3, 37, 53), (2, 70, 130)):
        img = _image(shape, 13).to(DEV)
        for src in (img, img.contiguous(memory_format=torch.channels_last)):
            for mean, std in ((render.PLOT_MEAN, render.PLOT_STD), (render.IMAGENET_MEAN, render.IMAGENET_STD)):
                desc = capi.render_desc(*shape, flags=capi.RENDER_IMAGE, mean=mean, std=std)
                got = capi.image_range(desc, src)
                v = img.clone()
                for c in range(3):
                    v[:, c].mul_(std[c]).add_(mean[c])
                want = torch.stack([v.amin(dim=(1, 2, 3)), v.amax(dim=(1, 2, 3))], 1)
                assert torch.equal(got, want), shape


def test_constant_image_renders_as_zeros():
    img = torch.full((2, 3, 9, 20), 0.37, device=DEV)
    assert not render.image_u8(img, rescale=True).any()
    lab = torch.zeros(2, 9, 20, dtype=torch.int64, device=DEV)
    got = render.colorize(lab, np.array([[200, 100, 50]]), image=img, alpha=0.5, rescale=True, mean=render.PLOT_MEAN, std=render.PLOT_STD)
    want = np_levels64(0.5 * np.array([200, 100, 50]) / 255.0)
    assert np.array_equal(got.cpu().numpy(), np.broadcast_to(want, (2, 9, 20, 3)))


def test_repeat_launches_are_bitwise_equal():
    cmap = _cmap(27)
    lab = torch.from_numpy(_labels((3, 37, 53), 27, torch.int64, seed=14)).to(DEV)
    img = _image((3, 37, 53), 15).to(DEV)
    first = render.colorize(lab, cmap, image=img, alpha=0.3, edges=True, rescale=True)
    second = render.colorize(lab, cmap, image=img, alpha=0.3, edges=True, rescale=True)
    assert torch.equal(first, second)
    assert torch.equal(render.image_u8(img), render.image_u8(img))


def test_fallbacks_run_the_torch_chain():
    cmap = np.random.default_rng(16).integers(0, 256, (600, 3))                 # more colours than the kernel's table
    lab = torch.from_numpy(_labels((1, 9, 11), 600, torch.int64, seed=17)).to(DEV)
    assert np.array_equal(render.colorize(lab, cmap).cpu().numpy(), np_colorize(lab.cpu().numpy(), cmap))
    small = torch.from_numpy(_labels((1, 9, 11), 27, torch.int64, seed=18)).to(torch.int16).to(DEV)    # a dtype it does not read
    assert np.array_equal(render.colorize(small, _cmap(27)).cpu().numpy(), np_colorize(small.cpu().numpy().astype(np.int64), _cmap(27)))
    half = _image((1, 9, 11), 19).to(DEV).half()
    assert torch.equal(render.image_u8(half), render.torch_image_u8(half))


def test_comparison_sheet():
    cmap = render.cityscapes_colormap()
    lab = torch.from_numpy(_labels((3, 37, 53), 27, torch.int64, seed=20)).to(DEV)
    clu = torch.from_numpy(_labels((3, 37, 53), 7, torch.int64, seed=21)).to(DEV)
    mapping = np.array([3, -1, 0, 26, 5, 9, -1])
    img = _image((3, 37, 53), 22).to(DEV)
    rows = [{"image": img}, {"labels": lab, "cmap": cmap}, {"labels": clu, "cmap": cmap, "mapping": mapping},
            {"labels": clu[:2], "cmap": cmap, "mapping": mapping, "image": img[:2], "alpha": 0.6, "edges": True}]
    sheet = render.comparison_sheet(rows, pad=5, background=(10, 20, 30))
    assert tuple(sheet.shape) == (5 + 4 * 42, 5 + 3 * 58, 3) and sheet.dtype == torch.uint8 and sheet.is_cuda
    alone = [render.image_u8(img), render.colorize(lab, cmap), render.colorize(clu, cmap, mapping=mapping),
             render.colorize(clu[:2], cmap, mapping=mapping, image=img[:2], alpha=0.6, edges=True)]
    mask = torch.ones(sheet.shape[:2], dtype=torch.bool, device=DEV)
    for r, panels in enumerate(alone):
        for b in range(panels.shape[0]):
            y, x = 5 + 42 * r, 5 + 58 * b
            assert torch.equal(sheet[y:y + 37, x:x + 53], panels[b]), (r, b)
            mask[y:y + 37, x:x + 53] = False
    pad = sheet[mask]
    assert pad.shape[0] > 0 and (pad == torch.tensor([10, 20, 30], dtype=torch.uint8, device=DEV)).all()


# ---- end to end, on the tiny model of tests/test_demo_gpu.py
def _tiny_checkpoint(tmp_path, extra=2):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    mcfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=48", "dim=70", "dropout=False",
                                  "extra_clusters=%d" % extra])
    torch.manual_seed(1)
    model = LitUnsupervisedSegmenter(27, mcfg)
    ck = tmp_path / "tiny.ckpt"
    model.save_checkpoint(str(ck))
    return ck


@pytest.mark.parametrize("full_res", [False, True])
def test_demo_writes_colour_pictures(tmp_path, full_res):
    from stego_amd import demo_segmentation as D
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    ck = _tiny_checkpoint(tmp_path)
    d = tmp_path / "images"
    d.mkdir()
    rng = np.random.default_rng(2)
    sizes = {"wide": (60, 90), "tall": (100, 50)} if not full_res else {"large": (70, 101)}
    for name, (h, w) in sizes.items():
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / (name + ".png"))
    cfg = load_config(D.DEMO_CONFIG, overrides=["output_root=%s" % tmp_path, "model_path=%s" % ck, "image_dir=%s" % d,
                                                "experiment_name=t", "res=48", "batch_size=2", "num_workers=0", "run_crf=False",
                                                "save_color=True", "full_res=%s" % full_res])
    written = D.my_app(cfg)
    out = os.path.join(str(tmp_path), "results", "predictions", "t")
    assert written == [os.path.join(out, sub, s + ".png") for s in sorted(sizes) for sub in ("linear", "cluster")]
    cmap = LitUnsupervisedSegmenter.load_from_checkpoint(str(ck)).label_cmap
    for sub in ("linear", "cluster", "linear_color", "cluster_color", "overlay"):
        assert sorted(os.listdir(os.path.join(out, sub))) == sorted(s + ".png" for s in sizes), sub
    for s, (h, w) in sizes.items():
        size = (h, w) if full_res else (48, 48)
        for sub in ("linear", "cluster"):
            labels = np.asarray(Image.open(os.path.join(out, sub, s + ".png")))
            colour = Image.open(os.path.join(out, sub + "_color", s + ".png"))
            assert labels.shape == size and colour.mode == "RGB"
            assert np.array_equal(np.asarray(colour), cmap[labels].astype(np.uint8)), (sub, s)     # no stored assignment: identity
        overlay = Image.open(os.path.join(out, "overlay", s + ".png"))
        assert overlay.mode == "RGB" and np.asarray(overlay).shape == size + (3,)
        labels = np.asarray(Image.open(os.path.join(out, "cluster", s + ".png"))).astype(np.int64)
        edge = np_colorize(labels[None], cmap, edges=True)[0] != np_colorize(labels[None], cmap)[0]
        if edge.any():                                   # a boundary pixel: half white, so no channel below 127
            assert np.asarray(overlay)[edge.any(-1)].min() >= 127


def test_eval_writes_figures_and_keeps_its_metrics(tmp_path):
    from stego_amd import eval_segmentation as E
    from stego_amd.train_segmentation import load_config
    ck = _tiny_checkpoint(tmp_path)
    base = ["pytorch_data_dir=%s" % (tmp_path / "none"), "model_paths=[%s]" % ck, "res=48", "batch_size=2", "run_crf=False",
            "output_root=%s" % tmp_path]
    results = {}
    for native in (False, True):
        for figures in (False, True):
            cfg = load_config(E.EVAL_CONFIG, overrides=base + ["native_metrics=%s" % native, "save_figures=%s" % figures,
                                                               "experiment_name=e%d%d" % (native, figures)])
            results[native, figures] = {k: float(v) for k, v in E.my_app(cfg)[str(ck)].items()}
        assert results[native, True] == results[native, False]
        assert not os.path.exists(os.path.join(str(tmp_path), "results", "predictions", "e%d0" % native))
        out = os.path.join(str(tmp_path), "results", "predictions", "e%d1" % native)
        for sub, ext in (("img", ".jpg"), ("label", ".png"), ("linear", ".png"), ("cluster", ".png")):
            assert sorted(os.listdir(os.path.join(out, sub))) == sorted("%d%s" % (i, ext) for i in range(8)), sub
            assert Image.open(os.path.join(out, sub, "3" + ext)).size == (48, 48)
        assert [f for f in sorted(os.listdir(out)) if f.startswith("figure")] == ["figure_0.png"]
        sheet = Image.open(os.path.join(out, "figure_0.png"))
        assert sheet.mode == "RGB" and sheet.size == (4 + 8 * 52, 4 + 4 * 52)
        # the label row of the sheet is the label PNG, the cluster PNG holds only colours of classes (or the last colour for none)
        label3 = np.asarray(Image.open(os.path.join(out, "label", "3.png")))
        assert np.array_equal(np.asarray(sheet)[4 + 52:4 + 52 + 48, 4 + 3 * 52:4 + 3 * 52 + 48], label3)


def test_saved_data_and_cluster_mapping():
    """evaluate(keep=...) keeps the named images in loader order, and the cluster picture is label_cmap[map_clusters(preds)]."""
    from stego_amd import eval_segmentation as E
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    mcfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=48", "dim=70", "dropout=False", "extra_clusters=2"])
    torch.manual_seed(1)
    model = LitUnsupervisedSegmenter(27, mcfg).eval().to(DEV)
    ds = SyntheticContrastiveDataset(6, 48, 27, seed=0)
    loader = torch.utils.data.DataLoader(ds, 4, shuffle=False)
    E.evaluate(model, loader, run_crf=False, device=DEV, keep=[5, 1])
    data = model.saved_data
    assert data["index"] == [1, 5] and data["img"].is_cuda and tuple(data["img"].shape) == (2, 3, 48, 48)
    assert torch.equal(data["img"].cpu(), torch.stack([ds[1]["img"], ds[5]["img"]]))
    assert torch.equal(data["label"].cpu(), torch.stack([ds[1]["label"], ds[5]["label"]]))
    metrics = model.test_cluster_metrics
    vec = metrics.cluster_to_class()
    assert vec.shape == (29,) and (vec == -1).sum() == 2
    got = render.colorize(data["cluster_preds"], model.label_cmap, mapping=vec).cpu().numpy()
    mapped = metrics.map_clusters(data["cluster_preds"]).cpu().numpy()
    assert np.array_equal(got, model.label_cmap[mapped].astype(np.uint8))           # numpy wraps the -1 of an unmatched cluster
    assert np.array_equal(model.cluster_to_class, vec)
