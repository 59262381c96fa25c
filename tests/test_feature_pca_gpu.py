"""Feature pictures on the MI355X (csrc/feature_pca.hip) against the float64 oracle of tests/feature_pca_oracle.py: moments, basis,
statistics and scores under the project's 1e-3 fp32-relative contract, the residual of the device's eigen step, degenerate maps, a
fixed model, the bytes under the byte rule, a panel of a larger sheet, repeatability and the demo.

The byte cases use eight 5 x 7 images fitted jointly: in "range" mode the two extreme tokens of every component sit exactly at 0 and
255, where the last bit decides the byte, and only among 8 * 35 tokens are they under 1 % of a nearest-neighbour picture.  Seed 6 is
one at which the share of bytes within 1e-3 of an integer level is 0.73 % at the most over all 24 combinations (asserted)."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch
from conftest import assert_close
from PIL import Image

import feature_pca_oracle as O
from stego_amd import feature_pca, render

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = {
    "b2_5x7_c70": (2, 5, 7, 70, False, "cl"),
    "b3_6x6_c33_joint": (3, 6, 6, 33, True, "cl"),
    "b2_24x24_c33_joint": (2, 24, 24, 33, True, "cl"),          # 1152 tokens: crosses the 1024-token fold
    "b1_5x7_c768": (1, 5, 7, 768, False, "cl"),
    "b2_7x7_c384_cl": (2, 7, 7, 384, False, "cl"),
    "b2_7x7_c384_nchw": (2, 7, 7, 384, False, "nchw"),
    "b1_2x2_c3": (1, 2, 2, 3, False, "cl"),
    "b2_5x7_c70_offset": (2, 5, 7, 70, False, "cl"),            # an offset of 100 spreads: what an uncentred accumulation loses
}
SIZES = [(40, 56), (37, 53), (18, 523), (5, 17), (1, 1), None]


def _device_map(cl, layout="cl"):
    """channels-last numpy [B, h, w, C] -> a [B, C, h, w] device tensor: the channels-last view, or NCHW-contiguous."""
    t = torch.from_numpy(cl).to(DEV).permute(0, 3, 1, 2)
    return t.contiguous() if layout == "nchw" else t


@functools.lru_cache(maxsize=None)
def _case(name):
    B, h, w, C, joint, layout = CASES[name]
    cl = O.planted_map(B, h, w, C, joint, seed=len(name), offset=100.0 if name.endswith("offset") else 0.5)
    x = np.ascontiguousarray(cl.transpose(0, 3, 1, 2))
    return cl, x, O.fit(x, joint), joint, layout


@functools.lru_cache(maxsize=None)
def _byte_case(scale):
    cl = O.planted_map(8, 5, 7, 70, True, seed=6, gain=0.125 if scale == "unit" else 1.0)
    return cl, np.ascontiguousarray(cl.transpose(0, 3, 1, 2))


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_and_scores_against_the_oracle(name):
    cl, x, (mean, cov, basis, stats), joint, layout = _case(name)
    maps = _device_map(cl, layout)
    pca = feature_pca.fit(maps, joint=joint)
    got = {"mean": pca.mean.cpu().numpy(), "cov": pca.cov.cpu().numpy(), "basis": pca.basis.cpu().numpy(),
           "stats": pca.stats.cpu().numpy()}
    ref = feature_pca.torch_fit(torch.from_numpy(x), joint)                          # the torch fp32 chain, for the figures
    print(name, "mean %.2e" % np.abs(got["mean"] - mean).max(),
          "cov %.2e (torch %.2e)" % (np.abs(got["cov"] - cov).max(), np.abs(ref.cov.numpy() - cov).max()),
          "basis %.2e (torch %.2e)" % (np.abs(got["basis"] - basis).max(), np.abs(ref.basis.numpy() - basis).max()),
          "lambda %.2e" % np.abs(got["stats"][..., 0] - stats[..., 0]).max(), "residual %.2e" % got["stats"][..., 2].max())
    assert_close(got["mean"], mean, what=name + " mean")
    assert_close(got["cov"], cov, what=name + " cov")
    assert_close(got["basis"], basis, what=name + " basis")
    assert_close(got["stats"][..., :2], stats[..., :2], what=name + " stats")
    assert np.abs(got["cov"] - got["cov"].transpose(0, 2, 1)).max() == 0
    assert (got["stats"][..., 2] <= 1e-9).all(), got["stats"][..., 2]
    s, rng = O.scores(x, got["mean"], got["basis"])                                  # the oracle under the device's model
    dev_s = pca.scores(maps).cpu().numpy()
    full, _ = O.scores(x, mean, basis)
    ts = feature_pca._torch_scores(ref, torch.from_numpy(x))[0].numpy()
    print(name, "scores %.2e (torch %.2e)" % (np.abs(dev_s - full).max(), np.abs(ts - full).max()))
    assert_close(dev_s, s, what=name + " scores under the device's model")
    assert_close(dev_s, full, what=name + " scores")


def test_degenerate_maps():
    const = torch.full((2, 5, 3, 4), 0.7, device=DEV)
    pca = feature_pca.fit(const)
    assert not pca.basis.any() and not pca.stats.any() and not pca.cov.any()
    assert (feature_pca.feature_pictures(const, (9, 9)) == 127).all()
    rank2 = _device_map(O.planted_map(1, 5, 7, 33, False, seed=4, rank=2, gain=0.125))
    pca = feature_pca.fit(rank2)
    assert pca.basis[0, :2].abs().sum() > 0 and not pca.basis[0, 2].any() and not pca.stats[0, 2].any()
    pic = feature_pca.feature_pictures(rank2, (9, 9))
    assert (pic[..., 2] == 127).all() and (pic[..., :2] != 127).any()


def test_fixed_model():
    cl, x, _, _, _ = _case("b3_6x6_c33_joint")
    pca = feature_pca.fit(_device_map(cl), joint=True)
    other = O.planted_map(2, 5, 7, 33, True, seed=5)
    ox = np.ascontiguousarray(other.transpose(0, 3, 1, 2))
    model = (pca.mean.cpu().numpy(), pca.basis.cpu().numpy())
    s, rng = O.scores(ox, *model)
    assert_close(pca.scores(_device_map(other)).cpu().numpy(), s, what="scores under a fixed model")
    for scale in ("unit", "range"):
        _, a = O.pictures(ox, True, (20, 28), scale, "bilinear", model=model)
        got = feature_pca.feature_pictures(_device_map(other), (20, 28), scale=scale, pca=pca)
        O.byte_rule(got.cpu().numpy(), a)
    with pytest.raises(ValueError, match="per-image model"):
        feature_pca.feature_pictures(_device_map(other), pca=feature_pca.fit(_device_map(cl)))


@pytest.mark.parametrize("scale", ["unit", "range"])
@pytest.mark.parametrize("resize", ["bilinear", "nearest"])
@pytest.mark.parametrize("size", SIZES)
def test_bytes_against_the_oracle(scale, resize, size):
    cl, x = _byte_case(scale)
    _, a = O.pictures(x, True, size, scale, resize)
    got = feature_pca.feature_pictures(_device_map(cl), size, joint=True, scale=scale, resize=resize)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == a.shape
    share = O.byte_rule(got.cpu().numpy(), a)
    print(scale, resize, size, "exempt %.4f" % share)
    assert share <= 0.01, share
    if scale == "unit" and size != (1, 1):
        assert ((a < 0) | (a > 255)).any()                                           # the clamp is exercised


def test_minimum_map_bytes():
    """(1, 2, 2, 3): the replicated corners put an eighth of the pixels at 0 or 255 - the one-level rule only."""
    cl, x, _, joint, _ = _case("b1_2x2_c3")
    for scale in ("unit", "range"):
        for resize in ("bilinear", "nearest"):
            _, a = O.pictures(x, joint, (16, 16), scale, resize)
            got = feature_pca.feature_pictures(_device_map(cl), (16, 16), scale=scale, resize=resize)
            O.byte_rule(got.cpu().numpy(), a, strict=False)


def test_panel_of_a_larger_sheet():
    cl, _ = _byte_case("range")
    maps = _device_map(cl)[:3]
    H, W = 18, 37
    alone = feature_pca.feature_pictures(maps, (H, W), joint=True, scale="range")
    row, img, off = 3 * W + 23, 18 * (3 * W + 23) + 101, 7                           # strides that are no multiples of 16, an odd offset
    flat = torch.full((off + 3 * img + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    view = torch.as_strided(flat, (3, H, W, 3), (img, row, 3, 1), off)
    assert feature_pca.feature_pictures(maps, (H, W), joint=True, scale="range", out=view) is view
    assert torch.equal(view, alone)
    mask = torch.ones_like(flat, dtype=torch.bool)
    torch.as_strided(mask, (3, H, W, 3), (img, row, 3, 1), off)[:] = False
    assert (flat[mask] == 0xA5).all()
    sheet = render.comparison_sheet([{"features": maps, "size": (H, W), "joint": True, "scale": "range"}], pad=3, background=(9, 9, 9))
    for b in range(3):
        assert torch.equal(sheet[3:3 + H, 3 + b * (W + 3):3 + b * (W + 3) + W], alone[b])


def test_repeat_calls_are_bitwise_equal():
    cl, _, _, joint, _ = _case("b2_24x24_c33_joint")
    maps = _device_map(cl)
    runs = []
    for _ in range(2):
        pca = feature_pca.fit(maps, joint=joint)
        runs.append((pca.mean, pca.cov, pca.basis, pca.stats, pca.scores(maps),
                     feature_pictures_range(maps, pca)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def feature_pictures_range(maps, pca):
    return feature_pca.feature_pictures(maps, (50, 61), scale="range", pca=pca)


def test_demo_writes_both_feature_pictures(tmp_path):
    from stego_amd import demo_segmentation as D
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    res = 48
    mcfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=%d" % res, "dim=70", "dropout=False",
                                  "extra_clusters=2"])
    torch.manual_seed(1)
    model = LitUnsupervisedSegmenter(27, mcfg)
    ck = tmp_path / "demo.ckpt"
    model.save_checkpoint(str(ck))
    d = tmp_path / "images"
    d.mkdir()
    rng = np.random.default_rng(2)
    for stem, shape in (("a", (60, 90, 3)), ("b", (52, 80, 3)), ("c", (48, 48, 3))):
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(d / (stem + ".png"))
    outs = {}
    for key in ("plain", "pca"):
        cfg = load_config(D.DEMO_CONFIG, overrides=["output_root=%s" % (tmp_path / key), "model_path=%s" % ck, "image_dir=%s" % d,
                                                    "experiment_name=t", "res=%d" % res, "batch_size=1", "num_workers=0",
                                                    "run_crf=False"] + (["save_pca=True"] if key == "pca" else []))
        D.my_app(cfg)
        outs[key] = os.path.join(str(tmp_path / key), "results", "predictions", "t")
    assert sorted(os.listdir(outs["plain"])) == ["cluster", "linear"]
    assert sorted(os.listdir(outs["pca"])) == ["cluster", "linear", "pca_code", "pca_feats"]
    for sub in ("linear", "cluster"):
        for stem in "abc":
            with open(os.path.join(outs["plain"], sub, stem + ".png"), "rb") as f, open(os.path.join(outs["pca"], sub, stem + ".png"), "rb") as g:
                assert f.read() == g.read(), (sub, stem)
    for sub in ("pca_feats", "pca_code"):
        assert sorted(os.listdir(os.path.join(outs["pca"], sub))) == ["a.png", "b.png", "c.png"]
        for stem in "abc":
            png = Image.open(os.path.join(outs["pca"], sub, stem + ".png"))
            label = Image.open(os.path.join(outs["pca"], "linear", stem + ".png"))
            assert png.mode == "RGB" and png.size == label.size == (res, res)
            assert np.asarray(png).std() > 0
