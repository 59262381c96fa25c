"""stego_amd.demo_segmentation end to end on the MI355X: a randomly initialised checkpoint over a folder of JPEG and PNG files of
different sizes and modes, one file that is not an image and one name with two dots -> exactly the expected label PNGs, each equal to
segment() on the same preprocessed batch."""
import os
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("run_crf", [True, False])
def test_demo_writes_every_prediction(tmp_path, capsys, run_crf):
    from stego_amd import demo_segmentation as D
    from stego_amd.data import image_transform
    from stego_amd.segment import segment
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
    Image.fromarray(rng.integers(0, 256, (60, 90, 3), dtype=np.uint8)).save(d / "wide.jpg")
    Image.fromarray(rng.integers(0, 256, (100, 50), dtype=np.uint8), "L").save(d / "tall_gray.png")
    Image.fromarray(rng.integers(0, 256, (48, 48, 4), dtype=np.uint8), "RGBA").save(d / "alpha.png")
    Image.fromarray(rng.integers(0, 256, (70, 64), dtype=np.uint8), "L").convert("P").save(d / "palette.png")
    Image.fromarray(rng.integers(0, 256, (52, 80, 3), dtype=np.uint8)).save(d / "two.dots.jpeg")
    (d / "notes.txt").write_text("not an image")

    cfg = load_config(D.DEMO_CONFIG, overrides=["output_root=%s" % tmp_path, "model_path=%s" % ck, "image_dir=%s" % d,
                                                "experiment_name=t", "res=%d" % res, "batch_size=2", "num_workers=0",
                                                "run_crf=%s" % run_crf])
    written = D.my_app(cfg)
    assert "notes.txt" in capsys.readouterr().out
    stems = ["alpha", "palette", "tall_gray", "two.dots", "wide"]
    out = os.path.join(str(tmp_path), "results", "predictions", "t")
    expect = [os.path.join(out, sub, s + ".png") for s in stems for sub in ("linear", "cluster")]
    assert written == expect
    for sub in ("linear", "cluster"):
        assert sorted(os.listdir(os.path.join(out, sub))) == sorted(s + ".png" for s in stems)

    loaded = LitUnsupervisedSegmenter.load_from_checkpoint(str(ck)).eval().to(DEV)
    tf = image_transform(res, "center")
    listing = sorted(os.listdir(d))                     # the demo's order, the unreadable file included
    assert listing == ["alpha.png", "notes.txt", "palette.png", "tall_gray.png", "two.dots.jpeg", "wide.jpg"]
    for lo in range(0, len(listing), 4):                # its batches of 2 * batch_size, from which the bad file then drops out
        names = [n for n in listing[lo:lo + 4] if n != "notes.txt"]
        img = torch.stack([tf(Image.open(d / n).convert("RGB")) for n in names])
        lin, clu = segment(loaded, img.to(DEV), run_crf=run_crf)
        for j, n in enumerate(names):
            stem = os.path.splitext(n)[0]
            for sub, pred, bound in (("linear", lin[j], 27), ("cluster", clu[j], 29)):
                png = Image.open(os.path.join(out, sub, stem + ".png"))
                arr = np.asarray(png)
                assert png.mode == "L" and arr.dtype == np.uint8 and arr.shape == (res, res)
                assert arr.max() < bound
                assert np.array_equal(arr, pred.cpu().numpy().astype(np.uint8)), (sub, n)
