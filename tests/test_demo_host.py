"""stego_amd.demo_segmentation without a GPU: the config's keys and defaults, the output layout and names, the sorted file order, the
skipping of files PIL cannot read, and the errors for a missing image_dir or model_path."""
import os
import types

import numpy as np
import pytest
from PIL import Image

from stego_amd import demo_segmentation as D
from stego_amd.data import image_transform
from stego_amd.train_segmentation import load_config


def test_config_keys_and_defaults():
    cfg = load_config(D.DEMO_CONFIG)
    for k in ("output_root", "model_path", "image_dir", "experiment_name", "res", "batch_size", "num_workers", "run_crf", "use_ddp"):
        assert hasattr(cfg, k), k
    assert (cfg.res, cfg.batch_size, cfg.run_crf, cfg.use_ddp) == (320, 8, True, False)
    cfg = load_config(D.DEMO_CONFIG, overrides=["run_crf=False", "res=224", "experiment_name=mine"])
    assert (cfg.run_crf, cfg.res, cfg.experiment_name) == (False, 224, "mine")


def test_output_paths_and_stems():
    cfg = types.SimpleNamespace(output_root="/out", experiment_name="exp")
    assert D.result_dir(cfg) == os.path.join("/out", "results", "predictions", "exp")
    assert D.prediction_name("a.jpg") == "a.png"
    assert D.prediction_name("photo.v2.JPEG") == "photo.v2.png"        # the reference's ".".join(split(".")[:-1])
    assert D.prediction_name("noext") == "noext.png"                   # (the reference would write ".png")


def _folder(tmp_path):
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)).save(d / "b.jpg")
    Image.fromarray(rng.integers(0, 256, (40, 30), dtype=np.uint8)).save(d / "a.png")
    Image.fromarray(rng.integers(0, 256, (33, 33, 4), dtype=np.uint8), "RGBA").save(d / "c.two.png")
    (d / "broken.jpg").write_bytes(b"not an image")
    (d / "sub").mkdir()
    return d


def test_folder_is_sorted_and_skips_unreadable_files(tmp_path):
    ds = D.UnlabeledImageFolder(str(_folder(tmp_path)), image_transform(16, "center"))
    assert ds.images == ["a.png", "b.jpg", "broken.jpg", "c.two.png"]
    items = [ds[i] for i in range(len(ds))]
    assert items[2][0] is None and items[2][1] == "broken.jpg"
    for img, name in items[:2] + items[3:]:
        assert tuple(img.shape) == (3, 16, 16), name
    imgs, names, bad = D.collate(items)
    assert tuple(imgs.shape) == (3, 3, 16, 16) and names == ["a.png", "b.jpg", "c.two.png"] and bad == ["broken.jpg"]
    assert D.collate([items[2]]) == (None, [], ["broken.jpg"])


def test_missing_inputs_raise(tmp_path):
    cfg = load_config(D.DEMO_CONFIG, overrides=["output_root=%s" % tmp_path, "model_path=%s" % (tmp_path / "none.ckpt"),
                                                "image_dir=%s" % _folder(tmp_path)])
    with pytest.raises(FileNotFoundError, match="model_path"):
        D.my_app(cfg)
    ck = tmp_path / "m.ckpt"
    ck.write_bytes(b"")
    cfg.model_path, cfg.image_dir = str(ck), str(tmp_path / "nowhere")
    with pytest.raises(FileNotFoundError, match="image_dir"):
        D.my_app(cfg)
    cfg.use_ddp = True
    with pytest.raises(NotImplementedError):
        D.my_app(cfg)
