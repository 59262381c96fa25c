"""cfg.train_log end to end on the GPU: six steps of the tiny model (vit_tiny/16, res 64, synthetic data) with the log on and six with it
off from the same seed give bit-identical losses; the event file holds the step's scalars and the cd histograms at their steps, and a
validation pass adds the metrics and the picture sheet."""
import glob
import io
import os
import warnings

import numpy as np
import pytest
import torch

from stego_amd import train_log as TL
from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, Trainer, load_config

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="DinoFeaturizer")

B, S, NEG, RES, STEPS = 3, 3, 2, 64, 6
TINY = ["model_type=vit_tiny", "dino_patch_size=16", "res=%d" % RES, "batch_size=%d" % B, "feature_samples=%d" % S,
        "neg_samples=%d" % NEG, "dim=6", "max_steps=%d" % STEPS, "scalar_log_freq=2", "hist_freq=2", "experiment_name=logtest",
        # the torch probe losses sum their 2-D NLL forward with float atomics: two runs of the SAME configuration differ by an ulp in
        # loss/linear now and then (measured with the log off both times).  The fused probe kernel adds in a fixed order, so that a
        # bit-for-bit comparison of two runs says something about the flag and not about ATen
        "native_probes=True"]


def _fit(root, train_log):
    cfg = load_config(overrides=TINY + ["train_log=%s" % train_log, "output_root=%s" % root])
    torch.manual_seed(0)
    model = LitUnsupervisedSegmenter(27, cfg)
    ds = SyntheticContrastiveDataset(12, RES, 27)
    loader = torch.utils.data.DataLoader(ds, B, shuffle=False, drop_last=True)
    trainer = Trainer(STEPS, device=torch.device("cuda"), log_every=100, val_loader=torch.utils.data.DataLoader(ds, B, shuffle=False))
    torch.manual_seed(1)
    losses = trainer.fit(model, loader)
    return cfg, model, trainer, losses


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_log")
    off = _fit(root / "off", False)
    on = _fit(root / "on", True)
    return root, off, on


def _events(model):
    model.train_log.writer.flush()
    return [e for e in TL.read_events(model.train_log.writer.path)]


def test_losses_are_bit_identical_with_and_without_the_log(runs):
    root, (_, m_off, _, l_off), (_, m_on, _, l_on) = runs
    assert len(l_on) == STEPS and np.isfinite(l_on).all()
    assert np.array_equal(np.array(l_on, np.float32).view(np.uint32), np.array(l_off, np.float32).view(np.uint32)), (l_on, l_off)
    assert m_off.train_log is None and not os.path.exists(str(root / "off" / "logs"))
    for p_on, p_off in zip(m_on.parameters(), m_off.parameters()):
        assert torch.equal(p_on, p_off)


def test_event_file_holds_the_steps_scalars(runs):
    root, _, (cfg, model, _, losses) = runs
    files = glob.glob(os.path.join(str(root / "on"), "logs", str(cfg.log_dir), "%s_logtest_date_*" % cfg.dataset_name, "events.out.tfevents.*"))
    assert files == [model.train_log.writer.path]
    ev = _events(model)
    assert ev[0][3] == "file_version" and ev[0][4] == "brain.Event:2"
    total = {e[0]: e[4] for e in ev if e[2] == "loss/total"}
    assert sorted(total) == [0, 2, 4]
    for s, v in total.items():
        assert np.float32(v).view(np.uint32) == np.float32(losses[s]).view(np.uint32), (s, v, losses[s])
    tags = {e[2] for e in ev if e[3] == "scalar" and e[0] in (0, 2, 4)}
    for tag in ("loss/pos_intra", "loss/pos_inter", "loss/neg_inter", "loss/linear", "loss/cluster", "loss/total", "cd/pos_intra",
                "cd/pos_inter", "cd/neg_inter") + (("loss/rec",) if cfg.rec_weight > 0 else ()):
        assert tag in tags, tag
        assert sorted(e[0] for e in ev if e[2] == tag) == [0, 2, 4], tag
    assert all(np.isfinite(e[4]) for e in ev if e[2].startswith("cd/"))
    assert isinstance(model.logged["cd/pos_intra"], float) and np.isfinite(model.logged["cd/pos_intra"])


def test_event_file_holds_the_cd_histograms(runs):
    _, _, (_, model, _, _) = runs
    hist = [e for e in _events(model) if e[3] == "histogram"]
    assert sorted((e[0], e[2]) for e in hist) == sorted((s, t) for s in (2, 4) for t in ("intra_cd", "inter_cd", "neg_cd"))
    for step, _, tag, _, h in hist:
        assert h["num"] == (NEG if tag == "neg_cd" else 1) * B * S ** 4, (step, tag, h["num"])
        assert h["bucket"].sum() == h["num"] and h["bucket"][0] == 0 and len(h["bucket"]) == len(h["bucket_limit"])
        assert h["min"] <= h["sum"] / h["num"] <= h["max"] and h["sum_squares"] >= h["sum"] ** 2 / h["num"] * (1 - 1e-12)
        assert h["bucket_limit"][0] <= h["min"] and h["max"] < h["bucket_limit"][-1]
    # the cd mean logged as a scalar is the histogram's sum / num
    cd = {(e[0], e[2]): e[4] for e in _events(model) if e[2].startswith("cd/")}
    for step, _, tag, _, h in hist:
        name = {"intra_cd": "cd/pos_intra", "inter_cd": "cd/pos_inter", "neg_cd": "cd/neg_inter"}[tag]
        assert np.float32(cd[(step, name)]) == np.float32(h["sum"] / h["num"])


def test_validation_adds_metrics_and_the_picture_sheet(runs):
    from PIL import Image
    _, _, (cfg, model, trainer, _) = runs
    before = len(_events(model))
    metrics = trainer._validate(model)
    ev = _events(model)[before:]
    scal = {e[2]: e[4] for e in ev if e[3] == "scalar"}
    assert set(metrics) == set(scal) and all(e[0] == STEPS for e in ev)
    for k, v in metrics.items():
        assert np.float32(scal[k]) == np.float32(v), k
    sheets = [e[4] for e in ev if e[3] == "image" and e[2] == "plot_labels"]
    assert len(sheets) == 1
    n = min(int(cfg.n_images), B)
    assert (sheets[0]["height"], sheets[0]["width"], sheets[0]["colorspace"]) == (4 + 4 * (RES + 4), 4 + n * (RES + 4), 3)
    png = np.asarray(Image.open(io.BytesIO(sheets[0]["encoded"])))
    assert png.shape == (4 + 4 * (RES + 4), 4 + n * (RES + 4), 3) and png.dtype == np.uint8
    assert (png[:4] == 255).all() and len(np.unique(png.reshape(-1, 3), axis=0)) > 10      # the white margin, and pictures inside it
