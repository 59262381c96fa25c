"""The training log without a GPU (stego_amd.train_log): CRC-32C, the event-file framing and the hand-written protocol-buffer messages
through read_events, the histogram trimming against a restatement of torch.utils.tensorboard.summary.make_histogram, and TrainLog's
directory name and rank rule."""
import datetime
import io
import os
import types

import numpy as np
import pytest

from stego_amd import train_log as TL


def test_crc32c_known_answers():
    assert TL.crc32c(b"123456789") == 0xE3069283
    assert TL.crc32c(bytes(32)) == 0x8A9136AA
    assert TL.crc32c(b"") == 0
    crc = TL.crc32c(b"123456789")
    assert TL.masked_crc32c(b"123456789") == (((crc >> 15) | (crc << 17)) + 0xA282EAD8) % 2 ** 32


def _write(tmp_path):
    w = TL.EventWriter(str(tmp_path / "log"))
    w.add_scalar("loss/total", 1.25, 0, wall_time=100.5)
    w.add_scalar("loss/total", float(np.float32(-0.1)), 7)
    w.add_scalar("cd/nan", float("nan"), 2 ** 40 + 3)
    limits, counts = [-0.5, 0.0, 0.25, 1e20], [0.0, 3.0, 2.0, 7.0]
    w.add_histogram_raw("intra_cd", min=-0.25, max=0.75, num=12, sum=3.5, sum_squares=2.125, bucket_limits=limits, bucket_counts=counts,
                        step=100, wall_time=200.25)
    img = (np.arange(5 * 7 * 3) % 251).astype(np.uint8).reshape(5, 7, 3)
    w.add_image("plot_labels", img, 100)
    w.add_image("gray", img[:, :, 0], 101)
    w.close()
    w.close()
    return w.path, limits, counts, img


def test_event_file_reads_back(tmp_path):
    from PIL import Image
    path, limits, counts, img = _write(tmp_path)
    name = os.path.basename(path).split(".")
    assert name[:3] == ["events", "out", "tfevents"] and name[3].isdigit() and name[-1] == "0" and name[-2] == str(os.getpid())
    ev = list(TL.read_events(path))
    assert [e[3] for e in ev] == ["file_version", "scalar", "scalar", "scalar", "histogram", "image", "image"]
    assert ev[0][4] == "brain.Event:2" and ev[0][0] == 0 and ev[0][1] > 1e9
    assert ev[1][:4] == (0, 100.5, "loss/total", "scalar") and ev[1][4] == 1.25
    assert ev[2][0] == 7 and np.float32(ev[2][4]) == np.float32(-0.1) and ev[2][1] > 1e9
    assert ev[3][0] == 2 ** 40 + 3 and ev[3][2] == "cd/nan" and np.isnan(ev[3][4])
    step, wall, tag, _, h = ev[4]
    assert (step, wall, tag) == (100, 200.25, "intra_cd")
    assert (h["min"], h["max"], h["num"], h["sum"], h["sum_squares"]) == (-0.25, 0.75, 12.0, 3.5, 2.125)
    assert h["bucket_limit"].tolist() == limits and h["bucket"].tolist() == counts
    step, _, tag, _, im = ev[5]
    assert (step, tag, im["height"], im["width"], im["colorspace"]) == (100, "plot_labels", 5, 7, 3)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(im["encoded"]))), img)
    assert ev[6][4]["colorspace"] == 1 and np.array_equal(np.asarray(Image.open(io.BytesIO(ev[6][4]["encoded"]))), img[:, :, 0])


def test_a_flipped_byte_is_noticed(tmp_path):
    path = _write(tmp_path)[0]
    data = bytearray(open(path, "rb").read())
    first = 8 + 4 + int.from_bytes(data[:8], "little") + 4          # start of the second record
    for at in (first + 2, first + 9, first + 14, len(data) - 2, len(data) - 40):
        bad = bytearray(data)
        bad[at] ^= 0x10
        broken = str(tmp_path / ("bad%d" % at))
        open(broken, "wb").write(bad)
        with pytest.raises(ValueError, match="event file"):
            list(TL.read_events(broken))
    open(str(tmp_path / "short"), "wb").write(data[:-3])
    with pytest.raises(ValueError, match="truncated"):
        list(TL.read_events(str(tmp_path / "short")))


def _make_histogram_trim(values, bins):
    """torch/utils/tensorboard/summary.py make_histogram's trimming (max_bins=None), restated."""
    counts, limits = np.histogram(values, bins=bins)
    cum_counts = np.cumsum(np.greater(counts, 0))
    start, end = np.searchsorted(cum_counts, [0, cum_counts[-1] - 1], side="right")
    start, end = int(start), int(end) + 1
    counts = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
    limits = limits[start:end + 1]
    return limits.tolist(), counts.tolist()


def _bins():
    v, pos = 1e-12, []
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.array([-x for x in pos[::-1]] + [0] + pos)


@pytest.mark.parametrize("values", [
    (0.3 * np.random.default_rng(0).standard_normal(5000)).astype(np.float32),          # support in the middle
    np.array([-9.5e19, -1.0, 0.5, 0.5, 2.0], np.float32),                                 # ... touching bucket 0
    np.array([9.5e19, 1.0], np.float32),                                                  # ... touching the last bucket
    np.full(100, 0.25, np.float32),                                                       # a single bucket
    np.array([-9.5e19] * 3, np.float32),                                                  # a single bucket, the first
], ids=["middle", "bucket0", "last", "single", "single0"])
def test_histogram_fields_equal_make_histograms_trimming(values):
    bins = _bins()
    counts = np.histogram(values, bins=bins)[0].astype(np.uint32)
    v64 = values.astype(np.float64)
    rec = {"step": 3, "tensors": [None, dict(counts=counts, n_finite=len(values), min=values.min(), max=values.max(), sum=v64.sum(),
                                              sum_sq=(v64 * v64).sum())]}
    f = TL.histogram_fields(rec, 1, bins)
    limits, kept = _make_histogram_trim(values, bins)
    assert f["bucket_limits"] == limits and f["bucket_counts"] == [float(c) for c in kept]
    assert len(f["bucket_limits"]) == len(f["bucket_counts"]) and f["bucket_counts"][0] == 0
    assert f["num"] == len(values) and f["min"] == float(values.min()) and f["max"] == float(values.max())
    assert f["sum"] == v64.sum() and f["sum_squares"] == (v64 * v64).sum()


def test_an_empty_histogram_is_refused():
    rec = {"step": 3, "tensors": [dict(counts=np.zeros(1548, np.uint32), n_finite=0, min=np.inf, max=-np.inf, sum=0.0, sum_sq=0.0)]}
    with pytest.raises(ValueError, match="empty"):
        TL.histogram_fields(rec, 0, _bins())
    rec["tensors"][0]["counts"] = None
    with pytest.raises(ValueError, match="no bucket counts"):
        TL.histogram_fields(rec, 0, _bins())


def test_tensorboard_reads_the_file(tmp_path):
    loader = pytest.importorskip("tensorboard.backend.event_processing.event_file_loader")
    path, limits, counts, _ = _write(tmp_path)
    events = list(loader.EventFileLoader(path).Load())
    assert events[0].file_version == "brain.Event:2"
    assert events[1].summary.value[0].tag == "loss/total" and events[1].step == 0


def _cfg(root):
    return types.SimpleNamespace(output_root=str(root), log_dir="potsdam", dataset_name="potsdam", experiment_name="exp1", scalar_log_freq=2,
                                 hist_freq=4)


def test_log_directory_has_the_references_form(tmp_path):
    now = datetime.datetime(2024, 3, 9, 14, 5, 59)
    assert TL.log_dir_name(_cfg(tmp_path), now) == os.path.join(str(tmp_path), "logs", "potsdam", "potsdam_exp1_date_Mar09_14-05-59")
    log = TL.TrainLog(_cfg(tmp_path), 0, now)
    assert log.dir == TL.log_dir_name(_cfg(tmp_path), now) and os.path.dirname(log.writer.path) == log.dir
    assert [f for f in os.listdir(log.dir) if f.startswith("events.out.tfevents.")]
    log.close()


def test_rank_1_writes_nothing(tmp_path):
    log = TL.TrainLog(_cfg(tmp_path), 1)
    assert log.writer is None and log.dir is None
    rec = dict(step=0, with_hist=False, scalars=np.ones(1, np.float32), tensors=[dict(mean=0.5, counts=None)] * 3)
    log.consume([rec], ["loss/total"])
    log.scalars({"a": 1.0}, 3)
    log.image("x", np.zeros((2, 2, 3), np.uint8), 3)
    log.close()
    assert not os.path.exists(str(tmp_path / "logs"))
    assert log.wants_hist(4) and not log.wants_hist(0) and not log.wants_hist(6)      # the condition itself holds on every rank


def test_consume_writes_scalars_and_histograms_at_their_steps(tmp_path):
    log = TL.TrainLog(_cfg(tmp_path), 0)
    bins = _bins()
    vals = [np.full(10, 0.25, np.float32), np.full(10, -0.5, np.float32), np.zeros(0, np.float32)]

    def tensor(v, hist):
        v64 = v.astype(np.float64)
        return dict(counts=np.histogram(v, bins=bins)[0].astype(np.uint32) if hist else None, n_finite=len(v), n_nan=0, n_out=0,
                    min=v.min() if len(v) else np.float32(np.inf), max=v.max() if len(v) else np.float32(-np.inf), sum=v64.sum(),
                    sum_sq=(v64 * v64).sum(), mean=v64.mean() if len(v) else float("nan"))

    recs = [dict(step=s, with_hist=s in (4, 8), scalars=np.array([s + 0.5, -s], np.float32), tensors=[tensor(v, s in (4, 8)) for v in vals])
            for s in range(9)]
    log.consume(recs, ["loss/total", "loss/rec"])
    log.close()
    ev = [e for e in TL.read_events(log.writer.path) if e[3] != "file_version"]
    scal = [(e[0], e[2], e[4]) for e in ev if e[3] == "scalar"]
    assert [s for s, t, _ in scal if t == "loss/total"] == [0, 2, 4, 6, 8]
    assert (4, "loss/total", 4.5) in scal and (4, "loss/rec", -4.0) in scal and (6, "cd/pos_intra", 0.25) in scal and (6, "cd/pos_inter", -0.5) in scal
    hist = [(e[0], e[2]) for e in ev if e[3] == "histogram"]
    assert hist == [(4, "intra_cd"), (4, "inter_cd"), (8, "intra_cd"), (8, "inter_cd")]         # the empty neg tensor draws nothing
    h = [e[4] for e in ev if e[3] == "histogram"][0]
    assert h["num"] == 10 and h["bucket"].tolist() == [0.0, 10.0] and h["bucket_limit"][0] <= 0.25 < h["bucket_limit"][1]
