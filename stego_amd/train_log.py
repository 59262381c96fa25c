"""The training log: TensorBoard event files written by hand, and ``TrainLog``, which turns the records of
``stego_amd.step_stats.StepStats`` into the scalars and histograms the reference's ``training_step`` logs
(train_segmentation.py:144-146, 165-177) and writes what its ``validation_epoch_end`` writes (:277-330).

Neither ``tensorboard`` nor ``tensorboardX`` is needed: an event file is a sequence of framed records

    uint64 length (little endian) | masked CRC-32C of those 8 bytes | payload | masked CRC-32C of the payload

whose payload is an ``Event`` protocol buffer, and the handful of messages a scalar, a histogram and an image need are written here in
wire format (field numbers from tensorflow/core/util/event.proto, framework/summary.proto).  ``read_events`` is the inverse, for users
without TensorBoard and for the tests.  No file of this writer has been opened with TensorBoard itself where this was developed
(the package was not installed): the format follows the published .proto files and torch.utils.tensorboard's use of them.
"""
import io
import os
import socket
import struct
import time

import numpy as np

# ---- CRC-32C (Castagnoli), table driven, and TensorFlow's mask
_CRC_TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0x82F63B78 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)
_CRC_TABLE = tuple(_CRC_TABLE)


def crc32c(data):
    crc = 0xFFFFFFFF
    table = _CRC_TABLE
    for b in bytes(data):
        crc = table[(crc ^ b) & 0xFF] ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


def masked_crc32c(data):
    crc = crc32c(data)
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


# ---- protocol-buffer wire format: the few encoders and the decoder the messages below need
def _varint(n):
    n &= (1 << 64) - 1                 # int64 fields: negative values as 10-byte two's complement
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def _key(field, wire):
    return _varint((field << 3) | wire)


def _f_double(field, v):
    return _key(field, 1) + struct.pack("<d", float(v))


def _f_float(field, v):
    return _key(field, 5) + struct.pack("<f", float(v))


def _f_varint(field, v):
    return _key(field, 0) + _varint(int(v))


def _f_bytes(field, data):
    data = data.encode("utf-8") if isinstance(data, str) else bytes(data)
    return _key(field, 2) + _varint(len(data)) + data


def _f_packed_doubles(field, values):
    return _f_bytes(field, np.asarray(values, dtype="<f8").tobytes())


def _parse(buf):
    """One message -> a list of (field, wire type, value): ints for varints, bytes for the other kinds."""
    out, i, n = [], 0, len(buf)
    while i < n:
        key, shift = 0, 0
        while True:
            b = buf[i]
            i += 1
            key |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        field, wire = key >> 3, key & 7
        if wire == 0:
            v, shift = 0, 0
            while True:
                b = buf[i]
                i += 1
                v |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    break
        elif wire == 1:
            v, i = bytes(buf[i:i + 8]), i + 8
        elif wire == 5:
            v, i = bytes(buf[i:i + 4]), i + 4
        elif wire == 2:
            ln, shift = 0, 0
            while True:
                b = buf[i]
                i += 1
                ln |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    break
            v, i = bytes(buf[i:i + ln]), i + ln
        else:
            raise ValueError("event file: unsupported wire type %d" % wire)
        if i > n:
            raise ValueError("event file: a field runs past the end of its message")
        out.append((field, wire, v))
    return out


class EventWriter:
    """``EventWriter(logdir)`` creates ``events.out.tfevents.{time}.{host}.{pid}.0`` in `logdir` and writes the version record."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s.%d.0" % (int(time.time()), socket.gethostname(), os.getpid()))
        self._f = open(self.path, "wb")
        self._write_event(_f_double(1, time.time()) + _f_bytes(3, "brain.Event:2"))
        self.flush()

    def _write_event(self, payload):
        header = struct.pack("<Q", len(payload))
        self._f.write(header + struct.pack("<I", masked_crc32c(header)) + payload + struct.pack("<I", masked_crc32c(payload)))

    def _write_value(self, tag, value_field, step, wall_time):
        value = _f_bytes(1, tag) + value_field
        summary = _f_bytes(1, value)                                   # Summary.value (repeated) = 1
        wall_time = time.time() if wall_time is None else wall_time
        self._write_event(_f_double(1, wall_time) + _f_varint(2, step) + _f_bytes(5, summary))

    def add_scalar(self, tag, value, step, wall_time=None):
        self._write_value(tag, _f_float(2, value), step, wall_time)

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, step, wall_time=None):
        if len(bucket_limits) != len(bucket_counts):
            raise ValueError("add_histogram_raw: %d limits for %d counts" % (len(bucket_limits), len(bucket_counts)))
        histo = _f_double(1, min) + _f_double(2, max) + _f_double(3, num) + _f_double(4, sum) + _f_double(5, sum_squares) + \
            _f_packed_doubles(6, bucket_limits) + _f_packed_doubles(7, bucket_counts)
        self._write_value(tag, _f_bytes(5, histo), step, wall_time)

    def add_image(self, tag, image, step, wall_time=None):
        """`image`: uint8 [H, W, 3] or [H, W] (numpy array or tensor), stored as PNG."""
        from PIL import Image
        arr = np.ascontiguousarray(image.cpu().numpy() if hasattr(image, "cpu") else image)
        if arr.dtype != np.uint8 or arr.ndim not in (2, 3) or (arr.ndim == 3 and arr.shape[2] not in (1, 3, 4)):
            raise ValueError("add_image expects uint8 [H, W] or [H, W, 1 | 3 | 4], got %s %s" % (arr.dtype, arr.shape))
        if arr.ndim == 3 and arr.shape[2] == 1:
            arr = arr[:, :, 0]
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="PNG")
        colorspace = 1 if arr.ndim == 2 else arr.shape[2]
        img = _f_varint(1, arr.shape[0]) + _f_varint(2, arr.shape[1]) + _f_varint(3, colorspace) + _f_bytes(4, buf.getvalue())
        self._write_value(tag, _f_bytes(4, img), step, wall_time)

    def flush(self):
        self._f.flush()

    def close(self):
        if not self._f.closed:
            self._f.flush()
            self._f.close()


def _doubles(raw):
    return np.frombuffer(raw, dtype="<f8").copy()


def read_events(path):
    """Yields ``(step, wall_time, tag, kind, value)`` for every value of every record of an event file, checking both CRCs of every
    record (ValueError on a mismatch or a truncated record).  kind / value: "file_version" / str; "scalar" / float; "histogram" / dict
    with min, max, num, sum, sum_squares, bucket_limit, bucket; "image" / dict with height, width, colorspace, encoded (PNG bytes)."""
    with open(path, "rb") as f:
        data = f.read()
    i = 0
    while i < len(data):
        if i + 12 > len(data):
            raise ValueError("event file: truncated record header at byte %d" % i)
        header = data[i:i + 8]
        if struct.unpack("<I", data[i + 8:i + 12])[0] != masked_crc32c(header):
            raise ValueError("event file: the length CRC of the record at byte %d does not match" % i)
        n = struct.unpack("<Q", header)[0]
        if i + 12 + n + 4 > len(data):
            raise ValueError("event file: truncated record at byte %d" % i)
        payload = data[i + 12:i + 12 + n]
        if struct.unpack("<I", data[i + 12 + n:i + 16 + n])[0] != masked_crc32c(payload):
            raise ValueError("event file: the payload CRC of the record at byte %d does not match" % i)
        i += 16 + n
        step, wall_time, version, summary = 0, 0.0, None, None
        for field, wire, v in _parse(payload):
            if field == 1 and wire == 1:
                wall_time = struct.unpack("<d", v)[0]
            elif field == 2 and wire == 0:
                step = v - (1 << 64) if v >> 63 else v
            elif field == 3 and wire == 2:
                version = v.decode("utf-8")
            elif field == 5 and wire == 2:
                summary = v
        if version is not None:
            yield step, wall_time, "", "file_version", version
        if summary is None:
            continue
        for field, wire, value in _parse(summary):
            if field != 1 or wire != 2:
                continue
            tag, kind, out = "", None, None
            for vf, vw, vv in _parse(value):
                if vf == 1 and vw == 2:
                    tag = vv.decode("utf-8")
                elif vf == 2 and vw == 5:
                    kind, out = "scalar", struct.unpack("<f", vv)[0]
                elif vf == 4 and vw == 2:
                    img = {"height": 0, "width": 0, "colorspace": 0, "encoded": b""}
                    for f4, w4, v4 in _parse(vv):
                        if w4 == 0 and f4 in (1, 2, 3):
                            img[("height", "width", "colorspace")[f4 - 1]] = v4
                        elif f4 == 4 and w4 == 2:
                            img["encoded"] = v4
                    kind, out = "image", img
                elif vf == 5 and vw == 2:
                    h = {"bucket_limit": np.zeros(0), "bucket": np.zeros(0)}
                    names = ("min", "max", "num", "sum", "sum_squares")
                    for f5, w5, v5 in _parse(vv):
                        if w5 == 1 and 1 <= f5 <= 5:
                            h[names[f5 - 1]] = struct.unpack("<d", v5)[0]
                        elif w5 == 2 and f5 == 6:
                            h["bucket_limit"] = _doubles(v5)
                        elif w5 == 2 and f5 == 7:
                            h["bucket"] = _doubles(v5)
                    kind, out = "histogram", h
            if kind is not None:
                yield step, wall_time, tag, kind, out


def trim_histogram(counts, limits):
    """The trimmed (bucket_limit, bucket) lists of torch.utils.tensorboard.summary.make_histogram for np.histogram's `counts` over
    `limits`: from the first to the last occupied bucket, with one empty bucket on the left (TensorBoard stores right limits only)."""
    counts = np.asarray(counts)
    limits = np.asarray(limits, np.float64)
    if counts.ndim != 1 or limits.shape != (counts.size + 1,):
        raise ValueError("trim_histogram: %s counts for %s limits" % (counts.shape, limits.shape))
    occupied = np.nonzero(counts > 0)[0]
    if occupied.size == 0:
        raise ValueError("The histogram is empty: no value lies inside the buckets")
    start, end = int(occupied[0]), int(occupied[-1]) + 1
    kept = counts[start - 1:end] if start > 0 else np.concatenate([[0], counts[:end]])
    return limits[start:end + 1].tolist(), [float(c) for c in kept]


def histogram_fields(record, i, limits=None):
    """Tensor i of a StepStats record (with buckets) -> the keyword arguments of EventWriter.add_histogram_raw, as make_histogram
    would fill them for the same values: num = n_finite, the limits and counts trimmed by trim_histogram."""
    t = record["tensors"][i]
    if t["counts"] is None:
        raise ValueError("histogram_fields: the record of step %d holds no bucket counts" % record["step"])
    if limits is None:
        from .step_stats import default_bins
        limits = default_bins()
    bucket_limits, bucket_counts = trim_histogram(t["counts"], limits)
    return dict(min=float(t["min"]), max=float(t["max"]), num=t["n_finite"], sum=t["sum"], sum_squares=t["sum_sq"],
                bucket_limits=bucket_limits, bucket_counts=bucket_counts)


def log_dir_name(cfg, now=None):
    """{output_root}/logs/{log_dir}/{dataset_name}_{experiment_name}_date_{%b%d_%H-%M-%S}: the reference's directory
    (train_segmentation.py:392-396, 464-467)."""
    import datetime
    now = now or datetime.datetime.now()
    prefix = "{}/{}_{}".format(cfg.log_dir, cfg.dataset_name, cfg.experiment_name)
    return os.path.join(cfg.output_root, "logs", "{}_date_{}".format(prefix, now.strftime("%b%d_%H-%M-%S")))


CD_TAGS = ("cd/pos_intra", "cd/pos_inter", "cd/neg_inter")          # the scalar of each cd tensor: its mean
HIST_TAGS = ("intra_cd", "inter_cd", "neg_cd")                      # ... and its histogram's tag


class TrainLog:
    """The log of one training run.  Only rank 0 opens a file (the reference logs with rank_zero_only=True); on every other rank the
    methods do nothing.  ``consume(records, scalar_tags)`` takes what ``StepStats.drain()`` returned: tensor i of a record is the
    cd tensor CD_TAGS[i], scalar j is the value logged as scalar_tags[j]."""

    def __init__(self, cfg, rank=0, now=None):
        self.scalar_freq = max(int(getattr(cfg, "scalar_log_freq", 10)), 1)
        self.hist_freq = getattr(cfg, "hist_freq", None)
        self.dir = self.writer = None
        self._limits = None
        if rank == 0:
            self.dir = log_dir_name(cfg, now)
            self.writer = EventWriter(self.dir)

    def wants_hist(self, step):
        """The reference's condition (train_segmentation.py:144): hist_freq is set, step % hist_freq == 0 and step > 0."""
        return self.hist_freq is not None and int(self.hist_freq) > 0 and step % int(self.hist_freq) == 0 and step > 0

    def consume(self, records, scalar_tags):
        if self.writer is None:
            return
        for rec in records:
            step = rec["step"]
            if step % self.scalar_freq == 0:
                for tag, v in zip(scalar_tags, rec["scalars"]):
                    self.writer.add_scalar(tag, v, step)
                for tag, t in zip(CD_TAGS, rec["tensors"]):
                    self.writer.add_scalar(tag, t["mean"], step)
            if rec["with_hist"] and self.wants_hist(step):
                if self._limits is None:
                    from .step_stats import default_bins
                    self._limits = default_bins()
                for i, tag in enumerate(HIST_TAGS[:len(rec["tensors"])]):
                    t = rec["tensors"][i]
                    if t["counts"] is not None and t["counts"].any():          # (neg_samples: 0 gives an empty tensor: nothing to draw)
                        self.writer.add_histogram_raw(tag, step=step, **histogram_fields(rec, i, self._limits))
        self.writer.flush()

    def scalars(self, values, step):
        if self.writer is None:
            return
        for k, v in values.items():
            self.writer.add_scalar(k, float(v), step)
        self.writer.flush()

    def image(self, tag, image, step):
        if self.writer is None:
            return
        self.writer.add_image(tag, image, step)
        self.writer.flush()

    def close(self):
        if self.writer is not None:
            self.writer.close()


def confusion_figure(hist, colors=None):
    """The column-normalised cluster histogram as the reference draws it (train_segmentation.py:305-330; imshow instead of seaborn's
    heatmap, class indices as names) -> uint8 [H, W, 3], or None when matplotlib is not installed."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return None
    hist = np.asarray(hist, np.float32)
    hist = hist / np.maximum(hist.sum(0, keepdims=True), 1)
    n = hist.shape[0]
    fig = plt.figure(figsize=(13, 10))
    try:
        ax = fig.gca()
        im = ax.imshow(hist.T, cmap="Blues", aspect="auto")
        fig.colorbar(im, ax=ax)
        ax.set_xlabel("Predicted labels")
        ax.set_ylabel("True labels")
        names = [str(i) for i in range(n)]
        ax.set_xticks(np.arange(n))
        ax.set_yticks(np.arange(hist.shape[1]))
        ax.xaxis.tick_top()
        ax.xaxis.set_ticklabels(names, fontsize=14, rotation=90)
        ax.yaxis.set_ticklabels([str(i) for i in range(hist.shape[1])], fontsize=14)
        if colors is not None:
            for labels in (ax.xaxis.get_ticklabels(), ax.yaxis.get_ticklabels()):
                for i, t in enumerate(labels):
                    t.set_color(np.asarray(colors[i % len(colors)], np.float32) / 255.0)
        ax.set_xticks(np.arange(n + 1) - 0.5, minor=True)
        ax.set_yticks(np.arange(hist.shape[1] + 1) - 0.5, minor=True)
        ax.grid(which="minor", color=(0.5, 0.5, 0.5))
        fig.tight_layout()
        fig.canvas.draw()
        rgba = np.asarray(fig.canvas.buffer_rgba())
        return np.ascontiguousarray(rgba[:, :, :3])
    finally:
        plt.close(fig)
