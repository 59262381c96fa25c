"""Times the device-side confusion matrices (csrc/confusion.hip) against what they replace, at the shapes validation and evaluation
run: B = 16, K = 70, 40^2 -> 320^2, 27 + 27 labels, flip on; and B = 32, 28^2 -> 224^2.

  (a) stego_probe_confusion: low-resolution code -> both matrices, one launch.
  (b) the fused path it replaces: stego_probe_head ARGMAX for both probes, then two UnsupervisedMetrics.update calls.
  (c) the torch chain of validation_step (F.interpolate, the 1x1 probe, ClusterLookup, two argmax) plus the two updates.
  (d) stego_confusion on [16, 27, 320, 320] scores against argmax + update.
  (e) one Trainer._validate pass of the tiny test model (vit_tiny/16, res 64) with and without cfg.native_metrics, wall time.

Every call is timed on its own (device events around one call, the median of `--calls` calls after `--warmup`); the inputs rotate
over sets larger than the 256 MB Infinity Cache.  For (b) and (c) the host time per batch is recorded as well (a host clock around
the call): the per-probe `.cpu()` of update() makes the host wait for the device there, while (a) returns after the enqueue.

    python tools/bench_confusion.py --out profiles/confusion_bench.json
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stego_amd import capi  # noqa: E402
from stego_amd.utils import UnsupervisedMetrics  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE = 6.29e12          # bytes/s: the device copy rate the README measures rooflines against


def _time(fn, calls, warmup):
    """Per call: device us (events around the one call) and host us (a clock around the call, no synchronise inside it unless the
    call itself makes one) -> {"us", "us_min", "us_max", "host_us"}, medians over `calls` calls."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    dev, host = [], []
    for i in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn(warmup + i)
        b.record()
        host.append((time.perf_counter() - t0) * 1e6)
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3)
    dev.sort()
    host.sort()
    return {"us": round(dev[len(dev) // 2], 2), "us_min": round(dev[0], 2), "us_max": round(dev[-1], 2),
            "host_us": round(host[len(host) // 2], 2), "calls": calls}


def probe_shape(B, K, h, H, n, args):
    g = torch.Generator(device=DEV).manual_seed(0)
    per_set = 2 * B * K * h * h * 4 + B * H * H * 8
    sets = max(2, -(-300 * 2 ** 20 // per_set) + 1)                 # rotate past the Infinity Cache
    codes = [torch.randn(B, h, h, K, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(sets)]     # channels-last views
    flips = [torch.randn(B, h, h, K, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(sets)]
    # piecewise-constant labels, as segmentation maps are: 16 x 16 blocks, one block in eight ignored (-1)
    labels = []
    for _ in range(sets):
        blocks = torch.randint(-1, n, (B, 1, -(-H // 16), -(-H // 16)), device=DEV, generator=g).float()
        blocks[torch.rand(blocks.shape, device=DEV, generator=g) < 0.125] = -1
        labels.append(F.interpolate(blocks, scale_factor=16, mode="nearest")[:, 0, :H, :H].long().contiguous())
    W = torch.randn(n, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(n, device=DEV, generator=g) * 0.1
    clusters = torch.randn(n, K, device=DEV, generator=g)
    cent = F.normalize(clusters, dim=1)
    stream = capi._stream()
    rows = {"rotating_sets": sets}

    # (a)
    lin_counts = torch.zeros(n, n, dtype=torch.int64, device=DEV)
    clu_counts = torch.zeros(n, n, dtype=torch.int64, device=DEV)
    cdesc = capi.probe_confusion_desc(B, K, h, h, H, H, n, n, 1, 1, 2.0, n)

    def native(i):
        s = i % sets
        capi._check(capi.probe_confusion_raw(cdesc, capi._map(codes[s]), capi._map(flips[s]), W, b, cent, labels[s], lin_counts,
                                             clu_counts, stream))
    rows["probe_confusion"] = _time(native, args.calls, args.warmup)
    rows["probe_confusion"]["bytes_read"] = per_set
    rows["probe_confusion"]["frac_of_copy_rate"] = round(per_set / COPY_RATE / (rows["probe_confusion"]["us"] * 1e-6), 4)

    # the ARGMAX call alone (the same arithmetic, writing two int64 label maps)
    outs = [[torch.empty(B, H, H, dtype=torch.int64, device=DEV) for _ in range(2)] for _ in range(sets)]
    hdesc = capi.probe_desc(B, K, h, h, H, H, n, n, capi.PROBE_ARGMAX, capi.PROBE_ARGMAX, 2.0)

    def head(i):
        s = i % sets
        capi._check(capi.probe_head_raw(hdesc, capi._map(codes[s]), capi._map(flips[s]), W, b, cent, outs[s][0], outs[s][1], stream))
    rows["probe_head_argmax"] = _time(head, args.calls, args.warmup)

    # (b)
    lin_m, clu_m = UnsupervisedMetrics("l/", n, 0, False), UnsupervisedMetrics("c/", n, 0, True)

    def fused(i):
        s = i % sets
        head(i)
        lin_m.update(outs[s][0], labels[s])
        clu_m.update(outs[s][1], labels[s])
    rows["probe_head_argmax_plus_two_updates"] = _time(fused, args.calls, args.warmup)

    # (c)
    lin = torch.nn.Conv2d(K, n, 1).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(W[:, :, None, None])
        lin.bias.copy_(b)

    def chain(i):
        s = i % sets
        with torch.no_grad():
            c = F.interpolate(codes[s], (H, H), mode="bilinear", align_corners=False)
            lp = lin(c).argmax(1)
            lin_m.update(lp, labels[s])
            inner = torch.einsum("bchw,nc->bnhw", F.normalize(c, dim=1), F.normalize(clusters, dim=1))
            clu_m.update(inner.argmax(1), labels[s])
    rows["torch_validation_chain_plus_two_updates"] = _time(chain, max(5, args.calls // 4), 3)

    a = rows["probe_confusion"]["us"]
    rows["speedup_vs_fused_path"] = round(rows["probe_head_argmax_plus_two_updates"]["us"] / a, 2)
    rows["speedup_vs_torch_chain"] = round(rows["torch_validation_chain_plus_two_updates"]["us"] / a, 2)
    rows["ratio_to_probe_head_argmax_alone"] = round(a / rows["probe_head_argmax"]["us"], 3)
    # the counts of (a) and of (b) agree: the same inputs were counted the same number of times
    torch.cuda.synchronize()
    rows["counts_total"] = int(lin_counts.sum())
    return rows


def scores_shape(B, n, H, args):
    g = torch.Generator(device=DEV).manual_seed(1)
    per_set = B * n * H * H * 4 + B * H * H * 8
    sets = max(2, -(-300 * 2 ** 20 // per_set) + 1)
    scores = [torch.randn(B, n, H, H, device=DEV, generator=g) for _ in range(sets)]
    labels = [torch.randint(-1, n, (B, H, H), device=DEV, generator=g) for _ in range(sets)]
    counts = torch.zeros(n, n, dtype=torch.int64, device=DEV)
    desc = capi.confusion_desc(B, n, H, H, n, capi.CONF_SCORES)
    stream = capi._stream()
    m = UnsupervisedMetrics("m/", n, 0, False)

    def native(i):
        capi._check(capi.confusion_raw(desc, scores[i % sets], labels[i % sets], counts, stream))

    def torch_path(i):
        m.update(scores[i % sets].argmax(1), labels[i % sets])
    rows = {"rotating_sets": sets, "confusion_scores": _time(native, args.calls, args.warmup),
            "argmax_plus_update": _time(torch_path, args.calls, args.warmup)}
    rows["confusion_scores"]["bytes_read"] = per_set
    rows["confusion_scores"]["frac_of_copy_rate"] = round(per_set / COPY_RATE / (rows["confusion_scores"]["us"] * 1e-6), 4)
    rows["speedup"] = round(rows["argmax_plus_update"]["us"] / rows["confusion_scores"]["us"], 2)
    return rows


def validate_pass(args):
    """Wall time of Trainer._validate over 32 synthetic images (8 batches of 4) of the tiny model, median of `--val-repeats`."""
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, Trainer, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    out = {}
    for flag in (False, True):
        cfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=2", "dim=70", "dropout=False",
                                     "extra_clusters=1", "native_metrics=%s" % flag])
        torch.manual_seed(0)
        model = LitUnsupervisedSegmenter(27, cfg).to(DEV)
        loader = torch.utils.data.DataLoader(SyntheticContrastiveDataset(32, 64, 27, seed=3), 4, shuffle=False)
        trainer = Trainer(max_steps=0, device=DEV, val_loader=loader)
        times = []
        for _ in range(args.val_repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            metrics = trainer._validate(model)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        times = sorted(times[1:])
        out["native_metrics=%s" % flag] = {"ms": round(times[len(times) // 2], 2), "ms_min": round(times[0], 2), "ms_max": round(times[-1], 2),
                                           "metrics": {k: round(float(v), 4) for k, v in metrics.items()}}
    out["images"] = 32
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--val-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_confusion needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "method": "median of individually timed calls, inputs rotating past the Infinity Cache"}
    rec["B16_K70_40x40_to_320x320_n27+27_flip"] = probe_shape(16, 70, 40, 320, 27, args)
    print(json.dumps(rec["B16_K70_40x40_to_320x320_n27+27_flip"]), flush=True)
    rec["B32_K70_28x28_to_224x224_n27+27_flip"] = probe_shape(32, 70, 28, 224, 27, args)
    print(json.dumps(rec["B32_K70_28x28_to_224x224_n27+27_flip"]), flush=True)
    rec["scores_16x27x320x320"] = scores_shape(16, 27, 320, args)
    print(json.dumps(rec["scores_16x27x320x320"]), flush=True)
    rec["validate_pass_vit_tiny16_res64"] = validate_pass(args)
    rec["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f)
            f.write("\n")


if __name__ == "__main__":
    main()
