"""Times the segments-as-objects calls (stego_amd.regions, csrc/regions.hip) - label_regions, region_table and one cleanup round at
min_area = 16, each alone - on int64 label maps of four kinds:

    batch_smooth    16 x 320 x 320   40-pixel blocks of 27 classes with 1 % of the pixels redrawn (a probe's argmax with its specks)
    batch_noise     16 x 320 x 320   per-pixel 27-class noise: the worst case for the number of regions
    canvas_smooth    1 x 4800 x 4800
    canvas_noise     1 x 4800 x 4800

Every call is timed on its own with a pair of device events (label_regions, the table launches) or, where the call reads a count on
the host (region_table, cleanup_round), by the wall clock between two synchronisations; the inputs rotate over as many sets as it takes
to walk past the 256 MB Infinity Cache between two uses of the same set; median, minimum and maximum are reported.  Beside them:

    the copy-rate bound    the bytes of the [B, H, W] arrays each call reads and writes, at 6.29 TB/s (pass_bytes below: sized from
                           the pass count before the kernels were written)
    the chain it replaces  .cpu(), scipy.ndimage.label per class, scipy.ndimage.sum and find_objects, on one thread
    the dense CRF          10 iterations on a 16 x 320 x 320 batch with 27 classes (the scenes of tools/bench_crf.py), in this process

    python tools/bench_regions.py --out profiles/regions_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from stego_amd import capi  # noqa: E402
from stego_amd import regions as R  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE = 6.29e12
CACHE = 256 << 20
CLASSES = 27
MIN_AREA = 16
CASES = {"batch_smooth": (16, 320, 320, "smooth"), "batch_noise": (16, 320, 320, "noise"),
         "canvas_smooth": (1, 4800, 4800, "smooth"), "canvas_noise": (1, 4800, 4800, "noise")}


def make_map(B, H, W, kind, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "noise":
        return torch.randint(0, CLASSES, (B, H, W), device=DEV, generator=g)
    coarse = torch.randint(0, CLASSES, (B, -(-H // 40), -(-W // 40)), device=DEV, generator=g)
    m = coarse.repeat_interleave(40, 1).repeat_interleave(40, 2)[:, :H, :W].contiguous()
    speck = torch.rand((B, H, W), device=DEV, generator=g) < 0.01
    return torch.where(speck, torch.randint(0, CLASSES, (B, H, W), device=DEV, generator=g), m)


def pass_bytes(pixels, regions, slabs):
    """Bytes of the [B, H, W] arrays (int64 labels, int32 ids and roots) and of the table rows that each call moves at the least."""
    label = pixels * (8 + 4 + 4 + 4 + 4 + 4 + 4 + 4)      # tile: labels in, roots out; flatten: in, out; number: in; spread: root, id of the root, id out
    table = pixels * 4 + regions * 48 * 2                  # ids in; the rows reset and written
    votes = slabs * pixels * (4 + 4) * 2                   # votes and relabel: ids and the region's rank, per slab
    return {"label": label, "table": table, "cleanup": label + table + pixels * 16 + votes}


def _events(fn, calls, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    per = []
    for i in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e3)
    per.sort()
    return per[len(per) // 2], per[0], per[-1]


def _wall(fn, calls, warmup):
    for i in range(warmup):
        fn(i)
    per = []
    for i in range(calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t) * 1e6)
    per.sort()
    return per[len(per) // 2], per[0], per[-1]


def _us(t):
    return {"us": round(t[0], 1), "us_min": round(t[1], 1), "us_max": round(t[2], 1)}


def scipy_chain(lab):
    """The chain this replaces, for one batch on the device -> (seconds, regions): .cpu(), then per image and class ndimage.label,
    ndimage.sum for the areas and find_objects for the boxes."""
    from scipy import ndimage
    t = time.perf_counter()
    host = lab.cpu().numpy()
    total = 0
    for img in host:
        for c in np.unique(img):
            ids, n = ndimage.label(img == c)
            ndimage.sum(np.ones_like(ids), ids, index=np.arange(1, n + 1))
            ndimage.find_objects(ids)
            total += n
    return time.perf_counter() - t, total


def bench_case(name, args):
    B, H, W, kind = CASES[name]
    pixels = B * H * W
    size = pixels * 8
    n_sets = max(2, min(-(-2 * CACHE // size), 48))
    sets = [make_map(B, H, W, kind, 7 * s + len(name)) for s in range(n_sets)]
    calls = args.calls if B > 1 else max(args.calls // 4, 5)
    rec = {"shape": [B, H, W], "kind": kind, "input_sets": n_sets, "calls": calls}
    found = [R.label_regions(m, 4) for m in sets]
    counts = [int(n.sum()) for _, n in found]
    rec["regions"] = counts[0]
    offs = [(torch.cumsum(n.long(), 0) - n.long()).contiguous() for _, n in found]
    table0 = R.region_table(sets[0], *found[0])
    n_small = int((table0.area < MIN_AREA).sum())
    slabs = len(R.vote_slabs(n_small, CLASSES, 2 ** 28))
    rec["small_regions"], rec["vote_slabs"] = n_small, slabs
    nbytes = pass_bytes(pixels, counts[0], slabs)
    rec["bound_us"] = {k: round(v / COPY_RATE * 1e6, 1) for k, v in nbytes.items()}
    label = _events(lambda i: capi.regions_label(sets[i % n_sets], 4), calls, args.warmup)
    rec["label_regions"] = _us(label)
    launches = _events(lambda i: capi.regions_table(sets[i % n_sets], found[i % n_sets][0], offs[i % n_sets], counts[i % n_sets]), calls,
                       args.warmup)
    rec["table_launches"] = _us(launches)
    rec["region_table"] = _us(_wall(lambda i: R.region_table(sets[i % n_sets], *found[i % n_sets]), calls, args.warmup))
    clean = _wall(lambda i: R.cleanup_round(sets[i % n_sets], MIN_AREA, CLASSES), calls, args.warmup)
    rec["cleanup_round"] = _us(clean)
    rec["frac_of_bound"] = {"label": round(rec["bound_us"]["label"] / label[0], 4), "table": round(rec["bound_us"]["table"] / launches[0], 4),
                            "cleanup": round(rec["bound_us"]["cleanup"] / clean[0], 4)}
    out, changed = R.cleanup_round(sets[0], MIN_AREA, CLASSES)
    rec["regions_changed"] = changed
    rec["pixels_changed"] = int((out != sets[0]).sum())
    if args.scipy and not (kind == "noise" and B == 1):
        try:
            seconds, total = scipy_chain(sets[0])
            rec["scipy_chain_ms"] = round(seconds * 1e3, 1)
            rec["scipy_regions_equal"] = total == counts[0]
            rec["speedup_label_and_table"] = round(seconds * 1e6 / (label[0] + rec["region_table"]["us"]), 1)
        except ImportError:
            rec["scipy_chain_ms"] = None
    return rec


def bench_crf(repeats):
    """The dense CRF on the 16 x 320 x 320 batch of tools/bench_crf.py, 27 classes, 10 iterations -> {scene: median ms}."""
    from bench_crf import scene
    out = {}
    for kind in ("noise", "smooth"):
        bgr, probs = scene(kind, 16, CLASSES, 320, 320, seed=1)
        tb, tp = torch.from_numpy(bgr).to(DEV), torch.from_numpy(probs).to(DEV)
        desc = capi.crf_desc(16, CLASSES, 320, 320, 10, 3, 1, 4, 67, 3)
        ws = torch.empty(capi.crf_workspace_bytes(desc), dtype=torch.uint8, device=DEV)
        t = _events(lambda i: capi.crf_run(desc, tb, tp, workspace=ws), repeats, 2)
        out[kind] = round(t[0] / 1e3, 2)
        del ws
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-scipy", dest="scipy", action="store_false")
    ap.add_argument("--crf-repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_regions needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12, "min_area": MIN_AREA, "classes": CLASSES}
    for name in args.cases.split(","):
        rec[name] = bench_case(name, args)
        print(json.dumps({"case": name, **rec[name]}), flush=True)
        torch.cuda.empty_cache()
    if args.crf_repeats > 0:
        rec["dense_crf_ms_16x320x320"] = bench_crf(args.crf_repeats)
        print(json.dumps({"dense_crf_ms_16x320x320": rec["dense_crf_ms_16x320x320"]}), flush=True)
    rec["wall_s"] = round(time.time() - t0, 1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f)
            f.write("\n")


if __name__ == "__main__":
    main()
