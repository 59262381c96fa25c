"""Times the region descriptors (stego_amd.region_descriptors, csrc/region_pool.hip) - the three launches of stego_region_pool together,
one range over the whole table - on the label scenes of tools/bench_regions.py:

    batch_smooth_code / batch_noise_code      16 x 320 x 320 ids, the code: C = 70 at 40 x 40, channels-last as the backbone returns it
    batch_smooth_feats / batch_noise_feats    the same ids, the features: C = 768 at 40 x 40
    canvas_colour                             1 x 4800 x 4800 smooth ids, C = 3 at 4800 x 4800 (identity taps: the mean colour)

Every call is timed on its own with a pair of device events; the inputs (ids, table, map) rotate over as many sets as it takes to walk
past the 256 MB Infinity Cache between two uses of the same set; median, minimum and maximum are reported.  Beside them:

    the torch chain it replaces   F.interpolate to [B, C, H, W] and index_add_ (float32 atomics), with its peak allocation
    bytes moved                   ids once, the map twice (range and pool), the sums reset, added and read, the descriptors - at 6.29 TB/s
    atomic bytes                  8 bytes per channel and flush (the flushes are counted from the ids and the plan's segment) at 1.3 TB/s,
                                  the guide's rate for well-shaped global float atomics
    the sized expectation         smooth scenes bound by launches and latency (tens of us: 50 us is taken as the mark), noise scenes by
                                  their atomic bytes at 1.3 TB/s; `expectation_held` is measured <= 1.5 x that, and a miss is a miss
    label_regions + the table     the parent's calls on the same ids, for scale

    python tools/bench_region_pool.py --out profiles/region_pool_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_regions import CACHE, COPY_RATE, DEV, _events, _us, make_map  # noqa: E402
from stego_amd import capi  # noqa: E402
from stego_amd import regions as R  # noqa: E402

ATOMIC_RATE = 1.3e12
LATENCY_MARK_US = 50.0
CASES = {"batch_smooth_code": (16, 320, 320, "smooth", 70, 40, 40), "batch_noise_code": (16, 320, 320, "noise", 70, 40, 40),
         "batch_smooth_feats": (16, 320, 320, "smooth", 768, 40, 40), "batch_noise_feats": (16, 320, 320, "noise", 768, 40, 40),
         "canvas_colour": (1, 4800, 4800, "smooth", 3, 4800, 4800)}


def count_flushes(ids, C):
    """The flushes of the pool launch, per channel block: a group's runs of one id >= 0 along its pixels of a segment."""
    B, H, W = ids.shape
    rc, L, cb, _ = capi.region_pool_plan(capi.region_pool_desc(B, C, 1, 1, H, W, 1))
    assert rc == 0
    groups = 1 if C > 32 else 64 >> max(C - 1, 0).bit_length()
    per = L // groups
    total = 0
    for g in range(groups):
        sub = ids[:, :, g::groups]
        start = torch.ones_like(sub, dtype=torch.bool)
        start[:, :, 1:] = sub[:, :, 1:] != sub[:, :, :-1]
        start[:, :, torch.arange(sub.shape[2], device=ids.device) % per == 0] = True
        total += int((start & (sub >= 0)).sum())
    return total, L


def torch_chain(m, ids, offs, area):
    B, C = m.shape[:2]
    v = torch.nn.functional.interpolate(m, ids.shape[1:], mode="bilinear", align_corners=False)
    rows = (ids.long() + offs[:, None, None]).reshape(-1)
    sums = torch.zeros((area.numel(), C), dtype=torch.float32, device=m.device)
    sums.index_add_(0, rows, v.permute(0, 2, 3, 1).reshape(-1, C))
    return sums / area[:, None].float()


def bench_case(name, args):
    B, H, W, kind, C, h, w = CASES[name]
    pixels = B * H * W
    map_bytes = B * C * h * w * 4
    per_set = pixels * 4 + map_bytes
    n_sets = max(2, min(-(-2 * CACHE // per_set), 40))
    calls = args.calls if B > 1 else max(args.calls // 4, 5)
    sets = []
    for s in range(n_sets):
        lab = make_map(B, H, W, kind, 7 * s + len(kind))
        ids, n = R.label_regions(lab, 4)
        table = R.region_table(lab, ids, n)
        g = torch.Generator(device=DEV).manual_seed(100 + s)
        m = torch.randn((B, h, w, C), device=DEV, generator=g).permute(0, 3, 1, 2) if C > 3 else torch.randn((B, C, h, w), device=DEV, generator=g)
        sets.append((ids, torch.tensor(table.row_offset, dtype=torch.int64, device=DEV), table.area.contiguous(), m, lab, len(table)))
        del table
    rows = sets[0][5]
    rec = {"ids": [B, H, W], "kind": kind, "map": [B, C, h, w], "channels_last": C > 3, "input_sets": n_sets, "calls": calls, "regions": rows}
    desc = capi.region_pool_desc(B, C, h, w, H, W, max(s[5] for s in sets))
    ws = torch.empty(capi.region_pool_workspace_bytes(desc), dtype=torch.uint8, device=DEV)
    out = torch.empty((max(s[5] for s in sets), C), dtype=torch.float32, device=DEV)

    def native(i):
        ids, offs, area, m, _, n = sets[i % n_sets]
        capi.region_pool(m, ids, offs, area, 0, n, out=out, workspace=ws)

    t = _events(native, calls, args.warmup)
    rec["region_pool"] = _us(t)
    flushes, L = count_flushes(sets[0][0], C)
    rec["segment"], rec["flushes"] = L, flushes
    moved = pixels * 4 + 2 * map_bytes + rows * C * (8 * 3 + 4)
    atomic = flushes * C * 8
    rec["bytes_moved"], rec["atomic_bytes"] = moved, atomic
    rec["copy_rate_us"], rec["atomic_rate_us"] = round(moved / COPY_RATE * 1e6, 1), round(atomic / ATOMIC_RATE * 1e6, 1)
    rec["frac_of_copy_rate"], rec["frac_of_atomic_rate"] = round(moved / COPY_RATE * 1e6 / t[0], 4), round(atomic / ATOMIC_RATE * 1e6 / t[0], 4)
    expected = LATENCY_MARK_US if kind == "smooth" and B > 1 else max(LATENCY_MARK_US, atomic / ATOMIC_RATE * 1e6, moved / COPY_RATE * 1e6)
    rec["expected_us"], rec["expectation_held"] = round(expected, 1), bool(t[0] <= 1.5 * expected)
    rec["expectation"] = "%s: expected about %.0f us (%s), measured %.0f us: %s" % (
        name, expected, "launches and latency" if expected == LATENCY_MARK_US else "atomic adds at 1.3 TB/s or the bytes at the copy rate",
        t[0], "held" if rec["expectation_held"] else "missed by %.1fx" % (t[0] / expected))
    # the parent's calls on the same ids, for scale
    rec["label_regions"] = _us(_events(lambda i: capi.regions_label(sets[i % n_sets][4], 4), calls, args.warmup))
    rec["table_launches"] = _us(_events(lambda i: capi.regions_table(sets[i % n_sets][4], sets[i % n_sets][0], sets[i % n_sets][1],
                                                                     sets[i % n_sets][5]), calls, args.warmup))
    # the chain it replaces
    if pixels * C * 4 * 2 <= args.chain_bytes:
        def chain(i):
            ids, offs, area, m, _, _ = sets[i % n_sets]
            return torch_chain(m, ids, offs, area)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ref = chain(0)
        torch.cuda.synchronize()
        rec["torch_chain_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        native(0)
        M = float(sets[0][3].abs().max())
        rec["max_abs_diff_to_chain_over_M"] = float((out[:rows] - ref).abs().max()) / M
        del ref
        tc = _events(chain, max(calls // 4, 5), 2)
        rec["torch_chain"] = _us(tc)
        rec["speedup_over_chain"] = round(tc[0] / t[0], 2)
    else:
        rec["torch_chain"] = None
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--chain-bytes", type=int, default=64 << 30, help="run the torch chain where its [B, C, H, W] tensors stay below this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_region_pool needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12, "atomic_rate_TBps": ATOMIC_RATE / 1e12}
    for name in args.cases.split(","):
        rec[name] = bench_case(name, args)
        print(json.dumps({"case": name, **rec[name]}), flush=True)
        torch.cuda.empty_cache()
    rec["wall_s"] = round(time.time() - t0, 1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f)
            f.write("\n")


if __name__ == "__main__":
    main()
