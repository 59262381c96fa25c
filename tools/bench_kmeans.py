"""Times one Lloyd step and one k-means++ seeding of the cluster refit (csrc/code_kmeans.hip) and, in the same process on the same
GPU, the torch chain of the same step (normalize, einsum, argmax, index_add_, bincount), on the codes a user refits on:

    folder   B = 5000, K = 70, 28 x 28     the ViT-S/8 codes of a 5000-image folder at 224 (3.92 M tokens, 1.1 GB)
    batch    B = 16,   K = 70, 28 x 28     one batch

each with n = 8, 27 and 64 clusters, as the channels-last tensor collect_codes returns.  Every call is timed on its own with a pair of
device events; the inputs rotate over as many sets as it takes to walk past the 256 MB Infinity Cache between two uses of the same set
(the folder's tensor is four times the cache on its own); the median, minimum and maximum of `--calls` calls are reported.  Per shape
the step's time is set against max(bytes / 6.29 TB/s, flops / 155 TF) - the codes read once, and the two products, scores and sums,
2 * 2 T K n flops - and the seeding's against n reads of the codes.

    python tools/bench_kmeans.py --out profiles/kmeans_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stego_amd import capi, cluster_refit  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE, MFMA_F32_RATE = 6.29e12, 155e12
CACHE = 256 << 20
SHAPES = {"folder": (5000, 70, 28), "batch": (16, 70, 28)}
COUNTS = (8, 27, 64)


def _time(fn, calls, warmup):
    """us per call over `calls` individually timed calls -> (median, min, max)."""
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


def _us(t):
    return {"us": round(t[0], 1), "us_min": round(t[1], 1), "us_max": round(t[2], 1)}


def _codes(name):
    B, K, s = SHAPES[name]
    size = B * K * s * s * 4
    n_sets = 1 if size >= 2 * CACHE else min(-(-2 * CACHE // size), 160)
    g = torch.Generator(device=DEV).manual_seed(len(name))
    return [torch.randn(B, s, s, K, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(n_sets)]


def torch_chain_step(codes, cent):
    """One Lloyd step as the torch chain a user would write."""
    B, K, h, w = codes.shape
    x = F.normalize(codes.permute(0, 2, 3, 1).reshape(-1, K), dim=1)
    c = F.normalize(cent, dim=1)
    inner = torch.einsum("tk,nk->tn", x, c)
    a = inner.argmax(1)
    sums = torch.zeros_like(c).index_add_(0, a, x)
    counts = torch.bincount(a, minlength=c.shape[0])
    new = torch.where((counts == 0)[:, None], c, F.normalize(sums, dim=1))
    return new, counts, inner.gather(1, a[:, None]).sum()


def bench_case(name, n, args):
    B, K, s = SHAPES[name]
    T = B * s * s
    sets = _codes(name)
    m = len(sets)
    calls = args.calls if name != "folder" else max(args.calls // 5, 5)
    desc = capi.kmeans_desc(B, K, s, s, n)
    ws = capi.kmeans_workspace(desc, DEV)
    lds, wgs = capi.kmeans_plan(desc)
    cent = F.normalize(torch.randn(n, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)), dim=1)
    out = torch.empty_like(cent)
    labels = torch.empty(B, s, s, dtype=torch.uint8, device=DEV)
    counts = torch.empty(n, dtype=torch.int64, device=DEV)
    stats = torch.empty(4, dtype=torch.float64, device=DEV)
    u = torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(n)).tolist()
    rec = {"shape": [B, K, s, s], "n": n, "tokens": T, "input_sets": m, "calls": calls, "workspace_bytes": ws[1], "lds_bytes": lds,
           "workgroups": wgs, "bytes": T * K * 4, "flops": 4 * T * K * n}
    model = max(rec["bytes"] / COPY_RATE, rec["flops"] / MFMA_F32_RATE)
    rec["model_us"] = round(model * 1e6, 1)
    rec["model_bound"] = "bytes" if rec["bytes"] / COPY_RATE >= rec["flops"] / MFMA_F32_RATE else "flops"
    step = _time(lambda i: capi.kmeans_step(desc, sets[i % m], cent, out, None, counts, stats, ws), calls, args.warmup)
    rec["step"] = _us(step)
    rec["step_frac_of_model"] = round(model * 1e6 / step[0], 4)
    rec["step_with_labels"] = _us(_time(lambda i: capi.kmeans_step(desc, sets[i % m], cent, out, labels, counts, stats, ws), calls, args.warmup))
    rec["assign_only"] = _us(_time(lambda i: capi.kmeans_step(desc, sets[i % m], cent, None, labels, counts, stats, ws), calls, args.warmup))
    seed_calls = max(calls // 5, 3)
    seed = _time(lambda i: capi.kmeans_seed(desc, sets[i % m], u, ws), seed_calls, 1)
    rec["seed"] = {**_us(seed), "calls": seed_calls}
    rec["seed_frac_of_copy_rate"] = round(n * rec["bytes"] / COPY_RATE * 1e6 / seed[0], 4)
    chain = _time(lambda i: torch_chain_step(sets[i % m], cent), args.chain_calls, 2)
    rec["torch_chain_step"] = {**_us(chain), "calls": args.chain_calls}
    rec["speedup"] = round(chain[0] / step[0], 2)
    got = cluster_refit.kmeans_step(sets[0], cent)
    ref = torch_chain_step(sets[0], cent)
    rec["counts_equal_torch"] = bool(torch.equal(got.counts, ref[1]))
    rec["centroids_max_diff_torch"] = float((got.centroids - ref[0]).abs().max())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--chain-calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kmeans needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12, "f32_mfma_TFs": MFMA_F32_RATE / 1e12}
    for name in args.cases.split(","):
        for n in COUNTS:
            key = "%s_n%d" % (name, n)
            rec[key] = bench_case(name, n, args)
            print(json.dumps({"case": key, **rec[key]}), flush=True)
            torch.cuda.empty_cache()
    rec["wall_s"] = round(time.time() - t0, 1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f)
            f.write("\n")


if __name__ == "__main__":
    main()
