"""Times the stitch kernel (csrc/stitch_probe.hip) on the aerial-scene shape of the reference's plot_potsdam.py - a 4800 x 4800
canvas, windows of 320 with 40 x 40 codes, K = 70, 27 + 27 labels, flip on - without overlap (stride 320, 15 x 15 windows) and with
half-window overlap (stride 160, 29 x 29 windows), writing label maps (ARGMAX) or probabilities (PROBS); and, in the same process,
the chain it replaces, built from what the project offered before: probe_head(..., "log_probs") per chunk of 16 windows, a torch
weighted accumulation of every window's map into the canvas (the tent weights precomputed, outside the timing), and the final
softmax or argmax.  The chain blends log-probabilities where the kernel blends logits; its traffic is the same.

Device events around each window of `--iters` calls, `--repeats` windows, median / min / max reported.  Every call writes far more
than the 256 MB Infinity Cache holds; the outputs still rotate over two sets.  Peak allocation is torch's, above what is allocated
before the timed calls (the codes and weights).  The fraction of the copy rate is the compulsory bytes (both code sets read once,
the canvas written once) over the time, against the measured float4 copy rate of the MI355X (6.29 TB/s).

    python tools/bench_stitch.py --out profiles/stitch_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stego_amd import capi  # noqa: E402
from stego_amd.segment import window_origins  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE = 6.29e12
H = W = 4800
WIN, HC, K, N = 320, 40, 70, 27
CHUNK = 16


def _time(fn, iters, warmup, repeats):
    """ms per call: (median, min, max) over `repeats` windows of `iters` calls each."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(repeats):
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / iters)
    per.sort()
    return per[len(per) // 2], per[0], per[-1]


def _peak(fn):
    """Bytes torch allocates at the most during fn(), above what is allocated before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    del out
    return peak


def bench_stride(stride, args):
    oys, oxs = window_origins(H, WIN, stride), window_origins(W, WIN, stride)
    wins = [(oy, ox) for oy in oys for ox in oxs]
    T = len(wins)
    g = torch.Generator(device=DEV).manual_seed(stride)
    code = torch.randn(T, HC, HC, K, device=DEV, generator=g).permute(0, 3, 1, 2)        # the head's channels-last view
    flip = torch.randn(T, HC, HC, K, device=DEV, generator=g).permute(0, 3, 1, 2)
    lw = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    lb = torch.randn(N, device=DEV, generator=g) * 0.1
    cent = F.normalize(torch.randn(N, K, device=DEV, generator=g), dim=1)
    code_bytes = 2 * T * K * HC * HC * 4
    rec = {"windows": T, "code_bytes": code_bytes}

    # ---- the fused call
    kinds = {"argmax": capi.PROBE_ARGMAX, "probs": capi.PROBE_PROBS}
    cm, fm, stream = capi._map(code), capi._map(flip), capi._stream()
    for kind, k in kinds.items():
        desc = capi.stitch_desc(H, W, WIN, stride, T, K, HC, HC, N, N, k, k, 2.0)
        outs = [[torch.empty(H, W, dtype=torch.int64, device=DEV) if kind == "argmax" else torch.empty(N, H, W, device=DEV)
                 for _ in range(2)] for _ in range(2)]

        def run(i):
            o = outs[i % 2]
            capi._check(capi.stitch_probe_raw(desc, cm, fm, lw, lb, cent, o[0], o[1], stream))
        ms, lo, hi = _time(run, args.iters, args.warmup, args.repeats)
        del outs
        byts = code_bytes + 2 * H * W * (8 if kind == "argmax" else 4 * N)
        peak = _peak(lambda: capi.stitch_probe(code, flip, lw, lb, cent, (H, W), WIN, stride, kind, kind, 2.0))
        rec["fused_" + kind] = {"ms": round(ms, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "compulsory_bytes": byts,
                                "TBps": round(byts / (ms * 1e-3) / 1e12, 3), "frac_of_copy_rate": round(byts / COPY_RATE / (ms * 1e-3), 3),
                                "peak_alloc_bytes": peak, "calls_per_window": args.iters, "windows_timed": args.repeats}

    # ---- the chain this replaces
    u = torch.arange(WIN, dtype=torch.float32, device=DEV)
    tent = torch.minimum(u + 1, WIN - u)
    a = tent[:, None] * tent[None, :]
    total = torch.zeros(H, W, device=DEV)
    for oy, ox in wins:
        total[oy:oy + WIN, ox:ox + WIN] += a
    weights = torch.stack([a / total[oy:oy + WIN, ox:ox + WIN] for oy, ox in wins])             # [T, win, win], not timed
    del total

    def chain(kind):
        canvas = [torch.zeros(N, H, W, device=DEV) for _ in range(2)]
        for t0 in range(0, T, CHUNK):
            lps = capi.probe_head(code[t0:t0 + CHUNK], flip[t0:t0 + CHUNK], lw, lb, cent, (WIN, WIN), "log_probs", "log_probs", 2.0)
            for c, lp in zip(canvas, lps):
                for i in range(lp.shape[0]):
                    oy, ox = wins[t0 + i]
                    c[:, oy:oy + WIN, ox:ox + WIN].addcmul_(lp[i], weights[t0 + i])
        if kind == "argmax":
            return canvas[0].argmax(0), canvas[1].argmax(0)
        return torch.softmax(canvas[0], 0), torch.softmax(canvas[1], 0)

    for kind in kinds:
        ms, lo, hi = _time(lambda i: chain(kind), args.chain_iters, 1, args.repeats)
        rec["chain_" + kind] = {"ms": round(ms, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                                "peak_alloc_bytes": _peak(lambda: chain(kind)), "calls_per_window": args.chain_iters,
                                "windows_timed": args.repeats}
        rec["speedup_" + kind] = round(ms / rec["fused_" + kind]["ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--chain-iters", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stitch needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0),
           "shape": "canvas %dx%d win=%d code=%dx%d K=%d n=%d+%d flip, chain chunk %d" % (H, W, WIN, HC, HC, K, N, N, CHUNK)}
    for stride in (320, 160):
        rec["stride_%d" % stride] = bench_stride(stride, args)
        print(json.dumps({"stride": stride, **rec["stride_%d" % stride]}), flush=True)
    rec["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f)
            f.write("\n")


if __name__ == "__main__":
    main()
