"""Times the dense CRF (stego_amd.crf, csrc/dense_crf.hip) at the evaluation shape: B = 16 (the eval loader's 2 * batch_size), 320^2,
C = 27, 10 mean-field iterations, on per-pixel colour noise (M ~ 6N bilateral vertices: the worst case) and on a smooth synthetic
scene.  Device events around each call after a warm-up; median and spread of the repeats.  Construction (n_iter = 0: lattices,
normalisation, unary) and the iterations ((t(10) - t(0)) / 10) are reported separately, with the compulsory and the nominal bytes an
iteration moves (computed from M, N and C, see iteration_bytes) over its time, and the CPU oracle's time for one image (tests/crf_oracle.py, numpy, one thread).

    python tools/bench_crf.py --out profiles/crf_bench.txt
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scene(kind, B, C, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        bgr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    else:                                             # gradients plus flat blocks
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        imgs = []
        for _ in range(B):
            img = np.stack([xx * 255 / (W - 1), yy * 255 / (H - 1), np.full_like(xx, 128)], -1)
            for _ in range(6):
                y0, x0 = rng.integers(0, H - H // 4), rng.integers(0, W - W // 4)
                h, w = rng.integers(H // 8, H // 3), rng.integers(W // 8, W // 3)
                img[y0:y0 + h, x0:x0 + w] = rng.integers(0, 256, 3)
            imgs.append(img.astype(np.uint8))
        bgr = np.stack(imgs)
    lg = rng.standard_normal((B, C, H, W)).astype(np.float32) * 3
    e = np.exp(lg - lg.max(1, keepdims=True))
    return bgr, (e / e.sum(1, keepdims=True)).astype(np.float32)


def iteration_bytes(N, C, M):
    """(nominal, compulsory) bytes of one mean-field iteration.  M = {2: Gaussian vertices, 5: bilateral vertices} summed over the
    batch, N = pixels of the batch.  Nominal counts every row access the kernels make (the blur reads 3 rows per vertex per pass,
    the splat and the slice d+1 rows per pixel): caches serve many of them, so nominal bytes over time is not DRAM bandwidth.
    Compulsory counts every array once per launch: a lower bound on the DRAM traffic."""
    Cp = (C + 3) // 4 * 4
    row = Cp * 4
    nominal = compulsory = 0
    for d, m in M.items():
        E = N * (d + 1)
        nominal += E * 8 + E * row + m * row + m * 4                # splat: (pixel, weight) records, gathered rows, piece rows written
        nominal += (d + 1) * (m * 8 + 4 * m * row)                  # blur: neighbours, 3 rows read + 1 written per vertex per pass
        nominal += E * 8 + E * row + N * 4                          # slice in the combine: (vertex, weight), rows, s
        compulsory += E * 8 + N * row + m * row + m * 4             # splat: records, each input row once, piece rows
        compulsory += (d + 1) * (m * 8 + 2 * m * row)               # blur: neighbours, each row read once and written once
        compulsory += E * 8 + m * row + N * 4                       # slice: records, each vertex row once, s
    nominal += N * row * 3                                          # combine: -U read, s_g Q and s_b Q written
    compulsory += N * row * 3
    return nominal, compulsory


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--res", type=int, default=320)
    ap.add_argument("--C", type=int, default=27)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--oracle-images", type=int, default=1, help="images the CPU oracle times (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crf times the MI355X: no GPU found"
    from stego_amd import capi
    dev = torch.device("cuda:0")
    B, C, H, W = a.B, a.C, a.res, a.res
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("dense CRF, B = %d, %dx%d, C = %d, %d iterations; device %s" % (B, H, W, C, a.iters, torch.cuda.get_device_name(0)))
    results = {}
    for kind in ("noise", "smooth"):
        bgr, probs = scene(kind, B, C, H, W, seed=1)
        tb, tp = torch.from_numpy(bgr).to(dev), torch.from_numpy(probs).to(dev)
        desc0 = capi.crf_desc(B, C, H, W, 0, 3, 1, 4, 67, 3)
        descn = capi.crf_desc(B, C, H, W, a.iters, 3, 1, 4, 67, 3)
        ws = torch.empty(capi.crf_workspace_bytes(descn), dtype=torch.uint8, device=dev)

        def timed(desc):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            capi.crf_run(desc, tb, tp, workspace=ws)
            e.record()
            e.synchronize()
            return s.elapsed_time(e)

        for desc in (desc0, descn):               # warm-up: code objects, rocprim's config selection, the output's allocation
            capi.crf_run(desc, tb, tp, workspace=ws)
        torch.cuda.synchronize()
        t0, tn = [], []
        for _ in range(a.repeats):                # alternate the two shapes
            t0.append(timed(desc0))
            tn.append(timed(descn))
        t0, tn = np.array(t0), np.array(tn)
        Mg = [capi.crf_lattice_info(descn, ws, b, 0)[0] for b in range(B)]
        Mb = [capi.crf_lattice_info(descn, ws, b, 1)[0] for b in range(B)]
        it_ms = (np.median(tn) - np.median(t0)) / a.iters
        nbytes, cbytes = iteration_bytes(B * H * W, C, {2: sum(Mg), 5: sum(Mb)})
        r = dict(scene=kind, construction_ms_median=float(np.median(t0)), construction_ms_spread=[float(t0.min()), float(t0.max())],
                 total_ms_median=float(np.median(tn)), total_ms_spread=[float(tn.min()), float(tn.max())],
                 iteration_ms=float(it_ms), ms_per_image=float(np.median(tn) / B),
                 bilateral_M_per_image=[int(min(Mb)), int(max(Mb))], gaussian_M_per_image=int(Mg[0]), N_per_image=H * W,
                 nominal_bytes_per_iteration=int(nbytes), nominal_GBps_per_iteration=float(nbytes / (it_ms * 1e-3) / 1e9),
                 compulsory_bytes_per_iteration=int(cbytes), compulsory_GBps_per_iteration=float(cbytes / (it_ms * 1e-3) / 1e9))
        results[kind] = r
        say("%-6s construction %.2f ms [%.2f .. %.2f]  total (%d it) %.2f ms [%.2f .. %.2f]  -> %.3f ms / iteration, %.3f ms / image"
            % (kind, r["construction_ms_median"], t0.min(), t0.max(), a.iters, r["total_ms_median"], tn.min(), tn.max(), it_ms,
               r["ms_per_image"]))
        say("       bilateral M per image %d .. %d (N = %d, 6N = %d), Gaussian M %d; per iteration: compulsory %.1f MB -> %.0f GB/s, "
            "nominal (every row access, caches serve many) %.1f MB -> %.0f GB/s"
            % (min(Mb), max(Mb), H * W, 6 * H * W, Mg[0], cbytes / 1e6, r["compulsory_GBps_per_iteration"], nbytes / 1e6,
               r["nominal_GBps_per_iteration"]))
        del ws
    if a.oracle_images > 0:
        import crf_oracle as O
        bgr, probs = scene("noise", a.oracle_images, C, H, W, seed=1)
        t = time.perf_counter()
        for b in range(a.oracle_images):
            O.dense_crf(bgr[b], probs[b])
        cpu = (time.perf_counter() - t) / a.oracle_images
        results["oracle_cpu_s_per_image"] = cpu
        say("CPU oracle (numpy, one thread, noise scene): %.2f s / image = %.0fx the device's noise-scene ms / image"
            % (cpu, cpu * 1e3 / results["noise"]["ms_per_image"]))
    say(json.dumps(results))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
