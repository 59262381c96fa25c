"""Times one capi.corr_heatmaps call (csrc/corr_heat.hip, two launches) at B = 1, a 64 x 64 map upsampled to 512 x 512, for the
backbone's features (C = 384, channels-last) and the code (C = 70), with N = 280 query points (the movie), 3 (the figure) and 1
(interactive), against the chain it replaces run with torch on the same GPU (plot_dino_correspondence.py:43-56: grid_sample, two
F.normalize, einsum, mean, clamp, F.interpolate).  Input maps and output buffers rotate over sets larger than the 256 MB Infinity
Cache; every call is timed on its own with device events, `--calls` calls after `--warmup`, median / min / max.

    python tools/bench_heatmaps.py --out profiles/heatmaps_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stego_amd import capi  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12            # the measured copy rate of the part: what a store-bound kernel can reach
H_MAP, RES = 64, 512
CACHE = 300 * 2 ** 20


def _time(fn, calls, warmup):
    """us per call: (median, min, max) over `calls` individually timed calls."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(warmup + i)
        b.record()
    torch.cuda.synchronize()
    per = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return per[len(per) // 2], per[0], per[-1]


def torch_chain(feats, pts, size):
    N = pts.shape[1]
    s = F.grid_sample(feats, pts.reshape(1, N, 1, 2).permute(0, 2, 1, 3), padding_mode="border", align_corners=True)
    attn = torch.einsum("nchw,ncij->nhwij", F.normalize(s, dim=1), F.normalize(feats, dim=1))
    attn -= attn.mean([3, 4], keepdims=True)
    attn = attn.clamp(0).squeeze(0)
    return F.interpolate(attn, size, mode="bilinear", align_corners=True)


def one_shape(args, C, N):
    g = torch.Generator(device=DEV).manual_seed(C * 1000 + N)
    in_sets = -(-CACHE // (C * H_MAP * H_MAP * 4)) + 1
    out_bytes = N * RES * RES * 4
    out_sets = -(-CACHE // out_bytes) + 1
    feats = [torch.randn(1, H_MAP, H_MAP, C, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(in_sets)]      # channels-last views
    pts = torch.rand(1, N, 2, device=DEV, generator=g) * 2 - 1
    heat = torch.empty(out_sets, 1, N, RES, RES, device=DEV)
    desc = capi.heat_desc(1, C, H_MAP, H_MAP, H_MAP, H_MAP, N, RES, RES, 0)
    n_ws = capi.heat_workspace_bytes(desc)
    ws = capi._empty_bytes(n_ws, DEV)
    maps = [capi._map(f) for f in feats]
    stream = capi._stream()

    def run(i):
        m = maps[i % in_sets]
        capi._check(capi.corr_heatmaps_raw(desc, m, m, None, pts, heat[i % out_sets], None, None, ws, n_ws, stream))
    us, lo, hi = _time(run, args.calls, args.warmup)

    def chain(i):
        with torch.no_grad():
            torch_chain(feats[i % in_sets], pts, (RES, RES))
    cus, clo, chi = _time(chain, args.calls, args.warmup)
    with torch.no_grad():
        diff = float((torch_chain(feats[0], pts, (RES, RES)) - capi.corr_heatmaps(feats[0], feats[0], pts, (RES, RES))[0]).abs().max())
    lds1, g1, g2, lds2, rows = capi.heat_plan(desc)
    return {"us": round(us, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "torch_chain_us": round(cus, 2), "torch_chain_us_min": round(clo, 2),
            "torch_chain_us_max": round(chi, 2), "speedup_vs_torch_chain": round(cus / us, 2), "output_bytes": out_bytes,
            "map_bytes": C * H_MAP * H_MAP * 4, "workspace_bytes": n_ws,
            "output_frac_of_hbm_peak_8TBps": round(out_bytes / HBM_PEAK / (us * 1e-6), 4),
            "output_frac_of_hbm_copy_rate_6.29TBps": round(out_bytes / HBM_COPY / (us * 1e-6), 4),
            "grid_low": list(g1), "grid_write": list(g2), "lds_low": lds1, "lds_write": lds2, "out_rows_per_workgroup": rows,
            "rotating_input_sets": in_sets, "rotating_output_sets": out_sets, "timed_calls": args.calls,
            "max_abs_diff_vs_torch_chain": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_heatmaps needs the MI355X"
    assert args.calls >= 50
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0),
           "shape": "B=1, 64x64 map (channels-last) against itself, heatmaps 512x512; every call timed on its own with device events",
           "rows": {}}
    for C, name in ((384, "feats_c384"), (70, "code_c70")):
        for N in (280, 3, 1):
            key = "%s_N%d" % (name, N)
            rec["rows"][key] = one_shape(args, C, N)
            print(json.dumps({key: rec["rows"][key]}), flush=True)
    rec["slower_than_torch_chain"] = [k for k, r in rec["rows"].items() if r["speedup_vs_torch_chain"] < 1.0]
    rec["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
