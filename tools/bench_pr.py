"""Times one capi.pr_accumulate (csrc/corr_pr.hip) at B = 16, 320^2 images: ViT-B/8 features (C = 768, 40^2, channels-last) and the
code (C = 70), labels 320^2, 27 classes, 4096 bins, for S = 11 (the reference's 121 points per side) and S = 40 (1600 points: one per
feature position), against the chain it replaces run with torch on the same GPU: four grid_samples (two feature maps, two one-hot
label maps; the one-hot maps are built outside the timed window), two normalisations, two einsums, the cast of ld and one histc per
class of pair.  Inputs rotate over sets larger than the 256 MB Infinity Cache; device events around each window of `--iters`
back-to-back launches, `--repeats` windows, median / min / max.  Also records how far the average precision of the 4096-bin histogram
is from the average precision of the unbinned float64 scores of the test oracle on one seeded input.

    python tools/bench_pr.py --out profiles/pr_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stego_amd import capi  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12
F32_MFMA_PEAK = 157.3e12
B, RES, H, N_CLASSES, N_BINS = 16, 320, 40, 27, 4096


def _time(fn, iters, warmup, repeats):
    """us per call: (median, min, max) over `repeats` windows of `iters` calls each."""
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
        per.append(a.elapsed_time(b) * 1e3 / iters)
    per.sort()
    return per[len(per) // 2], per[0], per[-1]


def _labels(g, n):
    blocks = torch.randint(-1, N_CLASSES, (n, RES // 16, RES // 16), generator=g, device=DEV)
    return blocks.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()


def torch_chain(feats, onehot, c1, c2):
    g1, g2 = c1.permute(0, 2, 1, 3), c2.permute(0, 2, 1, 3)
    s1 = F.grid_sample(feats, g1, padding_mode="border", align_corners=True)
    s2 = F.grid_sample(feats, g2, padding_mode="border", align_corners=True)
    l1 = F.grid_sample(onehot, g1, padding_mode="border", align_corners=True)
    l2 = F.grid_sample(onehot, g2, padding_mode="border", align_corners=True)
    fd = torch.einsum("nchw,ncij->nhwij", F.normalize(s1, dim=1, eps=1e-10), F.normalize(s2, dim=1, eps=1e-10))
    ld = torch.einsum("nchw,ncij->nhwij", l1, l2).to(torch.int64)
    return torch.histc(fd[ld == 0], N_BINS, -1.0, 1.0), torch.histc(fd[ld == 1], N_BINS, -1.0, 1.0)


def one_shape(args, C, S):
    g = torch.Generator(device=DEV).manual_seed(C * 100 + S)
    per_set = B * C * H * H * 4 + B * RES * RES * 8
    sets = max(2, -(-300 * 2 ** 20 // per_set) + 1)                                  # rotate past the Infinity Cache
    feats = [torch.randn(B, H, H, C, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(sets)]     # channels-last views
    labels = [_labels(g, B) for _ in range(sets)]
    c1 = torch.rand(B, S, S, 2, device=DEV, generator=g) * 2 - 1
    c2 = torch.rand(B, S, S, 2, device=DEV, generator=g) * 2 - 1
    hist = torch.zeros(N_BINS, 2, dtype=torch.int64, device=DEV)
    f1, f2 = c1.reshape(B, -1, 2).contiguous(), c2.reshape(B, -1, 2).contiguous()
    desc = capi.pr_desc(B, C, H, H, RES, RES, S * S, S * S, N_BINS, N_CLASSES, 0)
    maps = [capi._map(f) for f in feats]
    stream = capi._stream()

    def run(i):
        k = i % sets
        capi._check(capi.pr_accumulate_raw(desc, maps[k], maps[k], labels[k], labels[k], None, f1, f2, hist, stream))
    us, lo, hi = _time(run, args.iters, args.warmup, args.repeats)
    n_calls = args.warmup + args.iters * args.repeats
    assert int(hist.sum()) == n_calls * B * S ** 4, "every pair of every launch is counted"
    # bytes the kernel must read once: the map, the label pixels and coordinates of the points, and the histogram it adds to
    byts = B * C * H * H * 4 + 2 * B * S * S * (4 * 8 + 8) + N_BINS * 2 * 8
    flops = 2.0 * B * S ** 4 * C
    row = {"us": round(us, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "compulsory_bytes": byts,
           "frac_of_hbm_roofline_8TBps": round(byts / HBM_PEAK / (us * 1e-6), 4), "contraction_flop": flops,
           "frac_of_f32_mfma_peak_157TF": round(flops / F32_MFMA_PEAK / (us * 1e-6), 4), "rotating_sets": sets,
           "launches_per_window": args.iters, "windows": args.repeats, "workgroups": B * (-(-S * S // 128)) ** 2}

    onehot = [F.one_hot(lab + 1, N_CLASSES + 1).to(torch.float).permute(0, 3, 1, 2) for lab in labels[:2]]

    def chain(i):
        with torch.no_grad():
            torch_chain(feats[i % sets], onehot[i % 2], c1, c2)
    cus, clo, chi = _time(chain, max(3, args.iters // 20), 2, args.repeats)
    row["torch_chain_us"] = round(cus, 2)
    row["torch_chain_us_min"] = round(clo, 2)
    row["torch_chain_us_max"] = round(chi, 2)
    row["speedup_vs_torch_chain"] = round(cus / us, 2)
    # the chain's counts on one input, for the record: the positives differ by the pairs ld.to(int64) truncates to 0
    hk = capi.pr_accumulate(feats[0], feats[0], labels[0], labels[0], c1, c2, torch.zeros_like(hist), N_CLASSES)
    with torch.no_grad():
        hn, hp = torch_chain(feats[0], onehot[0], c1, c2)
    row["pairs"] = B * S ** 4
    row["positives_kernel"] = int(hk[:, 1].sum())
    row["positives_torch_chain"] = int(hp.sum().item())
    return row


def binning_error():
    """AP of the 4096-bin histogram minus AP of the unbinned float64 oracle scores (tests/corr_pr_oracle.py), one seeded input."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import corr_pr_oracle as P
    rng = np.random.default_rng(9)
    Bs, C, N = 2, 70, 400
    proto = rng.standard_normal((5, C))
    f = (np.einsum("brhw,rc->bchw", rng.standard_normal((Bs, 5, H, H)), proto) + 0.5 * rng.standard_normal((Bs, C, H, H))).astype(np.float32)
    lab = np.repeat(np.repeat(rng.integers(-1, 6, (Bs, RES // 16, RES // 16)), 16, 1), 16, 2).astype(np.int64)
    c1, c2 = [(rng.random((Bs, N, 2)) * 2 - 1).astype(np.float32) for _ in range(2)]
    o = P.net_fd(f, f, lab, lab, c1[:, :, None, :], c2[:, :, None, :], 6)
    t, tl = torch.from_numpy(f).to(DEV), torch.from_numpy(lab).to(DEV)
    hist = capi.pr_accumulate(t, t, tl, tl, torch.from_numpy(c1).to(DEV), torch.from_numpy(c2).to(DEV),
                              torch.zeros(N_BINS, 2, dtype=torch.int64, device=DEV), 6)
    ap_bins, ap_raw = P.pr_from_hist(hist.cpu().numpy())[3], P.ap_unbinned(o["fd"], o["target"])
    return {"pairs": int(o["target"].size), "positives": int(o["target"].sum()), "ap_4096_bins": ap_bins, "ap_unbinned_float64": ap_raw,
            "difference": ap_bins - ap_raw}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_pr needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "shape": "B=16 40x40 maps (channels-last), labels 320x320, 27 classes, 4096 bins, self pairs",
           "rows": {}}
    for C, name in ((768, "feats_c768"), (70, "code_c70")):
        for S in (11, 40):
            rec["rows"]["%s_S%d" % (name, S)] = one_shape(args, C, S)
            print(json.dumps({"%s_S%d" % (name, S): rec["rows"]["%s_S%d" % (name, S)]}), flush=True)
    slower = [k for k, r in rec["rows"].items() if k.endswith("S40") and r["speedup_vs_torch_chain"] < 1.0]
    rec["faster_than_torch_chain_at_S40"] = not slower
    rec["binning"] = binning_error()
    rec["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
