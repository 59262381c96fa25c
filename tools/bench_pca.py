"""Times the feature pictures (csrc/feature_pca.hip) through stego_amd.feature_pca and, in the same process on the same GPU, the torch
chain of the same function (feature_pca.torch_feature_pictures), on the maps a user draws:

    vits8_224   B = 32, C = 384, 28 x 28 -> 224 x 224     ViT-S/8 features of a 224 batch
    vitb8_320   B = 16, C = 768, 40 x 40 -> 320 x 320     ViT-B/8 features of a 320 batch
    code_224    B = 32, C = 70,  28 x 28 -> 224 x 224     the segmentation code
    code_320    B = 16, C = 70,  40 x 40 -> 320 x 320

each fitted per image and jointly, and each with a fixed model (stages d - e only).  The maps are channels-last views, as the backbone
returns them.  Every call is timed on its own with a pair of device events; the inputs rotate over as many sets as it takes to walk
past the 256 MB Infinity Cache between two uses of the same set; the median, minimum and maximum of `--calls` calls are reported, and
the same for the three API calls of a picture on their own (fit, scores, paint).

    python tools/bench_pca.py --out profiles/pca_bench.json

The stages' kernels are timed by a kernel trace in a run of its own, which this tool only feeds:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_pca.py --trace vitb8_320:joint

With the kernels' times from that trace, `--kernel-us gram=..,paint=..` adds the Gram stage as a fraction of the 155 TF fp32 matrix
rate (2 N C^2 flops, N = B h w) and the picture stage as a fraction of the 6.29 TB/s copy rate (scores read, bytes written) to the
named case of an existing --out file.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stego_amd import capi, feature_pca  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE, MFMA_F32_RATE = 6.29e12, 155e12
CACHE = 256 << 20
SHAPES = {"vits8_224": (32, 384, 28, 224), "vitb8_320": (16, 768, 40, 320), "code_224": (32, 70, 28, 224), "code_320": (16, 70, 40, 320)}


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


def _maps(name):
    B, C, s, S = SHAPES[name]
    n_sets = min(max(2, -(-2 * CACHE // (B * C * s * s * 4))), 16)
    g = torch.Generator(device=DEV).manual_seed(len(name))
    return [torch.randn(B, s, s, C, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(n_sets)]


def counts(name):
    """What the algorithm needs: the flops of the full Gram product and the bytes of the picture stage."""
    B, C, s, S = SHAPES[name]
    return {"gram_flops": 2 * B * s * s * C * C, "paint_bytes": B * s * s * 3 * 4 + B * S * S * 3, "map_bytes": B * C * s * s * 4}


def bench_case(name, joint, args):
    B, C, s, S = SHAPES[name]
    maps = _maps(name)
    n = len(maps)
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=DEV)
    model = feature_pca.fit(maps[0], joint=joint)
    scores, rng = feature_pca._scores(model, maps[0])
    desc = capi.pca_desc(B, C, s, s, S, S, joint=joint, scale=capi.PCA_RANGE, out_strides=(out.stride(0), out.stride(1)))
    rec = {"shape": [B, C, s, s], "size": [S, S], "joint": joint, "input_sets": n, "calls": args.calls, **counts(name)}
    rec["picture"] = _us(_time(lambda i: feature_pca.feature_pictures(maps[i % n], (S, S), joint=joint, scale="range", out=out),
                               args.calls, args.warmup))
    rec["fixed_model"] = _us(_time(lambda i: feature_pca.feature_pictures(maps[i % n], (S, S), scale="range", pca=model, out=out),
                                   args.calls, args.warmup))
    rec["fit"] = _us(_time(lambda i: feature_pca.fit(maps[i % n], joint=joint), args.calls, args.warmup))
    rec["scores"] = _us(_time(lambda i: feature_pca._scores(model, maps[i % n]), args.calls, args.warmup))
    rec["paint"] = _us(_time(lambda i: capi.pca_paint(desc, scores, rng, out), args.calls, args.warmup))
    rec["residual_max"] = float(model.stats[..., 2].max())
    chain = _time(lambda i: feature_pca.torch_feature_pictures(maps[i % n], (S, S), joint=joint, scale="range"), args.chain_calls, 2)
    chain_fixed = _time(lambda i: feature_pca.torch_feature_pictures(maps[i % n], (S, S), scale="range", pca=model), args.chain_calls, 2)
    rec["torch_chain"] = {**_us(chain), "calls": args.chain_calls}
    rec["torch_chain_fixed_model"] = {**_us(chain_fixed), "calls": args.chain_calls}
    rec["speedup"] = round(chain[0] / rec["picture"]["us"], 2)
    rec["speedup_fixed_model"] = round(chain_fixed[0] / rec["fixed_model"]["us"], 2)
    return rec


def trace(case):
    """Twenty pictures of one case and nothing else: what a kernel trace is taken of."""
    name, mode = case.split(":")
    B, C, s, S = SHAPES[name]
    maps = _maps(name)
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=DEV)
    for i in range(20):
        feature_pca.feature_pictures(maps[i % len(maps)], (S, S), joint=mode == "joint", scale="range", out=out)
    torch.cuda.synchronize()


def add_kernel_times(path, case, spec):
    with open(path) as f:
        rec = json.load(f)
    us = {k: float(v) for k, v in (item.split("=") for item in spec.split(","))}
    c = rec[case]
    c["kernel_us"] = us
    if "gram" in us:
        c["gram_frac_of_f32_mfma_rate"] = round(c["gram_flops"] / MFMA_F32_RATE / (us["gram"] * 1e-6), 4)
    if "paint" in us:
        c["paint_frac_of_copy_rate"] = round(c["paint_bytes"] / COPY_RATE / (us["paint"] * 1e-6), 4)
    with open(path, "w") as f:
        json.dump(rec, f)
        f.write("\n")
    print(json.dumps({case: c}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--chain-calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default=",".join(SHAPES))
    ap.add_argument("--trace", default=None, help="NAME:joint or NAME:per_image - run that case alone, for a kernel trace")
    ap.add_argument("--kernel-us", default=None, help="gram=..,paint=.. (us, from a kernel trace) added to --case of --out")
    ap.add_argument("--case", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_us:
        return add_kernel_times(args.out, args.case, args.kernel_us)
    assert torch.cuda.is_available(), "bench_pca needs the MI355X"
    if args.trace:
        return trace(args.trace)
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12, "f32_mfma_TFs": MFMA_F32_RATE / 1e12}
    for name in args.cases.split(","):
        for joint in (False, True):
            key = "%s_%s" % (name, "joint" if joint else "per_image")
            rec[key] = bench_case(name, joint, args)
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
