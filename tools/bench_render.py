"""Times the render kernel (csrc/render.hip) through stego_amd.render and, in the same process on the same GPU, the torch chain of
the same functions (render.torch_colorize / torch_image_u8), on the shapes a user meets:

    colorize   16 x 320 x 320 int64 labels (a demo / evaluation batch), PASCAL colormap
    image_u8   16 x 3 x 320 x 320, rescaled to each image's own range (two launches for the range, one for the picture)
    overlay    the image under the cluster colours with edges, 16 x 320 x 320
    colorize and overlay on one 4800 x 4800 canvas (what segment_large returns for the aerial scene)

Every call is timed on its own with a pair of device events; the inputs rotate over as many sets as it takes to walk past the 256 MB
Infinity Cache between two uses of the same set; the median, minimum and maximum of `--calls` calls are reported.  The fraction of the
copy rate is the compulsory bytes (labels and image read once, the picture written once) over the median, against the measured
float4 copy rate of the MI355X this project uses throughout (6.29 TB/s).  The 320 x 320 cases move 13 - 38 MB and are bounded by
their launches, not by the memory; the canvas cases are the ones that can approach the copy rate.

    python tools/bench_render.py --out profiles/render_bench.json
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stego_amd import render  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE = 6.29e12
CACHE = 256 << 20


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


def bench_case(name, shape, kind, args, chain_calls):
    B, H, W = shape
    cmap = render.pascal_label_colormap()
    label_bytes = B * H * W * 8 if kind != "image" else 0
    image_bytes = B * 3 * H * W * 4 if kind != "colorize" else 0
    out_bytes = B * H * W * 3
    byts = label_bytes + image_bytes + out_bytes
    n_sets = max(2, -(-2 * CACHE // (label_bytes + image_bytes)))
    g = torch.Generator(device=DEV).manual_seed(len(name))
    labels = [torch.randint(0, 27, (B, H // 8 + 1, W // 8 + 1), device=DEV, generator=g).repeat_interleave(8, 1)
              .repeat_interleave(8, 2)[:, :H, :W].contiguous() for _ in range(n_sets)] if label_bytes else None
    images = [torch.randn(B, 3, H, W, device=DEV, generator=g) for _ in range(n_sets)] if image_bytes else None
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=DEV)

    def native(i):
        k = i % n_sets
        if kind == "colorize":
            render.colorize(labels[k], cmap, out=out)
        elif kind == "image":
            render.image_u8(images[k], out=out)
        else:
            render.colorize(labels[k], cmap, image=images[k], alpha=0.5, edges=True, out=out)

    def chain(i):
        k = i % n_sets
        if kind == "colorize":
            return render.torch_colorize(labels[k], cmap)
        if kind == "image":
            return render.torch_image_u8(images[k])
        return render.torch_colorize(labels[k], cmap, image=images[k], alpha=0.5, edges=True)

    k = 0
    same = torch.equal(chain(k), (native(k), out)[1]) if kind == "colorize" else None
    us, lo, hi = _time(native, args.calls, args.warmup)
    cus, clo, chi = _time(chain, chain_calls, 2)
    rec = {"shape": [B, H, W], "input_sets": n_sets, "compulsory_bytes": byts,
           "native": {"us": round(us, 1), "us_min": round(lo, 1), "us_max": round(hi, 1), "calls": args.calls,
                      "TBps": round(byts / (us * 1e-6) / 1e12, 3), "frac_of_copy_rate": round(byts / COPY_RATE / (us * 1e-6), 3)},
           "torch_chain": {"us": round(cus, 1), "us_min": round(clo, 1), "us_max": round(chi, 1), "calls": chain_calls},
           "speedup": round(cus / us, 2)}
    if same is not None:
        rec["equals_torch_chain"] = bool(same)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--chain-calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12}
    cases = (("colorize_16x320", (16, 320, 320), "colorize", args.chain_calls), ("image_u8_16x320", (16, 320, 320), "image", args.chain_calls),
             ("overlay_16x320", (16, 320, 320), "overlay", args.chain_calls),
             ("colorize_4800", (1, 4800, 4800), "colorize", 5), ("overlay_4800", (1, 4800, 4800), "overlay", 5))
    for name, shape, kind, chain_calls in cases:
        rec[name] = bench_case(name, shape, kind, args, chain_calls)
        print(json.dumps({"case": name, **rec[name]}), flush=True)
        torch.cuda.empty_cache()
    rec["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f)
            f.write("\n")


if __name__ == "__main__":
    main()
