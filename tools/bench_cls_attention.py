"""Times the class-token attention and the attention salience masks (csrc/vit_cls_attn.hip) and, in the same process on the same GPU, the
torch chain they replace, on the batches a user runs:

    vits8_224   ViT-S/8, B = 32, 224 x 224     (785 tokens, 6 heads)
    vitb8_320   ViT-B/8, B = 16, 320 x 320     (1601 tokens, 12 heads)

in both precisions of the native backbone.  Per case:
    forward_tokens / forward_tokens_attn   NativeViT, ALTERNATING call by call in one timed loop, so that both see the same clocks and the
                                           same neighbours; `spread` is what forward_tokens alone does between the two halves of its
                                           own calls (median of the even calls minus median of the odd ones) - a difference below it
                                           is not a difference
    salience                               stego_attn_salience alone (soft and mask), on the attention of the case
    torch_chain                            get_last_selfattention(img)[:, :, 0] of the fp32 torch module, then the torch restatement of
                                           the masks (salience.torch_attention_salience) - what a user had before; torch_salience is
                                           its second half alone
Every call is timed on its own with a pair of device events; the images rotate over as many sets as it takes to walk past the 256 MB
Infinity Cache between two uses of the same set; median, minimum and maximum are reported.

    python tools/bench_cls_attention.py --out profiles/cls_attention_bench.json

The attention kernel alone is timed by a kernel trace in a run of its own, which this tool only feeds:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_cls_attention.py --trace vits8_224:f16x3

`--kernel-us cls_attn=..,salience=..` adds the traced times and the attention kernel's fraction of the 6.29 TB/s copy rate (K read once,
the attention written) to the named case of an existing --out file.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stego_amd import dino_vit, salience, vit_native  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE = 6.29e12
CACHE = 256 << 20
SHAPES = {"vits8_224": ("vit_small", 32, 224), "vitb8_320": ("vit_base", 16, 320)}
KEEP = 0.6


def _events(fn, calls, warmup):
    """us of each of `calls` individually timed calls, in call order."""
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
    return per


def _us(per):
    s = sorted(per)
    return {"us": round(s[len(s) // 2], 1), "us_min": round(s[0], 1), "us_max": round(s[-1], 1)}


def _median(per):
    return sorted(per)[len(per) // 2]


def _setup(name):
    arch, B, res = SHAPES[name]
    torch.manual_seed(len(name))
    model = dino_vit.ARCHS[arch](patch_size=8, num_classes=0).to(DEV).eval()
    n_sets = min(max(2, -(-2 * CACHE // (B * 3 * res * res * 4))), 16)
    g = torch.Generator(device=DEV).manual_seed(len(name))
    return model, [torch.randn(B, 3, res, res, device=DEV, generator=g) for _ in range(n_sets)]


def counts(name, precision):
    """What the attention kernel needs: K read once (both planes in f16x3), the class query, the attention written."""
    arch, B, res = SHAPES[name]
    heads = {"vit_small": 6, "vit_base": 12}[arch]
    ntok = 1 + (res // 8) ** 2
    ntok_pad = -(-ntok // 64) * 64
    planes = 2 if precision == "f16x3" else 1
    return {"tokens": ntok, "heads": heads, "cls_attn_bytes": B * heads * (ntok * 128 * planes + 128 * planes + ntok * 4),
            "k_buffer_bytes": B * heads * ntok_pad * 128 * planes,
            "torch_attention_map_bytes": B * heads * ntok * ntok * 4}


def bench_case(name, precision, args):
    arch, B, res = SHAPES[name]
    model, imgs = _setup(name)
    n = len(imgs)
    nat = vit_native.NativeViT(model, precision=precision)
    hw = (res // 8, res // 8)
    rec = {"arch": arch, "batch": B, "res": res, "precision": precision, "input_sets": n, "calls": args.calls, **counts(name, precision)}
    # alternating: even calls forward_tokens, odd calls forward_tokens_attn - and the same loop with forward_tokens in both places
    both = _events(lambda i: nat.forward_tokens_attn(imgs[(i // 2) % n]) if i % 2 else nat.forward_tokens(imgs[(i // 2) % n]),
                   2 * args.calls, args.warmup)
    same = _events(lambda i: nat.forward_tokens(imgs[(i // 2) % n]), 2 * args.calls, args.warmup)
    rec["forward_tokens"] = _us(both[0::2])
    rec["forward_tokens_attn"] = _us(both[1::2])
    rec["difference_us"] = round(_median(both[1::2]) - _median(both[0::2]), 1)
    rec["spread_us"] = round(abs(_median(same[1::2]) - _median(same[0::2])), 1)
    rec["forward_tokens_run_to_run_us"] = round(abs(_median(same) - _median(both[0::2])), 1)
    attn = nat.forward_tokens_attn(imgs[0])[1]
    rec["salience"] = _us(_events(lambda i: salience.attention_salience(attn, hw, 8, KEEP), args.calls, args.warmup))
    rec["torch_salience"] = _us(_events(lambda i: salience.torch_attention_salience(attn, hw, 8, KEEP), args.chain_calls, 2))

    def chain(i):
        with torch.no_grad():
            row = model.get_last_selfattention(imgs[i % n])[:, :, 0]
        return salience.torch_attention_salience(row, hw, 8, KEEP)
    rec["torch_chain"] = {**_us(_events(chain, args.chain_calls, 2)), "calls": args.chain_calls}
    with torch.no_grad():
        rec["torch_forward_tokens"] = {**_us(_events(lambda i: model.get_intermediate_feat(imgs[i % n], n=1)[0][0], args.chain_calls, 2)),
                                       "calls": args.chain_calls}
    native = rec["forward_tokens_attn"]["us"] + rec["salience"]["us"]
    rec["native_attn_and_mask_us"] = round(native, 1)
    rec["speedup_vs_torch_chain"] = round(rec["torch_chain"]["us"] / native, 2)
    rec["salience_speedup_vs_torch"] = round(rec["torch_salience"]["us"] / rec["salience"]["us"], 2)
    return rec


def trace(case):
    """Twenty forwards with attention and twenty masks of one case and nothing else: what a kernel trace is taken of."""
    name, precision = case.split(":")
    arch, B, res = SHAPES[name]
    model, imgs = _setup(name)
    nat = vit_native.NativeViT(model, precision=precision)
    for i in range(20):
        attn = nat.forward_tokens_attn(imgs[i % len(imgs)])[1]
        salience.attention_salience(attn, (res // 8, res // 8), 8, KEEP)
    torch.cuda.synchronize()


def add_kernel_times(path, case, spec):
    with open(path) as f:
        rec = json.load(f)
    us = {k: float(v) for k, v in (item.split("=") for item in spec.split(","))}
    c = rec[case]
    c["kernel_us"] = us
    if "cls_attn" in us:
        c["cls_attn_frac_of_copy_rate"] = round(c["cls_attn_bytes"] / COPY_RATE / (us["cls_attn"] * 1e-6), 4)
    with open(path, "w") as f:
        json.dump(rec, f)
        f.write("\n")
    print(json.dumps({case: c}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--chain-calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--cases", default=",".join(SHAPES))
    ap.add_argument("--precisions", default="f16x3,f16")
    ap.add_argument("--trace", default=None, help="NAME:PRECISION - run that case alone, for a kernel trace")
    ap.add_argument("--kernel-us", default=None, help="cls_attn=..,salience=.. (us, from a kernel trace) added to --case of --out")
    ap.add_argument("--case", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_us:
        return add_kernel_times(args.out, args.case, args.kernel_us)
    assert torch.cuda.is_available(), "bench_cls_attention needs the MI355X"
    if args.trace:
        return trace(args.trace)
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12, "keep": KEEP}
    for name in args.cases.split(","):
        for precision in args.precisions.split(","):
            key = "%s_%s" % (name, precision)
            rec[key] = bench_case(name, precision, args)
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
