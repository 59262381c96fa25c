"""Times the fused reconstruction loss call (csrc/rec_loss.hip), forward + backward and forward only, against the torch chain
(rec_loss.torch_rec_loss forward + backward) on the same GPU in the same process, at K = 70, C = 384, 28^2 with B = 32 and B = 16 and at
K = 70, C = 768, 40^2 with B = 16.  feats is the channels-last view that skips the class token, code the head's channels-last map.
Every call is timed on its own by a pair of device events; the median, the minimum and the maximum are reported.  Inputs rotate over
sets larger than the 256 MB Infinity Cache.  Reported with each time: the fraction of the 157.3 TFLOP/s fp32 matrix peak that the
6 T K C operations of the three contractions amount to, the fraction of the 6.29 TB/s copy rate over the bytes the call must move
(feats once, code, d_code, the decoder and its gradients), the workspace and torch's peak allocated bytes for its chain.

The cached-token training_step with rec_weight = 1 and the flag off and on is timed by tools/exp/trainer_step_time.py in fresh
processes (rec_weight=1.0 native_rec_loss=False / True); --steps FILE ... folds such outputs (flag off, on, off, on, ...) into the record.

    python tools/bench_rec_loss.py --out profiles/rec_loss_bench.json
"""
import argparse
import json
import os
import re
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stego_amd import capi  # noqa: E402
from stego_amd.rec_loss import rec_loss, torch_rec_loss  # noqa: E402

DEV = torch.device("cuda:0")
FP32_MFMA_PEAK = 157.3e12
COPY_RATE = 6.29e12
SHAPES = [(32, 70, 384, 28), (16, 70, 384, 28), (16, 70, 768, 40)]


def _each(fn, calls, warmup):
    """us of each of `calls` calls, every one between its own pair of events."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i)
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def _stats(per, unit="us"):
    s = sorted(per)
    return {unit: round(s[len(s) // 2], 2), unit + "_min": round(s[0], 2), unit + "_max": round(s[-1], 2), "calls": len(s)}


def call_and_chain(B, K, C, h, args):
    g = torch.Generator(device=DEV).manual_seed(0)
    hw = h * h
    per_set = B * (1 + hw) * C * 4 + 2 * B * hw * K * 4
    sets = max(2, -(-300 * 2 ** 20 // per_set) + 1)                 # rotate past the Infinity Cache
    feats = [torch.randn(B, 1 + hw, C, device=DEV, generator=g)[:, 1:].reshape(B, h, h, C).permute(0, 3, 1, 2) for _ in range(sets)]
    codes = [torch.randn(B, h, h, K, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(sets)]
    dec = nn.Conv2d(K, C, 1).to(DEV)
    weight, bias = dec.weight.detach(), dec.bias.detach()
    desc = capi.rec_desc(B, K, C, h, h)
    nws = capi.rec_loss_workspace_bytes(desc)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    loss = torch.empty(1, device=DEV)
    d_codes = [torch.empty_like(c) for c in codes]
    d_weight, d_bias = torch.empty_like(weight), torch.empty_like(bias)
    fm, cm, dm = [capi._map(t) for t in feats], [capi._map(t) for t in codes], [capi._map(t) for t in d_codes]
    stream = capi._stream()

    def raw(i):
        j = i % sets
        capi._check(capi.rec_loss_raw(desc, cm[j], fm[j], weight, bias, loss, dm[j], d_weight, d_bias, ws, nws, stream))

    def raw_fwd(i):
        j = i % sets
        capi._check(capi.rec_loss_raw(desc, cm[j], fm[j], weight, bias, loss, None, None, None, ws, nws, stream))

    leaves = [c.detach().requires_grad_(True) for c in codes]

    def autograd(fn):
        def run(i):
            j = i % sets
            leaves[j].grad = dec.weight.grad = dec.bias.grad = None
            fn(leaves[j], feats[j], dec).backward()
        return run

    row = {"fused_call": _stats(_each(raw, args.calls, args.warmup)),
           "fused_call_forward_only": _stats(_each(raw_fwd, args.calls, args.warmup)),
           "rec_loss_fwd_bwd": _stats(_each(autograd(rec_loss), args.calls, args.warmup))}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    row["torch_chain_fwd_bwd"] = _stats(_each(autograd(torch_rec_loss), max(5, args.calls // 2), 5))
    row["torch_chain_peak_allocated_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    us = row["fused_call"]["us"]
    T = B * hw
    flops = 6.0 * T * K * C
    must_move = 4.0 * (T * C + 2 * T * K + 2 * (C * K + C))
    rc, launches = capi.rec_loss_plan(desc)
    row.update({"speedup_call_vs_torch": round(row["torch_chain_fwd_bwd"]["us"] / us, 2),
                "speedup_autograd_vs_torch": round(row["torch_chain_fwd_bwd"]["us"] / row["rec_loss_fwd_bwd"]["us"], 2),
                "gemm_flops": flops, "frac_of_fp32_mfma_peak": round(flops / FP32_MFMA_PEAK / (us * 1e-6), 4),
                "must_move_bytes": must_move, "frac_of_copy_rate": round(must_move / COPY_RATE / (us * 1e-6), 4),
                "floor_us_mfma": round(flops / FP32_MFMA_PEAK * 1e6, 2), "floor_us_bytes": round(must_move / COPY_RATE * 1e6, 2),
                "stage_breakdown": "the two launches are not timed apart",
                "workspace_bytes": nws, "feats_bytes": 4 * T * C, "launches_lds_bytes_workgroups": launches, "rotating_sets": sets})
    return row


def fold_steps(paths):
    """The wall ms per step that tools/exp/trainer_step_time.py printed into each file, in the order given: the runs alternate,
    native_rec_loss off first."""
    out = []
    for i, p in enumerate(paths):
        m = re.search(r"wall ([0-9.]+) ms per step", open(p).read())
        out.append({"process": i + 1, "native_rec_loss": bool(i % 2), "wall_ms_per_step": float(m.group(1)) if m else None})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rec_loss needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0),
           "shape": "code channels-last, feats the channels-last view that skips the class token, nn.Conv2d default init"}
    for B, K, C, h in SHAPES:
        key = "B%d_K%d_C%d_%dx%d" % (B, K, C, h, h)
        rec[key] = call_and_chain(B, K, C, h, args)
        print(json.dumps({"shape": key, **rec[key]}), flush=True)
    if args.steps:
        rec["training_step_rec_weight_1"] = fold_steps(args.steps)
    rec["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f)
            f.write("\n")


if __name__ == "__main__":
    main()
