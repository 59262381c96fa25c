"""Times the fused ContrastiveCRFLoss call (csrc/crf_loss.hip), forward + backward, at the training shape - K = 70, code 28^2, image
224^2, grid 56^2, N = 1000, B = 16 and B = 32 - against the torch chain (crf_loss.torch_crf_mean_loss forward + backward) on the same
GPU in the same process, and the cached-token training_step of the trainer with crf_weight = 1 and cfg.native_crf_loss off and on.
Every call is timed on its own by a pair of device events; the median, the minimum and the maximum are reported.  Inputs rotate over
sets larger than the 256 MB Infinity Cache.  Also recorded: torch's peak allocated bytes for its chain, the call's workspace, and the
fraction of the 157.3 TFLOP/s fp32 matrix peak that the two GEMMs' 4 B N^2 K operations amount to at the measured time of the whole call
(three launches: they are not timed apart).

    python tools/bench_crf_loss.py --out profiles/crf_loss_bench.json
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stego_amd import capi  # noqa: E402
from stego_amd.crf_loss import crf_mean_loss, torch_crf_mean_loss  # noqa: E402

DEV = torch.device("cuda:0")
FP32_MFMA_PEAK = 157.3e12
PARAMS = (0.5, 0.15, 0.05, 10.0, 3.0, 0.0)


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


def call_and_chain(B, args):
    K, h, R, S, N = 70, 28, 224, 56, 1000
    g = torch.Generator(device=DEV).manual_seed(0)
    per_set = B * 3 * R * R * 4 + 2 * B * K * h * h * 4
    sets = max(2, -(-300 * 2 ** 20 // per_set) + 1)                 # rotate past the Infinity Cache
    imgs = [torch.randn(B, 3, R, R, device=DEV, generator=g) for _ in range(sets)]
    codes = [torch.randn(B, h, h, K, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(sets)]   # the head's channels-last view
    coords = [torch.randint(0, S, (2, N), device=DEV, generator=g) for _ in range(sets)]
    desc = capi.crf_loss_desc(B, K, 3, h, h, R, R, S, S, N, *PARAMS)
    nws = capi.crf_loss_workspace_bytes(desc)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    loss, per_image = torch.empty(1, device=DEV), torch.empty(B, device=DEV)
    d_codes = [torch.empty_like(c) for c in codes]
    gm, cm, dm = [capi._map(t) for t in imgs], [capi._map(t) for t in codes], [capi._map(t) for t in d_codes]
    stream = capi._stream()

    def raw(i):
        j = i % sets
        capi._check(capi.crf_loss_raw(desc, gm[j], cm[j], coords[j], loss, per_image, dm[j], ws, nws, stream))

    def raw_fwd(i):
        j = i % sets
        capi._check(capi.crf_loss_raw(desc, gm[j], cm[j], coords[j], loss, per_image, None, ws, nws, stream))

    leaves = [c.detach().requires_grad_(True) for c in codes]

    def autograd(fn):
        def run(i):
            j = i % sets
            leaves[j].grad = None
            fn(imgs[j], leaves[j], coords[j], (S, S), PARAMS, True).backward()
        return run

    row = {"fused_call": _stats(_each(raw, args.calls, args.warmup)),
           "fused_call_forward_only": _stats(_each(raw_fwd, args.calls, args.warmup)),
           "crf_mean_loss_fwd_bwd": _stats(_each(autograd(crf_mean_loss), args.calls, args.warmup))}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    row["torch_chain_fwd_bwd"] = _stats(_each(autograd(torch_crf_mean_loss), max(5, args.calls // 10), 3))
    row["torch_chain_peak_allocated_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    us = row["fused_call"]["us"]
    flops = 4.0 * B * N * N * K
    rc, launches = capi.crf_loss_plan(desc)
    row.update({"speedup_call_vs_torch": round(row["torch_chain_fwd_bwd"]["us"] / us, 2),
                "speedup_autograd_vs_torch": round(row["torch_chain_fwd_bwd"]["us"] / row["crf_mean_loss_fwd_bwd"]["us"], 2),
                "gemm_flops": flops, "frac_of_fp32_mfma_peak_whole_call": round(flops / FP32_MFMA_PEAK / (us * 1e-6), 4),
                "stage_breakdown": "the three launches are not timed apart",
                "workspace_bytes": nws, "launches_lds_bytes_workgroups": launches, "rotating_sets": sets})
    return row


def trainer_steps(args):
    """ms per cached-token training_step (B = 32 pairs, resident batches) with crf_weight = 1 and cfg.native_crf_loss off and on, the
    two trainers' steps alternating, every step between its own pair of events."""
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, Trainer, load_config
    warnings.simplefilter("ignore")
    models, batches = {}, None
    for native in (False, True):
        cfg = load_config(overrides=["batch_size=32", "cache_backbone_tokens=True", "native_backbone=True", "crf_weight=1.0",
                                     "native_crf_loss=%s" % native])
        torch.manual_seed(0)
        model = LitUnsupervisedSegmenter(27, cfg)
        loader = torch.utils.data.DataLoader(SyntheticContrastiveDataset(256, cfg.res, 27), batch_size=cfg.batch_size, shuffle=False,
                                             drop_last=True)
        tr = Trainer(max_steps=8, log_every=1000)
        tr.fit(model, loader)                      # builds the optimizers and the token cache and fills it for the 8 batches below
        if batches is None:
            batches = []
            for b in loader:
                batches.append({k: (v.to(tr.device) if torch.is_tensor(v) else v) for k, v in b.items()})
                if len(batches) == 8:
                    break
        for i in range(16):
            model.training_step(batches[i % 8], i)
        models[native] = model
    torch.cuda.synchronize()
    per = {False: [], True: []}
    for r in range(args.repeats):
        for native in (False, True):
            per[native] += [t / 1e3 for t in _each(lambda i: models[native].training_step(batches[i % 8], 100 + i), args.steps, 0)]
    off, on = _stats(per[False], "ms"), _stats(per[True], "ms")
    return {"shape": "B=32 pairs, vit_small/8 at 224, cached tokens, resident batches, crf_weight=1, crf_samples=1000",
            "native_crf_loss_off": off, "native_crf_loss_on": on, "on_minus_off_ms": round(on["ms"] - off["ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crf_loss needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0),
           "shape": "K=70 code 28x28 (channels-last), image 3x224x224, grid 56x56, N=1000, shipped parameters, normalised"}
    for B in (16, 32):
        rec["B%d" % B] = call_and_chain(B, args)
        print(json.dumps({"B": B, **rec["B%d" % B]}), flush=True)
    if not args.no_trainer:
        rec["training_step"] = trainer_steps(args)
    rec["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f)
            f.write("\n")


if __name__ == "__main__":
    main()
