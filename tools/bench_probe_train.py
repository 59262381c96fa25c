"""Times the fused probe training call (csrc/probe_train.hip) at the training shape - K = 70, 28^2 -> 224^2, 27 + 27 labels, B = 16 and
B = 32 - against the torch chain of training_step on the same GPU (forward plus backward to the three parameter gradients), and
the cached-token training_step of the trainer with cfg.native_probes off and on.  Device events around each window of launches /
steps, `--repeats` windows, median / min / max reported; the two trainers' windows alternate.  Inputs rotate over sets larger than the
256 MB Infinity Cache.  Also recorded: the compulsory bytes of the call (labels + code + parameters and their gradients) and the
fraction of the 8 TB/s HBM peak they amount to at the measured time.

    python tools/bench_probe_train.py --out profiles/probe_train_bench.json
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
from stego_amd.featurizers import ClusterLookup  # noqa: E402
from stego_amd.probe_train import probe_losses, torch_probe_losses  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12


def _windows(fn, iters, warmup, repeats):
    """us per call of each of `repeats` windows of `iters` calls."""
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
    return per


def _stats(per, unit="us"):
    s = sorted(per)
    return {unit: round(s[len(s) // 2], 2), unit + "_min": round(s[0], 2), unit + "_max": round(s[-1], 2)}


def call_and_chain(B, args):
    K, h, H, n = 70, 28, 224, 27
    g = torch.Generator(device=DEV).manual_seed(0)
    per_set = B * H * H * 8 + B * K * h * h * 4
    sets = max(2, -(-300 * 2 ** 20 // per_set) + 1)                 # rotate past the Infinity Cache
    codes = [torch.randn(B, h, h, K, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(sets)]   # the head's channels-last view
    labels = [torch.randint(-1, n, (B, H, H), device=DEV, generator=g) for _ in range(sets)]
    lin = torch.nn.Conv2d(K, n, (1, 1)).to(DEV)
    clu = ClusterLookup(K, n).to(DEV)
    params = (lin.weight, lin.bias, clu.clusters)

    desc = capi.probe_train_desc(B, K, h, h, H, H, n, n)
    nws = capi.probe_train_workspace_bytes(desc)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    losses, n_valid = torch.empty(2, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV)
    dW, db, dC = torch.empty(n, K, device=DEV), torch.empty(n, device=DEV), torch.empty(n, K, device=DEV)
    Wm, bm, Cm = lin.weight.detach().reshape(n, K), lin.bias.detach(), clu.clusters.detach()
    maps = [capi._map(c) for c in codes]
    stream = capi._stream()

    def raw(i):
        capi._check(capi.probe_train_raw(desc, maps[i % sets], labels[i % sets], Wm, bm, Cm, losses, n_valid, dW, db, dC, ws, nws, stream))

    def autograd(fn):
        def run(i):
            for p in params:
                p.grad = None
            l, c = fn(codes[i % sets], labels[i % sets], lin, clu)
            (l + c).backward()
        return run

    row = {"fused_call": _stats(_windows(raw, args.iters, args.warmup, args.repeats)),
           "probe_losses_fwd_bwd": _stats(_windows(autograd(probe_losses), args.iters, args.warmup, args.repeats)),
           "torch_chain_fwd_bwd": _stats(_windows(autograd(torch_probe_losses), max(3, args.iters // 10), 3, args.repeats))}
    byts = per_set + 2 * (2 * n * K + n) * 4
    us = row["fused_call"]["us"]
    lds, wgs = capi.probe_train_plan(desc)
    row.update({"speedup_call_vs_torch": round(row["torch_chain_fwd_bwd"]["us"] / us, 2),
                "speedup_autograd_vs_torch": round(row["torch_chain_fwd_bwd"]["us"] / row["probe_losses_fwd_bwd"]["us"], 2),
                "compulsory_bytes": byts, "frac_of_8TBps": round(byts / HBM_PEAK / (us * 1e-6), 4),
                "stage_breakdown": "not broken down",
                "workspace_bytes": nws, "lds_bytes": lds, "workgroups": wgs,
                "rotating_sets": sets, "launches_per_window": args.iters, "windows": args.repeats})
    return row


def trainer_steps(args):
    """ms per cached-token training_step (B = 32 pairs, resident batches) with cfg.native_probes off and on, windows alternating."""
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, Trainer, load_config
    warnings.simplefilter("ignore")
    models, batches = {}, None
    for native in (False, True):
        cfg = load_config(overrides=["batch_size=32", "cache_backbone_tokens=True", "native_backbone=True", "native_probes=%s" % native])
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
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = {False: [], True: []}
    for _ in range(args.repeats):
        for native in (False, True):
            a.record()
            for i in range(args.steps):
                models[native].training_step(batches[i % 8], 100 + i)
            b.record()
            b.synchronize()
            per[native].append(a.elapsed_time(b) / args.steps)
    off, on = _stats(per[False], "ms"), _stats(per[True], "ms")
    return {"shape": "B=32 pairs, vit_small/8 at 224, cached tokens, resident batches", "steps_per_window": args.steps,
            "windows": args.repeats, "native_probes_off": off, "native_probes_on": on,
            "on_minus_off_ms": round(on["ms"] - off["ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_probe_train needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "shape": "K=70 28x28->224x224 n=27+27, channels-last code, labels randint(-1, 27)"}
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
