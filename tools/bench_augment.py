"""Times the device-side augmentation and the fused aug-alignment loss (csrc/augment.hip):

  stego_augment      B = 16 and 32, 224^2 -> 224^2, drawn parameters (every image has contrast: both launches run), against its own
                     byte count (image read once, img_aug and coord_aug written) at the 6.29 TB/s copy rate measured on this device
  stego_aug_align    K = 70, code 28^2 (channels-last), coord 224^2, forward + backward, against the torch chain
                     (augment.torch_aug_alignment forward + backward) on the same GPU in the same process
  training_step      the cached-token step with aug_alignment_weight = 0.5 on batches that carry img_aug / coord_aug, with
                     cfg.native_aug on (the fused term) and off (the torch chain)

Every call is timed on its own by a pair of device events; the median, the minimum and the maximum are reported.  Inputs rotate over
sets larger than the 256 MB Infinity Cache.  The two launches of either call are not timed apart.

    python tools/bench_augment.py --out profiles/augment_bench.json
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
from stego_amd.augment import aug_alignment_loss, augment_batch, draw_aug_params, torch_aug_alignment  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE = 6.29e12


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


def augment_call(B, args):
    R = 224
    g = torch.Generator(device=DEV).manual_seed(0)
    per_set = B * R * R * 4 * (3 + 3 + 2)
    sets = max(2, -(-300 * 2 ** 20 // per_set) + 1)                 # rotate past the Infinity Cache
    imgs = [torch.randn(B, 3, R, R, device=DEV, generator=g) for _ in range(sets)]
    outs = [(torch.empty(B, 3, R, R, device=DEV), torch.empty(B, R, R, 2, device=DEV)) for _ in range(sets)]
    table = draw_aug_params(B, R, R, R, torch.Generator().manual_seed(1))
    dev_table = capi.aug_table(table, DEV)
    desc = capi.aug_desc(B, R, R, R)
    nws = capi.augment_workspace_bytes(desc)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=DEV)
    maps = [capi._map(t) for t in imgs]
    stream = capi._stream()

    def raw(i):
        j = i % sets
        capi._check(capi.augment_raw(desc, maps[j], table, dev_table, outs[j][0], outs[j][1], ws, nws, stream))

    def whole(i):
        augment_batch(imgs[i % sets], table)                        # with the upload of the table and the allocations

    row = {"fused_call": _stats(_each(raw, args.calls, args.warmup)), "augment_batch": _stats(_each(whole, args.calls, args.warmup))}
    us = row["fused_call"]["us"]
    rc, launches = capi.augment_plan(desc)
    row.update({"bytes": per_set, "us_at_copy_rate": round(per_set / COPY_RATE * 1e6, 2),
                "frac_of_copy_rate": round(per_set / COPY_RATE / (us * 1e-6), 3), "launches_lds_bytes_workgroups": launches,
                "blurred_images": sum(1 for r in table if r.blur_sigma > 0), "stage_breakdown": "the two launches are not timed apart",
                "rotating_sets": sets})
    return row


def align_call(B, args):
    K, h, S, R = 70, 28, 28, 224
    g = torch.Generator(device=DEV).manual_seed(0)
    per_set = 2 * B * K * h * h * 4 + B * R * R * 2 * 4
    sets = max(2, -(-300 * 2 ** 20 // per_set) + 1)
    codes = [torch.randn(B, h, h, K, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(sets)]      # the head's channels-last view
    augs = [torch.randn(B, S, S, K, device=DEV, generator=g).permute(0, 3, 1, 2) for _ in range(sets)]
    imgs = torch.randn(B, 3, R, R, device=DEV, generator=g)
    coords = [augment_batch(imgs, draw_aug_params(B, R, R, R, torch.Generator().manual_seed(s)))[1] for s in range(sets)]
    desc = capi.aug_align_desc(B, K, h, h, S, R, R)
    nws = capi.aug_align_workspace_bytes(desc)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    loss = torch.empty(1, device=DEV)
    d1, d2 = [torch.empty_like(c) for c in codes], [torch.empty_like(c) for c in augs]
    cm, am, d1m, d2m = ([capi._map(t) for t in ts] for ts in (codes, augs, d1, d2))
    stream = capi._stream()

    def raw(i):
        j = i % sets
        capi._check(capi.aug_align_raw(desc, cm[j], am[j], coords[j], loss, d1m[j], d2m[j], ws, nws, stream))

    def raw_fwd(i):
        j = i % sets
        capi._check(capi.aug_align_raw(desc, cm[j], am[j], coords[j], loss, None, None, ws, nws, stream))

    leaves = [(c.detach().requires_grad_(True), a.detach().requires_grad_(True)) for c, a in zip(codes, augs)]

    def autograd(fn):
        def run(i):
            j = i % sets
            leaves[j][0].grad = leaves[j][1].grad = None
            fn(leaves[j][0], leaves[j][1], coords[j]).backward()
        return run

    row = {"fused_call": _stats(_each(raw, args.calls, args.warmup)),
           "fused_call_forward_only": _stats(_each(raw_fwd, args.calls, args.warmup)),
           "aug_alignment_loss_fwd_bwd": _stats(_each(autograd(aug_alignment_loss), args.calls, args.warmup))}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    row["torch_chain_fwd_bwd"] = _stats(_each(autograd(torch_aug_alignment), max(5, args.calls // 5), 3))
    row["torch_chain_peak_allocated_bytes"] = int(torch.cuda.max_memory_allocated() - base)
    rc, launches = capi.aug_align_plan(desc)
    row.update({"speedup_call_vs_torch": round(row["torch_chain_fwd_bwd"]["us"] / row["fused_call"]["us"], 2),
                "speedup_autograd_vs_torch": round(row["torch_chain_fwd_bwd"]["us"] / row["aug_alignment_loss_fwd_bwd"]["us"], 2),
                "workspace_bytes": nws, "launches_lds_bytes_workgroups": launches, "rotating_sets": sets,
                "stage_breakdown": "the two launches are not timed apart"})
    return row


def trainer_steps(args):
    """ms per cached-token training_step (B = 32 pairs, resident batches that carry img_aug / coord_aug) with aug_alignment_weight = 0.5
    and cfg.native_aug off and on, the two trainers' steps alternating, every step between its own pair of events."""
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, Trainer, load_config
    warnings.simplefilter("ignore")
    models, batches = {}, None
    for native in (False, True):
        base = ["batch_size=32", "cache_backbone_tokens=True", "native_backbone=True"]
        cfg = load_config(overrides=base)
        torch.manual_seed(0)
        model = LitUnsupervisedSegmenter(27, cfg)
        loader = torch.utils.data.DataLoader(SyntheticContrastiveDataset(256, cfg.res, 27), batch_size=cfg.batch_size, shuffle=False,
                                             drop_last=True)
        tr = Trainer(max_steps=8, log_every=1000)
        tr.fit(model, loader)                      # builds the optimizers and the token cache and fills it for the 8 batches below
        if batches is None:
            batches = []
            for s, b in enumerate(loader):
                b = {k: (v.to(tr.device) if torch.is_tensor(v) else v) for k, v in b.items()}
                b["img_aug"], b["coord_aug"] = augment_batch(b["img"], draw_aug_params(32, cfg.res, cfg.res, cfg.res, torch.Generator().manual_seed(s)))
                batches.append(b)
                if len(batches) == 8:
                    break
        model.cfg.aug_alignment_weight, model.cfg.native_aug = 0.5, native
        for i in range(16):
            model.training_step(batches[i % 8], i)
        models[native] = model
    torch.cuda.synchronize()
    per = {False: [], True: []}
    for r in range(args.repeats):
        for native in (False, True):
            per[native] += [t / 1e3 for t in _each(lambda i: models[native].training_step(batches[i % 8], 100 + i), args.steps, 0)]
    off, on = _stats(per[False], "ms"), _stats(per[True], "ms")
    return {"shape": "B=32 pairs, vit_small/8 at 224, cached tokens for img / img_pos, a third backbone pass over img_aug, resident "
                     "batches with img_aug / coord_aug, aug_alignment_weight=0.5",
            "native_aug_off": off, "native_aug_on": on, "on_minus_off_ms": round(on["ms"] - off["ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_augment needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0),
           "shape": "augment: 3x224x224 -> 224^2, drawn parameters; aug_align: K=70 code 28x28 and code_aug 28x28 (channels-last), coord 224x224"}
    for B in (16, 32):
        rec["augment_B%d" % B] = augment_call(B, args)
        print(json.dumps({"augment_B": B, **rec["augment_B%d" % B]}), flush=True)
    for B in (16, 32):
        rec["aug_align_B%d" % B] = align_call(B, args)
        print(json.dumps({"aug_align_B": B, **rec["aug_align_B%d" % B]}), flush=True)
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
