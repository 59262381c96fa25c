"""Times the fused probe head (csrc/probe_head.hip) at the eval shape - B = 16, K = 70, 40^2 -> 320^2, 27 + 27 labels, flip on - in
each output kind, against the reference's torch chain on the same GPU (flip average, F.interpolate, the linear probe, ClusterLookup,
log_softmax, then crf._probs_at's softmax per probe), and the demo loop's images/s split into backbone, head and CRF with random
ViT-B/8 weights at 320.  Kernel outputs rotate over sets larger than the 256 MB Infinity Cache; device events around each window of
`--iters` launches, `--repeats` windows, median / min / max reported.  The demo loop runs on two kinds of image: per-pixel noise (the
CRF's worst case: the bilateral lattice has ~6 vertices per pixel) and a smooth synthetic scene (gradients and flat blocks, closer to
photographs); it starts from normalised device tensors, so JPEG decoding and the CPU preprocessing are not in it.

    python tools/bench_probe_head.py --out profiles/probe_head_bench_b16_320.json
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stego_amd import capi  # noqa: E402
from stego_amd.crf import _probs_at, dense_crf_batch, image_to_bgr_u8  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12


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


def kernel_and_chain(args):
    B, K, h, H, n = 16, 70, 40, 320, 27
    g = torch.Generator(device=DEV).manual_seed(0)
    code = torch.randn(B, h, h, K, device=DEV, generator=g).permute(0, 3, 1, 2)        # the head's channels-last view
    flip = torch.randn(B, h, h, K, device=DEV, generator=g).permute(0, 3, 1, 2)
    W = torch.randn(n, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(n, device=DEV, generator=g) * 0.1
    cent = F.normalize(torch.randn(n, K, device=DEV, generator=g), dim=1)
    lk = {"log_probs": capi.PROBE_LOG_PROBS, "probs": capi.PROBE_PROBS, "argmax": capi.PROBE_ARGMAX}
    code_bytes = 2 * B * K * h * h * 4
    rows = {}
    for kind in ("probs", "log_probs", "argmax"):
        per = B * H * H * (8 if kind == "argmax" else 4 * n) * 2
        sets = max(2, -(-300 * 2 ** 20 // per) + 1)                 # rotate past the Infinity Cache
        outs = [[torch.empty(B, H, H, dtype=torch.int64, device=DEV) if kind == "argmax" else
                 torch.empty(B, n, H, H, device=DEV) for _ in range(2)] for _ in range(sets)]
        desc = capi.probe_desc(B, K, h, h, H, H, n, n, lk[kind], lk[kind], 2.0)
        cm, fm = capi._map(code), capi._map(flip)
        stream = capi._stream()

        def run(i):
            o = outs[i % sets]
            capi._check(capi.probe_head_raw(desc, cm, fm, W, b, cent, o[0], o[1], stream))
        us, lo, hi = _time(run, args.iters, args.warmup, args.repeats)
        byts = code_bytes + per
        rows[kind] = {"us": round(us, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "compulsory_bytes": byts,
                      "frac_of_8TBps": round(byts / HBM_PEAK / (us * 1e-6), 3), "TBps": round(byts / (us * 1e-6) / 1e12, 3),
                      "rotating_sets": sets, "launches_per_window": args.iters, "windows": args.repeats}

    lin = torch.nn.Conv2d(K, n, 1).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(W[:, :, None, None])
        lin.bias.copy_(b)
    clusters = torch.randn(n, K, device=DEV, generator=g)

    def chain(i):
        with torch.no_grad():
            c = (code + flip.flip(dims=[3])) / 2
            c = F.interpolate(c, (H, H), mode="bilinear", align_corners=False)
            lp = torch.log_softmax(lin(c), dim=1)
            inner = torch.einsum("bchw,nc->bnhw", F.normalize(c, dim=1), F.normalize(clusters, dim=1))
            cp = F.log_softmax(inner * 2, dim=1)
            return _probs_at(lp, H, H), _probs_at(cp, H, H)
    chain_us, lo, hi = _time(chain, max(3, args.iters // 10), 2, args.repeats)
    rows["torch_chain_to_probs"] = {"us": round(chain_us, 2), "us_min": round(lo, 2), "us_max": round(hi, 2)}
    rows["speedup_probs_vs_torch"] = round(chain_us / rows["probs"]["us"], 2)
    return rows


def _smooth_images(B, R, seed):
    """Normalised [B, 3, R, R] images of gradients with flat coloured blocks (tests/test_crf_gpu.py's smooth scene, in colour)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(R, dtype=torch.float32), torch.arange(R, dtype=torch.float32), indexing="ij")
    imgs = []
    for _ in range(B):
        im = torch.stack([xx / (R - 1), yy / (R - 1), torch.full_like(xx, 0.5)])
        for _ in range(6):
            y0, x0 = torch.randint(0, R - R // 4, (2,), generator=g).tolist()
            hh, ww = torch.randint(R // 8, R // 3, (2,), generator=g).tolist()
            im[:, y0:y0 + hh, x0:x0 + ww] = torch.rand(3, 1, 1, generator=g)
        imgs.append(im)
    x = torch.stack(imgs)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return ((x - mean) / std).to(DEV)


def demo_loop(args):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=["model_type=vit_base", "dino_patch_size=8", "res=320", "dim=70", "dropout=False"])
    torch.manual_seed(0)
    model = LitUnsupervisedSegmenter(27, cfg).to(DEV).eval()
    out = {}
    for scene, img in (("noise", torch.randn(16, 3, 320, 320, device=DEV)), ("smooth", _smooth_images(16, 320, 0))):
        out[scene] = _demo_stages(model, img, args.demo_iters)
    return out


def _demo_stages(model, img, n):
    from stego_amd.segment import probe_head
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    tot = [0.0, 0.0, 0.0]
    with torch.no_grad():
        for it in range(n + 2):
            ev[0].record()
            _, c1 = model.net(img)
            _, c2 = model.net(img.flip(dims=[3]))
            ev[1].record()
            pl, pc = probe_head(model, c1, c2, (320, 320), linear="probs", cluster="probs")
            ev[2].record()
            bgr = image_to_bgr_u8(img)
            dense_crf_batch(bgr, pl).argmax(1)
            dense_crf_batch(bgr, pc).argmax(1)
            ev[3].record()
            ev[3].synchronize()
            if it >= 2:
                for s in range(3):
                    tot[s] += ev[s].elapsed_time(ev[s + 1])
    ms = [t / n for t in tot]
    return {"images": 16, "backbone_ms": round(ms[0], 3), "head_ms": round(ms[1], 3), "crf_ms": round(ms[2], 3),
            "images_per_s": round(16 / (sum(ms) * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--demo-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_probe_head needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "shape": "B=16 K=70 40x40->320x320 n=27+27 flip", "kernel": kernel_and_chain(args)}
    print(json.dumps(rec["kernel"]), flush=True)
    rec["demo_loop_vitb8_320_from_device_tensors"] = demo_loop(args)
    rec["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f)
            f.write("\n")


if __name__ == "__main__":
    main()
