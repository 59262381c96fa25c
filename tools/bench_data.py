"""Input pipeline on real (synthetic-JPEG) cropped data: the batch-preparation kernel, the device loader, the CPU loader, and a
cached-token training step fed by each.  Prints one JSON line.

    python tools/bench_data.py [--sources 80] [--steps 40] [--cpu-workers 16]
    python tools/bench_data.py --directory      # stego_data_prepare_dir against stego_data_prepare -> profiles/data_dir_bench.json

The tree: `--sources` smooth random 640 x 480 images written with data.write_cropped (five 320 x 240 crops each) under a temporary
directory, and a random neighbour table.  Kernel times are CUDA-event means over back-to-back launches into preallocated outputs;
the roofline fraction counts the output bytes (21 per pixel) plus the source bytes read, against 8 TB/s."""
import argparse
import json
import os
import sys
import tempfile
import time
import types
from os.path import join

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stego_amd import capi  # noqa: E402
from stego_amd import data as D  # noqa: E402
from stego_amd import device_data as DD  # noqa: E402
from stego_amd.precompute_knns import nns_filename, save_nns  # noqa: E402

HBM_BYTES_PER_S = 8e12


def make_tree(root, n_src, seed=0):
    g = torch.Generator().manual_seed(seed)

    def items():
        for _ in range(n_src):
            low = torch.rand(3, 15, 20, generator=g)
            img = torch.nn.functional.interpolate(low[None], (480, 640), mode="bilinear", align_corners=False)[0]
            img = (img + 0.05 * torch.rand(3, 480, 640, generator=g)).clamp(0, 1)
            lab = torch.nn.functional.interpolate(torch.randint(-1, 27, (1, 1, 15, 20), generator=g).float(), (480, 640))[0, 0].long()
            yield img, lab
    n = D.write_cropped(root, "cocostuff27", "five", 0.5, "train", items())
    rng = np.random.default_rng(seed)
    nns = np.stack([np.concatenate([[i], rng.permutation(np.delete(np.arange(n), i))[:29]]) for i in range(n)]).astype(np.int64)
    os.makedirs(join(root, "nns"), exist_ok=True)
    save_nns(join(root, "nns", nns_filename("vit_small", "cocostuff27", "train", "five", 224)), nns)
    return n, nns


def time_kernel(store, n_items, R=224, iters=200, directory=False):
    """directory=True: stego_data_prepare_dir (float32 mask, 24 output bytes per pixel) on the same arenas and records."""
    dev = store.device
    t = store.table(R)
    ind = torch.randint(0, len(store), (n_items,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    img = torch.empty(n_items, 3, R, R, device=dev)
    label = torch.empty(n_items, R, R, dtype=torch.int64, device=dev)
    mask = torch.empty(n_items, 1, R, R, dtype=torch.float32 if directory else torch.bool, device=dev)
    desc = capi.data_desc(n_items, *t["desc"])
    args = (desc, t["items"], store.images, store.labels, t["maps"], store.lut, ind, None, img, label, mask)
    run = capi.data_prepare_dir_raw if directory else capi.data_prepare_raw
    out_bytes = 24.0 if directory else 21.0
    for _ in range(10):
        assert run(*args) == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run(*args)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    rec = t["records"][ind.cpu().numpy()]
    src = float((rec["h"].astype(np.int64) * rec["w"] * 4).sum())      # upper bound: every source byte of the items read once
    nbytes = out_bytes * R * R * n_items + min(src, 4.0 * R * R * n_items)
    return dict(items=n_items, R=R, us=round(us, 2), out_mb=round(out_bytes * R * R * n_items / 1e6, 2),
                roofline_frac=round(nbytes / (us * 1e-6) / HBM_BYTES_PER_S, 3))


def directory_main(a):
    """--directory: stego_data_prepare_dir against stego_data_prepare on the same arenas, records and indices in one process, each
    timed twice in alternation (the order of two back-to-back measurements can matter) -> profiles/data_dir_bench.json."""
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as root:
        n, _ = make_tree(root, a.sources)
        store = DD.DeviceImageStore(root, "cocostuff27", "five", 0.5, "train", device=dev)
    rows = []
    for b in (16, 32):
        runs = [(time_kernel(store, 2 * b), time_kernel(store, 2 * b, directory=True)) for _ in range(2)]
        base, dirs = min(r[0]["us"] for r in runs), min(r[1]["us"] for r in runs)
        rows.append(dict(items=2 * b, R=224, prepare_us=[r[0]["us"] for r in runs], prepare_dir_us=[r[1]["us"] for r in runs],
                         ratio_of_best=round(dirs / base, 3), output_bytes_ratio=round(24 / 21, 3),
                         prepare_dir_roofline_frac=max(r[1]["roofline_frac"] for r in runs)))
    result = dict(tool="bench_data --directory", crops=n, crop_hw=[240, 320], rows=rows)
    out = join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "data_dir_bench.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def loader_rate(it, n_batches, sync):
    b = next(it)                     # (worker start-up / first table build excluded)
    sync()
    t0 = time.perf_counter()
    for _ in range(n_batches):
        b = next(it)
    sync()
    return n_batches / (time.perf_counter() - t0), b


def cycle(make):
    while True:
        for b in make():
            yield b


def step_ms(batches, n_items, steps, warm):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    dev = torch.device("cuda", 0)
    cfg = load_config(overrides=["cache_backbone_tokens=True", "pretrained_weights=~", "batch_size=16", "res=224"])
    model = LitUnsupervisedSegmenter(27, cfg).to(dev).train()
    model.net.enable_token_cache(n_items, (224, 224), dev)
    for i in range(warm):
        b = {k: v.to(dev, non_blocking=True) for k, v in next(batches).items()}
        model.training_step(b, i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        b = {k: v.to(dev, non_blocking=True) for k, v in next(batches).items()}
        model.training_step(b, i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=80)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--cpu-workers", type=int, default=16)
    ap.add_argument("--directory", action="store_true", help="time stego_data_prepare_dir against stego_data_prepare on the same bytes")
    a = ap.parse_args()
    if a.directory:
        return directory_main(a)
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as root:
        n, nns = make_tree(root, a.sources)
        t0 = time.perf_counter()
        store = DD.DeviceImageStore(root, "cocostuff27", "five", 0.5, "train", device=dev)
        load_s = time.perf_counter() - t0
        kernel = [time_kernel(store, 2 * b) for b in (16, 32)]
        dl = DD.DeviceContrastiveLoader(store, nns, 16, 7, 224, seed=0)
        dev_rate, _ = loader_rate(cycle(lambda: iter(dl)), a.steps, torch.cuda.synchronize)
        cfg = types.SimpleNamespace(crop_ratio=0.5, model_type="vit_small", res=224)
        ds = D.ContrastiveSegDataset(root, "cocostuff27", "five", "train", D.image_transform(224), D.label_transform(224), cfg,
                                     num_neighbors=7, mask=True, pos_images=True, pos_labels=True)
        cl = torch.utils.data.DataLoader(ds, 16, shuffle=True, num_workers=a.cpu_workers, drop_last=True, pin_memory=True,
                                         persistent_workers=True, prefetch_factor=4)
        cpu_rate, _ = loader_rate(cycle(lambda: iter(cl)), min(a.steps, 2 * len(cl)), lambda: None)
        warm = 2 * len(dl) + 2                                        # the token table is full after this
        dev_step = step_ms(cycle(lambda: iter(dl)), n, a.steps, warm)
        cpu_step = step_ms(cycle(lambda: iter(cl)), n, min(a.steps, len(cl)), warm)
    print(json.dumps(dict(tool="bench_data", crops=n, crop_hw=[240, 320], store_load_s=round(load_s, 2),
                          store_gb=round(store.nbytes / 1e9, 3), prep_kernel=kernel,
                          device_loader_batches_per_s=round(dev_rate, 1), cpu_loader_batches_per_s=round(cpu_rate, 1),
                          cpu_workers=a.cpu_workers, batch_size=16,
                          ms_per_step_cached_device_loader=round(dev_step, 3), ms_per_step_cached_cpu_loader=round(cpu_step, 3))))


if __name__ == "__main__":
    main()
