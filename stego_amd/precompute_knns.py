"""KNN precompute on the MI355X: the role of the reference's ``src/precompute_knns.py``.

  get_feats(model, loader)                      reference :15-21 (mean-pooled, L2-normalised features)
  compute_nearest_neighbors(normed_feats, k)    reference :86-96 (16 row blocks of einsum + topk) -> int64 [N, k];
                                                here ONE fused call, the [N, N] matrix is never materialised
  sharded_nearest_neighbors(local_feats, k)     SURVEY.md 8(e): rows sharded over the ranks of one node, one RCCL
                                                all-gather of the feature matrix, every rank answers its own rows
  save_nns(path, nns)                           the reference's file format: np.savez_compressed(..., nns=...)
  my_app(cfg)                                   reference :24-97 for the configured dataset and crop type:
                                                    python -m stego_amd.precompute_knns pytorch_data_dir=/data

The kernels live behind the C ABI (include/stego_corr.h: stego_knn_topk); there is no CPU path.
"""
import os
import random
import sys
from os.path import exists, join

import numpy as np
import torch
import torch.nn.functional as F

from . import capi

_backend = capi            # tests swap in an oracle-backed double (the product never does)


def get_feats(model, loader, device=None):
    """precompute_knns.py:15-21.  Stays on the device (the reference bounces every batch to the CPU)."""
    all_feats = []
    device = device or next(model.parameters()).device
    with torch.no_grad():
        for pack in loader:
            img = pack["img"]
            feats = F.normalize(model.forward(img.to(device)).mean([2, 3]), dim=1)
            all_feats.append(feats)
    return torch.cat(all_feats, dim=0).contiguous()


def compute_nearest_neighbors(normed_feats, k=30):
    """int64 [N, k], neighbours by descending cosine similarity (rank 0 is the row itself; data.py:524 skips it)."""
    return _backend.knn_topk(normed_feats.float(), k=k)


def shard_rows(n, world, rank):
    """Contiguous row shards whose starts are multiples of 128 (the kernel's query-block size)."""
    blocks = (n + 127) // 128
    per = (blocks + world - 1) // world
    b0 = min(blocks, rank * per)
    b1 = min(blocks, b0 + per)
    return min(n, b0 * 128), min(n, b1 * 128)


def sharded_nearest_neighbors(local_feats, k=30, group=None):
    """Every rank holds ``local_feats`` = its shard (``shard_rows`` of the global row order) of the normalised
    feature matrix.  One all-gather (RCCL over xGMI) rebuilds X on every rank, each rank answers its own rows and
    rank 0 receives the full [N, k] table (other ranks get None)."""
    import torch.distributed as dist
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    dev = local_feats.device
    counts = torch.zeros(world, dtype=torch.int64, device=dev)
    counts[rank] = local_feats.shape[0]
    dist.all_reduce(counts, group=group)
    counts = [int(c) for c in counts.tolist()]
    n, d = sum(counts), local_feats.shape[1]
    bounds = [shard_rows(n, world, r) for r in range(world)]
    if [b1 - b0 for b0, b1 in bounds] != counts:
        raise ValueError("local shards must follow shard_rows(): expected %s rows per rank, got %s" %
                         ([b1 - b0 for b0, b1 in bounds], counts))
    pad = max(counts)
    buf = torch.zeros(pad, d, dtype=torch.float32, device=dev)
    buf[:counts[rank]] = local_feats
    gathered = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(gathered, buf, group=group)
    x = torch.cat([g[:c] for g, c in zip(gathered, counts)], dim=0)
    q0, q1 = bounds[rank]
    mine = _backend.knn_topk(x, k=k, q_begin=q0, q_count=q1 - q0) if q1 > q0 else \
        torch.empty(0, k, dtype=torch.int64, device=dev)
    out = torch.full((pad, k), -1, dtype=torch.int64, device=dev)
    out[:mine.shape[0]] = mine
    parts = [torch.empty_like(out) for _ in range(world)] if rank == 0 else None
    dist.gather(out, parts, dst=0, group=group)
    if rank != 0:
        return None
    return torch.cat([p[:c] for p, c in zip(parts, counts)], dim=0)


def nns_filename(model_type, dataset_name, image_set, crop_type, res):
    """The cache file name data.py:503-511 looks up (precompute_knns.py:66-67)."""
    return "nns_{}_{}_{}_{}_{}.npz".format(model_type, dataset_name, image_set, crop_type, res)


def load_nns(path):
    """int64 [N, k] neighbour table (data.py:511: np.load(...)["nns"])."""
    return torch.from_numpy(np.load(path)["nns"])


def save_nns(path, nns):
    """Same on-disk format as the reference (:96): a compressed npz with the single key ``nns``."""
    np.savez_compressed(path, nns=nns.cpu().numpy() if torch.is_tensor(nns) else np.asarray(nns))


KNN_RES = 224           # the reference hard-codes the resolution of the precompute (:45), and the file name carries it
KNN_BATCH = 256         # :74


def _feature_model(cfg):
    """:49-58: the backbone's features, p[0] of DinoFeaturizer (dim does not matter), or the trunk without its last block."""
    import torch.nn as nn
    from .featurizers import DinoFeaturizer, LambdaLayer
    if cfg.arch == "dino":
        return nn.Sequential(DinoFeaturizer(20, cfg), LambdaLayer(lambda p: p[0]))
    from .trunks import load_model
    cut_model = load_model(cfg.model_type, join(cfg.output_root, "data"), allow_random_init=getattr(cfg, "allow_random_trunk", False))
    return nn.Sequential(*list(cut_model.children())[:-1])


def _split_loader(cfg, image_set, device):
    """The split's centre crops at KNN_RES in order, from the device store; on the CPU (ContrastiveSegDataset) when it does not fit."""
    from .data import ContrastiveSegDataset, image_transform, label_transform
    from .device_data import DeviceContrastiveLoader, DeviceImageStore, StoreTooLarge
    max_bytes = float(getattr(cfg, "device_dataset_max_gb", 200)) * 2 ** 30
    try:
        if cfg.dataset_name == "directory":
            # only the centre crops at KNN_RES are read: the store holds every image reduced to that resolution
            store = DeviceImageStore.from_directory(cfg.pytorch_data_dir, cfg.dir_dataset_name, image_set, device=device,
                                                    max_bytes=max_bytes, store_res=KNN_RES)
        else:
            store = DeviceImageStore(cfg.pytorch_data_dir, cfg.dataset_name, cfg.crop_type, cfg.crop_ratio, image_set, device=device,
                                     max_bytes=max_bytes)
        return DeviceContrastiveLoader(store, None, batch_size=KNN_BATCH, res=KNN_RES, drop_last=False)
    except StoreTooLarge as e:
        print("%s: reading it on the CPU" % e)
    ds = ContrastiveSegDataset(cfg.pytorch_data_dir, cfg.dataset_name, _crop_type(cfg), image_set, image_transform(KNN_RES),
                               label_transform(KNN_RES), cfg)
    return torch.utils.data.DataLoader(ds, KNN_BATCH, shuffle=False, num_workers=getattr(cfg, "num_workers", 0))


def _crop_type(cfg):
    """precompute_knns.py:43-45, :64 - an image folder (dataset_name "directory") has no crops: crop_type None, and the table's name
    carries cfg.dir_dataset_name and the literal "None"."""
    return None if cfg.dataset_name == "directory" else cfg.crop_type


def nns_path(cfg, image_set, res):
    """Where the neighbour table of a split lies: {pytorch_data_dir}/nns/nns_filename(...) with the reference's nice_dataset_name."""
    name = cfg.dir_dataset_name if cfg.dataset_name == "directory" else cfg.dataset_name
    return join(cfg.pytorch_data_dir, "nns", nns_filename(cfg.model_type, name, image_set, _crop_type(cfg), res))


def split_dir(cfg, image_set):
    """The folder that holds a split's images: the cropped tree's img/{split}, or {dir_dataset_name}/imgs/{split}."""
    from .data import crop_dir
    if cfg.dataset_name == "directory":
        return join(cfg.pytorch_data_dir, cfg.dir_dataset_name, "imgs", image_set)
    return join(crop_dir(cfg.pytorch_data_dir, cfg.dataset_name, cfg.crop_type, cfg.crop_ratio), "img", image_set)


def my_app(cfg):
    """precompute_knns.py:24-97 for cfg.dataset_name and cfg.crop_type: for the val and train splits of the cropped tree (or, for
    dataset_name "directory", of the image folder {pytorch_data_dir}/{dir_dataset_name}/imgs) whose table
    {pytorch_data_dir}/nns/nns_filename(...) does not exist yet, the mean-pooled, L2-normalised backbone features of the centre crops
    at 224 and their 30 nearest neighbours, written with save_nns.  The backbone runs in eval mode (the reference leaves the
    featurizer's feature dropout on).  Returns the paths written."""
    pytorch_data_dir = cfg.pytorch_data_dir
    os.makedirs(join(cfg.output_root, "data"), exist_ok=True)
    os.makedirs(join(cfg.output_root, "logs"), exist_ok=True)
    os.makedirs(join(pytorch_data_dir, "nns"), exist_ok=True)
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)                      # seed_everything(0)
    device = torch.device("cuda", torch.cuda.current_device())
    model = None
    written = []
    for image_set in ["val", "train"]:
        path = nns_path(cfg, image_set, KNN_RES)
        if exists(path):
            print("{} exists, skipping".format(path))
            continue
        if not exists(split_dir(cfg, image_set)):
            print("no {} {} split under {}: nothing to compute".format("directory" if cfg.dataset_name == "directory" else "cropped",
                                                                       image_set, pytorch_data_dir))
            continue
        print("{} not found, computing".format(path))
        if model is None:
            model = _feature_model(cfg).to(device).eval()
        with torch.no_grad():
            normed_feats = get_feats(model, _split_loader(cfg, image_set, device), device=device)
            print(tuple(normed_feats.shape))
            # a user's folder may hold fewer than 30 images (the cropped trees never do): then every image is a neighbour
            k = min(30, normed_feats.shape[0]) if cfg.dataset_name == "directory" else 30
            nearest_neighbors = compute_nearest_neighbors(normed_feats, k=k)
        save_nns(path, nearest_neighbors)
        print("Saved NNs", cfg.model_type, cfg.dataset_name, image_set)
        written.append(path)
    return written


if __name__ == "__main__":
    from .train_segmentation import load_config
    from .utils import prep_args
    prep_args()
    my_app(load_config(overrides=sys.argv[1:]))
