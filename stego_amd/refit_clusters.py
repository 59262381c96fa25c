"""Refit a checkpoint's cluster probe for other cluster counts, on a folder of the user's own images or on the checkpoint's dataset.

    python -m stego_amd.refit_clusters model_path=run.ckpt image_dir=my_images n_clusters=[5,10,20,40] experiment_name=mine

The codes of every image are collected once (stego_amd.cluster_refit.collect_codes: the backbone on the images and their mirror
images, kept on the device as one channels-last tensor).  For every count of `n_clusters` the probe is refitted by cosine k-means
(csrc/code_kmeans.hip; `n_init` k-means++ seedings, the best kept) and the model is written as
`{output_root}/refit/{experiment_name}/clusters_{n}.ckpt`: a checkpoint like any other, which demo_segmentation, eval_segmentation
and load_from_checkpoint take as it is (its cfg holds `cluster_probe_n`).  `sweep.json` beside them is the table one reads to choose
n: per count the objective per token (the mean cosine of a token to its centroid), the smallest and largest cluster, the iterations
and whether the fit converged.
"""
import json
import os
import sys
from os.path import dirname, exists, isdir, join

import torch

from .cluster_refit import collect_codes, refit_cluster_probe
from .data import image_transform
from .demo_segmentation import UnlabeledImageFolder, collate
from .train_segmentation import LitUnsupervisedSegmenter, load_config

REFIT_CONFIG = join(dirname(__file__), "configs", "refit_config.yml")


def result_dir(cfg):
    return join(cfg.output_root, "refit", cfg.experiment_name)


def _folder_batches(cfg, skipped):
    dataset = UnlabeledImageFolder(cfg.image_dir, image_transform(cfg.res, "center"))
    loader = torch.utils.data.DataLoader(dataset, cfg.batch_size * 2, shuffle=False, num_workers=cfg.num_workers, collate_fn=collate)
    for imgs, _, bad in loader:
        skipped.extend(bad)
        if imgs is not None:
            yield imgs


def _dataset_batches(cfg, model):
    """The images of the checkpoint's dataset split: the folder of a "directory" checkpoint, else the cropped tree."""
    from .data import CroppedDataset, DirectoryDataset, crop_dir, label_transform
    mcfg, root, split = model.cfg, getattr(cfg, "pytorch_data_dir", None), getattr(cfg, "split", "train")
    if not root:
        raise ValueError("refit_clusters: give image_dir, or pytorch_data_dir for the checkpoint's dataset")
    if mcfg.dataset_name == "directory":
        ds = DirectoryDataset(root, mcfg.dir_dataset_name, split, transform=image_transform(cfg.res), target_transform=label_transform(cfg.res))
    else:
        crop_type, crop_ratio = getattr(mcfg, "crop_type", "five"), getattr(mcfg, "crop_ratio", 0.5)
        if not exists(join(crop_dir(root, mcfg.dataset_name, crop_type, crop_ratio), "img", split)):
            raise FileNotFoundError("refit_clusters: no cropped %s split of %s under %r" % (split, mcfg.dataset_name, root))
        ds = CroppedDataset(root, mcfg.dataset_name, crop_type, crop_ratio, split, transform=image_transform(cfg.res),
                            target_transform=label_transform(cfg.res))
    loader = torch.utils.data.DataLoader(ds, cfg.batch_size * 2, shuffle=False, num_workers=cfg.num_workers)
    for batch in loader:
        yield batch[0] if isinstance(batch, (tuple, list)) else batch["img"]


def my_app(cfg):
    """Every count of cfg.n_clusters -> {result_dir}/clusters_{n}.ckpt, and {result_dir}/sweep.json.  Returns the rows of sweep.json."""
    if not exists(cfg.model_path):
        raise FileNotFoundError("model_path %r does not exist" % cfg.model_path)
    image_dir = getattr(cfg, "image_dir", None)
    if image_dir and not isdir(image_dir):
        raise FileNotFoundError("image_dir %r is not a directory" % image_dir)
    counts = cfg.n_clusters if isinstance(cfg.n_clusters, (list, tuple)) else [cfg.n_clusters]
    counts = [int(n) for n in counts]
    if not counts or min(counts) < 1:
        raise ValueError("n_clusters = %r: expected a positive int or a list of them" % (cfg.n_clusters,))
    out = result_dir(cfg)
    os.makedirs(out, exist_ok=True)

    dev = torch.device("cuda", 0)
    model = LitUnsupervisedSegmenter.load_from_checkpoint(cfg.model_path)
    model.eval().to(dev)
    skipped = []
    batches = _folder_batches(cfg, skipped) if image_dir else _dataset_batches(cfg, model)
    codes = collect_codes(model, batches, flip=getattr(cfg, "flip", True))
    if skipped:
        print("skipped %d file(s) PIL cannot read: %s" % (len(skipped), ", ".join(skipped)))
    tokens = codes.shape[0] * codes.shape[2] * codes.shape[3]
    generator = torch.Generator().manual_seed(int(getattr(cfg, "seed", 0)))
    rows = []
    for n in counts:
        res = refit_cluster_probe(model, codes, n, n_iter=int(getattr(cfg, "n_iter", 100)), tol=float(getattr(cfg, "tol", 1e-6)),
                                  n_init=int(getattr(cfg, "n_init", 1)), generator=generator)
        path = join(out, "clusters_%d.ckpt" % n)
        model.save_checkpoint(path)
        sizes = res.counts.cpu()
        rows.append({"n_clusters": n, "checkpoint": path, "images": int(codes.shape[0]), "tokens": int(tokens),
                     "objective_per_token": res.objective / tokens, "min_cluster": int(sizes.min()), "max_cluster": int(sizes.max()),
                     "iterations": res.n_iter, "converged": res.converged})
        print("n = %d: mean cosine %.4f, clusters of %d .. %d tokens, %d iterations%s"
              % (n, rows[-1]["objective_per_token"], rows[-1]["min_cluster"], rows[-1]["max_cluster"], res.n_iter,
                 "" if res.converged else " (not converged)"))
    with open(join(out, "sweep.json"), "w") as f:
        json.dump(rows, f, indent=1)
    return rows


if __name__ == "__main__":
    my_app(load_config(REFIT_CONFIG, overrides=sys.argv[1:]))
