"""The reference's evaluation loop (``src/eval_segmentation.py:118-161``) without PiCIE or DataParallel: flip-averaged code, both
probes, the dense CRF (stego_amd.crf, on the device) and the final metrics.

    python -m stego_amd.eval_segmentation model_paths=[run.ckpt] run_crf=True       # a CroppedDataset val split, or synthetic data

With `save_figures=True` the qualitative figure of the reference (eval_segmentation.py:178-210) is written too, without matplotlib:
the images `figure_images` names stay on the device with their labels and predictions, are coloured there (stego_amd.render) and
saved as {img/N.jpg, label/N.png, linear/N.png, cluster/N.png} and as figure_K.png contact sheets of up to 10 columns with the rows
image / label / linear probe / cluster probe, the clusters coloured by their Hungarian class.
"""
import os
import sys
from os.path import dirname, exists, join

import torch
import torch.nn.functional as F

from .crf import batched_crf, dense_crf_batch, image_to_bgr_u8
from .data import _MEAN, _STD, CroppedDataset, DirectoryDataset, _resize_center_crop, crop_dir, image_transform, label_transform  # noqa: F401
from .train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config

EVAL_CONFIG = join(dirname(__file__), "configs", "eval_config.yml")


def _img_label(batch):
    if isinstance(batch, dict):
        return batch["img"], batch["label"]
    return batch[0], batch[1]                    # CroppedDataset items: (image, target, mask)


def _fused_preds(model, img, code1, code2, size, run_crf):
    """The same predictions from the fused probe head: the log-probabilities at the label's size `size`, or with run_crf the CRF's
    probabilities straight from the kernel at the image's size, where the CRF runs (the unfused path resizes to it in _probs_at)."""
    from .segment import probe_head
    if not run_crf:
        linear_probs, cluster_probs = probe_head(model, code1, code2, size, linear="log_probs", cluster="log_probs")
        return linear_probs.argmax(1), cluster_probs.argmax(1)
    linear_probs, cluster_probs = probe_head(model, code1, code2, img.shape[-2:], linear="probs", cluster="probs")
    bgr = image_to_bgr_u8(img)
    return dense_crf_batch(bgr, linear_probs).argmax(1), dense_crf_batch(bgr, cluster_probs).argmax(1)


def _native_update(model, img, code1, code2, label, run_crf):
    """One batch into the model's DeviceUnsupervisedMetrics with no label map, no log-probability tensor and no host sync: without
    CRF one fused call from the low-resolution codes to both confusion matrices; with CRF the fused head's probabilities go through
    the dense CRF as in _fused_preds and the kernel takes the argmax of its output while it counts."""
    from .metrics import probe_confusion
    if not run_crf:
        probe_confusion(model, code1, code2, label, model.test_linear_metrics, model.test_cluster_metrics)
        return
    from .segment import probe_head
    linear_probs, cluster_probs = probe_head(model, code1, code2, img.shape[-2:], linear="probs", cluster="probs")
    bgr = image_to_bgr_u8(img)
    model.test_linear_metrics.update_scores(dense_crf_batch(bgr, linear_probs), label)
    model.test_cluster_metrics.update_scores(dense_crf_batch(bgr, cluster_probs), label)


def _kept_preds(model, img, code1, code2, size, run_crf):
    """The label maps of a batch that native_metrics scored without any: the fused head's argmax, after the CRF with run_crf."""
    if run_crf:
        return _fused_preds(model, img, code1, code2, size, True)
    from .segment import probe_head
    return probe_head(model, code1, code2, size, linear="argmax", cluster="argmax")


def evaluate(model, loader, run_crf=True, device=None, fused_head=False, native_metrics=False, keep=None, min_region_area=0,
             region_connectivity=4):
    """eval_segmentation.py:118-161 over `loader` (batches with "img" / "label", or (img, label, ...) tuples) -> the metrics dict of
    model.test_linear_metrics and model.test_cluster_metrics (reset first, then updated batch by batch, then computed).
    fused_head: the flip average, resize and both probes in one launch (stego_amd.segment.probe_head), which writes the CRF's
    probabilities directly (run_crf) or the log-probabilities the argmax takes, instead of the torch chain.
    native_metrics: the confusion matrices are counted on the device (stego_amd.metrics) and read once, in compute(); implies the
    fused head.  The model's test metrics become DeviceUnsupervisedMetrics for it when they are not already.
    keep: indices of images, counted through the loader, whose image, label and both predictions stay on the device: afterwards
    model.saved_data = {"index": [...], "img": [n, 3, H, W], "label", "linear_preds", "cluster_preds": [n, h, w]} in the order the
    loader met them (the reference's saved_data).  With native_metrics the batches that hold one additionally run the fused head with
    the argmax output, since the metrics path has no label map; the metrics do not change.
    min_region_area > 0: the small-region cleanup of stego_amd.regions (regions under `region_connectivity`) on both predictions, after
    the CRF or the argmax and before they are scored.  With native_metrics the label maps are then made (the fused head's argmax, after
    the CRF with run_crf), cleaned and counted by the label-map confusion launch: the fused code-to-matrix launch never makes a map."""
    min_region_area = int(min_region_area)
    keeping = keep is not None
    keep = set(int(k) for k in keep) if keeping else set()
    saved = {"index": [], "img": [], "label": [], "linear_preds": [], "cluster_preds": []}
    seen = 0
    device = device or next(model.parameters()).device
    if hasattr(model, "check_cluster_scoring"):
        model.check_cluster_scoring()
    model.eval()
    if native_metrics:
        from .metrics import DeviceUnsupervisedMetrics
        for name in ("test_linear_metrics", "test_cluster_metrics"):
            m = getattr(model, name)
            if not isinstance(m, DeviceUnsupervisedMetrics):
                setattr(model, name, DeviceUnsupervisedMetrics(m.prefix, m.n_classes, m.extra_clusters, m.compute_hungarian))
    model.test_linear_metrics.reset()
    model.test_cluster_metrics.reset()
    with torch.no_grad():
        for batch in loader:
            img, label = _img_label(batch)
            img, label = img.to(device), label.to(device)
            _, code1 = model.net(img)
            _, code2 = model.net(img.flip(dims=[3]))
            wanted = [j for j in range(img.shape[0]) if seen + j in keep]
            first, seen = seen, seen + img.shape[0]
            if native_metrics and min_region_area > 0:
                from .segment import _clean
                linear_preds, cluster_preds = _clean(model, *_kept_preds(model, img, code1, code2, label.shape[-2:], run_crf),
                                                     min_region_area, region_connectivity)
                model.test_linear_metrics.update(linear_preds, label)
                model.test_cluster_metrics.update(cluster_preds, label)
                if wanted:
                    _keep(saved, wanted, first, img, label, linear_preds, cluster_preds)
                continue
            if native_metrics:
                _native_update(model, img, code1, code2, label, run_crf)
                if wanted:
                    _keep(saved, wanted, first, img, label, *_kept_preds(model, img, code1, code2, label.shape[-2:], run_crf))
                continue
            if fused_head:
                linear_preds, cluster_preds = _fused_preds(model, img, code1, code2, label.shape[-2:], run_crf)
            else:
                code = (code1 + code2.flip(dims=[3])) / 2
                code = F.interpolate(code, label.shape[-2:], mode="bilinear", align_corners=False)
                linear_probs = torch.log_softmax(model.linear_probe(code), dim=1)
                cluster_probs = model.cluster_probe(code, 2, log_probs=True)
                if run_crf:
                    linear_preds = batched_crf(None, img, linear_probs).argmax(1)
                    cluster_preds = batched_crf(None, img, cluster_probs).argmax(1)
                else:
                    linear_preds = linear_probs.argmax(1)
                    cluster_preds = cluster_probs.argmax(1)
            if min_region_area > 0:
                from .segment import _clean
                linear_preds, cluster_preds = _clean(model, linear_preds, cluster_preds, min_region_area, region_connectivity)
            model.test_linear_metrics.update(linear_preds, label)
            model.test_cluster_metrics.update(cluster_preds, label)
            if wanted:
                _keep(saved, wanted, first, img, label, linear_preds, cluster_preds)
    if keeping:
        model.saved_data = {k: (torch.stack(v) if k != "index" else v) for k, v in saved.items()} if saved["index"] else saved
    return {**model.test_linear_metrics.compute(), **model.test_cluster_metrics.compute()}


def _keep(saved, wanted, first, img, label, linear_preds, cluster_preds):
    size = label.shape[-2:]
    for j in wanted:
        saved["index"].append(first + j)
        saved["img"].append(img[j])
        saved["label"].append(label[j].reshape(size))
        saved["linear_preds"].append(linear_preds[j].reshape(size))
        saved["cluster_preds"].append(cluster_preds[j].reshape(size))


def result_dir(cfg, i=0):
    base = join(getattr(cfg, "output_root", "../"), "results", "predictions", str(getattr(cfg, "experiment_name", "eval")))
    return base if i == 0 else "%s_%d" % (base, i)


def save_figures(model, out, columns=10):
    """model.saved_data (evaluate(keep=...)) and the computed test_cluster_metrics -> the pictures under `out`; returns the paths.
    Everything is coloured on the device; a picture crosses to the host as the uint8 bytes PIL writes."""
    from PIL import Image

    from .render import colorize, comparison_sheet, image_u8
    data = model.saved_data
    n = len(data["index"])
    written = []
    if n == 0:
        return written
    for sub in ("img", "label", "linear", "cluster"):
        os.makedirs(join(out, sub), exist_ok=True)
    cmap, mapping = model.label_cmap, model.test_cluster_metrics.cluster_to_class()
    panels = (("img", ".jpg", image_u8(data["img"])), ("label", ".png", colorize(data["label"], cmap)),
              ("linear", ".png", colorize(data["linear_preds"], cmap)),
              ("cluster", ".png", colorize(data["cluster_preds"], cmap, mapping=mapping)))
    for sub, ext, rgb in panels:
        rgb = rgb.cpu().numpy()
        for i in range(n):
            written.append(join(out, sub, str(i) + ext))
            Image.fromarray(rgb[i]).save(written[-1])
    for k, lo in enumerate(range(0, n, columns)):
        cols = slice(lo, lo + columns)
        sheet = comparison_sheet([{"image": data["img"][cols]}, {"labels": data["label"][cols], "cmap": cmap},
                                  {"labels": data["linear_preds"][cols], "cmap": cmap},
                                  {"labels": data["cluster_preds"][cols], "cmap": cmap, "mapping": mapping}])
        written.append(join(out, "figure_%d.png" % k))
        Image.fromarray(sheet.cpu().numpy()).save(written[-1])
    return written


def make_loader(cfg, model):
    """The val split of the cropped tree under cfg.pytorch_data_dir when it exists (crop_datasets.py's layout); for a checkpoint
    trained on an image folder (dataset_name "directory") that folder's val split when it has labels; else synthetic data."""
    mcfg = model.cfg
    root = getattr(cfg, "pytorch_data_dir", None)
    crop_type, crop_ratio = getattr(mcfg, "crop_type", "five"), getattr(mcfg, "crop_ratio", 0.5)
    name = getattr(mcfg, "dir_dataset_name", None)
    if root and mcfg.dataset_name == "directory" and name and exists(join(root, name, "imgs", "val")) and \
            exists(join(root, name, "labels", "val")):
        ds = DirectoryDataset(root, name, "val", transform=image_transform(cfg.res), target_transform=label_transform(cfg.res))
    elif root and mcfg.dataset_name == "directory":
        print("no labelled val split of the folder %r under %r: synthetic data" % (name, root))
        ds = SyntheticContrastiveDataset(cfg.batch_size * 4, cfg.res, model.n_classes, seed=0)
    elif root and exists(join(crop_dir(root, mcfg.dataset_name, crop_type, crop_ratio), "img", "val")):
        ds = CroppedDataset(root, mcfg.dataset_name, crop_type, crop_ratio, "val", transform=image_transform(cfg.res),
                            target_transform=label_transform(cfg.res))
    else:
        print("no cropped val split under %r: synthetic data" % root)
        ds = SyntheticContrastiveDataset(cfg.batch_size * 4, cfg.res, model.n_classes, seed=0)
    return torch.utils.data.DataLoader(ds, cfg.batch_size * 2, shuffle=False, num_workers=getattr(cfg, "num_workers", 0))


def my_app(cfg):
    """eval_segmentation.py:57-161: every checkpoint of cfg.model_paths evaluated on the val split; returns {path: metrics}."""
    results = {}
    dev = torch.device("cuda", 0)
    figures = getattr(cfg, "save_figures", False)
    wanted = getattr(cfg, "figure_images", None)
    keep = (list(wanted) if wanted is not None else list(range(8))) if figures else None
    for i, model_path in enumerate(cfg.model_paths):
        model = LitUnsupervisedSegmenter.load_from_checkpoint(model_path)
        model.eval().to(dev)
        metrics = evaluate(model, make_loader(cfg, model), run_crf=cfg.run_crf, device=dev, fused_head=getattr(cfg, "fused_head", False),
                           native_metrics=getattr(cfg, "native_metrics", False), keep=keep,
                           min_region_area=getattr(cfg, "min_region_area", 0), region_connectivity=getattr(cfg, "region_connectivity", 4))
        if figures:
            save_figures(model, result_dir(cfg, i))
        print("")
        print(model_path)
        print({k: float(v) for k, v in metrics.items()})
        results[model_path] = metrics
    return results


if __name__ == "__main__":
    my_app(load_config(EVAL_CONFIG, overrides=sys.argv[1:]))
