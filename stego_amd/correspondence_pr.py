"""Label co-occurrence precision / recall of feature correspondences: the reference's ``src/plot_pr_curves.py`` without its five
``[B, S, S, S, S]`` tensors, the concatenation of 100 batches of them and scikit-learn's sort of ~23 M scores per curve.

*Do the correspondences of a feature map predict whether two pixels carry the same label?*  Per batch one kernel launch
(``capi.pr_accumulate``, ``include/stego_pr.h``) samples both maps and both label maps at random points, correlates the normalised
samples and adds every pair to a histogram of the cosine over fixed bins of [-1, 1], split into positive (same class) and negative
pairs; precision, recall and average precision come from that histogram on the host, with scikit-learn's arithmetic applied to the
bin indices.  A pair attracts in the loss exactly when its feature cosine exceeds the shift of its pair kind, so ``at(shift)`` is
the number to look at when ``pos_intra_shift`` / ``pos_inter_shift`` / ``neg_inter_shift`` are tuned on a new dataset.

    python -m stego_amd.correspondence_pr model_paths=[run.ckpt] pairs=[self,knn,random]      # add --plot for the figure

Out of scope: the reference's MoCo and learned-CRF-kernel curves (its ``self.dino`` / ``self.crf`` are commented out there and the
script does not run as shipped) and its confusion-matrix plot.
"""
import json
import math
import os
import sys
from os.path import dirname, join

import numpy as np
import torch

from . import capi

PR_CONFIG = join(dirname(__file__), "configs", "pr_config.yml")
MAPS = ("feats", "code")
PAIR_SHIFT = {"self": "pos_intra_shift", "knn": "pos_inter_shift", "random": "neg_inter_shift"}    # the loss's three pair kinds


def pr_from_hist(hist):
    """sklearn.metrics.precision_recall_curve / average_precision_score on scores that are bin indices: `hist` [n_bins, 2]
    (negatives, positives) -> precision, recall (increasing threshold, then the final (1, 0) point), the occupied bins (the
    thresholds) and the step integral sum (R_k - R_{k-1}) P_k; float64.  Without a positive: recall and the integral are nan."""
    hist = np.asarray(hist, dtype=np.int64)
    neg, pos = hist[:, 0], hist[:, 1]
    bins = np.nonzero(neg + pos)[0]
    d = bins[::-1]                                           # one threshold per distinct score, descending
    tps = np.cumsum(pos[d]).astype(np.float64)
    fps = np.cumsum(neg[d]).astype(np.float64)
    n_pos = int(pos.sum())
    precision = tps / (tps + fps)                            # (occupied bins only: never 0 / 0)
    recall = tps / n_pos if n_pos else np.full(tps.shape, np.nan)
    # the step integral is a convex combination of the precisions (weights pos_k / n_pos): summed as an offset from the lowest one, so
    # that a constant precision (a single occupied bin; every pair positive) comes out exactly
    ap = float(precision.min() + math.fsum(pos[d] / n_pos * (precision - precision.min()))) if n_pos else float("nan")
    return np.concatenate([precision[::-1], [1.0]]), np.concatenate([recall[::-1], [0.0]]), bins, ap


class CorrespondencePR:
    """The device histogram of one curve.  update() adds the pairs of a batch (one launch, nothing synchronised), compute() sums it
    across ranks when a process group is initialised (as UnsupervisedMetrics.compute does) and turns it into the curve."""

    def __init__(self, n_classes, n_bins=4096, skip_unlabeled=False):
        if not capi.PR_MIN_BINS <= n_bins <= capi.PR_MAX_BINS:
            raise ValueError("n_bins = %d outside [%d, %d]" % (n_bins, capi.PR_MIN_BINS, capi.PR_MAX_BINS))
        self.n_classes, self.n_bins, self.skip_unlabeled = int(n_classes), int(n_bins), bool(skip_unlabeled)
        self.hist = None                                     # int64 [n_bins, 2] on the device of the first update

    def reset(self):
        if self.hist is not None:
            self.hist.zero_()

    def update(self, a, b, labels_a, labels_b, coords1, coords2, index_b=None):
        if self.hist is None:
            capi._require_dev(a)
            self.hist = torch.zeros(self.n_bins, 2, dtype=torch.int64, device=a.device)
        capi.pr_accumulate(a, b, labels_a, labels_b, coords1, coords2, self.hist, self.n_classes, index_b=index_b,
                           skip_unlabeled=self.skip_unlabeled)

    def histogram(self):
        """int64 [n_bins, 2] on the host, summed across ranks."""
        if self.hist is None:
            return np.zeros((self.n_bins, 2), dtype=np.int64)
        h = self.hist.clone()
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            buf = h if dist.get_backend() == "nccl" else h.cpu()
            dist.all_reduce(buf)
            h = buf
        return h.cpu().numpy()

    def edge(self, k):
        """The cosine at the lower edge of bin k."""
        return -1.0 + 2.0 * np.asarray(k, dtype=np.float64) / self.n_bins

    def compute(self):
        hist = self.histogram()
        precision, recall, bins, ap = pr_from_hist(hist)
        return dict(precision=precision, recall=recall, thresholds=self.edge(bins), average_precision=ap,
                    n_pos=int(hist[:, 1].sum()), n_total=int(hist.sum()), hist=hist)

    def at(self, shift, hist=None):
        """Precision, recall and the share of all pairs among the pairs with fd >= edge, where `edge` is the lowest bin edge that is
        not below `shift` (returned too: the quantisation is 2 / n_bins)."""
        hist = self.histogram() if hist is None else hist
        k = min(self.n_bins, max(0, int(math.ceil((float(shift) + 1.0) / 2.0 * self.n_bins))))
        sel = hist[k:]
        n_sel, p_sel, n_pos, n_total = int(sel.sum()), int(sel[:, 1].sum()), int(hist[:, 1].sum()), int(hist.sum())
        nan = float("nan")
        return dict(shift=float(shift), edge=float(self.edge(k)), precision=p_sel / n_sel if n_sel else nan,
                    recall=p_sel / n_pos if n_pos else nan, share=n_sel / n_total if n_total else nan)


def draw_points(gen, B, n_samples, device, want_perm):
    """One batch's draws from the seeded device generator: coords1, coords2 (`torch.rand(...) * 2 - 1`, plot_pr_curves.py:134-136)
    and, for the "random" pairs, super_perm(B) (modules.py:291-295) from the same generator."""
    shape = (B, n_samples, n_samples, 2)
    coords1 = torch.rand(shape, generator=gen, device=device) * 2 - 1
    coords2 = torch.rand(shape, generator=gen, device=device) * 2 - 1
    perm = None
    if want_perm:
        from .modules import _unfix
        perm = _unfix(torch.randperm(B, generator=gen, device=device, dtype=torch.long))
    return coords1, coords2, perm


def evaluate_correspondence(model, loader, n_samples=11, max_batches=100, pairs=("self",), seed=0, n_bins=4096, skip_unlabeled=False,
                            device=None):
    """plot_pr_curves.py:126-150 over `loader` (batches with "img" / "label" and, for "knn", "img_pos" / "label_pos"; or
    (img, label, ...) tuples) for the maps "feats" and "code" of model.net and the pair kinds of `pairs`:
      "self"   the reference's: every image against itself
      "knn"    the image against its KNN positive (left out, with a note, when the batches carry none)
      "random" the image against another image of the batch (index_b = super_perm(B))
    -> {map: {kind: CorrespondencePR.compute() + "at_shift": at(the shift model.cfg uses for that kind)}}."""
    for kind in pairs:
        if kind not in PAIR_SHIFT:
            raise ValueError("unknown pair kind %r (one of %s)" % (kind, sorted(PAIR_SHIFT)))
    device = device or next(model.parameters()).device
    if torch.device(device).type != "cuda":
        raise RuntimeError("stego_amd runs on MI355X only: got device %s (no CPU fallback exists)" % (device,))
    model.eval()
    kinds = list(pairs)
    metrics = {m: {k: CorrespondencePR(model.n_classes, n_bins, skip_unlabeled) for k in kinds} for m in MAPS}
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    with torch.no_grad():
        for bi, batch in enumerate(loader):
            if max_batches is not None and bi >= max_batches:
                break
            is_dict = isinstance(batch, dict)
            img, label = (batch["img"], batch["label"]) if is_dict else (batch[0], batch[1])
            img, label = img.to(device), label.to(device)
            if label.dim() == 4:
                label = label[:, 0]
            if "knn" in kinds and not (is_dict and "img_pos" in batch and "label_pos" in batch):
                print("batches carry no img_pos / label_pos: the \"knn\" pairs are left out")
                kinds.remove("knn")
                for m in MAPS:
                    del metrics[m]["knn"]
            maps = dict(zip(MAPS, model.net(img)))
            coords1, coords2, perm = draw_points(gen, img.shape[0], n_samples, device, "random" in kinds)
            if "knn" in kinds:
                maps_pos = dict(zip(MAPS, model.net(batch["img_pos"].to(device))))
                label_pos = batch["label_pos"].to(device)
                label_pos = label_pos[:, 0] if label_pos.dim() == 4 else label_pos
            for m in MAPS:
                t = maps[m].float()
                for kind in kinds:
                    if kind == "self":
                        metrics[m][kind].update(t, t, label, label, coords1, coords2)
                    elif kind == "knn":
                        metrics[m][kind].update(t, maps_pos[m].float(), label, label_pos, coords1, coords2)
                    else:
                        metrics[m][kind].update(t, t, label, label, coords1, coords2, index_b=perm)
    out = {}
    for m in MAPS:
        out[m] = {}
        for kind in kinds:
            res = metrics[m][kind].compute()
            res["at_shift"] = metrics[m][kind].at(getattr(model.cfg, PAIR_SHIFT[kind], 0.0), res["hist"])
            out[m][kind] = res
    return out


def _decimate(res, limit=512):
    """The curve as JSON lists of at most `limit` points (every ceil(n / limit)-th threshold, the end points kept)."""
    n = len(res["thresholds"])
    idx = np.unique(np.concatenate([np.arange(0, n, max(1, -(-n // limit)))[:limit - 1], [n - 1]])) if n else np.zeros(0, dtype=np.int64)
    return dict(average_precision=res["average_precision"], n_pos=res["n_pos"], n_total=res["n_total"], at_shift=res["at_shift"],
                thresholds=[float(v) for v in res["thresholds"][idx]], precision=[float(v) for v in res["precision"][:-1][idx]],
                recall=[float(v) for v in res["recall"][:-1][idx]])


def result_dir(cfg):
    return join(cfg.output_root, "results", "pr_curves", cfg.experiment_name)


def plot(results, path):
    """The reference's figure (plot_pr_curves.py:206-218): recall against precision, one line per map and pair kind."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.figure(figsize=(5, 4), dpi=100)
    for name, by_map in results.items():
        for m, by_kind in by_map.items():
            for kind, res in by_kind.items():
                plt.plot(res["recall"], res["precision"], label="AP=%d%% %s %s %s" % (int(res["average_precision"] * 100), os.path.basename(name), m, kind))
    plt.xlim([0, 1])
    plt.ylim([0, 1])
    plt.legend(fontsize=8)
    plt.ylabel("Precision", fontsize=16)
    plt.xlabel("Recall", fontsize=16)
    plt.tight_layout()
    plt.savefig(path)
    plt.close()


def my_app(cfg, do_plot=False):
    """Every checkpoint of cfg.model_paths on the val split eval_segmentation.make_loader finds (synthetic data otherwise): prints the
    average precision per map and pair kind and writes {result_dir}/pr_curves.json; returns {path: evaluate_correspondence(...)}."""
    from .eval_segmentation import make_loader
    from .train_segmentation import LitUnsupervisedSegmenter
    dev = torch.device("cuda", 0)
    results = {}
    for model_path in cfg.model_paths:
        model = LitUnsupervisedSegmenter.load_from_checkpoint(model_path)
        model.eval().to(dev)
        res = evaluate_correspondence(model, make_loader(cfg, model), n_samples=cfg.feature_samples, max_batches=cfg.limit_val_batches,
                                      pairs=tuple(cfg.pairs), seed=getattr(cfg, "seed", 0), n_bins=cfg.pr_bins,
                                      skip_unlabeled=getattr(cfg, "skip_unlabeled", False), device=dev)
        print(model_path)
        for m, by_kind in res.items():
            for kind, r in by_kind.items():
                a = r["at_shift"]
                print("  %-5s %-6s AP %.4f  (%d of %d pairs positive)  at shift %.3f (edge %.4f): precision %.4f recall %.4f share %.4f"
                      % (m, kind, r["average_precision"], r["n_pos"], r["n_total"], a["shift"], a["edge"], a["precision"], a["recall"], a["share"]))
        results[model_path] = res
    out = result_dir(cfg)
    os.makedirs(out, exist_ok=True)
    with open(join(out, "pr_curves.json"), "w") as f:
        json.dump({p: {m: {k: _decimate(r) for k, r in by_kind.items()} for m, by_kind in res.items()} for p, res in results.items()}, f, indent=1)
    if do_plot:
        try:
            plot(results, join(out, "pr_curves.png"))
        except ImportError as e:
            print("--plot needs matplotlib (%s): no figure written" % e)
    return results


if __name__ == "__main__":
    from .train_segmentation import load_config
    argv = [a for a in sys.argv[1:] if a != "--plot"]
    my_app(load_config(PR_CONFIG, overrides=argv), do_plot="--plot" in sys.argv[1:])
