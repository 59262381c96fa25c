"""Scoring without a host round trip: the confusion matrices behind mIoU and accuracy stay on the device (include/stego_confusion.h).

``UnsupervisedMetrics.update`` (stego_amd.utils; the reference's utils.py:215-228) masks, gathers and bincounts the predictions of a
batch and ends in ``.cpu()``: one host synchronisation per probe per batch, after a chain that resized the code to the label's
resolution and ran both probes there.  ``DeviceUnsupervisedMetrics`` keeps the matrix on the device and counts with
csrc/confusion.hip; ``probe_confusion`` goes from the low-resolution code to both probes' matrices in one launch, with no per-pixel
tensor in between.  The host sees the matrix when ``stats`` is read or ``compute()`` runs, not before.
"""
import torch
import torch.nn.functional as F

from . import capi
from .utils import UnsupervisedMetrics


class DeviceUnsupervisedMetrics(UnsupervisedMetrics):
    """UnsupervisedMetrics whose state is an int64 [n_classes + extra_clusters, n_classes] matrix on the device, allocated at the
    first device input.  update() / update_scores() enqueue one stego_confusion launch and never synchronise; on CPU tensors both
    run the parent's arithmetic, so the class works everywhere.  `stats` is the host copy of the matrix (the only device -> host
    copy, made when the property is read or inside compute()); compute() returns what the parent returns for that matrix.

    The reference drops every prediction >= n_classes (utils.py:223), which matters with extra_clusters > 0: rows n_classes and up
    of the state stay zero there.  The kernels count every row of the matrix they are given; this class keeps the reference's
    behaviour by folding only rows < n_classes into its state.  The quirk lives here, not in the C ABI."""

    def __init__(self, prefix, n_classes, extra_clusters, compute_hungarian):
        self._host = None
        self._dev = None
        super().__init__(prefix, n_classes, extra_clusters, compute_hungarian)

    @property
    def stats(self):
        """The host matrix.  Reading it moves what the device matrix holds into it (the one device -> host copy) and zeroes the
        device matrix, so the two never count a pixel twice; the tensor returned is the object's own, as the parent's is."""
        if self._dev is not None:
            self._host += self._dev.cpu()
            self._dev.zero_()
        return self._host

    @stats.setter
    def stats(self, value):
        self._host = value
        if self._dev is not None:
            self._dev.zero_()

    @property
    def device_stats(self):
        """The matrix on the device (None before the first device input): what the kernels add onto and reset() zeroes."""
        return self._dev

    def reset(self):
        self._host.zero_()
        if self._dev is not None:
            self._dev.zero_()

    def _state(self, device):
        if self._dev is None or self._dev.device != device:
            self.stats                                             # (another device than before: its counts move to the host first)
            self._dev = torch.zeros(self.n_classes + self.extra_clusters, self.n_classes, dtype=torch.int64, device=device)
        return self._dev

    def counts_for(self, device, n):
        """The int64 [n, n_classes] device matrix a kernel that predicts n labels adds onto, and what to do after the launch:
        (rows [0, n) of the state, None) when every row is one the reference counts (n <= n_classes), else (a zeroed matrix of its
        own, that matrix): pass the second to fold() once the launch is enqueued."""
        if n <= self.n_classes:
            return self._state(device)[:n], None
        full = torch.zeros(n, self.n_classes, dtype=torch.int64, device=device)
        return full, full

    def fold(self, full):
        """Add rows < n_classes of a matrix from counts_for() to the state (see the class docstring)."""
        if full is not None:
            self._state(full.device)[:self.n_classes] += full[:self.n_classes]

    def update(self, preds, target):
        if not preds.is_cuda:
            return super().update(preds, target)
        with torch.no_grad():
            # the kernel is given rows [0, n_classes) only: predictions >= n_classes fall outside and count nothing, as in the reference
            capi.confusion(preds.reshape(1, 1, -1).long(), target.reshape(1, 1, -1).long(), self._state(preds.device)[:self.n_classes],
                           "labels")

    def update_scores(self, scores, target):
        """update(scores.argmax(1), target) for float scores [B, n, H, W] without the argmax tensor: the kernel takes the first
        maximum over n itself (torch.argmax for finite scores)."""
        if not scores.is_cuda:
            return self.update(scores.argmax(1), target)
        with torch.no_grad():
            counts, full = self.counts_for(scores.device, int(scores.shape[1]))
            capi.confusion(scores.float(), target.reshape(scores.shape[0], scores.shape[2], scores.shape[3]).long(), counts, "scores")
            self.fold(full)

    def compute(self):
        import torch.distributed as dist
        if self._dev is not None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 \
                and dist.get_backend() == "nccl":
            total = self._dev + self._host.to(self._dev.device)    # the cross-rank sum runs on the device matrix itself
            dist.all_reduce(total)
            return self._scores(total.cpu())
        return super().compute()


def probe_confusion(model, code, code_flip, label, linear_metrics, cluster_metrics, alpha=2):
    """Both probes of `model` (a LitUnsupervisedSegmenter) on code [B, K, h, w] (flip-averaged with `code_flip` when not None),
    resized to label.shape[-2:], scored against `label` (int64 [B, H, W]) into the two DeviceUnsupervisedMetrics objects: one
    stego_probe_confusion launch, no per-pixel tensor, no synchronisation.  Either metrics object may be None: that probe is
    skipped."""
    if linear_metrics is None and cluster_metrics is None:
        raise ValueError("probe_confusion: both metrics objects are None")
    for m in (linear_metrics, cluster_metrics):
        if m is not None and not isinstance(m, DeviceUnsupervisedMetrics):
            raise TypeError("probe_confusion: expected DeviceUnsupervisedMetrics, got %s" % type(m).__name__)
    if not code.is_cuda:
        raise RuntimeError("stego_amd runs on MI355X only: got a %s tensor (no CPU fallback exists)" % code.device)
    if code.dim() != 4:
        raise ValueError("code: expected [B, K, h, w], got %s" % (tuple(code.shape),))
    dev = code.device
    with torch.no_grad():
        label = label.reshape(code.shape[0], label.shape[-2], label.shape[-1]).long()
        lw = lb = cent = lin_counts = clu_counts = lin_full = clu_full = None
        if linear_metrics is not None:
            lw = model.linear_probe.weight.detach()
            lw = lw.reshape(lw.shape[0], lw.shape[1])
            lb = model.linear_probe.bias.detach()
            lin_counts, lin_full = linear_metrics.counts_for(dev, int(lw.shape[0]))
        if cluster_metrics is not None:
            cent = F.normalize(model.cluster_probe.clusters.detach(), dim=1)
            clu_counts, clu_full = cluster_metrics.counts_for(dev, int(cent.shape[0]))
        capi.probe_confusion(code.detach().float(), None if code_flip is None else code_flip.detach().float(), lw, lb, cent, label,
                             lin_counts, clu_counts, alpha)
        if linear_metrics is not None:
            linear_metrics.fold(lin_full)
        if cluster_metrics is not None:
            cluster_metrics.fold(clu_full)
