"""The training tail of the two probes: the linear probe's cross-entropy at label resolution and the cluster probe's cosine k-means
loss on the detached code (train_segmentation.py:199-224 of the reference), as the torch chain or as one fused native call
(include/stego_probe_train.h) that returns both losses and keeps their gradients to the three probe parameters."""
import torch
import torch.nn.functional as F

from . import capi


def torch_probe_losses(code, label, linear_probe, cluster_probe):
    """(linear_loss, cluster_loss) of LitUnsupervisedSegmenter.training_step as torch operations."""
    detached_code = torch.clone(code.detach())
    linear_logits = linear_probe(detached_code)
    linear_logits = F.interpolate(linear_logits, label.shape[-2:], mode='bilinear', align_corners=False)
    # train_segmentation.py:199-203 flattens to [pixels, classes], boolean-indexes the valid pixels (a host sync) and takes the mean
    # cross-entropy.  The same number from the spatial form: invalid labels become ignore_index, the mean runs over the rest - no
    # sync, no 170 MB permute / gather, and the 2-D NLL kernels instead of the one-block reduction ATen runs on [1.6 M, 27] (7 of the
    # 9 ms of a cached-backbone step, rocprofv3)
    valid = (label >= 0) & (label < linear_probe.out_channels)
    linear_loss = F.cross_entropy(linear_logits, torch.where(valid, label, torch.full_like(label, -100)), ignore_index=-100)
    cluster_loss, _ = cluster_probe(detached_code, None)
    return linear_loss, cluster_loss


class _ProbeLosses(torch.autograd.Function):
    """Forward: the one fused call; it already holds d loss / d parameter of both losses.  Backward: scale them by the upstream scalars."""

    @staticmethod
    def forward(ctx, code, label, weight, bias, clusters):
        losses, _, d_w, d_b, d_c = capi.probe_train(code, label, weight.detach().reshape(weight.shape[0], -1), bias.detach(),
                                                    clusters.detach())
        ctx.save_for_backward(d_w.view(weight.shape), d_b, d_c)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_linear, g_cluster):
        d_w, d_b, d_c = ctx.saved_tensors
        return None, None, d_w * g_linear, d_b * g_linear, d_c * g_cluster


def _native_ok(code, label, linear_probe, cluster_probe):
    if not (code.is_cuda and label.is_cuda and code.dtype == torch.float32 and code.dim() == 4 and label.dtype == torch.int64):
        return False
    if label.dim() != 3 or label.shape[0] != code.shape[0] or min(code.shape) < 1 or min(label.shape) < 1:
        return False
    w, c = linear_probe.weight, cluster_probe.clusters
    if not (label.device == code.device and w.device == code.device and c.device == code.device):
        return False
    if w.dtype != torch.float32 or c.dtype != torch.float32 or tuple(w.shape[2:]) != (1, 1) or linear_probe.bias is None:
        return False
    B, K, h, wd = code.shape
    return (K <= capi.PTRAIN_MAX_K and w.shape[1] == K and c.shape[1] == K and 1 <= w.shape[0] <= capi.PTRAIN_MAX_N and
            1 <= c.shape[0] <= capi.PTRAIN_MAX_N and B <= 65535 and max(h, wd) <= capi.PTRAIN_MAX_CODE and
            max(label.shape[1:]) <= capi.PTRAIN_MAX_OUT)


def probe_losses(code, label, linear_probe, cluster_probe):
    """(linear_loss, cluster_loss) as 0-dim tensors whose backward reaches linear_probe.weight, .bias and cluster_probe.clusters and
    nothing else (the code is detached).  One native call on a HIP device; the torch chain, with today's numbers, for CPU tensors,
    labels that are not int64 and shapes outside the kernel's limits."""
    if not _native_ok(code, label, linear_probe, cluster_probe):
        return torch_probe_losses(code, label, linear_probe, cluster_probe)
    return _ProbeLosses.apply(code.detach(), label, linear_probe.weight, linear_probe.bias, cluster_probe.clusters)
