"""Inference tail of the reference (``src/demo_segmentation.py:62-78``, ``src/eval_segmentation.py:124-138``) on the fused probe head.

The reference flip-averages the code, resizes it to the image's resolution with bilinear interpolation and runs both probes and their
(log-)softmax over full-resolution tensors.  Here csrc/probe_head.hip (include/stego_probe.h) does all of it in one launch from the
low-resolution code, and writes per probe what the next step needs: the probabilities the dense CRF takes, the log-probabilities the
metrics take, or the label map directly when the CRF is off.  There is no CPU path: CPU tensors raise.
"""
import torch
import torch.nn.functional as F

from . import capi
from .crf import _device_tensor, dense_crf_batch, image_to_bgr_u8

KINDS = ("log_probs", "probs", "argmax", None)


def probe_head(model, code, code_flip, size, linear="log_probs", cluster="log_probs", alpha=2):
    """Both probes of `model` (a LitUnsupervisedSegmenter) on code [B, K, h, w] and, when not None, the code of the flipped images
    (flip-averaged as (code + code_flip.flip(3)) / 2), resized to `size` = (H, W).  `linear` / `cluster` each name the output:
    "log_probs" (float32 [B, n, H, W], log_softmax), "probs" (softmax), "argmax" (int64 [B, H, W]) or None (skipped).  Returns
    (linear, cluster) on the code's device."""
    if linear not in KINDS or cluster not in KINDS:
        raise ValueError("probe_head: output kinds are %s, got %r / %r" % (KINDS, linear, cluster))
    _device_tensor(code, "code")
    if code_flip is not None:
        _device_tensor(code_flip, "code_flip")
    if code.dim() != 4:
        raise ValueError("code: expected [B, K, h, w], got %s" % (tuple(code.shape),))
    H, W = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    with torch.no_grad():
        lw = model.linear_probe.weight.detach()
        lw = lw.reshape(lw.shape[0], lw.shape[1])
        lb = model.linear_probe.bias.detach()
        cent = F.normalize(model.cluster_probe.clusters.detach(), dim=1)
        return capi.probe_head(code.detach().float(), None if code_flip is None else code_flip.detach().float(), lw, lb, cent, (H, W),
                               linear, cluster, alpha)


def segment(model, img, run_crf=True, flip=True, res=None):
    """Normalised images [B, 3, H, W] -> (linear_preds, cluster_preds), int64 [B, res, res] (default: the images' H, W): the backbone
    on the images and on their mirror images, the fused probe head, then the dense CRF on both probes' probabilities (run_crf) and
    the argmax.  The CRF runs at the image's resolution, so `res` must equal it when run_crf is set."""
    _device_tensor(img, "img")
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError("img: expected [B, 3, H, W], got %s" % (tuple(img.shape),))
    size = tuple(img.shape[-2:]) if res is None else ((int(res), int(res)) if isinstance(res, int) else tuple(res))
    if run_crf and size != tuple(img.shape[-2:]):
        raise ValueError("segment: the CRF runs at the image's resolution %s, res = %s" % (tuple(img.shape[-2:]), size))
    with torch.no_grad():
        _, code1 = model.net(img)
        code2 = model.net(img.flip(dims=[3]))[1] if flip else None
        kind = "probs" if run_crf else "argmax"
        lin, clu = probe_head(model, code1, code2, size, linear=kind, cluster=kind)
        if not run_crf:
            return lin, clu
        bgr = image_to_bgr_u8(img)
        return dense_crf_batch(bgr, lin).argmax(1), dense_crf_batch(bgr, clu).argmax(1)
