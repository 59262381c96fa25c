"""Inference tail of the reference (``src/demo_segmentation.py:62-78``, ``src/eval_segmentation.py:124-138``) on the fused probe head.

The reference flip-averages the code, resizes it to the image's resolution with bilinear interpolation and runs both probes and their
(log-)softmax over full-resolution tensors.  Here csrc/probe_head.hip (include/stego_probe.h) does all of it in one launch from the
low-resolution code, and writes per probe what the next step needs: the probabilities the dense CRF takes, the log-probabilities the
metrics take, or the label map directly when the CRF is off.  There is no CPU path: CPU tensors raise.

segment_large() segments an image of any size at least the window's: overlapping windows (include/stego_stitch.h) cut out on the device,
run through the backbone in chunks, and stitched on the canvas by csrc/stitch_probe.hip in one launch that reads the windows' codes and
writes only the canvas.  The reference's plot_potsdam.py tiles 320-pixel windows without overlap, one by one, in Python.
"""
import torch
import torch.nn.functional as F

from . import capi
from .crf import Bi_RGB_STD, Bi_W, Bi_XY_STD, MAX_ITER, POS_W, POS_XY_STD, _device_tensor, dense_crf_batch, image_to_bgr_u8

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


def _clean(model, lin, clu, min_region_area, connectivity):
    """The small-region cleanup of stego_amd.regions on both probes' label maps (a probe's label count is its n_labels)."""
    from .regions import clean_label_maps
    return (clean_label_maps(lin, min_region_area, int(model.linear_probe.weight.shape[0]), connectivity),
            clean_label_maps(clu, min_region_area, int(model.cluster_probe.clusters.shape[0]), connectivity))


def segment(model, img, run_crf=True, flip=True, res=None, maps=None, min_region_area=0, connectivity=4):
    """Normalised images [B, 3, H, W] -> (linear_preds, cluster_preds), int64 [B, res, res] (default: the images' H, W): the backbone
    on the images and on their mirror images, the fused probe head, then the dense CRF on both probes' probabilities (run_crf) and
    the argmax.  The CRF runs at the image's resolution, so `res` must equal it when run_crf is set.
    maps: a dict that receives what the backbone returned for the unflipped images, "feats" [B, C, h, w] and "code" [B, K, h, w]
    (stego_amd.feature_pca draws them); nothing else changes.
    min_region_area > 0: regions of either map (connected under `connectivity`, 4 or 8) with fewer pixels take the label most of their
    neighbours have (stego_amd.regions.merge_small_regions, on the device); 0 is the path without it."""
    if int(min_region_area) > 0:
        lin, clu = segment(model, img, run_crf=run_crf, flip=flip, res=res, maps=maps)
        return _clean(model, lin, clu, int(min_region_area), connectivity)
    _device_tensor(img, "img")
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError("img: expected [B, 3, H, W], got %s" % (tuple(img.shape),))
    size = tuple(img.shape[-2:]) if res is None else ((int(res), int(res)) if isinstance(res, int) else tuple(res))
    if run_crf and size != tuple(img.shape[-2:]):
        raise ValueError("segment: the CRF runs at the image's resolution %s, res = %s" % (tuple(img.shape[-2:]), size))
    with torch.no_grad():
        feats, code1 = model.net(img)
        if maps is not None:
            maps["feats"], maps["code"] = feats, code1
        code2 = model.net(img.flip(dims=[3]))[1] if flip else None
        kind = "probs" if run_crf else "argmax"
        lin, clu = probe_head(model, code1, code2, size, linear=kind, cluster=kind)
        if not run_crf:
            return lin, clu
        bgr = image_to_bgr_u8(img)
        return dense_crf_batch(bgr, lin).argmax(1), dense_crf_batch(bgr, clu).argmax(1)


def window_origins(L, win, stride):
    """Origins of the windows along an axis of length L (include/stego_stitch.h): n = 1 + ceil((L - win) / stride) windows at
    min(i * stride, L - win); the last one is shifted back so that it ends at the edge."""
    L, win, stride = int(L), int(win), int(stride)
    if win < 1 or L < win or stride > win or 2 * stride < win:
        raise ValueError("window_origins: need 1 <= win <= L and win <= 2 * stride <= 2 * win, got L = %d, win = %d, stride = %d"
                         % (L, win, stride))
    n = 1 + -((win - L) // stride)
    return [min(i * stride, L - win) for i in range(n)]


def _crf_fits(dev, n_labels, H, W):
    """Raise when the dense CRF's workspace and its two [n, H, W] planes do not fit the free device memory."""
    desc = capi.crf_desc(1, n_labels, H, W, MAX_ITER, POS_W, POS_XY_STD, Bi_W, Bi_XY_STD, Bi_RGB_STD)
    need = capi.crf_workspace_bytes(desc)
    if need == 0:
        raise RuntimeError("segment_large: the dense CRF does not take a %d x %d canvas with %d labels; pass run_crf=False"
                           % (H, W, n_labels))
    need += 4 * n_labels * H * W            # the CRF's output beside the probabilities that are already there
    free = torch.cuda.mem_get_info(dev)[0]
    if need > free:
        raise RuntimeError("segment_large: the dense CRF needs %.1f GiB for a %d x %d canvas with %d labels and %.1f GiB are free; "
                           "pass run_crf=False" % (need / 2.0 ** 30, H, W, n_labels, free / 2.0 ** 30))


def _segment_large_one(model, img, window, stride, batch, run_crf, flip):
    H, W = int(img.shape[1]), int(img.shape[2])
    T = len(window_origins(H, window, stride)) * len(window_origins(W, window, stride))
    codes, codes_flip = [], []
    for t0 in range(0, T, batch):
        n = min(batch, T - t0)
        wins = capi.window_gather(img, window, stride, t0, n, flip=flip)
        if flip:
            codes.append(model.net(wins[0])[1])
            codes_flip.append(model.net(wins[1])[1])
        else:
            codes.append(model.net(wins)[1])
    code = codes[0] if len(codes) == 1 else torch.cat(codes)
    code_flip = None if not flip else (codes_flip[0] if len(codes_flip) == 1 else torch.cat(codes_flip))
    lw = model.linear_probe.weight.detach()
    lw = lw.reshape(lw.shape[0], lw.shape[1])
    lb = model.linear_probe.bias.detach()
    cent = F.normalize(model.cluster_probe.clusters.detach(), dim=1)
    kind = "probs" if run_crf else "argmax"
    if run_crf:
        _crf_fits(img.device, max(int(lw.shape[0]), int(cent.shape[0])), H, W)
    lin, clu = capi.stitch_probe(code.detach().float(), None if code_flip is None else code_flip.detach().float(), lw, lb, cent, (H, W),
                                 window, stride, kind, kind, 2)
    del codes, codes_flip, code, code_flip
    if not run_crf:
        return lin, clu
    bgr = image_to_bgr_u8(img)
    lin = dense_crf_batch(bgr, lin.unsqueeze(0)).argmax(1)[0]
    return lin, dense_crf_batch(bgr, clu.unsqueeze(0)).argmax(1)[0]


def segment_large(model, img, window, stride=None, batch=16, run_crf=True, flip=True, min_region_area=0, connectivity=4):
    """A normalised image [3, H, W] of any size with H, W >= window (or [B, 3, H, W], image by image) -> (linear_preds,
    cluster_preds), int64 [H, W] (or [B, H, W]).  The image is cut into overlapping window x window pieces `stride` apart (default
    ceil(window / 2); window <= 2 * stride <= 2 * window; the last window of a row or column is shifted back to end at the edge), the
    windows - and their mirror images when `flip` - go through the backbone `batch` at a time, and one stitch_probe launch blends the
    windows' logits per pixel with tent weights and writes the canvas: the label maps directly, or the probabilities for the dense
    CRF (run_crf), which then runs on the whole canvas.  min_region_area, connectivity: as in segment(), on the canvas."""
    if int(min_region_area) > 0:
        lin, clu = segment_large(model, img, window, stride=stride, batch=batch, run_crf=run_crf, flip=flip)
        return _clean(model, lin, clu, int(min_region_area), connectivity)
    if not torch.is_tensor(img):
        raise TypeError("img: expected a torch tensor, got %s" % type(img).__name__)
    if img.dim() not in (3, 4) or img.shape[-3] != 3:
        raise ValueError("img: expected [3, H, W] or [B, 3, H, W], got %s" % (tuple(img.shape),))
    window = int(window)
    stride = (window + 1) // 2 if stride is None else int(stride)
    H, W = int(img.shape[-2]), int(img.shape[-1])
    if H < window or W < window:
        raise ValueError("segment_large: the image (%d x %d) is smaller than the window (%d); resize it and use segment()" % (H, W, window))
    if window < 1 or stride > window or 2 * stride < window:
        raise ValueError("segment_large: need window <= 2 * stride <= 2 * window, got window = %d, stride = %d" % (window, stride))
    if int(batch) < 1:
        raise ValueError("segment_large: batch = %r" % (batch,))
    _device_tensor(img, "img")
    with torch.no_grad():
        if img.dim() == 3:
            return _segment_large_one(model, img.float(), window, stride, int(batch), run_crf, flip)
        outs = [_segment_large_one(model, im.float(), window, stride, int(batch), run_crf, flip) for im in img]
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
