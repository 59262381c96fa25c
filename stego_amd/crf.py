"""Drop-in for the reference's ``src/crf.py`` (and ``batched_crf`` of ``src/eval_segmentation.py:48-54``): the fully-connected CRF
STEGO's "+CRF" numbers are evaluated with, on the MI355X.

The reference hands every image to pydensecrf on the CPU, one image per process of a multiprocessing.Pool.  Here the whole batch
goes through csrc/dense_crf.hip (include/stego_crf.h) in one call: the same mathematics - unary -log(clip(p, 1e-5, 1)), a Gaussian
kernel on position and a bilateral kernel on position and colour, each a symmetric-normalised permutohedral-lattice filter, ten
mean-field iterations with Potts compatibility - computed on device tensors.  There is no CPU path: CPU tensors raise.

Agreement with pydensecrf itself is not verified (the library is not available offline); tests/crf_oracle.py restates the algorithm
as densecrf implements it and the kernels are tested against that restatement, see INTEGRATION.md.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import capi

MAX_ITER = 10
POS_W = 3
POS_XY_STD = 1
Bi_W = 4
Bi_XY_STD = 67
Bi_RGB_STD = 3
BGR_MEAN = np.array([104.008, 116.669, 122.675])

# ImageNet normalisation the loaders apply and utils.unnorm undoes (reference src/utils.py:141)
_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)


def _device_tensor(t, what):
    if not torch.is_tensor(t):
        raise TypeError("%s: expected a torch tensor, got %s" % (what, type(t).__name__))
    if not t.is_cuda:
        raise RuntimeError("stego_amd runs on MI355X only: %s is a %s tensor (no CPU fallback exists)" % (what, t.device))
    return t


def image_to_bgr_u8(img):
    """Normalised images [B, 3, H, W] (or [3, H, W]) -> uint8 [B, H, W, 3] in BGR order, as crf.py:23 makes them:
    unnorm (x * std + mean per channel), then torchvision's to_pil_image (x * 255 truncated to uint8), then `[:, :, ::-1]`.
    Values outside [0, 255] are clamped before the truncation: to_pil_image leaves their conversion to the cast (undefined for
    out-of-range floats), and an image that went through the loaders' normalisation has none."""
    _device_tensor(img, "image")
    return _to_bgr_u8(img)


def _to_bgr_u8(img):
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[1] != 3 or not img.is_floating_point():
        raise ValueError("image: expected a floating-point [B, 3, H, W] tensor, got %s %s" % (img.dtype, tuple(img.shape)))
    img = img.float()
    mean = torch.tensor(_MEAN, dtype=torch.float32, device=img.device).view(1, 3, 1, 1)
    std = torch.tensor(_STD, dtype=torch.float32, device=img.device).view(1, 3, 1, 1)
    x = (img * std + mean) * 255.0                  # UnNormalize: t.mul_(s).add_(m); to_pil_image: pic.mul(255).byte()
    x = x.clamp_(0.0, 255.0).to(torch.uint8)        # float -> uint8 truncates toward zero, as .byte() does
    return x.flip(1).permute(0, 2, 3, 1).contiguous()


def dense_crf_batch(bgr_u8, probs, n_iter=MAX_ITER, pos_w=POS_W, pos_xy_std=POS_XY_STD, bi_w=Bi_W, bi_xy_std=Bi_XY_STD,
                    bi_rgb_std=Bi_RGB_STD):
    """The CRF on device tensors: bgr_u8 uint8 [B, H, W, 3] (BGR), probs float32 [B, C, H, W] at the image's resolution ->
    Q float32 [B, C, H, W].  1 <= C <= 64."""
    if not torch.is_tensor(bgr_u8) or not torch.is_tensor(probs):
        raise TypeError("dense_crf_batch expects torch tensors")
    if bgr_u8.dtype != torch.uint8 or bgr_u8.dim() != 4 or bgr_u8.shape[3] != 3:
        raise ValueError("bgr_u8: expected uint8 [B, H, W, 3], got %s %s" % (bgr_u8.dtype, tuple(bgr_u8.shape)))
    if probs.dtype != torch.float32 or probs.dim() != 4:
        raise ValueError("probs: expected float32 [B, C, H, W], got %s %s" % (probs.dtype, tuple(probs.shape)))
    B, C, H, W = probs.shape
    if tuple(bgr_u8.shape[:3]) != (B, H, W):
        raise ValueError("bgr_u8 %s does not match probs %s" % (tuple(bgr_u8.shape), tuple(probs.shape)))
    if bgr_u8.device != probs.device:
        raise ValueError("bgr_u8 and probs are on different devices (%s, %s)" % (bgr_u8.device, probs.device))
    if not 1 <= C <= 64:
        raise ValueError("probs: %d labels, the CRF kernels take 1 .. 64" % C)
    _device_tensor(bgr_u8, "bgr_u8")
    _device_tensor(probs, "probs")
    desc = capi.crf_desc(B, C, H, W, n_iter, pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std)
    return capi.crf_run(desc, bgr_u8.contiguous(), probs.contiguous())


def _probs_at(logits, H, W):
    """crf.py:27-29: bilinear resize (align_corners=False) of [B, C, h, w] logits to (H, W), softmax over C."""
    logits = logits.float()
    if tuple(logits.shape[-2:]) != (H, W):
        logits = F.interpolate(logits, size=(H, W), mode="bilinear", align_corners=False)
    return F.softmax(logits, dim=1).contiguous()


def dense_crf(image_tensor, output_logits):
    """crf.py:22-45: image_tensor [3, H, W] (normalised), output_logits [C, h, w] -> Q as a numpy float32 [C, H, W] array."""
    _device_tensor(image_tensor, "image_tensor")
    _device_tensor(output_logits, "output_logits")
    if image_tensor.dim() != 3 or output_logits.dim() != 3:
        raise ValueError("dense_crf expects image [3, H, W] and logits [C, h, w], got %s and %s"
                         % (tuple(image_tensor.shape), tuple(output_logits.shape)))
    with torch.no_grad():
        bgr = image_to_bgr_u8(image_tensor)
        H, W = bgr.shape[1:3]
        q = dense_crf_batch(bgr, _probs_at(output_logits.unsqueeze(0), H, W))
    return q[0].cpu().numpy()


def batched_crf(pool, img_tensor, prob_tensor):
    """eval_segmentation.py:52-54: images [B, 3, H, W], (log-)probabilities or logits [B, C, h, w] -> Q [B, C, H, W] on the
    input's device.  `pool` (the reference's multiprocessing.Pool) is accepted and ignored: the batch is one device call."""
    _device_tensor(img_tensor, "img_tensor")
    _device_tensor(prob_tensor, "prob_tensor")
    if img_tensor.dim() != 4 or prob_tensor.dim() != 4 or img_tensor.shape[0] != prob_tensor.shape[0]:
        raise ValueError("batched_crf expects images [B, 3, H, W] and logits [B, C, h, w], got %s and %s"
                         % (tuple(img_tensor.shape), tuple(prob_tensor.shape)))
    with torch.no_grad():
        bgr = image_to_bgr_u8(img_tensor.detach())
        H, W = bgr.shape[1:3]
        return dense_crf_batch(bgr, _probs_at(prob_tensor.detach(), H, W))
