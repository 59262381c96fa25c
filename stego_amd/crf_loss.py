"""The mean of the reference's ContrastiveCRFLoss (modules.py:437-469) over sampled points of resized maps, as the torch chain
train_segmentation.py:202-208 runs it - interpolate both maps, normalise the code, gather the points, build the [B, N, N] kernel and
gram matrices, .mean() - or as one fused native call (include/stego_crf_loss.h) that samples only the N points and returns the scalar
with its gradient to the code."""
import math

import torch
import torch.nn.functional as F

from . import capi


def _params(params):
    alpha, beta, gamma, w1, w2, shift = (float(v) for v in params)
    return alpha, beta, gamma, w1, w2, shift


def torch_crf_mean_loss(guidance, code, coords, size, params, normalize=True):
    """crf(resize(guidance, size), norm(resize(code, size))).mean() with the points `coords` (int64 [2, N]: rows, columns) instead of
    the module's own draw; size = (H, W); params = (alpha, beta, gamma, w1, w2, shift); normalize=False skips the norm."""
    alpha, beta, gamma, w1, w2, shift = _params(params)
    size = (int(size[0]), int(size[1]))
    guidance = F.interpolate(guidance, size, mode="bilinear", align_corners=False)
    clusters = F.interpolate(code, size, mode="bilinear", align_corners=False)
    if normalize:
        clusters = F.normalize(clusters, dim=1, eps=1e-10)
    g = guidance[:, :, coords[0], coords[1]]
    d_xy = (coords.unsqueeze(-1) - coords.unsqueeze(1)).square().sum(0).unsqueeze(0)
    d_g = (g.unsqueeze(-1) - g.unsqueeze(2)).square().sum(1)
    kernel = w1 * torch.exp(-d_xy / (2 * alpha) - d_g / (2 * beta)) + w2 * torch.exp(-d_xy / (2 * gamma)) - shift
    c = clusters[:, :, coords[0], coords[1]]
    return (-(torch.einsum("nka,nkb->nab", c, c) * kernel)).mean()


class _CrfMeanLoss(torch.autograd.Function):
    """Forward: the one fused call; it already holds d loss / d code for a unit upstream.  Backward: scale it."""

    @staticmethod
    def forward(ctx, code, guidance, coords, size, params, normalize):
        need = ctx.needs_input_grad[0]
        loss, _, d_code = capi.crf_loss(guidance, code.detach(), coords, size, params, normalize=normalize, need_grad=need,
                                        want_per_image=False)
        if need:
            ctx.save_for_backward(d_code)
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (d_code,) = ctx.saved_tensors
        return d_code * g, None, None, None, None, None


def _native_ok(guidance, code, coords, size, params):
    if not (torch.is_tensor(guidance) and torch.is_tensor(code) and torch.is_tensor(coords)):
        return False
    if not (code.is_cuda and guidance.device == code.device and coords.device == code.device):
        return False
    if code.dtype != torch.float32 or guidance.dtype != torch.float32 or coords.dtype != torch.int64 or guidance.requires_grad:
        return False
    if code.dim() != 4 or guidance.dim() != 4 or coords.dim() != 2 or coords.shape[0] != 2 or guidance.shape[0] != code.shape[0]:
        return False
    B, K, h, w = code.shape
    G, hg, wg = guidance.shape[1:]
    sides = (h, w, hg, wg, int(size[0]), int(size[1]))
    if not (1 <= B <= 65535 and 1 <= K <= capi.CRFLOSS_MAX_K and 1 <= G <= capi.CRFLOSS_MAX_G and
            1 <= coords.shape[1] <= capi.CRFLOSS_MAX_POINTS and all(1 <= s <= capi.CRFLOSS_MAX_SIDE for s in sides)):
        return False
    p = _params(params)
    return all(math.isfinite(v) and abs(v) < 1e30 for v in p) and all(v > 1e-30 for v in p[:3])     # finite and > 0 as float32 too


def crf_mean_loss(guidance, code, coords, size, params, normalize=True):
    """The 0-dim mean CRF loss whose backward reaches `code` alone.  One native call for float32 tensors on a HIP device with sizes
    inside the kernel's limits and a guidance that needs no gradient; the torch chain for anything else."""
    if not _native_ok(guidance, code, coords, size, params):
        return torch_crf_mean_loss(guidance, code, coords, size, params, normalize)
    return _CrfMeanLoss.apply(code, guidance, coords, (int(size[0]), int(size[1])), _params(params), bool(normalize))
