"""The reconstruction term of the reference's training step (train_segmentation.py:183-187): the negative mean cosine between the
decoded code and the backbone features, as the torch chain runs it - decode, normalise both maps, multiply, sum, mean - or as one fused
native call (include/stego_rec.h) that writes no [B, C, h, w] tensor and returns the scalar with its gradients to the code and to the
decoder's weight and bias."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import capi


def torch_rec_loss(code, feats, decoder):
    """-(norm(decoder(code)) * norm(feats)).sum(1).mean() as it stands in the training step: runs on any device and dtype (the oracle
    of the fused call)."""
    return -(F.normalize(decoder(code), dim=1, eps=1e-10) * F.normalize(feats, dim=1, eps=1e-10)).sum(1).mean()


class _RecLoss(torch.autograd.Function):
    """Forward: the one fused call; it already holds the three gradients for a unit upstream.  Backward: scale them."""

    @staticmethod
    def forward(ctx, code, weight, bias, feats):
        need = ctx.needs_input_grad[:3]
        loss, d_code, d_weight, d_bias = capi.rec_loss(code.detach(), feats, weight.detach(), bias.detach(), need_code=need[0],
                                                       need_weight=need[1], need_bias=need[2])
        ctx.need = need
        ctx.save_for_backward(*[g for g in (d_code, d_weight, d_bias) if g is not None])
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        return tuple(saved.pop(0) * g if n else None for n in ctx.need) + (None,)


def _native_ok(code, feats, decoder):
    if not (torch.is_tensor(code) and torch.is_tensor(feats) and isinstance(decoder, nn.Conv2d)):
        return False
    if not (code.is_cuda and feats.device == code.device and code.dtype == torch.float32 and feats.dtype == torch.float32):
        return False
    if code.dim() != 4 or feats.dim() != 4 or feats.shape[0] != code.shape[0] or feats.shape[2:] != code.shape[2:] or feats.requires_grad:
        return False
    B, K, h, w = code.shape
    C = feats.shape[1]
    if decoder.kernel_size != (1, 1) or decoder.stride != (1, 1) or decoder.padding != (0, 0) or decoder.dilation != (1, 1) or \
            decoder.groups != 1 or decoder.bias is None or (decoder.in_channels, decoder.out_channels) != (K, C):
        return False
    if decoder.weight.device != code.device or decoder.weight.dtype != torch.float32 or decoder.bias.dtype != torch.float32:
        return False
    return (1 <= B <= capi.REC_MAX_B and 1 <= K <= capi.REC_MAX_K and 1 <= C <= capi.REC_MAX_C and 1 <= h <= capi.REC_MAX_SIDE and
            1 <= w <= capi.REC_MAX_SIDE and B * h * w <= capi.REC_MAX_TOKENS)


def rec_loss(code, feats, decoder):
    """The 0-dim reconstruction term whose backward reaches `code` and the decoder's weight and bias.  One native call for float32 maps
    on a HIP device, a decoder that is a 1 x 1 nn.Conv2d with a bias, feats that need no gradient and sizes inside the kernel's limits
    (include/stego_rec.h); the torch chain for anything else."""
    if not _native_ok(code, feats, decoder):
        return torch_rec_loss(code, feats, decoder)
    return _RecLoss.apply(code, decoder.weight, decoder.bias, feats)
