"""Attention salience masks: a foreground mask per image from the class token's attention in the last block of the DINO backbone
(include/stego_vit.h: stego_vit_forward_attn, stego_attn_salience; csrc/vit_cls_attn.hip).

The class token's attention of a DINO ViT outlines the foreground.  ``cfg.use_salience`` needs a foreground mask per image; a folder of
unlabelled photos has none, and the reference reads its masks from disk.  Here the mask is the smallest set of strongest patches that
holds ``keep`` of the attention mass (DINO's own visualisation recipe, per head with ``per_head=True``).

Definition (include/stego_vit.h), per image, in fp64 from the fp32 attention:
  m_i = sum over the heads of attn[b, head, 1 + i];  T = sum_i m_i;  ahead_i = sum of m_j over the patches before i in the order
  (m descending, index ascending on ties);  kept_i = ahead_i < keep * T;  soft = m / T;  mask = kept replicated over its patch.
"""
import torch

from . import capi

MAX_PATCHES = 4096          # the native limit of stego_attn_salience: 512 x 512 pixels at patch 8


def torch_attention_salience(attn, hw, patch, keep=0.6):
    """The definition in torch: fp64, a stable sort by (-m, index), an exclusive cumsum in that order.  Any device, any size."""
    h, w = hw
    B, heads, ntok = attn.shape
    m = attn[:, 0, 1:].double()
    for hd in range(1, heads):                              # head order
        m = m + attn[:, hd, 1:].double()
    T = m.cumsum(1)[:, -1:]                                 # index order
    order = torch.sort(-m, dim=1, stable=True)[1]
    sorted_m = m.gather(1, order)
    ahead_sorted = sorted_m.cumsum(1) - sorted_m
    ahead = torch.empty_like(m).scatter_(1, order, ahead_sorted)
    limit = torch.tensor(float(keep), dtype=torch.float32).double().item() * T
    kept = (ahead < limit).reshape(B, h, w)
    soft = (m / T).float().reshape(B, h, w)
    mask = kept.to(torch.uint8).repeat_interleave(patch, 1).repeat_interleave(patch, 2)
    return soft, mask


def attention_salience(attn, hw, patch, keep=0.6, per_head=False):
    """attn [B, heads, 1 + h*w] (DinoFeaturizer.class_attention) -> (soft float32 [B, h, w], mask uint8 [B, h*patch, w*patch]).
    per_head: one mask per head, [B * heads, ...] (the same call on attn.reshape(B * heads, 1, -1)).
    One native launch for float32 HIP tensors of up to 4096 patches, the torch restatement of the same definition otherwise."""
    h, w = int(hw[0]), int(hw[1])
    if attn.dim() != 3 or attn.shape[2] != 1 + h * w:
        raise ValueError("attention_salience: attn %s is not [B, heads, 1 + %d * %d]" % (tuple(attn.shape), h, w))
    if not 0.0 < keep <= 1.0:
        raise ValueError("attention_salience: keep = %r, expected 0 < keep <= 1" % (keep,))
    if per_head:
        attn = attn.reshape(attn.shape[0] * attn.shape[1], 1, attn.shape[2])
    B, heads = int(attn.shape[0]), int(attn.shape[1])
    if not (attn.is_cuda and attn.dtype == torch.float32 and patch in (8, 16) and h * w <= MAX_PATCHES and B > 0):
        return torch_attention_salience(attn, (h, w), patch, keep)
    attn = attn.contiguous()
    soft = torch.empty(B, h, w, dtype=torch.float32, device=attn.device)
    mask = torch.empty(B, h * patch, w * patch, dtype=torch.uint8, device=attn.device)
    with torch.cuda.device(attn.device):
        capi._check(capi.load().stego_attn_salience(attn.data_ptr(), B, heads, h, w, int(patch), float(keep), soft.data_ptr(), mask.data_ptr(),
                                                    capi._stream()))
    return soft, mask


def image_salience(featurizer, img, keep=0.6, per_head=False):
    """(soft, mask) of an image batch [B, 3, H, W] through a DinoFeaturizer: class_attention, then attention_salience."""
    ps = featurizer.patch_size
    return attention_salience(featurizer.class_attention(img), (img.shape[2] // ps, img.shape[3] // ps), ps, keep, per_head)
