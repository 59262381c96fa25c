"""The augmented view of the reference's aug-alignment term and the term itself.

The reference makes `img_aug` / `coord_aug` per item on CPU workers with torchvision (data.py:556-563, train_segmentation.py:408-416):
RandomHorizontalFlip -> RandomResizedCrop(res, scale=(0.8, 1)) -> ColorJitter(.3, .3, .3, .1) -> RandomGrayscale(.2) ->
RandomApply([GaussianBlur((5, 5))]), the geometric part replayed on a coordinate image.  torchvision is not part of this build: the
operators are restated in include/stego_aug.h and run on the device in one call (stego_augment) from a table of explicit draws.

  draw_aug_params      the draws of B images on the host: the reference's distributions from a CPU torch.Generator
  augment_batch        img [B, 3, H, W] + draws -> img_aug [B, 3, R, R], coord_aug [B, R, R, 2]
  aug_alignment_loss   -einsum(norm(sample(code, resize(coord_aug))), norm(code_aug)).mean() and its gradients to code and code_aug as
                       one fused call (stego_aug_align); torch_aug_alignment is the same chain in torch, for CPU tensors
  Augmenter            adds img_aug / coord_aug to a batch dict

The DISTRIBUTION of the draws is the reference's; the stream is not: it comes from one generator seeded from (seed, rank), as
DeviceContrastiveLoader's does, not from torchvision's calls on the per-worker global generators."""
import math

import torch
import torch.nn.functional as F

from . import capi

BRIGHTNESS, CONTRAST, SATURATION, HUE, NONE = capi.AUG_BRIGHTNESS, capi.AUG_CONTRAST, capi.AUG_SATURATION, capi.AUG_HUE, capi.AUG_NONE
SCALE = (0.8, 1.0)                  # RandomResizedCrop(scale=...)
RATIO = (3.0 / 4.0, 4.0 / 3.0)      # its default aspect range
JITTER = (0.3, 0.3, 0.3, 0.1)       # ColorJitter(brightness, contrast, saturation, hue)
P_FLIP, P_GRAY, P_BLUR = 0.5, 0.2, 0.5
SIGMA = (0.1, 2.0)                  # GaussianBlur's default sigma range


def make_params(H, W, flip=0, top=0, left=0, ch=None, cw=None, order=(NONE,) * 4, factors=(1.0, 1.0, 1.0, 0.0), gray=0, blur_sigma=0.0):
    """One StegoAugParams record; the defaults are the identity on an H x W image."""
    r = capi.StegoAugParams()
    r.flip, r.top, r.left = int(flip), int(top), int(left)
    r.ch, r.cw = int(H if ch is None else ch), int(W if cw is None else cw)
    r.order[:] = [int(o) for o in order]
    r.factor[:] = [float(f) for f in factors]
    r.gray, r.blur_sigma, r.reserved = int(gray), float(blur_sigma), 0
    return r


def params_table(records):
    """A list of StegoAugParams -> the ctypes array the native calls take."""
    return (capi.StegoAugParams * len(records))(*records)


def crop_size(H, W, area_fractions, aspects):
    """RandomResizedCrop.get_params without its generator: the first of the (up to ten) tries whose
    w = int(round(sqrt(area * aspect))), h = int(round(sqrt(area / aspect))) (Python's round: half to even) fits the image ->
    (h, w, index of the try); after the last failure the centred fallback with the aspect clamped to RATIO -> (h, w, None)."""
    for i, (frac, aspect) in enumerate(zip(area_fractions, aspects)):
        area = H * W * frac
        w = int(round(math.sqrt(area * aspect)))
        h = int(round(math.sqrt(area / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return h, w, i
    in_ratio = float(W) / float(H)
    if in_ratio < RATIO[0]:
        w = W
        h = int(round(w / RATIO[0]))
    elif in_ratio > RATIO[1]:
        h = H
        w = int(round(h * RATIO[1]))
    else:
        w, h = W, H
    return h, w, None


def _uniform(gen, lo, hi, n=None):
    u = torch.rand(() if n is None else (n,), generator=gen, dtype=torch.float64)
    return lo + (hi - lo) * u


def draw_aug_params(B, H, W, R, generator):
    """The draws of B images of H x W for a view of side R, from the CPU torch.Generator `generator`: a ctypes array of B
    StegoAugParams.  Per image, in this order: the flip (p = .5); RandomResizedCrop.get_params (ten tries of area = H W U(.8, 1),
    aspect = exp(U(log 3/4, log 4/3)), see crop_size; top and left uniform over the positions that fit; the centred fallback);
    a random permutation of the four jitter operators and their factors (brightness, contrast, saturation ~ U(.7, 1.3), hue ~
    U(-.1, .1)); gray (p = .2); blur (p = .5) with sigma ~ U(.1, 2).  The distribution is the reference's; the stream is this
    generator's own, not torchvision's (module docstring).  R does not enter the draws; it is checked with the records."""
    if generator is None or generator.device.type != "cpu":
        raise ValueError("draw_aug_params draws on the host: it needs a CPU torch.Generator")
    records = []
    for _ in range(int(B)):
        flip = int(torch.rand((), generator=generator).item() < P_FLIP)
        fracs = _uniform(generator, SCALE[0], SCALE[1], 10).tolist()
        aspects = torch.exp(_uniform(generator, math.log(RATIO[0]), math.log(RATIO[1]), 10)).tolist()
        ch, cw, hit = crop_size(H, W, fracs, aspects)
        if hit is None:
            top, left = (H - ch) // 2, (W - cw) // 2
        else:
            top = int(torch.randint(0, H - ch + 1, (), generator=generator).item())
            left = int(torch.randint(0, W - cw + 1, (), generator=generator).item())
        order = torch.randperm(4, generator=generator).tolist()
        factors = [float(_uniform(generator, 1 - j, 1 + j)) for j in JITTER[:3]] + [float(_uniform(generator, -JITTER[3], JITTER[3]))]
        gray = int(torch.rand((), generator=generator).item() < P_GRAY)
        blur = torch.rand((), generator=generator).item() < P_BLUR
        sigma = float(_uniform(generator, SIGMA[0], SIGMA[1])) if blur else 0.0
        records.append(make_params(H, W, flip, top, left, ch, cw, order, factors, gray, sigma))
    table = params_table(records)
    rc, bad, _ = capi.aug_check_params(capi.aug_desc(B, H, W, R), table)
    if rc != 0:
        raise ValueError("draw_aug_params(B=%d, H=%d, W=%d, R=%d): error %d%s" % (B, H, W, R, rc, " at record %d" % bad if bad >= 0 else ""))
    return table


def augment_batch(img, params, res=None):
    """img float32 [B, 3, H, W] on a HIP device + the B records `params` (draw_aug_params, or params_table of make_params records)
    -> (img_aug [B, 3, R, R], coord_aug [B, R, R, 2]) with R = `res` (default H, what the reference's RandomResizedCrop(cfg.res) on
    its res x res items gives).  One native call of at most two launches; the records go up in one small copy, nothing waits."""
    return capi.augment(img, params, int(img.shape[2] if res is None else res))


def torch_aug_alignment(code, code_aug, coord_aug):
    """train_segmentation.py:189-198 of the reference as it stands there: runs on any device and dtype (the oracle of the fused call)."""
    coord = F.interpolate(coord_aug.permute(0, 3, 1, 2), code_aug.shape[2], mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    sampled = F.grid_sample(code, coord.permute(0, 2, 1, 3), padding_mode="border", align_corners=True)
    return -torch.einsum("bkhw,bkhw->bhw", F.normalize(sampled, dim=1, eps=1e-10), F.normalize(code_aug, dim=1, eps=1e-10)).mean()


class _AugAlign(torch.autograd.Function):
    """Forward: the one fused call; it already holds both gradients for a unit upstream.  Backward: scale them."""

    @staticmethod
    def forward(ctx, code, code_aug, coord):
        need = ctx.needs_input_grad[:2]
        loss, d_code, d_code_aug = capi.aug_align(code.detach(), code_aug.detach(), coord, need_code=need[0], need_code_aug=need[1])
        ctx.need = need
        ctx.save_for_backward(*[g for g in (d_code, d_code_aug) if g is not None])
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        d_code = saved.pop(0) * g if ctx.need[0] else None
        d_code_aug = saved.pop(0) * g if ctx.need[1] else None
        return d_code, d_code_aug, None


def _native_ok(code, code_aug, coord):
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for t in (code, code_aug, coord)):
        return False
    if code_aug.device != code.device or coord.device != code.device or coord.requires_grad:
        return False
    if code_aug.shape[:2] != code.shape[:2] or code_aug.shape[2] != code_aug.shape[3] or coord.shape[0] != code.shape[0] or coord.shape[3] != 2:
        return False
    B, K, h, w = code.shape
    return (1 <= B <= 65535 and 1 <= K <= capi.AUGALIGN_MAX_K and all(1 <= s <= capi.AUGALIGN_MAX_SIDE for s in (h, w, code_aug.shape[2]))
            and all(1 <= s <= capi.AUG_MAX_SIDE for s in coord.shape[1:3]))


def aug_alignment_loss(code, code_aug, coord_aug):
    """The 0-dim aug-alignment term whose backward reaches `code` and `code_aug`.  One native call for float32 tensors on a HIP device
    with sizes inside the kernel's limits (include/stego_aug.h); the torch chain for anything else."""
    if not _native_ok(code, code_aug, coord_aug):
        return torch_aug_alignment(code, code_aug, coord_aug)
    return _AugAlign.apply(code, code_aug, coord_aug)


class Augmenter:
    """Adds `img_aug` / `coord_aug` to a batch dict from its `img`.  The draws come from a CPU generator seeded from (seed, rank):
    two augmenters built alike give identical views, but the stream is not torchvision's per-worker one.  `last_params` holds the
    records of the latest batch."""

    def __init__(self, res, seed=0, rank=0):
        self.res = int(res)
        self._gen = torch.Generator()
        self._gen.manual_seed((int(seed) * 1000003 + int(rank) + 0x5A17) & 0x7FFFFFFFFFFFFFFF)
        self.last_params = None

    def views(self, img):
        B, _, H, W = img.shape
        self.last_params = draw_aug_params(B, H, W, self.res, self._gen)
        return augment_batch(img, self.last_params, self.res)

    def __call__(self, batch):
        batch["img_aug"], batch["coord_aug"] = self.views(batch["img"])
        return batch


def needs_torchvision(cfg):
    """The message with which my_app refuses a configuration on real data, or None: aug_alignment_weight > 0 needs the augmented
    view, which exists only as the native path behind cfg.native_aug."""
    if cfg.aug_alignment_weight > 0 and not getattr(cfg, "native_aug", False):
        return ("cfg.aug_alignment_weight = %s: the img_aug / coord_aug augmentations need torchvision's photometric transforms, which "
                "this build does not have; set native_aug=True (the views and the term from stego_amd.augment's native kernels) or "
                "aug_alignment_weight=0 to train on real data" % cfg.aug_alignment_weight)
    return None
