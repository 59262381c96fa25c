"""Feature pictures: a backbone feature map or the segmentation code as the false-colour picture of its three principal components
(include/stego_pca.h, csrc/feature_pca.hip).

The reference draws it on the host (src/train_crf.py:145-150): ``PCA(n_components=3).fit_transform(code)``, ``(p + 1) / 2``, clip,
``imshow``.  Here the map stays on the device: the centred second moments on the fp32-input matrix instruction, the three leading
eigenpairs in fp64 by one workgroup per fit, the scores in one read of the map, and one launch that resizes the small score map and
writes packed RGB bytes - into a tensor of its own or into a panel of a larger sheet (``render.comparison_sheet``).

A map is float32 [B, C, h, w] with any strides (the channels-last view the backbone returns is the fast case).  ``joint=False`` fits
every image on its own, as the reference does; ``joint=True`` fits all B h w tokens together, so the images of a batch share their
colours.  CPU tensors go through ``torch_feature_pictures``, the same arithmetic as a torch chain; a HIP tensor outside the kernels'
limits is an error that names the limit.
"""
import torch
import torch.nn.functional as F

from . import capi
from .render import _check_out, _native_target

DROP = 2.0 ** -20          # a component whose eigenvalue is at most this share of the trace is dropped (include/stego_pca.h)


class FeaturePCA:
    """A fitted model: ``mean`` float32 [G, C], ``basis`` float32 [G, 3, C], ``stats`` float32 [G, 3, 3] = (eigenvalue, its share of the
    trace, residual |cov v - lambda v| / lambda_1) and ``cov`` float64 [G, C, C], device tensors nobody has synchronised on.  G is 1
    for a joint model, which applies to any batch, else the number of images it was fitted on."""

    def __init__(self, mean, basis, stats, cov, joint):
        self.mean, self.basis, self.stats, self.cov, self.joint = mean, basis, stats, cov, bool(joint)

    @property
    def groups(self):
        return int(self.mean.shape[0])

    def scores(self, maps):
        """(x - mean) . basis of every token -> float32 [B, h, w, 3]."""
        return _scores(self, _checked(maps))[0]


def _checked(maps):
    if not torch.is_tensor(maps) or maps.dim() != 4:
        raise ValueError("maps: expected a [B, C, h, w] tensor, got %s" % (tuple(maps.shape) if torch.is_tensor(maps) else type(maps),))
    return maps


def _native(maps):
    return maps.is_cuda and maps.dtype == torch.float32


def _check_limits(B, C, h, w, joint, size=None, n_iter=capi.PCA_DEFAULT_ITER):
    """The limits of include/stego_pca.h, by name."""
    if not capi.PCA_MIN_C <= C <= capi.PCA_MAX_C:
        raise ValueError("feature_pca: C = %d channels, the kernels take %d .. %d" % (C, capi.PCA_MIN_C, capi.PCA_MAX_C))
    if not 1 <= B <= capi.PCA_MAX_B:
        raise ValueError("feature_pca: B = %d images, the kernels take 1 .. %d" % (B, capi.PCA_MAX_B))
    if not (1 <= h <= capi.PCA_MAX_SIDE and 1 <= w <= capi.PCA_MAX_SIDE):
        raise ValueError("feature_pca: a %d x %d map, the kernels take sides of 1 .. %d" % (h, w, capi.PCA_MAX_SIDE))
    if B * h * w > capi.PCA_MAX_TOKENS:
        raise ValueError("feature_pca: %d tokens, the kernels take %d at the most" % (B * h * w, capi.PCA_MAX_TOKENS))
    if h * w * (B if joint else 1) < capi.PCA_MIN_TOKENS:
        raise ValueError("feature_pca: %d tokens in a group, a fit needs %d at the least" % (h * w * (B if joint else 1), capi.PCA_MIN_TOKENS))
    if not 1 <= int(n_iter) <= capi.PCA_MAX_ITER:
        raise ValueError("feature_pca: n_iter = %d, the kernels take 1 .. %d" % (n_iter, capi.PCA_MAX_ITER))
    if size is not None and not (1 <= size[0] <= capi.STITCH_MAX_SIDE and 1 <= size[1] <= capi.STITCH_MAX_SIDE):
        raise ValueError("feature_pca: a %d x %d picture, the kernels take sides of 1 .. %d" % (size[0], size[1], capi.STITCH_MAX_SIDE))


def _mode(table, value, name):
    if value not in table:
        raise ValueError("feature_pca: %s = %r, expected one of %s" % (name, value, sorted(table)))
    return table[value]


# ---- the torch chain
def _tokens(maps, joint):
    """[B, C, h, w] -> float32 [G, n, C]."""
    B, C, h, w = maps.shape
    x = maps.float().permute(0, 2, 3, 1).reshape(B, h * w, C)
    return x.reshape(1, B * h * w, C) if joint else x


def torch_fit(maps, joint=False):
    """fit as a torch chain on the tensor's device: the float32 of the fp64 mean, the centred second moments as an fp32 product,
    torch.linalg.eigh in float64, the sign rule and the drop rule of include/stego_pca.h."""
    maps = _checked(maps)
    x = _tokens(maps, joint)
    G, n, C = x.shape
    if C < 3 or n < 2:
        raise ValueError("feature_pca: a fit needs 3 channels and 2 tokens, got C = %d, n = %d" % (C, n))
    mean = x.double().mean(1).float()
    xc = x - mean[:, None, :]
    cov = (xc.transpose(1, 2) @ xc).double() / (n - 1)
    lam, vec = torch.linalg.eigh(cov)
    lam, vec = lam.flip(-1)[:, :3], vec.flip(-1)[:, :, :3].transpose(1, 2)            # descending; [G, 3, C]
    top = vec.abs().argmax(-1, keepdim=True)                                           # the first of equal maxima: the lowest channel
    vec = vec * torch.where(vec.gather(-1, top) < 0, -1.0, 1.0)
    trace = cov.diagonal(dim1=1, dim2=2).sum(-1, keepdim=True)
    keep = lam > DROP * trace
    resid = ((cov @ vec.transpose(1, 2)).transpose(1, 2) - lam[..., None] * vec).norm(dim=-1)
    lam1 = lam[:, :1]
    zero = torch.zeros_like(lam)
    stats = torch.stack([torch.where(keep, lam, zero), torch.where(keep, lam / trace, zero),
                         torch.where(keep, resid / lam1, zero)], -1).float()
    basis = torch.where(keep[..., None], vec, torch.zeros_like(vec)).float()
    return FeaturePCA(mean, basis, stats, cov, joint)


def _torch_scores(pca, maps):
    B, C, h, w = maps.shape
    joint = pca.groups == 1
    x = _tokens(maps, joint)
    s = (x - pca.mean[:, None, :]) @ pca.basis.transpose(1, 2)                         # [G, n, 3]
    rng = torch.stack([s.amin(1), s.amax(1)], -1)                                      # [G, 3, 2]
    return s.reshape(B, h, w, 3), rng


def _torch_paint(scores, rng, size, scale, resize):
    B, h, w, _ = scores.shape
    s = scores.permute(0, 3, 1, 2)
    if resize == "bilinear":
        s = F.interpolate(s, size=size, mode="bilinear", align_corners=False)
    else:
        s = F.interpolate(s, size=size, mode="nearest")
    s = s.permute(0, 2, 3, 1)
    if scale == "unit":
        v = (s + 1.0) / 2.0
    else:
        lo, hi = rng[..., 0], rng[..., 1]                                              # [G, 3]
        lo, hi = lo[:, None, None, :], hi[:, None, None, :]
        v = torch.where(hi > lo, (s - lo) / (hi - lo), torch.zeros_like(s))
    v = v * 255.0
    return torch.where(torch.isnan(v), torch.zeros_like(v), v).clamp(0, 255).to(torch.uint8)


def torch_feature_pictures(maps, size=None, joint=False, scale="unit", resize="bilinear", pca=None, out=None):
    """feature_pictures as a torch chain on the tensor's device."""
    maps = _checked(maps)
    B, C, h, w = maps.shape
    size = (h, w) if size is None else (int(size[0]), int(size[1]))
    _mode(capi.PCA_SCALES, scale, "scale")
    _mode(capi.PCA_RESIZES, resize, "resize")
    _check_out(out, (B, size[0], size[1], 3))
    pca = torch_fit(maps, joint) if pca is None else _usable(pca, B, C)
    scores, rng = _torch_scores(pca, maps.float())
    res = _torch_paint(scores, rng, size, scale, resize)
    if out is not None:
        out.copy_(res)
        return out
    return res


# ---- the kernels
def _usable(pca, B, C):
    if pca.mean.shape[1] != C:
        raise ValueError("feature_pca: the model has %d channels, the map %d" % (pca.mean.shape[1], C))
    if pca.groups != 1 and pca.groups != B:
        raise ValueError("feature_pca: a per-image model of %d images does not apply to a batch of %d (a joint model applies to any batch)"
                         % (pca.groups, B))
    return pca


def fit(maps, joint=False, n_iter=capi.PCA_DEFAULT_ITER):
    """The three leading principal components of a map [B, C, h, w]: per image, or of all its tokens together (joint) -> FeaturePCA.
    n_iter: iterations of the subspace iteration (1 .. 256); ``stats[..., 2]`` tells how far they got."""
    maps = _checked(maps)
    if not _native(maps):
        return torch_fit(maps, joint)
    B, C, h, w = maps.shape
    _check_limits(B, C, h, w, joint, n_iter=n_iter)
    desc = capi.pca_desc(B, C, h, w, joint=bool(joint), n_iter=n_iter)
    mean, cov, basis, stats = capi.pca_fit(desc, maps)
    return FeaturePCA(mean, basis, stats, cov, joint)


def _scores(pca, maps):
    """-> (scores [B, h, w, 3], range [G, 3, 2]) of a map under a model."""
    B, C, h, w = maps.shape
    _usable(pca, B, C)
    if not (_native(maps) and pca.mean.is_cuda):
        return _torch_scores(pca, maps.float())
    joint = pca.groups == 1
    _check_limits(B, C, h, w, joint)
    desc = capi.pca_desc(B, C, h, w, joint=joint)
    return capi.pca_scores(desc, maps, pca.mean, pca.basis)


def feature_pictures(maps, size=None, joint=False, scale="unit", resize="bilinear", pca=None, out=None, n_iter=capi.PCA_DEFAULT_ITER):
    """A map [B, C, h, w] -> uint8 [B, H, W, 3], its three leading principal components as red, green and blue, or into the view `out`
    of that shape (a panel of a larger sheet: any image and row stride).
    size: (H, W) of the picture, default (h, w); resize: "bilinear" (F.interpolate's, align_corners=False) or "nearest".
    scale: "unit" shows (p + 1) / 2 clipped, the reference's, meant for L2-normalised codes; "range" brings every component to the
    range it has in its group.
    pca: a model fitted earlier (``fit``) instead of a fit of this map: a joint model applies to any batch, a per-image model to a
    batch of as many images."""
    maps = _checked(maps)
    B, C, h, w = maps.shape
    size = (h, w) if size is None else (int(size[0]), int(size[1]))
    H, W = size
    rs, sc = _mode(capi.PCA_RESIZES, resize, "resize"), _mode(capi.PCA_SCALES, scale, "scale")
    _check_out(out, (B, H, W, 3))
    if not _native(maps) or (pca is not None and not pca.mean.is_cuda):
        return torch_feature_pictures(maps, size, joint, scale, resize, pca, out)
    if pca is None:
        pca = fit(maps, joint, n_iter)
    joint = pca.groups == 1
    _check_limits(B, C, h, w, joint, size)
    scores, rng = _scores(pca, maps)
    direct = _native_target(out, B, H, W, maps.device)
    res = out if (out is not None and direct) else torch.empty((B, H, W, 3), dtype=torch.uint8, device=maps.device)
    desc = capi.pca_desc(B, C, h, w, H, W, joint=joint, resize=rs, scale=sc, out_strides=(res.stride(0), res.stride(1)))
    capi.pca_paint(desc, scores, rng, res)
    if out is not None and not direct:
        out.copy_(res)
    return out if out is not None else res
