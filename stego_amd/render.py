"""Coloured segmentation pictures: label maps through a colormap, images as uint8, the image under the label colours with the
boundaries drawn, and contact sheets of such panels (include/stego_render.h, csrc/render.hip).

The reference colours on the host, pixel by pixel in numpy: ``model.label_cmap[label]`` and ``(prep_for_plot(img) * 255)
.astype(np.uint8)`` (src/eval_segmentation.py:181-193).  Here the label maps, the images and the canvases of ``segment_large`` are on
the device already, and one launch writes packed RGB bytes - into a tensor of its own or into its place on a larger sheet.

Every function runs anywhere: CPU tensors, label dtypes the kernel does not read, tables of more than 512 colours and sides beyond the
kernel's limits go through ``torch_colorize`` / ``torch_image_u8``, the same arithmetic as a torch chain.

``prep_for_plot`` hands ``unnorm`` a [1, 3, H, W] tensor, and ``UnNormalize.__call__`` walks its leading axis beside the three
constants: one step, so all three channels are un-normalised with the first channel's std and mean (0.229, 0.485).  With the rescale
to the image's own range that is what the reference's pictures show, and ``PLOT_MEAN`` / ``PLOT_STD``, the defaults of ``image_u8``,
reproduce it.  ``IMAGENET_MEAN`` / ``IMAGENET_STD`` are the per-channel constants the loaders normalise with: the true colours.
"""
import numpy as np
import torch

from . import capi

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
PLOT_MEAN, PLOT_STD = (0.485, 0.485, 0.485), (0.229, 0.229, 0.229)
EDGE_COLOR = (255, 255, 255)

# The 27 classes of the Cityscapes evaluation as this project's datasets number them, with the colour the Cityscapes label table gives
# each, and black for everything else.
_CITYSCAPES = (
    ("road", (128, 64, 128)), ("sidewalk", (244, 35, 232)), ("parking", (250, 170, 160)), ("rail track", (230, 150, 140)),
    ("building", (70, 70, 70)), ("wall", (102, 102, 156)), ("fence", (190, 153, 153)), ("guard rail", (180, 165, 180)),
    ("bridge", (150, 100, 100)), ("tunnel", (150, 120, 90)), ("pole", (153, 153, 153)), ("polegroup", (153, 153, 153)),
    ("traffic light", (250, 170, 30)), ("traffic sign", (220, 220, 0)), ("vegetation", (107, 142, 35)), ("terrain", (152, 251, 152)),
    ("sky", (70, 130, 180)), ("person", (220, 20, 60)), ("rider", (255, 0, 0)), ("car", (0, 0, 142)), ("truck", (0, 0, 70)),
    ("bus", (0, 60, 100)), ("caravan", (0, 0, 90)), ("trailer", (0, 0, 110)), ("train", (0, 80, 100)), ("motorcycle", (0, 0, 230)),
    ("bicycle", (119, 11, 32)), ("void", (0, 0, 0)))


def pascal_label_colormap(n=512):
    """The PASCAL VOC colormap, int [n, 3]: bit k of a channel's value, counted from the top, is bit 3 k + channel of the index."""
    index = np.arange(n, dtype=int)
    cmap = np.zeros((n, 3), dtype=int)
    for channel in range(3):
        for k in range(8):
            cmap[:, channel] |= ((index >> (3 * k + channel)) & 1) << (7 - k)
    return cmap


def cityscapes_colormap():
    """The Cityscapes palette in the 27-class order plus black, int [28, 3]."""
    return np.array([rgb for _, rgb in _CITYSCAPES], dtype=int)


def label_cmap(dataset_name):
    """The colormap LitUnsupervisedSegmenter.label_cmap holds for a dataset (the reference's train_segmentation.py:100-103)."""
    return cityscapes_colormap() if str(dataset_name).startswith("cityscapes") else pascal_label_colormap()


def _table(cmap, mapping):
    """-> (uint8 [n_lut, 3] table, its ignore colour): cmap itself, or cmap[mapping[k]] per cluster k with cmap[-1] where the
    mapping has no class (-1, or anything outside the colormap)."""
    cmap = np.asarray(cmap.cpu() if torch.is_tensor(cmap) else cmap)
    if cmap.ndim != 2 or cmap.shape[1] != 3 or cmap.shape[0] < 1:
        raise ValueError("cmap: expected [n, 3], got %s" % (cmap.shape,))
    cmap = cmap.astype(np.uint8)
    ignore = cmap[-1]
    if mapping is None:
        return cmap, ignore
    mapping = np.asarray(mapping.cpu() if torch.is_tensor(mapping) else mapping).astype(np.int64).reshape(-1)
    ok = (mapping >= 0) & (mapping < cmap.shape[0])
    table = np.where(ok[:, None], cmap[np.where(ok, mapping, 0)], ignore[None, :]).astype(np.uint8)
    return table, ignore


def _unnormalised(img, mean, std):
    v = img.clone()
    for c in range(3):
        v[:, c].mul_(float(std[c])).add_(float(mean[c]))
    return v


def _unit(img, rescale, mean, std):
    """float32 [B, 3, H, W] -> v' of include/stego_render.h as [B, H, W, 3]."""
    v = _unnormalised(img.float(), mean, std).permute(0, 2, 3, 1)
    if not rescale:
        return v.clamp(0, 1)
    lo = v.amin(dim=(1, 2, 3), keepdim=True)
    hi = v.amax(dim=(1, 2, 3), keepdim=True)
    return torch.where(hi > lo, (v - lo) / (hi - lo), torch.zeros_like(v))


def _levels(f):
    return (f * 255.0).clamp(0, 255).to(torch.uint8)


def _batched(t, dims, name):
    """A tensor of `dims` dimensions, or one with a leading batch axis -> (the batched tensor, whether the axis was added)."""
    if t.dim() == dims:
        return t.unsqueeze(0), True
    if t.dim() != dims + 1:
        raise ValueError("%s: expected %d or %d dimensions, got %s" % (name, dims, dims + 1, tuple(t.shape)))
    return t, False


def torch_image_u8(img, rescale=True, mean=PLOT_MEAN, std=PLOT_STD):
    """image_u8 as a torch chain, on the tensor's device."""
    img, single = _batched(img, 3, "img")
    out = _levels(_unit(img, rescale, mean, std))
    return out[0] if single else out


def torch_colorize(labels, cmap, mapping=None, image=None, alpha=0.5, edges=False, rescale=False, mean=IMAGENET_MEAN,
                   std=IMAGENET_STD, edge_color=EDGE_COLOR):
    """colorize as a torch chain, on the labels' device and for every integer dtype."""
    labels, single = _batched(labels, 2, "labels")
    dev = labels.device
    table, ignore = _table(cmap, mapping)
    n = table.shape[0]
    full = torch.from_numpy(np.concatenate([table, ignore[None, :]], 0)).to(dev)
    lab = labels.long()
    rgb = full[torch.where((lab >= 0) & (lab < n), lab, torch.full_like(lab, n))]
    if edges:
        edge = torch.zeros_like(lab, dtype=torch.bool)
        edge[:, :, :-1] |= lab[:, :, 1:] != lab[:, :, :-1]
        edge[:, :-1, :] |= lab[:, 1:, :] != lab[:, :-1, :]
        rgb[edge] = torch.tensor(edge_color, dtype=torch.uint8, device=dev)
    if image is not None:
        image, _ = _batched(image, 3, "image")
        alpha = float(alpha)
        rgb = _levels((1.0 - alpha) * _unit(image.to(dev), rescale, mean, std) + alpha * (rgb.float() / 255.0))
    return rgb[0] if single else rgb


def _native_target(out, B, H, W, dev):
    """Whether `out` (or a fresh tensor when None) can be the kernel's target: uint8 [B, H, W, 3] on the device with packed pixels."""
    if out is None:
        return True
    return out.is_cuda and out.device == dev and out.dtype == torch.uint8 and tuple(out.shape) == (B, H, W, 3) and \
        (W == 1 or out.stride(2) == 3) and out.stride(3) == 1


def _native_size(B, H, W):
    return 1 <= B <= capi.RENDER_MAX_B and 1 <= H <= capi.STITCH_MAX_SIDE and 1 <= W <= capi.STITCH_MAX_SIDE


def _finish(res, out, single):
    if out is not None:
        out.copy_(res.reshape(out.shape))
        return out
    return res[0] if single else res


def _check_out(out, shape):
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape)):
        raise ValueError("out: expected uint8 %s, got %s %s" % (tuple(shape), out.dtype, tuple(out.shape)))


def image_u8(img, rescale=True, mean=PLOT_MEAN, std=PLOT_STD, out=None):
    """``(prep_for_plot(img, rescale) * 255).astype(np.uint8)`` of a normalised float image [3, H, W] or [B, 3, H, W] (any strides) ->
    uint8 [H, W, 3] or [B, H, W, 3] on its device, or into the view `out` of that shape.  rescale: every image to its own range, the
    minimum and maximum found by stego_image_range; else clamped to [0, 1]."""
    img, single = _batched(img, 3, "img")
    B, _, H, W = img.shape
    _check_out(out, (H, W, 3) if single else (B, H, W, 3))
    view = None if out is None else (out.unsqueeze(0) if single else out)
    if not (img.is_cuda and img.dtype == torch.float32 and img.shape[1] == 3 and _native_size(B, H, W)
            and _native_target(view, B, H, W, img.device)):
        return _finish(torch_image_u8(img, rescale, mean, std), out, single)
    res = view if view is not None else torch.empty((B, H, W, 3), dtype=torch.uint8, device=img.device)
    flags = capi.RENDER_IMAGE | (capi.RENDER_RESCALE if rescale else 0)
    desc = capi.render_desc(B, H, W, flags=flags, mean=mean, std=std, out_strides=(res.stride(0), res.stride(1)))
    rng = capi.image_range(desc, img) if rescale else None
    capi.render(desc, img, None, None, rng, res)
    return out if out is not None else (res[0] if single else res)


def colorize(labels, cmap, mapping=None, image=None, alpha=0.5, edges=False, out=None, rescale=False, mean=IMAGENET_MEAN,
             std=IMAGENET_STD, edge_color=EDGE_COLOR):
    """``cmap[labels]`` as uint8: integer labels [H, W] or [B, H, W] (any strides) -> [H, W, 3] or [B, H, W, 3] on their device, or
    into the view `out` of that shape (a panel of a larger sheet: any image and row stride).  A label outside the table takes
    cmap[-1], which is where numpy's wrap-around puts the label -1.
    mapping: a cluster -> class vector (UnsupervisedMetrics.cluster_to_class()): cluster k takes cmap[mapping[k]], and cmap[-1]
    where the mapping is -1.  It is composed into the table on the host; the label map is read once.
    image: a normalised float image of the labels' size; the picture is then (1 - alpha) * image + alpha * colours, the image
    un-normalised with `mean` / `std` and clamped to [0, 1] (rescale: brought to its own range instead).
    edges: a pixel whose label differs from its right or lower neighbour takes `edge_color`."""
    labels, single = _batched(labels, 2, "labels")
    B, H, W = labels.shape
    _check_out(out, (H, W, 3) if single else (B, H, W, 3))
    view = None if out is None else (out.unsqueeze(0) if single else out)
    table, ignore = _table(cmap, mapping)
    img = None
    if image is not None:
        img, _ = _batched(image, 3, "image")
        if tuple(img.shape) != (B, 3, H, W):
            raise ValueError("image %s does not match labels %s" % (tuple(img.shape), tuple(labels.shape)))
    native = labels.is_cuda and labels.dtype in capi.RENDER_DTYPES and table.shape[0] <= capi.RENDER_MAX_LUT and _native_size(B, H, W) \
        and _native_target(view, B, H, W, labels.device) and \
        (img is None or (img.is_cuda and img.device == labels.device and img.dtype == torch.float32))
    if not native:
        return _finish(torch_colorize(labels, cmap, mapping, img, alpha, edges, rescale, mean, std, edge_color), out, single)
    dev = labels.device
    res = view if view is not None else torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    flags = capi.RENDER_LABELS | (capi.RENDER_EDGES if edges else 0)
    if img is not None:
        flags |= capi.RENDER_IMAGE | capi.RENDER_BLEND | (capi.RENDER_RESCALE if rescale else 0)
    desc = capi.render_desc(B, H, W, n_lut=table.shape[0], label_dtype=capi.RENDER_DTYPES[labels.dtype], flags=flags, alpha=alpha,
                            mean=mean, std=std, ignore_rgb=ignore, edge_rgb=edge_color, label_strides=labels.stride(),
                            out_strides=(res.stride(0), res.stride(1)))
    lut = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    rng = capi.image_range(desc, img) if (img is not None and rescale) else None
    capi.render(desc, img, labels, lut, rng, res)
    return out if out is not None else (res[0] if single else res)


def _panel_shape(spec):
    if "features" in spec:
        t = spec["features"]
        if t.dim() != 4:
            raise ValueError("features: expected [B, C, h, w], got %s" % (tuple(t.shape),))
        H, W = spec["size"] if spec.get("size") is not None else t.shape[-2:]
        return int(t.shape[0]), int(H), int(W), t.device
    t = spec["labels"] if "labels" in spec else spec["image"]
    dims = 2 if "labels" in spec else 3
    t, _ = _batched(t, dims, "panel")
    return int(t.shape[0]), int(t.shape[-2]), int(t.shape[-1]), t.device


def comparison_sheet(rows, pad=4, background=(255, 255, 255)):
    """One uint8 [SH, SW, 3] sheet of panels.  `rows` is a list of rows; a row is the keyword arguments of one call as a dict:
    ``{"image": img, "rescale": True}`` for image_u8, ``{"labels": l, "cmap": c, ...}`` for colorize, or ``{"features": maps, "size":
    (H, W), "joint": ..., "scale": ..., "resize": ...}`` for feature_pca.feature_pictures (a [B, C, h, w] map; size defaults to (h, w)).
    The tensors of a row are batched ([B, ...]; an unbatched image or label map is a row of one panel): its B panels stand side by side, `pad` pixels of `background` around
    and between them, the rows below one another.  The sheet is allocated once and every row renders straight into its place
    through the strided target: no per-panel tensor, no copy."""
    if not rows:
        raise ValueError("comparison_sheet: no rows")
    pad = int(pad)
    shapes = [_panel_shape(spec) for spec in rows]
    dev = shapes[0][3]
    SW = max(pad + B * (W + pad) for B, _, W, _ in shapes)
    SH = pad + sum(H + pad for _, H, _, _ in shapes)
    sheet = torch.empty((SH, SW, 3), dtype=torch.uint8, device=dev)
    sheet[:] = torch.tensor(background, dtype=torch.uint8, device=dev)
    y = pad
    for spec, (B, H, W, _) in zip(rows, shapes):
        view = torch.as_strided(sheet, (B, H, W, 3), ((W + pad) * 3, SW * 3, 3, 1), (y * SW + pad) * 3)
        spec = dict(spec)
        if "features" in spec:
            from .feature_pca import feature_pictures
            feature_pictures(spec.pop("features"), out=view, **spec)
        elif "labels" in spec:
            labels, _ = _batched(spec.pop("labels"), 2, "labels")
            colorize(labels, spec.pop("cmap"), out=view, **spec)
        else:
            img, _ = _batched(spec.pop("image"), 3, "image")
            image_u8(img, out=view, **spec)
        y += H + pad
    return sheet
