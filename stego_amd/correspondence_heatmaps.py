"""Query-point correspondence heatmaps: the reference's ``src/plot_dino_correspondence.py``, the paper's correspondence figure.

*Where do the frozen features place a point of this image, in the image itself and in its KNN positive?*  Per target map one call
(``capi.corr_heatmaps``, ``include/stego_heat.h``) samples the source map at the query points, correlates the normalised samples with
every normalised cell of the target, centres each query's map, clamps it and upsamples it to the image's size; the full-resolution
heatmaps are the only large tensor that is written.  It is the qualitative partner of ``stego_amd.correspondence_pr``.

    python -m stego_amd.correspondence_heatmaps image=a.jpg image_pos=b.jpg pretrained_weights=dino.pth result_dir=out

Deviations from the reference: no mp4 is written (ffmpeg is not assumed), the frames of the movie are written as PNG files instead;
the batch is a real dimension of ``correspondence_heatmaps`` (the reference's ``get_heatmaps`` breaks for B > 1, the one here refuses
it by name); the figures are drawn with PIL and numpy, not matplotlib; the image is item ``image_num`` of the train split, not item
``image_num`` of a shuffled first batch; the raw ``crop_type: None`` dataset reader is not part of this build (the cropped tree, two
image files or synthetic data are).
"""
import os
import sys
from os.path import dirname, exists, join

import numpy as np
import torch

from . import capi

PLOT_CONFIG = join(dirname(__file__), "configs", "plot_config.yml")
MAPS = ("feats", "code")
COLOURS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0))                     # plot_dino_correspondence.py:108
KEY_POINTS = ((-.7, -.7), (-.1, 0.0), (.5, .8))                             # :158-162
GREY = (0.2989, 0.5870, 0.1140)                                             # plot_heatmap, :22
RAMP = 255                                                                  # ListedColormap([(r, g, b, i / 255) for i in range(255)])


def correspondence_heatmaps(src, tgt, points, size, center=True, clamp=True, index_t=None, want_best=False):
    """Heatmaps of `points` [B, N, 2] or [B, N, 1, 2] ((x, y) in [-1, 1]) of the maps `src` [B, C, hs, ws] in the maps `tgt`
    [B, C, h, w] (image index_t[i] of `tgt` for image i, i itself without index_t) -> float32 [B, N, H, W] on the device for
    size = (H, W).  center=False keeps each map's mean, clamp=False its negative part (both False: the raw cosines).  With
    want_best also `peak` [B, N], the maximum of each low-resolution map, and `best` [B, N, 2], the (x, y) of its cell: the point
    correspondence itself.  CPU tensors raise."""
    return capi.corr_heatmaps(src, tgt, points, size, center=center, clamp=clamp, index_t=index_t, want_best=want_best)


def get_heatmaps(net, img, img_pos, query_points, which="feats"):
    """plot_dino_correspondence.py:39-58 for one image: `query_points` [1, N, 1, 2] -> (heatmap_intra, heatmap_inter), each [N, H, W]
    on the CPU, at the size of `img` / `img_pos`.  `which` picks the backbone features or the head's code."""
    if img.shape[0] != 1 or img_pos.shape[0] != 1:
        raise ValueError("get_heatmaps takes one image (the reference's squeeze(0)), got a batch of %d: use correspondence_heatmaps, "
                         "whose batch is a real dimension" % img.shape[0])
    dev = torch.device("cuda", torch.cuda.current_device())
    with torch.no_grad():
        m1 = dict(zip(MAPS, net(img.to(dev))))[which].float()
        m2 = dict(zip(MAPS, net(img_pos.to(dev))))[which].float()
        q = query_points.to(dev)
        intra = correspondence_heatmaps(m1, m1, q, img.shape[2:])
        inter = correspondence_heatmaps(m1, m2, q, img_pos.shape[2:])
    return intra[0].cpu(), inter[0].cpu()


def movie_points(n_hold=60, n_move=50):
    """The key-point path of the reference's movie (:158-173): every key point held for 60 frames, 50 frames between two."""
    pts = []
    for i, k in enumerate(KEY_POINTS):
        pts.extend([list(k)] * n_hold)
        if i < len(KEY_POINTS) - 1:
            nxt = KEY_POINTS[i + 1]
            pts.extend(np.stack([np.linspace(k[0], nxt[0], n_move), np.linspace(k[1], nxt[1], n_move)], axis=1).tolist())
    return pts


def prep_for_plot(img):
    """A normalised image tensor [3, H, W] -> uint8 [H, W, 3] (the reference's unnorm + clamp + permute)."""
    from .data import _MEAN, _STD
    x = img.detach().cpu().float().numpy().transpose(1, 2, 0) * _STD + _MEAN
    return np.floor(np.clip(x, 0.0, 1.0).astype(np.float64) * 255.0 + 0.5).astype(np.uint8)


def grey_background(image_u8):
    """plot_heatmap's background: the image turned grey, times 0.8 -> float64 [H, W, 3] in [0, 0.8]."""
    rgb = np.asarray(image_u8)[..., :3].astype(np.float64) / 255.0
    return np.repeat((rgb @ np.array(GREY) * 0.8)[..., None], 3, axis=2)


def composite(background, heat, colour, vmax=None):
    """One imshow(heat, alpha=.5, cmap=ramp of `colour`) over `background` (float64 [H, W, 3]): a pixel's opacity is
    0.5 * i / 255 with i = min(floor(heat / vmax * 255), 254), the 255-step ramp over [0, vmax]."""
    heat = np.asarray(heat, dtype=np.float64)
    if heat.shape != background.shape[:2]:
        raise ValueError("heatmap %s does not match the image %s" % (heat.shape, background.shape[:2]))
    vmax = float(heat.max()) if vmax is None else float(vmax)
    t = np.clip(heat / vmax, 0.0, 1.0) if vmax > 0 else np.zeros_like(heat)
    a = (0.5 * np.minimum(np.floor(t * RAMP), RAMP - 1) / 255.0)[..., None]
    return background * (1.0 - a) + np.asarray(colour, dtype=np.float64) * a


def to_u8(x):
    return np.floor(np.clip(x, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def render_overlay(image_u8, heat, colour, vmax=None):
    """plot_heatmap(ax, image * .8, heat, cmap=ramp of `colour`, symmetric=False) as pixels: uint8 [H, W, 3].  `vmax` defaults to the
    map's own maximum (matplotlib's autoscale; the lower end is 0, what a clamped map has)."""
    return to_u8(composite(grey_background(image_u8), heat, colour, vmax))


def mark_points(image_u8, points_xy, colours, arm=None, width=None):
    """The image with an x at every (x, y) in [-1, 1] (the reference's scatter(marker="x"))."""
    from PIL import Image, ImageDraw
    im = Image.fromarray(np.ascontiguousarray(image_u8))
    H, W = image_u8.shape[:2]
    arm = arm or max(2, W // 40)
    width = width or max(1, W // 128)
    draw = ImageDraw.Draw(im)
    for (x, y), c in zip(points_xy, colours):
        px, py = (x + 1) / 2 * W, (y + 1) / 2 * H                           # the reference's (q + 1) / 2 * high_res
        fill = tuple(int(255 * v) for v in c)
        draw.line([(px - arm, py - arm), (px + arm, py + arm)], fill=fill, width=width)
        draw.line([(px - arm, py + arm), (px + arm, py - arm)], fill=fill, width=width)
    return np.asarray(im)


def figure(image_u8, image_pos_u8, points_xy, heat_intra, heat_inter, colours):
    """Three panels side by side: the image with its points, self correspondence, KNN correspondence -> uint8 [H, 3 W + 2 gaps, 3]."""
    left = mark_points(image_u8, points_xy, colours)
    panels = [left]
    for img, heats in ((image_u8, heat_intra), (image_pos_u8, heat_inter)):
        acc = grey_background(img)
        for hm, c in zip(heats, colours):
            acc = composite(acc, np.asarray(hm), c)
        panels.append(to_u8(acc))
    H = max(p.shape[0] for p in panels)
    gap = np.zeros((H, 8, 3), dtype=np.uint8)                                # dark background, as plt.style.use('dark_background')
    padded = [np.pad(p, ((0, H - p.shape[0]), (0, 0), (0, 0))) for p in panels]
    return np.concatenate([padded[0], gap, padded[1], gap, padded[2]], axis=1)


def result_dir(cfg):
    return getattr(cfg, "result_dir", None) or join(cfg.output_root, "results", "correspondence")


def load_pair(cfg):
    """(img, img_pos), each [1, 3, high_res, high_res], from the first source that applies: the files cfg.image / cfg.image_pos, item
    cfg.image_num of the cropped tree's train split with its KNN positive, synthetic data."""
    from .data import ContrastiveSegDataset, crop_dir, image_transform, label_transform
    res = int(cfg.high_res)
    image, image_pos = getattr(cfg, "image", None), getattr(cfg, "image_pos", None)
    if image or image_pos:
        if not (image and image_pos):
            raise ValueError("give both image and image_pos, or neither")
        from PIL import Image
        tf = image_transform(res, "center")
        out = []
        for path in (image, image_pos):
            with Image.open(path) as im:
                out.append(tf(im.convert("RGB")).unsqueeze(0))
        return out[0], out[1]
    root, crop_type = getattr(cfg, "pytorch_data_dir", None), getattr(cfg, "crop_type", None)
    if root and crop_type and exists(join(crop_dir(root, cfg.dataset_name, crop_type, cfg.crop_ratio), "img", "train")):
        nn_file = join(root, "nns", "nns_{}_{}_{}_{}_{}.npz".format(cfg.model_type, cfg.dataset_name, "train", crop_type, cfg.res))
        if exists(nn_file):
            ds = ContrastiveSegDataset(root, cfg.dataset_name, crop_type, "train", image_transform(res, "center"), label_transform(res, "center"),
                                       cfg, num_neighbors=2, mask=True, pos_images=True, pos_labels=True)
            item = ds[int(cfg.image_num) % len(ds)]
            return item["img"].unsqueeze(0), item["img_pos"].unsqueeze(0)
        print("no KNN file %r (run precompute_knns): synthetic data" % nn_file)
    else:
        print("no image / image_pos and no cropped train split under %r: synthetic data" % root)
    from .train_segmentation import SyntheticContrastiveDataset
    item = SyntheticContrastiveDataset(int(cfg.image_num) + 1, res, 27, seed=0)[int(cfg.image_num)]
    return item["img"].unsqueeze(0), item["img_pos"].unsqueeze(0)


def my_app(cfg):
    """plot_dino_correspondence.py:61-214: cfg.plot_correspondence writes {result_dir}/correspondence.png, cfg.plot_movie the frames
    {result_dir}/attention_interp/frame_%04d.png (all 280, or the first cfg.movie_frames).  Returns the written paths."""
    from PIL import Image
    from .featurizers import DinoFeaturizer
    if cfg.arch != "dino":
        raise ValueError("Unknown arch {} (this build has the dino featurizer only)".format(cfg.arch))
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)                                                     # seed_everything(seed=0)
    net = DinoFeaturizer(cfg.dim, cfg).to(dev).eval()
    img, img_pos = load_pair(cfg)
    image_u8, image_pos_u8 = prep_for_plot(img[0]), prep_for_plot(img_pos[0])
    out = result_dir(cfg)
    os.makedirs(out, exist_ok=True)
    which = getattr(cfg, "map", "feats")
    written = []
    if cfg.plot_correspondence:
        pts = [list(map(float, p)) for p in cfg.query_points]
        if not 1 <= len(pts) <= len(COLOURS):
            raise ValueError("query_points: 1 .. %d points (one colour each), got %d" % (len(COLOURS), len(pts)))
        q = torch.tensor(pts, dtype=torch.float32).reshape(1, len(pts), 1, 2)
        intra, inter = get_heatmaps(net, img, img_pos, q, which)
        path = join(out, "correspondence.png")
        Image.fromarray(figure(image_u8, image_pos_u8, pts, intra.numpy(), inter.numpy(), COLOURS[:len(pts)])).save(path)
        written.append(path)
    if cfg.plot_movie:
        pts = movie_points()
        n_frames = getattr(cfg, "movie_frames", None)
        if n_frames is not None:
            pts = pts[:int(n_frames)]
        q = torch.tensor(pts, dtype=torch.float32).reshape(1, len(pts), 1, 2)
        intra, inter = get_heatmaps(net, img, img_pos, q, which)
        os.makedirs(join(out, "attention_interp"), exist_ok=True)
        for i, p in enumerate(pts):
            path = join(out, "attention_interp", "frame_%04d.png" % i)
            Image.fromarray(figure(image_u8, image_pos_u8, [p], intra[i:i + 1].numpy(), inter[i:i + 1].numpy(), COLOURS[:1])).save(path)
            written.append(path)
    return written


if __name__ == "__main__":
    from .train_segmentation import load_config
    my_app(load_config(PLOT_CONFIG, overrides=sys.argv[1:]))
