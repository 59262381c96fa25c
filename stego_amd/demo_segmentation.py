"""The reference's demo (``src/demo_segmentation.py``): a checkpoint run over a folder of the user's own images, one label map per
image and probe written as a PNG.

    python -m stego_amd.demo_segmentation model_path=run.ckpt image_dir=my_images experiment_name=mine

Each batch goes through stego_amd.segment.segment: the backbone on the images and their mirror images, the fused probe head
(csrc/probe_head.hip) and the dense CRF on the device.  Deviations from the reference: a prediction is named after the file's stem
(os.path.splitext, the reference's name for every file with an extension), files PIL cannot open are skipped and named instead of
ending the run, the files are read in sorted order, and DataParallel (`use_ddp`) is not supported.

With `full_res=True` no file is cropped or shrunk: each goes through stego_amd.segment.segment_large at its own size, as overlapping
res x res windows `window_stride` apart (default: half a window) stitched on the device (csrc/stitch_probe.hip), and its PNGs have the
image's size.  A file whose shorter side is below `res` is first resized so that it equals `res`.

With `save_color=True` every prediction is also written as a picture (stego_amd.render, csrc/render.hip), coloured on the device
before it is copied to the host: `linear_color/` and `cluster_color/` are the label maps through the model's `label_cmap`, and
`overlay/` is the image, at weight 1 - `overlay_alpha`, under the cluster colours with the segment boundaries drawn.  The clusters
are coloured by class through the checkpoint's cluster -> class assignment when it stores one (`model.cluster_to_class`), else by
their own index.  `linear/` and `cluster/` and the returned list are the same with and without it.

With `save_pca=True` every image also gets the two three-principal-component pictures of stego_amd.feature_pca (csrc/feature_pca.hip),
at the size of its label maps: `pca_feats/` shows the backbone features, every component brought to its own range, and `pca_code/`
the segmentation code, L2-normalised per token, as (p + 1) / 2 - the picture of the reference's src/train_crf.py:145-150.  One model
is fitted per batch, so the images of a batch share their colours.  Under `full_res` an image is a set of overlapping windows, each
with a low-resolution map of its own, and there is no single map per image short of running the backbone again: `save_pca` writes
nothing there.

With `save_salience=True` every image also gets its attention salience mask (stego_amd.salience: the strongest patches holding
`salience_keep` of the class token's attention in the backbone's last block) as `salience/NAME.png` (0 / 255) and, beside the image,
as `salience_sheet/NAME.png`.  It costs one more backbone pass per batch and, like `save_pca`, writes nothing under `full_res`.

With `min_region_area` > 0 both probes' label maps are cleaned on the device before anything is written (stego_amd.regions,
csrc/regions.hip): a connected region - `region_connectivity` 4 or 8 - with fewer pixels takes the label most of its neighbours
have.  `linear/`, `cluster/`, the colour pictures and the regions then all show the cleaned maps.  With `save_regions=True` every
image also gets `regions/NAME.json`, the table of the connected regions of its cluster map (id, label, class - through
`model.cluster_to_class` when the checkpoint stores one -, area, box, centroid, first pixel), and the id map itself as
`region_ids/NAME.png`, a 16-bit PNG (mode "I;16"), or as `region_ids/NAME.npy` (int32) from 65536 regions on; the JSON names the
file ("id_map").  Both work under `full_res`: the canvas is a larger label map.  The returned list is the same with and without them.
With `save_region_index=True` as well, the `code` the backbone returned (`region_descriptor: "feats"` for its features), its tokens
L2-normalised, is pooled over every region on the device (stego_amd.region_descriptors, csrc/region_pool.hip) and the folder's
`regions/index.npz` is written for `python -m stego_amd.find_objects`.  Under `full_res` no index is written, and the run says so.
"""
import os
import sys
from os.path import dirname, exists, isdir, join

import numpy as np
import torch
from PIL import Image

from .data import full_image_transform, image_transform
from .segment import segment, segment_large
from .train_segmentation import LitUnsupervisedSegmenter, load_config

DEMO_CONFIG = join(dirname(__file__), "configs", "demo_config.yml")


class UnlabeledImageFolder(torch.utils.data.Dataset):
    """The files of `root` in sorted order; an item is (image tensor, file name), or (None, file name) for a file PIL cannot read."""

    def __init__(self, root, transform):
        super().__init__()
        self.root = root
        self.transform = transform
        self.images = sorted(f for f in os.listdir(root) if not isdir(join(root, f)))

    def __getitem__(self, index):
        name = self.images[index]
        try:
            with Image.open(join(self.root, name)) as im:
                image = im.convert("RGB")
        except (OSError, ValueError, Image.DecompressionBombError):
            return None, name
        return self.transform(image), name

    def __len__(self):
        return len(self.images)


def collate(items):
    """-> (images [N, 3, res, res] or None, their names, the names of the unreadable files of the batch)."""
    good = [(img, name) for img, name in items if img is not None]
    bad = [name for img, name in items if img is None]
    imgs = torch.stack([img for img, _ in good]) if good else None
    return imgs, [name for _, name in good], bad


def first(items):
    """collate_fn of the full-resolution run: one file per batch, nothing stacked."""
    return items[0]


def result_dir(cfg):
    return join(cfg.output_root, "results", "predictions", cfg.experiment_name)


def prediction_name(name):
    """`photo.v2.jpg` -> `photo.v2.png` (the reference's ".".join(name.split(".")[:-1]) + ".png" for a name with an extension)."""
    return os.path.splitext(name)[0] + ".png"


def my_app(cfg):
    """demo_segmentation.py:34-78: every readable image of cfg.image_dir -> {result_dir}/{linear,cluster}/{stem}.png (uint8 labels,
    PIL mode "L").  Returns the written paths, linear and cluster interleaved in file order."""
    if getattr(cfg, "use_ddp", False):
        raise NotImplementedError("use_ddp: DataParallel is not supported by stego_amd.demo_segmentation (one device)")
    if not exists(cfg.model_path):
        raise FileNotFoundError("model_path %r does not exist" % cfg.model_path)
    if not isdir(cfg.image_dir):
        raise FileNotFoundError("image_dir %r is not a directory" % cfg.image_dir)
    out = result_dir(cfg)
    for sub in ("linear", "cluster"):
        os.makedirs(join(out, sub), exist_ok=True)

    dev = torch.device("cuda", 0)
    model = LitUnsupervisedSegmenter.load_from_checkpoint(cfg.model_path)
    model.eval().to(dev)
    run_crf = getattr(cfg, "run_crf", True)
    written, skipped = [], []

    def save(name, linear, cluster):
        for sub, pred in (("linear", linear), ("cluster", cluster)):
            path = join(out, sub, prediction_name(name))
            Image.fromarray(pred.astype(np.uint8)).save(path)          # 2-D uint8: mode "L"
            written.append(path)

    save_color = getattr(cfg, "save_color", False)
    if save_color:
        from .render import IMAGENET_MEAN, IMAGENET_STD, colorize
        for sub in ("linear_color", "cluster_color", "overlay"):
            os.makedirs(join(out, sub), exist_ok=True)
        cmap, mapping = model.label_cmap, model.cluster_to_class
        overlay_alpha = float(getattr(cfg, "overlay_alpha", 0.5))

    def save_colors(names, imgs, linear, cluster):
        """The three pictures of every image of a batch on the device: imgs [N, 3, H, W], label maps [N, H, W]."""
        pictures = (("linear_color", colorize(linear, cmap)),
                    ("cluster_color", colorize(cluster, cmap, mapping=mapping)),
                    ("overlay", colorize(cluster, cmap, mapping=mapping, image=imgs, alpha=overlay_alpha, edges=True,
                                         mean=IMAGENET_MEAN, std=IMAGENET_STD)))
        for sub, rgb in pictures:
            rgb = rgb.cpu().numpy()
            for j, name in enumerate(names):
                Image.fromarray(rgb[j]).save(join(out, sub, prediction_name(name)))         # [H, W, 3] uint8: mode "RGB"

    save_pca = getattr(cfg, "save_pca", False) and not getattr(cfg, "full_res", False)
    if save_pca:
        from .feature_pca import feature_pictures
        for sub in ("pca_feats", "pca_code"):
            os.makedirs(join(out, sub), exist_ok=True)

    def save_pcas(names, maps, size):
        """Both feature pictures of every image of a batch: one joint fit per map, painted at the label maps' size."""
        code = torch.nn.functional.normalize(maps["code"].detach().float(), dim=1)
        pictures = (("pca_feats", feature_pictures(maps["feats"].detach().float(), size=size, joint=True, scale="range")),
                    ("pca_code", feature_pictures(code, size=size, joint=True, scale="unit")))
        for sub, rgb in pictures:
            rgb = rgb.cpu().numpy()
            for j, name in enumerate(names):
                Image.fromarray(rgb[j]).save(join(out, sub, prediction_name(name)))

    save_salience = getattr(cfg, "save_salience", False) and not getattr(cfg, "full_res", False)
    if save_salience:
        from .render import IMAGENET_MEAN, IMAGENET_STD, colorize, image_u8
        from .salience import image_salience
        for sub in ("salience", "salience_sheet"):
            os.makedirs(join(out, sub), exist_ok=True)
        salience_keep = float(getattr(cfg, "salience_keep", 0.6))

    def save_saliences(names, imgs):
        """The attention salience mask of every image of a batch (stego_amd.salience) as a 0 / 255 PNG, and the image beside it."""
        mask = image_salience(model.net, imgs, keep=salience_keep)[1]
        N, H, W = mask.shape
        pad = 4
        sheet = torch.full((N, H, 2 * W + pad, 3), 255, dtype=torch.uint8, device=mask.device)
        image_u8(imgs, rescale=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, out=sheet[:, :, :W])
        colorize(mask, np.array([[0, 0, 0], [255, 255, 255]], dtype=np.uint8), out=sheet[:, :, W + pad:])
        mask, sheet = (mask * 255).cpu().numpy(), sheet.cpu().numpy()
        for j, name in enumerate(names):
            Image.fromarray(mask[j]).save(join(out, "salience", prediction_name(name)))
            Image.fromarray(sheet[j]).save(join(out, "salience_sheet", prediction_name(name)))

    min_area = int(getattr(cfg, "min_region_area", 0))
    connectivity = int(getattr(cfg, "region_connectivity", 4))
    save_regions = getattr(cfg, "save_regions", False)
    if save_regions:
        from .regions import label_regions, region_table, write_id_map, write_regions
        for sub in ("regions", "region_ids"):
            os.makedirs(join(out, sub), exist_ok=True)

    region_index = None
    if save_regions and getattr(cfg, "save_region_index", False):
        if getattr(cfg, "full_res", False):
            print("save_region_index: no index under full_res (an image is a set of windows there, each with a map of its own)")
        else:
            from .region_descriptors import RegionIndex, region_descriptors
            region_index = RegionIndex(getattr(cfg, "region_descriptor", "code"))

    def save_region_files(names, cluster, maps=None):
        """The region table and the id map of every image of a batch: cluster [N, H, W] on the device.  With the backbone's `maps`
        the regions' descriptors go into the folder's index."""
        cluster = cluster.contiguous()
        ids, counts = label_regions(cluster, connectivity)
        table = region_table(cluster, ids, counts)
        if region_index is not None:
            pooled = region_descriptors(ids, table, maps[region_index.pooled].detach().float(), normalize=True)
            for j, name in enumerate(names):
                region_index.add(name, table, j, pooled[table.rows(j)])
        ids = ids.cpu().numpy()
        for j, name in enumerate(names):
            stem = os.path.splitext(name)[0]
            id_map = write_id_map(join(out, "region_ids", stem), ids[j], table.n_regions[j])
            write_regions(join(out, "regions", stem + ".json"), table, j, cluster.shape[1], cluster.shape[2], connectivity,
                          class_of=model.cluster_to_class, id_map=os.path.basename(id_map))

    if getattr(cfg, "full_res", False):
        dataset = UnlabeledImageFolder(cfg.image_dir, full_image_transform(cfg.res))
        loader = torch.utils.data.DataLoader(dataset, 1, shuffle=False, num_workers=cfg.num_workers, collate_fn=first)
        for img, name in loader:
            if img is None:
                skipped.append(name)
                continue
            img = img.to(dev)
            linear, cluster = segment_large(model, img, window=cfg.res, stride=getattr(cfg, "window_stride", None),
                                            batch=cfg.batch_size * 2, run_crf=run_crf, min_region_area=min_area,
                                            connectivity=connectivity)
            if save_regions:
                save_region_files([name], cluster.unsqueeze(0))
            if save_color:
                save_colors([name], img.unsqueeze(0), linear.unsqueeze(0), cluster.unsqueeze(0))
            save(name, linear.cpu().numpy(), cluster.cpu().numpy())
        if skipped:
            print("skipped %d file(s) PIL cannot read: %s" % (len(skipped), ", ".join(skipped)))
        return written

    dataset = UnlabeledImageFolder(cfg.image_dir, image_transform(cfg.res, "center"))
    loader = torch.utils.data.DataLoader(dataset, cfg.batch_size * 2, shuffle=False, num_workers=cfg.num_workers, collate_fn=collate)
    for imgs, names, bad in loader:
        skipped.extend(bad)
        if imgs is None:
            continue
        imgs = imgs.to(dev)
        maps = {} if save_pca or region_index is not None else None
        linear, cluster = segment(model, imgs, run_crf=run_crf, maps=maps, min_region_area=min_area, connectivity=connectivity)
        if save_regions:
            save_region_files(names, cluster, maps)
        if save_color:
            save_colors(names, imgs, linear, cluster)
        if save_pca:
            save_pcas(names, maps, tuple(linear.shape[-2:]))
        if save_salience:
            save_saliences(names, imgs)
        linear, cluster = linear.cpu().numpy(), cluster.cpu().numpy()
        for j, name in enumerate(names):
            save(name, linear[j], cluster[j])
    if region_index is not None:
        region_index.save(join(out, "regions", "index.npz"))
    if skipped:
        print("skipped %d file(s) PIL cannot read: %s" % (len(skipped), ", ".join(skipped)))
    return written


if __name__ == "__main__":
    my_app(load_config(DEMO_CONFIG, overrides=sys.argv[1:]))
