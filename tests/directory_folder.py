"""Image folders for the directory-dataset tests (tests/test_directory_host.py, tests/test_directory_gpu.py): written with PIL in the
layout data.DirectoryDataset reads, and the restatement of an item the tests compare against."""
import os
from os.path import join

import numpy as np
import torch
from PIL import Image

from stego_amd import data as D

HOST_SIZES = [(40, 52), (36, 30), (1, 9), (224, 300)]          # (h, w)


def write_folder(root, name, split, sizes, seed=0, labels=True, grey=1, rgba=2, fmt=None):
    """One split of a folder: image k has size sizes[k] = (h, w); file names sort differently from their creation order (k = 0 is
    written first and sorts last); image `grey` is a mode-L file and image `rgba` an RGBA PNG; PNG and JPEG alternate (or `fmt`);
    labels hold 0, 1, 255 and a few other values, as mode-L PNGs, every third one as a mode-P PNG.  Returns the sorted file stems."""
    rng = np.random.default_rng(seed)
    img_dir = join(str(root), name, "imgs", split)
    os.makedirs(img_dir, exist_ok=True)
    if labels:
        label_dir = join(str(root), name, "labels", split)
        os.makedirs(label_dir, exist_ok=True)
    stems = []
    n = len(sizes)
    for k, (h, w) in enumerate(sizes):
        stem = "im_%04d" % (n - 1 - k)
        stems.append(stem)
        arr = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        if k == grey:
            im = Image.fromarray(arr[..., 0], "L")
        elif k == rgba:
            im = Image.fromarray(arr, "RGBA")
        else:
            im = Image.fromarray(arr[..., :3], "RGB")
        ext = fmt or ("png" if (k % 2 == 0 or k == rgba) else "jpg")
        if ext == "jpg" and im.mode == "RGBA":
            ext = "png"
        im.save(join(img_dir, "%s.%s" % (stem, ext)))
        if labels:
            lab = rng.choice(np.array([0, 0, 1, 1, 2, 7, 255], dtype=np.uint8), size=(h, w))
            lim = Image.fromarray(lab, "L")
            if k % 3 == 2:
                lim = lim.convert("P")
                lim.putpalette([v for i in range(256) for v in (i, 255 - i, (7 * i) % 256)])
            lim.save(join(label_dir, "%s.png" % stem))
    return sorted(stems)


def files(root, name, split):
    """(sorted image paths, sorted label paths or None), listed independently of the code under test."""
    d = join(str(root), name)
    imgs = [join(d, "imgs", split, f) for f in sorted(os.listdir(join(d, "imgs", split)))]
    if not os.path.exists(join(d, "labels")):
        return imgs, None
    return imgs, [join(d, "labels", split, f) for f in sorted(os.listdir(join(d, "labels", split)))]


def open_pair(imgs, labs, i):
    with Image.open(imgs[i]) as im:
        rgb = im.convert("RGB")
    lab = None
    if labs is not None:
        with Image.open(labs[i]) as lb:
            lab = lb.copy()
    return rgb, lab


def restated_item(rgb, lab, R, origin=None):
    """(img float32 [3,R,R], label int64 [R,R], mask float32 [1,R,R]) of a directory item: PIL image -> image_transform /
    label_transform (or resize, then a crop at the explicit (top, left) origin), the label's stored value with no "- 1" (-1 everywhere
    without a label file), mask = label > 0."""
    if origin is None:
        img = D.image_transform(R)(rgb)
        label = D.label_transform(R)(lab)[0] if lab is not None else None
    else:
        top, left = origin
        box = (left, top, left + R, top + R)
        x = np.asarray(D._resize(rgb, R).crop(box), dtype=np.float32) / np.float32(255.0)
        img = torch.from_numpy(((x - D._MEAN) / D._STD).transpose(2, 0, 1).copy())
        label = torch.as_tensor(np.array(D._resize(lab, R).crop(box)), dtype=torch.int64) if lab is not None else None
    if label is None:
        label = torch.full((R, R), -1, dtype=torch.int64)
    return img, label, (label > 0).to(torch.float32).unsqueeze(0)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
