"""The cropped-dataset tree of the reference, reader and writer:

    {root}/cropped/{dataset}_{five|random}_crop_{ratio}/img/{split}/{i}.jpg
                                                       /label/{split}/{i}.png

written by `src/crop_datasets.py:76-123` (five crops per source image: image i * 5 + crop number; labels stored + 1 as uint8 PNG so
that "unlabelled" -1 becomes 0) and read by `CroppedDataset` `src/data.py:370-400` (target - 1, mask = target == -1).
torchvision is not part of this image: crops and tensor conversion are done with PIL / numpy / torch directly.

And the reader of a user's own image folder, the reference's DirectoryDataset (dataset_name "directory"):

    {root}/{dir_dataset_name}/imgs/{split}/*        and, optionally,        {root}/{dir_dataset_name}/labels/{split}/*"""
import os
import random
from os.path import join

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset


def crop_dir(root, dataset_name, crop_type, crop_ratio):
    return join(root, "cropped", "{}_{}_crop_{}".format(dataset_name, crop_type, crop_ratio))


def five_crop_boxes(height, width, crop_h, crop_w):
    """(top, left) of the four corners and the centre crop, torchvision.transforms.functional.five_crop's order (tl, tr, bl, br,
    centre; centre = round((size - crop) / 2))."""
    if crop_w > width or crop_h > height:
        raise ValueError("Requested crop size {} is bigger than input size {}".format((crop_h, crop_w), (height, width)))
    ct, cl = int(round((height - crop_h) / 2.0)), int(round((width - crop_w) / 2.0))
    return [(0, 0), (0, width - crop_w), (height - crop_h, 0), (height - crop_h, width - crop_w), (ct, cl)]


def random_crop_boxes(height, width, crop_h, crop_w, seed, n=5):
    """crop_datasets.py:14-57: box i of image `seed` from hash((seed, i, 0)) / hash((seed, i, 1))."""
    if crop_w > width or crop_h > height:
        raise ValueError("Requested crop size {} is bigger than input size {}".format((crop_h, crop_w), (height, width)))
    return [(hash((seed, i, 0)) % (height - crop_h), hash((seed, i, 1)) % (width - crop_w)) for i in range(n)]


def write_cropped(root, dataset_name, crop_type, crop_ratio, split, items):
    """items: iterable of (img float [3,H,W] in [0,1], label int [H,W] with -1 = unlabelled).  Writes five crops per item exactly
    as RandomCropComputer.__getitem__ does (crop_datasets.py:112-123).  Returns the number of files per directory."""
    if crop_type not in ("five", "random"):
        raise ValueError('Unknown crop type {}'.format(crop_type))
    save = crop_dir(root, dataset_name, crop_type, crop_ratio)
    img_dir, label_dir = join(save, "img", split), join(save, "label", split)
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(label_dir, exist_ok=True)
    n = 0
    for item, (img, label) in enumerate(items):
        H, W = img.shape[1], img.shape[2]
        ch, cw = int(H * crop_ratio), int(W * crop_ratio)                        # _get_size, crop_datasets.py:62-68
        boxes = five_crop_boxes(H, W, ch, cw) if crop_type == "five" else random_crop_boxes(H, W, ch, cw, item)
        for crop_num, (t, l) in enumerate(boxes):
            img_num = item * 5 + crop_num
            im = img[:, t:t + ch, l:l + cw]
            lb = label[t:t + ch, l:l + cw]
            img_arr = im.mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
            label_arr = (lb + 1).to("cpu", torch.uint8).numpy()
            Image.fromarray(img_arr).save(join(img_dir, "{}.jpg".format(img_num)), "JPEG")
            Image.fromarray(label_arr).save(join(label_dir, "{}.png".format(img_num)), "PNG")
            n += 1
    return n


_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def resized_size(w, h, res):
    """(nw, nh) after torchvision Resize(res, NEAREST): the short side becomes res, the long side int(res * long / short) (truncated);
    an image whose short side already is res keeps its size."""
    short, long = min(w, h), max(w, h)
    if short == res:
        return w, h
    new_long = int(res * long / short)
    return (res, new_long) if w <= h else (new_long, res)


def _resize(im, res):
    nw, nh = resized_size(im.size[0], im.size[1], res)
    return im if (nw, nh) == im.size else im.resize((nw, nh), Image.NEAREST)


def _resize_center_crop(im, res):
    """The reference's get_transform(res, _, "center") on a PIL image (src/utils.py:164-183): torchvision Resize(res, Image.NEAREST)
    for images and labels alike - the short side becomes res, the long side int(res * long / short) (truncated), and an image
    whose short side already is res is left as it is - then CenterCrop(res) (offsets int(round((size - res) / 2)))."""
    im = _resize(im, res)
    w, h = im.size
    left, top = int(round((w - res) / 2.0)), int(round((h - res) / 2.0))
    return im.crop((left, top, left + res, top + res))


def random_crop_origin(h, w, res):
    """torchvision RandomCrop.get_params on an h x w image: (0, 0) without a draw when it is res x res already, else
    top = torch.randint(0, h - res + 1), left = torch.randint(0, w - res + 1) from torch's global generator."""
    if h < res or w < res:
        raise ValueError("Required crop size {} is larger than input image size {}".format((res, res), (h, w)))
    if h == res and w == res:
        return 0, 0
    top = torch.randint(0, h - res + 1, size=(1,)).item()
    left = torch.randint(0, w - res + 1, size=(1,)).item()
    return top, left


def _resize_random_crop(im, res):
    """get_transform(res, _, "random"): Resize(res, NEAREST), then RandomCrop(res)."""
    im = _resize(im, res)
    top, left = random_crop_origin(im.size[1], im.size[0], res)
    return im.crop((left, top, left + res, top + res))


def _cropper(crop):
    if crop == "center":
        return _resize_center_crop
    if crop == "random":
        return _resize_random_crop
    raise ValueError("Unknown Cropper {}".format(crop))


def image_transform(res, crop="center"):
    """get_transform(res, False, crop): resize + crop, ToTensor (x / 255), Normalize(ImageNet mean, std)."""
    rc = _cropper(crop)

    def f(im):
        x = np.asarray(rc(im, res), dtype=np.float32) / np.float32(255.0)
        return torch.from_numpy(((x - _MEAN) / _STD).transpose(2, 0, 1).copy())
    return f


def full_image_transform(res):
    """The image at its own size for sliding-window segmentation (stego_amd.segment.segment_large): no crop, and no resize unless the
    shorter side is below `res` (then Resize(res, NEAREST) as in image_transform, so that one window fits); ToTensor, Normalize."""
    def f(im):
        if min(im.size) < res:
            im = _resize(im, res)
        x = np.asarray(im, dtype=np.float32) / np.float32(255.0)
        return torch.from_numpy(((x - _MEAN) / _STD).transpose(2, 0, 1).copy())
    return f


def label_transform(res, crop="center"):
    """get_transform(res, True, crop): resize + crop, ToTargetTensor (int64 [1, res, res])."""
    rc = _cropper(crop)

    def f(im):
        return torch.as_tensor(np.array(rc(im, res)), dtype=torch.int64).unsqueeze(0)
    return f


def to_tensor(pil_img):
    """PIL RGB -> float [3,H,W] in [0,1] (torchvision's ToTensor)."""
    return torch.from_numpy(np.asarray(pil_img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255)


def to_target_tensor(pil_label):
    """data.py ToTargetTensor: PIL label -> int64 [1,H,W]."""
    return torch.as_tensor(np.array(pil_label), dtype=torch.int64).unsqueeze(0)


def _seeded(fn, x, seed):
    """fn(x) with python's and torch's global generators reset to `seed` first: a random transform draws the same crop / flip for an image
    and for its label when both calls get the same seed (what reference src/data.py:388-394 does inline)."""
    random.seed(seed)
    torch.manual_seed(seed)
    return fn(x)


class CroppedDataset(Dataset):
    """Reader of the pre-cropped tree `cropped/{dataset}_{crop_type}_crop_{ratio}/{img,label}/{split}/{i}.{jpg,png}` that the reference's
    crop_datasets.py writes (format pinned by tests/golden/cropped_ref), with the reference dataset's constructor and item contract
    (src/data.py:370-400): item i -> (image, target [H, W] int64 with -1 = unlabelled, mask = target == -1); image and label go through
    their transforms under ONE random seed per item, drawn from numpy's global generator as the reference does (so that a run seeded
    like the reference sees the same augmentations)."""

    def __init__(self, root, dataset_name, crop_type, crop_ratio, image_set, transform=to_tensor, target_transform=to_target_tensor):
        super().__init__()
        self.dataset_name, self.split = dataset_name, image_set
        self.transform, self.target_transform = transform, target_transform
        self.root = crop_dir(root, dataset_name, crop_type, crop_ratio)
        self.img_dir, self.label_dir = (join(self.root, kind, image_set) for kind in ("img", "label"))
        self.num_images = len(os.listdir(self.img_dir))
        if self.num_images != len(os.listdir(self.label_dir)):
            raise AssertionError("%s: %d images but %d labels" % (self.root, self.num_images, len(os.listdir(self.label_dir))))

    def __len__(self):
        return self.num_images

    def __getitem__(self, index):
        seed = int(np.random.randint(2147483647))
        with Image.open(join(self.img_dir, "%d.jpg" % index)) as im:
            image = _seeded(self.transform, im.convert("RGB"), seed)
        with Image.open(join(self.label_dir, "%d.png" % index)) as lab:
            target = _seeded(self.target_transform, lab, seed) - 1      # the tree stores label + 1: 0 on disk = unlabelled
        return image, target.squeeze(0), target == -1


LABEL_MODES = ("L", "P")            # 8-bit single-channel label files: the stored byte (or palette index) is the label


def open_label(path):
    """The label file `path` as a loaded PIL image of mode L or P; anything else (16-bit, RGB, bilevel ...) is a ValueError that
    names the file."""
    with Image.open(path) as lab:
        if lab.mode not in LABEL_MODES:
            raise ValueError("%s: label files must be 8-bit single-channel images (PIL mode L or P), got mode %r" % (path, lab.mode))
        return lab.copy()


class DirectoryDataset(Dataset):
    """A folder of the user's own images, the reference's DirectoryDataset (src/data.py:75-118):

        {root}/{path}/imgs/{split}/*          images, any format PIL reads
        {root}/{path}/labels/{split}/*        optional: one label image per image

    Both listings are sorted and pair up by position; their counts must agree and the split must not be empty.  Item i is (image,
    label, mask): image and label go through `transform` / `target_transform` under one seed drawn from numpy's global generator (as
    CroppedDataset does), the label is the stored value itself (no "- 1"), -1 everywhere when the folder has no `labels`, and
    mask = (label > 0) as float32: the foreground / salience mask cfg.use_salience reads.

    Three deviations from the reference:
      * images are .convert("RGB") (the reference hands a grey or RGBA file to Normalize as it is);
      * the label is always [H, W] int64 and the mask [1, H, W] float32, the ranks of CroppedDataset's items (the reference gives
        [1, H, W] labels for labelled folders and [H, W] for unlabelled ones);
      * a label file must decode to an 8-bit single-channel array (PIL mode L or P), else ValueError with the file's name."""

    def __init__(self, root, path, image_set, transform=to_tensor, target_transform=to_target_tensor):
        super().__init__()
        self.split = image_set
        self.transform, self.target_transform = transform, target_transform
        self.dir = join(root, path)
        self.img_dir, self.label_dir = join(self.dir, "imgs", image_set), join(self.dir, "labels", image_set)
        self.img_files, self.label_files = directory_files(root, path, image_set)

    def __len__(self):
        return len(self.img_files)

    def __getitem__(self, index):
        seed = int(np.random.randint(2147483647))
        with Image.open(self.img_files[index]) as im:
            image = _seeded(self.transform, im.convert("RGB"), seed)
        if self.label_files is not None:
            label = _seeded(self.target_transform, open_label(self.label_files[index]), seed)
            label = label.reshape(label.shape[-2:])
        else:
            label = torch.zeros(image.shape[1], image.shape[2], dtype=torch.int64) - 1
        return image, label, (label > 0).to(torch.float32).unsqueeze(0)


def directory_files(root, path, image_set):
    """(image paths, label paths or None) of DirectoryDataset's split, both sorted by file name."""
    d = join(root, path)
    img_dir, label_dir = join(d, "imgs", image_set), join(d, "labels", image_set)
    imgs = [join(img_dir, f) for f in sorted(os.listdir(img_dir))]
    if not imgs:
        raise ValueError("%s: empty split %r" % (d, image_set))
    if not os.path.exists(join(d, "labels")):
        return imgs, None
    labels = [join(label_dir, f) for f in sorted(os.listdir(label_dir))]
    if len(imgs) != len(labels):
        raise AssertionError("%s: %d images but %d labels" % (d, len(imgs), len(labels)))
    return imgs, labels


class ContrastiveSegDataset(Dataset):
    """The reference's training / evaluation dataset (src/data.py:419-565) for the cropped trees (cocostuff27, cityscapes with a
    crop_type) and for dataset_name "directory" with crop_type None (DirectoryDataset of cfg.dir_dataset_name, n_classes =
    cfg.dir_dataset_n_classes; the table's name then carries cfg.dir_dataset_name and the literal "None"):
    CroppedDataset / DirectoryDataset items at `transform` / `target_transform`, and with pos_images / pos_labels a KNN positive per item,
    nns[ind][r] with r uniform in [1, num_neighbors] from the precomputed table {pytorch_data_dir}/nns/nns_{model_type}_{dataset}_
    {image_set}_{crop_type}_{res}.npz.  The random draws come in the reference's order: the item's own CroppedDataset seed (numpy),
    torch.randint for the neighbour rank, the positive's CroppedDataset seed, then one more numpy seed that reseeds python's and
    torch's generators (what the reference's augmentations would draw from).  The img_aug / coord_aug augmentations are not made
    here: they are made on the device, from the batch, by stego_amd.augment (cfg.native_aug; device_data.DeviceContrastiveLoader's
    aug=True, or training_step itself for batches of this loader).

    This is the CPU loader of train_segmentation when the split does not fit the device, and the oracle of
    device_data.DeviceContrastiveLoader."""

    def __init__(self, pytorch_data_dir, dataset_name, crop_type, image_set, transform, target_transform, cfg,
                 aug_geometric_transform=None, aug_photometric_transform=None, num_neighbors=5, compute_knns=False, mask=False,
                 pos_labels=False, pos_images=False, extra_transform=None, model_type_override=None):
        super().__init__()
        directory = dataset_name == "directory" and crop_type is None
        if not directory and (crop_type is None or dataset_name not in ("cocostuff27", "cityscapes")):
            raise ValueError("ContrastiveSegDataset reads the cropped trees (cocostuff27 / cityscapes with a crop_type) and image "
                             "folders (directory with crop_type None), got dataset %r, crop_type %r" % (dataset_name, crop_type))
        if aug_geometric_transform is not None or aug_photometric_transform is not None:
            raise ValueError("the img_aug / coord_aug augmentations are not supported")
        self.num_neighbors, self.image_set, self.dataset_name = num_neighbors, image_set, dataset_name
        self.mask, self.pos_labels, self.pos_images, self.extra_transform = mask, pos_labels, pos_images, extra_transform
        if directory:
            self.n_classes = cfg.dir_dataset_n_classes
            self.dataset = DirectoryDataset(pytorch_data_dir, cfg.dir_dataset_name, image_set, transform=transform,
                                            target_transform=target_transform)
        else:
            self.n_classes = 27
            self.dataset = CroppedDataset(pytorch_data_dir, dataset_name, crop_type, cfg.crop_ratio, image_set, transform=transform,
                                          target_transform=target_transform)
        model_type = model_type_override if model_type_override is not None else cfg.model_type
        from .precompute_knns import nns_filename
        nice_dataset_name = cfg.dir_dataset_name if directory else dataset_name
        feature_cache_file = join(pytorch_data_dir, "nns", nns_filename(model_type, nice_dataset_name, image_set, crop_type, cfg.res))
        self.feature_cache_file = feature_cache_file
        if pos_labels or pos_images:
            if not os.path.exists(feature_cache_file) or compute_knns:
                raise ValueError("could not find nn file {} please run precompute_knns".format(feature_cache_file))
            self.nns = np.load(feature_cache_file)["nns"]
            assert len(self.dataset) == self.nns.shape[0]

    def __len__(self):
        return len(self.dataset)

    def _set_seed(self, seed):
        random.seed(seed)
        torch.manual_seed(seed)

    def __getitem__(self, ind):
        pack = self.dataset[ind]
        if self.pos_images or self.pos_labels:
            ind_pos = self.nns[ind][torch.randint(low=1, high=self.num_neighbors + 1, size=[]).item()]
            pack_pos = self.dataset[ind_pos]
        seed = np.random.randint(2147483647)
        self._set_seed(seed)
        extra = self.extra_transform if self.extra_transform is not None else (lambda i, x: x)
        ret = {"ind": ind, "img": extra(ind, pack[0]), "label": extra(ind, pack[1])}
        if self.pos_images:
            ret["img_pos"] = extra(ind, pack_pos[0])
            ret["ind_pos"] = ind_pos
        if self.mask:
            ret["mask"] = pack[2]
        if self.pos_labels:
            ret["label_pos"] = extra(ind, pack_pos[1])
            ret["mask_pos"] = pack_pos[2]
        return ret
