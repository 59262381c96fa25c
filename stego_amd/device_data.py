"""A cropped split kept on the device, and the training / evaluation loaders that read it.

The reference feeds every training step from CPU workers (data.py ContrastiveSegDataset: PIL decode, Resize(NEAREST), crop,
ToTensor, Normalize per item).  Here the split is decoded once, its RGB and label bytes are uploaded once, and every batch - anchors
and KNN positives together - comes out of one launch of stego_data_prepare (include/stego_data.h, csrc/batch_prep.hip):

  DeviceImageStore           the decoded split on the device: two byte arenas, a record per crop, PIL's NEAREST index maps per R;
                             .from_directory: a user's image folder (data.DirectoryDataset) instead of a cropped split, with or
                             without labels, optionally reduced to one resolution (store_res); batches from stego_data_prepare_dir
  DeviceContrastiveLoader    batches with the reference's keys (ind, img, label, mask, img_pos, ind_pos, label_pos, mask_pos) as
                             device tensors, in DistributedSampler's epoch order; or, without a neighbour table, the split in order
                             (img, label, mask, ind) for validation and the KNN precompute
  epoch_indices              DistributedSampler(shuffle=True, seed).set_epoch(epoch)'s indices of one rank, as a pure function

The images are bitwise what data.image_transform / label_transform give the same PIL image (the resize maps are PIL's own, the
normalisation is a float32 table computed with the same numpy operations).
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor
from os.path import join

import numpy as np
import torch
from PIL import Image

from . import capi
from .data import _MEAN, _STD, _resize, crop_dir, directory_files, open_label, resized_size

DEFAULT_MAX_BYTES = 200 * 2 ** 30          # of the MI355X's 288 GB: what the split may take on the device (images + labels)

ITEM_DTYPE = np.dtype([("img_offset", "<i8"), ("label_offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("nh", "<i4"), ("nw", "<i4"),
                       ("row_map", "<i4"), ("col_map", "<i4"), ("center_top", "<i4"), ("center_left", "<i4")])
assert ITEM_DTYPE.itemsize == 48                # sizeof(StegoDataItem)


class StoreTooLarge(ValueError):
    """The split does not fit the device budget (DeviceImageStore's max_bytes)."""


def decode_threads():
    """At most 16 host threads; fewer when OMP_NUM_THREADS says so."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "16"))
    except ValueError:
        n = 16
    return max(1, min(16, n))


def pil_nearest_map(src, dst):
    """int32 [dst]: the source index PIL's NEAREST resize takes for every output position along one axis of length src -> dst.
    PIL's nearest resize is separable, so resizing a 1 x src int32 ramp (mode "I") to 1 x dst reads the map off PIL itself
    (no closed formula reproduces its column choice in every case)."""
    if src == dst:
        return np.arange(src, dtype=np.int32)
    ramp = Image.fromarray(np.arange(src, dtype=np.int32)[None, :], "I")
    return np.asarray(ramp.resize((dst, 1), Image.NEAREST), dtype=np.int32)[0].copy()


def normalize_lut():
    """float32 [3, 256]: (u8 / 255 - mean_c) / std_c with the float32 numpy operations of data.image_transform."""
    x = np.arange(256, dtype=np.float32)[:, None] / np.float32(255.0)
    return np.ascontiguousarray(((x - _MEAN) / _STD).T)


def epoch_indices(n, world, rank, seed, epoch):
    """int64 [ceil(n / world)]: DistributedSampler(n items, num_replicas=world, rank=rank, shuffle=True, seed=seed,
    drop_last=False) after set_epoch(epoch) - one permutation for all ranks, padded by repeating its head, every world-th index."""
    g = torch.Generator()
    g.manual_seed(seed + epoch)
    perm = torch.randperm(n, generator=g)
    per = math.ceil(n / world)
    total = per * world
    if total > n:
        perm = torch.cat([perm] * math.ceil(total / n))[:total]
    return perm[rank:total:world].clone()


def _split_files(root, dataset_name, crop_type, crop_ratio, split):
    d = crop_dir(root, dataset_name, crop_type, crop_ratio)
    img_dir, label_dir = join(d, "img", split), join(d, "label", split)
    n = len(os.listdir(img_dir))
    if n != len(os.listdir(label_dir)):
        raise AssertionError("%s: %d images but %d labels" % (d, n, len(os.listdir(label_dir))))
    return [(join(img_dir, "%d.jpg" % i), join(label_dir, "%d.png" % i)) for i in range(n)]


def _sizes(files, threads):
    def one(f):
        with Image.open(f[0]) as im:           # the header only
            return im.size
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, files))


def split_bytes(root, dataset_name, crop_type, crop_ratio, split):
    """Device bytes a DeviceImageStore of the split takes (RGB + label bytes), from the image headers alone."""
    sizes = _sizes(_split_files(root, dataset_name, crop_type, crop_ratio, split), decode_threads())
    return sum(w * h * 4 for w, h in sizes)


def _reduce(im, store_res):
    """What a directory store keeps of a decoded image or label: data._resize(im, store_res) when that makes it smaller (short side
    above store_res), else the image itself - an image at or below store_res is upscaled by prepare's index maps, not in the store."""
    return im if store_res is None or min(im.size) <= store_res else _resize(im, store_res)


def _stored_sizes(files, store_res, threads):
    """(w, h) of every image as a directory store keeps it (_reduce), from the headers alone."""
    sizes = _sizes([(f,) for f in files], threads)
    return [(w, h) if store_res is None or min(w, h) <= store_res else resized_size(w, h, store_res) for w, h in sizes]


def directory_bytes(root, path, split, store_res=None):
    """Device bytes DeviceImageStore.from_directory(root, path, split, store_res=store_res) takes (RGB bytes, and label bytes when
    the folder has labels), from the image headers alone."""
    imgs, labels = directory_files(root, path, split)
    per_pixel = 3 if labels is None else 4
    return sum(w * h * per_pixel for w, h in _stored_sizes(imgs, store_res, decode_threads()))


class DeviceImageStore:
    """Every crop of `{root}/cropped/{dataset}_{crop_type}_crop_{ratio}/{img,label}/{split}` decoded once (PIL, .convert("RGB") for
    the images, the label PNG's bytes as they are) and kept on `device`: `images` uint8 [sum h*w*3] (HWC RGB per crop) and `labels`
    uint8 [sum h*w] (stored value = label + 1).  `prepare(index, R, origin)` makes a batch; the record table and PIL's index maps of
    a resolution are built on first use of that R.  Raises StoreTooLarge when the split needs more than `max_bytes`."""

    def __init__(self, root, dataset_name, crop_type, crop_ratio, split, device=None, max_bytes=DEFAULT_MAX_BYTES):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.split = split
        files = _split_files(root, dataset_name, crop_type, crop_ratio, split)
        if not files:
            raise ValueError("%s: empty split %r" % (crop_dir(root, dataset_name, crop_type, crop_ratio), split))
        threads = decode_threads()
        sizes = _sizes(files, threads)
        self.w = np.array([s[0] for s in sizes], dtype=np.int64)
        self.h = np.array([s[1] for s in sizes], dtype=np.int64)
        npx = self.h * self.w
        self.nbytes = int(npx.sum()) * 4
        if self.nbytes > max_bytes:
            raise StoreTooLarge("the %s split of %s needs %.2f GB on the device (%d crops) and the budget is %.2f GB"
                                % (split, crop_dir(root, dataset_name, crop_type, crop_ratio), self.nbytes / 1e9, len(files), max_bytes / 1e9))
        self.label_offsets = np.concatenate([[0], np.cumsum(npx)[:-1]]).astype(np.int64)
        self.img_offsets = self.label_offsets * 3
        host_img = np.empty(int(npx.sum()) * 3, dtype=np.uint8)
        host_lab = np.empty(int(npx.sum()), dtype=np.uint8)

        def decode(i):
            h, w = int(self.h[i]), int(self.w[i])
            with Image.open(files[i][0]) as im:
                rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
            with Image.open(files[i][1]) as lb:
                lab = np.asarray(lb)
            if lab.dtype != np.uint8 or lab.shape != (h, w) or rgb.shape != (h, w, 3):
                raise ValueError("%s: expected a %d x %d 8-bit label PNG for %s, got %s %s"
                                 % (files[i][1], w, h, files[i][0], lab.dtype, lab.shape))
            o = int(self.label_offsets[i])
            host_img[3 * o:3 * (o + h * w)] = rgb.reshape(-1)
            host_lab[o:o + h * w] = lab.reshape(-1)

        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(decode, range(len(files))))
        self.images = torch.from_numpy(host_img).to(self.device)
        self.labels = torch.from_numpy(host_lab).to(self.device)
        self.lut = torch.from_numpy(normalize_lut()).to(self.device)
        self._tables = {}

    kind, store_res = "cropped", None       # from_directory: "directory", and the one R a reduced store serves

    @classmethod
    def from_directory(cls, root, path, split, device=None, max_bytes=DEFAULT_MAX_BYTES, store_res=None):
        """The store of a data.DirectoryDataset split, `{root}/{path}/imgs/{split}/*` and, when `{root}/{path}/labels` exists,
        `{root}/{path}/labels/{split}/*`: the same two arenas and record table, `labels` None when the folder has none.  `prepare`
        then goes through stego_data_prepare_dir: label = the stored byte (-1 without labels), mask float32 = label > 0.

        store_res = R: every decoded image and label whose short side is above R is reduced on the host with data._resize(im, R)
        (PIL's NEAREST) before the upload - a folder of megapixel photos does not fit the device at full size; smaller images are
        kept as they are (the store never grows).  resized_size leaves an image whose short side already is R alone, so
        prepare(index, R) is still bitwise the transform of the original file, for centre and random crops alike; such a store
        serves that R only (table / prepare raise ValueError for another one)."""
        self = cls.__new__(cls)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.split, self.kind, self.store_res = split, "directory", None if store_res is None else int(store_res)
        if self.store_res is not None and not 1 <= self.store_res <= capi.DATA_MAX_RES:
            raise ValueError("store_res = %d outside [1, %d] (include/stego_data.h)" % (self.store_res, capi.DATA_MAX_RES))
        imgs, labs = directory_files(root, path, split)
        threads = decode_threads()
        sizes = _stored_sizes(imgs, self.store_res, threads)
        self.w = np.array([s[0] for s in sizes], dtype=np.int64)
        self.h = np.array([s[1] for s in sizes], dtype=np.int64)
        npx = self.h * self.w
        total = int(npx.sum())
        self.nbytes = total * (3 if labs is None else 4)
        if self.nbytes > max_bytes:
            raise StoreTooLarge("the %s split of %s needs %.2f GB on the device (%d images%s) and the budget is %.2f GB"
                                % (split, join(root, path), self.nbytes / 1e9, len(imgs),
                                   "" if self.store_res is None else ", reduced to store_res = %d" % self.store_res, max_bytes / 1e9))
        self.label_offsets = np.concatenate([[0], np.cumsum(npx)[:-1]]).astype(np.int64)
        self.img_offsets = self.label_offsets * 3
        host_img = np.empty(total * 3, dtype=np.uint8)
        host_lab = None if labs is None else np.empty(total, dtype=np.uint8)

        def decode(i):
            h, w = int(self.h[i]), int(self.w[i])
            o = int(self.label_offsets[i])
            with Image.open(imgs[i]) as im:
                im = im.convert("RGB")
                rgb = np.asarray(_reduce(im, self.store_res), dtype=np.uint8)
            if rgb.shape != (h, w, 3):
                raise ValueError("%s: decoded to %s, its header said %d x %d" % (imgs[i], rgb.shape, w, h))
            host_img[3 * o:3 * (o + h * w)] = rgb.reshape(-1)
            if labs is not None:
                lab = np.asarray(_reduce(open_label(labs[i]), self.store_res))
                if lab.dtype != np.uint8 or lab.shape != (h, w):
                    raise ValueError("%s: expected a %d x %d 8-bit label image for %s, got %s %s"
                                     % (labs[i], w, h, imgs[i], lab.dtype, lab.shape))
                host_lab[o:o + h * w] = lab.reshape(-1)

        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(decode, range(len(imgs))))
        self.images = torch.from_numpy(host_img).to(self.device)
        self.labels = None if labs is None else torch.from_numpy(host_lab).to(self.device)
        self._label_bytes = total           # what the records' label offsets are checked against, with or without the arena
        self.lut = torch.from_numpy(normalize_lut()).to(self.device)
        self._tables = {}
        return self

    def __len__(self):
        return len(self.h)

    def table(self, R):
        """The record table of resolution R: dict(items = uint8 device bytes of StegoDataItem [n], maps = int32 device pool,
        span = int64 device [n, 2] (nh - R, nw - R), desc = the descriptor's (R, n, arena sizes, pool length), records = host copy)."""
        t = self._tables.get(R)
        if t is not None:
            return t
        if not 1 <= R <= capi.DATA_MAX_RES:
            raise ValueError("resolution R = %d outside [1, %d] (include/stego_data.h)" % (R, capi.DATA_MAX_RES))
        if self.store_res is not None and R != self.store_res:
            raise ValueError("this store was reduced to store_res = %d and serves that resolution only, not R = %d" % (self.store_res, R))
        n = len(self)
        rec = np.zeros(n, dtype=ITEM_DTYPE)
        pool, where, at = [], {}, 0

        def map_of(src, dst):
            nonlocal at
            if (src, dst) not in where:
                m = pil_nearest_map(src, dst)
                where[(src, dst)] = at
                pool.append(m)
                at += len(m)
            return where[(src, dst)]

        for i in range(n):
            h, w = int(self.h[i]), int(self.w[i])
            nw, nh = resized_size(w, h, R)
            rec[i] = (self.img_offsets[i], self.label_offsets[i], h, w, nh, nw, map_of(h, nh), map_of(w, nw),
                      int(round((nh - R) / 2.0)), int(round((nw - R) / 2.0)))
        maps = np.concatenate(pool).astype(np.int32)
        desc = (R, n, self.images.numel(), self.labels.numel() if self.labels is not None else self._label_bytes, len(maps))
        rc, bad = capi.data_check_items(capi.data_desc(1, *desc), rec)
        if rc != 0:
            raise ValueError("record %d of the %s split is invalid at R = %d: %s (error %d)"
                             % (bad, self.split, R, rec[bad], rc))
        t = dict(items=torch.from_numpy(rec.view(np.uint8)).to(self.device), maps=torch.from_numpy(maps).to(self.device),
                 span=torch.from_numpy(np.stack([rec["nh"] - R, rec["nw"] - R], 1).astype(np.int64)).to(self.device),
                 desc=desc, records=rec)
        self._tables[R] = t
        return t

    def prepare(self, index, R, origin=None, validate=False):
        """One launch: index int64 [N] (device) -> img float32 [N,3,R,R], label int64 [N,R,R] (stored value - 1), mask bool [N,1,R,R]
        (label == -1); on a from_directory store label = the stored value (-1 without labels) and mask float32 (label > 0).  origin: int32 [N, 2] (top, left) in resized coordinates, or None for centre crops.  validate=True checks the
        indices and origins on the host first (a device -> host copy) and raises ValueError with the offending value."""
        t = self.table(R)
        index = index.to(self.device, torch.int64).contiguous()
        if origin is not None:
            origin = origin.to(self.device, torch.int32).contiguous()
            if tuple(origin.shape) != (index.numel(), 2):
                raise ValueError("origin must be int32 [N, 2] for N = %d indices, got %s" % (index.numel(), tuple(origin.shape)))
        if not 1 <= index.numel() <= capi.DATA_MAX_N:
            raise ValueError("N = %d items per launch outside [1, %d]" % (index.numel(), capi.DATA_MAX_N))
        if validate:
            ind = index.cpu().numpy()
            bad = np.flatnonzero((ind < 0) | (ind >= len(self)))
            if bad.size:
                raise ValueError("index %d at position %d outside [0, %d)" % (ind[bad[0]], bad[0], len(self)))
            if origin is not None:
                o, rec = origin.cpu().numpy(), t["records"][ind]
                bad = np.flatnonzero((o[:, 0] < 0) | (o[:, 1] < 0) | (o[:, 0] > rec["nh"] - R) | (o[:, 1] > rec["nw"] - R))
                if bad.size:
                    k = bad[0]
                    raise ValueError("crop origin %s of item %d (resized %d x %d) does not fit R = %d"
                                     % (tuple(o[k]), ind[k], rec["nh"][k], rec["nw"][k], R))
        if self.kind == "directory":
            return capi.data_prepare_dir(t["desc"], t["items"], self.images, self.labels, t["maps"], self.lut, index, origin)
        return capi.data_prepare(t["desc"], t["items"], self.images, self.labels, t["maps"], self.lut, index, origin)


class _LoaderDataset:
    """What Trainer.fit reads from `loader.dataset`: the number of items and how the token cache may key them."""

    def __init__(self, n, deterministic):
        self.n, self.deterministic_items = n, deterministic
        self.n_cache_items = n              # ind and ind_pos are both indices of the store
        self.per_rank = True                # the loader slices the epoch by rank itself

    def __len__(self):
        return self.n


class DeviceContrastiveLoader:
    """Batches of a DeviceImageStore as device tensors.

    With a neighbour table `nns` (int64 [n, >= num_neighbors + 1], row i's neighbours by similarity, column 0 = i itself): the
    reference's training batches (data.py ContrastiveSegDataset with pos_images, pos_labels and mask): `ind`, `img`, `label`,
    `mask`, `img_pos`, `ind_pos`, `label_pos`, `mask_pos`, and with aug=True `img_aug` and `coord_aug`, the augmented view of the
    anchors of the batch just prepared (stego_amd.augment: one more native call; `last_aug_params` holds its draws, which come from
    a host generator seeded from (seed, rank) as well).  Epoch e visits epoch_indices(n, world, rank, seed, e) in batches of
    `batch_size` (the last incomplete batch dropped with drop_last) - DistributedSampler's order.  The positive of `ind` is
    nns[ind, r], r uniform in [1, num_neighbors] (data.py:524); with crop="random" every crop origin is uniform over the resized
    image (RandomCrop).  Both come from a device generator seeded from (seed, rank) at construction: two loaders built alike give
    identical batches, but the stream is not the reference's per-worker one.  `last_origin` holds the int32 [2B, 2] origins
    (anchors, then positives) of the latest random-crop batch.

    Without `nns`: the split in order, `img`, `label`, `mask`, `ind` (validation, the KNN precompute); rank and world are ignored.
    One stego_data_prepare launch per batch covers anchors and positives together."""

    def __init__(self, store, nns=None, batch_size=16, num_neighbors=7, res=224, crop="center", seed=0, rank=0, world=1, drop_last=True,
                 aug=False):
        if crop not in ("center", "random"):
            raise ValueError("Unknown Cropper {}".format(crop))
        self.store, self.batch_size, self.num_neighbors, self.res, self.crop = store, int(batch_size), int(num_neighbors), int(res), crop
        self.seed, self.rank, self.world, self.drop_last = int(seed), int(rank), int(world), bool(drop_last)
        self.positives = nns is not None
        n = len(store)
        if self.positives:
            nns = torch.as_tensor(np.asarray(nns) if not torch.is_tensor(nns) else nns.cpu(), dtype=torch.int64)
            if nns.dim() != 2 or nns.shape[0] != n or nns.shape[1] <= self.num_neighbors:
                raise ValueError("nns table of shape %s for %d items and num_neighbors = %d: need [%d, > %d]"
                                 % (tuple(nns.shape), n, self.num_neighbors, n, self.num_neighbors))
            if bool(((nns < 0) | (nns >= n)).any()):
                raise ValueError("nns table holds indices outside [0, %d)" % n)
            self._nns = nns.to(store.device)
        self.dataset = _LoaderDataset(n, crop == "center")
        self.deterministic_items, self.n_cache_items, self.per_rank = crop == "center", n, True
        self.epoch = 0
        self.last_origin = None
        self.last_aug_params = None
        self._augmenter = None
        if aug:
            from .augment import Augmenter
            self._augmenter = Augmenter(self.res, self.seed, self.rank)
        self._gen = torch.Generator(device=store.device)
        self._gen.manual_seed((self.seed * 1000003 + self.rank) & 0x7FFFFFFFFFFFFFFF)
        store.table(self.res)

    def _items_per_epoch(self):
        n = len(self.store)
        return math.ceil(n / self.world) if self.positives else n

    def __len__(self):
        m = self._items_per_epoch()
        return m // self.batch_size if self.drop_last else math.ceil(m / self.batch_size)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _origins(self, ind):
        span = self.store.table(self.res)["span"][ind]
        u = torch.rand(ind.numel(), 2, generator=self._gen, device=self.store.device)
        return torch.minimum((u * (span + 1).float()).floor().long(), span).int()

    def __iter__(self):
        dev, B = self.store.device, self.batch_size
        if self.positives:
            order = epoch_indices(len(self.store), self.world, self.rank, self.seed, self.epoch)
        else:
            order = torch.arange(len(self.store), dtype=torch.int64)
        self.epoch += 1
        order = order.to(dev)
        for b in range(len(self)):
            ind = order[b * B:(b + 1) * B]
            if not self.positives:
                origin = self._origins(ind) if self.crop == "random" else None
                img, label, mask = self.store.prepare(ind, self.res, origin)
                self.last_origin = origin
                yield dict(ind=ind, img=img, label=label, mask=mask)
                continue
            r = torch.randint(1, self.num_neighbors + 1, (ind.numel(),), generator=self._gen, device=dev)
            ind_pos = self._nns[ind, r]
            both = torch.cat([ind, ind_pos])
            origin = self._origins(both) if self.crop == "random" else None
            img, label, mask = self.store.prepare(both, self.res, origin)
            self.last_origin = origin
            k = ind.numel()
            batch = dict(ind=ind, img=img[:k], label=label[:k], mask=mask[:k], img_pos=img[k:], ind_pos=ind_pos, label_pos=label[k:],
                         mask_pos=mask[k:])
            if self._augmenter is not None:
                self._augmenter(batch)
                self.last_aug_params = self._augmenter.last_params
            yield batch
