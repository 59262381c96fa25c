"""Region descriptors and object search: the mean of a low-resolution map over every full-resolution region (include/stego_region_pool.h,
csrc/region_pool.hip), a folder-wide index of them, and the lookup "where else is an object like this one?".

Definitions - the kernels, the torch chain below and the oracle of tests/region_pool_oracle.py implement exactly these:

  inputs       ``maps [B, C, h, w]`` float32, any strides, finite; ``ids [B, H, W]`` int32 as ``label_regions`` writes it (-1: no
               region); the ``RegionTable`` of the same ids: the row of region ``id`` of image b is ``row_offset[b] + id``.
  pixel value  ``v(b, Y, X, c) = F.interpolate(maps, (H, W), mode="bilinear", align_corners=False)``: the source index in float32, every
               operation rounded on its own, taps ``i0``, ``i1 = i0 + (i0 < in - 1)`` and the weight ``l1 = s - i0`` of ``i1``.  With
               ``h == H`` and ``w == W`` the taps are the pixel itself: mean colours of an image, ``C = 3``.
  descriptor   the mean of v over the pixels of the region; 0 for a row without pixels.

The kernels evaluate v in float32, quantise it to a 30-bit integer against the largest magnitude of the map and sum in int64, so their
result does not depend on the order of the adds: two calls, and two ways to cut the rows into ranges, are bitwise equal.  The torch
chain (CPU tensors, and whatever the kernels' limits exclude) uses the same taps and float64 sums with ``index_add_`` and does not
quantise.  The two paths agree to ``2^-21 * max |maps|`` per element (tests/test_region_pool_gpu.py derives the bound), not bitwise.
"""
import numpy as np
import torch

from . import capi

MAX_ASK = 32                     # the most neighbours stego_knn_topk answers


# ---- arguments
def _checked(ids, table, maps):
    if not torch.is_tensor(ids) or ids.dim() != 3 or ids.dtype != torch.int32:
        raise ValueError("ids: expected the int32 [B, H, W] tensor of label_regions")
    if not torch.is_tensor(maps) or maps.dim() != 4 or not maps.dtype.is_floating_point:
        raise ValueError("maps: expected a floating-point [B, C, h, w] tensor")
    if maps.shape[0] != ids.shape[0] or len(table.n_regions) != ids.shape[0]:
        raise ValueError("ids, table and maps disagree on the number of images: %d, %d, %d" % (ids.shape[0], len(table.n_regions), maps.shape[0]))
    if min(ids.shape) < 1 or min(maps.shape) < 1:
        raise ValueError("an empty tensor: ids %s, maps %s" % (tuple(ids.shape), tuple(maps.shape)))


def _native(ids, maps):
    B, C, h, w = maps.shape
    return ids.is_cuda and maps.is_cuda and ids.shape[0] <= capi.REGIONS_MAX_B and C <= capi.REGION_POOL_MAX_C and \
        ids.shape[1] * ids.shape[2] <= capi.REGIONS_MAX_PIXELS and h * w <= capi.REGIONS_MAX_PIXELS


def pool_slabs(n_rows, channels, pool_bytes):
    """The [lo, hi) ranges of table rows whose int64 sums [rows, channels] fit `pool_bytes` together; at least one row a range, and no
    more than 2^31 - 1 sums in one."""
    rows = max(1, min(int(pool_bytes) // (8 * int(channels)), ((1 << 31) - 1) // int(channels)))
    return [(lo, min(lo + rows, n_rows)) for lo in range(0, n_rows, rows)]


# ---- the torch chain
def _taps(out, inp, device):
    """ATen's align_corners=False source index in float32 -> (i0, i1, the float64 weight of i1)."""
    scale = torch.tensor(inp, dtype=torch.float32, device=device) / torch.tensor(out, dtype=torch.float32, device=device)
    s = scale * (torch.arange(out, dtype=torch.float32, device=device) + 0.5) - 0.5
    s = torch.clamp(s, min=0)
    i0 = torch.clamp(s.long(), max=inp - 1)
    i1 = i0 + (i0 < inp - 1).long()
    return i0, i1, (s - i0.float()).double()


def _torch_chain_f64(ids, table, maps):
    """The descriptors in float64 [len(table), C] on the ids' device."""
    B, C, h, w = maps.shape
    H, W = ids.shape[1:]
    dev = ids.device
    maps = maps.detach().to(dev)
    y0, y1, ly = _taps(H, h, dev)
    x0, x1, lx = _taps(W, w, dev)
    ly, lx = ly[None, :, None], lx[None, None, :]
    sums = torch.zeros((len(table), C), dtype=torch.float64, device=dev)
    for b in range(B):
        m = maps[b].double()
        top, bot = m[:, y0], m[:, y1]
        v = (1 - ly) * ((1 - lx) * top[:, :, x0] + lx * top[:, :, x1]) + ly * ((1 - lx) * bot[:, :, x0] + lx * bot[:, :, x1])
        has = ids[b] >= 0
        rows = ids[b][has].long() + table.row_offset[b]
        keep = rows < len(table)
        sums.index_add_(0, rows[keep], v.permute(1, 2, 0)[has][keep])
    area = table.area.to(dev).double()[:, None]
    return torch.where(area > 0, sums / area.clamp(min=1), torch.zeros_like(sums))


def region_descriptors(ids, table, maps, normalize=False, pool_bytes=2 ** 28):
    """The mean of ``maps [B, C, h, w]``, bilinearly resized to the ids' size, over every region of ``table`` -> float32 [len(table), C]
    on the ids' device.  ``normalize=True`` L2-normalises the low-resolution tokens first (``F.normalize(maps, dim=1)``, what
    ClusterLookup does before its product); the kernel always pools the map it is given.  On the kernels the rows are answered in
    ranges whose int64 sums fit ``pool_bytes`` (at least one row a range) and nothing is read back: no host sync beyond what the table
    cost.  The native path and the torch chain agree to 2^-21 * max |maps| per element, not bitwise (module docstring)."""
    _checked(ids, table, maps)
    if int(pool_bytes) < 1:
        raise ValueError("pool_bytes must be positive, got %r" % (pool_bytes,))
    maps = maps.detach()
    if normalize:
        maps = torch.nn.functional.normalize(maps.float(), dim=1)
    C, n = maps.shape[1], len(table)
    if n == 0:
        return torch.zeros((0, C), dtype=torch.float32, device=ids.device)
    if not _native(ids, maps):
        return _torch_chain_f64(ids, table, maps).float()
    dev = ids.device
    maps, ids = maps.float(), ids.contiguous()
    offs = torch.tensor(table.row_offset, dtype=torch.int64, device=dev)
    area = table.area.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty((n, C), dtype=torch.float32, device=dev)
    ws = None
    for lo, hi in pool_slabs(n, C, pool_bytes):
        if ws is None:
            need = capi.region_pool_workspace_bytes(capi.region_pool_desc(ids.shape[0], C, maps.shape[2], maps.shape[3], ids.shape[1],
                                                                          ids.shape[2], hi - lo))
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        capi.region_pool(maps, ids, offs, area, lo, hi, out=out[lo:hi], workspace=ws)
    return out


def region_at(ids, b, x, y):
    """The region id under pixel (x, y) of image b of ``ids [B, H, W]`` (a tensor or an array; one [H, W] map with b = 0), or -1: no
    region there, or a pixel outside the map."""
    if ids.ndim == 2:
        ids = ids[None]
    if not (0 <= int(b) < ids.shape[0] and 0 <= int(y) < ids.shape[1] and 0 <= int(x) < ids.shape[2]):
        return -1
    return int(ids[int(b), int(y), int(x)])


# ---- the index of a folder
class RegionIndex:
    """The regions of many images as one table: ``descriptors`` float32 [R, C]; per row ``image`` (the number of the image in
    ``names``), ``region`` (its id in that image), ``label``, ``area`` and ``box`` (x0, y0, x1, y1, inclusive) as int64 arrays;
    ``names``, the images in the order they were added; ``pooled``, which map the descriptors are means of, "code" or "feats".
    Everything lives on the host as numpy arrays; ``search`` moves the descriptors to the device it is given."""
    COLUMNS = ("image", "region", "label", "area")

    def __init__(self, pooled="code"):
        if pooled not in ("code", "feats"):
            raise ValueError('pooled is "code" or "feats", got %r' % (pooled,))
        self.pooled = pooled
        self.names = []
        self._parts = []
        self._cache = None

    def add(self, name, table, b, descriptors):
        """Image b of `table` under `name`; `descriptors` are the rows of that image (float32 [n_regions[b], C], any device)."""
        rows = table.rows(b)
        d = descriptors.detach().float().cpu().numpy() if torch.is_tensor(descriptors) else np.asarray(descriptors, dtype=np.float32)
        n = table.n_regions[b]
        if d.ndim != 2 or d.shape[0] != n:
            raise ValueError("descriptors: expected [%d, C] for image %d of the table, got %s" % (n, b, d.shape))
        if self._parts and self._parts[0]["descriptors"].shape[1] != d.shape[1]:
            raise ValueError("descriptors: %d channels, the index holds %d" % (d.shape[1], self._parts[0]["descriptors"].shape[1]))
        col = lambda c: getattr(table, c)[rows].cpu().numpy().astype(np.int64)
        self._parts.append({"descriptors": np.ascontiguousarray(d), "image": np.full(n, len(self.names), dtype=np.int64),
                            "region": np.arange(n, dtype=np.int64), "label": col("label"), "area": col("area"),
                            "box": np.stack([col("x0"), col("y0"), col("x1"), col("y1")], 1).reshape(n, 4)})
        self.names.append(str(name))
        self._cache = None

    def _all(self):
        if self._cache is None:
            if self._parts:
                self._cache = {k: np.concatenate([p[k] for p in self._parts]) for k in self._parts[0]}
            else:
                self._cache = {"descriptors": np.zeros((0, 0), np.float32), "box": np.zeros((0, 4), np.int64),
                               **{k: np.zeros(0, np.int64) for k in self.COLUMNS}}
            self._parts = [self._cache] if self._parts else []
        return self._cache

    descriptors = property(lambda self: self._all()["descriptors"])
    image = property(lambda self: self._all()["image"])
    region = property(lambda self: self._all()["region"])
    label = property(lambda self: self._all()["label"])
    area = property(lambda self: self._all()["area"])
    box = property(lambda self: self._all()["box"])

    def __len__(self):
        return len(self.image)

    def save(self, path):
        """One .npz (uncompressed: the descriptors come back bit for bit)."""
        a = self._all()
        with open(path, "wb") as f:
            np.savez(f, names=np.array(self.names, dtype=np.str_), pooled=np.array(self.pooled), **a)
        return path

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            index = cls(str(z["pooled"]))
            index.names = [str(n) for n in z["names"]]
            part = {k: z[k] for k in ("descriptors", "box") + cls.COLUMNS}
        index._parts = [part] if len(part["image"]) else []
        return index

    def row_of(self, name, region_id):
        """The row of region `region_id` of image `name`; KeyError for an image or a region the index does not hold."""
        if name not in self.names:
            raise KeyError("no image %r in the index" % (name,))
        hit = np.nonzero((self.image == self.names.index(name)) & (self.region == int(region_id)))[0]
        if hit.size == 0:
            raise KeyError("image %r has no region %r" % (name, region_id))
        return int(hit[0])

    def row_info(self, row):
        """A row as a plain dict: image, region, label, area, box."""
        row = int(row)
        return {"image": self.names[int(self.image[row])], "region": int(self.region[row]), "label": int(self.label[row]),
                "area": int(self.area[row]), "box": [int(v) for v in self.box[row]]}

    def search(self, rows, k=8, min_area=0, other_images_only=True, device=None):
        """Per query row the k most similar rows by cosine -> (rows int64 [Q, k], similarities float32 [Q, k]), most similar first.
        Dropped: the query itself, rows with ``area < min_area`` and, with ``other_images_only``, the rows of the query's own image.
        On a HIP `device` this is one capi.knn_topk(normalize=True) over the whole index that asks for min(32, R) neighbours - the
        kernel's limit - and filters them on the host, so a query of which fewer than k survive among those 32 (or in the index at
        all, on either path) gets the survivors first and then row -1 with similarity -inf.  On the CPU (device None or "cpu") it is
        a torch chain of the same definition over every row: normalised float32 descriptors, one product, the same filter."""
        rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
        k, R = int(k), len(self)
        if k < 1:
            raise ValueError("k must be at least 1, got %r" % (k,))
        if rows.size and (rows.min() < 0 or rows.max() >= R):
            raise ValueError("a query row outside 0 .. %d" % (R - 1))
        out_rows = np.full((rows.size, k), -1, dtype=np.int64)
        out_sims = np.full((rows.size, k), -np.inf, dtype=np.float32)
        if rows.size == 0 or R == 0:
            return out_rows, out_sims
        dev = torch.device(device) if device is not None else torch.device("cpu")
        d = torch.from_numpy(self.descriptors).to(dev)
        if dev.type == "cuda":
            near, sims = capi.knn_topk(d, k=min(MAX_ASK, R), normalize=True, return_sims=True)
            near, sims = near[torch.from_numpy(rows).to(dev)].cpu().numpy(), sims[torch.from_numpy(rows).to(dev)].cpu().numpy()
        else:
            unit = torch.nn.functional.normalize(d, dim=1)
            full = unit[torch.from_numpy(rows)] @ unit.t()
            sims, near = torch.sort(full, dim=1, descending=True, stable=True)
            near, sims = near.numpy(), sims.numpy()
        for q, row in enumerate(rows):
            keep = (near[q] != row) & (self.area[near[q]] >= int(min_area))
            if other_images_only:
                keep &= self.image[near[q]] != self.image[row]
            n = min(k, int(keep.sum()))
            out_rows[q, :n] = near[q][keep][:n]
            out_sims[q, :n] = sims[q][keep][:n]
        return out_rows, out_sims
