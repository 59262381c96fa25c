"""Segments as objects: the connected regions of a label map, their table, and the cleanup of small regions (include/stego_regions.h,
csrc/regions.hip).

Definitions - the kernels, the CPU chain below and the oracle of tests/regions_oracle.py implement exactly these:

  input        ``labels [B, H, W]``, an integer tensor, contiguous.  Every image is on its own.
  region       a maximal set of pixels with the same label >= 0, connected under ``connectivity`` 4 or 8.  A pixel with a negative label
               belongs to no region: its id is -1.
  first pixel  the pixel of a region with the smallest raster index ``y * W + x``.
  region id    the regions of an image are numbered 0 .. n - 1 in increasing order of their first pixel.
  table        integer columns, a row per region: label, area, y0, x0, y1, x1 (an inclusive box), first, sum_y, sum_x.  There are no
               float sums, so every output is independent of the order of the adds: two calls are bitwise equal.
  cleanup      one round, ``min_area >= 1``, ``n_labels <= 256``: a region is small when ``area < min_area``; ``votes[r][c]`` of a small
               region r counts the ordered pairs of 4-neighbours (p, q) with p in r, q in a region that is not small, label(q) = c
               (always 4-neighbours, whatever the regions' connectivity; a label >= n_labels casts no vote); r takes the class with the
               most votes, the smallest class on a tie, and keeps its label without votes.  Every small region is relabelled at once,
               from the round's input state.  ``merge_small_regions`` repeats rounds, with the regions found anew each time, until a
               round changes nothing or ``max_rounds`` rounds have run.

Two properties of this cleanup, both intended: a blocky 5-class 96 x 96 map with 8 % speckle is clean after one round at
``min_area = 6`` - and a map of pure 27-class noise is left as it is, because no region there has a neighbour that is not small.

int64, int32 and uint8 HIP tensors with at most 65535 images run on the kernels; everything else (CPU tensors, other integer dtypes)
takes the numpy chain of the same definitions: the public functions never fail on where the tensor lives.
"""
import json

import numpy as np
import torch

from . import capi

MAX_LABELS = capi.REGIONS_MAX_LABELS
NO_REGION_U16 = 65535            # the id of a pixel without a region in a 16-bit id map


# ---- arguments
def _checked(labels, connectivity):
    if not torch.is_tensor(labels) or labels.dim() != 3:
        raise ValueError("labels: expected a [B, H, W] tensor, got %s" % (tuple(labels.shape) if torch.is_tensor(labels) else type(labels),))
    if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise ValueError("labels: expected an integer tensor, got %s" % labels.dtype)
    if connectivity not in (4, 8):
        raise ValueError("connectivity is 4 or 8, got %r" % (connectivity,))
    B, H, W = labels.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError("labels: an empty tensor %s" % (tuple(labels.shape),))
    if H * W > capi.REGIONS_MAX_PIXELS:
        raise ValueError("labels: %d x %d pixels an image; raster indices are int32, H * W must stay below 2^31" % (H, W))
    if not labels.is_contiguous():
        raise ValueError("labels: expected a contiguous tensor (strides %s)" % (labels.stride(),))
    return labels


def _native(labels):
    return labels.is_cuda and labels.dtype in capi.REGIONS_DTYPES and labels.shape[0] <= capi.REGIONS_MAX_B


# ---- the numpy chain
def _np_label_one(lab, connectivity):
    """int64 [H, W] -> (ids int32 [H, W], n): every pixel takes the smallest raster index among itself and its neighbours of the same
    label, then jumps to where that index points, until nothing moves."""
    H, W = lab.shape
    valid = lab >= 0
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    cur = idx.copy()
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    pairs = []
    for dy, dx in steps:                    # views of the two ends of every neighbour pair
        ya, yb = slice(0, H - dy), slice(dy, H)
        xa, xb = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        same = (lab[ya, xa] == lab[yb, xb]) & valid[ya, xa]
        pairs.append((ya, xa, yb, xb, same))
    while True:
        new = cur.copy()
        for ya, xa, yb, xb, same in pairs:
            a, b = new[ya, xa], new[yb, xb]
            low = np.minimum(a, b)
            np.minimum(a, low, out=a, where=same)           # a pixel is an end of several pairs: never raise what another pair lowered
            np.minimum(b, low, out=b, where=same)
        flat = new.reshape(-1)
        for _ in range(4):
            flat = flat[flat]
        new = flat.reshape(H, W)
        if np.array_equal(new, cur):
            break
        cur = new
    roots = valid & (cur == idx)
    rank = np.cumsum(roots.reshape(-1)) - 1
    ids = np.where(valid, rank[cur.reshape(-1)].reshape(H, W), -1).astype(np.int32)
    return ids, int(roots.sum())


def _np_table_one(lab, ids, n):
    """-> the nine int64 columns of one image, in RegionTable.COLUMNS order."""
    H, W = lab.shape
    ys, xs = np.nonzero(ids >= 0)
    r = ids[ys, xs].astype(np.int64)
    raster = ys.astype(np.int64) * W + xs
    cols = {name: np.zeros(n, dtype=np.int64) for name in RegionTable.COLUMNS}
    big = np.iinfo(np.int64).max
    for name in ("y0", "x0", "first"):
        cols[name][:] = big
    cols["y1"][:] = -1
    cols["x1"][:] = -1
    np.add.at(cols["area"], r, 1)
    np.add.at(cols["sum_y"], r, ys)
    np.add.at(cols["sum_x"], r, xs)
    np.minimum.at(cols["y0"], r, ys)
    np.minimum.at(cols["x0"], r, xs)
    np.maximum.at(cols["y1"], r, ys)
    np.maximum.at(cols["x1"], r, xs)
    np.minimum.at(cols["first"], r, raster)
    cols["label"] = lab.reshape(-1)[cols["first"]] if n else cols["label"]
    return cols


def _np_votes(lab, ids, small, rank, lo, hi, n_labels):
    """One image, int64 [H, W] labels: the votes [hi - lo, n_labels] of the small regions whose rank is in [lo, hi)."""
    H, W = lab.shape
    votes = np.zeros((hi - lo, n_labels), dtype=np.int64)
    has = ids >= 0
    safe = np.where(has, ids, 0)
    px_rank = np.where(has, rank[safe] if rank.size else -1, -1)
    voter = has & ~(small[safe] if small.size else False) & (lab < n_labels)
    mine = (px_rank >= lo) & (px_rank < hi)
    for (pa, qa) in (((slice(1, H), slice(None)), (slice(0, H - 1), slice(None))), ((slice(0, H - 1), slice(None)), (slice(1, H), slice(None))),
                     ((slice(None), slice(1, W)), (slice(None), slice(0, W - 1))), ((slice(None), slice(0, W - 1)), (slice(None), slice(1, W)))):
        hit = mine[pa] & voter[qa]
        np.add.at(votes, (px_rank[pa][hit] - lo, lab[qa][hit]), 1)
    return votes


# ---- the table
class RegionTable:
    """The regions of a batch of label maps, a row per region, image after image: the rows of image b are
    ``row_offset[b] .. row_offset[b] + n_regions[b]`` (``rows(b)`` is that slice; both are host lists).  The columns are integer
    tensors on the labels' device: ``label`` ``sum_y`` ``sum_x`` int64, ``area`` ``y0`` ``x0`` ``y1`` ``x1`` ``first`` int32 (int64
    from the CPU chain); the box is inclusive, ``first`` is the raster index y * W + x of the region's first pixel."""
    COLUMNS = ("label", "area", "y0", "x0", "y1", "x1", "first", "sum_y", "sum_x")

    def __init__(self, columns, n_regions, width):
        self.n_regions = [int(n) for n in n_regions]
        self.row_offset = [int(v) for v in np.concatenate([[0], np.cumsum(self.n_regions)[:-1]])] if self.n_regions else []
        self.width = int(width)
        for name in self.COLUMNS:
            setattr(self, name, columns[name])

    def __len__(self):
        return sum(self.n_regions)

    def rows(self, b):
        return slice(self.row_offset[b], self.row_offset[b] + self.n_regions[b])

    def centroids(self):
        """float64 [rows, 2]: (sum_y / area, sum_x / area), computed here and nowhere on the device."""
        area = self.area.double()
        return torch.stack([self.sum_y.double() / area, self.sum_x.double() / area], dim=1)


def label_regions(labels, connectivity=4):
    """labels [B, H, W] -> (ids int32 [B, H, W], n_regions int32 [B]) on the labels' device; no host sync on the kernels."""
    labels = _checked(labels, connectivity)
    if _native(labels):
        ids, n, _ = capi.regions_label(labels, connectivity)
        return ids, n
    lab = labels.detach().cpu().numpy().astype(np.int64)
    outs = [_np_label_one(lab[b], connectivity) for b in range(lab.shape[0])]
    ids = torch.from_numpy(np.stack([o[0] for o in outs])).to(labels.device)
    return ids, torch.tensor([o[1] for o in outs], dtype=torch.int32, device=labels.device)


def _ids_arg(labels, ids, n_regions):
    if not torch.is_tensor(ids) or ids.shape != labels.shape or ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError("ids: expected the contiguous int32 %s tensor of label_regions" % (tuple(labels.shape),))
    if not torch.is_tensor(n_regions) or tuple(n_regions.shape) != (labels.shape[0],):
        raise ValueError("n_regions: expected a [%d] tensor" % labels.shape[0])


def region_table(labels, ids, n_regions):
    """The RegionTable of label_regions' (ids, n_regions).  One host sync, the only one: n_regions is read to size the table."""
    labels = _checked(labels, 4)
    _ids_arg(labels, ids, n_regions)
    counts = [int(v) for v in n_regions.cpu()]                      # the sync
    if _native(labels) and ids.is_cuda:
        total = sum(counts)
        offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64), device=labels.device)
        c32, c64 = capi.regions_table(labels, ids, offs, total)
        cols = dict(zip(capi.REGIONS_COLS32, c32))
        cols.update(zip(capi.REGIONS_COLS64, c64))
        return RegionTable(cols, counts, labels.shape[2])
    lab = labels.detach().cpu().numpy().astype(np.int64)
    idn = ids.cpu().numpy()
    per = [_np_table_one(lab[b], idn[b], counts[b]) for b in range(lab.shape[0])]
    cols = {name: torch.from_numpy(np.concatenate([p[name] for p in per])).to(labels.device) for name in RegionTable.COLUMNS}
    return RegionTable(cols, counts, labels.shape[2])


# ---- the cleanup
def _cleanup_args(min_area, n_labels, vote_bytes):
    if int(min_area) < 1:
        raise ValueError("min_area must be at least 1, got %r" % (min_area,))
    if not 1 <= int(n_labels) <= MAX_LABELS:
        raise ValueError("n_labels must lie in 1 .. %d, got %r" % (MAX_LABELS, n_labels))
    if int(vote_bytes) < 1:
        raise ValueError("vote_bytes must be positive, got %r" % (vote_bytes,))
    return int(min_area), int(n_labels), max(1, int(vote_bytes) // (4 * int(n_labels)))


def vote_slabs(n_small, n_labels, vote_bytes):
    """The [lo, hi) ranges of small regions whose int32 vote rows fit `vote_bytes` together; at least one row a slab."""
    rows = max(1, int(vote_bytes) // (4 * int(n_labels)))
    return [(lo, min(lo + rows, n_small)) for lo in range(0, n_small, rows)]


def cleanup_round(labels, min_area, n_labels, connectivity=4, vote_bytes=2 ** 28):
    """One round of the small-region cleanup -> (the relabelled map, a new tensor of the input's dtype, or `labels` itself when no
    region is small; the number of regions whose label changed).  Syncs with the host: the table's size, the number of small regions
    and the changed count are read."""
    labels = _checked(labels, connectivity)
    min_area, n_labels, _ = _cleanup_args(min_area, n_labels, vote_bytes)
    ids, n = label_regions(labels, connectivity)
    table = region_table(labels, ids, n)
    if len(table) == 0:
        return labels, 0
    small = table.area < min_area
    rank = torch.where(small, torch.cumsum(small, 0) - 1, torch.full_like(table.first, -1, dtype=torch.int64)).to(torch.int32)
    n_small = int(small.sum())
    if n_small == 0:
        return labels, 0
    slabs = vote_slabs(n_small, n_labels, vote_bytes)
    if _native(labels):
        out = labels.clone()
        offs = torch.tensor(table.row_offset, dtype=torch.int64, device=labels.device)
        changed = torch.zeros(1, dtype=torch.int32, device=labels.device)
        votes = torch.empty((slabs[0][1] - slabs[0][0], n_labels), dtype=torch.int32, device=labels.device)
        first = table.first.contiguous()
        for lo, hi in slabs:
            capi.regions_votes(labels, ids, offs, rank, lo, hi, n_labels, votes=votes)
            capi.regions_relabel(labels, out, ids, offs, rank, first, lo, hi, n_labels, votes, changed)
        return out, int(changed)
    lab = labels.detach().cpu().numpy().astype(np.int64)
    idn, out = ids.cpu().numpy(), lab.copy()
    small_n, rank_n, label_n = small.cpu().numpy(), rank.cpu().numpy().astype(np.int64), table.label.cpu().numpy()
    changed = 0
    for b in range(lab.shape[0]):
        rows = table.rows(b)
        sm, rk = small_n[rows], rank_n[rows]
        has = idn[b] >= 0
        px_rank = np.where(has, rk[np.where(has, idn[b], 0)] if rk.size else -1, -1)
        for lo, hi in slabs:
            if not ((rk >= lo) & (rk < hi)).any():
                continue
            votes = _np_votes(lab[b], idn[b], sm, rk, lo, hi, n_labels)
            best, cls = votes.max(1), votes.argmax(1)                  # numpy's argmax is the first maximum
            mine = (px_rank >= lo) & (px_rank < hi)
            win = mine & (best[np.where(mine, px_rank - lo, 0)] > 0)
            out[b][win] = cls[px_rank[win] - lo]
            in_slab = (rk >= lo) & (rk < hi)
            changed += int(((best[rk[in_slab] - lo] > 0) & (cls[rk[in_slab] - lo] != label_n[rows][in_slab])).sum())
    return torch.from_numpy(out).to(labels.dtype).to(labels.device), changed


def merge_small_regions(labels, min_area, n_labels, connectivity=4, max_rounds=4, vote_bytes=2 ** 28):
    """Rounds of cleanup_round, the regions found anew each time, until one changes nothing or `max_rounds` have run -> (the cleaned
    map in the input's dtype, the rounds run - the one that changed nothing counts).  `vote_bytes` bounds the vote table: the small
    regions are voted on in slabs of vote_bytes // (4 n_labels) rows, so a canvas of noise does not ask for gigabytes."""
    labels = _checked(labels, connectivity)
    _cleanup_args(min_area, n_labels, vote_bytes)
    rounds = 0
    for _ in range(int(max_rounds)):
        rounds += 1
        labels, changed = cleanup_round(labels, min_area, n_labels, connectivity, vote_bytes)
        if changed == 0:
            break
    return labels, rounds


def clean_label_maps(maps, min_area, n_labels, connectivity=4):
    """What segment(), the demo and evaluate() apply: merge_small_regions on [B, H, W] (or one [H, W]) label maps -> the cleaned maps."""
    if maps.dim() == 2:
        return merge_small_regions(maps.unsqueeze(0).contiguous(), min_area, n_labels, connectivity)[0][0]
    return merge_small_regions(maps.contiguous(), min_area, n_labels, connectivity)[0]


# ---- files
def regions_to_json(table, b, height, width, connectivity, class_of=None, id_map=None):
    """Image b of `table` as a plain dict: {"height", "width", "connectivity", "regions": [{"id", "label", "class", "area",
    "bbox": [x0, y0, x1, y1], "centroid": [x, y], "first": [x, y]}]}.  "class" is class_of[label] with a cluster -> class assignment
    (None without one, or for a label it does not cover); "id_map", when given, names the file that holds the image's id map."""
    rows = table.rows(b)
    cols = {name: getattr(table, name)[rows].cpu().tolist() for name in RegionTable.COLUMNS}
    if class_of is not None:
        class_of = [int(c) for c in (class_of.cpu().tolist() if torch.is_tensor(class_of) else class_of)]
    regions = []
    for i in range(table.n_regions[b]):
        label, area = cols["label"][i], cols["area"][i]
        regions.append({"id": i, "label": label,
                        "class": class_of[label] if class_of is not None and 0 <= label < len(class_of) else None,
                        "area": area, "bbox": [cols["x0"][i], cols["y0"][i], cols["x1"][i], cols["y1"][i]],
                        "centroid": [cols["sum_x"][i] / area, cols["sum_y"][i] / area],
                        "first": [cols["first"][i] % int(width), cols["first"][i] // int(width)]})
    out = {"height": int(height), "width": int(width), "connectivity": int(connectivity), "regions": regions}
    if id_map is not None:
        out["id_map"] = str(id_map)
    return out


def write_regions(path, table, b, height, width, connectivity, class_of=None, id_map=None):
    """regions_to_json as a JSON file."""
    with open(path, "w") as f:
        json.dump(regions_to_json(table, b, height, width, connectivity, class_of, id_map), f)
    return path


def write_id_map(stem, ids, n_regions):
    """One image's id map (int32 [H, W], numpy or tensor) -> `stem`.png, a 16-bit PNG (PIL mode "I;16", 65535 where a pixel has no
    region), when it has fewer than 65536 regions, else `stem`.npy as int32.  Returns the path written."""
    ids = ids.cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
    if int(n_regions) < 65536:
        from PIL import Image
        path = stem + ".png"
        Image.fromarray(np.where(ids < 0, NO_REGION_U16, ids).astype(np.uint16)).save(path)
        return path
    path = stem + ".npy"
    np.save(path, ids.astype(np.int32))
    return path


def read_id_map(path):
    """What write_id_map wrote -> int32 [H, W], -1 where a pixel has no region."""
    if path.endswith(".npy"):
        return np.load(path).astype(np.int32)
    from PIL import Image
    with Image.open(path) as im:
        ids = np.array(im).astype(np.int32)
    return np.where(ids == NO_REGION_U16, -1, ids).astype(np.int32)
