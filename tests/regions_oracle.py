"""A plain oracle of the region definitions (INTEGRATION.md "Regions"), written from the definitions with explicit loops and nothing
shared with stego_amd/regions.py: a union-find over the pixels, the table, one cleanup round and the loop over rounds.  Slow on
purpose; the tests keep their maps small.  The pattern generators the host and GPU tests share are at the end."""
import numpy as np

COLUMNS = ("label", "area", "y0", "x0", "y1", "x1", "first", "sum_y", "sum_x")


def _neighbours(connectivity):
    if connectivity == 4:
        return ((0, -1), (-1, 0))
    assert connectivity == 8
    return ((0, -1), (-1, 0), (-1, -1), (-1, 1))


def label(lab, connectivity=4):
    """One image, integer [H, W] -> (ids int32 [H, W], n): union-find with the smaller raster index as the root, numbered by it."""
    lab = np.asarray(lab).astype(np.int64)
    H, W = lab.shape
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for y in range(H):
        for x in range(W):
            if lab[y, x] < 0:
                continue
            for dy, dx in _neighbours(connectivity):
                qy, qx = y + dy, x + dx
                if 0 <= qy < H and 0 <= qx < W and lab[qy, qx] == lab[y, x]:
                    a, b = find(y * W + x), find(qy * W + qx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)
    ids = np.full((H, W), -1, dtype=np.int32)
    number = {}
    for i in range(H * W):                           # raster order: a root is met before every other pixel of its region
        y, x = divmod(i, W)
        if lab[y, x] < 0:
            continue
        r = find(i)
        if r not in number:
            assert r == i
            number[r] = len(number)
        ids[y, x] = number[r]
    return ids, len(number)


def table(lab, ids, n):
    """-> {column: int64 [n]} of one image."""
    lab = np.asarray(lab).astype(np.int64)
    H, W = lab.shape
    t = {c: np.zeros(n, dtype=np.int64) for c in COLUMNS}
    seen = np.zeros(n, dtype=bool)
    for y in range(H):
        for x in range(W):
            r = ids[y, x]
            if r < 0:
                continue
            if not seen[r]:
                seen[r] = True
                t["label"][r], t["first"][r] = lab[y, x], y * W + x
                t["y0"][r], t["x0"][r], t["y1"][r], t["x1"][r] = y, x, y, x
            t["area"][r] += 1
            t["y0"][r], t["x0"][r] = min(t["y0"][r], y), min(t["x0"][r], x)
            t["y1"][r], t["x1"][r] = max(t["y1"][r], y), max(t["x1"][r], x)
            t["sum_y"][r] += y
            t["sum_x"][r] += x
    return t


def cleanup_round(lab, min_area, n_labels, connectivity=4):
    """One round on one image -> (the new map in the input's dtype, the number of regions whose label changed)."""
    src = np.asarray(lab)
    lab = src.astype(np.int64)
    H, W = lab.shape
    ids, n = label(lab, connectivity)
    t = table(lab, ids, n)
    small = t["area"] < min_area
    votes = np.zeros((n, n_labels), dtype=np.int64)
    for y in range(H):
        for x in range(W):
            r = ids[y, x]
            if r < 0 or not small[r]:
                continue
            for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
                qy, qx = y + dy, x + dx
                if not (0 <= qy < H and 0 <= qx < W):
                    continue
                q = ids[qy, qx]
                if q < 0 or small[q] or lab[qy, qx] >= n_labels:
                    continue
                votes[r, lab[qy, qx]] += 1
    new_label = t["label"].copy()
    for r in range(n):
        if not small[r]:
            continue
        best, cls = 0, -1
        for c in range(n_labels):
            if votes[r, c] > best:
                best, cls = votes[r, c], c
        if cls >= 0:
            new_label[r] = cls
    out = lab.copy()
    for y in range(H):
        for x in range(W):
            if ids[y, x] >= 0:
                out[y, x] = new_label[ids[y, x]]
    return out.astype(src.dtype), int((new_label != t["label"]).sum())


def merge(lab, min_area, n_labels, connectivity=4, max_rounds=4):
    """-> (the cleaned map of one image, the rounds run: the round that changed nothing counts)."""
    rounds = 0
    for _ in range(max_rounds):
        rounds += 1
        lab, changed = cleanup_round(lab, min_area, n_labels, connectivity)
        if changed == 0:
            break
    return lab, rounds


def merge_batch(labs, min_area, n_labels, connectivity=4, max_rounds=4):
    """A batch [B, H, W]: a round runs on every image, and the loop ends when no image changed -> (maps, rounds)."""
    labs = np.asarray(labs).copy()
    rounds = 0
    for _ in range(max_rounds):
        rounds += 1
        total = 0
        for b in range(labs.shape[0]):
            labs[b], changed = cleanup_round(labs[b], min_area, n_labels, connectivity)
            total += changed
        if total == 0:
            break
    return labs, rounds


def region_dicts(lab, connectivity=4, class_of=None):
    """The "regions" list of the JSON format for one image."""
    ids, n = label(lab, connectivity)
    t = table(lab, ids, n)
    W = np.asarray(lab).shape[1]
    out = []
    for r in range(n):
        lb = int(t["label"][r])
        out.append({"id": r, "label": lb, "class": int(class_of[lb]) if class_of is not None and 0 <= lb < len(class_of) else None,
                    "area": int(t["area"][r]), "bbox": [int(t["x0"][r]), int(t["y0"][r]), int(t["x1"][r]), int(t["y1"][r])],
                    "centroid": [int(t["sum_x"][r]) / int(t["area"][r]), int(t["sum_y"][r]) / int(t["area"][r])],
                    "first": [int(t["first"][r]) % W, int(t["first"][r]) // W]})
    return out


# ---- patterns: (H, W) -> int64 [H, W]
def uniform(H, W):
    return np.full((H, W), 3, dtype=np.int64)


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return ((y + x) & 1).astype(np.int64)


def spiral(H, W):
    """A one-pixel corridor of label 1 winding inwards over the whole image, a wall of label 0 between its turns: walk ahead while the
    next cell is free and the one behind it is not corridor yet, else turn right; two turns in a row end it."""
    m = np.zeros((H, W), dtype=np.int64)
    y, x, dy, dx, turns = 0, 0, 0, 1, 0
    m[0, 0] = 1

    def inside(yy, xx):
        return 0 <= yy < H and 0 <= xx < W

    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and m[ny, nx] == 0 and not (inside(ay, ax) and m[ay, ax] == 1):
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m


def comb(H, W):
    """Teeth of label 1 in every other column, joined only by the last row; the first pixel is the top of the first tooth."""
    m = np.zeros((H, W), dtype=np.int64)
    m[:, ::2] = 1
    m[H - 1, :] = 1
    return m


def rings(H, W):
    y, x = np.mgrid[0:H, 0:W]
    d = np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x))
    return (d % 3).astype(np.int64)


def u_shape(H, W):
    """Two arms of label 2 that start in the first row, far apart, and meet in the last row."""
    m = np.zeros((H, W), dtype=np.int64)
    m[:, 0] = 2
    m[:, W - 1] = 2
    m[H - 1, :] = 2
    return m


def random_map(H, W, classes, seed):
    return np.random.default_rng(seed).integers(0, classes, (H, W)).astype(np.int64)


def with_negatives(H, W, seed):
    m = random_map(H, W, 3, seed)
    m[np.random.default_rng(seed + 1).random((H, W)) < 0.3] = -1
    return m


def blocky(H, W, classes=5, block=12, speckle=0.08, seed=0):
    """Square blocks of `block` pixels with random classes, a share `speckle` of the pixels redrawn."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, classes, ((H + block - 1) // block, (W + block - 1) // block))
    m = np.kron(coarse, np.ones((block, block), dtype=np.int64))[:H, :W].astype(np.int64)
    noise = rng.random((H, W)) < speckle
    m[noise] = rng.integers(0, classes, int(noise.sum()))
    return m


PATTERNS = {"uniform": uniform, "checkerboard": checkerboard, "spiral": spiral, "comb": comb, "rings": rings, "u": u_shape,
            "random2": lambda H, W: random_map(H, W, 2, 2), "random3": lambda H, W: random_map(H, W, 3, 3),
            "random27": lambda H, W: random_map(H, W, 27, 27), "negatives": lambda H, W: with_negatives(H, W, 5)}
