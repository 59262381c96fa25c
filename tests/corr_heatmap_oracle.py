"""CPU oracle of the query-point correspondence heatmaps (include/stego_heat.h)  --  TEST INFRASTRUCTURE ONLY.

A float64 numpy restatement of the reference's src/plot_dino_correspondence.py:39-58 (get_heatmaps) with a real batch dimension:
    s    = sample(feats1, q)                        modules.py:287: grid_sample, bilinear, border padding, align_corners=True
    attn = einsum("nchw,ncij->nhwij", F.normalize(s, dim=1), F.normalize(feats_t, dim=1))          eps = 1e-12
    attn -= attn.mean([3, 4], keepdims=True);  attn = attn.clamp(0)
    heat = F.interpolate(attn, (H, W), mode="bilinear", align_corners=True)
plus the two flags of the C ABI (no centring, no clamp), `peak` / `best` and the top-2 gap the GPU tests use to decide which `best`
can be compared.  Nothing here imports the package under test."""
import numpy as np

EPS = 1e-12


def sample(feats, points):
    """feats [B, C, h, w], points [B, N, 2] as (x, y) -> [B, N, C]: bilinear, border-clamped, align_corners=True."""
    feats, points = np.asarray(feats, dtype=np.float64), np.asarray(points, dtype=np.float64)
    B, C, h, w = feats.shape
    ix = np.clip((points[..., 0] + 1.0) * 0.5 * (w - 1), 0.0, w - 1)
    iy = np.clip((points[..., 1] + 1.0) * 0.5 * (h - 1), 0.0, h - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = ix - x0, iy - y0
    b = np.arange(B)[:, None]
    f = feats.transpose(0, 2, 3, 1)                                   # [B, h, w, C]
    return (f[b, y0, x0] * ((1 - fx) * (1 - fy))[..., None] + f[b, y0, x1] * (fx * (1 - fy))[..., None]
            + f[b, y1, x0] * ((1 - fx) * fy)[..., None] + f[b, y1, x1] * (fx * fy)[..., None])


def normalize(v, axis):
    return v / np.maximum(np.sqrt((v * v).sum(axis, keepdims=True)), EPS)


def low_res(src, tgt, points, index_t=None, center=True, clamp=True):
    """-> (a [B, N, h, w]: the centred / clamped map, r: the raw cosines)."""
    tgt = np.asarray(tgt, dtype=np.float64)
    if index_t is not None:
        tgt = tgt[np.clip(np.asarray(index_t), 0, tgt.shape[0] - 1)]
    r = np.einsum("bnc,bcij->bnij", normalize(sample(src, points), 2), normalize(tgt, 1))
    a = r - r.mean((2, 3), keepdims=True) if center else r.copy()
    if clamp:
        a = np.maximum(a, 0.0)
    return a, r


def _axis(n_in, n_out):
    """align_corners=True: source index i0, its neighbour i1 and the weight of i1 for every output index (scale 0 for n_out == 1)."""
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    pos = scale * np.arange(n_out, dtype=np.float64)
    i0 = np.minimum(np.floor(pos).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, pos - i0


def upsample(a, size):
    """F.interpolate(a, size, mode="bilinear", align_corners=True) on the last two axes."""
    a = np.asarray(a, dtype=np.float64)
    H, W = size
    if (H, W) == a.shape[-2:]:
        return a.copy()                                               # every weight is exactly 0 or 1
    y0, y1, ly = _axis(a.shape[-2], H)
    x0, x1, lx = _axis(a.shape[-1], W)
    top = a[..., y0, :][..., x0] * (1 - lx) + a[..., y0, :][..., x1] * lx
    bot = a[..., y1, :][..., x0] * (1 - lx) + a[..., y1, :][..., x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def heatmaps(src, tgt, points, size, index_t=None, center=True, clamp=True):
    """-> dict(heat [B, N, H, W], low [B, N, h, w], raw, peak [B, N], best [B, N, 2] as (x, y), cell [B, N], gap [B, N]: the
    difference between the two largest values of `low` (inf for a one-cell map))."""
    a, r = low_res(src, tgt, points, index_t, center, clamp)
    B, N, h, w = a.shape
    flat = a.reshape(B, N, h * w)
    cell = flat.argmax(2)                                             # the first maximum in row-major order
    peak = np.take_along_axis(flat, cell[..., None], 2)[..., 0]
    if h * w > 1:
        top2 = np.sort(flat, axis=2)[..., -2:]
        gap = top2[..., 1] - top2[..., 0]
    else:
        gap = np.full((B, N), np.inf)
    cx, cy = cell % w, cell // w
    best = np.stack([2.0 * cx / (w - 1) - 1.0 if w > 1 else np.zeros_like(cx, dtype=np.float64),
                     2.0 * cy / (h - 1) - 1.0 if h > 1 else np.zeros_like(cy, dtype=np.float64)], -1)
    return dict(heat=upsample(a, size), low=a, raw=r, peak=peak, best=best, cell=cell, gap=gap)
