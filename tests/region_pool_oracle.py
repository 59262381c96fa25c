"""A plain oracle of the region descriptors (INTEGRATION.md "Region descriptors"), written from the definitions and sharing nothing with
stego_amd/region_descriptors.py: the taps as tests/feature_pca_oracle._taps computes them (float32 source index, float64 everything
after), the sums with np.add.at in float64 and no quantisation - and an exact integer version that evaluates the pixel value in float32
as the header writes it, quantises and sums in Python integers: that one is what the bitwise cases are checked against."""
import numpy as np

from feature_pca_oracle import _taps


def rows_of(ids, row_offset):
    """ids int [B, H, W], row_offset [B] -> the table row of every pixel, -1 where there is no region."""
    ids = np.asarray(ids).astype(np.int64)
    off = np.asarray(row_offset, dtype=np.int64)[:, None, None]
    return np.where(ids >= 0, ids + off, -1)


def pixel_values(maps, H, W):
    """maps [B, C, h, w] -> v float64 [B, H, W, C]."""
    m = np.asarray(maps).astype(np.float64)
    y0, y1, ly = _taps(H, m.shape[2])
    x0, x1, lx = _taps(W, m.shape[3])
    ly, lx = ly[None, None, :, None], lx[None, None, None, :]
    top = (1 - lx) * m[:, :, y0][:, :, :, x0] + lx * m[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * m[:, :, y1][:, :, :, x0] + lx * m[:, :, y1][:, :, :, x1]
    return np.transpose((1 - ly) * top + ly * bot, (0, 2, 3, 1))


def descriptors(maps, ids, row_offset, area, lo=0, hi=None):
    """float64 [hi - lo, C]: the means, no quantisation; 0 where area <= 0."""
    area = np.asarray(area).astype(np.int64)
    hi = len(area) if hi is None else hi
    rows = rows_of(ids, row_offset)
    v = pixel_values(maps, ids.shape[1], ids.shape[2])
    sums = np.zeros((hi - lo, v.shape[-1]), dtype=np.float64)
    keep = (rows >= lo) & (rows < hi)
    np.add.at(sums, rows[keep] - lo, v[keep])
    a = area[lo:hi, None].astype(np.float64)
    return np.where(a > 0, sums / np.maximum(a, 1), 0.0)


def shift_of(maps):
    """s = 30 - e with 2^(e-1) <= M < 2^e (e = -126 for a subnormal M); None for M == 0."""
    M = float(np.abs(np.asarray(maps, dtype=np.float32)).max())
    if M == 0:
        return None
    e = max(int(np.floor(np.log2(M))) + 1, -126)
    assert M < 2.0 ** e and (e == -126 or 2.0 ** (e - 1) <= M)
    return 30 - e


def _fma32(a, b, c):
    """float32 fused multiply-add: the product of two float32 is exact in float64, and for the operands of these tests the float64 sum
    is exact as well or rounds the same way twice; the exact cases do not depend on it at all (every intermediate is exact there)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def quantised(maps, H, W):
    """q int64 [B, H, W, C] as the header defines it (float32 pixel value, rint(v * 2^s)), and s; (zeros, None) for an all-zero map."""
    m = np.asarray(maps, dtype=np.float32)
    s = shift_of(m)
    if s is None:
        return np.zeros((m.shape[0], H, W, m.shape[1]), dtype=np.int64), None
    y0, y1, ly = _taps(H, m.shape[2])
    x0, x1, lx = _taps(W, m.shape[3])
    h1, w1 = ly.astype(np.float32)[None, None, :, None], lx.astype(np.float32)[None, None, None, :]
    h0, w0 = np.float32(1) - h1, np.float32(1) - w1
    a, b = m[:, :, y0][:, :, :, x0], m[:, :, y0][:, :, :, x1]
    c, d = m[:, :, y1][:, :, :, x0], m[:, :, y1][:, :, :, x1]
    v = _fma32(h0, _fma32(w0, a, w1 * b), h1 * _fma32(w0, c, w1 * d))
    q = np.rint(np.ldexp(v.astype(np.float64), s)).astype(np.int64)
    return np.transpose(q, (0, 2, 3, 1)), s


def descriptors_exact(maps, ids, row_offset, area, lo=0, hi=None):
    """float32 [hi - lo, C]: float32((double) S * 2^-s / area) with S summed in Python integers."""
    area = np.asarray(area).astype(np.int64)
    hi = len(area) if hi is None else hi
    q, s = quantised(maps, ids.shape[1], ids.shape[2])
    rows = rows_of(ids, row_offset)
    S = np.zeros((hi - lo, q.shape[-1]), dtype=object)
    S[:] = 0
    keep = (rows >= lo) & (rows < hi)
    for r, qs in zip(rows[keep] - lo, q[keep]):
        S[r] = S[r] + qs.astype(object)
    out = np.zeros(S.shape, dtype=np.float32)
    if s is None:
        return out
    for r in range(hi - lo):
        if area[lo + r] > 0:
            out[r] = [np.float32(np.ldexp(float(int(v)), -s) / float(area[lo + r])) for v in S[r]]
    return out


def table_of(ids):
    """ids int [B, H, W] with ids 0 .. n - 1 per image -> (row_offset int64 [B], area int64 [R])."""
    ids = np.asarray(ids)
    counts = [int(i.max()) + 1 if (i >= 0).any() else 0 for i in ids]
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    area = np.zeros(sum(counts), dtype=np.int64)
    rows = rows_of(ids, offs)
    np.add.at(area, rows[rows >= 0], 1)
    return offs, area
