"""A float64 numpy restatement of the five stages of include/stego_pca.h from the same float32 inputs, the builder of planted maps, and
the byte rule the pictures are compared under.

Planted maps.  Per group X = U diag(s) V^T + offset with U [n, r] orthonormal and orthogonal to the ones vector, V [C, r] orthonormal
and s_i = sqrt((n - 1) lambda_i): the sample covariance is V diag(lambda) V^T exactly (up to the float32 rounding of X), with
lambda = 16, 8, 4 and then 2^(-(i - 3) / 8) for i = 3 .. r - 1 - gaps of a factor two between the leading three, so their vectors are
well conditioned, and lambda_9 / lambda_3 = 0.16, so 32 steps of a subspace iteration on 8 columns reach fp64 round-off.
"""
import numpy as np

DROP = 2.0 ** -20


def spectrum(r):
    lam = np.array([16.0, 8.0, 4.0] + [2.0 ** (-(i - 3) / 8.0) for i in range(3, max(r, 3))])
    return lam[:r]


def planted_map(B, h, w, C, joint, seed=0, offset=0.5, gain=1.0, rank=None):
    """-> float32 [B, h, w, C] (channels last; the caller permutes).  offset: the channel offsets, in units of the map's spread
    sqrt(trace / C); gain: a factor on the whole map; rank: fewer planted components than min(n - 1, C)."""
    rng = np.random.default_rng(seed)
    G, n = (1, B * h * w) if joint else (B, h * w)
    out = np.empty((G, n, C))
    for g in range(G):
        r = min(n - 1, C) if rank is None else rank
        u = rng.standard_normal((n, r))
        u -= u.mean(0, keepdims=True)
        u, _ = np.linalg.qr(u)
        u -= u.mean(0, keepdims=True)                     # (the QR of centred columns stays centred; this removes its round-off)
        v, _ = np.linalg.qr(rng.standard_normal((C, r)))
        lam = spectrum(r)
        x = (u * np.sqrt((n - 1) * lam)) @ v.T
        spread = np.sqrt(lam.sum() / C)
        out[g] = x + offset * spread * rng.standard_normal(C)
    return (gain * out).reshape(B, h, w, C).astype(np.float32)


def tokens(x, joint):
    """float32 [B, C, h, w] -> float64 [G, n, C]."""
    B, C, h, w = x.shape
    t = np.asarray(x, dtype=np.float64).transpose(0, 2, 3, 1).reshape(B, h * w, C)
    return t.reshape(1, B * h * w, C) if joint else t


def fit(x, joint):
    """Stages (a) - (c) -> mean float32 [G, C], cov [G, C, C], basis [G, 3, C], stats [G, 3, 3] (float64; the residual of an exact
    eigenvector is 0)."""
    t = tokens(x, joint)
    G, n, C = t.shape
    mean = (t.sum(1) / n).astype(np.float32)
    xc = t - mean.astype(np.float64)[:, None, :]
    cov = np.einsum("gni,gnj->gij", xc, xc) / (n - 1)
    basis, stats = np.zeros((G, 3, C)), np.zeros((G, 3, 3))
    for g in range(G):
        lam, vec = np.linalg.eigh(cov[g])
        lam, vec = lam[::-1][:3], vec[:, ::-1][:, :3].T
        trace = np.trace(cov[g])
        for i in range(3):
            if not lam[i] > DROP * trace:
                continue
            v = vec[i]
            top = int(np.argmax(np.abs(v)))                # the first of equal maxima: the lowest channel
            basis[g, i] = -v if v[top] < 0 else v
            stats[g, i] = (lam[i], lam[i] / trace, 0.0)
    return mean, cov, basis, stats


def scores(x, mean, basis):
    """Stage (d) under a model (G = 1: every image takes it) -> scores [B, h, w, 3], range [G, 3, 2]."""
    B, C, h, w = x.shape
    G = mean.shape[0]
    t = tokens(x, G == 1)
    s = np.einsum("gnc,gic->gni", t - np.asarray(mean, np.float64)[:, None, :], np.asarray(basis, np.float64))
    rng = np.stack([s.min(1), s.max(1)], -1)
    return s.reshape(B, h, w, 3), rng


def _taps(out, inp):
    """ATen's align_corners=False source index in float32 -> (i0, i1, lambda of i1)."""
    scale = np.float32(inp) / np.float32(out)
    s = scale * (np.arange(out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    s = np.maximum(s, np.float32(0))
    i0 = np.minimum(s.astype(np.int64), inp - 1)
    i1 = i0 + (i0 < inp - 1)
    return i0, i1, (s - i0.astype(np.float32)).astype(np.float64)


def _nearest(out, inp):
    scale = np.float32(inp) / np.float32(out)
    return np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), inp - 1)


def levels(s, rng, size, scale, resize):
    """Stage (e) before the clamp: a = v' * 255 in float64, [B, H, W, 3]."""
    B, h, w, _ = s.shape
    H, W = size
    if resize == "nearest":
        r = s[:, _nearest(H, h)][:, :, _nearest(W, w)]
    else:
        y0, y1, ly = _taps(H, h)
        x0, x1, lx = _taps(W, w)
        ly, lx = ly[None, :, None, None], lx[None, None, :, None]
        top = (1 - lx) * s[:, y0][:, :, x0] + lx * s[:, y0][:, :, x1]
        bot = (1 - lx) * s[:, y1][:, :, x0] + lx * s[:, y1][:, :, x1]
        r = (1 - ly) * top + ly * bot
    if scale == "unit":
        v = (r + 1.0) / 2.0
    else:
        lo, hi = rng[:, None, None, :, 0], rng[:, None, None, :, 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.where(hi > lo, (r - lo) / np.where(hi > lo, hi - lo, 1.0), 0.0)
    return v * 255.0


def to_bytes(a):
    return np.clip(np.nan_to_num(a, nan=0.0), 0, 255).astype(np.uint8)


def pictures(x, joint, size=None, scale="unit", resize="bilinear", model=None):
    """The whole chain -> (bytes uint8 [B, H, W, 3], a)."""
    mean, basis = fit(x, joint)[0::2] if model is None else model
    s, rng = scores(x, mean, basis)
    a = levels(s, rng, tuple(x.shape[-2:]) if size is None else size, scale, resize)
    return to_bytes(a), a


def byte_rule(got, a, strict=True):
    """Every byte within one level of the oracle's; a byte whose a lies 1e-3 or more from an integer equals it (strict).  -> the share of
    bytes that are exempt from equality."""
    got = np.asarray(got).astype(np.int64)
    want = to_bytes(a).astype(np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = np.abs(got - want)
    assert diff.max() <= 1, "a byte is %d levels off" % diff.max()
    a = np.nan_to_num(a, nan=0.0)
    exempt = np.abs(a - np.round(a)) < 1e-3                  # a before the clamp
    if strict:
        bad = (diff != 0) & ~exempt
        assert not bad.any(), "%d bytes differ away from an integer level" % int(bad.sum())
    return float(exempt.mean())
