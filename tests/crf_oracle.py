"""Numpy restatement of the fully-connected CRF the reference evaluates with (src/crf.py:22-45, pydensecrf's DenseCRF2D): the
permutohedral lattice of Adams, Baek & Davis (2010) in the form densecrf builds it, the symmetric normalisation and the mean-field
loop.  Test helper only: the product (stego_amd/crf.py + csrc/dense_crf.hip) never imports it.

Vectorised over pixels; np.unique / searchsorted stand in for densecrf's hash table.  The embedding runs in float32 in densecrf's
operation order (integer remainders are cast to float32 before they meet floats: numpy would otherwise promote to float64), so its
keys, vertex counts and barycentric weights are the ones csrc/dense_crf.hip computes, bit for bit.  The filtering sums differ from
the kernels' only in their order.

dtype=np.float64 on Lattice.filter / norm, softmax and dense_crf is the yardstick of the GPU tests: the embedding (keys, ranks,
barycentric weights: geometry densecrf defines in float) stays in float32, everything after it - log(clip(p)), the s * Q products,
splat, blur, slice, 1 / sqrt(L(1) + 1e-20), the weighted sum, exp and the division of the softmax - runs in float64 on the same
float32 inputs and constants.  With the default, np.float32, every result is bitwise what it was before the argument existed."""
import numpy as np

F32 = np.float32

MAX_ITER, POS_W, POS_XY_STD, Bi_W, Bi_XY_STD, Bi_RGB_STD = 10, 3.0, 1.0, 4.0, 67.0, 3.0


def key_bits(d):
    """Bits per stored coordinate of a packed 64-bit key (include/stego_crf.h)."""
    return 32 if d <= 2 else 12


def scale_factors(d):
    """densecrf: inv_std_dev = float(sqrt(2/3) * (d + 1)); scale[i] = float(1 / sqrt((i + 1)(i + 2)) * inv_std_dev)."""
    inv = float(F32(np.sqrt(2.0 / 3.0) * (d + 1)))
    return np.array([1.0 / np.sqrt(float((i + 1) * (i + 2))) * inv for i in range(d)], dtype=F32)


def gaussian_features(H, W, sxy):
    ys, xs = np.meshgrid(np.arange(H, dtype=F32), np.arange(W, dtype=F32), indexing="ij")
    s = F32(sxy)
    return np.stack([xs.reshape(-1) / s, ys.reshape(-1) / s], 1).astype(F32)


def bilateral_features(bgr, sxy, srgb):
    """(x/sxy, y/sxy, B/srgb, G/srgb, R/srgb) per pixel, k = y*W + x (DenseCRF2D::addPairwiseBilateral)."""
    H, W, _ = bgr.shape
    pos = gaussian_features(H, W, sxy)
    col = bgr.reshape(-1, 3).astype(F32) / F32(srgb)
    return np.concatenate([pos, col], 1).astype(F32)


def embed(f):
    """f float32 [N, d] -> (keys int64 [N, d+1, d], bary float32 [N, d+1])."""
    f = np.asarray(f, dtype=F32)
    N, d = f.shape
    sc = scale_factors(d)
    el = np.zeros((N, d + 1), F32)
    sm = np.zeros(N, F32)
    for j in range(d, 0, -1):
        cf = f[:, j - 1] * sc[j - 1]
        el[:, j] = sm - F32(j) * cf
        sm = sm + cf
    el[:, 0] = sm
    down = F32(1.0) / F32(d + 1)
    up = F32(d + 1)
    v = down * el
    hi = np.ceil(v) * up
    lo = np.floor(v) * up
    rem0 = np.where(hi - el < el - lo, hi, lo).astype(np.int64)         # nearest multiple of d+1, a tie goes down
    s = rem0.sum(1) // (d + 1)
    rank = np.zeros((N, d + 1), np.int64)
    for i in range(d):
        di = el[:, i] - rem0[:, i].astype(F32)
        for j in range(i + 1, d + 1):
            lt = di < (el[:, j] - rem0[:, j].astype(F32))
            rank[:, i] += lt
            rank[:, j] += ~lt
    rank += s[:, None]
    neg = rank < 0
    rank[neg] += d + 1
    rem0[neg] += d + 1
    pos = rank > d
    rank[pos] -= d + 1
    rem0[pos] -= d + 1
    b = np.zeros((N, d + 2), F32)
    ar = np.arange(N)
    for i in range(d + 1):
        v = (el[:, i] - rem0[:, i].astype(F32)) * down
        b[ar, d - rank[:, i]] += v
        b[ar, d - rank[:, i] + 1] -= v
    b[:, 0] = (b[:, 0].astype(np.float64) + (1.0 + b[:, d + 1].astype(np.float64))).astype(F32)   # densecrf: float += 1.0 (a double)
    canon = np.array([[r if k <= d - r else r - (d + 1) for k in range(d + 1)] for r in range(d + 1)], np.int64)
    keys = rem0[:, None, :d] + canon[:, rank[:, :d]].transpose(1, 0, 2)     # [N, r, i] = rem0[i] + canonical[r][rank[i]]
    return keys, b[:, :d + 1]


def pack(keys, d):
    """int coordinates [..., d] -> uint64 key: coordinate i + 2^(bits-1) in bits [i*bits, (i+1)*bits)."""
    bits = key_bits(d)
    bias = 1 << (bits - 1)
    k = np.asarray(keys, np.int64) + bias
    assert (k >= 0).all() and (k < (1 << bits)).all(), "lattice coordinate out of the packed range"
    out = np.zeros(k.shape[:-1], np.uint64)
    for i in range(d):
        out |= k[..., i].astype(np.uint64) << np.uint64(i * bits)
    return out


def unpack(packed, d):
    bits = key_bits(d)
    mask = np.uint64((1 << bits) - 1)
    return np.stack([((packed >> np.uint64(i * bits)) & mask).astype(np.int64) - (1 << (bits - 1)) for i in range(d)], -1)


class Lattice:
    """Unique vertices (ascending packed key: the order of the kernels' sort), entry -> vertex map, blur neighbours."""

    def __init__(self, f):
        f = np.asarray(f, F32)
        self.N, self.d = f.shape
        d = self.d
        keys, self.bary = embed(f)
        packed = pack(keys, d).reshape(-1)                       # entry e = pixel * (d+1) + r
        self.keys, self.vid = np.unique(packed, return_inverse=True)
        self.vid = self.vid.reshape(self.N, d + 1)
        self.M = len(self.keys)
        order = np.argsort(self.vid.reshape(-1), kind="stable")  # CSR: each vertex's entries in pixel order
        self.order = order
        self.seg = np.searchsorted(self.vid.reshape(-1)[order], np.arange(self.M))
        self.reverse = False                                     # True: the splat sums each vertex's entries last pixel first
        self.nbr = [(self._find(n1), self._find(n2)) for n1, n2 in self.neighbour_coords()]

    def neighbour_coords(self):
        """Per blur pass j = 0 .. d: the integer coordinates [M, d] of every vertex's two neighbours (n1 = key - 1 with coordinate j
        + d, n2 = key + 1 with coordinate j - d), whether or not a vertex lives there."""
        d = self.d
        coords = unpack(self.keys, d)
        for j in range(d + 1):
            n1, n2 = coords - 1, coords + 1
            if j < d:
                n1[:, j] = coords[:, j] + d
                n2[:, j] = coords[:, j] - d
            yield n1, n2

    def _find(self, c):
        bits = key_bits(self.d)
        ok = ((c >= -(1 << (bits - 1))) & (c < (1 << (bits - 1)))).all(1)
        p = pack(np.where(ok[:, None], c, 0), self.d)
        i = np.minimum(np.searchsorted(self.keys, p), self.M - 1)
        return np.where(ok & (self.keys[i] == p), i, -1).astype(np.int64)

    def filter(self, x, dtype=F32):
        """L(x): splat (barycentric-weighted sums into vertices), d+1 blur passes, slice.  x [N, C], evaluated in `dtype` (the
        barycentric weights are the float32 ones either way)."""
        x = np.asarray(x, dtype)
        d = self.d
        bary = self.bary.astype(dtype, copy=False)
        order = self.order
        if self.reverse:                                            # same segments, each walked backwards: another order of the same sum
            order = order[np.lexsort((-np.arange(len(order)), self.vid.reshape(-1)[order]))]
        flat_w = bary.reshape(-1)[order]
        pix = order // (d + 1)
        v = np.add.reduceat(flat_w[:, None] * x[pix], self.seg, axis=0).astype(dtype)
        z = np.zeros((1, x.shape[1]), dtype)
        for j in range(d + 1):
            p = np.concatenate([v, z], 0)                           # index -1 -> the zero row
            n1, n2 = self.nbr[j]
            v = v + dtype(0.5) * (p[n1] + p[n2])
        out = np.zeros_like(x)
        for r in range(d + 1):
            out += bary[:, r, None] * v[self.vid[:, r]]
        return out

    def norm(self, dtype=F32):
        """s = 1 / sqrt(L(1) + 1e-20) (densecrf NORMALIZE_SYMMETRIC, in double, stored as float; kept in double with float64)."""
        n = self.filter(np.ones((self.N, 1), dtype), dtype)[:, 0]
        return (1.0 / np.sqrt(n.astype(np.float64) + 1e-20)).astype(dtype)


def softmax(x, axis, dtype=F32):
    x = np.asarray(x, dtype)
    e = np.exp(x - x.max(axis, keepdims=True))
    return e / e.sum(axis, keepdims=True)


def dense_crf(bgr, probs, n_iter=MAX_ITER, pos_w=POS_W, pos_xy_std=POS_XY_STD, bi_w=Bi_W, bi_xy_std=Bi_XY_STD, bi_rgb_std=Bi_RGB_STD,
              lattices=None, dtype=F32):
    """bgr uint8 [H, W, 3], probs float32 [C, H, W] -> Q `dtype` [C, H, W] (crf.py:37-45 with pydensecrf).  `lattices`: a prebuilt
    (Gaussian, bilateral) pair, so that a float32 and a float64 evaluation share one construction.  The inputs and constants are the
    float32 ones in either mode (the clip at float(1e-5), the weights as the descriptor stores them)."""
    C, H, W = probs.shape
    T = dtype
    neg_u = np.log(np.clip(np.asarray(probs, F32), F32(1e-5), F32(1.0)).astype(T)).reshape(C, -1).T.astype(T)     # -unary_from_softmax
    lg, lb = lattices or (Lattice(gaussian_features(H, W, pos_xy_std)), Lattice(bilateral_features(bgr, bi_xy_std, bi_rgb_std)))
    sg, sb = lg.norm(T)[:, None], lb.norm(T)[:, None]
    q = softmax(neg_u, 1, T)
    for _ in range(n_iter):
        kg = sg * lg.filter(sg * q, T)
        kb = sb * lb.filter(sb * q, T)
        q = softmax((neg_u + T(F32(pos_w)) * kg) + T(F32(bi_w)) * kb, 1, T)
    return q.T.reshape(C, H, W)


def exact_gaussian_filter(f, x):
    """sum_j exp(-|f_i - f_j|^2 / 2) x_j in float64 (the filter the lattice approximates, up to scale)."""
    f = np.asarray(f, np.float64)
    d2 = ((f[:, None, :] - f[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * d2) @ np.asarray(x, np.float64)


def symmetric(filter_fn, x):
    """s * L(s * x) with s = 1 / sqrt(L(1))."""
    n = filter_fn(np.ones((x.shape[0], 1)))[:, 0]
    s = 1.0 / np.sqrt(np.asarray(n, np.float64) + 1e-20)
    return s[:, None] * np.asarray(filter_fn((s[:, None] * x).astype(F32)), np.float64)


def dense_crf_args(args):
    """dense_crf(*args) with the defaults: a picklable entry for process pools."""
    return dense_crf(*args)
