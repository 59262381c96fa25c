"""Inputs, descriptors and the yardstick shared by tests/test_crf_params_host.py and tests/test_crf_params_gpu.py.  Test helper only.

The yardstick: for one image, q64 = the float64 oracle, q32 = the float32 oracle (tests/crf_oracle.py, one lattice construction for
both), e32 = max|q32 - q64|.  A float32 evaluation q of the same mean-field passes when max|q - q64| <= 4 e32 + 1e-6 and its argmax
is q64's except at near-ties of q64 (top-2 gap <= twice that bar), at most 0.5 % of the pixels.  The bar comes from the reference
alone: the kernels and the float32 oracle are two float32 evaluations that differ in summation order (the splat sums pieces of 64
records four at a time, the blur sums the pieces) and in expf / logf against numpy's; e32 is one draw of the largest rounding error
over H W C values, the kernels' error another.  4 is the 2 - 3 x of the project's GEMM yardsticks, widened because the mean-field
multiplies the spread; 1e-6 is a floor for a Q in [0, 1]."""
import functools

import numpy as np

import crf_oracle as O

F32 = np.float32
FACTOR, FLOOR, MAX_EXCEPTED = 4.0, 1e-6, 0.005

#        name         pos_w  pos_xy_std  bi_w  bi_xy_std  bi_rgb_std
ROWS = {"default":   (3.0,   1.0,        4.0,  67.0,      3.0),
        "wide_pos":  (3.0,   2.5,        4.0,  67.0,      3.0),
        "tight_xy":  (3.0,   1.0,        4.0,  9.0,       3.0),
        "loose_rgb": (3.0,   1.0,        4.0,  67.0,      20.0),
        "tight_rgb": (3.0,   1.0,        4.0,  67.0,      0.9),
        "neg_w":     (-1.5,  1.0,        6.0,  30.0,      8.0),
        "pos_only":  (3.0,   0.7,        0.0,  67.0,      3.0),
        "bi_only":   (0.0,   1.0,        4.0,  67.0,      3.0)}
TABLE_SHAPES = [(23, 31, 5), (37, 53, 27)]        # group widths 2 and 8
TABLE_SEED = 0


def softmax_probs(rng, C, H, W, sharp=3.0):
    lg = rng.standard_normal((C, H, W)).astype(F32) * F32(sharp)
    e = np.exp(lg - lg.max(0, keepdims=True))
    return (e / e.sum(0, keepdims=True)).astype(F32)


def noise_image(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def blocks_image(rng, H, W):
    """Gradients plus flat blocks: long runs of equal and of slowly varying colours, unlike per-pixel noise."""
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    img = np.stack([xx * 255 / max(W - 1, 1), yy * 255 / max(H - 1, 1), np.full_like(xx, 128)], -1)
    for _ in range(5):
        y0, x0 = rng.integers(0, max(H - H // 4, 1)), rng.integers(0, max(W - W // 4, 1))
        h, w = rng.integers(max(H // 8, 1), max(H // 3, 2)), rng.integers(max(W // 8, 1), max(W // 3, 2))
        img[y0:y0 + h, x0:x0 + w] = rng.integers(0, 256, 3)
    return img.astype(np.uint8)


def corner_image(rng, H, W):
    """Colours over {0, 255} only, the corners at (0,0,0), (255,255,255), (255,0,0) and (0,0,255): the extremes of every lattice
    coordinate at the extremes of the position."""
    img = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    img[0, 0], img[0, -1], img[-1, 0], img[-1, -1] = (0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255)
    return img


def inputs(kind, H, W, C, seed, sharp=3.0):
    """(bgr uint8 [H, W, 3], probs float32 [C, H, W]) of one image."""
    rng = np.random.default_rng([seed, H, W, C, {"noise": 0, "blocks": 1, "corner": 2}[kind]])
    img = {"noise": noise_image, "blocks": blocks_image, "corner": corner_image}[kind](rng, H, W)
    return img, softmax_probs(rng, C, H, W, sharp)


@functools.lru_cache(maxsize=None)
def table_inputs(H, W, C):
    """The two images of a parameter-table shape as one batch: (bgr [2, H, W, 3], probs [2, C, H, W]), noise then blocks."""
    pairs = [inputs(kind, H, W, C, TABLE_SEED) for kind in ("noise", "blocks")]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def lattices(bgr, pos_xy_std, bi_xy_std, bi_rgb_std):
    H, W, _ = bgr.shape
    return O.Lattice(O.gaussian_features(H, W, pos_xy_std)), O.Lattice(O.bilateral_features(bgr, bi_xy_std, bi_rgb_std))


class Ref:
    """q64, q32, e32 and the bar of one image under one descriptor; the lattices for the key comparison."""

    def __init__(self, bgr, probs, n_iter, params):
        pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std = params
        self.lat = lattices(bgr, pos_xy_std, bi_xy_std, bi_rgb_std)
        kw = dict(n_iter=n_iter, pos_w=pos_w, pos_xy_std=pos_xy_std, bi_w=bi_w, bi_xy_std=bi_xy_std, bi_rgb_std=bi_rgb_std,
                  lattices=self.lat)
        self.q64 = O.dense_crf(bgr, probs, dtype=np.float64, **kw)
        self.q32 = O.dense_crf(bgr, probs, **kw)
        assert self.q64.dtype == np.float64 and self.q32.dtype == F32
        self.e32 = float(np.abs(self.q32 - self.q64).max())
        self.bar = FACTOR * self.e32 + FLOOR

    def excepted(self, q):
        """Pixels where q's argmax is not q64's; asserts that each is a near-tie of q64.  -> their fraction."""
        a, r = q.argmax(0), self.q64.argmax(0)
        if self.q64.shape[0] == 1:
            return 0.0
        srt = np.sort(self.q64, 0)
        gap = (srt[-1] - srt[-2])[a != r]
        assert (gap <= 2 * self.bar).all(), (gap.max(), self.bar)
        return float((a != r).mean())

    def check(self, q, what=""):
        """The bar and the argmax rule for q [C, H, W]; prints and returns err / e32."""
        assert q.shape == self.q64.shape and np.isfinite(q).all(), what
        err = float(np.abs(q.astype(np.float64) - self.q64).max())
        ratio = err / self.e32 if self.e32 > 0 else (0.0 if err == 0 else float("inf"))
        print("[crf %s] err %.3e  e32 %.3e  err/e32 %.2f  bar %.3e" % (what, err, self.e32, ratio, self.bar))
        assert err <= self.bar, (what, err, self.e32, self.bar)
        frac = self.excepted(q)
        assert frac <= MAX_EXCEPTED, (what, frac)
        return ratio


@functools.lru_cache(maxsize=None)
def table_ref(row, H, W, C, n_iter, b):
    bgr, probs = table_inputs(H, W, C)
    return Ref(bgr[b], probs[b], n_iter, ROWS[row])


# ---- the last descriptors the host-side range check accepts
STD_FIELDS = ("pos_xy_std", "bi_xy_std", "bi_rgb_std")
DEFAULT_STD = {"pos_xy_std": O.POS_XY_STD, "bi_xy_std": O.Bi_XY_STD, "bi_rgb_std": O.Bi_RGB_STD}


def _f32_bits(x):
    return int(np.array(x, F32).view(np.int32))


def _bits_f32(b):
    return float(np.array(b, np.int32).view(F32))


def range_desc(H, W, field, value, C=3, n_iter=2, B=1):
    from stego_amd import capi
    std = dict(DEFAULT_STD)
    std[field] = value
    return capi.crf_desc(B, C, H, W, n_iter, O.POS_W, std["pos_xy_std"], O.Bi_W, std["bi_xy_std"], std["bi_rgb_std"])


@functools.lru_cache(maxsize=None)
def smallest_accepted(H, W, field):
    """Bisection over the float32 values (positive floats order as their bit patterns): (the smallest `field` that
    stego_crf_workspace_bytes accepts for H x W with the other two stds at their defaults, the float32 just below it)."""
    from stego_amd import capi
    ok = lambda bits: capi.crf_workspace_bytes(range_desc(H, W, field, _bits_f32(bits))) > 0
    lo, hi = _f32_bits(1e-30), _f32_bits(DEFAULT_STD[field])
    assert not ok(lo) and ok(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            hi = mid
        else:
            lo = mid
    return _bits_f32(hi), _bits_f32(lo)


def range_params(H, W, field):
    std = dict(DEFAULT_STD)
    std[field] = smallest_accepted(H, W, field)[0]
    return (O.POS_W, std["pos_xy_std"], O.Bi_W, std["bi_xy_std"], std["bi_rgb_std"])
