"""CPU oracle of the label co-occurrence PR histogram (include/stego_pr.h)  --  TEST INFRASTRUCTURE ONLY.

A float64 numpy restatement of the reference's ``get_net_fd`` (src/plot_pr_curves.py:108-121) on top of the already pinned
``oracle.corr_oracle.sample / norm / tensor_correlation``: per pair the score ``fd``, the reference's ``ld`` (float64), the exact
target (from the integer labels: every bilinear tap with a non-zero weight of both points carries one class), the per-tap label
weights, and from them the histogram; plus ``pr_from_hist``, precision / recall / average precision without scikit-learn.

Coordinates are ``[B, S1, S2, 2]``; every result is laid out like ``sample()``'s output: point ``(u, v)`` of a result was sampled at
``coords[b, v, u]`` (the reference's ``coords.permute(0, 2, 1, 3)``).  A flat list of N points is ``[B, N, 1, 2]``.
"""
import numpy as np

from oracle import corr_oracle as O

# A bilinear weight inside the open interval (0, RISKY_WEIGHT): fp32 may pick other taps than float64 there.  The weights meant are
# the four one-dimensional ones (left / right, top / bottom): a tap joins or leaves a point's purity code only where one of them
# crosses 0.  (A tap's weight is a product of two of them; with uniform coordinates a point has such a factor with probability
# 4e-4, a pair with 8e-4.)
RISKY_WEIGHT = 1e-4


def label_taps(labels, coords, n_classes):
    """The four label taps of every point: classes [B, U, V, 4] (0 = unlabeled, l + 1 otherwise: one_hot(label + 1, n_classes + 1))
    and float64 weights [B, U, V, 4] of ATen's grid_sampler_2d (bilinear, border, align_corners=True), U = S2, V = S1; and the
    one-dimensional weights [B, U, V, 4] (left, right, top, bottom) they are products of."""
    labels = np.asarray(labels)
    B, HL, WL = labels.shape
    grid = np.asarray(coords, dtype=np.float64).transpose(0, 2, 1, 3)
    ix = np.minimum(np.maximum((grid[..., 0] + 1) / 2 * (WL - 1), 0), WL - 1)
    iy = np.minimum(np.maximum((grid[..., 1] + 1) / 2 * (HL - 1), 0), HL - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    cls, wts = [], []
    bidx = np.arange(B)[:, None, None]
    for xx, yy, ww in ((x0, y0, (x1 - ix) * (y1 - iy)), (x1, y0, (ix - x0) * (y1 - iy)), (x0, y1, (x1 - ix) * (iy - y0)), (x1, y1, (ix - x0) * (iy - y0))):
        inb = (xx <= WL - 1) & (yy <= HL - 1)
        lab = labels[bidx, np.clip(yy, 0, HL - 1).astype(np.int64), np.clip(xx, 0, WL - 1).astype(np.int64)]
        cls.append(np.where((lab >= 0) & (lab < n_classes), lab + 1, 0))
        wts.append(ww * inb)
    axes = np.stack([x1 - ix, (ix - x0) * (x1 <= WL - 1), y1 - iy, (iy - y0) * (y1 <= HL - 1)], -1)
    return np.stack(cls, -1), np.stack(wts, -1), axes


def purity(cls, wts, axes):
    """Per point: the class all taps with a non-zero weight agree on (-1 if they do not), whether such a tap is unlabeled, and
    whether a one-dimensional weight lies in (0, RISKY_WEIGHT)."""
    on = wts > 0
    hi = np.where(on, cls, -1).max(-1)
    lo = np.where(on, cls, 1 << 30).min(-1)
    code = np.where(hi == lo, hi, -1)
    unlabeled = (on & (cls == 0)).any(-1)
    risky = ((axes > 0) & (axes < RISKY_WEIGHT)).any(-1)
    return code, unlabeled, risky


def one_hot_maps(labels, n_classes, dtype=np.float64):
    """F.one_hot(label + 1, n_classes + 1).permute(0, 3, 1, 2) with everything outside [0, n_classes) in channel 0."""
    labels = np.asarray(labels)
    c = np.where((labels >= 0) & (labels < n_classes), labels + 1, 0)
    return np.moveaxis(np.eye(n_classes + 1, dtype=dtype)[c], -1, 1)


def net_fd(feats1, feats2, label1, label2, coords1, coords2, n_classes, normalize=True, index_b=None):
    """get_net_fd in float64 -> dict(fd, ld [B, U1, V1, U2, V2], target (exact, bool), skip (a point of the pair has an unlabeled
    tap), risky (a point of the pair has a one-dimensional label weight in (0, RISKY_WEIGHT)), w1, w2 (the per-tap label weights))."""
    f1 = np.asarray(feats1, dtype=np.float64)
    f2 = np.asarray(feats2, dtype=np.float64)
    label2 = np.asarray(label2)
    if index_b is not None:
        f2, label2 = f2[np.asarray(index_b)], label2[np.asarray(index_b)]
    c1 = np.asarray(coords1, dtype=np.float64)
    c2 = np.asarray(coords2, dtype=np.float64)
    s1, s2 = O.sample(f1, c1), O.sample(f2, c2)
    if normalize:
        s1, s2 = O.norm(s1), O.norm(s2)
    fd = O.tensor_correlation(s1, s2)
    ld = O.tensor_correlation(O.sample(one_hot_maps(label1, n_classes), c1), O.sample(one_hot_maps(label2, n_classes), c2))
    cls1, w1, ax1 = label_taps(label1, c1, n_classes)
    cls2, w2, ax2 = label_taps(label2, c2, n_classes)
    k1, u1, r1 = purity(cls1, w1, ax1)
    k2, u2, r2 = purity(cls2, w2, ax2)

    def pairs(a, b, op):
        return op(a[:, :, :, None, None], b[:, None, None, :, :])
    target = pairs(k1, k2, np.equal) & pairs(k1 >= 0, k2 >= 0, np.logical_and)
    return dict(fd=fd, ld=ld, target=target, skip=pairs(u1, u2, np.logical_or), risky=pairs(r1, r2, np.logical_or), w1=w1, w2=w2)


def bins_of(fd, n_bins, normalize=True):
    fd = np.asarray(fd, dtype=np.float64)
    if not normalize:
        fd = np.clip(fd, -1.0, 1.0)
    return np.clip(np.floor((fd + 1.0) / 2.0 * n_bins), 0, n_bins - 1).astype(np.int64)


def hist_from(fd, target, n_bins, keep=None, normalize=True):
    """int64 [n_bins, 2] (negatives, positives) of the pairs `keep` selects (all of them by default)."""
    b = bins_of(fd, n_bins, normalize).reshape(-1)
    t = np.asarray(target).reshape(-1).astype(np.int64)
    if keep is not None:
        k = np.asarray(keep).reshape(-1)
        b, t = b[k], t[k]
    return np.bincount(b * 2 + t, minlength=2 * n_bins).reshape(n_bins, 2)


def pr_from_hist(hist):
    """Precision and recall at every occupied bin taken as threshold (ascending, then the final (1, 0) point), the occupied bins,
    and the step integral sum (R_k - R_{k-1}) P_k, with plain loops over the bins from the top."""
    hist = np.asarray(hist, dtype=np.int64)
    n_pos = int(hist[:, 1].sum())
    prec, rec, bins = [], [], []
    tp = fp = 0
    ap, last_r = 0.0, 0.0
    for k in range(hist.shape[0] - 1, -1, -1):
        if hist[k, 0] + hist[k, 1] == 0:
            continue
        tp += int(hist[k, 1])
        fp += int(hist[k, 0])
        p = tp / (tp + fp)
        r = tp / n_pos if n_pos else float("nan")
        ap += (r - last_r) * p
        last_r = r
        prec.append(p)
        rec.append(r)
        bins.append(k)
    return np.array(prec[::-1] + [1.0]), np.array(rec[::-1] + [0.0]), np.array(bins[::-1], dtype=np.int64), (ap if n_pos else float("nan"))


def ap_unbinned(scores, targets):
    """average_precision_score on raw scores: one threshold per distinct score, the same step integral."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    t = np.asarray(targets).reshape(-1).astype(np.int64)
    order = np.argsort(-s, kind="stable")
    s, t = s[order], t[order]
    last = np.r_[np.nonzero(np.diff(s))[0], s.size - 1]          # the last element of every run of equal scores
    tps = np.cumsum(t)[last].astype(np.float64)
    n = (last + 1).astype(np.float64)
    if tps[-1] == 0:
        return float("nan")
    recall = tps / tps[-1]
    return float(np.sum(np.diff(np.r_[0.0, recall]) * (tps / n)))
