"""The float64 oracle of the cluster refit (include/stego_kmeans.h), in numpy: spherical k-means with ClusterLookup's definitions -
x^ = x / max(|x|, 1e-12), c^ = c / max(|c|, 1e-12), the label is the first maximum of x^ . c^ - and the k-means++ seeding from
given uniform numbers."""
import numpy as np

EPS = 1e-12


def tokens(x):
    """[B, K, h, w] -> float64 [T, K], token (b, y, x) at (b h + y) w + x."""
    x = np.asarray(x)
    return x.transpose(0, 2, 3, 1).reshape(-1, x.shape[1]).astype(np.float64)


def normalize(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), EPS)


def assign(x, cent):
    """-> (labels [T] (first maximum), the winning similarities [T], the gap between the two largest similarities [T] (inf at n = 1))."""
    inner = normalize(tokens(x)) @ normalize(cent).T
    labels = inner.argmax(1)
    top = np.sort(inner, axis=1)
    gap = top[:, -1] - top[:, -2] if inner.shape[1] > 1 else np.full(inner.shape[0], np.inf)
    return labels, inner[np.arange(inner.shape[0]), labels], gap


def update(x, cent, labels):
    """The new centroids of a step whose assignment was `labels` -> (centroids [n, K], kept [n] bool, shift)."""
    xh, ch = normalize(tokens(x)), normalize(cent)
    n = ch.shape[0]
    sums = np.zeros_like(ch)
    np.add.at(sums, labels, xh)
    counts = np.bincount(labels, minlength=n)
    norm = np.linalg.norm(sums, axis=1)
    kept = (counts == 0) | ~(norm > 0)
    new = np.where(kept[:, None], ch, sums / np.where(kept, 1.0, norm)[:, None])
    return new, kept, 1.0 - (ch * new).sum(1).min()


def step(x, cent):
    """One Lloyd iteration -> dict(labels, counts, objective, centroids, kept, shift, gap)."""
    labels, sim, gap = assign(x, cent)
    new, kept, shift = update(x, cent, labels)
    return dict(labels=labels, counts=np.bincount(labels, minlength=np.asarray(cent).shape[0]), objective=sim.sum(), centroids=new,
                kept=kept, shift=shift, gap=gap)


def seed(x, n, u, snap=False):
    """k-means++ from the uniform numbers u [n] -> dict(picks [n], centroids [n, K], u (the numbers used), margin).
    Round 0 weighs every token of non-zero norm 1; round r weighs max(0, 1 - best) with best the largest similarity to a centroid so
    far, kept as float32, and 0 for zero-norm tokens; a round without weight uses round 0's.  The pick is the first token whose
    inclusive cumulative weight exceeds u_r * total.
    snap: after a round's pick, u_r is moved to the middle of the picked token's interval.  margin: the smallest distance, over the
    rounds, of u_r * total to an edge of the picked interval, as a share of the total."""
    t = tokens(x)
    norm = np.linalg.norm(t, axis=1)
    xh = t / np.maximum(norm, EPS)[:, None]
    w0 = (norm > 0).astype(np.float64)
    u = np.array(u, dtype=np.float64)
    K = t.shape[1]
    picks, cent = np.zeros(n, dtype=np.int64), np.zeros((n, K))
    best = np.full(t.shape[0], -2.0, dtype=np.float32)
    margin = np.inf
    for r in range(n):
        if r == 0:
            w = w0
        else:
            best = np.maximum(best, (xh @ cent[r - 1]).astype(np.float32))
            w = np.maximum(0.0, 1.0 - best.astype(np.float64)) * w0
            if not w.sum() > 0:
                w = w0
        cum = np.cumsum(w)
        total = cum[-1]
        if not total > 0:
            picks[r] = 0
        else:
            pick = int(np.searchsorted(cum, u[r] * total, side="right"))
            pick = min(pick, int(np.nonzero(w > 0)[0][-1]))
            lo, hi = cum[pick] - w[pick], cum[pick]
            if snap:
                u[r] = 0.5 * (lo + hi) / total
            margin = min(margin, (u[r] * total - lo) / total, (hi - u[r] * total) / total)
            picks[r] = pick
        cent[r] = np.float32(t[picks[r]]).astype(np.float64) / np.float32(max(norm[picks[r]], EPS))
        cent[r] = cent[r].astype(np.float32)
    return dict(picks=picks, centroids=cent, u=u, margin=margin)


def fit(x, cent, n_iter=100):
    """Lloyd iterations from `cent` until the labels repeat -> (centroids, labels, objectives)."""
    cent = normalize(cent)
    objectives, last = [], None
    for _ in range(n_iter):
        s = step(x, cent)
        objectives.append(s["objective"])
        cent = s["centroids"]
        if last is not None and np.array_equal(last, s["labels"]):
            break
        last = s["labels"]
    return cent, assign(x, cent)[0], objectives


def planted(n=5, K=70, B=3, h=7, w=5, noise=0.05, seed=0):
    """Tokens around n random unit directions, noise per channel, token norms in [0.5, 3] -> (map float32 [B, K, h, w], the
    direction of every token [T])."""
    rng = np.random.default_rng(seed)
    T = B * h * w
    dirs = normalize(rng.standard_normal((n, K)))
    which = np.arange(T) % n
    rng.shuffle(which)
    t = dirs[which] + noise * rng.standard_normal((T, K))
    t = normalize(t) * rng.uniform(0.5, 3.0, (T, 1))
    return np.ascontiguousarray(t.reshape(B, h, w, K).transpose(0, 3, 1, 2)).astype(np.float32), which


def same_partition(a, b):
    """Whether two label vectors describe one partition (up to the names of the clusters)."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))
