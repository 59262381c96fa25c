"""Refit the cluster probe for any cluster count: spherical (cosine) k-means over a dataset's codes (include/stego_kmeans.h,
csrc/code_kmeans.hip).

The cluster probe (``ClusterLookup``) is trained by minibatch gradient steps, for ``n_classes + extra_clusters`` clusters fixed at
training time.  Here the codes of a folder are collected once (``collect_codes``) and the probe is refitted on them by batch k-means
for any count, with ``ClusterLookup``'s own definitions - L2-normalised tokens and centroids, the first maximum of their inner
products - so a refitted probe means what a trained one means and runs through ``segment``, the stitcher and the metrics as it is.

``kmeans_seed`` / ``kmeans_step`` / ``kmeans_fit`` run on the kernels for a float32 HIP tensor [B, K, h, w] of any strides with K <= 128
and n <= 64; everything else (CPU tensors, another dtype, larger K or n) takes ``torch_kmeans_*``, the same arithmetic as a torch
chain: the public functions never fail on size.
"""
import collections

import torch
import torch.nn.functional as F

from . import capi

KMeansStep = collections.namedtuple("KMeansStep", ["centroids", "counts", "stats", "labels"])
KMeansStep.__doc__ = """One Lloyd iteration: centroids float32 [n, K] (unit rows; None for an assignment-only step), counts int64 [n], stats
float64 [4] = (objective = the sum of the winning similarities, clusters that kept their row, shift = 1 - min_n c_old . c_new, tokens),
labels uint8 [B, h, w] or None."""


class KMeansResult:
    """What kmeans_fit returns: ``centroids`` float32 [n, K] (unit rows), ``counts`` int64 [n] and ``objective`` (a float: the sum over
    the tokens of their similarity to their centroid) of the assignment under these centroids, ``history`` (the objective of every
    iteration, a list), ``n_iter`` (iterations run) and ``converged`` (shift < tol was seen)."""

    def __init__(self, centroids, counts, objective, history, n_iter, converged):
        self.centroids, self.counts, self.objective = centroids, counts, float(objective)
        self.history, self.n_iter, self.converged = list(history), int(n_iter), bool(converged)

    def __repr__(self):
        return "KMeansResult(n=%d, objective=%.6g, n_iter=%d, converged=%s)" % (self.centroids.shape[0], self.objective, self.n_iter,
                                                                              self.converged)


def _checked(codes, n):
    if not torch.is_tensor(codes) or codes.dim() != 4:
        raise ValueError("codes: expected a [B, K, h, w] tensor, got %s" % (tuple(codes.shape) if torch.is_tensor(codes) else type(codes),))
    if int(n) < 1:
        raise ValueError("k-means needs at least one cluster, got n = %r" % (n,))
    if codes.numel() == 0:
        raise ValueError("codes: an empty tensor %s" % (tuple(codes.shape),))
    return codes


def _native(codes, n):
    B, K, h, w = codes.shape
    return (codes.is_cuda and codes.dtype == torch.float32 and K <= capi.KMEANS_MAX_K and n <= capi.KMEANS_MAX_N and
            B <= capi.KMEANS_MAX_B and B * h * w <= capi.KMEANS_MAX_TOKENS)


def _tokens(codes):
    """[B, K, h, w] -> float32 [T, K], token (b, y, x) at (b h + y) w + x."""
    B, K, h, w = codes.shape
    return codes.permute(0, 2, 3, 1).reshape(B * h * w, K).float()


def _draws(n, generator):
    dev = generator.device if generator is not None else "cpu"
    return torch.rand(int(n), dtype=torch.float64, generator=generator, device=dev).cpu()


def _centroids_arg(centroids, K):
    if not torch.is_tensor(centroids) or centroids.dim() != 2 or centroids.shape[1] != K:
        raise ValueError("centroids: expected a [n, %d] tensor, got %s" % (K, tuple(centroids.shape) if torch.is_tensor(centroids) else type(centroids)))
    return centroids


# ---- the torch chain
def torch_kmeans_seed(codes, n, generator=None, u=None):
    """kmeans_seed as a torch chain on the tensor's device -> (centroids float32 [n, K], picks int64 [n]).
    u: the n uniform numbers instead of a draw from `generator`."""
    codes, n = _checked(codes, n), int(n)
    x = _tokens(codes)
    T, K = x.shape
    u = _draws(n, generator) if u is None else torch.as_tensor(u, dtype=torch.float64)
    if u.numel() != n or bool(((u < 0) | (u >= 1)).any()):
        raise ValueError("kmeans_seed: u must be %d numbers in [0, 1)" % n)
    xd = x.double()
    norm = xd.norm(dim=1)
    live = norm > 0
    w0 = live.double()
    cent = torch.zeros(n, K, dtype=torch.float32, device=x.device)
    picks = torch.zeros(n, dtype=torch.int64, device=x.device)
    best = None
    for r in range(n):
        if r == 0:
            w = w0
        else:
            sim = ((xd @ cent[r - 1].double()) / norm.clamp_min(1e-12)).float()
            best = sim if best is None else torch.maximum(best, sim)
            w = (1.0 - best.double()).clamp_min(0.0) * w0
            if not bool(w.sum() > 0):
                w = w0
        cum = w.cumsum(0)
        positive = torch.nonzero(w > 0)
        if positive.numel() == 0:
            pick = 0
        else:
            target = (u[r].to(cum.device) * cum[-1]).reshape(1)
            pick = min(int(torch.searchsorted(cum, target, right=True)), int(positive[-1]))     # the first cum > target
        picks[r] = pick
        cent[r] = x[pick] / norm[pick].clamp_min(1e-12).float()
    return cent, picks


def torch_kmeans_step(codes, centroids, out=None, labels=False, update=True):
    """kmeans_step as a torch chain on the tensor's device: normalize, the inner products, argmax (the first maximum), index_add_
    in float64, bincount."""
    codes = _checked(codes, 1)
    x = F.normalize(_tokens(codes), dim=1)
    T, K = x.shape
    c = F.normalize(_centroids_arg(centroids, K).to(x.device).float(), dim=1)
    n = c.shape[0]
    inner = x @ c.t()
    a = inner.argmax(1)
    objective = inner.gather(1, a[:, None]).double().sum()
    counts = torch.bincount(a, minlength=n)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    new = None
    kept, shift = zero, zero
    if update:
        sums = torch.zeros(n, K, dtype=torch.float64, device=x.device).index_add_(0, a, x.double())
        norm = sums.norm(dim=1)
        keep = (counts == 0) | ~(norm > 0)
        new = torch.where(keep[:, None], c.double(), sums / norm.clamp_min(1e-300)[:, None]).float()
        kept = keep.sum().double()
        shift = 1.0 - (c.double() * new.double()).sum(1).min()
        if out is not None:
            out.copy_(new)
            new = out
    stats = torch.stack([objective, kept, shift, torch.full((), float(T), dtype=torch.float64, device=x.device)])
    lab = a.to(torch.uint8 if n <= 256 else torch.int64).reshape(codes.shape[0], codes.shape[2], codes.shape[3]) if labels else None
    return KMeansStep(new, counts, stats, lab)


# ---- the kernels
def kmeans_seed(codes, n, generator=None, u=None):
    """k-means++ seeding of n centroids from the tokens of codes [B, K, h, w] -> (centroids float32 [n, K], unit rows; picks int64
    [n], the token indices).  The first token is drawn uniformly among the tokens of non-zero norm, every further one with weight
    max(0, 1 - its largest similarity to a centroid so far).  The n uniform numbers come from `generator` (torch.rand, float64) or
    are given as `u`: the draw stream is the caller's."""
    codes, n = _checked(codes, n), int(n)
    if not _native(codes, n):
        return torch_kmeans_seed(codes, n, generator, u)
    u = _draws(n, generator) if u is None else torch.as_tensor(u, dtype=torch.float64).cpu()
    if u.numel() != n:
        raise ValueError("kmeans_seed: u must be %d numbers in [0, 1)" % n)
    B, K, h, w = codes.shape
    return capi.kmeans_seed(capi.kmeans_desc(B, K, h, w, n), codes, u.tolist())


def kmeans_step(codes, centroids, out=None, labels=False, update=True):
    """One Lloyd iteration on codes [B, K, h, w] under centroids [n, K] (any scale) -> KMeansStep.  out: a float32 [n, K] tensor that
    takes the new centroids (`centroids` itself for an update in place), default a new one.  labels=True also returns every token's
    cluster.  update=False is assignment only: labels, counts and the objective, no new centroids.  Nothing is synchronised."""
    codes = _checked(codes, 1)
    K = codes.shape[1]
    centroids = _centroids_arg(centroids, K)
    n = int(centroids.shape[0])
    if not (_native(codes, n) and centroids.is_cuda and (out is None or out.is_cuda)):
        return torch_kmeans_step(codes, centroids, out, labels, update)
    B, _, h, w = codes.shape
    cin = centroids if (centroids.dtype == torch.float32 and centroids.is_contiguous()) else centroids.float().contiguous()
    cout = None
    if update:
        cout = out if out is not None else torch.empty((n, K), dtype=torch.float32, device=codes.device)
    lab = torch.empty((B, h, w), dtype=torch.uint8, device=codes.device) if labels else None
    counts, stats = capi.kmeans_step(capi.kmeans_desc(B, K, h, w, n), codes, cin, cout, lab)
    return KMeansStep(cout, counts, stats, lab)


def _fit_once(codes, cent, n_iter, tol, check_every):
    """Lloyd iterations in place on `cent` -> (counts, objective, history, iterations, converged).  The statistics of the steps stay on
    the device and are read once per `check_every` steps."""
    B, K, h, w = codes.shape
    n = int(cent.shape[0])
    native = _native(codes, n) and cent.is_cuda
    if native:
        desc = capi.kmeans_desc(B, K, h, w, n)
        ws = capi.kmeans_workspace(desc, codes.device)
        counts = torch.empty((n,), dtype=torch.int64, device=codes.device)
        rows = torch.empty((max(n_iter, 1) + 1, 4), dtype=torch.float64, device=codes.device)
    history, pending, done, converged = [], [], 0, False
    for it in range(n_iter):
        if native:
            capi.kmeans_step(desc, codes, cent, cent, None, counts, rows[it], ws)
            pending.append(rows[it])
        else:
            pending.append(torch_kmeans_step(codes, cent, out=cent).stats)
        done = it + 1
        if done % check_every == 0 or done == n_iter:
            got = torch.stack(pending).cpu()
            pending = []
            history.extend(float(v) for v in got[:, 0])
            if bool((got[:, 2] < tol).any()):
                converged = True
                break
    if native:
        capi.kmeans_step(desc, codes, cent, None, None, counts, rows[-1], ws)
        last = rows[-1]
    else:
        final = torch_kmeans_step(codes, cent, update=False)
        counts, last = final.counts, final.stats
    return counts.clone(), float(last[0]), history, done, converged


def kmeans_fit(codes, n_clusters, n_iter=100, tol=1e-6, n_init=1, init="k-means++", generator=None, check_every=10):
    """Spherical k-means of the tokens of codes [B, K, h, w] into n_clusters clusters -> KMeansResult.
    init: "k-means++" (kmeans_seed with `generator`) or a tensor [n_clusters, K] of starting centroids; n_init seedings are fitted and
    the one with the largest objective is kept.  A fit iterates in place, at most n_iter times; the steps' statistics are read once
    per `check_every` steps, with no host synchronisation in between, and the fit stops when a step moved no centroid by more than
    `tol` (shift = 1 - min_n c_old . c_new < tol)."""
    n = int(n_clusters)
    codes = _checked(codes, n)
    n_iter, check_every = int(n_iter), max(int(check_every), 1)
    if n_iter < 0:
        raise ValueError("kmeans_fit: n_iter = %r" % (n_iter,))
    given = torch.is_tensor(init)
    if not given and init != "k-means++":
        raise ValueError("kmeans_fit: init = %r, expected 'k-means++' or a tensor [n_clusters, K]" % (init,))
    if given and tuple(init.shape) != (n, codes.shape[1]):
        raise ValueError("kmeans_fit: init has shape %s, expected %s" % (tuple(init.shape), (n, codes.shape[1])))
    best = None
    with torch.no_grad():
        for _ in range(1 if given else max(int(n_init), 1)):
            if given:
                cent = F.normalize(init.detach().to(codes.device).float(), dim=1).contiguous().clone()
            else:
                cent = kmeans_seed(codes, n, generator)[0]
            counts, objective, history, done, converged = _fit_once(codes, cent, n_iter, float(tol), check_every)
            if best is None or objective > best.objective:
                best = KMeansResult(cent, counts, objective, history, done, converged)
    return best


# ---- the model
def collect_codes(model, batches, flip=True):
    """The low-resolution codes of every image of `batches` (image tensors [N, 3, H, W], or batches with "img" / (img, ...) tuples)
    under model.net, in eval mode and without gradients -> one channels-last float32 tensor [N, K, h, w] on the model's device.
    flip: the code is averaged with that of the mirror image, as evaluation and segment() do."""
    dev = next(model.parameters()).device
    was_training = model.training
    model.eval()
    outs = []
    try:
        with torch.no_grad():
            for batch in batches:
                img = batch["img"] if isinstance(batch, dict) else batch[0] if isinstance(batch, (tuple, list)) else batch
                if img is None:
                    continue
                img = img.to(dev)
                code = model.net(img)[1]
                if flip:
                    code = (code + model.net(img.flip(dims=[3]))[1].flip(dims=[3])) / 2
                outs.append(code.float())
    finally:
        model.train(was_training)
    if not outs:
        raise ValueError("collect_codes: no images")
    return torch.cat(outs).contiguous(memory_format=torch.channels_last)


def set_cluster_probe(model, centroids):
    """Replace model.cluster_probe by a ClusterLookup holding `centroids` [n, dim]: cfg.cluster_probe_n records the count, the cluster
    metrics are rebuilt for it, the stored cluster -> class assignment and the optimizers (which hold the old probe's parameter) are
    dropped."""
    from .featurizers import ClusterLookup
    n, dim = int(centroids.shape[0]), int(centroids.shape[1])
    old = model.cluster_probe
    if dim != old.clusters.shape[1]:
        raise ValueError("refit: the centroids have %d channels, the model's code %d" % (dim, old.clusters.shape[1]))
    probe = ClusterLookup(dim, n).to(old.clusters.device)
    with torch.no_grad():
        probe.clusters.copy_(centroids.to(old.clusters.device, old.clusters.dtype))
    model.cluster_probe = probe
    if isinstance(model.cfg, dict):
        model.cfg["cluster_probe_n"] = n
    else:
        model.cfg.cluster_probe_n = n
    extra = max(n - model.n_classes, 0)
    for name in ("cluster_metrics", "test_cluster_metrics"):
        m = getattr(model, name)
        setattr(model, name, type(m)(m.prefix, m.n_classes, extra, m.compute_hungarian))
    model._cluster_to_class = None
    model._optims = None
    model._fused = None
    return model


def refit_cluster_probe(model, codes, n_clusters, **fit_args):
    """kmeans_fit(codes, n_clusters, **fit_args) and its centroids as the model's cluster probe (set_cluster_probe) -> KMeansResult."""
    result = kmeans_fit(codes, n_clusters, **fit_args)
    set_cluster_probe(model, result.centroids)
    return result
