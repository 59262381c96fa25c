"""csrc/corr_pr.hip on the MI355X against the float64 oracle (tests/corr_pr_oracle.py) on the same fp32 inputs.

A histogram cannot be compared element by element: a score within rounding of a bin edge may land on either side, and a label tap
whose weight is a rounding error away from 0 may or may not take part in a point's purity code.  So:
  targets  per column, |kernel total - oracle total| is at most the number of pairs in which a point has a bilinear label weight
           (left / right / top / bottom) inside the open interval (0, 1e-4) in float64 (the "risky" pairs: only there can fp32 pick
           other taps than float64); they are at most 1 % of the pairs of every input, asserted on the oracle side first;
  scores   per column and bin edge e, |cum_kernel(e) - cum_oracle(e)| is at most the number of oracle scores within delta of e plus
           the risky pairs.  delta = 2e-5, the absolute bar tests/test_dense_corr.py:55 holds unit-scale correlations to; where the
           existing capi.sample + capi.dense_corr chain itself exceeds 2e-5 against the oracle on the same points, delta is twice
           that chain's measured maximum error (never derived from the new kernel).  Every case prints both.
Everything that integers decide (accumulation on top of a histogram, repeatability, evaluate_correspondence against replayed direct
calls, the two closed-form curves) is compared exactly."""
import math
import types
import warnings

import numpy as np
import pytest
import torch

import corr_pr_oracle as P
from oracle import corr_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DELTA = 2e-5
N_CLASSES = 6


def _labels(rng, B, HL, block):
    """Blocky label maps with unlabeled regions: -1 and a value beyond n_classes."""
    nb = -(-HL // block)
    lab = rng.integers(-1, N_CLASSES + 1, (B, nb, nb))
    lab = np.where(lab == N_CLASSES, 255, lab)
    return np.repeat(np.repeat(lab, block, 1), block, 2)[:, :HL, :HL].astype(np.int64)


def _features(rng, B, C, h, unit=False):
    """Low-rank structure plus noise, so that the cosines spread over the bins instead of piling up around 0."""
    proto = rng.standard_normal((5, C))
    z = rng.standard_normal((B, 5, h, h))
    f = np.einsum("brhw,rc->bchw", z, proto) + 0.5 * rng.standard_normal((B, C, h, h))
    if unit:
        f /= np.sqrt((f * f).sum(1, keepdims=True))
    return f.astype(np.float32)


def _dev_map(f, layout):
    t = torch.from_numpy(f).to(DEV)
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if layout == "cl" else t


def _chain_error(ta, tb, fa, fb, c1, c2, index_b, normalize):
    """Max |capi.sample + capi.dense_corr - oracle| on the same points (both lists padded to one S x S square by repetition)."""
    from stego_amd import capi
    B = fa.shape[0]
    S = int(math.ceil(math.sqrt(max(c1.shape[1], c2.shape[1]))))
    q1, q2 = [c[:, np.arange(S * S) % c.shape[1]].reshape(B, S, S, 2) for c in (c1, c2)]
    idx = None if index_b is None else torch.from_numpy(index_b).to(DEV)
    s1 = capi.sample(ta, torch.from_numpy(q1).to(DEV))
    s2 = capi.sample(tb, torch.from_numpy(q2).to(DEV), index=idx)
    got = capi.dense_corr(s1, s2, normalize=normalize).cpu().numpy().astype(np.float64)
    fb64 = fb.astype(np.float64) if index_b is None else fb.astype(np.float64)[index_b]
    r1, r2 = O.sample(fa.astype(np.float64), q1.astype(np.float64)), O.sample(fb64, q2.astype(np.float64))
    if normalize:
        r1, r2 = O.norm(r1), O.norm(r2)
    return float(np.abs(got - O.tensor_correlation(r1, r2)).max())


def _check(hist, o, n_bins, normalize, skip_unlabeled, delta, what):
    keep = ~o["skip"] if skip_unlabeled else np.ones(o["target"].shape, dtype=bool)
    n_pairs = o["target"].size
    n_risky = int(o["risky"].sum())
    assert n_risky <= 0.01 * n_pairs, (what, n_risky, n_pairs)                      # the cap, on the oracle side, before the kernel is looked at
    want = P.hist_from(o["fd"], o["target"], n_bins, keep=keep, normalize=normalize)
    fd = o["fd"] if normalize else np.clip(o["fd"], -1.0, 1.0)
    print("%s: %d pairs, %d kept, %d positive, %d risky; kernel totals %s oracle totals %s"
          % (what, n_pairs, int(keep.sum()), int((o["target"] & keep).sum()), n_risky, hist.sum(0).tolist(), want.sum(0).tolist()))
    assert (hist >= 0).all()
    if not skip_unlabeled and n_risky == 0:
        assert int(hist.sum()) == n_pairs
    worst = 0
    for col in (0, 1):
        assert abs(int(hist[:, col].sum()) - int(want[:, col].sum())) <= n_risky, (what, col)
        s = fd[keep & (o["target"] == bool(col))]
        k = np.rint((s + 1.0) / 2.0 * n_bins).astype(np.int64)                          # the nearest edge (delta is far below half a bin)
        near = np.bincount(k[np.abs(s - (-1.0 + 2.0 * k / n_bins)) <= delta], minlength=n_bins + 1)
        diff = np.abs(np.cumsum(hist[:, col]) - np.cumsum(want[:, col]))[:-1]           # below edge k, k = 1 .. n_bins - 1
        slack = near[1:n_bins] + n_risky
        worst = max(worst, int((diff - slack).max()))
        assert (diff <= slack).all(), (what, col, int(np.argmax(diff - slack)) + 1, int(diff.max()))
    print("%s: max cumulative difference beyond its allowance %d (<= 0 passes); elementwise differing bins %d of %d"
          % (what, worst, int((hist != want).any(1).sum()), n_bins))


CASES = {
    # name: (C, layout, h, HL, N1, N2, n_bins, normalize, skip_unlabeled, index_b, special)
    "c27_nchw_121":        (27, "nchw", 12, 48, 121, 121, 4096, True, False, None, None),
    "c27_border_zero":     (27, "nchw", 12, 48, 121, 121, 4096, True, False, None, "border_zero"),
    "c70_cl_784_skip":     (70, "cl", 40, 320, 784, 784, 4096, True, True, None, None),
    "c70_cl_784":          (70, "cl", 40, 320, 784, 784, 4096, True, False, None, None),
    "c70_nchw_raw_50x333": (70, "nchw", 28, 100, 50, 333, 4096, False, False, None, None),
    "c384_cl_50x333_b64":  (384, "cl", 28, 224, 50, 333, 64, True, True, None, None),
    "c768_cl_121_b8192":   (768, "cl", 40, 320, 121, 121, 8192, True, False, [1, 1], None),
    "c768_nchw_784":       (768, "nchw", 40, 160, 784, 784, 4096, True, True, [1, 0], None),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_histogram_against_float64_oracle(name):
    """Measured maximum error of the existing capi.sample + capi.dense_corr chain against the oracle on these inputs (MI355X, printed
    per case): 6.2e-7 (c70_nchw_raw_50x333) to 6.6e-6 (c70_cl_784_skip), C = 768: 1.0e-6 - 1.6e-6.  All below 2e-5, so delta is 2e-5
    in every case; a case whose chain error exceeded it would run with twice that error."""
    from stego_amd import capi
    C, layout, h, HL, N1, N2, n_bins, normalize, skip, index_b, special = CASES[name]
    B = 2
    rng = np.random.default_rng(sum(map(ord, name)))
    fa, fb = _features(rng, B, C, h, unit=not normalize), _features(rng, B, C, h, unit=not normalize)
    la, lb = _labels(rng, B, HL, 8), _labels(rng, B, HL, 8)
    c1 = (rng.random((B, N1, 2)) * 2 - 1).astype(np.float32)
    c2 = (rng.random((B, N2, 2)) * 2 - 1).astype(np.float32)
    if special == "border_zero":
        c1[:, :20] = (rng.random((B, 20, 2)) * 5 - 2.5).astype(np.float32)               # outside [-1, 1]: border
        c2[:, :20] = (rng.random((B, 20, 2)) * 5 - 2.5).astype(np.float32)
        c2[0, 20], c2[0, 21], c2[1, 20] = (-1.0, -1.0), (1.0, 1.0), (1.0, -1.0)            # the corners themselves: weights exactly 0 and 1
        fa[0, :, 4:8, 4:8] = 0.0                                                         # zero feature vectors: the eps branch of norm()
        c1[0, 30], c1[0, 31] = (0.0, 0.0), (0.05, -0.05)                                 # ... sampled well inside the zero region
    idx = None if index_b is None else np.array(index_b, dtype=np.int64)
    ta, tb = _dev_map(fa, layout), _dev_map(fb, layout)
    chain = _chain_error(ta, tb, fa, fb, c1, c2, idx, normalize)
    delta = DELTA if chain <= DELTA else 2 * chain
    print("%s: sample + dense_corr chain max error %.3e -> delta %.3e" % (name, chain, delta))
    o = P.net_fd(fa, fb, la, lb, c1[:, :, None, :], c2[:, :, None, :], N_CLASSES, normalize=normalize, index_b=idx)
    if special == "border_zero":
        assert (o["fd"][0, 0, 30] == 0).all() and (o["fd"][0, 0, 31] == 0).all()        # the eps branch really is exercised
    hist = torch.zeros(n_bins, 2, dtype=torch.int64, device=DEV)
    capi.pr_accumulate(ta, tb, torch.from_numpy(la).to(DEV), torch.from_numpy(lb).to(DEV), torch.from_numpy(c1).to(DEV),
                       torch.from_numpy(c2).to(DEV), hist, N_CLASSES, index_b=None if idx is None else torch.from_numpy(idx).to(DEV),
                       normalize=normalize, skip_unlabeled=skip)
    _check(hist.cpu().numpy(), o, n_bins, normalize, skip, delta, name)


def _small_inputs(seed, B=3, C=70, h=20, HL=80, N1=200, N2=150):
    rng = np.random.default_rng(seed)
    t = lambda x: torch.from_numpy(x).to(DEV)            # noqa: E731
    return dict(a=_dev_map(_features(rng, B, C, h), "cl"), b=t(_features(rng, B, C, h)), labels_a=t(_labels(rng, B, HL, 8)),
                labels_b=t(_labels(rng, B, HL, 8)), coords1=t((rng.random((B, N1, 2)) * 2 - 1).astype(np.float32)),
                coords2=t((rng.random((B, N2, 2)) * 2 - 1).astype(np.float32)))


@pytest.mark.parametrize("skip", [False, True])
def test_accumulates_on_top_and_repeats_bitwise(skip):
    from stego_amd import capi
    x, y = _small_inputs(1), _small_inputs(2)

    def run(d, hist):
        return capi.pr_accumulate(hist=hist, n_classes=N_CLASSES, skip_unlabeled=skip, **d)
    h1 = run(x, torch.zeros(4096, 2, dtype=torch.int64, device=DEV))
    h2 = run(y, torch.zeros(4096, 2, dtype=torch.int64, device=DEV))
    both = run(y, run(x, torch.zeros(4096, 2, dtype=torch.int64, device=DEV)))
    assert torch.equal(both, h1 + h2)                                                   # two calls into one histogram
    for _ in range(3):                                                                  # the same bytes every time
        assert torch.equal(run(x, torch.zeros(4096, 2, dtype=torch.int64, device=DEV)), h1)
    pre = torch.randint(0, 1 << 40, (4096, 2), dtype=torch.int64, device=DEV)           # only ever added to, beyond 32 bits too
    assert torch.equal(run(x, pre.clone()) - pre, h1)
    n = 3 * 200 * 150
    assert int(h1.sum()) == n if not skip else 0 < int(h1.sum()) < n
    assert int(h1[:, 1].sum()) > 0 and int(h1[:, 0].sum()) > 0


def test_correspondence_pr_class_on_device():
    from stego_amd import capi
    from stego_amd.correspondence_pr import CorrespondencePR
    x = _small_inputs(3)
    m = CorrespondencePR(n_classes=N_CLASSES, n_bins=1024)
    m.update(**x)
    m.update(**x)
    direct = capi.pr_accumulate(hist=torch.zeros(1024, 2, dtype=torch.int64, device=DEV), n_classes=N_CLASSES, **x)
    res = m.compute()
    assert np.array_equal(res["hist"], 2 * direct.cpu().numpy()) and res["n_total"] == 2 * 3 * 200 * 150
    assert 0.0 < res["average_precision"] <= 1.0 and res["precision"][-1] == 1.0 and res["recall"][-1] == 0.0
    a = m.at(0.18)
    assert a["edge"] >= 0.18 > a["edge"] - 2 / 1024 and 0 < a["share"] < 1
    m.reset()
    assert m.compute()["n_total"] == 0


def _tiny_model():
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=2", "dim=70", "dropout=False"])
    torch.manual_seed(0)
    model = LitUnsupervisedSegmenter(27, cfg).to(DEV).eval()
    loader = torch.utils.data.DataLoader(SyntheticContrastiveDataset(8, 64, 27, seed=3), 4, shuffle=False)
    return model, loader


def test_evaluate_correspondence_equals_replayed_direct_calls():
    from stego_amd import capi
    from stego_amd.correspondence_pr import evaluate_correspondence
    from stego_amd.modules import _unfix
    model, loader = _tiny_model()
    S, seed, n_bins = 7, 5, 2048
    res = evaluate_correspondence(model, loader, n_samples=S, max_batches=100, pairs=("self", "knn", "random"), seed=seed, n_bins=n_bins)
    assert sorted(res) == ["code", "feats"] and all(sorted(v) == ["knn", "random", "self"] for v in res.values())
    want = {m: {k: torch.zeros(n_bins, 2, dtype=torch.int64, device=DEV) for k in ("self", "knn", "random")} for m in ("feats", "code")}
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    with torch.no_grad():
        for batch in loader:
            img, label = batch["img"].to(DEV), batch["label"].to(DEV)
            B = img.shape[0]
            c1 = torch.rand((B, S, S, 2), generator=gen, device=DEV) * 2 - 1
            c2 = torch.rand((B, S, S, 2), generator=gen, device=DEV) * 2 - 1
            perm = _unfix(torch.randperm(B, generator=gen, device=DEV, dtype=torch.long))
            maps = dict(zip(("feats", "code"), model.net(img)))
            maps_pos = dict(zip(("feats", "code"), model.net(batch["img_pos"].to(DEV))))
            lp = batch["label_pos"].to(DEV)
            for m in ("feats", "code"):
                capi.pr_accumulate(maps[m], maps[m], label, label, c1, c2, want[m]["self"], 27)
                capi.pr_accumulate(maps[m], maps_pos[m], label, lp, c1, c2, want[m]["knn"], 27)
                capi.pr_accumulate(maps[m], maps[m], label, label, c1, c2, want[m]["random"], 27, index_b=perm)
    shifts = dict(self=model.cfg.pos_intra_shift, knn=model.cfg.pos_inter_shift, random=model.cfg.neg_inter_shift)
    for m in want:
        for k in want[m]:
            assert np.array_equal(res[m][k]["hist"], want[m][k].cpu().numpy()), (m, k)
            assert res[m][k]["n_total"] == 8 * S ** 4
            assert res[m][k]["at_shift"]["shift"] == shifts[k] and res[m][k]["at_shift"]["edge"] >= shifts[k]
    only_self = evaluate_correspondence(model, loader, n_samples=S, max_batches=1, seed=seed, n_bins=n_bins)
    assert sorted(only_self["feats"]) == ["self"] and only_self["feats"]["self"]["n_total"] == 4 * S ** 4


class _ConstNet(torch.nn.Module):
    """Spatially constant maps: every score falls in one bin."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, img):
        v = torch.linspace(0.1, 1.0, 8, device=img.device).view(1, 8, 1, 1)
        return v.expand(img.shape[0], 8, 4, 4).contiguous(), (-v[:, :5]).expand(img.shape[0], 5, 4, 4).contiguous()


def _stub_model(n_classes):
    m = torch.nn.Module()
    m.net = _ConstNet()
    m.n_classes = n_classes
    m.cfg = types.SimpleNamespace(pos_intra_shift=0.18, pos_inter_shift=0.12, neg_inter_shift=0.46)
    return m.to(DEV)


def test_closed_form_curves():
    from stego_amd.correspondence_pr import evaluate_correspondence
    model, _ = _tiny_model()
    one_class = [dict(img=torch.randn(4, 3, 64, 64), label=torch.full((4, 64, 64), 3, dtype=torch.int64)) for _ in range(2)]
    res = evaluate_correspondence(model, one_class, n_samples=6, pairs=("self", "random"))
    for m in res:
        for k in res[m]:
            r = res[m][k]
            assert r["n_pos"] == r["n_total"] == 2 * 4 * 6 ** 4 and r["average_precision"] == 1.0, (m, k)
    rng = np.random.default_rng(4)
    blocky = [dict(img=torch.randn(4, 3, 16, 16), label=torch.from_numpy(_labels(rng, 4, 32, 8))) for _ in range(2)]
    res = evaluate_correspondence(_stub_model(N_CLASSES), blocky, n_samples=9, pairs=("self",))
    for m in res:
        r = res[m]["self"]
        assert (r["hist"].sum(1) > 0).sum() == 1 and 0 < r["n_pos"] < r["n_total"] == 8 * 9 ** 4
        assert r["average_precision"] == r["n_pos"] / r["n_total"], m


def test_binned_average_precision_against_unbinned_scores():
    """Printed, not asserted: nobody has measured how far the 4096-bin AP is from the AP of the unbinned float64 scores."""
    from stego_amd import capi
    rng = np.random.default_rng(9)
    B, C, h, HL, N = 2, 70, 40, 320, 400
    f, lab = _features(rng, B, C, h), _labels(rng, B, HL, 16)
    c1, c2 = [(rng.random((B, N, 2)) * 2 - 1).astype(np.float32) for _ in range(2)]
    o = P.net_fd(f, f, lab, lab, c1[:, :, None, :], c2[:, :, None, :], N_CLASSES)
    t = _dev_map(f, "cl")
    tl = torch.from_numpy(lab).to(DEV)
    hist = capi.pr_accumulate(t, t, tl, tl, torch.from_numpy(c1).to(DEV), torch.from_numpy(c2).to(DEV),
                              torch.zeros(4096, 2, dtype=torch.int64, device=DEV), N_CLASSES)
    ap_bins = P.pr_from_hist(hist.cpu().numpy())[3]
    ap_raw = P.ap_unbinned(o["fd"], o["target"])
    try:
        from sklearn.metrics import average_precision_score
        ap_raw = float(average_precision_score(o["target"].reshape(-1), o["fd"].reshape(-1)))
    except ImportError:
        pass
    print("AP from 4096 bins %.9f, AP of the unbinned float64 scores %.9f, difference %.3e" % (ap_bins, ap_raw, ap_bins - ap_raw))
    assert 0.0 < ap_bins <= 1.0
