"""csrc/confusion.hip on the MI355X: the probe-confusion kernel's counts equal, element for element, the bincount of the fused probe
head's ARGMAX output (the same arithmetic with another sink) and stay within the float64 reference chain's unclear pixels; counts add
up across calls, ignore the code's layout and a skipped probe, survive the all-one-bin extreme of the wave aggregation, and repeat
bit for bit; stego_confusion equals torch.argmax plus UnsupervisedMetrics' masking; evaluate() and validation_step() with
native_metrics agree with the paths they replace."""
import functools
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _inputs(B, K, h, w, n_lin, n_clu, seed, scale=1.0):
    """The seeded generator of tests/test_probe_head_gpu.py::_inputs."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randn(B, K, h, w, generator=g) * scale
    flip = torch.randn(B, K, h, w, generator=g) * scale
    W = torch.randn(n_lin, K, generator=g) / K ** 0.5
    b = torch.randn(n_lin, generator=g) * 0.1
    cent = torch.randn(n_clu, K, generator=g)
    return code, flip, W, b, cent


def _labels(B, H, W, n_classes, seed):
    """Ignored values on both sides of [0, n_classes): -1, n_classes and n_classes + 1."""
    return torch.randint(-1, n_classes + 2, (B, H, W), generator=torch.Generator().manual_seed(seed + 1))


def _chain(code, flip, W, b, cent, size, alpha=2.0):
    """eval_segmentation.py:124-128 of the reference, in the inputs' dtype and on their device."""
    c = (code + flip.flip(dims=[3])) / 2 if flip is not None else code
    c = F.interpolate(c, size, mode="bilinear", align_corners=False)
    lin = torch.log_softmax(F.conv2d(c, W[:, :, None, None], b), dim=1)
    inner = torch.einsum("bchw,nc->bnhw", F.normalize(c, dim=1), F.normalize(cent, dim=1))
    return lin, torch.log_softmax(inner * alpha, dim=1)


def _bincount(pred, labels, n, n_classes):
    """Plain torch indexing: rows are predictions, columns labels; labels outside [0, n_classes) and predictions outside [0, n) drop."""
    pred, labels = pred.reshape(-1), labels.reshape(-1)
    keep = (labels >= 0) & (labels < n_classes) & (pred >= 0) & (pred < n)
    return torch.bincount(pred[keep] * n_classes + labels[keep], minlength=n * n_classes).reshape(n, n_classes).cpu()


def _counts(code, flip, W, b, cent, labels, n_classes, lin=True, clu=True, into=None):
    """capi.probe_confusion onto zeroed (or the given) matrices -> (linear counts, cluster counts) on the device."""
    from stego_amd import capi
    lc, cc = into if into is not None else (torch.zeros(W.shape[0], n_classes, dtype=torch.int64, device=DEV) if lin else None,
                                            torch.zeros(cent.shape[0], n_classes, dtype=torch.int64, device=DEV) if clu else None)
    capi.probe_confusion(code, flip, W, b, F.normalize(cent, dim=1), labels, lc, cc, 2.0)
    return lc, cc


CASES = [  # B, K, h, w, H, W, n_lin, n_clu, flip; n_classes = n_lin
    (2, 70, 12, 12, 96, 96, 27, 27, True),
    (2, 70, 20, 20, 160, 160, 27, 32, True),
    (2, 32, 15, 17, 121, 135, 12, 16, False),
    (2, 24, 9, 11, 70, 86, 5, 8, True),
    (1, 128, 17, 23, 136, 184, 40, 64, False),
    (2, 70, 40, 40, 24, 24, 27, 27, True),
    (3, 70, 7, 7, 56, 56, 27, 27, True),
]
IDS = ["B%d_K%d_%dx%d_%dx%d_n%d+%d_%s" % (c[:8] + ("flip" if c[8] else "noflip",)) for c in CASES]


@functools.lru_cache(maxsize=None)
def _case(case):
    """Everything tests 1 and 2 need for one case, computed once: the kernel's counts, the ARGMAX kind's, the float64 chain's."""
    from stego_amd import capi
    B, K, h, w, H, W, n_lin, n_clu, flip = case
    n_classes = n_lin
    seed = sum(case[:8])
    code, fl, Wt, b, cent = [t.to(DEV) for t in _inputs(B, K, h, w, n_lin, n_clu, seed)]
    fl = fl if flip else None
    labels = _labels(B, H, W, n_classes, seed).to(DEV)
    got = [c.cpu() for c in _counts(code, fl, Wt, b, cent, labels, n_classes)]
    am = capi.probe_head(code, fl, Wt, b, F.normalize(cent, dim=1), (H, W), "argmax", "argmax", 2.0)
    head = [_bincount(am[0], labels, n_lin, n_classes), _bincount(am[1], labels, n_clu, n_classes)]
    t64 = _chain(*[t.double() if t is not None else None for t in (code, fl, Wt, b, cent)], (H, W))
    valid = (labels >= 0) & (labels < n_classes)
    ref64, unclear = [], []
    for lp, n in zip(t64, (n_lin, n_clu)):
        top2 = lp.topk(2, dim=1).values
        unclear.append(int((((top2[:, 0] - top2[:, 1]) < 2e-4) & valid).sum()))
        ref64.append(_bincount(lp.argmax(1), labels, n, n_classes))
    return dict(got=got, head=head, ref64=ref64, unclear=unclear, n_valid=int(valid.sum()), n_pix=B * H * W)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_equal_the_argmax_kind_exactly(case):
    r = _case(case)
    for name, got, head in zip(("linear", "cluster"), r["got"], r["head"]):
        assert got.dtype == torch.int64 and got.shape == head.shape, name
        assert torch.equal(got, head), (name, int((got - head).abs().sum()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_counts_against_the_float64_chain(case):
    """A pixel can change bins only where the float64 top-2 margin is below 2e-4: twice the 1e-4 bar
    test_probe_head_gpu.py::test_log_probs_against_torch_and_float64 holds this arithmetic to."""
    r = _case(case)
    for name, got, ref, unclear in zip(("linear", "cluster"), r["got"], r["ref64"], r["unclear"]):
        moved = int((got - ref).abs().sum()) / 2
        print("%s: moved %d, unclear %d of %d pixels (%.3f %%)" % (name, moved, unclear, r["n_pix"], 100.0 * unclear / r["n_pix"]))
        assert int(got.sum()) == r["n_valid"], name
        assert unclear < 0.01 * r["n_pix"], (name, unclear)
        assert moved <= unclear, (name, moved, unclear)


def _setup(case, seed=None):
    B, K, h, w, H, W, n_lin, n_clu, flip = case
    seed = sum(case[:8]) if seed is None else seed
    code, fl, Wt, b, cent = [t.to(DEV) for t in _inputs(B, K, h, w, n_lin, n_clu, seed)]
    return code, (fl if flip else None), Wt, b, cent, _labels(B, H, W, n_lin, seed).to(DEV)


def test_counts_accumulate():
    case = CASES[1]
    n_classes = case[6]
    code, fl, Wt, b, cent, labels = _setup(case)
    code2, fl2, _, _, _, labels2 = _setup(case, seed=99)
    one = _counts(code, fl, Wt, b, cent, labels, n_classes)
    twice = _counts(code, fl, Wt, b, cent, labels, n_classes, into=_counts(code, fl, Wt, b, cent, labels, n_classes))
    other = _counts(code2, fl2, Wt, b, cent, labels2, n_classes)
    both = _counts(code2, fl2, Wt, b, cent, labels2, n_classes, into=_counts(code, fl, Wt, b, cent, labels, n_classes))
    for i in range(2):
        assert int(one[i].sum()) > 0 and not torch.equal(one[i], other[i])
        assert torch.equal(twice[i], 2 * one[i])
        assert torch.equal(both[i], one[i] + other[i])


def test_channels_last_strided_code():
    case = CASES[0]
    code, fl, Wt, b, cent, labels = _setup(case)
    cl = code.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    fcl = fl.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert cl.stride(1) == 1 and not cl.is_contiguous()
    a = _counts(cl, fcl, Wt, b, cent, labels, case[6])
    c = _counts(code, fl, Wt, b, cent, labels, case[6])
    assert all(torch.equal(x, y) and int(x.sum()) > 0 for x, y in zip(a, c))


@pytest.mark.parametrize("skip", ["linear", "cluster"])
def test_skipped_probe_reads_nothing_of_it(skip):
    """Through the C ABI with real buffers: the skipped probe keeps a nonzero n and passes NULL weights and counts."""
    from stego_amd import capi
    case = CASES[1]
    B, K, h, w, H, W, n_lin, n_clu, _ = case
    code, fl, Wt, b, cent, labels = _setup(case)
    both = _counts(code, fl, Wt, b, cent, labels, n_lin)
    cn = F.normalize(cent, dim=1)
    out = torch.zeros(n_clu if skip == "linear" else n_lin, n_lin, dtype=torch.int64, device=DEV)
    desc = capi.probe_confusion_desc(B, K, h, w, H, W, n_lin, n_clu, skip != "linear", skip != "cluster", 2.0, n_lin)
    args = (None, None, cn, labels, None, out) if skip == "linear" else (Wt, b, None, labels, out, None)
    with torch.cuda.device(DEV):
        rc = capi.probe_confusion_raw(desc, capi._map(code), capi._map(fl), *args, stream=capi._stream())
    torch.cuda.synchronize()
    assert rc == 0, capi.load().stego_error_string(rc)
    assert torch.equal(out, both[1] if skip == "linear" else both[0])


@pytest.mark.parametrize("pattern", ["constant", "checkerboard"])
def test_all_lanes_in_one_bin(pattern):
    """A constant code and a constant label: every lane of every wave holds the same bin, the extreme of the wave aggregation; a
    checkerboard label gives every wave two bins."""
    B, K, h, w, H, W, n = 2, 70, 8, 8, 64, 64, 27
    code, _, Wt, b, cent = [t.to(DEV) for t in _inputs(B, K, h, w, n, n, seed=31)]
    code = code[:, :, :1, :1].expand(B, K, h, w).contiguous()
    labels = torch.full((B, H, W), 3, dtype=torch.int64, device=DEV)
    if pattern == "checkerboard":
        yy, xx = torch.meshgrid(torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
        labels = (3 + 2 * ((yy + xx) % 2)).expand(B, H, W).contiguous()
    got = _counts(code, None, Wt, b, cent, labels, n)
    t32 = _chain(code, None, Wt, b, cent, (H, W))
    for g, lp in zip(got, t32):
        pred = lp.argmax(1)
        assert all(len(pred[i].unique()) == 1 for i in range(B))                 # one prediction per image: one or two bins per wave
        assert torch.equal(g.cpu(), _bincount(pred, labels, n, n))
        assert int(g.sum()) == B * H * W and int((g > 0).sum()) <= 2 * B


@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (2, 27, 37, 53), (2, 64, 37, 53), (1, 5, 1, 7)], ids=lambda s: "x".join(map(str, s)))
def test_confusion_against_torch(shape):
    from stego_amd import capi
    B, n, H, W = shape
    n_classes = max(n - 2, 2)
    g = torch.Generator().manual_seed(sum(shape))
    scores = (torch.randn(B, n, H, W, generator=g) * 4).round() / 4                  # multiples of 0.25: ties are frequent
    labels = torch.randint(-1, n_classes + 2, (B, H, W), generator=g)
    am = scores.argmax(1)
    assert ((scores == scores.amax(1, keepdim=True)).sum(1) > 1).any() or n * H * W < 64
    want = _bincount(am, labels, n, n_classes)
    counts = torch.zeros(n, n_classes, dtype=torch.int64, device=DEV)
    capi.confusion(scores.to(DEV), labels.to(DEV), counts, "scores")
    assert torch.equal(counts.cpu(), want), int((counts.cpu() - want).abs().sum())
    # label maps, with predictions outside [0, n) on both sides
    pred = torch.randint(-2, n + 3, (B, H, W), generator=g)
    counts = torch.zeros(n, n_classes, dtype=torch.int64, device=DEV)
    capi.confusion(pred.to(DEV), labels.to(DEV), counts, "labels")
    assert torch.equal(counts.cpu(), _bincount(pred, labels, n, n_classes))
    assert int(counts.sum()) < B * H * W or H * W < 64
    capi.confusion(pred.to(DEV), labels.to(DEV), counts, "labels")                   # adds onto
    assert torch.equal(counts.cpu(), 2 * _bincount(pred, labels, n, n_classes))


def test_repeatable():
    from stego_amd import capi
    case = CASES[0]
    code, fl, Wt, b, cent, labels = _setup(case)
    a = _counts(code, fl, Wt, b, cent, labels, case[6])
    c = _counts(code, fl, Wt, b, cent, labels, case[6])
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    g = torch.Generator().manual_seed(5)
    scores = torch.randn(2, 27, 96, 96, generator=g).to(DEV)
    pred = torch.randint(0, 27, (2, 96, 96), generator=g).to(DEV)
    for p, kind in ((scores, "scores"), (pred, "labels")):
        runs = []
        for _ in range(2):
            counts = torch.zeros(27, 27, dtype=torch.int64, device=DEV)
            capi.confusion(p, labels, counts, kind)
            runs.append(counts)
        assert torch.equal(*runs) and int(runs[0].sum()) > 0, kind


def _tiny_model(*extra):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=2", "dim=70", "dropout=False",
                                 "extra_clusters=1"] + list(extra))
    torch.manual_seed(0)
    model = LitUnsupervisedSegmenter(27, cfg).to(DEV).eval()
    loader = torch.utils.data.DataLoader(SyntheticContrastiveDataset(8, 64, 27, seed=3), 4, shuffle=False)
    return model, loader


N_PIX = 8 * 64 * 64


@pytest.mark.parametrize("run_crf", [False, True])
def test_evaluate_native_metrics_matches_the_fused_head(run_crf):
    from stego_amd.eval_segmentation import evaluate
    from stego_amd.metrics import DeviceUnsupervisedMetrics
    model, loader = _tiny_model()
    ref_metrics = evaluate(model, loader, run_crf=run_crf, fused_head=True)
    ref = (model.test_linear_metrics.stats.clone(), model.test_cluster_metrics.stats.clone())
    got_metrics = evaluate(model, loader, run_crf=run_crf, native_metrics=True)
    assert isinstance(model.test_linear_metrics, DeviceUnsupervisedMetrics)
    got = (model.test_linear_metrics.stats.clone(), model.test_cluster_metrics.stats.clone())
    for a, b in zip(got, ref):
        assert int(a.sum()) == int(b.sum()) > 0
        if run_crf:                                      # the CRF's own float order may differ between runs
            assert int((a - b).abs().sum()) // 2 <= 0.001 * N_PIX, (a - b).abs().sum()
        else:
            assert torch.equal(a, b), (a - b).abs().sum()
    if not run_crf:
        assert got_metrics == ref_metrics


def test_update_scores_equals_argmax_plus_update_on_one_crf_output():
    from stego_amd.crf import dense_crf_batch, image_to_bgr_u8
    from stego_amd.metrics import DeviceUnsupervisedMetrics
    from stego_amd.segment import probe_head
    from stego_amd.utils import UnsupervisedMetrics
    model, loader = _tiny_model()
    batch = next(iter(loader))
    img, label = batch["img"].to(DEV), batch["label"].to(DEV)
    with torch.no_grad():
        _, c1 = model.net(img)
        _, c2 = model.net(img.flip(dims=[3]))
        probs = probe_head(model, c1, c2, img.shape[-2:], linear="probs", cluster="probs")
        bgr = image_to_bgr_u8(img)
        for p, extra, hungarian in zip(probs, (0, 1), (False, True)):
            q = dense_crf_batch(bgr, p)
            ref, dev = UnsupervisedMetrics("m/", 27, extra, hungarian), DeviceUnsupervisedMetrics("m/", 27, extra, hungarian)
            ref.update(q.argmax(1), label)
            dev.update_scores(q, label)
            assert dev.device_stats is not None and dev.device_stats.is_cuda
            assert torch.equal(dev.stats, ref.stats) and int(ref.stats.sum()) > 0
            assert dev.compute() == ref.compute()


def test_validation_step_native_metrics():
    ref_model, loader = _tiny_model("n_images=2")
    model, _ = _tiny_model("n_images=2", "native_metrics=True")
    n_valid = 0
    for i, batch in enumerate(loader):
        batch = {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in batch.items()}
        ref_out = ref_model.validation_step(batch, i)
        out = model.validation_step(batch, i)
        n_valid += int(((batch["label"] >= 0) & (batch["label"] < 27)).sum())
        for k in ("linear_preds", "cluster_preds"):
            assert out[k].shape == (2, 64, 64) and out[k].dtype == torch.int64 and not out[k].is_cuda
            assert (out[k] == ref_out[k]).float().mean().item() >= 0.999, k
        assert torch.equal(out["label"], ref_out["label"]) and out["img"].shape[0] == 2
    for name in ("linear_metrics", "cluster_metrics"):
        m, r = getattr(model, name), getattr(ref_model, name)
        # between reset() and compute() the whole state is the device matrix: every counted pixel is in it
        assert m.device_stats is not None and m.device_stats.is_cuda
        on_device = int(m.device_stats.sum())
        a, b = m.stats.clone(), r.stats
        assert on_device == int(a.sum()) == int(b.sum())
        assert int((a - b).abs().sum()) // 2 <= 0.001 * N_PIX, (a - b).abs().sum()
        m.compute()
        m.reset()
        assert int(m.device_stats.sum()) == 0 and int(m.stats.sum()) == 0
    assert n_valid == N_PIX
