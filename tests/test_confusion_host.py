"""The device-side confusion matrices without a GPU: every host check of stego_probe_confusion, stego_confusion and
stego_probe_confusion_plan (include/stego_confusion.h) returns its documented code before anything is launched, the tile plan fits its
LDS budget with the histograms in it, DeviceUnsupervisedMetrics equals UnsupervisedMetrics on CPU tensors, and the flag is off in both
shipped configs."""
import ctypes

import pytest
import torch

from stego_amd import capi

A = 0x10000          # a 256-byte aligned stand-in address: the checks reject before any pointer is read
NULL, ALIGN = 1, 5   # STEGO_ERR_NULL, STEGO_ERR_ALIGN


def _desc(**kw):
    d = dict(B=2, K=70, h=40, w=40, H=320, W=320, n_lin=27, n_clu=27, lin_on=1, clu_on=1, alpha=2.0, n_classes=27)
    d.update(kw)
    return capi.probe_confusion_desc(**d)


def _map(addr=A):
    return capi.StegoMap(addr, 70 * 1600, 1600, 40, 1)


def _rc(desc, code=None, flip=None, lw=A, lb=A, cent=A, labels=A, lc=A, cc=A):
    return capi.probe_confusion_raw(desc, _map() if code is None else code, flip, lw, lb, cent, labels, lc, cc)


@pytest.mark.parametrize("kw,rc", [
    (dict(K=0), capi.CONF_ERR_DIM), (dict(K=129), capi.CONF_ERR_DIM),
    (dict(n_lin=0), capi.CONF_ERR_DIM), (dict(n_lin=65), capi.CONF_ERR_DIM),
    (dict(n_clu=0), capi.CONF_ERR_DIM), (dict(n_clu=65), capi.CONF_ERR_DIM),
    (dict(n_classes=0), capi.CONF_ERR_DIM), (dict(n_classes=65), capi.CONF_ERR_DIM),
    (dict(B=0), capi.CONF_ERR_SIZE), (dict(B=65536), capi.CONF_ERR_SIZE),
    (dict(h=0), capi.CONF_ERR_SIZE), (dict(h=65536), capi.CONF_ERR_SIZE), (dict(w=0), capi.CONF_ERR_SIZE), (dict(w=65536), capi.CONF_ERR_SIZE),
    (dict(H=0), capi.CONF_ERR_SIZE), (dict(H=2049), capi.CONF_ERR_SIZE), (dict(W=0), capi.CONF_ERR_SIZE), (dict(W=2049), capi.CONF_ERR_SIZE),
    (dict(lin_on=0, clu_on=0), capi.CONF_ERR_PROBES), (dict(lin_on=2), capi.CONF_ERR_PROBES), (dict(clu_on=-1), capi.CONF_ERR_PROBES),
])
def test_probe_confusion_descriptor_checks(kw, rc):
    assert _rc(_desc(**kw)) == rc
    assert capi.probe_confusion_plan(_desc(**kw))[0] == 0


@pytest.mark.parametrize("which", ["desc", "code", "flip", "labels", "lw", "lb", "cent", "lc", "cc"])
def test_probe_confusion_null_pointers(which):
    if which == "desc":
        assert capi.load().stego_probe_confusion(None, ctypes.byref(_map()), None, A, A, A, A, A, A, None) == NULL
        return
    kw = {}
    if which in ("code", "flip"):
        kw[which] = _map(0)
    else:
        kw[which] = None
    assert _rc(_desc(), **kw) == NULL
    if which == "code":
        assert capi.probe_confusion_raw(_desc(), None, None, A, A, A, A, A, A) == NULL


def test_skipped_probe_ignores_its_labels_and_pointers():
    """A skipped probe's n, weights and counts are not checked.  Every call still fails a later check (a misaligned code pointer), so
    nothing is launched: reaching that check shows the skipped probe passed the ones before it."""
    for n in (0, 27, 99, -1):
        assert _rc(_desc(lin_on=0, n_lin=n), code=_map(A + 2), lw=None, lb=None, lc=None) == ALIGN
        assert _rc(_desc(clu_on=0, n_clu=n), code=_map(A + 2), cent=None, cc=None) == ALIGN
        assert capi.probe_confusion_plan(_desc(lin_on=0, n_lin=n))[0] > 0
    assert _rc(_desc(lin_on=0), lw=None, lb=None, lc=None, cc=None) == NULL      # the active probe's counts are still required
    assert _rc(_desc(clu_on=0), cent=None, cc=None, lc=None) == NULL


@pytest.mark.parametrize("which", ["code", "flip", "lw", "lb", "cent", "labels", "lc", "cc"])
def test_probe_confusion_misaligned_pointers(which):
    kw = {}
    if which in ("code", "flip"):
        kw[which] = _map(A + 2)
    else:
        kw[which] = A + 2
    assert _rc(_desc(), **kw) == ALIGN
    if which in ("labels", "lc", "cc"):                   # int64: 8-byte alignment
        assert _rc(_desc(), **{which: A + 4}) == ALIGN
    elif which in ("lw", "lb", "cent"):                   # float32: 4 bytes are enough; the call then fails on the next thing wrong
        assert _rc(_desc(), **{which: A + 4, "labels": A + 4}) == ALIGN


def _cdesc(**kw):
    d = dict(B=2, n=27, H=320, W=320, n_classes=27, pred_kind=capi.CONF_SCORES)
    d.update(kw)
    return capi.confusion_desc(**d)


@pytest.mark.parametrize("kw,rc", [
    (dict(n=0), capi.CONF_ERR_DIM), (dict(n=65), capi.CONF_ERR_DIM), (dict(n_classes=0), capi.CONF_ERR_DIM), (dict(n_classes=65), capi.CONF_ERR_DIM),
    (dict(B=0), capi.CONF_ERR_SIZE), (dict(H=0), capi.CONF_ERR_SIZE), (dict(W=-1), capi.CONF_ERR_SIZE),
    (dict(B=1 << 20, H=1 << 10, W=1 << 10), capi.CONF_ERR_SIZE),              # B * H * W = 2^40
    (dict(B=1, H=1 << 30, W=1 << 30), capi.CONF_ERR_SIZE),
    (dict(pred_kind=2), capi.CONF_ERR_KIND), (dict(pred_kind=-1), capi.CONF_ERR_KIND),
])
def test_confusion_descriptor_checks(kw, rc):
    assert capi.confusion_raw(_cdesc(**kw), A, A, A) == rc


def test_confusion_pointer_checks():
    assert capi.confusion_raw(None, A, A, A) == NULL
    for args in ((None, A, A), (A, None, A), (A, A, None)):
        assert capi.confusion_raw(_cdesc(), *args) == NULL
    for args in ((A + 2, A, A), (A, A + 4, A), (A, A, A + 4)):
        assert capi.confusion_raw(_cdesc(), *args) == ALIGN
    assert capi.confusion_raw(_cdesc(pred_kind=capi.CONF_LABELS), A + 4, A, A) == ALIGN       # int64 label maps: 8 bytes
    # the largest size the limit admits passes the size check: it fails on the alignment checked after it
    assert capi.confusion_raw(_cdesc(B=(1 << 20) - 1, H=1 << 10, W=1 << 10), A + 2, A, A) == ALIGN


def test_error_strings():
    lib = capi.load()
    for rc in (capi.CONF_ERR_DIM, capi.CONF_ERR_SIZE, capi.CONF_ERR_PROBES, capi.CONF_ERR_KIND):
        assert lib.stego_error_string(rc).decode().startswith("confusion:"), rc
    assert lib.stego_abi_version() == 7


@pytest.mark.parametrize("shape", [(40, 40, 320, 320), (37, 53, 291, 419), (40, 40, 24, 24), (1, 1, 2048, 2048), (2048, 2048, 7, 2048),
                                   (65535, 3, 1, 1), (3, 65535, 5, 2048), (40, 40, 1, 1)])
@pytest.mark.parametrize("K,n", [(70, 27), (128, 64), (1, 1)])
def test_plan_fits_lds_with_the_histograms(shape, K, n):
    h, w, H, W = shape
    lds, ty, tx = capi.probe_confusion_plan(_desc(K=K, n_lin=n, n_clu=n, n_classes=n, h=h, w=w, H=H, W=W))
    assert 2 * n * n * 4 < lds <= 64 * 1024, lds                     # both int32 histograms are inside the figure
    assert 1 <= ty * tx <= 256 and ty <= H and tx <= W, (ty, tx)
    head = capi.probe_head_plan(capi.probe_desc(2, K, h, w, H, W, n, n, capi.PROBE_ARGMAX, capi.PROBE_ARGMAX, 2.0))
    if (ty, tx) == head[1:]:                                          # same tile: the head's footprint plus histograms and parameters
        assert lds - head[0] >= 2 * n * n * 4
    one = capi.probe_confusion_plan(_desc(K=K, n_lin=n, n_clu=n, n_classes=n, h=h, w=w, H=H, W=W, clu_on=0))
    if (one[1], one[2]) == (ty, tx):
        assert lds - one[0] == n * n * 4                              # a skipped probe has no histogram


def test_plan_at_eval_shape():
    lds, ty, tx = capi.probe_confusion_plan(_desc())
    assert (ty, tx) == (4, 64)
    assert capi.probe_confusion_plan(_desc(n_classes=0))[0] == 0


# ---- the metrics class on CPU tensors
def _both(n_classes, extra, hungarian):
    from stego_amd.metrics import DeviceUnsupervisedMetrics
    from stego_amd.utils import UnsupervisedMetrics
    return UnsupervisedMetrics("m/", n_classes, extra, hungarian), DeviceUnsupervisedMetrics("m/", n_classes, extra, hungarian)


@pytest.mark.parametrize("n_classes,extra,hungarian", [(27, 0, False), (27, 0, True), (5, 3, True)])
def test_metrics_class_on_cpu(n_classes, extra, hungarian):
    ref, dev = _both(n_classes, extra, hungarian)
    g = torch.Generator().manual_seed(n_classes + extra)
    for _ in range(3):
        target = torch.randint(-1, n_classes + 2, (2, 24, 24), generator=g)
        target[0, 0, :5] = 255
        preds = torch.randint(0, n_classes + extra, (2, 24, 24), generator=g)            # predictions >= n_classes when extra > 0
        preds = torch.where(torch.rand(2, 24, 24, generator=g) < 0.6, target.clamp(0, n_classes - 1), preds)
        ref.update(preds, target)
        dev.update(preds, target)
    assert (target == -1).any() and (target == 255).any() and (extra == 0 or (preds >= n_classes).any())
    assert dev.stats.dtype == torch.int64 and dev.stats.shape == ref.stats.shape
    assert torch.equal(dev.stats, ref.stats) and int(ref.stats.sum()) > 0
    assert dev.compute() == ref.compute()
    scores = torch.randn(2, n_classes + extra, 24, 24, generator=g)
    ref.update(scores.argmax(1), target)
    dev.update_scores(scores, target)
    assert torch.equal(dev.stats, ref.stats)
    assert dev.device_stats is None                                    # CPU inputs never allocate device state
    dev.reset()
    assert int(dev.stats.sum()) == 0


# ---- config and wrappers
def test_flag_is_off_in_both_configs():
    from stego_amd.eval_segmentation import EVAL_CONFIG
    from stego_amd.train_segmentation import load_config
    assert load_config().native_metrics is False
    assert load_config(EVAL_CONFIG).native_metrics is False


def test_wrappers_refuse_bad_kinds_and_cpu_tensors():
    from stego_amd import metrics
    pred, lab, counts = torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="kinds"):
        capi.confusion(pred, lab, counts, "argmax")
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.confusion(pred, lab, counts, "labels")
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.probe_confusion(torch.zeros(1, 4, 2, 2), None, torch.zeros(3, 4), torch.zeros(3), None, lab, counts, None, 2.0)
    with pytest.raises(ValueError, match="both probes"):
        capi.probe_confusion(torch.zeros(1, 4, 2, 2), None, None, None, None, lab, None, None, 2.0)
    with pytest.raises(ValueError):
        metrics.probe_confusion(torch.nn.Module(), torch.zeros(1, 4, 2, 2), None, lab, None, None)
    with pytest.raises(TypeError):
        from stego_amd.utils import UnsupervisedMetrics
        metrics.probe_confusion(torch.nn.Module(), torch.zeros(1, 4, 2, 2), None, lab, UnsupervisedMetrics("m/", 3, 0, False), None)
