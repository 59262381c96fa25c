"""csrc/probe_head.hip on the MI355X against the reference's torch chain (flip average, F.interpolate bilinear, the 1x1 linear probe,
ClusterLookup's normalised einsum, log_softmax) in fp32 and in float64: the fp32-class bars, the hard inputs (zero vectors,
opposite neighbours, scaled magnitudes), the consistency of the three output kinds, bitwise repeatability, and segment() /
evaluate(fused_head=True) against the composition evaluate() runs without the flag."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _inputs(B, K, h, w, n_lin, n_clu, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    code = torch.randn(B, K, h, w, generator=g) * scale
    flip = torch.randn(B, K, h, w, generator=g) * scale
    W = torch.randn(n_lin, K, generator=g) / K ** 0.5
    b = torch.randn(n_lin, generator=g) * 0.1
    cent = torch.randn(n_clu, K, generator=g)
    return code, flip, W, b, cent


def _chain(code, flip, W, b, cent, size, alpha=2.0):
    """eval_segmentation.py:124-128 of the reference, in the inputs' dtype and on their device."""
    c = (code + flip.flip(dims=[3])) / 2 if flip is not None else code
    c = F.interpolate(c, size, mode="bilinear", align_corners=False)
    lin = torch.log_softmax(F.conv2d(c, W[:, :, None, None], b), dim=1)
    inner = torch.einsum("bchw,nc->bnhw", F.normalize(c, dim=1), F.normalize(cent, dim=1))
    return lin, torch.log_softmax(inner * alpha, dim=1)


def _kernel(code, flip, W, b, cent, size, kind="log_probs", alpha=2.0):
    from stego_amd import capi
    return capi.probe_head(code, flip, W.to(DEV), b.to(DEV), F.normalize(cent.to(DEV), dim=1), size, kind, kind, alpha)


def _check(code, flip, W, b, cent, size, bar=1e-4):
    d = [t.to(DEV) if t is not None else None for t in (code, flip, W, b, cent)]
    t32 = _chain(*d, size)
    t64 = _chain(*[t.double() if t is not None else None for t in d], size)
    k = _kernel(*d, size)
    torch.cuda.synchronize()
    for name, kk, tt, dd in zip(("linear", "cluster"), k, t32, t64):
        assert kk.shape == tt.shape, (name, kk.shape, tt.shape)
        assert torch.isfinite(kk).all(), name
        vs_torch = (kk - tt).abs().max().item()
        err_k = (kk.double() - dd).abs().max().item()
        err_t = (tt.double() - dd).abs().max().item()
        assert vs_torch <= bar, (name, vs_torch)
        assert err_k <= 2 * err_t + 1e-6, (name, err_k, err_t)


CASES = [  # B, K, h, w, H, W, n_lin, n_clu, flip
    (2, 70, 40, 40, 320, 320, 27, 27, True),
    (3, 16, 37, 53, 291, 419, 27, 27, True),
    (2, 70, 40, 40, 24, 24, 27, 27, True),
    (2, 64, 20, 24, 160, 192, 27, 28, False),
    (2, 90, 20, 20, 160, 160, 3, 64, True),
    (1, 128, 17, 23, 136, 184, 64, 3, False),
    (2, 70, 12, 12, 96, 96, 28, 28, False),
    (2, 70, 20, 20, 160, 160, 7, 5, True),          # probe_head_kernel<8>: the plan's NMAX is 8 when max(n_lin, n_clu) <= 8
    (2, 32, 15, 17, 121, 135, 12, 16, False),       # probe_head_kernel<16>: 8 < max(n_lin, n_clu) <= 16
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_K%d_%dx%d_%dx%d_n%d+%d_%s" % (c[:8] + ("flip" if c[8] else "noflip",)))
def test_log_probs_against_torch_and_float64(case):
    B, K, h, w, H, W, n_lin, n_clu, flip = case
    code, fl, Wt, b, cent = _inputs(B, K, h, w, n_lin, n_clu, seed=sum(case[:8]))
    _check(code, fl if flip else None, Wt, b, cent, (H, W))


def test_channels_last_strided_code():
    """The head's channels-last views go in without a copy (strides (h w K, 1, w K, K))."""
    code, fl, Wt, b, cent = _inputs(2, 70, 40, 40, 27, 27, seed=5)
    cl = code.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    fcl = fl.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert cl.stride(1) == 1 and not cl.is_contiguous()
    _check(cl, fcl, Wt, b, cent, (320, 320))
    a = _kernel(cl, fcl, Wt, b, cent, (320, 320))
    c = _kernel(cl.contiguous(), fcl.contiguous(), Wt, b, cent, (320, 320))
    assert all(torch.equal(x, y) for x, y in zip(a, c))          # the layout changes nothing: same values, same bits


def test_zero_vectors_take_the_eps_branch():
    code, fl, Wt, b, cent = _inputs(2, 70, 16, 16, 27, 27, seed=7)
    code[:, :, 4:9, 3:10] = 0                       # a block of zero vectors: whole output regions interpolate zeros only
    code[1] = 0
    _check(code, None, Wt, b, cent, (128, 128))
    _, clu = _kernel(code.to(DEV), None, Wt, b, cent, (128, 128))
    torch.testing.assert_close(clu[1], torch.full_like(clu[1], -float(np.log(27))), atol=1e-6, rtol=0)


def test_opposite_neighbours():
    """A checkerboard of v and -v: the interpolated vector nearly cancels between the source pixels (down to 1/64 of |v| at 8x, 1/16
    at 4x).  (At a ratio whose weights make the sum cancel exactly, any fp32 chain returns rounding noise, torch's included: no bar.)"""
    B, K, h, w = 2, 70, 10, 10
    code, _, Wt, b, cent = _inputs(B, K, h, w, 27, 27, seed=11)
    sign = torch.tensor([[(-1.0) ** (y + x) for x in range(w)] for y in range(h)])
    code = code[:, :, :1, :1] * sign                # one vector per image, alternating sign
    _check(code, None, Wt, b, cent, (80, 80))
    _check(code, None, Wt, b, cent, (40, 40))


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_scaled_magnitudes(scale):
    code, fl, Wt, b, cent = _inputs(2, 70, 20, 20, 27, 27, seed=13, scale=scale)
    # at 1e3 the linear logits are ~1e3 and fp32 log-probs carry ~1e-4 of rounding in torch as well: the bar scales with them
    _check(code, fl, Wt, b, cent, (160, 160), bar=1e-4 * max(1.0, scale / 10))


def test_probs_argmax_consistent_and_repeatable():
    code, fl, Wt, b, cent = _inputs(3, 70, 40, 40, 27, 28, seed=17)
    code, fl = code.to(DEV), fl.to(DEV)
    lp = _kernel(code, fl, Wt, b, cent, (320, 320), "log_probs")
    pr = _kernel(code, fl, Wt, b, cent, (320, 320), "probs")
    am = _kernel(code, fl, Wt, b, cent, (320, 320), "argmax")
    t32 = _chain(code, fl, Wt.to(DEV), b.to(DEV), cent.to(DEV), (320, 320))
    for i in range(2):
        assert (lp[i].exp() - pr[i]).abs().max().item() <= 1e-6
        assert am[i].dtype == torch.int64 and am[i].shape == (3, 320, 320)
        assert torch.equal(am[i], lp[i].argmax(1))
        top2 = t32[i].topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 1e-4
        assert clear.float().mean().item() > 0.99
        assert torch.equal(am[i][clear], t32[i].argmax(1)[clear])
    for kind, first in (("log_probs", lp), ("probs", pr), ("argmax", am)):
        again = _kernel(code, fl, Wt, b, cent, (320, 320), kind)
        assert all(torch.equal(x, y) for x, y in zip(first, again)), kind


def test_mixed_kinds_and_a_skipped_probe():
    from stego_amd import capi
    code, fl, Wt, b, cent = _inputs(2, 70, 40, 40, 27, 27, seed=19)
    code, fl = code.to(DEV), fl.to(DEV)
    lp = _kernel(code, fl, Wt, b, cent, (320, 320), "log_probs")
    cn = F.normalize(cent.to(DEV), dim=1)
    lin, clu = capi.probe_head(code, fl, Wt.to(DEV), b.to(DEV), cn, (320, 320), "argmax", None, 2.0)
    assert clu is None and torch.equal(lin, lp[0].argmax(1))
    lin, clu = capi.probe_head(code, fl, Wt.to(DEV), b.to(DEV), cn, (320, 320), None, "probs", 2.0)
    assert lin is None and (clu - lp[1].exp()).abs().max().item() <= 1e-6


@pytest.mark.parametrize("skip", ["linear", "cluster"])
def test_skipped_probe_reads_nothing_of_it(skip):
    """Through the C ABI with real buffers: a skipped probe keeps a nonzero n (27) and passes NULL weights and output.  The kernel
    must not touch them, and the other probe's output equals, bit for bit, a run that computes both probes."""
    from stego_amd import capi
    code, fl, Wt, b, cent = _inputs(2, 70, 40, 40, 27, 28, seed=23)
    code, fl, Wt, b = code.to(DEV), fl.to(DEV), Wt.to(DEV), b.to(DEV)
    cn = F.normalize(cent.to(DEV), dim=1)
    both = capi.probe_head(code, fl, Wt, b, cn, (320, 320), "log_probs", "log_probs", 2.0)
    lk = capi.PROBE_SKIP if skip == "linear" else capi.PROBE_LOG_PROBS
    ck = capi.PROBE_SKIP if skip == "cluster" else capi.PROBE_LOG_PROBS
    out = torch.full((2, 27 if skip == "cluster" else 28, 320, 320), float("nan"), device=DEV)
    desc = capi.probe_desc(2, 70, 40, 40, 320, 320, 27, 28, lk, ck, 2.0)
    if skip == "linear":
        args = (None, None, cn, None, out)
    else:
        args = (Wt, b, None, out, None)
    with torch.cuda.device(DEV):
        rc = capi.probe_head_raw(desc, capi._map(code), capi._map(fl), *args, stream=capi._stream())
    torch.cuda.synchronize()
    assert rc == 0, capi.load().stego_error_string(rc)
    assert torch.equal(out, both[1] if skip == "linear" else both[0])


def _tiny_model():
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=2", "dim=70", "dropout=False",
                                 "extra_clusters=1"])
    torch.manual_seed(0)
    model = LitUnsupervisedSegmenter(27, cfg).to(DEV).eval()
    loader = torch.utils.data.DataLoader(SyntheticContrastiveDataset(8, 64, 27, seed=3), 4, shuffle=False)
    return model, loader


@pytest.mark.parametrize("run_crf", [False, True])
def test_segment_against_the_existing_composition(run_crf):
    from stego_amd.crf import _probs_at, batched_crf, dense_crf_batch, image_to_bgr_u8
    from stego_amd.segment import probe_head, segment
    model, loader = _tiny_model()
    for batch in loader:
        img = batch["img"].to(DEV)
        lin, clu = segment(model, img, run_crf=run_crf)
        with torch.no_grad():
            _, c1 = model.net(img)
            _, c2 = model.net(img.flip(dims=[3]))
            code = F.interpolate((c1 + c2.flip(dims=[3])) / 2, img.shape[-2:], mode="bilinear", align_corners=False)
            lp = torch.log_softmax(model.linear_probe(code), dim=1)
            cp = model.cluster_probe(code, 2, log_probs=True)
            if run_crf:
                ql, qc = batched_crf(None, img, lp), batched_crf(None, img, cp)
                pl, pc = probe_head(model, c1, c2, img.shape[-2:], linear="probs", cluster="probs")
                bgr = image_to_bgr_u8(img)
                assert (dense_crf_batch(bgr, pl) - ql).abs().max().item() <= 1e-3
                assert (dense_crf_batch(bgr, pc) - qc).abs().max().item() <= 1e-3
                assert (pl - _probs_at(lp, *img.shape[-2:])).abs().max().item() <= 1e-5
                ref_l, ref_c = ql.argmax(1), qc.argmax(1)
            else:
                ref_l, ref_c = lp.argmax(1), cp.argmax(1)
        assert lin.shape == ref_l.shape and lin.dtype == torch.int64
        for got, ref in ((lin, ref_l), (clu, ref_c)):
            agree = (got == ref).flatten(1).float().mean(1)
            assert agree.min().item() >= 0.999, agree


@pytest.mark.parametrize("run_crf", [False, True])
def test_evaluate_fused_head_matches(run_crf):
    from stego_amd.eval_segmentation import evaluate
    model, loader = _tiny_model()
    stats = []
    for fused in (False, True):
        evaluate(model, loader, run_crf=run_crf, fused_head=fused)
        stats.append((model.test_linear_metrics.stats.clone(), model.test_cluster_metrics.stats.clone()))
    n_pix = 8 * 64 * 64
    for a, b in zip(*stats):
        assert int(a.sum()) == int(b.sum())
        assert int((a - b).abs().sum()) // 2 <= 0.001 * n_pix, (a - b).abs().sum()


def test_fused_crf_runs_at_the_image_size():
    """evaluate(fused_head=True, run_crf=True) asks the kernel for the image's size, where the CRF runs, whatever the label's."""
    from stego_amd.eval_segmentation import _fused_preds
    model, loader = _tiny_model()
    img = next(iter(loader))["img"].to(DEV)
    with torch.no_grad():
        _, c1 = model.net(img)
        _, c2 = model.net(img.flip(dims=[3]))
    a = _fused_preds(model, img, c1, c2, (32, 32), True)
    b = _fused_preds(model, img, c1, c2, img.shape[-2:], True)
    assert a[0].shape == img.shape[:1] + img.shape[-2:]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
