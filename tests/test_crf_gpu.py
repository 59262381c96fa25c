"""csrc/dense_crf.hip on the MI355X against tests/crf_oracle.py, both in fp32: lattice keys and vertex counts equal, Q within fp32-class
bars, argmax equal; the eval shape (B = 16, 320^2, C = 27) on per-pixel colour noise (M ~ 6N, the worst case) and on a smooth scene;
bitwise repeatability; the reference's entry points (crf.dense_crf / batched_crf, eval_segmentation.evaluate)."""
import multiprocessing as mp
import warnings

import numpy as np
import pytest
import torch

import crf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _probs(rng, B, C, H, W, sharp=3.0):
    lg = rng.standard_normal((B, C, H, W)).astype(np.float32) * sharp
    e = np.exp(lg - lg.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def _smooth_scene(rng, H, W, C):
    """Gradients plus flat blocks (closer to natural images than noise), with logits that follow the blocks."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([xx * 255 / max(W - 1, 1), yy * 255 / max(H - 1, 1), np.full_like(xx, 128)], -1)
    lab = np.zeros((H, W), np.int64)
    for i in range(6):
        y0, x0 = rng.integers(0, H - H // 4), rng.integers(0, W - W // 4)
        h, w = rng.integers(H // 8, H // 3), rng.integers(W // 8, W // 3)
        img[y0:y0 + h, x0:x0 + w] = rng.integers(0, 256, 3)
        lab[y0:y0 + h, x0:x0 + w] = rng.integers(0, C)
    lg = rng.standard_normal((C, H, W)).astype(np.float32) * 1.5
    lg[lab, yy.astype(int), xx.astype(int)] += 2.0
    e = np.exp(lg - lg.max(0, keepdims=True))
    return img.astype(np.uint8), (e / e.sum(0, keepdims=True)).astype(np.float32)


def _case(kind, B, C, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8), _probs(rng, B, C, H, W)
    if kind == "flat":
        return np.full((B, H, W, 3), 77, np.uint8), _probs(rng, B, C, H, W, sharp=1.0)
    pairs = [_smooth_scene(rng, H, W, C) for _ in range(B)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _gpu(bgr, probs, keep=False, n_iter=O.MAX_ITER):
    from stego_amd import capi
    B, C, H, W = probs.shape
    desc = capi.crf_desc(B, C, H, W, n_iter, O.POS_W, O.POS_XY_STD, O.Bi_W, O.Bi_XY_STD, O.Bi_RGB_STD)
    out = capi.crf_run(desc, torch.from_numpy(bgr).to(DEV), torch.from_numpy(probs).to(DEV), keep_workspace=keep)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), out[1], desc) if keep else out.cpu().numpy()


def _oracle(bgr, probs, workers=1):
    jobs = [(bgr[b], probs[b]) for b in range(len(bgr))]
    if workers <= 1 or len(jobs) == 1:
        return np.stack([O.dense_crf_args(j) for j in jobs])
    with mp.get_context("spawn").Pool(workers) as pool:          # numpy only in the children: they never open the GPU
        return np.stack(pool.map(O.dense_crf_args, jobs))


# Bars, calibrated on the MI355X: mean-field amplifies last-bit differences (summation order, expf / logf) about a hundredfold over
# ten iterations on random unaries - the fp32 oracle itself differs from its float64 evaluation by 2.9e-5 on the 37x53, C = 27 noise
# case, where the kernels differ from it by 2.8e-5.  Observed maxima: 4.8e-5 (small shapes), 1.9e-4 (eval shape, noise), 8.3e-7 (eval
# shape, smooth scene).
ATOL_SMALL, ATOL_EVAL = 1e-4, 5e-4


def _compare(q, ref, atol, min_agree=1.0):
    """max |Q - Q_oracle| <= atol; argmax agreement >= min_agree, and every disagreement at a near-tie of the oracle (top-2 gap
    <= 2 atol: a last-bit difference may decide those either way)."""
    err = float(np.abs(q - ref).max())
    a, r = q.argmax(1), ref.argmax(1)
    srt = np.sort(ref, 1)
    gap = srt[:, -1] - srt[:, -2] if ref.shape[1] > 1 else np.full(a.shape, np.inf)
    agree = float((a == r).mean())
    assert err <= atol, err
    assert agree >= min_agree, agree
    assert (gap[a != r] <= 2 * atol).all(), gap[a != r]
    return err, agree


@pytest.mark.parametrize("H,W,C", [(1, 1, 3), (7, 13, 1), (7, 13, 27), (37, 53, 3), (37, 53, 27), (37, 53, 64), (16, 24, 64),
                                   (7, 13, 6), (37, 53, 12)])     # (iterate<G>: G = 1, 8, 16 above; G = 2 for 5 <= C <= 8, G = 4 for 9..16)
def test_small_shapes_match_oracle(H, W, C):
    bgr, probs = _case("noise", 2, C, H, W, seed=H * 1000 + W + C)
    q, ws, desc = _gpu(bgr, probs, keep=True)
    ref = _oracle(bgr, probs)
    _compare(q, ref, ATOL_SMALL)
    from stego_amd import capi
    for b in range(2):
        for which, lat in ((0, O.Lattice(O.gaussian_features(H, W, O.POS_XY_STD))),
                           (1, O.Lattice(O.bilateral_features(bgr[b], O.Bi_XY_STD, O.Bi_RGB_STD)))):
            M, keys = capi.crf_lattice_info(desc, ws, b, which, max_keys=lat.M + 1)
            assert M == lat.M, (b, which, M, lat.M)
            np.testing.assert_array_equal(keys, lat.keys)


def test_flat_colour_long_segments_match_oracle():
    """One colour: the bilateral lattice's points lie on a plane, each vertex collects thousands of records (cut into pieces)."""
    bgr, probs = _case("flat", 2, 27, 96, 128, seed=5)
    q, ws, desc = _gpu(bgr, probs, keep=True)
    from stego_amd import capi
    lat = O.Lattice(O.bilateral_features(bgr[0], O.Bi_XY_STD, O.Bi_RGB_STD))
    assert np.diff(lat.seg).max() > 64                                   # there are segments longer than one piece
    M, keys = capi.crf_lattice_info(desc, ws, 0, 1, max_keys=lat.M + 1)
    assert M == lat.M
    np.testing.assert_array_equal(keys, lat.keys)
    _compare(q, _oracle(bgr, probs), ATOL_SMALL)


def test_zero_iterations_and_zero_weights():
    from stego_amd import capi
    bgr, probs = _case("noise", 1, 5, 9, 11, seed=3)
    expect = O.softmax(np.log(np.clip(probs, 1e-5, 1)), 1)
    np.testing.assert_allclose(_gpu(bgr, probs, n_iter=0), expect, atol=1e-6)
    desc = capi.crf_desc(1, 5, 9, 11, 4, 0.0, 1.0, 0.0, 67.0, 3.0)
    q = capi.crf_run(desc, torch.from_numpy(bgr).to(DEV), torch.from_numpy(probs).to(DEV)).cpu().numpy()
    np.testing.assert_allclose(q, expect, atol=1e-6)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_eval_shape_batch_matches_oracle(kind):
    """B = 16 at 320^2, C = 27 (eval_config.yml res 320, 2 * batch_size).  Bars: Q within ATOL_EVAL, argmax >= 99.99 %."""
    bgr, probs = _case(kind, 16, 27, 320, 320, seed=11 if kind == "noise" else 12)
    q, ws, desc = _gpu(bgr, probs, keep=True)
    from stego_amd import capi
    Ms = [capi.crf_lattice_info(desc, ws, b, 1)[0] for b in range(16)]
    ref = _oracle(bgr, probs, workers=8)
    err, agree = _compare(q, ref, ATOL_EVAL, min_agree=0.9999)
    lat = O.Lattice(O.bilateral_features(bgr[0], O.Bi_XY_STD, O.Bi_RGB_STD))
    M, keys = capi.crf_lattice_info(desc, ws, 0, 1, max_keys=lat.M + 1)
    assert M == lat.M == Ms[0]
    np.testing.assert_array_equal(keys, lat.keys)
    print("\n[crf eval shape %s] max|dQ| %.3e  argmax agreement %.6f  bilateral M per image %d .. %d (N = %d)"
          % (kind, err, agree, min(Ms), max(Ms), 320 * 320))


def test_repeat_runs_are_bitwise_identical():
    for kind in ("noise", "flat"):
        bgr, probs = _case(kind, 3, 27, 37, 53, seed=8)
        a, b = _gpu(bgr, probs), _gpu(bgr, probs)
        assert np.array_equal(a, b), kind


def test_batched_crf_equals_per_image_dense_crf():
    from stego_amd import crf
    g = torch.Generator().manual_seed(4)
    img = torch.randn(3, 3, 40, 56, generator=g).to(DEV)
    logits = torch.log_softmax(torch.randn(3, 7, 20, 28, generator=g) * 2, 1).to(DEV)
    out = crf.batched_crf(None, img, logits)
    assert out.device == img.device and tuple(out.shape) == (3, 7, 40, 56)
    for b in range(3):
        one = crf.dense_crf(img[b], logits[b])
        assert isinstance(one, np.ndarray) and one.shape == (7, 40, 56)
        np.testing.assert_allclose(out[b].cpu().numpy(), one, rtol=0, atol=1e-6)
    # and the path from normalised image + logits is the oracle's on the converted inputs
    bgr = crf.image_to_bgr_u8(img).cpu().numpy()
    probs = torch.softmax(torch.nn.functional.interpolate(logits, size=(40, 56), mode="bilinear", align_corners=False), 1).cpu().numpy()
    _compare(out.cpu().numpy(), _oracle(bgr, probs), ATOL_SMALL)


def test_limits_return_error_codes():
    from stego_amd import capi
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    for C, std, code in [(65, 3.0, capi.CRF_ERR_LIMITS), (3, 0.05, capi.CRF_ERR_RANGE)]:
        p = torch.full((1, C, 8, 8), 1.0 / C, device=DEV)
        desc = capi.crf_desc(1, C, 8, 8, 10, 3, 1, 4, 67, std)
        with pytest.raises(RuntimeError, match="error %d" % code):
            capi.crf_run(desc, u8, p)
    torch.cuda.synchronize()
    _gpu(*_case("noise", 1, 3, 8, 8, seed=1))        # the device is fine afterwards


def _tiny_model():
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=2", "dim=10", "dropout=False"])
    torch.manual_seed(0)
    model = LitUnsupervisedSegmenter(27, cfg).to(DEV).eval()
    loader = torch.utils.data.DataLoader(SyntheticContrastiveDataset(4, 64, 27, seed=3), 4, shuffle=False)
    return model, loader


def test_evaluate_with_and_without_crf():
    from stego_amd import crf
    from stego_amd.eval_segmentation import evaluate
    model, loader = _tiny_model()
    seen = []
    upd = model.test_linear_metrics.update
    model.test_linear_metrics.update = lambda p, t: (seen.append(p.detach().cpu().numpy()), upd(p, t))
    plain = evaluate(model, loader, run_crf=False)
    with_crf = evaluate(model, loader, run_crf=True)
    keys = {"final/linear/mIoU", "final/linear/Accuracy", "final/cluster/mIoU", "final/cluster/Accuracy"}
    assert set(plain) == keys and set(with_crf) == keys
    assert all(np.isfinite(v) for v in with_crf.values())
    # the CRF predictions are the argmax of the oracle-refined linear log-probs of the same batch
    batch = next(iter(loader))
    img, label = batch["img"].to(DEV), batch["label"].to(DEV)
    with torch.no_grad():
        code = (model.net(img)[1] + model.net(img.flip(dims=[3]))[1].flip(dims=[3])) / 2
        code = torch.nn.functional.interpolate(code, label.shape[-2:], mode="bilinear", align_corners=False)
        lp = torch.log_softmax(model.linear_probe(code), dim=1)
        assert np.array_equal(seen[0], lp.argmax(1).cpu().numpy())        # (run_crf=False: the plain argmax)
        probs = crf._probs_at(lp, 64, 64).cpu().numpy()
    ref = _oracle(crf.image_to_bgr_u8(img).cpu().numpy(), probs)
    pred, r = seen[1], ref.argmax(1)
    srt = np.sort(ref, 1)
    gap = (srt[:, -1] - srt[:, -2])[pred != r]
    assert (gap <= 2 * ATOL_SMALL).all(), (int((pred != r).sum()), gap)
