"""The dense CRF without a GPU: the numpy restatement (tests/crf_oracle.py) against the exact Gaussian filter and the mean-field's
properties, the reference's image conversion, the host-side checks of stego_amd.crf and of the C ABI (include/stego_crf.h), and the
register / spill guard of csrc/dense_crf.hip."""
import ctypes

import numpy as np
import pytest
import torch

import crf_oracle as O
from stego_amd import _build


def _lattice_vs_exact(d, scale, seed=0, n=1500):
    rng = np.random.default_rng(seed)
    f = rng.uniform(0, 3, (n, d)).astype(np.float32)
    x = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    exact = O.symmetric(lambda v: O.exact_gaussian_filter(f, v), x)
    lat = O.symmetric(O.Lattice(f * np.float32(scale)).filter, x)
    return float(np.linalg.norm(lat - exact) / np.linalg.norm(exact))


@pytest.mark.parametrize("d,bound", [(2, 0.02), (5, 0.03)])
def test_lattice_approximates_exact_gaussian(d, bound):
    """Symmetric-normalised lattice filter vs exp(-|fi - fj|^2 / 2), 1500 uniform points in [0, 3)^d, positive values: relative L2
    0.0117 (d = 2) and 0.0196 (d = 5) measured; features scaled by 2 or 1/2 give 0.05 - 0.17 - the embedding's scale is the
    Gaussian's."""
    err = _lattice_vs_exact(d, 1.0)
    assert err < bound, err
    for s in (2.0, 0.5):
        worse = _lattice_vs_exact(d, s)
        assert worse > 2.4 * err and worse > bound, (s, worse, err)


def test_embedding_invariants():
    """Barycentric weights sum to 1 and are >= 0; every vertex key is a remainder-r point (coordinates congruent mod d+1)."""
    rng = np.random.default_rng(1)
    for d in (2, 5):
        f = rng.uniform(-20, 20, (4000, d)).astype(np.float32)
        keys, bary = O.embed(f)
        np.testing.assert_allclose(bary.sum(1), 1.0, atol=1e-5)
        assert bary.min() > -1e-6
        for r in range(d + 1):
            assert (np.mod(keys[:, r, :], d + 1) == r).all()


def _flat_case(n_iter, pos_w=O.POS_W, bi_w=O.Bi_W):
    H = W = 24
    bgr = np.full((H, W, 3), 120, np.uint8)
    lab = np.zeros((H, W), np.int64)
    lab[:, W // 2:] = 1
    noisy = lab.copy()
    for (y, x) in [(5, 5), (17, 8), (11, 19)]:
        noisy[y, x] = 1 - noisy[y, x]
    p = np.where(np.arange(2)[:, None, None] == noisy[None], 0.7, 0.3).astype(np.float32)
    return bgr, p, lab, noisy, O.dense_crf(bgr, p, n_iter=n_iter, pos_w=pos_w, bi_w=bi_w)


def test_mean_field_zero_weights_is_softmax_of_unary():
    rng = np.random.default_rng(2)
    bgr = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    p = rng.dirichlet(np.ones(5), size=99).T.reshape(5, 9, 11).astype(np.float32)
    expect = O.softmax(np.log(np.clip(p, 1e-5, 1)), 0)
    for it in (0, 1, 4):
        q = O.dense_crf(bgr, p, n_iter=it, pos_w=0.0, bi_w=0.0)
        np.testing.assert_allclose(q, expect, atol=1e-6)


def test_mean_field_sums_to_one_and_removes_isolated_pixels():
    bgr, p, lab, noisy, q = _flat_case(O.MAX_ITER)
    np.testing.assert_allclose(q.sum(0), 1.0, atol=1e-5)
    assert (noisy != lab).sum() == 3
    assert (q.argmax(0) == lab).all()
    _, _, _, _, q0 = _flat_case(O.MAX_ITER, pos_w=0.0, bi_w=0.0)
    assert (q0.argmax(0) != lab).sum() == 3           # without the pairwise terms they stay


def test_reference_image_conversion():
    """utils.unnorm -> to_pil_image (x * 255 truncated) -> [:, :, ::-1] on hand-computed pixels."""
    from stego_amd import crf
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    rgb = np.array([[[10.7, 200.2], [0.5, 254.6]], [[99.9, 3.3], [128.5, 254.9]], [[47.3, 180.6], [1.2, 0.4]]])   # [3, 2, 2] in 0..255
    img = torch.tensor((rgb / 255.0 - mean[:, None, None]) / std[:, None, None], dtype=torch.float32)
    out = crf._to_bgr_u8(img)
    assert out.shape == (1, 2, 2, 3) and out.dtype == torch.uint8
    expect = np.floor(rgb).astype(np.uint8).transpose(1, 2, 0)[:, :, ::-1]     # truncated (fractions away from the float round trip's error)
    np.testing.assert_array_equal(out[0].numpy(), expect)
    # out-of-range values are clamped, not wrapped
    extreme = torch.tensor([[[-9.0]], [[9.0]], [[0.0]]])
    assert crf._to_bgr_u8(extreme)[0, 0, 0].tolist() == [int(0.406 * 255), 255, 0]


def test_crf_rejects_bad_inputs_on_host():
    from stego_amd import crf
    u8 = torch.zeros(1, 4, 5, 3, dtype=torch.uint8)
    p = torch.full((1, 3, 4, 5), 1.0 / 3)
    with pytest.raises(ValueError):
        crf.dense_crf_batch(u8.float(), p)
    with pytest.raises(ValueError):
        crf.dense_crf_batch(u8, p.double())
    with pytest.raises(ValueError):
        crf.dense_crf_batch(u8[:, :3], p)
    with pytest.raises(ValueError):
        crf.dense_crf_batch(u8, torch.zeros(1, 65, 4, 5))
    with pytest.raises(RuntimeError, match="MI355X"):
        crf.dense_crf_batch(u8, p)                    # valid, but on the CPU: no fallback
    with pytest.raises(RuntimeError, match="MI355X"):
        crf.batched_crf(None, torch.zeros(1, 3, 4, 5), p)
    with pytest.raises(RuntimeError, match="MI355X"):
        crf.dense_crf(torch.zeros(3, 4, 5), p[0])


def _desc(**kw):
    from stego_amd import capi
    a = dict(B=16, C=27, H=320, W=320, n_iter=10, pos_w=3, pos_xy_std=1, bi_w=4, bi_xy_std=67, bi_rgb_std=3)
    a.update(kw)
    return capi.crf_desc(**a)


def test_workspace_bytes_and_error_codes_through_ctypes():
    from stego_amd import capi
    lib = capi.load()
    ws = capi.crf_workspace_bytes(_desc())
    N, Cp = 320 * 320, 28
    vals = 16 * 2 * (3 + 6) * N * Cp * 4                      # the two [M, C_pad] value buffers of both lattices, worst case M
    assert vals < ws < 2 * vals, ws
    assert capi.crf_workspace_bytes(_desc(B=8)) < ws
    assert capi.crf_workspace_bytes(_desc(B=1, C=1, H=1, W=1)) > 0
    for kw, code in [({"C": 0}, capi.CRF_ERR_LIMITS), ({"C": 65}, capi.CRF_ERR_LIMITS), ({"H": 20000, "W": 20000}, capi.CRF_ERR_LIMITS),
                     ({"H": 0}, 2), ({"B": 65536}, 2), ({"n_iter": -1}, 2), ({"bi_rgb_std": 0.0}, 2), ({"pos_xy_std": float("nan")}, 2),
                     ({"bi_rgb_std": 0.05}, capi.CRF_ERR_RANGE), ({"H": 3000, "W": 3000, "bi_xy_std": 1.0}, capi.CRF_ERR_RANGE)]:
        d = _desc(**kw)
        assert capi.crf_workspace_bytes(d) == 0, kw
        # every check is on the host, before anything touches a device: null pointers never get used
        assert lib.stego_crf_run(ctypes.byref(d), None, None, None, None, 0, None) == code, kw
    d = _desc(B=1, H=8, W=8)
    assert lib.stego_crf_run(ctypes.byref(d), None, None, None, None, 0, None) == 1          # STEGO_ERR_NULL
    assert b"dense CRF" in lib.stego_error_string(capi.CRF_ERR_LIMITS)
    assert b"dense CRF" in lib.stego_error_string(capi.CRF_ERR_RANGE)


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_crf_kernels_do_not_spill():
    """Every kernel of csrc/dense_crf.hip keeps its working set in registers (the embedding's per-pixel arrays are indexed by
    unrolled compares, not through private memory) at full occupancy but for the combine kernel."""
    kernels = _build.kernel_resources("dense_crf.hip")
    ours = {k: v for k, v in kernels.items() if "9stego_crf" in k}
    # embed / emit / neighbours x 2 lattices, count, scan, norm x 2, splat / blur x 2 / unary / combine x 5 group widths
    assert len(ours) == 3 * 2 + 2 + 2 + 5 * 5, sorted(ours)
    for k, v in ours.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= (4 if "combine" in k else 8), (k, v)
