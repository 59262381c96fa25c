"""Feature pictures without a GPU: the float64 oracle against sklearn, the torch chain against the oracle, the C ABI's surface and
host checks (include/stego_pca.h), and a comparison sheet with a features row."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import feature_pca_oracle as O
from stego_amd import capi, feature_pca, render

A = 0x10000          # an aligned stand-in address: the checks reject before any pointer is read
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stego_pca.h")).read()
SIZES = [(40, 56), (37, 53), (18, 523), (5, 17), (1, 1), None]


def _map(B, h, w, C, joint, **kw):
    return np.ascontiguousarray(O.planted_map(B, h, w, C, joint, **kw).transpose(0, 3, 1, 2))


def test_oracle_equals_sklearn():
    decomposition = pytest.importorskip("sklearn.decomposition")
    x = _map(1, 5, 7, 70, False, seed=3)
    mean, cov, basis, stats = O.fit(x, False)
    t = O.tokens(x, False)[0]
    pca = decomposition.PCA(3, svd_solver="full").fit(t)
    assert np.abs(pca.components_ - basis[0]).max() < 1e-6            # sklearn centres on the float64 mean, the oracle on its float32
    assert np.abs(pca.explained_variance_ - stats[0, :, 0]).max() < 1e-5
    assert np.abs(pca.explained_variance_ - [16, 8, 4]).max() < 1e-4  # the planted spectrum
    s, _ = O.scores(x, mean, basis)
    assert np.abs(pca.transform(t) - s.reshape(-1, 3)).max() < 1e-5


def test_oracle_spectrum_is_the_planted_one():
    for joint, shape in ((False, (2, 5, 7, 70)), (True, (2, 24, 24, 33)), (False, (1, 2, 2, 3))):
        x = _map(*shape, joint)
        cov = O.fit(x, joint)[1]
        for g in range(cov.shape[0]):
            lam = np.linalg.eigvalsh(cov[g])[::-1]
            r = min(lam.size, (shape[0] if joint else 1) * shape[1] * shape[2] - 1)
            assert np.abs(lam[:r] - O.spectrum(r)).max() < 1e-4, (shape, g)


@pytest.mark.parametrize("scale", ["unit", "range"])
@pytest.mark.parametrize("resize", ["bilinear", "nearest"])
@pytest.mark.parametrize("size", SIZES)
def test_torch_chain_against_the_oracle(scale, resize, size):
    # eight images fitted jointly: in "range" mode the two extreme tokens of a component sit exactly at 0 and 255, and only among
    # 8 * 35 tokens are they less than 1 % of a nearest-neighbour picture
    x = _map(8, 5, 7, 70, True, seed=6, gain=0.125 if scale == "unit" else 1.0)
    want, a = O.pictures(x, True, size, scale, resize)
    got = feature_pca.torch_feature_pictures(torch.from_numpy(x), size, True, scale, resize)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    share = O.byte_rule(got.numpy(), a)
    assert share <= 0.01, share
    if scale == "unit":
        assert ((a < 0) | (a > 255)).any() or size == (1, 1)          # the clamp is exercised
    same = feature_pca.feature_pictures(torch.from_numpy(x), size, True, scale, resize)         # a CPU tensor takes the torch chain
    assert torch.equal(same, got)


def test_torch_fit_against_the_oracle_and_fixed_model():
    x = _map(3, 6, 6, 33, True, seed=2)
    mean, cov, basis, stats = O.fit(x, True)
    pca = feature_pca.fit(torch.from_numpy(x), joint=True)
    assert pca.groups == 1 and pca.basis.shape == (1, 3, 33) and pca.stats.shape == (1, 3, 3)
    assert np.abs(pca.mean.numpy() - mean).max() == 0
    assert np.abs(pca.basis.numpy() - basis).max() < 1e-5
    assert np.abs(pca.stats.numpy()[..., :2] - stats[..., :2]).max() < 1e-4
    other = _map(2, 5, 7, 33, True, seed=5)
    s, rng = O.scores(other, pca.mean.numpy(), pca.basis.numpy())
    assert np.abs(pca.scores(torch.from_numpy(other)).numpy() - s).max() < 1e-4
    want, a = O.pictures(other, True, (20, 28), "range", "bilinear", model=(pca.mean.numpy(), pca.basis.numpy()))
    got = feature_pca.feature_pictures(torch.from_numpy(other), (20, 28), scale="range", pca=pca)
    assert O.byte_rule(got.numpy(), a) <= 0.01
    with pytest.raises(ValueError, match="per-image model"):
        feature_pca.feature_pictures(torch.from_numpy(other), pca=feature_pca.fit(torch.from_numpy(x)))      # 3 images' model, 2 images


def test_degenerate_maps_on_the_host():
    const = torch.full((2, 5, 3, 4), 0.7)
    pca = feature_pca.fit(const)
    assert not pca.basis.any() and not pca.stats.any()
    assert (feature_pca.feature_pictures(const, (9, 9)) == 127).all()
    rank2 = torch.from_numpy(_map(1, 5, 7, 33, False, seed=4, rank=2, gain=0.125))
    pca = feature_pca.fit(rank2)
    assert pca.basis[0, :2].abs().sum() > 0 and not pca.basis[0, 2].any() and not pca.stats[0, 2].any()
    assert (feature_pca.feature_pictures(rank2, (9, 9))[..., 2] == 127).all()


def test_symbols_abi_and_error_constants():
    lib = capi.load()
    for name in ("stego_pca_workspace_bytes", "stego_pca_fit", "stego_pca_scores", "stego_pca_paint"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, HEADER), name
    names = ("DIM", "SIZE", "ITER", "MODE")
    for name in names:
        rc = getattr(capi, "PCA_ERR_" + name)
        assert re.search(r"STEGO_ERR_PCA_%s = %d\b" % (name, rc), HEADER), name
        assert lib.stego_error_string(rc).decode().startswith("pca:"), rc
    assert len(re.findall(r"STEGO_ERR_PCA_\w+ = \d+", HEADER)) == len(names)
    for name in ("PER_IMAGE", "JOINT", "BILINEAR", "NEAREST", "UNIT", "RANGE"):
        assert re.search(r"STEGO_PCA_%s = %d\b" % (name, getattr(capi, "PCA_" + name)), HEADER), name
    for name in ("MAX_C", "MAX_SIDE", "MAX_ITER", "DEFAULT_ITER", "FOLD"):
        assert re.search(r"#define STEGO_PCA_%s %d\b" % (name, getattr(capi, "PCA_" + name)), HEADER), name
    assert re.search(r"#define STEGO_PCA_MAX_TOKENS \(1 << 28\)", HEADER) and capi.PCA_MAX_TOKENS == 1 << 28


def test_descriptor_fields_follow_the_header():
    body = re.search(r"typedef struct StegoPcaDesc \{(.*?)\} StegoPcaDesc;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            fields += [(ctype, n.strip()) for n in rest.split(",")]
    ctypes_of = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    assert [(ctypes_of[c], n) for c, n in fields] == [(t, n) for n, t in capi.StegoPcaDesc._fields_]


def _desc(**kw):
    d = dict(B=2, C=70, h=5, w=7, H=40, W=56, joint=False, n_iter=32, resize=capi.PCA_BILINEAR, scale=capi.PCA_UNIT,
             out_strides=(40 * 56 * 3, 56 * 3))
    d.update(kw)
    return capi.pca_desc(**d)


BAD = [
    (dict(C=2), capi.PCA_ERR_DIM), (dict(C=769), capi.PCA_ERR_DIM),
    (dict(B=0), capi.PCA_ERR_SIZE), (dict(B=65536), capi.PCA_ERR_SIZE),
    (dict(h=0), capi.PCA_ERR_SIZE), (dict(w=4097), capi.PCA_ERR_SIZE),
    (dict(B=65535, h=4096, w=2), capi.PCA_ERR_SIZE),                     # more than 2^28 tokens
    (dict(B=5, h=1, w=3), capi.PCA_ERR_SIZE),                            # three tokens in a per-image group
    (dict(B=1, h=1, w=3, joint=True), capi.PCA_ERR_SIZE),
    (dict(H=0), capi.PCA_ERR_SIZE), (dict(W=32769), capi.PCA_ERR_SIZE),
    (dict(n_iter=0), capi.PCA_ERR_ITER), (dict(n_iter=257), capi.PCA_ERR_ITER),
    (dict(joint=2), capi.PCA_ERR_MODE), (dict(resize=2), capi.PCA_ERR_MODE), (dict(scale=-1), capi.PCA_ERR_MODE),
]


@pytest.mark.parametrize("kw,rc", BAD)
def test_descriptor_checks_come_first(kw, rc):
    d = _desc(**kw)
    m = capi.StegoMap(A, 1, 1, 1, 1)
    assert capi.pca_workspace_bytes(d) == 0
    for null in (True, False):                      # with NULL pointers the code is the descriptor's too: nothing was enqueued
        p = None if null else A
        assert capi.pca_fit_raw(d, None if null else m, p, p, p, p, p, 1 << 40) == rc
        assert capi.pca_scores_raw(d, None if null else m, p, p, p, p, p, 1 << 40) == rc
        assert capi.pca_paint_raw(d, p, p, p) == rc


def test_good_descriptors_and_pointer_checks():
    assert capi.pca_workspace_bytes(_desc(B=4, h=1, w=1, joint=True)) > 0          # four tokens in a joint group
    assert capi.pca_workspace_bytes(_desc(C=3, B=1, h=2, w=2)) > 0
    assert capi.pca_workspace_bytes(_desc(C=768, n_iter=256, B=65535, h=2, w=2)) > 0
    d, m = _desc(), capi.StegoMap(A, 1, 1, 1, 1)
    need = capi.pca_workspace_bytes(d)
    assert capi.load().stego_pca_fit(None, None, A, A, A, A, A, need, None) == 1
    assert capi.pca_fit_raw(d, None, A, A, A, A, A, need) == 1
    assert capi.pca_fit_raw(d, m, A, None, A, A, A, need) == 1
    assert capi.pca_fit_raw(d, m, A, A, A, A, A, need - 1) == 4
    assert capi.pca_fit_raw(d, m, A, A + 4, A, A, A, need) == 5                     # cov at 4 mod 8
    assert capi.pca_fit_raw(d, m, A, A, A, A, A + 8, need) == 5                     # the workspace at 8 mod 16
    assert capi.pca_scores_raw(d, m, A, A, None, A, A, need) == 1
    assert capi.pca_scores_raw(d, m, A, A, A, A, A, need - 1) == 4
    assert capi.pca_scores_raw(d, m, A, A + 2, A, A, A, need) == 5
    assert capi.pca_paint_raw(d, A, None, None) == 1                                # no target
    assert capi.pca_paint_raw(_desc(scale=capi.PCA_RANGE), A, None, A) == 1         # RANGE selected, no range
    assert capi.pca_paint_raw(d, A + 2, None, A + 1) == 5


def test_workspace_is_bounded_for_joint_fits():
    tiles = 300 * 8192                                                              # the 32 x 32 fp64 tiles with j >= i at C = 768
    small = capi.pca_workspace_bytes(_desc(C=768, B=16, h=40, w=40, joint=True))
    large = capi.pca_workspace_bytes(_desc(C=768, B=4096, h=256, w=256, joint=True))
    assert 13 * tiles <= small <= large <= 16 * tiles + 256 * 768 * 8 + 64         # 13 slabs of 2048 tokens; 16 at the most
    per_image = capi.pca_workspace_bytes(_desc(C=768, B=16, h=40, w=40))            # one slab per image: as many tiles as cov has
    assert 16 * tiles <= per_image <= 16 * tiles + 256 * 768 * 8 + 64


def test_limits_are_named():
    with pytest.raises(ValueError, match="768"):
        feature_pca._check_limits(1, 769, 4, 4, False)
    with pytest.raises(ValueError, match="tokens in a group"):
        feature_pca._check_limits(2, 8, 1, 3, False)
    with pytest.raises(ValueError, match="n_iter"):
        feature_pca._check_limits(2, 8, 4, 4, False, n_iter=0)
    with pytest.raises(ValueError, match="scale"):
        feature_pca.feature_pictures(torch.zeros(1, 3, 2, 2), scale="minmax")


def test_comparison_sheet_with_a_features_row():
    cmap = render.cityscapes_colormap()
    lab = torch.arange(2 * 4 * 5).reshape(2, 4, 5) % 27
    img = torch.randn(2, 3, 4, 5, generator=torch.Generator().manual_seed(0))
    feats = torch.from_numpy(_map(2, 2, 3, 8, True, seed=6))
    row = {"features": feats, "size": (4, 5), "joint": True, "scale": "range", "resize": "nearest"}
    plain = render.comparison_sheet([{"image": img}, {"image": img}, {"labels": lab, "cmap": cmap}], pad=2, background=(1, 2, 3))
    sheet = render.comparison_sheet([{"image": img}, row, {"labels": lab, "cmap": cmap}], pad=2, background=(1, 2, 3))
    assert sheet.shape == plain.shape == (2 + 3 * 6, 2 + 2 * 7, 3)
    panels = feature_pca.feature_pictures(feats, (4, 5), joint=True, scale="range", resize="nearest")
    mask = torch.ones(sheet.shape[:2], dtype=torch.bool)
    for b in range(2):
        assert torch.equal(sheet[8:12, 2 + 7 * b:7 + 7 * b], panels[b])
        mask[8:12, 2 + 7 * b:7 + 7 * b] = False
    assert torch.equal(sheet[mask], plain[mask])                                   # the other rows and the background: the same bytes
    alone = render.comparison_sheet([{"features": feats}], pad=1)
    assert alone.shape == (1 + 3, 1 + 2 * 4, 3)
