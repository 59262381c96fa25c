"""The cluster refit without a GPU: the C ABI's surface and host checks (include/stego_kmeans.h), the torch chain against the float64
oracle of tests/kmeans_oracle.py, kmeans_fit's fallback on planted clusters, and a refitted model through its checkpoint."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import kmeans_oracle as O
from stego_amd import capi, cluster_refit

A = 0x10000          # an aligned stand-in address: the checks reject before any pointer is read
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stego_kmeans.h")).read()


def test_symbols_abi_and_error_constants():
    lib = capi.load()
    for name in ("stego_kmeans_workspace_bytes", "stego_kmeans_plan", "stego_kmeans_step", "stego_kmeans_seed"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, HEADER), name
    assert lib.stego_abi_version() == 7 == capi.ABI_VERSION
    names = ("DIM", "SIZE", "DRAW")
    for name in names:
        rc = getattr(capi, "KMEANS_ERR_" + name)
        assert re.search(r"STEGO_ERR_KMEANS_%s = %d\b" % (name, rc), HEADER), name
        assert lib.stego_error_string(rc).decode().startswith("kmeans:"), rc
    assert len(re.findall(r"STEGO_ERR_KMEANS_\w+ = \d+", HEADER)) == len(names)
    assert (capi.KMEANS_ERR_DIM, capi.KMEANS_ERR_SIZE, capi.KMEANS_ERR_DRAW) == (180, 181, 182)
    for name in ("MAX_K", "MAX_N", "FOLD", "TILE", "MAX_WORKGROUPS"):
        assert re.search(r"#define STEGO_KMEANS_%s %d\b" % (name, getattr(capi, "KMEANS_" + name)), HEADER), name
    assert capi.KMEANS_MAX_N == capi.PROBE_MAX_N and capi.KMEANS_FOLD == 1024


def test_descriptor_fields_follow_the_header():
    body = re.search(r"typedef struct StegoKmeansDesc \{(.*?)\} StegoKmeansDesc;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            fields += [(ctype, n.strip()) for n in rest.split(",")]
    assert [(ctypes.c_int32, n) for c, n in fields if c == "int32_t"] == [(t, n) for n, t in capi.StegoKmeansDesc._fields_]
    assert len(fields) == 5


def _desc(**kw):
    d = dict(B=3, K=70, h=7, w=5, n=27)
    d.update(kw)
    return capi.kmeans_desc(**d)


def _u(*values):
    return (ctypes.c_double * len(values))(*values)


BAD = [
    (dict(K=0), capi.KMEANS_ERR_DIM), (dict(K=129), capi.KMEANS_ERR_DIM), (dict(n=0), capi.KMEANS_ERR_DIM), (dict(n=65), capi.KMEANS_ERR_DIM),
    (dict(B=0), capi.KMEANS_ERR_SIZE), (dict(B=65536), capi.KMEANS_ERR_SIZE), (dict(h=0), capi.KMEANS_ERR_SIZE),
    (dict(w=-1), capi.KMEANS_ERR_SIZE),
    (dict(B=2, h=32768, w=32768), capi.KMEANS_ERR_SIZE),                 # 2^31 tokens
    (dict(B=1, h=65536, w=65536), capi.KMEANS_ERR_SIZE),                 # h * w alone leaves 32 bits
    (dict(B=65535, h=2 ** 31 - 1, w=2 ** 31 - 1), capi.KMEANS_ERR_SIZE),
]


@pytest.mark.parametrize("kw,rc", BAD)
def test_descriptor_checks_come_first(kw, rc):
    d = _desc(**kw)
    m = capi.StegoMap(A, 1, 1, 1, 1)
    assert capi.kmeans_workspace_bytes(d) == 0
    assert capi.kmeans_plan(d) == (0, 0)
    for null in (True, False):                      # with NULL pointers the code is the descriptor's too: nothing was enqueued
        p = None if null else A
        assert capi.kmeans_step_raw(d, None if null else m, p, p, p, p, p, p, 1 << 40) == rc
        assert capi.kmeans_seed_raw(d, None if null else m, None if null else _u(*([0.5] * 64)), p, p, p, 1 << 40) == rc


def test_good_descriptors_pointer_checks_and_draws():
    assert capi.kmeans_workspace_bytes(_desc(B=1, K=1, h=1, w=1, n=1)) > 0
    assert capi.kmeans_workspace_bytes(_desc(B=1, K=128, h=46340, w=46340, n=64)) >= 4 * 46340 ** 2      # best_p of every token
    assert capi.kmeans_workspace_bytes(_desc(B=65535, K=128, h=181, w=181, n=64)) > 0                    # 2 147 090 235 tokens
    d, m = _desc(), capi.StegoMap(A, 1, 1, 1, 1)
    need = capi.kmeans_workspace_bytes(d)
    assert capi.load().stego_kmeans_step(None, None, A, A, A, A, A, A, need, None) == 1
    assert capi.kmeans_step_raw(d, None, A, A, A, A, A, A, need) == 1
    assert capi.kmeans_step_raw(d, capi.StegoMap(0, 1, 1, 1, 1), A, A, A, A, A, A, need) == 1
    assert capi.kmeans_step_raw(d, m, None, A, A, A, A, A, need) == 1
    assert capi.kmeans_step_raw(d, m, A, A, A, None, A, A, need) == 1               # counts
    assert capi.kmeans_step_raw(d, m, A, A, A, A, None, A, need) == 1               # stats
    assert capi.kmeans_step_raw(d, m, A, A, A, A, A, None, need) == 1               # the workspace
    assert capi.kmeans_step_raw(d, m, A, None, None, A, A, A, need - 1) == 4        # NULL centroids_out and labels are legal
    assert capi.kmeans_step_raw(d, m, A, A, A, A, A, A, need - 1) == 4
    assert capi.kmeans_step_raw(d, m, A + 2, A, A, A, A, A, need) == 5
    assert capi.kmeans_step_raw(d, m, A, A, A + 1, A + 4, A, A, need) == 5          # labels are bytes; counts at 4 mod 8
    assert capi.kmeans_step_raw(d, m, A, A, A, A, A + 4, A, need) == 5
    assert capi.kmeans_step_raw(d, m, A, A, A, A, A, A + 8, need) == 5              # the workspace at 8 mod 16
    good = _u(*([0.25] * 27))
    assert capi.kmeans_seed_raw(d, None, good, A, A, A, need) == 1
    assert capi.kmeans_seed_raw(d, m, None, A, A, A, need) == 1
    assert capi.kmeans_seed_raw(d, m, good, None, A, A, need) == 1
    assert capi.kmeans_seed_raw(d, m, good, A, None, A, need) == 1
    assert capi.kmeans_seed_raw(d, m, good, A, A, A, need - 1) == 4
    assert capi.kmeans_seed_raw(d, m, good, A, A + 4, A, need) == 5
    for bad in (1.0, -1e-300, float("nan"), 2.0):                                  # the draws are read on the host, last of all checks
        u = [0.25] * 27
        u[26] = bad
        assert capi.kmeans_seed_raw(d, m, _u(*u), A, A, A, need) == capi.KMEANS_ERR_DRAW, bad
        assert capi.kmeans_seed_raw(d, m, _u(*u), A, A, A, need - 1) == 4


def test_plan_and_workspace_sizes():
    lds, wgs = capi.kmeans_plan(_desc())                                           # 105 tokens: one tile, one workgroup
    fixed = 256 * 8 + 128 * 4 + 64 * 4
    assert wgs == 1 and lds == fixed + 70 * (64 + 129) * 4
    lds, wgs = capi.kmeans_plan(_desc(B=2, h=40, w=40, K=128, n=64))               # 3200 tokens: 25 tiles
    assert wgs == 25 and lds == fixed + 128 * (64 + 129) * 4 <= 160 * 1024
    lds, wgs = capi.kmeans_plan(_desc(B=5000, h=28, w=28, K=33))                   # an odd K is staged as 34 rows
    assert wgs == 511 and lds == fixed + 34 * (64 + 129) * 4                       # 30625 tiles, 60 per workgroup
    step = 511 * (27 * 33 * 8 + 27 * 8 + 8)
    assert step <= capi.kmeans_workspace_bytes(_desc(B=5000, h=28, w=28, K=33)) == -(-5000 * 784 * 4 // 16) * 16 + 2 * 1024 * 8
    small = capi.kmeans_workspace_bytes(_desc(K=128, n=64))                        # 105 tokens: the step's single partial is the larger
    assert small >= 64 * 128 * 8 + 64 * 8 + 8 + 2 * 64 * 8


def _gauss(B, h, w, K, seed):
    return np.random.default_rng(seed).standard_normal((B, K, h, w)).astype(np.float32)


@pytest.mark.parametrize("shape", [(3, 7, 5, 70, 27), (2, 9, 9, 33, 2), (1, 1, 1, 70, 1), (2, 6, 6, 130, 70)])
def test_torch_step_against_the_oracle(shape):
    B, h, w, K, n = shape
    x = _gauss(B, h, w, K, 1)
    x[0, :, 0, 0] = 0                                                             # a zero-norm token
    cent = np.random.default_rng(2).standard_normal((n, K)).astype(np.float32)
    if n > 2:
        cent[2] = cent[1]                                                         # a tie: the lower index wins, the higher keeps its row
    want = O.step(x, cent)
    got = cluster_refit.kmeans_step(torch.from_numpy(x), torch.from_numpy(cent), labels=True)      # a CPU tensor takes the torch chain
    sure = want["gap"] >= 1e-5
    assert got.labels.dtype == torch.uint8 and tuple(got.labels.shape) == (B, h, w)
    assert np.array_equal(got.labels.numpy().ravel()[sure], want["labels"][sure]) and sure.mean() >= 0.9
    assert got.labels[0, 0, 0] == 0
    assert np.array_equal(got.counts.numpy(), np.bincount(got.labels.numpy().ravel(), minlength=n))
    new, kept, shift = O.update(x, cent, got.labels.numpy().ravel().astype(np.int64))
    assert np.abs(got.centroids.numpy() - new).max() < 1e-5
    stats = got.stats.numpy()
    assert abs(stats[0] - want["objective"]) <= B * h * w * (K + 3) * 2.0 ** -24
    assert stats[1] == kept.sum() and abs(stats[2] - shift) < 1e-5 and stats[3] == B * h * w
    if n > 2:
        assert kept[2] and got.counts[2] == 0
    only = cluster_refit.torch_kmeans_step(torch.from_numpy(x), torch.from_numpy(cent), update=False)
    assert only.centroids is None and only.labels is None and torch.equal(only.counts, got.counts) and only.stats[0] == got.stats[0]
    out = torch.from_numpy(cent.copy())
    same = cluster_refit.torch_kmeans_step(torch.from_numpy(x), out, out=out)
    assert same.centroids is out and torch.equal(out, got.centroids)


@pytest.mark.parametrize("shape", [(3, 7, 5, 70, 5), (2, 12, 12, 33, 9)])
def test_torch_seed_against_the_oracle(shape):
    B, h, w, K, n = shape
    x = _gauss(B, h, w, K, 3)
    x[1, :, 2, 3] = 0
    zero = (1 * h + 2) * w + 3
    u = np.random.default_rng(4).random(n)
    want = O.seed(x, n, u, snap=True)
    assert want["margin"] >= 1e-5 and zero not in want["picks"]
    cent, picks = cluster_refit.kmeans_seed(torch.from_numpy(x), n, u=want["u"])
    assert np.array_equal(picks.numpy(), want["picks"])
    assert np.abs(cent.numpy() - want["centroids"]).max() <= 3 * 2.0 ** -24
    g = torch.Generator().manual_seed(5)
    drawn = cluster_refit.kmeans_seed(torch.from_numpy(x), n, generator=g)
    again = O.seed(x, n, torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(5)).numpy())
    assert np.array_equal(drawn[1].numpy(), again["picks"])                       # the draw stream is torch.rand's, float64
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        cluster_refit.torch_kmeans_seed(torch.from_numpy(x), n, u=[1.0] * n)


def test_seed_with_fewer_distinct_tokens_than_clusters():
    x = np.zeros((1, 8, 2, 3), dtype=np.float32)
    x[0, 0, 0, :] = 1.0                                                           # three equal tokens and three zero ones
    x[0, 1, 1, 0] = 2.0
    want = O.seed(x, 4, [0.1, 0.6, 0.5, 0.9])                                      # round 2 on: no weight left, round 0's weights
    cent, picks = cluster_refit.kmeans_seed(torch.from_numpy(x), 4, u=[0.1, 0.6, 0.5, 0.9])
    assert np.array_equal(picks.numpy(), want["picks"]) and set(picks.tolist()) <= {0, 1, 2, 3}
    assert picks[1] == 3 and np.abs(cent.numpy() - want["centroids"]).max() == 0
    nothing = cluster_refit.kmeans_seed(torch.zeros(1, 4, 2, 2), 2, u=[0.3, 0.7])
    assert nothing[1].tolist() == [0, 0] and not nothing[0].any()


def test_fit_on_the_cpu_recovers_planted_clusters():
    x, which = O.planted()
    g = torch.Generator().manual_seed(0)
    u = torch.rand(5, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).numpy()
    start = O.seed(x, 5, u)
    assert len(set(which[start["picks"]].tolist())) == 5                           # the oracle's seeding picks one token per direction
    cent, labels, _ = O.fit(x, start["centroids"])
    assert O.same_partition(labels, which)
    res = cluster_refit.kmeans_fit(torch.from_numpy(x), 5, n_iter=30, generator=g, check_every=3)
    assert res.converged and res.n_iter % 3 == 0 and res.n_iter < 30 and len(res.history) == res.n_iter
    assert np.abs(res.centroids.numpy() - cent).max() < 1e-5
    assert res.counts.tolist() == np.bincount(labels, minlength=5).tolist() and int(res.counts.sum()) == 105
    assert abs(res.objective - O.step(x, cent)["objective"]) < 1e-3
    assert all(b >= a - 1e-3 for a, b in zip(res.history, res.history[1:]))
    given = cluster_refit.kmeans_fit(torch.from_numpy(x), 5, n_iter=30, init=torch.from_numpy(start["centroids"]).float())
    assert np.abs(given.centroids.numpy() - cent).max() < 1e-5
    best = cluster_refit.kmeans_fit(torch.from_numpy(x), 5, n_iter=30, n_init=3, generator=torch.Generator().manual_seed(7))
    assert best.objective >= res.objective - 1e-3
    wide = cluster_refit.kmeans_fit(torch.from_numpy(x).double(), 70, n_iter=2)     # another dtype, n > 64: never an error
    assert wide.centroids.shape == (70, 70) and wide.n_iter == 2 and int(wide.counts.sum()) == 105
    with pytest.raises(ValueError, match="init"):
        cluster_refit.kmeans_fit(torch.from_numpy(x), 5, init="random")


def _tiny_model(**kw):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    ov = ["model_type=vit_tiny", "dino_patch_size=16", "res=32", "batch_size=2", "dim=12", "dropout=False"] + ["%s=%s" % (k, v) for k, v in kw.items()]
    torch.manual_seed(1)
    return LitUnsupervisedSegmenter(5, load_config(overrides=ov)).cpu()


def test_a_model_without_the_key_is_built_as_before():
    model = _tiny_model(extra_clusters=2)
    assert not hasattr(model.cfg, "cluster_probe_n")
    assert model.cluster_probe.clusters.shape == (7, 12) and model.train_cluster_probe.clusters.shape == (5, 12)
    assert model.cluster_metrics.extra_clusters == model.test_cluster_metrics.extra_clusters == 2
    assert model.cluster_metrics.stats.shape == (7, 5)
    model.check_cluster_scoring()
    assert "cluster_probe_n" not in model.checkpoint_dict()["hyper_parameters"]["cfg"]
    for name in os.listdir(os.path.join(ROOT, "stego_amd", "configs")):
        if name != "refit_config.yml":
            assert "cluster_probe_n" not in open(os.path.join(ROOT, "stego_amd", "configs", name)).read(), name


@pytest.mark.parametrize("n", [8, 3])
def test_a_refitted_model_round_trips_through_its_checkpoint(tmp_path, n):
    from stego_amd.eval_segmentation import evaluate
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter
    model = _tiny_model()
    model._cluster_to_class = np.arange(5)
    imgs = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(2))
    codes = cluster_refit.collect_codes(model, [imgs[:2], {"img": imgs[2:]}])
    assert tuple(codes.shape) == (3, 12, 2, 2) and codes.is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        model.eval()
        want = (model.net(imgs)[1] + model.net(imgs.flip(dims=[3]))[1].flip(dims=[3])) / 2
    assert torch.allclose(codes, want, atol=1e-6)
    res = cluster_refit.refit_cluster_probe(model, codes, n, n_iter=5, generator=torch.Generator().manual_seed(3))
    assert model.cfg.cluster_probe_n == n and model.cluster_probe.clusters.shape == (n, 12) and model.cluster_to_class is None
    assert torch.equal(model.cluster_probe.clusters.detach(), res.centroids)
    assert model.cluster_metrics.extra_clusters == model.test_cluster_metrics.extra_clusters == max(n - 5, 0)
    assert model.cluster_metrics.stats.shape == (max(n, 5), 5)
    assert any(p is model.cluster_probe.clusters for p in model.optimizers()[2].param_groups[0]["params"])
    path = str(tmp_path / "refit.ckpt")
    model.save_checkpoint(path)
    back = LitUnsupervisedSegmenter.load_from_checkpoint(path, strict=True)
    assert back.cfg.cluster_probe_n == n and torch.equal(back.cluster_probe.clusters, model.cluster_probe.clusters)
    assert back.test_cluster_metrics.extra_clusters == max(n - 5, 0) and back.cluster_to_class is None
    assert not back.load_result.missing_keys and not back.load_result.unexpected_keys
    if n < 5:
        with pytest.raises(ValueError, match="cluster_probe_n"):
            back.check_cluster_scoring()
        with pytest.raises(ValueError, match="cluster_probe_n"):
            evaluate(back, [], run_crf=False)
        with pytest.raises(ValueError, match="cluster_probe_n"):
            back.validation_step({"img": imgs, "label": torch.zeros(3, 32, 32, dtype=torch.int64)}, 0)
    else:
        back.check_cluster_scoring()
