"""The cluster refit on the MI355X (csrc/code_kmeans.hip) against the float64 oracle of tests/kmeans_oracle.py.

Labels must equal the oracle's wherever its two largest similarities are at least 1e-5 apart: both vectors are unit vectors and the
products are accumulated exactly as fp32, so a similarity is off by at most (K + 3) * 2^-24 <= 7.8e-6 at K = 128.  Tokens inside
that margin may go either way; their share is asserted on the oracle (at most 1 %) before the kernel is compared.  The new centroids
are compared with the oracle's update computed from the kernel's own labels; the bound is 4 x the error of the torch fp32 CPU chain
(index_add_ + normalize) on the same input against the same oracle (another summation order), at least 1e-6."""
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import kmeans_oracle as O
from stego_amd import capi, cluster_refit

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STEP_SHAPES = [(3, 7, 5, 70, 27),          # ragged tile, the shipped K and n
               (2, 40, 40, 70, 33),        # crosses the 32-row centroid tile and the 1024-token fold
               (2, 40, 40, 128, 64),       # the limits
               (3, 7, 5, 3, 5),            # small K
               (1, 1, 1, 70, 1),           # one token, one cluster
               (2, 9, 9, 33, 2),           # odd K
               # kmeans_assign_kernel<NT, CT, DENSE>, NT = ceil(n / 32), CT = ceil(K / 32): the rows above reach <1,1> <1,2> <1,3> <2,3>
               # <2,4>; these the rest of dispatch_assign's table, each under the three layouts (DENSE and not)
               (2, 6, 5, 40, 5),           # <1,2> once more, K between the tiles
               (1, 9, 17, 128, 27),        # <1,4>: 153 tokens, a second 128-token tile of 25
               (2, 8, 9, 20, 40),          # <2,1>
               (3, 11, 13, 64, 64)]        # <2,2>: both counts at a tile's edge, 429 tokens in four tiles
SEED_SHAPES = [(3, 7, 5, 70, 5), (2, 40, 40, 70, 33)]
LAYOUTS = ["nchw", "cl", "cl_view"]
MARGIN = 1e-5


def _dev(x, layout):
    """numpy [B, K, h, w] -> the NCHW-contiguous device tensor, the dense channels-last view of the same values (read as one flat
    array), or the first K channels of a wider channels-last tensor (the strided read with a lane per channel)."""
    t = torch.from_numpy(x).to(DEV)
    if layout == "nchw":
        return t
    if layout == "cl":
        return t.contiguous(memory_format=torch.channels_last)
    B, K, h, w = t.shape
    wide = torch.full((B, h, w, K + 3), 7.0, device=DEV)
    wide[..., :K] = t.permute(0, 2, 3, 1)
    return wide[..., :K].permute(0, 3, 1, 2)


def _sim_bound(T, K):
    return T * (K + 3) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _step_case(shape):
    B, h, w, K, n = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal((B, K, h, w)).astype(np.float32)
    cent = rng.standard_normal((n, K)).astype(np.float32)
    want = O.step(x, cent)
    return x, cent, want


def _torch_chain_centroids(x, cent, labels):
    """The update of the torch fp32 CPU chain under the given labels: index_add_ + normalize; an empty cluster keeps its row."""
    xh = F.normalize(torch.from_numpy(O.tokens(x).astype(np.float32)), dim=1)
    ch = F.normalize(torch.from_numpy(cent), dim=1)
    sums = torch.zeros_like(ch).index_add_(0, torch.from_numpy(labels), xh)
    keep = (torch.bincount(torch.from_numpy(labels), minlength=ch.shape[0]) == 0) | ~(sums.norm(dim=1) > 0)
    return torch.where(keep[:, None], ch, F.normalize(sums, dim=1)).numpy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_against_the_oracle(shape, layout):
    B, h, w, K, n = shape
    T = B * h * w
    x, cent, want = _step_case(shape)
    sure = want["gap"] >= MARGIN
    assert 1.0 - sure.mean() <= 0.01, 1.0 - sure.mean()
    got = cluster_refit.kmeans_step(_dev(x, layout), torch.from_numpy(cent).to(DEV), labels=True)
    labels = got.labels.cpu().numpy().reshape(-1).astype(np.int64)
    counts, stats, new = got.counts.cpu().numpy(), got.stats.cpu().numpy(), got.centroids.cpu().numpy()
    assert got.labels.dtype == torch.uint8 and tuple(got.labels.shape) == (B, h, w) and labels.max() < n
    assert np.array_equal(labels[sure], want["labels"][sure]), (labels[sure] != want["labels"][sure]).sum()
    assert np.array_equal(counts, np.bincount(labels, minlength=n))
    assert stats[3] == T
    print(shape, layout, "unsure %.4f" % (1.0 - sure.mean()), "objective off %.2e (bound %.2e)" % (abs(stats[0] - want["objective"]), _sim_bound(T, K)))
    assert abs(stats[0] - want["objective"]) <= _sim_bound(T, K)
    ref, kept, shift = O.update(x, cent, labels)
    chain = np.abs(_torch_chain_centroids(x, cent, labels) - ref).max()
    err = np.abs(new - ref).max()
    print(shape, layout, "centroids off %.2e, torch fp32 chain %.2e, ratio %.2f" % (err, chain, err / max(chain, 1e-30)))
    assert err <= max(4 * chain, 1e-6), (err, chain)
    assert stats[1] == kept.sum() and abs(stats[2] - shift) <= 1e-5
    assert np.abs(np.linalg.norm(new.astype(np.float64), axis=1) - 1).max() < 1e-6


def _run(x, cent, out=None, labels=True, update=True):
    got = cluster_refit.kmeans_step(x, cent, out=out, labels=labels, update=update)
    torch.cuda.synchronize()
    return got


def test_identical_centroids_and_zero_tokens():
    x, cent, _ = _step_case(STEP_SHAPES[1])                 # 3200 tokens in 33 clusters: none is empty on its own
    x, cent = x.copy(), cent.copy()
    cent[3] = cent[1]                                       # every tie goes to the lower index; the higher one keeps its old row
    x[1, :, 2, 3] = 0                                       # a zero-norm token: cluster 0, counted, adds nothing
    zero = (1 * 40 + 2) * 40 + 3
    for layout in LAYOUTS:
        got = _run(_dev(x, layout), torch.from_numpy(cent).to(DEV))
        labels = got.labels.cpu().numpy().reshape(-1).astype(np.int64)
        assert not (labels == 3).any() and (labels == 1).any() and got.counts[3] == 0
        assert got.stats[1] == 1
        assert np.abs(got.centroids[3].cpu().numpy() - O.normalize(cent)[3]).max() <= 2.0 ** -24
        assert labels[zero] == 0
        ref, kept, _ = O.update(x, cent, labels)
        assert kept.tolist() == [j == 3 for j in range(33)]
        assert np.abs(got.centroids.cpu().numpy() - ref).max() <= 1e-6
        assert got.counts.cpu().numpy().tolist() == np.bincount(labels, minlength=33).tolist()
    nothing = _run(torch.zeros(2, 70, 5, 5, device=DEV), torch.from_numpy(cent).to(DEV))
    assert not nothing.labels.any() and nothing.counts[0] == 50 and nothing.stats.tolist() == [0.0, 33.0, nothing.stats[2].item(), 50.0]
    assert np.abs(nothing.centroids.cpu().numpy() - O.normalize(cent)).max() <= 2.0 ** -24 and abs(nothing.stats[2].item()) < 1e-6


@pytest.mark.parametrize("shape", [STEP_SHAPES[1], STEP_SHAPES[2]], ids=lambda s: "x".join(map(str, s)))
def test_assignment_only_in_place_and_repeat_calls(shape):
    x, cent, _ = _step_case(shape)
    xd, cd = _dev(x, "cl"), torch.from_numpy(cent).to(DEV)
    a, b = _run(xd, cd), _run(xd, cd)
    for u, v in zip(a, b):                                  # two calls on the same input: every output bitwise
        assert torch.equal(u, v)
    only = _run(xd, cd, update=False)
    assert only.centroids is None and torch.equal(only.labels, a.labels) and torch.equal(only.counts, a.counts)
    assert only.stats[0] == a.stats[0] and only.stats[1] == 0 and only.stats[2] == 0 and only.stats[3] == a.stats[3]
    quiet = _run(xd, cd, labels=False)
    assert quiet.labels is None and torch.equal(quiet.centroids, a.centroids) and torch.equal(quiet.stats, a.stats)
    place = cd.clone()
    c = _run(xd, place, out=place)
    assert c.centroids is place and torch.equal(place, a.centroids) and torch.equal(c.stats, a.stats) and torch.equal(c.counts, a.counts)


# ---- seeding
@functools.lru_cache(maxsize=None)
def _seed_case(shape):
    B, h, w, K, n = shape
    rng = np.random.default_rng(sum(shape) + 1)
    x = rng.standard_normal((B, K, h, w)).astype(np.float32)
    x[0, :, 1, 2] = 0
    want = O.seed(x, n, rng.random(n), snap=True)           # every u_r in the middle of the picked token's interval
    return x, want, (0 * h + 1) * w + 2


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SEED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_seed_against_the_oracle(shape, layout):
    B, h, w, K, n = shape
    x, want, zero = _seed_case(shape)
    assert want["margin"] >= MARGIN, want["margin"]
    assert zero not in want["picks"]
    cent, picks = cluster_refit.kmeans_seed(_dev(x, layout), n, u=want["u"])
    again = cluster_refit.kmeans_seed(_dev(x, layout), n, u=want["u"])
    assert np.array_equal(picks.cpu().numpy(), want["picks"]), (picks.cpu().numpy(), want["picks"])
    ulp = np.spacing(np.abs(want["centroids"]).astype(np.float32)).astype(np.float64)
    assert (np.abs(cent.cpu().numpy() - want["centroids"]) <= 3 * ulp).all()
    assert torch.equal(again[0], cent) and torch.equal(again[1], picks)


def test_seed_degenerate_inputs_and_bad_draws():
    x = np.zeros((1, 8, 2, 3), dtype=np.float32)
    x[0, 0, 0, :] = 1.0                                      # three equal tokens, one other, two zero ones: fewer distinct tokens than n
    x[0, 1, 1, 0] = 2.0
    u = [0.1, 0.6, 0.5, 0.9]
    want = O.seed(x, 4, u)
    for layout in LAYOUTS:
        cent, picks = cluster_refit.kmeans_seed(_dev(x, layout), 4, u=u)
        assert picks.tolist() == want["picks"].tolist() == [0, 3, 2, 3]
        assert np.abs(cent.cpu().numpy() - want["centroids"]).max() == 0
    nothing = cluster_refit.kmeans_seed(torch.zeros(1, 4, 2, 2, device=DEV), 2, u=[0.3, 0.7])
    assert nothing[1].tolist() == [0, 0] and not nothing[0].any()
    with pytest.raises(RuntimeError, match="182"):
        cluster_refit.kmeans_seed(_dev(x, "cl"), 4, u=[0.1, 0.6, 0.5, 1.0])
    torch.cuda.synchronize()


# ---- end to end
def test_fit_recovers_planted_clusters():
    x, which = O.planted()
    u = torch.rand(5, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).numpy()
    start = O.seed(x, 5, u)
    assert len(set(which[start["picks"]].tolist())) == 5
    cent, labels, _ = O.fit(x, start["centroids"])
    assert O.same_partition(labels, which)
    for layout in LAYOUTS:
        xd = _dev(x, layout)
        res = cluster_refit.kmeans_fit(xd, 5, generator=torch.Generator().manual_seed(0), check_every=10)
        assert res.converged and res.n_iter == 10 and len(res.history) == 10          # stops on shift < tol at the first check
        got = cluster_refit.kmeans_step(xd, res.centroids, labels=True, update=False)
        assert O.same_partition(got.labels.cpu().numpy(), which)
        assert np.abs(res.centroids.cpu().numpy() - cent).max() <= 1e-5
        assert res.counts.tolist() == np.bincount(labels, minlength=5).tolist()
        assert abs(res.objective - O.step(x, cent)["objective"]) <= _sim_bound(105, 70)
    slow = cluster_refit.kmeans_fit(_dev(x, "cl"), 5, n_iter=7, tol=-1.0, generator=torch.Generator().manual_seed(0), check_every=3)
    assert not slow.converged and slow.n_iter == 7 and len(slow.history) == 7


def test_the_objective_never_drops():
    shape = STEP_SHAPES[1]
    B, h, w, K, n = shape
    T = B * h * w
    x, cent, _ = _step_case(shape)
    xd, cd = _dev(x, "cl"), F.normalize(torch.from_numpy(cent), dim=1).to(DEV)
    objs = []
    for _ in range(10):
        objs.append(cluster_refit.kmeans_step(xd, cd, out=cd).stats)
    objs = torch.stack(objs).cpu().numpy()[:, 0]
    print("objective", objs[0], "->", objs[-1])
    assert (np.diff(objs) >= -2 * _sim_bound(T, K)).all(), np.diff(objs)
    assert objs[-1] >= 1.1 * objs[0]


def test_a_captured_step_replays_bitwise():
    shape = STEP_SHAPES[1]
    B, h, w, K, n = shape
    x, cent, _ = _step_case(shape)
    xd, cd = _dev(x, "cl"), torch.from_numpy(cent).to(DEV)
    eager = _run(xd, cd)
    desc = capi.kmeans_desc(B, K, h, w, n)
    ws = capi.kmeans_workspace(desc, DEV)
    out = torch.zeros(n, K, device=DEV)
    labels = torch.zeros(B, h, w, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(n, dtype=torch.int64, device=DEV)
    stats = torch.zeros(4, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        capi.kmeans_step(desc, xd, cd, out, labels, counts, stats, ws)
    for _ in range(2):
        for t in (out, labels, counts, stats):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager.centroids) and torch.equal(labels, eager.labels)
        assert torch.equal(counts, eager.counts) and torch.equal(stats, eager.stats)


def _tiny_model(*extra):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=2", "dim=70", "dropout=False",
                                 "extra_clusters=1"] + list(extra))
    torch.manual_seed(0)
    model = LitUnsupervisedSegmenter(27, cfg).to(DEV).eval()
    loader = torch.utils.data.DataLoader(SyntheticContrastiveDataset(8, 64, 27, seed=3), 4, shuffle=False)
    return model, loader


def test_a_refitted_model_segments_and_evaluates():
    from stego_amd.eval_segmentation import evaluate
    from stego_amd.segment import segment
    model, loader = _tiny_model()
    codes = cluster_refit.collect_codes(model, loader)
    assert tuple(codes.shape) == (8, 70, 4, 4) and codes.is_cuda and codes.is_contiguous(memory_format=torch.channels_last)
    res = cluster_refit.refit_cluster_probe(model, codes, 30, n_iter=20, generator=torch.Generator().manual_seed(1))
    assert model.cluster_probe.clusters.shape == (30, 70) and model.cfg.cluster_probe_n == 30 and int(res.counts.sum()) == 128
    assert model.test_cluster_metrics.extra_clusters == 3
    img = next(iter(loader))["img"].to(DEV)
    _, cluster = segment(model, img, run_crf=False)
    with torch.no_grad():
        code = (model.net(img)[1] + model.net(img.flip(dims=[3]))[1].flip(dims=[3])) / 2
        code = F.interpolate(code, img.shape[-2:], mode="bilinear", align_corners=False)
        inner = torch.einsum("bchw,nc->bnhw", F.normalize(code, dim=1), F.normalize(model.cluster_probe.clusters, dim=1))
    top = inner.topk(2, dim=1).values
    sure = (top[:, 0] - top[:, 1]) >= 1e-5                   # the fused head resizes in another order: fp32 near-ties may go either way
    assert cluster.max() < 30 and len(cluster.unique()) > 1
    assert torch.equal(cluster[sure], inner.argmax(1)[sure])
    assert (cluster == inner.argmax(1)).flatten(1).float().mean(1).min().item() >= 0.999
    metrics = evaluate(model, loader, run_crf=False, native_metrics=True)
    assert set(metrics) == {"final/linear/mIoU", "final/linear/Accuracy", "final/cluster/mIoU", "final/cluster/Accuracy"}
    assert all(np.isfinite(v) for v in metrics.values()) and metrics["final/cluster/Accuracy"] > 0
    assert model.test_cluster_metrics.stats.shape == (30, 27) and len(model.cluster_to_class) == 30


def test_the_entry_point_writes_checkpoints_and_the_sweep(tmp_path):
    from stego_amd import refit_clusters as R
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    res = 48
    mcfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=%d" % res, "dim=70", "dropout=False"])
    torch.manual_seed(1)
    model = LitUnsupervisedSegmenter(27, mcfg)
    ck = tmp_path / "run.ckpt"
    model.save_checkpoint(str(ck))
    d = tmp_path / "images"
    d.mkdir()
    rng = np.random.default_rng(2)
    for stem, shape in (("a", (60, 90, 3)), ("b", (52, 80, 3)), ("c", (48, 48, 3))):
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(d / (stem + ".png"))
    cfg = load_config(R.REFIT_CONFIG, overrides=["output_root=%s" % tmp_path, "model_path=%s" % ck, "image_dir=%s" % d, "experiment_name=t",
                                                 "res=%d" % res, "batch_size=1", "num_workers=0", "n_clusters=[2, 3]", "n_init=2",
                                                 "n_iter=20"])
    rows = R.my_app(cfg)
    out = os.path.join(str(tmp_path), "refit", "t")
    assert sorted(os.listdir(out)) == ["clusters_2.ckpt", "clusters_3.ckpt", "sweep.json"]
    table = json.load(open(os.path.join(out, "sweep.json")))
    assert table == rows and [r["n_clusters"] for r in table] == [2, 3]
    for r in table:
        assert r["tokens"] == 27 and r["images"] == 3 and 0 < r["objective_per_token"] <= 1 and 1 <= r["min_cluster"] <= r["max_cluster"]
        assert r["iterations"] >= 1 and isinstance(r["converged"], bool)
        back = LitUnsupervisedSegmenter.load_from_checkpoint(r["checkpoint"], strict=True)
        assert back.cluster_probe.clusters.shape == (r["n_clusters"], 70) and back.cfg.cluster_probe_n == r["n_clusters"]
        with pytest.raises(ValueError, match="cluster_probe_n"):
            back.check_cluster_scoring()
    assert table[1]["objective_per_token"] >= table[0]["objective_per_token"] - 1e-6
