"""Segments as objects on the MI355X (csrc/regions.hip) against the explicit-loop oracle of tests/regions_oracle.py.  Everything is
integer arithmetic with one right answer, so every comparison is exact: the id map, n_regions, every column of the table, the cleaned
map and the number of rounds.  The shapes hang on the tile edge T the plan reports: one pixel, single rows and columns longer than two
tiles, a tile less and more one, exactly a tile, more than two tiles each way, and widths 3 and 67 for the ends of the rows."""
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import regions_oracle as O
from stego_amd import capi
from stego_amd import regions as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = capi.REGIONS_TILE
SHAPES = [(1, 1), (1, 2 * T + 3), (2 * T + 3, 1), (T - 1, T + 1), (T, T), (2 * T + 1, 2 * T + 3), (5, 3), (9, 67)]


def test_tile_edge_is_the_plans():
    rc, tile, launches = capi.regions_plan(capi.regions_desc(1, 2 * T + 1, 2 * T + 3))
    assert rc == 0 and tile == T and launches[0][1] == 9


@functools.lru_cache(maxsize=None)
def _want(name, shape, connectivity):
    m = O.PATTERNS[name](*shape)
    ids, n = O.label(m, connectivity)
    return m, ids, n, O.table(m, ids, n)


def _check_batch(maps, connectivity, dtype=torch.int64, want=None):
    """maps: a list of [H, W] arrays of one shape -> label_regions and region_table on the device equal the oracle, image by image."""
    lab = torch.from_numpy(np.stack(maps)).to(dtype).to(DEV)
    ids, n = R.label_regions(lab, connectivity)
    table = R.region_table(lab, ids, n)
    assert ids.dtype == torch.int32 and n.dtype == torch.int32 and ids.shape == lab.shape
    ids, n = ids.cpu().numpy(), n.cpu().numpy()
    if want is None:
        want = []
        for m in maps:
            w_ids, w_n = O.label(m, connectivity)
            want.append((w_ids, w_n, O.table(m, w_ids, w_n)))
    for b, m in enumerate(maps):
        w_ids, w_n, w_table = want[b]
        assert n[b] == w_n == table.n_regions[b], (b, n[b], w_n)
        assert np.array_equal(ids[b], w_ids), (b, np.argwhere(ids[b] != w_ids)[:5])
        for c in O.COLUMNS:
            got = getattr(table, c)[table.rows(b)].cpu().numpy()
            assert np.array_equal(got, w_table[c]), (b, c, got[:8], w_table[c][:8])
    return ids, n


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(O.PATTERNS))
def test_patterns_at_every_shape(name, connectivity):
    for shape in SHAPES:
        m, w_ids, w_n, w_table = _want(name, shape, connectivity)
        _check_batch([m], connectivity, want=[(w_ids, w_n, w_table)])


@pytest.mark.parametrize("connectivity", [4, 8])
def test_pattern_properties(connectivity):
    shape = (2 * T + 1, 2 * T + 3)
    H, W = shape
    assert _want("uniform", shape, connectivity)[2] == 1 and _want("uniform", shape, connectivity)[3]["first"][0] == 0
    assert _want("checkerboard", shape, connectivity)[2] == (H * W if connectivity == 4 else 2)
    comb = _want("comb", shape, connectivity)
    assert comb[1][0, 0] == 0 and comb[3]["first"][0] == 0 and comb[3]["area"][0] == (W + 1) // 2 * (H - 1) + W
    u = _want("u", shape, connectivity)
    assert u[1][0, 0] == 0 == u[1][0, W - 1]
    m = _want("spiral", shape, 4)[0]
    ids, n = O.label(m, 4)
    assert (ids[m == 1] == 0).all() and (m == 1).sum() > H * W // 3                  # one corridor over the whole image


@pytest.mark.parametrize("connectivity", [4, 8])
def test_a_batch_whose_images_differ(connectivity):
    shape = (2 * T + 1, 2 * T + 3)
    maps = [O.random_map(*shape, 3, 11), O.comb(*shape), np.full(shape, -1, dtype=np.int64), O.rings(*shape)]
    ids, n = _check_batch(maps, connectivity)
    assert n[2] == 0 and (ids[2] == -1).all() and ids[1].max() == n[1] - 1 and ids[3].min() == 0


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_negative_labels(dtype):
    shape = (T + 5, 2 * T + 3)
    maps = [O.with_negatives(*shape, 7), np.full(shape, -3, dtype=np.int64), O.with_negatives(*shape, 9)]
    ids, n = _check_batch(maps, 8, dtype=dtype)
    assert n[1] == 0 and ((ids[0] == -1) == (maps[0] < 0)).all()


def test_dtypes_give_the_same_ids():
    shape = (2 * T + 1, 67)
    maps = [O.random_map(*shape, 3, 4), O.rings(*shape)]
    got = [_check_batch(maps, 4, dtype=dt) for dt in (torch.int64, torch.int32, torch.uint8)]
    for ids, n in got[1:]:
        assert np.array_equal(ids, got[0][0]) and np.array_equal(n, got[0][1])


def test_other_integer_dtypes_take_the_chain():
    m = O.random_map(9, 67, 3, 4)
    ids, n = R.label_regions(torch.from_numpy(m).to(torch.int16).to(DEV)[None], 4)
    w_ids, w_n = O.label(m, 4)
    assert ids.is_cuda and int(n[0]) == w_n and np.array_equal(ids[0].cpu().numpy(), w_ids)


def test_the_larger_case_repeats_and_replays():
    """One 320 x 320 3-class random map: equal to the oracle, to a second call and to the replay of a captured graph, bit for bit."""
    m = O.random_map(320, 320, 3, 1)
    lab = torch.from_numpy(m).to(DEV)[None]
    ids, n = _check_batch([m], 4)
    ids2, n2 = R.label_regions(lab, 4)
    assert np.array_equal(ids2.cpu().numpy(), ids) and np.array_equal(n2.cpu().numpy(), n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        R.label_regions(lab, 4)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ids3, n3 = R.label_regions(lab, 4)
    ids3.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(ids3.cpu().numpy(), ids) and np.array_equal(n3.cpu().numpy(), n)
    t1, t2 = R.region_table(lab, ids2, n2), R.region_table(lab, ids2, n2)
    for c in O.COLUMNS:
        assert torch.equal(getattr(t1, c), getattr(t2, c)), c


# ---- the cleanup
def _check_merge(maps, min_area, n_labels, connectivity=4, dtype=torch.int64, **kw):
    lab = torch.from_numpy(np.stack(maps)).to(dtype).to(DEV)
    before = lab.clone()
    got, rounds = R.merge_small_regions(lab, min_area, n_labels, connectivity, **kw)
    want, w_rounds = O.merge_batch(np.stack(maps), min_area, n_labels, connectivity, max_rounds=kw.get("max_rounds", 4))
    assert got.dtype == dtype and got.shape == lab.shape and torch.equal(lab, before)
    assert rounds == w_rounds, (rounds, w_rounds)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want), np.argwhere(got.cpu().numpy() != want)[:5]
    return got.cpu().numpy().astype(np.int64), rounds


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("min_area", [2, 6, 50])
def test_speckled_blocks(min_area, connectivity):
    got, rounds = _check_merge([O.blocky(96, 96, seed=3)], min_area, 5, connectivity)
    _check_merge([O.blocky(2 * T + 1, 2 * T + 3, seed=4), O.blocky(2 * T + 1, 2 * T + 3, block=20, seed=5)], min_area, 5, connectivity)
    if min_area == 6 and connectivity == 4:
        first, _ = O.cleanup_round(O.blocky(96, 96, seed=3), 6, 5)
        assert np.array_equal(got[0], first) and rounds == 2         # clean after one round; the second finds nothing to do


def test_a_tie_goes_to_the_smaller_class():
    m = np.array([[2, 2, 2, 1, 1, 1, 1],
                  [2, 2, 2, 5, 1, 1, 1],
                  [2, 2, 2, 2, 1, 1, 1]], dtype=np.int64)
    got, _ = _check_merge([m], 2, 6)
    assert got[0][1, 3] == 1


def test_enclosed_by_small_regions_and_the_round_limit():
    m = np.zeros((7, 7), dtype=np.int64)
    m[3, 3], m[2, 3], m[4, 3], m[3, 2], m[3, 4] = 7, 3, 4, 5, 6
    one, rounds = _check_merge([m], 2, 8, max_rounds=1)
    assert rounds == 1 and one[0][3, 3] == 7 and (one[0] != 0).sum() == 1      # no neighbour that is not small: it stays
    full, rounds = _check_merge([m], 2, 8)
    assert rounds == 3 and (full[0] == 0).all()


def test_noise_is_left_alone():
    m = O.random_map(2 * T + 1, 67, 27, 8)
    got, rounds = _check_merge([m], 16, 27)
    assert rounds == 1 and np.array_equal(got[0], m)


def test_three_slabs_equal_one():
    m = O.blocky(2 * T + 1, 2 * T + 3, seed=6)
    ids, n = O.label(m, 4)
    n_small = int((O.table(m, ids, n)["area"] < 6).sum())
    assert n_small >= 3
    rows = -(-n_small // 3)
    assert len(R.vote_slabs(n_small, 5, 4 * 5 * rows)) == 3
    one, _ = _check_merge([m], 6, 5)
    three, _ = _check_merge([m], 6, 5, vote_bytes=4 * 5 * rows)
    assert np.array_equal(one, three)


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
def test_the_cleaned_map_keeps_the_dtype(dtype):
    _check_merge([O.blocky(T + 3, 67, seed=7)], 6, 5, dtype=dtype)


# ---- end to end on a tiny model
RES = 48


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    tmp = tmp_path_factory.mktemp("regions_demo")
    mcfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=%d" % RES, "dim=70", "dropout=False",
                                  "extra_clusters=2"])
    torch.manual_seed(1)
    model = LitUnsupervisedSegmenter(27, mcfg)
    model._cluster_to_class = np.arange(29, dtype=np.int64) % 27
    ck = tmp / "demo.ckpt"
    model.save_checkpoint(str(ck))
    d = tmp / "images"
    d.mkdir()
    rng = np.random.default_rng(2)
    Image.fromarray(rng.integers(0, 256, (60, 90, 3), dtype=np.uint8)).save(d / "wide.jpg")
    Image.fromarray(rng.integers(0, 256, (100, 50), dtype=np.uint8), "L").save(d / "tall.png")
    big = tmp / "big"
    big.mkdir()
    Image.fromarray(rng.integers(0, 256, (70, 101, 3), dtype=np.uint8)).save(big / "large.png")
    loaded = LitUnsupervisedSegmenter.load_from_checkpoint(str(ck)).eval().to(DEV)
    return tmp, ck, d, big, loaded


def _run_demo(demo, name, image_dir, *extra):
    from stego_amd import demo_segmentation as D
    from stego_amd.train_segmentation import load_config
    tmp, ck = demo[0], demo[1]
    cfg = load_config(D.DEMO_CONFIG, overrides=["output_root=%s" % tmp, "model_path=%s" % ck, "image_dir=%s" % image_dir,
                                                "experiment_name=%s" % name, "res=%d" % RES, "batch_size=2", "num_workers=0"] + list(extra))
    written = D.my_app(cfg)
    return written, os.path.join(str(tmp), "results", "predictions", name)


def _check_region_files(out, stem, linear, cluster, class_of):
    """linear / cluster: the uncleaned int64 [H, W] maps of one image -> every file the demo wrote for it equals the oracle's."""
    H, W = cluster.shape
    w_lin, w_clu = O.merge(linear, 4, 27)[0], O.merge(cluster, 4, 29)[0]
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "linear", stem + ".png"))), w_lin.astype(np.uint8))
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, "cluster", stem + ".png"))), w_clu.astype(np.uint8))
    with open(os.path.join(out, "regions", stem + ".json")) as f:
        doc = json.load(f)
    assert doc == {"height": H, "width": W, "connectivity": 4, "id_map": stem + ".png", "regions": O.region_dicts(w_clu, 4, class_of)}
    png = Image.open(os.path.join(out, "region_ids", stem + ".png"))
    assert png.mode == "I;16"
    assert np.array_equal(np.asarray(png).astype(np.int32), O.label(w_clu, 4)[0])
    assert np.array_equal(R.read_id_map(os.path.join(out, "region_ids", stem + ".png")), O.label(w_clu, 4)[0])


def test_demo_with_the_keys_off_writes_what_it_wrote(demo):
    written, out = _run_demo(demo, "keys_off", demo[2], "run_crf=False")
    assert sorted(os.listdir(out)) == ["cluster", "linear"]
    assert written == [os.path.join(out, sub, stem + ".png") for stem in ("tall", "wide") for sub in ("linear", "cluster")]


def test_demo_regions(demo):
    from stego_amd.data import image_transform
    from stego_amd.segment import segment
    written, out = _run_demo(demo, "keys_on", demo[2], "run_crf=False", "save_regions=True", "min_region_area=4")
    assert written == [os.path.join(out, sub, stem + ".png") for stem in ("tall", "wide") for sub in ("linear", "cluster")]
    assert sorted(os.listdir(out)) == ["cluster", "linear", "region_ids", "regions"]
    tf = image_transform(RES, "center")
    names = ["tall.png", "wide.jpg"]
    img = torch.stack([tf(Image.open(demo[2] / n).convert("RGB")) for n in names]).to(DEV)
    lin, clu = segment(demo[4], img, run_crf=False)
    for j, stem in enumerate(("tall", "wide")):
        _check_region_files(out, stem, lin[j].cpu().numpy(), clu[j].cpu().numpy(), demo[4].cluster_to_class)
    # segment(min_region_area) is the oracle on segment()
    lin4, clu4 = segment(demo[4], img, run_crf=False, min_region_area=4)
    assert lin4.dtype == torch.int64 and np.array_equal(lin4.cpu().numpy(), O.merge_batch(lin.cpu().numpy(), 4, 27)[0])
    assert np.array_equal(clu4.cpu().numpy(), O.merge_batch(clu.cpu().numpy(), 4, 29)[0])
    lin8, _ = segment(demo[4], img, run_crf=False, min_region_area=4, connectivity=8)
    assert np.array_equal(lin8.cpu().numpy(), O.merge_batch(lin.cpu().numpy(), 4, 27, 8)[0])


def test_demo_regions_full_res(demo):
    from stego_amd.data import full_image_transform
    from stego_amd.segment import segment_large
    written, out = _run_demo(demo, "keys_on_full", demo[3], "run_crf=False", "save_regions=True", "min_region_area=4", "full_res=True")
    assert len(written) == 2
    img = full_image_transform(RES)(Image.open(demo[3] / "large.png").convert("RGB")).to(DEV)
    lin, clu = segment_large(demo[4], img, RES, batch=4, run_crf=False)
    assert tuple(clu.shape) == (70, 101)
    _check_region_files(out, "large", lin.cpu().numpy(), clu.cpu().numpy(), demo[4].cluster_to_class)
    lin4, clu4 = segment_large(demo[4], img, RES, batch=4, run_crf=False, min_region_area=4)
    assert np.array_equal(clu4.cpu().numpy(), O.merge(clu.cpu().numpy(), 4, 29)[0])
    assert np.array_equal(lin4.cpu().numpy(), O.merge(lin.cpu().numpy(), 4, 27)[0])


def _tiny_eval_model():
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=%d" % RES, "batch_size=2", "dim=70", "dropout=False",
                                 "extra_clusters=1"])
    torch.manual_seed(0)
    model = LitUnsupervisedSegmenter(27, cfg).to(DEV).eval()
    loader = torch.utils.data.DataLoader(SyntheticContrastiveDataset(4, RES, 27, seed=3), 2, shuffle=False)
    return model, loader


def _plain(metrics):
    return {k: float(v) for k, v in metrics.items()}


@pytest.mark.parametrize("native", [False, True])
def test_evaluate_scores_the_cleaned_maps(native):
    from stego_amd.eval_segmentation import evaluate
    model, loader = _tiny_eval_model()
    today = _plain(evaluate(model, loader, run_crf=False, native_metrics=native))
    off = _plain(evaluate(model, loader, run_crf=False, native_metrics=native, min_region_area=0, keep=range(4)))
    assert off == today
    data = model.saved_data
    labels = data["label"]
    lin = torch.from_numpy(O.merge_batch(data["linear_preds"].cpu().numpy(), 4, 27)[0]).to(DEV)
    clu = torch.from_numpy(O.merge_batch(data["cluster_preds"].cpu().numpy(), 4, 28)[0]).to(DEV)
    assert not (torch.equal(lin, data["linear_preds"]) and torch.equal(clu, data["cluster_preds"]))      # there is something to clean
    got = _plain(evaluate(model, loader, run_crf=False, native_metrics=native, min_region_area=4))
    model.test_linear_metrics.reset()
    model.test_cluster_metrics.reset()
    for lo in (0, 2):                                                 # the loader's batches
        model.test_linear_metrics.update(lin[lo:lo + 2], labels[lo:lo + 2])
        model.test_cluster_metrics.update(clu[lo:lo + 2], labels[lo:lo + 2])
    want = _plain({**model.test_linear_metrics.compute(), **model.test_cluster_metrics.compute()})
    assert got == want
