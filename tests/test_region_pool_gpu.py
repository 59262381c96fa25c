"""Region descriptors on the GPU (csrc/region_pool.hip behind stego_amd.region_descriptors) against the float64 oracle of
tests/region_pool_oracle.py.

Bound: |got - want| <= 2^-21 M per element, M the largest magnitude of the map.  The taps are shared with the oracle (the kernel rounds
every operation of the source index on its own).  What differs is 1 - lambda twice, the roundings of the interpolation, the quantisation
(2^-31 M) and the final conversion: at most eight roundings of relative 2^-24 on quantities no larger than M, and the mean of bounded
errors is bounded by the same.  A numpy restatement gives 0.26 x 2^-24 M for the worst descriptor of a smooth scene; observed on the
MI355X over every case below: at most 1.63 x 2^-24 M against the oracle (checkerboards, where a region is one pixel and nothing
averages out) and 3.5 x 2^-24 M between the native path and the float32 result of the torch chain (whose maps, normalised on two devices, differ by a rounding
themselves).

The shapes hang on the plan: L, the pixels of the row segment one wave walks (64 for C > 32, up to 512 below), and CB = 128, the channels
of one wave.  Exact cases are compared bitwise with the oracle's integer version."""
import os
import warnings

import numpy as np
import pytest
import torch
from PIL import Image

import region_pool_oracle as PO
import regions_oracle as O
from stego_amd import capi
from stego_amd import region_descriptors as D
from stego_amd import regions as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CB = capi.REGION_POOL_CB
PATTERNS = [("checkerboard", O.checkerboard), ("uniform", O.uniform), ("comb", O.comb), ("spiral", O.spiral),
            ("negatives", lambda H, W: O.with_negatives(H, W, 5))]


def _segment(C):
    rc, L, cb, _ = capi.region_pool_plan(capi.region_pool_desc(1, C, 5, 7, 33, 67, 1))
    assert rc == 0 and cb == CB
    return L


def _regions(label_maps):
    lab = torch.from_numpy(np.stack(label_maps)).to(DEV)
    ids, n = R.label_regions(lab, 4)
    return ids, R.region_table(lab, ids, n)


def _layout(maps, kind):
    """The float32 numpy map [B, C, h, w] on the device: dense NCHW, the channels-last strided view the backbone returns, or a view at
    an odd element offset into a larger buffer."""
    t = torch.from_numpy(maps).to(DEV)
    if kind == "nchw":
        return t
    if kind == "nhwc":
        v = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert v.stride(1) == 1 or v.shape[1] == 1
        return v
    buf = torch.full((t.numel() + 7,), float("nan"), device=DEV)
    v = buf[3:3 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _check(label_maps, maps, kind="nchw", what=""):
    ids, table = _regions(label_maps)
    got = D.region_descriptors(ids, table, _layout(maps, kind)).cpu().numpy()
    want = PO.descriptors(maps, ids.cpu().numpy(), table.row_offset, table.area.cpu().numpy())
    M = float(np.abs(maps).max())
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print(what, kind, maps.shape, ids.shape, "err / (2^-24 M) = %.3f" % (err / (2.0 ** -24 * M) if M else 0.0))
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    assert err <= 2.0 ** -21 * M, (what, kind, err, M)
    return got, ids, table


def _maps(seed, B, C, h, w, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((B, C, h, w)) * scale).astype(np.float32)


@pytest.mark.parametrize("C", [1, 3, 63, 64, 65, 70, CB, CB + 1, 384])
def test_shapes_channels_and_layouts(C):
    L = _segment(C)
    assert L == (64 if C > 32 else 512)
    k = 0
    for W in (1, 3, L - 1, L, L + 1, 2 * L + 3):
        for H in (1, 5):
            h, w = [(H, W), (-(-H // 8), -(-W // 8)), (5, 7), (-(-H // 2), W)][k % 4]         # identity, factor 8, non-integer, mixed
            name, pattern = PATTERNS[k % len(PATTERNS)]
            _check([pattern(H, W)], _maps(k, 1, C, h, w), ("nchw", "nhwc", "offset")[k % 3], name)
            k += 1


@pytest.mark.parametrize("hw,HW", [((40, 40), (40, 40)), ((5, 5), (40, 40)), ((5, 7), (33, 67)), ((9, 4), (4, 9))])
@pytest.mark.parametrize("kind", ["nchw", "nhwc", "offset"])
def test_scales_from_identity_to_non_integer(hw, HW, kind):
    for C in (3, 70):
        _check([O.random_map(*HW, 3, 3), O.with_negatives(*HW, 5)], _maps(1, 2, C, *hw), kind)


@pytest.mark.parametrize("name,pattern", PATTERNS)
def test_id_patterns(name, pattern):
    for C in (3, 70, 200):
        _check([pattern(33, 67)], _maps(2, 1, C, 5, 7), "nhwc", name)


def test_a_batch_whose_images_differ_one_without_a_region():
    maps = [O.checkerboard(5, 131), np.full((5, 131), -1, dtype=np.int64), O.spiral(5, 131), O.with_negatives(5, 131, 7)]
    for C in (3, 70):
        got, ids, table = _check(maps, _maps(3, 4, C, 3, 17), "nhwc")
        assert table.n_regions[1] == 0 and len(table) == got.shape[0]


def test_magnitudes_zero_and_the_edge_of_the_exponent():
    labels = [O.random_map(33, 67, 3, 3)]
    for scale in (1e4, 1e-6):
        _check(labels, _maps(4, 1, 70, 5, 7, scale), "nchw", "scale %g" % scale)
    got, _, _ = _check(labels, np.zeros((1, 70, 5, 7), dtype=np.float32), "nchw", "zero")
    assert not got.any()
    for top in (4.0, -0.5, np.float32(4.0) - np.float32(2.0 ** -22)):                   # M an exact power of two, and the float below one
        m = np.clip(_maps(5, 1, 70, 5, 7), -0.4, 0.4)
        m[0, 11, 2, 3] = top
        assert float(np.abs(m).max()) == abs(float(top))
        _check(labels, m, "nhwc", "top %r" % top)
        ids, table = _regions(labels)
        got = D.region_descriptors(ids, table, torch.from_numpy(m).to(DEV)).cpu().numpy()
        assert np.array_equal(got, PO.descriptors_exact(m, ids.cpu().numpy(), table.row_offset, table.area.cpu().numpy()))


@pytest.mark.parametrize("C", [3, 70])
def test_exact_cases_are_the_correctly_rounded_mean(C):
    """Identity taps with small integers; a factor-2 upsample (weights 1/4 and 3/4, products in sixteenths) with multiples of 8: every
    intermediate is exact, so the kernel returns float32((double) S 2^-s / area) of the exact sum."""
    L = _segment(C)
    rng = np.random.default_rng(6)
    for (h, w), (H, W), values in (((5, L + 1), (5, L + 1), rng.integers(-9, 10, (2, C, 5, L + 1))),
                                   ((4, 33), (8, 66), 8 * rng.integers(-7, 8, (2, C, 4, 33)))):
        m = values.astype(np.float32)
        labels = [O.random_map(H, W, 3, 3), O.with_negatives(H, W, 5)]
        for kind in ("nchw", "nhwc"):
            got, ids, table = _check(labels, m, kind, "exact")
            want = PO.descriptors_exact(m, ids.cpu().numpy(), table.row_offset, table.area.cpu().numpy())
            assert np.array_equal(got, want), (h, w, kind, np.abs(got - want).max())


def test_repeatable_and_independent_of_the_ranges():
    labels = [O.random_map(33, 67, 3, 3), O.checkerboard(33, 67), O.with_negatives(33, 67, 5)]
    ids, table = _regions(labels)
    maps = _layout(_maps(7, 3, 70, 5, 7), "nhwc")
    R_ = len(table)
    one = D.region_descriptors(ids, table, maps)
    assert torch.equal(one, D.region_descriptors(ids, table, maps))
    offs = torch.tensor(table.row_offset, dtype=torch.int64, device=DEV)
    area = table.area.contiguous()
    a = table.row_offset[1] + 5                                          # cuts inside the rows of the second image
    b = a + 1                                                            # a range of one row
    c = table.row_offset[2] - 3
    parts = [capi.region_pool(maps, ids, offs, area, lo, hi) for lo, hi in ((0, a), (a, b), (b, c), (c, R_))]
    assert 0 < a < b < c < R_ and torch.equal(torch.cat(parts), one)
    for budget in (1, 70 * 8 * 7, 70 * 8 * 1000):
        assert len(D.pool_slabs(R_, 70, budget)) == -(-R_ // max(1, budget // 560))
        assert torch.equal(D.region_descriptors(ids, table, maps, pool_bytes=budget), one), budget
    assert capi.region_pool(maps, ids, offs, area, 4, 4).shape == (0, 70)


def test_a_captured_graph_replays_the_same_bits():
    """The three launches captured once (a linear chain on one stream), replayed after the output and the workspace were overwritten:
    the call resets what it uses, so the replay equals the plain call bit for bit."""
    ids, table = _regions([O.random_map(33, 67, 3, 3), O.checkerboard(33, 67)])
    maps = _layout(_maps(11, 2, 70, 5, 7), "nhwc")
    offs = torch.tensor(table.row_offset, dtype=torch.int64, device=DEV)
    area, n = table.area.contiguous(), len(table)
    want = capi.region_pool(maps, ids, offs, area, 0, n)
    need = capi.region_pool_workspace_bytes(capi.region_pool_desc(2, 70, 5, 7, 33, 67, n))
    ws, out = torch.empty(need, dtype=torch.uint8, device=DEV), torch.empty((n, 70), dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        capi.region_pool(maps, ids, offs, area, 0, n, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        capi.region_pool(maps, ids, offs, area, 0, n, out=out, workspace=ws)
    out.fill_(-7)
    ws.fill_(255)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_the_native_path_and_the_torch_chain_agree():
    labels = [O.random_map(33, 67, 3, 3), O.with_negatives(33, 67, 5)]
    ids, table = _regions(labels)
    m = _maps(8, 2, 70, 5, 7)
    native = D.region_descriptors(ids, table, torch.from_numpy(m).to(DEV), normalize=True)
    chain = D.region_descriptors(ids.cpu(), table, torch.from_numpy(m), normalize=True)
    assert native.is_cuda and not chain.is_cuda
    M = float(torch.nn.functional.normalize(torch.from_numpy(m), dim=1).abs().max())
    err = float((native.cpu() - chain).abs().max())
    print("err / (2^-24 M) = %.3f" % (err / (2.0 ** -24 * M)))
    assert err <= 2.0 ** -21 * M


def test_search_on_the_device_against_float64_cosines():
    rng = np.random.default_rng(9)
    per, C, k = 60, 70, 8
    descs = rng.standard_normal((5 * per, C)).astype(np.float32)
    planted = [(3, 100), (70, 250), (130, 299), (200, 10)]
    for i, j in planted:
        descs[j] = descs[i] * 2.5 + 1e-3 * rng.standard_normal(C).astype(np.float32)
    index = D.RegionIndex("code")
    for b in range(5):
        cols = {c: torch.zeros(per, dtype=torch.int64) for c in R.RegionTable.COLUMNS}
        cols["area"] += 10
        index.add("im%d.png" % b, R.RegionTable(cols, [per], 8), 0, descs[b * per:(b + 1) * per])
    rows, sims = index.search(np.arange(5 * per), k=k, other_images_only=False, device=DEV)
    unit = descs.astype(np.float64) / np.linalg.norm(descs.astype(np.float64), axis=1, keepdims=True)
    full = unit @ unit.T
    for q in range(5 * per):                                             # no row is excluded
        others = np.delete(full[q], q)
        kth = np.sort(others)[-k]
        assert (rows[q] >= 0).all() and q not in rows[q] and len(set(rows[q])) == k
        assert (full[q, rows[q]] >= kth - 1e-5).all(), q
        assert np.abs(sims[q] - full[q, rows[q]]).max() <= 1e-5 and (np.diff(sims[q]) <= 0).all()
    for i, j in planted:
        assert rows[i][0] == j and rows[j][0] == i
    cpu_rows, _ = index.search([3, 70], k=k, other_images_only=False)
    assert np.array_equal(cpu_rows[:, 0], rows[[3, 70], 0])
    other, _ = index.search([3], k=k, device=DEV)
    assert other[0][0] == 100 and (index.image[other[0][other[0] >= 0]] != 0).all()


# ---- end to end on a tiny model
RES = 48


@pytest.fixture(scope="module")
def demo(tmp_path_factory):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    tmp = tmp_path_factory.mktemp("region_pool_demo")
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
    return tmp, ck, d, LitUnsupervisedSegmenter.load_from_checkpoint(str(ck)).eval().to(DEV)


def _run_demo(demo, name, *extra):
    from stego_amd import demo_segmentation as DS
    from stego_amd.train_segmentation import load_config
    tmp, ck, d = demo[:3]
    cfg = load_config(DS.DEMO_CONFIG, overrides=["output_root=%s" % tmp, "model_path=%s" % ck, "image_dir=%s" % d, "experiment_name=%s" % name,
                                                 "res=%d" % RES, "batch_size=2", "num_workers=0", "run_crf=False"] + list(extra))
    return DS.my_app(cfg), os.path.join(str(tmp), "results", "predictions", name)


@pytest.mark.parametrize("pooled", ["code", "feats"])
def test_demo_writes_the_index(demo, pooled):
    from stego_amd.data import image_transform
    from stego_amd.segment import segment
    written, out = _run_demo(demo, "index_" + pooled, "save_regions=True", "save_region_index=True", "region_descriptor=" + pooled)
    assert sorted(os.listdir(out)) == ["cluster", "linear", "region_ids", "regions"]
    assert sorted(os.listdir(os.path.join(out, "regions"))) == ["index.npz", "tall.json", "wide.json"]
    index = D.RegionIndex.load(os.path.join(out, "regions", "index.npz"))
    tf = image_transform(RES, "center")
    names = ["tall.png", "wide.jpg"]
    img = torch.stack([tf(Image.open(demo[2] / n).convert("RGB")) for n in names]).to(DEV)
    maps = {}
    _, clu = segment(demo[3], img, run_crf=False, maps=maps)
    ids, n = R.label_regions(clu.contiguous(), 4)
    table = R.region_table(clu.contiguous(), ids, n)
    want = D.region_descriptors(ids, table, maps[pooled].detach().float(), normalize=True)
    assert index.names == names and index.pooled == pooled and len(index) == len(table) == sum(table.n_regions)
    assert index.descriptors.shape == (len(table), maps[pooled].shape[1]) and np.array_equal(index.descriptors, want.cpu().numpy())
    assert np.array_equal(index.area, table.area.cpu().numpy()) and np.array_equal(index.label, table.label.cpu().numpy())
    assert np.array_equal(index.image, np.repeat([0, 1], table.n_regions))
    row = index.row_of("wide.jpg", D.region_at(ids, 1, 20, 30))
    assert index.row_info(row)["region"] == int(ids[1, 30, 20]) and index.search([row], k=3, device=DEV)[0].shape == (1, 3)


def test_demo_without_the_key_and_under_full_res_writes_no_index(demo, capsys):
    _, out = _run_demo(demo, "index_off", "save_regions=True")
    assert sorted(os.listdir(os.path.join(out, "regions"))) == ["tall.json", "wide.json"]
    _, out = _run_demo(demo, "index_full", "save_regions=True", "save_region_index=True", "full_res=True")
    assert sorted(os.listdir(os.path.join(out, "regions"))) == ["tall.json", "wide.json"]
    assert capsys.readouterr().out.count("save_region_index: no index under full_res") == 1
