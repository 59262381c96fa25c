"""Segments as objects without a GPU: the C ABI's surface and host checks (include/stego_regions.h), the numpy chain of
stego_amd/regions.py against the explicit-loop oracle of tests/regions_oracle.py, the slab arithmetic of the vote budget, the JSON and
id-map writers, and the config files with the new keys off."""
import json
import os
import re

import numpy as np
import pytest
import torch

import regions_oracle as O
from stego_amd import capi
from stego_amd import regions as R

A = 0x10000          # an aligned stand-in address: the checks reject before any pointer is read
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stego_regions.h")).read()
SYMBOLS = ("stego_regions_workspace_bytes", "stego_regions_plan", "stego_regions_label", "stego_regions_table", "stego_regions_votes",
           "stego_regions_relabel")
SIZES = [(1, 1), (1, 7), (7, 1), (13, 17), (40, 33)]


def test_symbols_abi_and_error_constants():
    lib = capi.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, HEADER), name
    assert lib.stego_abi_version() == 7 == capi.ABI_VERSION
    names = ("SIZE", "CONN", "DTYPE", "LABELS", "RANGE")
    for i, name in enumerate(names):
        rc = getattr(capi, "REGIONS_ERR_" + name)
        assert rc == 190 + i and re.search(r"STEGO_ERR_REGIONS_%s = %d\b" % (name, rc), HEADER), name
        assert lib.stego_error_string(rc).decode().startswith("regions:"), rc
    assert len(re.findall(r"STEGO_ERR_REGIONS_\w+ = \d+", HEADER)) == len(names)
    for name in ("TILE", "CHUNK", "MAX_LABELS", "LAUNCHES"):
        assert re.search(r"#define STEGO_REGIONS_%s %d\b" % (name, getattr(capi, "REGIONS_" + name)), HEADER), name
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct StegoRegionsDesc \{(.*?)\} StegoRegionsDesc;", HEADER, re.S).group(1), flags=re.S)
    fields = [f.strip() for line in body.split(";") if "int32_t" in line for f in line.replace("int32_t", "").split(",")]
    assert fields == [f for f, _ in capi.StegoRegionsDesc._fields_]


def test_signatures_have_the_headers_argument_counts():
    for name in SYMBOLS:
        decl = re.search(r"\b%s\((.*?)\);" % name, HEADER, re.S).group(1)
        assert len(decl.split(",")) == len(capi.SIGNATURES[name][1]), name


def test_descriptor_errors_come_before_any_hip_call():
    ok = capi.regions_desc(2, 40, 33, 4, capi.REGIONS_I64)
    assert capi.regions_workspace_bytes(ok) > 0
    bad = [(capi.regions_desc(2, 40, 33, 6), capi.REGIONS_ERR_CONN), (capi.regions_desc(2, 40, 33, 0), capi.REGIONS_ERR_CONN),
           (capi.regions_desc(1, 65536, 32768), capi.REGIONS_ERR_SIZE),              # H * W = 2^31: nothing is allocated for it
           (capi.regions_desc(1, 1, (1 << 31) - 1), 0), (capi.regions_desc(0, 4, 4), capi.REGIONS_ERR_SIZE),
           (capi.regions_desc(65536, 4, 4), capi.REGIONS_ERR_SIZE), (capi.regions_desc(1, 0, 4), capi.REGIONS_ERR_SIZE),
           (capi.regions_desc(1, 4, 4, 4, 3), capi.REGIONS_ERR_DTYPE)]
    for desc, rc in bad:
        assert capi.regions_plan(desc)[0] == rc, (desc.H, desc.W, rc)
        assert (capi.regions_workspace_bytes(desc) == 0) == (rc != 0)
        if rc:
            assert capi.regions_label_raw(desc, A, A, A, A, A, 1 << 20) == rc
            assert capi.regions_table_raw(desc, A, A, A, 4, A, A) == rc
            assert capi.regions_votes_raw(desc, A, A, A, 4, A, 0, 2, 5, A) == rc
            assert capi.regions_relabel_raw(desc, A, A, A, A, 4, A, A, 0, 2, 5, A, A) == rc
    for n_labels in (0, 257, -1):
        assert capi.regions_votes_raw(ok, A, A, A, 4, A, 0, 2, n_labels, A) == capi.REGIONS_ERR_LABELS
        assert capi.regions_relabel_raw(ok, A, A, A, A, 4, A, A, 0, 2, n_labels, A, A) == capi.REGIONS_ERR_LABELS
    for lo, hi in ((-1, 2), (3, 2), (0, 1 << 31)):
        assert capi.regions_votes_raw(ok, A, A, A, 4, A, lo, hi, 5, A) == capi.REGIONS_ERR_RANGE
    assert capi.regions_table_raw(ok, A, A, A, -1, A, A) == capi.REGIONS_ERR_RANGE
    assert capi.regions_label_raw(ok, None, A, A, A, A, 1 << 20) == 1              # STEGO_ERR_NULL
    assert capi.regions_label_raw(ok, A, A, A, A, A, 0) == 4                       # STEGO_ERR_WORKSPACE
    assert capi.regions_label_raw(ok, A + 4, A, A, A, A, 1 << 20) == 5             # int64 labels on 4 bytes: STEGO_ERR_ALIGN
    assert capi.regions_label_raw(capi.regions_desc(2, 40, 33, 4, capi.REGIONS_U8), A + 1, A, A, A, A + 8, 1 << 20) == 5   # the workspace
    assert capi.regions_table_raw(ok, A, A + 2, A, 4, A, A) == 5
    assert capi.regions_table_raw(ok, A, A, A, 0, None, None) == 0                 # an empty table is legal


def test_python_argument_errors():
    lab = torch.zeros(1, 4, 6, dtype=torch.int64)
    for call in (lambda: R.label_regions(lab, 6), lambda: R.label_regions(lab.transpose(1, 2), 4),
                 lambda: R.label_regions(lab[0], 4), lambda: R.label_regions(lab.float(), 4),
                 lambda: R.label_regions(torch.empty((1, 65536, 32768), dtype=torch.uint8, device="meta"), 4),
                 lambda: R.merge_small_regions(lab, 0, 5), lambda: R.merge_small_regions(lab, 4, 0),
                 lambda: R.merge_small_regions(lab, 4, 257), lambda: R.merge_small_regions(lab, 4, 5, connectivity=5),
                 lambda: R.merge_small_regions(lab, 4, 5, vote_bytes=0), lambda: R.cleanup_round(lab.transpose(1, 2), 4, 5)):
        with pytest.raises(ValueError):
            call()


def test_plan_values():
    T = capi.REGIONS_TILE
    for (B, H, W), tiles, seams in (((1, 1, 1), 1, 0), ((2, T, T), 2, 0), ((1, T + 1, T), 2, 1), ((3, 2 * T + 1, 2 * T + 3), 27, 3 * 2),
                                    ((1, 4800, 4800), 22500, 5588)):
        rc, tile, launches = capi.regions_plan(capi.regions_desc(B, H, W, 8))
        chunks = -(-H * W // capi.REGIONS_CHUNK) * B
        assert rc == 0 and tile == T and len(launches) == capi.REGIONS_LAUNCHES
        assert [w for _, w in launches] == [tiles, seams, chunks, B, chunks, chunks], (B, H, W, launches)
        assert launches[0][0] == T * T * 12 and all(lds < 160 * 1024 for lds, _ in launches)
        assert capi.regions_workspace_bytes(capi.regions_desc(B, H, W)) >= 4 * chunks
    rc, tile, launches = capi.regions_plan(capi.regions_desc(1, 4, 4, 5))
    assert rc == capi.REGIONS_ERR_CONN and tile == 0 and launches == [(0, 0)] * capi.REGIONS_LAUNCHES


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(O.PATTERNS))
def test_the_chain_equals_the_oracle(name, connectivity):
    for H, W in SIZES:
        m = O.PATTERNS[name](H, W)
        w_ids, w_n = O.label(m, connectivity)
        lab = torch.from_numpy(m)[None]
        ids, n = R.label_regions(lab, connectivity)
        assert ids.dtype == torch.int32 and n.dtype == torch.int32
        assert int(n[0]) == w_n and np.array_equal(ids[0].numpy(), w_ids), (H, W)
        table, want = R.region_table(lab, ids, n), O.table(m, w_ids, w_n)
        for c in O.COLUMNS:
            assert np.array_equal(getattr(table, c).numpy(), want[c]), (H, W, c)
        if w_n:
            assert np.array_equal(table.centroids().numpy(), np.stack([want["sum_y"] / want["area"], want["sum_x"] / want["area"]], 1))


def test_the_chain_on_a_batch_and_other_dtypes():
    maps = [O.random_map(13, 17, 3, 1), np.full((13, 17), -1, dtype=np.int64), O.comb(13, 17)]
    for dtype in (torch.int64, torch.int16, torch.uint8):
        use = [m for m in maps if dtype != torch.uint8 or m.min() >= 0]
        ids, n = R.label_regions(torch.from_numpy(np.stack(use)).to(dtype), 4)
        table = R.region_table(torch.from_numpy(np.stack(use)).to(dtype), ids, n)
        for b, m in enumerate(use):
            w_ids, w_n = O.label(m, 4)
            assert int(n[b]) == w_n == table.n_regions[b] and np.array_equal(ids[b].numpy(), w_ids)
            assert np.array_equal(table.area[table.rows(b)].numpy(), O.table(m, w_ids, w_n)["area"])


def test_the_partition_is_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    for connectivity, structure in ((4, None), (8, np.ones((3, 3)))):
        for m in (O.random_map(40, 33, 3, 5), O.rings(40, 33), O.spiral(40, 33), O.with_negatives(40, 33, 2)):
            ids, n = O.label(m, connectivity)
            pairs, total = set(), 0
            for c in np.unique(m[m >= 0]):
                theirs, k = ndi.label(m == c, structure=structure)
                total += k
                pairs |= {(int(c), int(t), int(i)) for t, i in zip(theirs[m == c], ids[m == c])}
            assert n == total == len(pairs) and (ids[m < 0] == -1).all()          # a bijection between their pieces and the ids


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("min_area", [2, 6, 50])
def test_the_cleanup_chain_equals_the_oracle(min_area, connectivity):
    maps = np.stack([O.blocky(40, 37, seed=min_area), O.blocky(40, 37, block=7, seed=1)])
    want, w_rounds = O.merge_batch(maps, min_area, 5, connectivity)
    for dtype in (torch.int64, torch.uint8):
        got, rounds = R.merge_small_regions(torch.from_numpy(maps).to(dtype), min_area, 5, connectivity)
        assert got.dtype == dtype and rounds == w_rounds and np.array_equal(got.numpy().astype(np.int64), want)


def test_two_properties_of_the_cleanup():
    m = O.blocky(96, 96, seed=3)
    got, rounds = R.merge_small_regions(torch.from_numpy(m)[None], 6, 5)
    first, _ = O.cleanup_round(m, 6, 5)
    assert rounds == 2 and np.array_equal(got[0].numpy(), first)                     # clean after one round
    ids, n = O.label(first, 4)
    assert (O.table(first, ids, n)["area"] >= 6).all()
    noise = O.random_map(40, 40, 27, 1)
    got, rounds = R.merge_small_regions(torch.from_numpy(noise)[None], 16, 27)
    assert rounds == 1 and np.array_equal(got[0].numpy(), noise)                     # no region has a neighbour that is not small


def test_tie_no_votes_and_the_round_limit():
    m = np.array([[2, 2, 2, 1, 1, 1, 1], [2, 2, 2, 5, 1, 1, 1], [2, 2, 2, 2, 1, 1, 1]], dtype=np.int64)
    assert O.merge(m, 2, 6)[0][1, 3] == 1 == int(R.merge_small_regions(torch.from_numpy(m)[None], 2, 6)[0][0, 1, 3])
    m = np.zeros((7, 7), dtype=np.int64)
    m[3, 3], m[2, 3], m[4, 3], m[3, 2], m[3, 4] = 7, 3, 4, 5, 6
    one, rounds = R.merge_small_regions(torch.from_numpy(m)[None], 2, 8, max_rounds=1)
    assert rounds == 1 and int(one[0, 3, 3]) == 7 and int((one != 0).sum()) == 1 and np.array_equal(one[0].numpy(), O.merge(m, 2, 8, 4, 1)[0])
    full, rounds = R.merge_small_regions(torch.from_numpy(m)[None], 2, 8)
    assert rounds == 3 == O.merge(m, 2, 8)[1] and int((full != 0).sum()) == 0
    # a label at or beyond n_labels casts no vote
    m = np.array([[9, 9, 9], [9, 1, 9], [9, 9, 9]], dtype=np.int64)
    got, _ = R.merge_small_regions(torch.from_numpy(m)[None], 2, 5)
    assert np.array_equal(got[0].numpy(), m) and np.array_equal(O.merge(m, 2, 5)[0], m)


def test_vote_slabs():
    assert R.vote_slabs(0, 5, 100) == []
    assert R.vote_slabs(7, 5, 2 ** 28) == [(0, 7)]
    assert R.vote_slabs(7, 5, 4 * 5 * 3) == [(0, 3), (3, 6), (6, 7)]
    assert R.vote_slabs(3, 256, 1) == [(0, 1), (1, 2), (2, 3)]                       # a budget below one row: one row a slab
    noise = 4800 * 4800
    assert all((hi - lo) * 27 * 4 <= 2 ** 28 for lo, hi in R.vote_slabs(noise, 27, 2 ** 28)) and len(R.vote_slabs(noise, 27, 2 ** 28)) == 10
    m = O.blocky(40, 37, seed=2)
    ids, n = O.label(m, 4)
    n_small = int((O.table(m, ids, n)["area"] < 6).sum())
    one, r1 = R.merge_small_regions(torch.from_numpy(m)[None], 6, 5)
    each, r2 = R.merge_small_regions(torch.from_numpy(m)[None], 6, 5, vote_bytes=4 * 5)      # one row: a slab per small region
    assert len(R.vote_slabs(n_small, 5, 4 * 5)) == n_small > 3 and r1 == r2 and torch.equal(one, each)


def test_json_and_id_maps_round_trip(tmp_path):
    m = O.random_map(13, 17, 4, 6)
    lab = torch.from_numpy(np.stack([O.rings(13, 17), m]))
    ids, n = R.label_regions(lab, 8)
    table = R.region_table(lab, ids, n)
    class_of = [5, 6, -1]
    doc = R.regions_to_json(table, 1, 13, 17, 8, class_of=class_of, id_map="x.png")
    assert doc == {"height": 13, "width": 17, "connectivity": 8, "id_map": "x.png", "regions": O.region_dicts(m, 8, class_of)}
    assert {r["class"] for r in doc["regions"]} == {5, 6, -1, None}
    assert sorted(doc["regions"][0]) == ["area", "bbox", "centroid", "class", "first", "id", "label"]
    path = R.write_regions(str(tmp_path / "r.json"), table, 1, 13, 17, 8, class_of=np.asarray(class_of))
    with open(path) as f:
        back = json.load(f)
    del doc["id_map"]
    assert back == doc
    assert all(r["class"] is None for r in R.regions_to_json(table, 0, 13, 17, 8)["regions"])
    # the id map: a 16-bit PNG below 65536 regions, int32 .npy from there on
    from PIL import Image
    with_hole = ids[1].numpy().copy()
    with_hole[0, 0] = -1
    p = R.write_id_map(str(tmp_path / "a"), with_hole, int(n[1]))
    assert p.endswith("a.png") and Image.open(p).mode == "I;16" and np.array_equal(R.read_id_map(p), with_hole)
    assert np.array_equal(np.asarray(Image.open(p))[1:], with_hole[1:])
    many = np.arange(300 * 300, dtype=np.int32).reshape(300, 300)
    p = R.write_id_map(str(tmp_path / "b"), many, 65535)
    assert p.endswith("b.png") and np.array_equal(R.read_id_map(p)[:200], many[:200])
    p = R.write_id_map(str(tmp_path / "c"), torch.from_numpy(many), 65536)
    assert p.endswith("c.npy") and np.load(p).dtype == np.int32 and np.array_equal(R.read_id_map(p), many)
    # a synthetic table of 65536 one-pixel regions: the JSON has them all
    big = R.RegionTable({c: torch.zeros(65536, dtype=torch.int64) if c != "area" else torch.ones(65536, dtype=torch.int64)
                         for c in R.RegionTable.COLUMNS}, [65536], 256)
    assert len(R.regions_to_json(big, 0, 256, 256, 4)["regions"]) == 65536


def test_configs_load_with_the_keys_off():
    from stego_amd.demo_segmentation import DEMO_CONFIG
    from stego_amd.eval_segmentation import EVAL_CONFIG
    from stego_amd.train_segmentation import load_config
    demo, ev = load_config(DEMO_CONFIG), load_config(EVAL_CONFIG)
    assert demo.save_regions is False and demo.min_region_area == 0 and demo.region_connectivity == 4
    assert ev.min_region_area == 0 and ev.region_connectivity == 4


def test_segment_and_evaluate_take_the_arguments():
    import inspect

    from stego_amd.eval_segmentation import evaluate
    from stego_amd.segment import segment, segment_large
    for fn in (segment, segment_large):
        sig = inspect.signature(fn).parameters
        assert sig["min_region_area"].default == 0 and sig["connectivity"].default == 4
    assert inspect.signature(evaluate).parameters["min_region_area"].default == 0
