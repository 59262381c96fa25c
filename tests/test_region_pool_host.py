"""Region descriptors without a GPU: the C ABI's surface and host checks (include/stego_region_pool.h), the torch chain of
stego_amd/region_descriptors.py against the float64 oracle of tests/region_pool_oracle.py, the slab arithmetic of the byte budget,
RegionIndex (round trip, row_of, search on the CPU chain) and find_objects end to end on a two-image index."""
import json
import os
import re

import numpy as np
import pytest
import torch

import region_pool_oracle as PO
import regions_oracle as O
from stego_amd import capi
from stego_amd import region_descriptors as D
from stego_amd import regions as R

A = 0x10000          # an aligned stand-in address: the checks reject before any pointer is read
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stego_region_pool.h")).read()
SYMBOLS = ("stego_region_pool_workspace_bytes", "stego_region_pool_plan", "stego_region_pool")
MAP = capi.StegoMap(A, 1, 1, 1, 1)
PATTERNS = {"uniform": O.uniform, "checkerboard": O.checkerboard, "comb": O.comb, "spiral": O.spiral,
            "negatives": lambda H, W: O.with_negatives(H, W, 5)}
SHAPES = [((7, 7), (7, 7)), ((5, 5), (40, 40)), ((5, 7), (33, 67)), ((9, 4), (4, 9)), ((3, 5), (1, 12)), ((4, 2), (9, 1))]


def _desc(B=2, C=70, h=5, w=7, H=33, W=67, rows=10):
    return capi.region_pool_desc(B, C, h, w, H, W, rows)


def _call(desc, lo=0, hi=10, capacity=10, map_=MAP, ids=A, row_offset=A, area=A, out=A, ws=A, ws_bytes=1 << 40):
    return capi.region_pool_raw(desc, map_, ids, row_offset, area, capacity, lo, hi, out, ws, ws_bytes)


def test_symbols_abi_and_error_constants():
    lib = capi.load()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, HEADER), name
        decl = re.search(r"\b%s\((.*?)\);" % name, HEADER, re.S).group(1)
        assert len(decl.split(",")) == len(capi.SIGNATURES[name][1]), name
    assert lib.stego_abi_version() == capi.ABI_VERSION
    names = ("SIZE", "DIM", "RANGE")
    for i, name in enumerate(names):
        rc = getattr(capi, "REGION_POOL_ERR_" + name)
        assert rc == 200 + i and re.search(r"STEGO_ERR_REGION_POOL_%s = %d\b" % (name, rc), HEADER), name
        assert lib.stego_error_string(rc).decode().startswith("region pool:"), rc
    assert len(re.findall(r"STEGO_ERR_REGION_POOL_\w+ = \d+", HEADER)) == len(names)
    for name in ("MAX_C", "CB", "PARTIALS", "LAUNCHES"):
        assert re.search(r"#define STEGO_REGION_POOL_%s %d\b" % (name, getattr(capi, "REGION_POOL_" + name)), HEADER), name
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct StegoRegionPoolDesc \{(.*?)\} StegoRegionPoolDesc;", HEADER, re.S).group(1),
                  flags=re.S)
    fields = [f.strip() for line in body.split(";") if "int" in line for f in re.sub(r"int(32|64)_t", "", line).split(",")]
    assert fields == [f for f, _ in capi.StegoRegionPoolDesc._fields_]


def test_every_limit_at_its_edge_before_any_hip_call():
    """A good descriptor is recognised by the host-only exports; a call with stand-in pointers is only ever made where a check rejects it
    (or hi == lo ends it), so nothing is enqueued on a machine that has a device."""
    S, Dm, Rg = capi.REGION_POOL_ERR_SIZE, capi.REGION_POOL_ERR_DIM, capi.REGION_POOL_ERR_RANGE
    cases = [(_desc(B=0), S), (_desc(B=1), 0), (_desc(B=65535), 0), (_desc(B=65536), S),
             (_desc(H=65536, W=32768), S), (_desc(H=1, W=(1 << 31) - 1), 0), (_desc(H=0), S), (_desc(W=0), S),
             (_desc(h=0), S), (_desc(w=0), S), (_desc(h=1, w=1), 0),
             (_desc(C=0), Dm), (_desc(C=1), 0), (_desc(C=2048), 0), (_desc(C=2049), Dm),
             (_desc(rows=-1), Rg), (_desc(rows=0), 0), (_desc(C=2048, rows=(1 << 20) - 1), 0), (_desc(C=2048, rows=1 << 20), Rg)]
    for desc, rc in cases:
        got, seg, cb, launches = capi.region_pool_plan(desc)
        assert got == rc, (desc.B, desc.C, desc.h, desc.w, desc.H, desc.W, desc.rows, rc)
        assert (capi.region_pool_workspace_bytes(desc) == 0) == (rc != 0)
        if rc:
            assert seg == 0 and cb == 0 and launches == [(0, 0)] * capi.REGION_POOL_LAUNCHES
            assert _call(desc) == rc and _call(desc, hi=0) == rc                       # the descriptor comes first, also for no rows
    ok = _desc()
    for lo, hi, cap in ((-1, 2, 10), (3, 2, 10), (0, 11, 10), (0, 1, 0)):
        assert _call(ok, lo, hi, cap) == Rg, (lo, hi, cap)
    wide = _desc(C=2048, rows=0)
    assert _call(wide, 0, 1 << 20, 1 << 20) == Rg                                          # (hi - lo) * C = 2^31
    assert _call(wide, 0, (1 << 20) - 1, 1 << 20, ws_bytes=0) == 4                         # one row fewer passes the range: STEGO_ERR_WORKSPACE
    assert _call(wide, 5, (1 << 20) + 4, (1 << 20) + 4, ws_bytes=0) == 4                   # the limit is on hi - lo, hi == capacity is legal
    for lo in (0, 4, 10):
        assert _call(ok, lo, lo, 10) == 0 and _call(ok, lo, lo, 10, None, None, None, None, None, None, 0) == 0   # hi == lo does nothing
    for k in ("map_", "ids", "row_offset", "area", "out", "ws"):
        assert _call(ok, **{k: None}) == 1, k                                              # STEGO_ERR_NULL
    assert _call(ok, map_=capi.StegoMap(None, 1, 1, 1, 1)) == 1
    need = capi.region_pool_workspace_bytes(ok)
    assert need == capi.REGION_POOL_PARTIALS * 4 + 10 * 70 * 8
    assert _call(ok, ws_bytes=need - 1) == 4 and _call(ok, 0, 9, ws_bytes=need - 70 * 8 - 1) == 4
    for k, off in (("ids", 2), ("row_offset", 4), ("area", 2), ("out", 2), ("ws", 8)):
        assert _call(ok, ws_bytes=need, **{k: A + off}) == 5, k                            # STEGO_ERR_ALIGN
    assert _call(ok, ws_bytes=need, map_=capi.StegoMap(A + 2, 1, 1, 1, 1)) == 5


def test_plan_values():
    for (B, C, H, W, rows), seg in (((2, 70, 33, 67, 10), 64), ((1, 33, 5, 64, 1), 64), ((1, 32, 5, 129, 1), 128), ((1, 17, 5, 129, 1), 128),
                                    ((1, 16, 5, 300, 1), 256), ((1, 8, 1, 513, 3), 512), ((1, 3, 4800, 4800, 1000), 512),
                                    ((1, 1, 1, 1, 1), 512), ((16, 768, 320, 320, 4000), 64)):
        rc, L, cb, launches = capi.region_pool_plan(capi.region_pool_desc(B, C, 5, 7, H, W, rows))
        assert rc == 0 and L == seg and cb == capi.REGION_POOL_CB == 128 and len(launches) == 3
        nseg = -(-W // L)
        assert launches[1][1] == -(-H * nseg // 4) * -(-C // cb) * B, (B, C, H, W)
        assert launches[0][1] == min(capi.REGION_POOL_PARTIALS, -(-B * C * 35 // 4096)) and launches[2][1] == -(-rows * C // 1024)
        assert all(lds == 16 for lds, _ in launches)


def test_slabs_cover_every_row_once():
    for n, C, budget in ((0, 70, 1 << 20), (1, 70, 1), (10, 70, 559), (10, 70, 560), (10, 70, 1120), (1000, 3, 240), (7, 2048, 1 << 28),
                         (5, 1, 1 << 40)):
        slabs = D.pool_slabs(n, C, budget)
        assert [lo for lo, _ in slabs] == [0] * bool(n) + [hi for _, hi in slabs[:-1]] and (not n or slabs[-1][1] == n)
        assert all(hi > lo for lo, hi in slabs)
        assert all((hi - lo) * C * 8 <= budget or hi - lo == 1 for lo, hi in slabs) and all((hi - lo) * C < 1 << 31 for lo, hi in slabs)
    assert len(D.pool_slabs(10, 70, 1120)) == 5 and len(D.pool_slabs(10, 70, 559)) == 10


def _table(pattern, H, W, B=1):
    lab = torch.from_numpy(np.stack([pattern(H, W) for _ in range(B)]))
    ids, n = R.label_regions(lab, 4)
    return ids, R.region_table(lab, ids, n)


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_the_chain_equals_the_oracle(name):
    """Bound: a float64 sum of n values no larger than M is off by at most n 2^-53 M, and so is its mean; the interpolation adds a
    handful of roundings more: (n + 16) 2^-53 M with n = H W.  Observed maximum over all cases: 0 (M about 4) - on the CPU index_add_ and np.add.at add in the
    same order, and the interpolation is the same expression."""
    worst = 0.0
    for k, ((h, w), (H, W)) in enumerate(SHAPES):
        ids, table = _table(PATTERNS[name], H, W, B=2)
        maps = torch.from_numpy(np.random.default_rng(k).standard_normal((2, 6, h, w)).astype(np.float32))
        for m in (maps, maps.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)):
            got = D._torch_chain_f64(ids, table, m).numpy()
            want = PO.descriptors(maps.numpy(), ids.numpy(), table.row_offset, table.area.numpy())
            err, bound = np.abs(got - want).max() if got.size else 0.0, (H * W + 16) * 2.0 ** -53 * float(maps.abs().max())
            worst = max(worst, err)
            assert got.shape == (len(table), 6) and err <= bound, (name, h, w, H, W, err, bound)
            pub = D.region_descriptors(ids, table, m)
            assert pub.dtype == torch.float32 and np.array_equal(pub.numpy(), got.astype(np.float32))
    print("worst", worst)


def test_normalize_rows_without_pixels_and_argument_errors():
    ids, table = _table(lambda H, W: O.with_negatives(H, W, 5), 9, 11, B=2)
    maps = torch.randn(2, 5, 3, 4, generator=torch.Generator().manual_seed(0))
    want = D.region_descriptors(ids, table, torch.nn.functional.normalize(maps, dim=1))
    assert torch.equal(D.region_descriptors(ids, table, maps, normalize=True), want)
    gone = ids.clone()
    gone[gone == 0] = -1                                             # region 0 of both images loses its pixels; the table still has the rows
    got = D.region_descriptors(gone, table, maps)
    assert torch.equal(got[table.row_offset[1]], torch.zeros(5)) and torch.equal(got[0], torch.zeros(5)) and torch.isfinite(got).all()
    keep = torch.ones(len(table), dtype=torch.bool)
    keep[[0, table.row_offset[1]]] = False
    assert torch.equal(got[keep], D.region_descriptors(ids, table, maps)[keep])
    assert D.region_at(ids, 1, 3, 2) == int(ids[1, 2, 3]) and D.region_at(ids[0].numpy(), 0, 10, 8) == int(ids[0, 8, 10])
    assert D.region_at(ids, 0, 11, 0) == -1 and D.region_at(ids, 2, 0, 0) == -1 and D.region_at(ids, 0, 0, -1) == -1
    for call in (lambda: D.region_descriptors(ids.long(), table, maps), lambda: D.region_descriptors(ids, table, maps[0]),
                 lambda: D.region_descriptors(ids, table, maps[:1]), lambda: D.region_descriptors(ids, table, maps, pool_bytes=0),
                 lambda: D.RegionIndex("logits")):
        with pytest.raises(ValueError):
            call()


def _planted_index():
    """Three images with 6, 5 and 4 regions, C = 8: random descriptors, and row 0 of image "a" planted, slightly perturbed, as region 2 of
    "b" (area 3: small) and region 1 of "c", and a little further off as region 3 of "a" itself."""
    rng = np.random.default_rng(0)
    index, descs = D.RegionIndex("code"), []
    for name, n in (("a.jpg", 6), ("b.jpg", 5), ("c.jpg", 4)):
        cols = {c: torch.arange(n, dtype=torch.int64) + 10 for c in R.RegionTable.COLUMNS}
        cols["area"] = torch.full((n,), 50, dtype=torch.int64)
        descs.append(rng.standard_normal((n, 8)).astype(np.float32))
        index_args = (name, R.RegionTable(cols, [n], 64), 0)
        if name == "a.jpg":
            descs[-1][3] = descs[0][0] + 0.05 * rng.standard_normal(8).astype(np.float32)
        if name == "b.jpg":
            descs[-1][2] = descs[0][0] * 3 + 0.001
            cols["area"][2] = 3
        if name == "c.jpg":
            descs[-1][1] = descs[0][0] + 0.01 * rng.standard_normal(8).astype(np.float32)
        index.add(*index_args, torch.from_numpy(descs[-1]))
    return index, np.concatenate(descs)


def test_region_index_round_trip_row_of_and_search(tmp_path):
    index, descs = _planted_index()
    assert len(index) == 15 and np.array_equal(index.descriptors, descs) and index.names == ["a.jpg", "b.jpg", "c.jpg"]
    assert index.row_of("a.jpg", 0) == 0 and index.row_of("b.jpg", 2) == 8 and index.row_of("c.jpg", 3) == 14
    for bad in (("d.jpg", 0), ("b.jpg", 5)):
        with pytest.raises(KeyError):
            index.row_of(*bad)
    assert index.row_info(8) == {"image": "b.jpg", "region": 2, "label": 12, "area": 3, "box": [12, 12, 12, 12]}
    back = D.RegionIndex.load(index.save(str(tmp_path / "index.npz")))
    assert back.names == index.names and back.pooled == "code" and len(back) == 15
    for k in ("descriptors", "image", "region", "label", "area", "box"):
        assert getattr(back, k).dtype == getattr(index, k).dtype and getattr(back, k).tobytes() == getattr(index, k).tobytes(), k
    for ix in (index, back):
        rows, sims = ix.search([0], k=3)
        assert rows.shape == sims.shape == (1, 3) and rows.dtype == np.int64 and sims.dtype == np.float32
        assert list(rows[0][:2]) == [8, 12] and sims[0][0] > sims[0][1] > 0.99 > sims[0][2]           # the planted ones first
        assert 3 not in rows[0] and 0 not in rows[0]
        rows, sims = ix.search([0], k=3, min_area=4)
        assert rows[0][0] == 12 and 8 not in rows[0]
        rows, sims = ix.search([0, 8], k=4, other_images_only=False)
        assert list(rows[0][:3]) == [8, 12, 3] and list(rows[1][:2]) == [0, 12] and (rows[0] != 0).all() and (rows[1] != 8).all()
    unit = descs / np.linalg.norm(descs, axis=1, keepdims=True)
    rows, sims = index.search(np.arange(15), k=5, other_images_only=False)
    full = unit.astype(np.float64) @ unit.astype(np.float64).T
    for q in range(15):
        assert np.allclose(sims[q], full[q, rows[q]], atol=1e-6) and full[q, rows[q]].min() >= np.sort(np.delete(full[q], q))[-5] - 1e-6


def test_fewer_than_k_survivors_are_padded():
    index, _ = _planted_index()
    rows, sims = index.search([0], k=12)                                # 9 rows live in other images
    assert (rows[0][:9] >= 6).all() and len(set(rows[0][:9])) == 9 and (rows[0][9:] == -1).all()
    assert np.isfinite(sims[0][:9]).all() and (np.diff(sims[0][:9]) <= 0).all() and np.isneginf(sims[0][9:]).all()
    rows, sims = index.search([0], k=2, min_area=51)
    assert (rows == -1).all() and np.isneginf(sims).all()
    assert D.RegionIndex().search([], k=3)[0].shape == (0, 3)
    with pytest.raises(ValueError):
        index.search([15])


def test_find_objects_names_the_planted_match(tmp_path):
    """Two 12 x 16 images of two halves each; the left half of a.png and the right half of b.png carry the same colour."""
    from stego_amd import find_objects as F
    from stego_amd.train_segmentation import load_config
    (tmp_path / "regions").mkdir()
    (tmp_path / "region_ids").mkdir()
    lab = torch.zeros(2, 12, 16, dtype=torch.int64)
    lab[:, :, 8:] = 1
    ids, n = R.label_regions(lab, 4)
    table = R.region_table(lab, ids, n)
    colours = {(0, 0): (1.0, 0.2, 0.1), (0, 1): (0.1, 0.9, 0.3), (1, 0): (0.2, 0.1, 1.0), (1, 1): (0.98, 0.22, 0.1)}
    maps = torch.zeros(2, 3, 12, 16)
    for (b, half), rgb in colours.items():
        maps[b, :, :, 8 * half:8 * half + 8] = torch.tensor(rgb)[:, None, None]
    descs = D.region_descriptors(ids, table, maps)
    index = D.RegionIndex("feats")
    for b, name in enumerate(("a.png", "b.png")):
        index.add(name, table, b, descs[table.rows(b)])
        id_map = R.write_id_map(str(tmp_path / "region_ids" / name[0]), ids[b], table.n_regions[b])
        R.write_regions(str(tmp_path / "regions" / (name[0] + ".json")), table, b, 12, 16, 4, id_map=os.path.basename(id_map))
    path = index.save(str(tmp_path / "regions" / "index.npz"))
    out = str(tmp_path / "matches.json")
    cfg = load_config(F.FIND_CONFIG, overrides=["index=" + path, "image=a.png", "x=3", "y=5", "k=2", "out=" + out, "device=cpu"])
    result = F.my_app(cfg)
    assert result == json.load(open(out))
    assert result["query"]["image"] == "a.png" and result["query"]["region"] == 0 and result["query"]["pooled"] == "feats"
    best = result["matches"][0]
    assert (best["image"], best["region"], best["label"], best["area"], best["box"]) == ("b.png", 1, 1, 96, [8, 0, 15, 11])
    assert best["similarity"] > 0.999 > result["matches"][1]["similarity"] and len(result["matches"]) == 2
    with pytest.raises(ValueError):
        F.my_app(load_config(F.FIND_CONFIG, overrides=["index=" + path, "image=a.png", "x=16", "y=5"]))


def test_configs_load_with_the_keys_off():
    from stego_amd.demo_segmentation import DEMO_CONFIG
    from stego_amd.find_objects import FIND_CONFIG
    from stego_amd.train_segmentation import load_config
    demo, find = load_config(DEMO_CONFIG), load_config(FIND_CONFIG)
    assert demo.save_region_index is False and demo.region_descriptor == "code" and demo.save_regions is False
    assert find.k == 8 and find.min_area == 0 and find.other_images_only is True and find.out is None and find.image is None
