"""KNN precompute: oracle vs the reference-generated golden vectors (CPU), the row-sharded
multi-rank path on gloo (CPU, oracle-backed backend double), and the HIP kernel through the C ABI (GPU)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import oracle_backend
from oracle import knn_oracle as K
from stego_amd import precompute_knns as PK

GOLD = os.path.join(os.path.dirname(__file__), "golden", "knn_small.npz")


def test_oracle_matches_reference_ops_golden():
    g = np.load(GOLD)
    idx, val = K.knn_topk(g["normed"], int(g["k"]))
    np.testing.assert_allclose(val, g["sims"], atol=1e-6)
    assert (idx == g["nns"]).mean() > 0.99                       # the rest are fp32 near-ties of the reference itself
    assert K.check_neighbours(g["normed"], g["nns"], int(g["k"]), sims=g["sims"], tol=2e-6) <= 600 // 20
    np.testing.assert_allclose(K.normalize_rows(g["feats"]), g["normed"], atol=1e-6)
    # the two duplicated rows sit at rank 0/1 of each other
    assert set(g["nns"][3, :2]) == {3, 17} and set(g["nns"][17, :2]) == {3, 17}


def test_shard_rows_cover_and_align():
    for n in (1, 127, 128, 129, 1000, 100000):
        for world in (1, 2, 3, 8):
            b = [PK.shard_rows(n, world, r) for r in range(world)]
            assert b[0][0] == 0 and b[-1][1] == n
            assert all(b[i][1] == b[i + 1][0] for i in range(world - 1))
            assert all(s % 128 == 0 for s, _ in b if s < n)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    PK._backend = oracle_backend
    g = np.load(GOLD)
    x = torch.from_numpy(g["normed"])
    q0, q1 = PK.shard_rows(x.shape[0], world, rank)
    res = PK.sharded_nearest_neighbors(x[q0:q1].clone(), k=int(g["k"]))
    if rank == 0:
        np.save(out, res.numpy())
    dist.destroy_process_group()


def test_two_rank_sharded_knn_gloo(tmp_path):
    """world_size 2: all-gather of the shards, per-rank query slices, gather to rank 0 == the single-rank table."""
    out = str(tmp_path / "nns.npy")
    mp.spawn(_shard_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    g = np.load(GOLD)
    got = np.load(out)
    ref, _ = K.knn_topk(g["normed"], int(g["k"]))
    np.testing.assert_array_equal(got, ref)


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu
DEV = "cuda:0"


def _run(x, k, **kw):
    from stego_amd import capi
    idx, sims = capi.knn_topk(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV), k=k, return_sims=True, **kw)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sims.cpu().numpy()


@gpu
def test_knn_golden_reference_vectors():
    g = np.load(GOLD)
    k = int(g["k"])
    idx, sims = _run(g["normed"], k)
    assert idx.dtype == np.int64 and idx.shape == (600, k)
    K.check_neighbours(g["normed"], idx, k, sims=sims)
    np.testing.assert_allclose(sims, g["sims"], atol=2e-5)          # the reference's own top-k similarities
    rows = np.setdiff1d(np.arange(600), [3, 17])
    np.testing.assert_array_equal(idx[rows, 0], rows)               # self at rank 0 (data.py:524 relies on it)
    assert set(idx[3, :2]) == {3, 17} and set(idx[17, :2]) == {3, 17}
    idx2, _ = _run(g["feats"], k, normalize=True)                   # F.normalize inside (precompute_knns.py:19)
    K.check_neighbours(g["normed"], idx2, k)


@gpu
@pytest.mark.parametrize("n,d,k", [(50, 7, 30), (129, 64, 1), (1000, 100, 32), (1500, 384, 30), (300, 130, 5)])
def test_knn_edge_shapes(n, d, k):
    """N below / not a multiple of the 128-row block, D straddling the 64-column chunk, k = 1 and k = 32."""
    rng = np.random.default_rng(n + d)
    x = K.normalize_rows(rng.standard_normal((n, d))).astype(np.float32)
    idx, sims = _run(x, k)
    assert idx.min() >= 0 and idx.max() < n
    K.check_neighbours(x, idx, k, sims=sims)


@gpu
def test_knn_query_slices_equal_full_table_and_are_deterministic():
    rng = np.random.default_rng(5)
    x = K.normalize_rows(rng.standard_normal((1100, 96))).astype(np.float32)
    full, fs = _run(x, 30)
    again, _ = _run(x, 30)
    np.testing.assert_array_equal(full, again)
    for q0, qc in ((0, 128), (128, 300), (1024, 76), (256, 844)):
        part, ps = _run(x, 30, q_begin=q0, q_count=qc)
        K.check_neighbours(x, part, 30, sims=ps, q_begin=q0)
        np.testing.assert_allclose(ps, fs[q0:q0 + qc], atol=2e-6)


@gpu
def test_knn_vits8_width_8k_rows_against_oracle():
    """D = 384 (ViT-S features), 8192 rows, clustered data so that neighbours are meaningful (config 5 shape, scaled)."""
    rng = np.random.default_rng(11)
    centers = rng.standard_normal((64, 384))
    x = centers[rng.integers(0, 64, 8192)] + 0.7 * rng.standard_normal((8192, 384))
    x = K.normalize_rows(x).astype(np.float32)
    idx, sims = _run(x, 30)
    differing = K.check_neighbours(x, idx, 30, sims=sims)
    assert differing <= 8192 // 100                                  # only tie-band swaps may differ
    np.testing.assert_array_equal(idx[:, 0], np.arange(8192))


@gpu
def test_knn_cfg5_100k_rows_sampled_against_exact_topk():
    """BASELINE config 5 at its real size: N = 100 000 ViT-S/8 feature vectors (D = 384), k = 30 (precompute_knns.py:86-96).
    The fp64 oracle over all 10^10 pairs is out of reach, so 2 048 sampled query rows are checked exactly: the returned
    neighbours must carry the exact top-30 similarities (they may differ from torch.topk only inside a tie band, which
    SURVEY 8c allows), be sorted, duplicate-free, and rank 0 must be the row itself (data.py:524 skips it)."""
    n, d, k = 100000, 384, 30
    g = torch.Generator(device=DEV).manual_seed(1234)
    centers = torch.randn(256, d, generator=g, device=DEV)
    x = centers[torch.randint(0, 256, (n,), generator=g, device=DEV)] + 0.7 * torch.randn(n, d, generator=g, device=DEV)
    x = torch.nn.functional.normalize(x, dim=1).contiguous()
    from stego_amd import capi
    idx, sims = capi.knn_topk(x, k=k, return_sims=True)
    torch.cuda.synchronize()
    idx, sims = idx.cpu().numpy(), sims.cpu().numpy()
    xc = x.cpu().double()
    assert idx.shape == (n, k) and idx.min() >= 0 and idx.max() < n
    np.testing.assert_array_equal(idx[:, 0], np.arange(n))                       # self first, every row
    rows = np.random.default_rng(7).choice(n, 2048, replace=False)
    differing = 0
    for blk in np.array_split(rows, 8):
        s = xc[blk] @ xc.T                                                       # exact (fp64) similarities of the sampled rows
        ref_val, ref_idx = torch.topk(s, k, dim=1)
        got_val = torch.gather(s, 1, torch.from_numpy(idx[blk]))
        np.testing.assert_allclose(got_val.numpy(), ref_val.numpy(), rtol=0, atol=5e-6)      # tie band only
        assert (np.diff(got_val.numpy(), axis=1) <= 5e-6).all()
        np.testing.assert_allclose(sims[blk], got_val.numpy(), rtol=0, atol=2e-5)
        srt = np.sort(idx[blk], axis=1)
        assert (np.diff(srt, axis=1) > 0).all()
        differing += int((np.sort(ref_idx.numpy(), axis=1) != srt).any(axis=1).sum())
    assert differing <= 2048 // 50, differing


@gpu
def test_knn_rejects_bad_arguments():
    from stego_amd import capi
    x = torch.randn(64, 16, device=DEV)
    with pytest.raises(RuntimeError):
        capi.knn_topk(x, k=33)
    with pytest.raises(RuntimeError):
        capi.knn_topk(x, k=65)                                       # k > N
    with pytest.raises(RuntimeError):
        capi.knn_topk(x.cpu(), k=5)                                  # no CPU path


@pytest.mark.gpu
def test_precompute_pipeline_native_backbone_to_neighbour_table():
    """precompute_knns.py end to end on the device: DinoFeaturizer (native backbone) -> get_feats :15-21 ->
    compute_nearest_neighbors :86-96; against the same pipeline with the torch fp32 backbone."""
    import torch
    from stego_amd import featurizers, precompute_knns as P

    class C:
        dino_patch_size = 16; dino_feat_type = "feat"; model_type = "vit_tiny"; projection_type = None
        dropout = False; pretrained_weights = None; native_backbone = True
    torch.manual_seed(3)
    fz = featurizers.DinoFeaturizer(20, C()).cuda().eval()
    model = torch.nn.Sequential(fz, featurizers.LambdaLayer(lambda p: p[0]))
    g = torch.Generator().manual_seed(4)
    base = torch.randn(40, 3, 64, 64, generator=g)
    imgs = torch.cat([base, base[:8] + 0.01 * torch.randn(8, 3, 64, 64, generator=g)])     # 8 near-duplicates
    loader = [{"img": imgs[i:i + 16]} for i in range(0, 48, 16)]
    feats = P.get_feats(model, loader)
    assert fz.backbone_path == "native" and feats.shape == (48, 192)
    assert torch.allclose(feats.norm(dim=1), torch.ones(48, device=feats.device), atol=1e-5)
    nns = P.compute_nearest_neighbors(feats, k=5).cpu()
    assert torch.equal(nns[:, 0], torch.arange(48))                                       # rank 0 = the row itself
    assert torch.equal(nns[40:, 1], torch.arange(8))                                      # the near-duplicates find their originals
    C.native_backbone = False
    feats_ref = P.get_feats(model, loader)
    assert fz.backbone_path == "torch"
    assert float((feats - feats_ref).norm() / feats_ref.norm()) < 5e-3


# ------------------------------------------------------------------------------------------------ GPU: every tile-kernel variant vs fp64
def _clustered(n, d, seed, scale=1.0):
    """Clustered fp32 rows on the device (64 centres + noise, as test_knn_vits8_width_8k_rows_against_oracle): L2-normalised when
    scale is None, else raw rows times scale."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    centers = torch.randn(64, d, generator=g, device=DEV)
    x = centers[torch.randint(0, 64, (n,), generator=g, device=DEV)] + 0.7 * torch.randn(n, d, generator=g, device=DEV)
    return torch.nn.functional.normalize(x, dim=1).contiguous() if scale is None else (scale * x).contiguous()


def _knn_vs_fp64(x, idx, sims, k, q_begin=0, normalize=False, rows_per_block=2048):
    """The kernel's table against fp64 similarities computed on the device (row blocks of x64[q] @ x64^T), and torch fp32 (einsum +
    topk) on the same data as the yardstick.  Checks validity / order / duplicates and returns the measured errors:
      gap     max |s64[returned] - exact top-k s64|      (elementwise in rank order: only tie-band swaps may differ)
      unsort  max s64[rank r + 1] - s64[rank r]
      sim     max |returned sims - s64[returned]|
      e32     max |s32 - s64| of torch fp32 over the same rows (all columns): the fp32 class of this data
      gap32   the gap of torch fp32's own top-k"""
    N = x.shape[0]
    q = idx.shape[0]
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (q, k)
    assert int(idx.min()) >= 0 and int(idx.max()) < N, "index out of [0, N) (or -1: an unfilled list slot)"
    srt = torch.sort(idx, dim=1).values
    assert bool((srt[:, 1:] > srt[:, :-1]).all()), "duplicate neighbour in a row"
    x64 = x.double()
    x32 = x
    if normalize:                                                    # F.normalize, eps 1e-12 (precompute_knns.py:19)
        x64 = torch.nn.functional.normalize(x64, dim=1, eps=1e-12)
        x32 = torch.nn.functional.normalize(x, dim=1, eps=1e-12)
    m = dict(gap=0.0, unsort=0.0, sim=0.0, e32=0.0, gap32=0.0)
    for r0 in range(0, q, rows_per_block):
        r1 = min(q, r0 + rows_per_block)
        s = x64[q_begin + r0:q_begin + r1] @ x64.T
        ref_val = torch.topk(s, k, dim=1).values
        got = torch.gather(s, 1, idx[r0:r1])
        s32 = torch.einsum("nf,mf->nm", x32[q_begin + r0:q_begin + r1], x32)
        i32 = torch.topk(s32, k, dim=1).indices
        m["gap"] = max(m["gap"], float((got - ref_val).abs().max()))
        if k > 1:
            m["unsort"] = max(m["unsort"], float((got[:, 1:] - got[:, :-1]).max()))
        m["sim"] = max(m["sim"], float((sims[r0:r1].double() - got).abs().max()))
        m["e32"] = max(m["e32"], float((s32.double() - s).abs().max()))
        m["gap32"] = max(m["gap32"], float((torch.gather(s, 1, i32) - ref_val).abs().max()))
    return m


def _assert_fp32_class(m, what=""):
    """The kernel's table is in the fp32 class of torch on the same data: its similarities err by at most 2 x torch fp32's largest
    similarity error e32, so a returned neighbour can miss the exact top-k only inside a tie band of 2 x that, and its rank order can
    be inverted only inside that band as well."""
    band = 2.0 * (2.0 * m["e32"])
    assert m["sim"] <= 2.0 * m["e32"], ("returned sims vs fp64", what, m)
    assert m["gap"] <= max(band, m["gap32"]), ("top-k similarities vs fp64", what, m)
    assert m["unsort"] <= band, ("neighbours not sorted by descending similarity", what, m)


def _knn(x, k, **kw):
    from stego_amd import capi
    idx, sims = capi.knn_topk(x, k=k, return_sims=True, **kw)
    torch.cuda.synchronize()
    return idx, sims


_WIDE = [(n, d, (1, 30, 32)[(i + j) % 3]) for i, n in enumerate((50, 129, 8192, 20000)) for j, d in enumerate((385, 448, 768, 1000))]


# knn_tile_kernel<false> (both operands staged in LDS): launch_knn takes it when NCH = ceil(D / 64) > KNN_AREG_CHUNKS = 6, i.e. D > 384
@gpu
@pytest.mark.parametrize("n,d,k", _WIDE)
def test_knn_wide_features_against_fp64(n, d, k):
    """D in {385 (NCH = 7, the first width past the register path), 448 (whole chunks), 768 (ViT-B), 1000 (a partial last chunk)};
    N = 8192 / 20000 cut every query block into several segments (at uneven places for 20000), merged by knn_merge_kernel."""
    x = _clustered(n, d, seed=n + d, scale=None)
    idx, sims = _knn(x, k)
    m = _knn_vs_fp64(x, idx, sims, k)
    _assert_fp32_class(m, (n, d, k))
    assert torch.equal(idx[:, 0].cpu(), torch.arange(n)), "rank 0 is not the row itself"


# both tile-kernel variants: knn_tile_kernel<true> at D = 384 (NCH = 6 <= KNN_AREG_CHUNKS), knn_tile_kernel<false> at D = 768 (NCH = 12)
@gpu
@pytest.mark.parametrize("d", [384, 768])
def test_knn_normalize_with_zero_rows_against_fp64(d):
    """normalize=True (F.normalize inside, eps 1e-12) on raw rows of varying norm, 7 of them all zero: the eps branch makes them zero
    vectors whose similarity to everything is exactly 0."""
    n, k = 1500, 30
    x = _clustered(n, d, seed=d + 1, scale=3.0)
    x *= torch.linspace(0.01, 40.0, n, device=DEV)[torch.randperm(n, generator=torch.Generator().manual_seed(2)).to(DEV)].unsqueeze(1)
    zero = torch.tensor([0, 5, 127, 128, 700, 1401, n - 1], device=DEV)
    x[zero] = 0.0
    idx, sims = _knn(x, k, normalize=True)
    m = _knn_vs_fp64(x, idx, sims, k, normalize=True)
    _assert_fp32_class(m, d)
    live = torch.ones(n, dtype=torch.bool, device=DEV)
    live[zero] = False
    assert torch.equal(idx[live, 0], torch.arange(n, device=DEV)[live])
    assert bool((sims[zero] == 0).all()), "a zero row's similarities must be exactly 0"


# both tile-kernel variants (D = 384: knn_tile_kernel<true>, D = 768: knn_tile_kernel<false>) reading rows ldx = x.stride(0) > D apart
@gpu
@pytest.mark.parametrize("d", [384, 768])
def test_knn_strided_rows_and_query_slices_against_fp64(d):
    """A column slice of a wider tensor (ldx = D + 37, first column 5: capi.knn_topk passes stride(0)), and query slices
    (q_begin, q_count) that must equal the full table's rows bit for bit."""
    n, k = 1100, 30
    wide = _clustered(n, d + 37, seed=d + 2, scale=None)
    x = wide[:, 5:5 + d]
    assert x.stride(0) == d + 37 and x.stride(1) == 1
    idx, sims = _knn(x, k, normalize=True)
    m = _knn_vs_fp64(x.contiguous(), idx, sims, k, normalize=True)
    _assert_fp32_class(m, d)
    assert torch.equal(idx[:, 0].cpu(), torch.arange(n))
    ref_idx, ref_sims = _knn(torch.nn.functional.normalize(x.contiguous(), dim=1), k)
    for q0, qc in ((0, 128), (128, 300), (1024, 76), (256, 844)):
        part, ps = _knn(x, k, normalize=True, q_begin=q0, q_count=qc)
        assert torch.equal(part, idx[q0:q0 + qc]) and torch.equal(ps, sims[q0:q0 + qc]), (q0, qc)
    mr = _knn_vs_fp64(torch.nn.functional.normalize(x.contiguous(), dim=1), ref_idx, ref_sims, k)
    _assert_fp32_class(mr, (d, "dense"))


# both tile-kernel variants (D = 384 / 768) on exact ties: a block of identical rows
@gpu
@pytest.mark.parametrize("d", [384, 768])
def test_knn_duplicated_rows_against_fp64(d):
    """40 copies of one row (exact ties at similarity 1 across two 128-row blocks): every returned similarity exact to the tie band,
    indices valid and distinct, the first min(k, 40) neighbours of a copy are copies."""
    n, k = 1000, 32
    x = _clustered(n, d, seed=d + 3, scale=None)
    dup = torch.arange(110, 150, device=DEV)
    x[dup] = x[110].clone()
    idx, sims = _knn(x, k)
    m = _knn_vs_fp64(x, idx, sims, k)
    _assert_fp32_class(m, d)
    assert bool(torch.isin(idx[dup], dup).all()), "a copy's 32 best are not all copies"
    rest = torch.ones(n, dtype=torch.bool, device=DEV)
    rest[dup] = False
    assert torch.equal(idx[rest, 0], torch.arange(n, device=DEV)[rest])
