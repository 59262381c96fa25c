"""The step-statistics kernel on the GPU (include/stego_stats.h, stego_amd.step_stats.StepStats) against numpy on the CPU over the same
float32 values: counts, n_*, min, max, the step number and the scalars for EQUALITY; sum and sum_sq against math.fsum of the values and
of their exact fp64 squares within n * 2^-53 * sum|x| and n * 2^-53 * sum x^2, the first-order bound of any fp64 summation order."""
import math
import warnings

import numpy as np
import pytest
import torch

from stego_amd import capi
from stego_amd.step_stats import StepStats, default_bins

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def edges():
    limits, thr = capi.step_stats_edges()
    limits.setflags(write=False)
    thr.setflags(write=False)
    return limits, thr


def _reference(x, limits):
    """numpy's answer for float32 values x."""
    x = np.asarray(x, np.float32)
    finite = np.isfinite(x)
    xf = x[finite].astype(np.float64)
    counts = np.histogram(x[finite], bins=limits)[0]
    n_nan = int(np.isnan(x).sum())
    return dict(n_finite=int(finite.sum()), n_nan=n_nan, n_out=int(x.size - n_nan - counts.sum()), counts=counts,
                min=np.float32(x[finite].min()) if xf.size else np.float32(np.inf),
                max=np.float32(x[finite].max()) if xf.size else np.float32(-np.inf),
                sum=math.fsum(xf), sum_sq=math.fsum(xf * xf), abs_sum=math.fsum(np.abs(xf)))


def _compare(got, x, limits, with_hist=True):
    ref = _reference(x, limits)
    for k in ("n_finite", "n_nan", "n_out"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert got["min"] == ref["min"] and got["max"] == ref["max"], (got["min"], ref["min"], got["max"], ref["max"])
    n = ref["n_finite"]
    err, err2 = abs(got["sum"] - ref["sum"]), abs(got["sum_sq"] - ref["sum_sq"])
    print("n %d  sum err %.3e (bound %.3e)  sum_sq err %.3e (bound %.3e)" % (n, err, n * 2.0 ** -53 * ref["abs_sum"], err2, n * 2.0 ** -53 * ref["sum_sq"]))
    assert err <= n * 2.0 ** -53 * ref["abs_sum"], (got["sum"], ref["sum"])
    assert err2 <= n * 2.0 ** -53 * ref["sum_sq"], (got["sum_sq"], ref["sum_sq"])
    if with_hist:
        assert got["counts"].dtype == np.uint32 and got["counts"].shape == (capi.STATS_BUCKETS,)
        bad = np.nonzero(got["counts"].astype(np.int64) != ref["counts"])[0]
        assert bad.size == 0, (bad[:8], got["counts"][bad[:8]], ref["counts"][bad[:8]])
    else:
        assert got["counts"] is None


def _run(arrays, with_hist=True, offsets=None):
    """One record of the float32 arrays (each uploaded to a 16-byte aligned buffer at element offset offsets[i])."""
    tensors = []
    for i, a in enumerate(arrays):
        off = 0 if offsets is None else offsets[i]
        buf = torch.zeros(len(a) + 8, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + len(a)]
        view.copy_(torch.from_numpy(np.asarray(a, np.float32)))
        tensors.append(view)
    ss = StepStats(0, 2, DEV)
    ss.record(tensors, (), with_hist)
    recs = ss.drain()
    assert len(recs) == 1 and recs[0]["step"] == 0 and recs[0]["with_hist"] == bool(with_hist)
    return recs[0]["tensors"]


def _normal(n, seed, scale=0.3):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _max_grid():
    rc, plan = capi.step_stats_plan(capi.stats_desc([capi.STATS_MAX_ELEMS - 1], 0, 0, 1))
    assert rc == 0
    return plan["grid"], plan["chunk"]


@pytest.mark.parametrize("with_hist", [1, 0])
def test_small_counts_and_chunk_edges(edges, with_hist):
    grid, chunk = _max_grid()
    for group in ([1, 63, 64, 65], [chunk - 1, chunk, chunk + 1]):
        arrays = [_normal(n, 10 + n) for n in group]
        got = _run(arrays, with_hist)
        for g, a in zip(got, arrays):
            _compare(g, a, edges[0], with_hist)


def test_second_round_of_a_workgroup(edges):
    grid, chunk = _max_grid()
    n = grid * chunk + 5                      # workgroup 0 takes chunk 0 and chunk `grid`
    rc, plan = capi.step_stats_plan(capi.stats_desc([n], 0, 1, 1))
    assert rc == 0 and plan["grid"] == grid and (n + chunk - 1) // chunk == grid + 1
    a = _normal(n, 3)
    _compare(_run([a])[0], a, edges[0])


def test_empty_tensor_between_two(edges):
    arrays = [_normal(300, 1), np.zeros(0, np.float32), _normal(5000, 2)]
    got = _run(arrays)
    for g, a in zip(got, arrays):
        _compare(g, a, edges[0])
    assert got[1]["n_finite"] == 0 and got[1]["min"] == np.inf and got[1]["max"] == -np.inf and got[1]["sum"] == 0.0
    assert math.isnan(got[1]["mean"]) and not got[1]["counts"].any()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_base_every_residue(edges, offset):
    for base in (4096, 8):
        arrays = [_normal(base + r, 40 + 4 * offset + r) for r in range(4)]
        got = _run(arrays, offsets=[offset] * 4)
        for g, a in zip(got, arrays):
            _compare(g, a, edges[0])
    # ... and the 16-byte path with every residue
    arrays = [_normal(4096 + r, 60 + r) for r in range(4)]
    for g, a in zip(_run(arrays, offsets=[0, 4, 0, 4]), arrays):
        _compare(g, a, edges[0])


def test_every_threshold_and_its_predecessor(edges):
    limits, thr = edges
    x = np.concatenate([thr, np.nextafter(thr, np.float32(-np.inf))]).astype(np.float32)
    assert x.size == 3098
    got = _run([x])[0]
    _compare(got, x, limits)
    # each bucket holds its own lower threshold and the predecessor of its upper one; the predecessor of the first threshold is out
    assert (got["counts"] == 2).all() and got["n_out"] == 2


def test_zeros_and_denormals(edges):
    tiny = np.float32(1.401298464324817e-45)
    x = np.array([0.0, -0.0, tiny, -tiny, 1e-38, -1e-38], np.float32)
    assert np.signbit(x[1]) and x[2] > 0 and x[3] < 0
    got = _run([x])[0]
    _compare(got, x, edges[0])
    # bucket 774 = [0, 1e-12): +0, -0, the positive denormal, 1e-38; bucket 773 = [-1e-12, 0): the negative denormal, -1e-38
    assert got["counts"][774] == 4 and got["counts"][773] == 2
    one = _run([x[:4]])[0]
    assert one["counts"][774] == 3 and one["counts"][773] == 1 and one["counts"].sum() == 4


def test_range_ends_infinities_and_nan(edges):
    x = _normal(3000, 5)
    special = np.array([1, -1, 9.9e19, -9.9e19, 1.1e20, -1.1e20, np.inf, -np.inf, np.nan, np.nan], np.float32)
    x[np.arange(10) * 293 + 7] = special
    got = _run([x])[0]
    _compare(got, x, edges[0])
    assert got["n_nan"] == 2 and got["n_out"] >= 4 and got["n_finite"] == 2996 and got["max"] == np.float32(1.1e20)


def test_one_bucket_holds_everything(edges):
    x = np.full(200000, 0.25, np.float32)
    got = _run([x])[0]
    _compare(got, x, edges[0])
    assert got["counts"].max() == 200000 and got["sum"] == 50000.0 and got["mean"] == 0.25


def test_spread_over_hundreds_of_buckets(edges):
    x = _normal(200000, 6)
    got = _run([x])[0]
    _compare(got, x, edges[0])
    # |x| between 3e-4 and 0.9 is certainly drawn on either side of zero: log(3000) / log(1.1) = 84 buckets per sign
    assert (got["counts"] > 0).sum() >= 160


def test_contended_buckets(edges):
    x = np.random.default_rng(7).uniform(0.2, 0.3, 2000000).astype(np.float32)
    _compare(_run([x])[0], x, edges[0])


def test_ring_wraps_and_drain(edges):
    ss = StepStats(1, 4, DEV)
    inputs = [_normal(500 + 37 * i, 20 + i, scale=0.1 * (i + 1)) for i in range(6)]
    scalars = torch.arange(6, dtype=torch.float32, device=DEV) + 0.5
    for i, a in enumerate(inputs):
        ss.record([torch.from_numpy(a).to(DEV)], [scalars[i:i + 1]], with_hist=i % 2)
    assert ss.steps_recorded() == 6
    p = ss.plan
    host = ss.ring.cpu().numpy().reshape(4, p["record_bytes"])
    assert [int(host[s, p["off_step"]:p["off_step"] + 8].view(np.int64)[0]) for s in range(4)] == [4, 5, 2, 3]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        recs = ss.drain()
        assert ss.drain() == []
    said = [str(x.message) for x in w if "overwritten" in str(x.message)]
    assert len(said) == 1 and "2 records" in said[0]
    assert [r["step"] for r in recs] == [2, 3, 4, 5]
    for r in recs:
        i = r["step"]
        assert r["with_hist"] == bool(i % 2) and r["scalars"][0] == np.float32(i + 0.5)
        _compare(r["tensors"][0], inputs[i], edges[0], with_hist=i % 2)       # slots 1 and 3 held the counts of steps 1 and 3 before


def test_scalars_arrive_bit_for_bit():
    rng = np.random.default_rng(8)
    vals = rng.standard_normal(16).astype(np.float32)
    vals[3], vals[9] = np.nan, -0.0
    vals[12] = np.float32(1e-42)
    pool = torch.from_numpy(vals[:10].copy()).to(DEV)
    ptrs = [pool[i:i + 1] for i in range(10)] + [torch.from_numpy(vals[i:i + 1].copy()).to(DEV).reshape(()) for i in range(10, 16)]
    ss = StepStats(16, 2, DEV)
    ss.record([torch.ones(3, device=DEV)], ptrs, False)
    rec = ss.drain()[0]
    assert (rec["scalars"].view(np.uint32) == vals.view(np.uint32)).all()


def test_two_runs_give_identical_rings():
    arrays = [_normal(468512 // 4, 30), _normal(70001, 31), _normal(300000, 32)]
    tensors = [torch.from_numpy(a).to(DEV) for a in arrays]
    s = torch.tensor([1.5, -2.5], device=DEV)
    rings = []
    for _ in range(2):
        ss = StepStats(2, 3, DEV)
        for i in range(4):
            ss.record(tensors, [s[0:1], s[1:2]], with_hist=i != 2)
        rings.append(ss.ring.cpu())
    assert torch.equal(rings[0], rings[1])


def test_graph_capture_and_replay(edges):
    a, b = _normal(20000, 33), _normal(777, 34)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    s = torch.tensor([3.25], device=DEV)
    ss = StepStats(1, 8, DEV)
    ss.record([ta, tb], [s], True)                       # eager: step 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ss.record([ta, tb], [s], True)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    recs = ss.drain()
    assert [r["step"] for r in recs] == [0, 1, 2, 3]
    for r in recs:
        _compare(r["tensors"][0], a, edges[0])
        _compare(r["tensors"][1], b, edges[0])
        assert r["scalars"][0] == np.float32(3.25)
        for t0, t in zip(recs[0]["tensors"], r["tensors"]):
            assert all(np.array_equal(t0[k], t[k]) for k in t0), r["step"]


def test_cpu_tensors_are_refused():
    ss = StepStats(0, 2, DEV)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ss.record([torch.ones(4)], (), False)
    with pytest.raises(RuntimeError, match="MI355X only"):
        StepStats(0, 2, "cpu")


def test_default_bins_are_tensorboards():
    v, pos = 1e-12, []
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    assert np.array_equal(default_bins(), np.array([-x for x in pos[::-1]] + [0] + pos))
