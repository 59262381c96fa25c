"""The step statistics without a GPU: every host check of stego_step_stats (include/stego_stats.h) returns its documented code before
anything is enqueued (made-up pointers, no device), the edges equal TensorBoard's loop bit for bit, the thresholds are the smallest
float32 not below each limit, and the plan's record layout is aligned and free of overlaps."""
import os
import re

import numpy as np
import pytest

from stego_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stego_stats.h")).read()
NULL, ALIGN = 1, 5   # STEGO_ERR_NULL, STEGO_ERR_ALIGN
A = 0x7f0000001000                    # a made-up, well aligned device address: no check may touch it


def _rc(counts=(100, 0, 7), n_scalars=2, with_hist=1, ring_slots=4, n_tensors=None, tensors="default", scalars="default", ring=A,
        state=A + 0x100000, ws=A + 0x200000, desc="default"):
    if desc == "default":
        desc = capi.stats_desc(counts, n_scalars, with_hist, ring_slots, n_tensors=n_tensors)
    if tensors == "default":
        tensors = [A + 0x300000 + 4 * i for i in range(len(counts))]
    if scalars == "default":
        scalars = [A + 0x400000 + 4 * i for i in range(max(n_scalars, 0))]
    return capi.step_stats_raw(desc, tensors, scalars, ring, state, ws)


def test_good_arguments_reach_the_launch():
    # everything the host can check is fine: what comes back is the runtime's answer (no device here, or a launch), never a host code
    rc, plan = capi.step_stats_plan(capi.stats_desc((100, 0, 7), 2, 1, 4))
    assert rc == 0 and plan["grid"] == 1


@pytest.mark.parametrize("kw, code", [
    (dict(desc=None), NULL), (dict(tensors=None), NULL), (dict(ring=None), NULL),
    (dict(state=None), NULL), (dict(ws=None), NULL), (dict(scalars=None), NULL),
    (dict(n_tensors=0), capi.STATS_ERR_COUNT), (dict(n_tensors=5), capi.STATS_ERR_COUNT), (dict(n_tensors=-1), capi.STATS_ERR_COUNT),
    (dict(n_scalars=17), capi.STATS_ERR_COUNT), (dict(n_scalars=-1, scalars=[A]), capi.STATS_ERR_COUNT),
    (dict(counts=(100, -1, 7)), capi.STATS_ERR_COUNT), (dict(counts=(100, 1 << 31, 7)), capi.STATS_ERR_COUNT),
    (dict(ring_slots=0), capi.STATS_ERR_RING), (dict(ring_slots=-3), capi.STATS_ERR_RING), (dict(ring_slots=65537), capi.STATS_ERR_RING),
    (dict(with_hist=2), capi.STATS_ERR_FLAGS), (dict(with_hist=-1), capi.STATS_ERR_FLAGS),
    (dict(tensors=[A, None, None]), NULL),                      # a NULL tensor with count 7 (the one with count 0 may be NULL)
    (dict(scalars=[A, None]), NULL),
    (dict(ring=A + 4), ALIGN), (dict(state=A + 0x100004), ALIGN), (dict(ws=A + 0x200004), ALIGN),
    (dict(tensors=[A + 2, A, A]), ALIGN), (dict(tensors=[A, A, A + 1]), ALIGN), (dict(scalars=[A, A + 3]), ALIGN),
])
def test_error_codes(kw, code):
    assert _rc(**kw) == code


def test_codes_come_in_the_documented_order():
    # each call has every later defect too: the earlier one is reported
    bad_t, bad_s = [A + 2, None, None], [A + 1, None]
    assert _rc(n_tensors=5, ring_slots=0, with_hist=2, tensors=bad_t, scalars=bad_s, ring=A + 4) == capi.STATS_ERR_COUNT
    assert _rc(ring_slots=0, with_hist=2, tensors=bad_t, scalars=bad_s, ring=A + 4) == capi.STATS_ERR_RING
    assert _rc(with_hist=2, tensors=bad_t, scalars=bad_s, ring=A + 4) == capi.STATS_ERR_FLAGS
    assert _rc(tensors=bad_t, scalars=bad_s, ring=A + 4) == NULL
    assert _rc(tensors=[A + 2, None, A], scalars=[A + 1, A], ring=A + 4) == ALIGN
    assert _rc(n_tensors=5, ring=None) == NULL
    order = re.search(r"Returns STEGO_ERR_NULL \(desc.*?in this order", HEADER, re.S).group(0)
    names = re.findall(r"STEGO_ERR_[A-Z_]+", order)
    assert names == ["STEGO_ERR_NULL", "STEGO_ERR_STATS_COUNT", "STEGO_ERR_STATS_RING", "STEGO_ERR_STATS_FLAGS", "STEGO_ERR_NULL",
                     "STEGO_ERR_ALIGN"]


def test_null_tensor_with_count_zero_is_allowed_by_the_checks():
    rc, _ = capi.step_stats_plan(capi.stats_desc((0,), 0, 0, 1))
    assert rc == 0
    assert _rc(counts=(5, 0), n_scalars=0, tensors=[A, None], scalars=None, ring=A + 4) == ALIGN     # ... past the NULL checks


def test_plan_checks_the_descriptor():
    assert capi.step_stats_plan(None)[0] == NULL
    assert capi.step_stats_plan(capi.stats_desc((1,), 0, 0, 1, n_tensors=9))[0] == capi.STATS_ERR_COUNT
    assert capi.step_stats_plan(capi.stats_desc((1,), 0, 0, 0))[0] == capi.STATS_ERR_RING
    assert capi.step_stats_plan(capi.stats_desc((1,), 0, 3, 1))[0] == capi.STATS_ERR_FLAGS
    assert int(capi.load().stego_step_stats_plan(capi.byref(capi.stats_desc((1,), 0, 0, 1)), None)) == NULL


def _tensorboard_limits():
    v, pos = 1e-12, []
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.array([-x for x in pos[::-1]] + [0] + pos, np.float64)


def test_edges_equal_tensorboards_loop_bit_for_bit():
    limits, _ = capi.step_stats_edges()
    ref = _tensorboard_limits()
    assert limits.shape == ref.shape == (capi.STATS_LIMITS,) and capi.STATS_BUCKETS == capi.STATS_LIMITS - 1
    assert (limits.view(np.uint64) == ref.view(np.uint64)).all()


def test_thresholds_are_the_smallest_float32_not_below_each_limit():
    limits, thr = capi.step_stats_edges()
    assert thr.dtype == np.float32 and (thr.astype(np.float64) >= limits).all()
    below = np.nextafter(thr, np.float32(-np.inf))
    assert (below.astype(np.float64) < limits).all()
    assert (np.diff(thr) > 0).all() and thr[774] == 0 and not np.signbit(thr[774])
    assert thr[-1].astype(np.float64) != limits[-1]       # no float32 equals the last limit: numpy's closed last bucket changes nothing
    # the threshold rule reproduces np.histogram on float32 data, the edge values included
    x = np.concatenate([thr, below, (0.3 * np.random.default_rng(0).standard_normal(20000)).astype(np.float32),
                        np.array([0.0, -0.0, 1e-45, -1e-45], np.float32)])
    idx = np.searchsorted(thr, x, "right") - 1
    inside = (idx >= 0) & (idx < capi.STATS_BUCKETS)
    assert (np.bincount(idx[inside], minlength=capi.STATS_BUCKETS) == np.histogram(x, bins=limits)[0]).all()


@pytest.mark.parametrize("n_tensors, n_scalars", [(1, 0), (3, 9), (4, 16), (2, 1)])
def test_record_layout_is_aligned_and_free_of_overlaps(n_tensors, n_scalars):
    rc, p = capi.step_stats_plan(capi.stats_desc([10] * n_tensors, n_scalars, 1, 5))
    assert rc == 0
    spans = [(p["off_step"], 8, 8), (p["off_with_hist"], 4, 4), (p["off_n_tensors"], 4, 4), (p["off_scalars"], 4 * n_scalars, 4)]
    for i in range(n_tensors):
        base = p["off_tensors"] + i * p["tensor_stride"]
        spans += [(base + p[k], 8, 8) for k in ("t_n_finite", "t_n_nan", "t_n_out", "t_sum", "t_sum_sq")]
        spans += [(base + p[k], 4, 4) for k in ("t_min", "t_max")]
        spans.append((p["off_hist"] + i * p["hist_stride"], 4 * capi.STATS_BUCKETS, 4))
    for off, size, align in spans:
        assert off >= 0 and off % align == 0 and off + size <= p["record_bytes"], (off, size, align)
    spans = sorted(s for s in spans if s[1])
    for (a, n, _), (b, _, _) in zip(spans, spans[1:]):
        assert a + n <= b, (a, n, b)
    assert p["record_bytes"] % 16 == 0 and p["ring_bytes"] == 5 * p["record_bytes"]
    assert p["state_bytes"] == 16 and p["workspace_bytes"] % 16 == 0 and p["workspace_bytes"] > 4 * 4 * capi.STATS_BUCKETS
    assert p["chunk"] == 4096 and p["grid"] == 1


def test_plan_grid_follows_the_largest_tensor():
    chunk = capi.step_stats_plan(capi.stats_desc([1], 0, 0, 1))[1]["chunk"]
    for counts, grid in (([0], 1), ([chunk], 1), ([chunk + 1, 5], 2), ([5, 0, 10 * chunk], 10), ([(1 << 31) - 1], 1024)):
        assert capi.step_stats_plan(capi.stats_desc(counts, 0, 1, 1))[1]["grid"] == grid


def test_symbols_are_exported_and_declared():
    lib = capi.load()
    for name in ("stego_step_stats", "stego_step_stats_plan", "stego_step_stats_edges"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, HEADER), name
    for rc in (capi.STATS_ERR_COUNT, capi.STATS_ERR_RING, capi.STATS_ERR_FLAGS):
        assert lib.stego_error_string(rc).decode().startswith("step stats:")
        assert re.search(r"= %d\b" % rc, HEADER)
