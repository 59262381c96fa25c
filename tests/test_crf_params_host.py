"""The dense CRF's yardstick without a GPU: the float64 mode of tests/crf_oracle.py (float32 stays bitwise the oracle from before the
mode existed), the bar of tests/crf_cases.py against a filter with one blur weight off by 1e-4, and the last descriptors the host-side
range check of csrc/dense_crf.hip accepts: at the smallest accepted pos_xy_std, bi_xy_std and bi_rgb_std every vertex key and every
blur-neighbour coordinate of the oracle's lattices is inside the packed field, and the float32 just below is refused.

Measured (37x53, C = 27, one iteration, default constants, noise image): the mutated filter errs by 1.97e-5 = 40 x e32 (e32 =
4.9e-7) against a bar of 2.95e-6, and stays under the 1e-4 of tests/test_crf_gpu.py.  At 12x16 the boundaries are bi_rgb_std =
0.785619 (bilateral keys -1426 .. 1109), bi_xy_std = 0.0426628 (keys -1092 .. 1930 on the test's image, neighbours -1223 .. 2030 over
every position under the eight extreme colours, of a field that ends at 2047) and pos_xy_std = 8.81699e-6 (Gaussian keys to
4194263, the limit being 2^22)."""
import ctypes

import numpy as np
import pytest

import crf_cases as K
import crf_oracle as O

F32 = np.float32


# ---- the float32 oracle as it stood before the dtype argument (Lattice.filter / norm, softmax, dense_crf), with the weight of the
# n1 blur neighbour as a parameter: w1 = 0.5 is the old code, operation for operation
def _old_filter(lat, x, w1=None):
    x = np.asarray(x, F32)
    d = lat.d
    flat_w = lat.bary.reshape(-1)[lat.order]
    pix = lat.order // (d + 1)
    v = np.add.reduceat(flat_w[:, None] * x[pix], lat.seg, axis=0).astype(F32)
    z = np.zeros((1, x.shape[1]), F32)
    for j in range(d + 1):
        p = np.concatenate([v, z], 0)
        n1, n2 = lat.nbr[j]
        v = v + F32(0.5) * (p[n1] + p[n2]) if w1 is None else v + (F32(w1) * p[n1] + F32(0.5) * p[n2])
    out = np.zeros_like(x)
    for r in range(d + 1):
        out += lat.bary[:, r, None] * v[lat.vid[:, r]]
    return out


def _old_norm(lat, w1=None):
    n = _old_filter(lat, np.ones((lat.N, 1), F32), w1)[:, 0]
    return (1.0 / np.sqrt(n.astype(np.float64) + 1e-20)).astype(F32)


def _old_softmax(x, axis):
    x = np.asarray(x, F32)
    e = np.exp(x - x.max(axis, keepdims=True))
    return e / e.sum(axis, keepdims=True)


def _old_dense_crf(bgr, probs, lattices, n_iter, pos_w, bi_w, w1=None):
    C, H, W = probs.shape
    neg_u = np.log(np.clip(np.asarray(probs, F32), F32(1e-5), F32(1.0))).reshape(C, -1).T.astype(F32)
    lg, lb = lattices
    sg, sb = _old_norm(lg, w1)[:, None], _old_norm(lb, w1)[:, None]
    q = _old_softmax(neg_u, 1)
    for _ in range(n_iter):
        kg = sg * _old_filter(lg, sg * q, w1)
        kb = sb * _old_filter(lb, sb * q, w1)
        q = _old_softmax((neg_u + F32(pos_w) * kg) + F32(bi_w) * kb, 1)
    return q.T.reshape(C, H, W)


@pytest.mark.parametrize("row,n_iter", [("default", 10), ("neg_w", 3), ("tight_rgb", 1), ("default", 0)])
def test_float32_mode_is_bitwise_the_old_oracle(row, n_iter):
    bgr, probs = K.inputs("noise", 23, 31, 5, seed=4)
    pos_w, pos_xy_std, bi_w, bi_xy_std, bi_rgb_std = K.ROWS[row]
    lat = K.lattices(bgr, pos_xy_std, bi_xy_std, bi_rgb_std)
    old = _old_dense_crf(bgr, probs, lat, n_iter, pos_w, bi_w)
    kw = dict(n_iter=n_iter, pos_w=pos_w, pos_xy_std=pos_xy_std, bi_w=bi_w, bi_xy_std=bi_xy_std, bi_rgb_std=bi_rgb_std)
    for new in (O.dense_crf(bgr, probs, lattices=lat, **kw), O.dense_crf(bgr, probs, dtype=np.float32, **kw)):
        assert new.dtype == F32 and np.array_equal(new, old)
    x = np.random.default_rng(0).uniform(0, 1, (23 * 31, 7)).astype(F32)
    for l in lat:
        assert np.array_equal(l.filter(x), _old_filter(l, x)) and l.filter(x).dtype == F32
        assert np.array_equal(l.norm(), _old_norm(l)) and l.norm().dtype == F32
    assert np.array_equal(O.softmax(x, 1), _old_softmax(x, 1))


def test_float64_mode_zero_weights_and_normalisation():
    rng = np.random.default_rng(2)
    bgr = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    p = rng.dirichlet(np.ones(5), size=99).T.reshape(5, 9, 11).astype(F32)
    u = np.log(np.clip(p, F32(1e-5), F32(1.0)).astype(np.float64))
    e = np.exp(u - u.max(0, keepdims=True))
    expect = e / e.sum(0, keepdims=True)
    for it in (0, 1, 4):
        q = O.dense_crf(bgr, p, n_iter=it, pos_w=0.0, bi_w=0.0, dtype=np.float64)
        assert q.dtype == np.float64
        np.testing.assert_allclose(q, expect, rtol=0, atol=1e-15)
    q = O.dense_crf(bgr, p, dtype=np.float64)
    assert q.dtype == np.float64 and np.abs(q.sum(0) - 1.0).max() <= 1e-12
    assert np.abs(q - expect).max() > 1e-3                    # the pairwise terms did something
    # float64 runs after the embedding only: the lattice it filters on holds the float32 weights
    lat = K.lattices(bgr, O.POS_XY_STD, O.Bi_XY_STD, O.Bi_RGB_STD)
    assert all(l.bary.dtype == F32 for l in lat)
    x = rng.uniform(0, 1, (99, 3))
    for l in lat:
        y = l.filter(x, np.float64)
        assert y.dtype == np.float64 and l.norm(np.float64).dtype == np.float64
        assert 0 < np.abs(y - l.filter(x.astype(F32))).max() < 1e-5 * np.abs(y).max()


def test_bar_catches_a_blur_weight_off_by_1e_4():
    """One neighbour weight of the blur at 0.5 (1 + 1e-4), in every filter pass of both lattices (those of s included, which takes
    part of the error back out): measured 1.97e-5 from q64 = 40 x e32 (4.9e-7; the bar is 2.95e-6), an error the 1e-4 of
    tests/test_crf_gpu.py lets through with 5x to spare.  (Mutating the iteration's passes alone: 3.4e-5.)"""
    bgr, probs = K.table_inputs(37, 53, 27)
    ref = K.table_ref("default", 37, 53, 27, 1, 0)
    good = _old_dense_crf(bgr[0], probs[0], ref.lat, 1, O.POS_W, O.Bi_W)
    assert np.array_equal(good, ref.q32)
    bad = _old_dense_crf(bgr[0], probs[0], ref.lat, 1, O.POS_W, O.Bi_W, w1=0.5 * (1 + 1e-4))
    err = float(np.abs(bad - ref.q64).max())
    print("[crf mutation] err %.3e  e32 %.3e  err/e32 %.1f  bar %.3e" % (err, ref.e32, err / ref.e32, ref.bar))
    assert err > ref.bar and err > 10 * ref.e32
    with pytest.raises(AssertionError):
        ref.check(bad, "mutated")
    assert err <= 1e-4 and np.abs(bad - ref.q32).max() <= 1e-4          # ATOL_SMALL of tests/test_crf_gpu.py
    ref.check(good, "unmutated")                                          # and the float32 oracle itself passes: ratio 1


def _field(lat):
    bits = O.key_bits(lat.d)
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


@pytest.mark.parametrize("field", K.STD_FIELDS)
@pytest.mark.parametrize("H,W", [(12, 16), (37, 53)])
def test_last_accepted_std_keeps_keys_and_neighbours_in_the_packed_field(H, W, field):
    from stego_amd import capi
    lib = capi.load()
    value, below = K.smallest_accepted(H, W, field)
    assert 0 < below < value and np.nextafter(F32(value), F32(0)) == F32(below)
    assert capi.crf_workspace_bytes(K.range_desc(H, W, field, value)) > 0
    d = K.range_desc(H, W, field, below)
    assert capi.crf_workspace_bytes(d) == 0
    assert lib.stego_crf_run(ctypes.byref(d), None, None, None, None, 0, None) == capi.CRF_ERR_RANGE      # host check: nothing is used
    bgr, _ = K.inputs("corner", H, W, 3, seed=1)
    assert [tuple(bgr[y, x]) for y, x in ((0, 0), (0, -1), (-1, 0), (-1, -1))] == [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255)]
    assert set(np.unique(bgr)) == {0, 255}
    p = K.range_params(H, W, field)
    lats = K.lattices(bgr, p[1], p[3], p[4])             # pack() asserts every vertex key of all d + 1 remainders
    for lat in lats:
        lo, hi = _field(lat)
        c = O.unpack(lat.keys, lat.d)
        assert lo <= c.min() and c.max() <= hi
        for j, (n1, n2) in enumerate(lat.neighbour_coords()):
            for n in (n1, n2):
                assert lo <= n.min() and n.max() <= hi, (field, lat.d, j, int(n.min()), int(n.max()))
    # a pixel's keys depend on its own position and colour only, and the elevated coordinates are linear in them: every position
    # under each of the eight extreme colours covers the extremes no one random image needs to hit
    if field != "pos_xy_std":
        seen = [0, 0]
        for colour in np.ndindex(2, 2, 2):
            flat = np.broadcast_to(np.array(colour, np.uint8) * 255, (H, W, 3))
            lat = O.Lattice(O.bilateral_features(flat, p[3], p[4]))
            lo, hi = _field(lat)
            for n1, n2 in lat.neighbour_coords():
                seen = [min(seen[0], int(n1.min()), int(n2.min())), max(seen[1], int(n1.max()), int(n2.max()))]
        print("[crf range %dx%d %s=%.6g] neighbour coordinates over the extreme colours %d .. %d" % (H, W, field, value, *seen))
        assert lo <= seen[0] and seen[1] <= hi, seen
    # the boundary is where a restatement of the bound outside the library puts it
    if (H, W) == (12, 16):
        expect = {"bi_rgb_std": 0.7856, "bi_xy_std": 0.04266}.get(field)
        assert expect is None or abs(value - expect) <= 2e-4 * expect, value
        if field == "bi_rgb_std":
            c = O.unpack(lats[1].keys, 5)
            assert (c.min(), c.max()) == (-1426, 1109)


def _reversed(ref, bgr, probs, n_iter, params):
    """The float32 oracle with every vertex's records summed last pixel first."""
    for lat in ref.lat:
        lat.reverse = True
    try:
        return O.dense_crf(bgr, probs, n_iter=n_iter, pos_w=params[0], pos_xy_std=params[1], bi_w=params[2], bi_xy_std=params[3],
                           bi_rgb_std=params[4], lattices=ref.lat)
    finally:
        for lat in ref.lat:
            lat.reverse = False


def test_reverse_summation_order_asks_for_no_wider_factor():
    """The one procedure that may move the factor 4: the float32 oracle with reversed splat sums against q64, twice the largest ratio
    to e32.  Over the 64 cases of the parameter table the largest ratio is 1.62 (wide_pos, 23x31, C = 5, noise, ten iterations: this
    case), then 1.19, 1.10 and 1.07, and the other 60 are at most 1.00: twice the largest is 3.24, so the factor stays 4.  (The procedure moves little: on these images
    most vertices hold one or two records, whose sum has one order.)"""
    bgr, probs = K.table_inputs(23, 31, 5)
    ref = K.table_ref("wide_pos", 23, 31, 5, 10, 0)
    qr = _reversed(ref, bgr[0], probs[0], 10, K.ROWS["wide_pos"])
    assert not np.array_equal(qr, ref.q32)                                # another order, another rounding
    assert np.array_equal(O.dense_crf(bgr[0], probs[0], n_iter=10, pos_xy_std=2.5, lattices=ref.lat), ref.q32)    # and the flag is off again
    ratio = float(np.abs(qr - ref.q64).max()) / ref.e32
    print("[crf reverse order] err / e32 %.2f" % ratio)
    assert 1.0 < ratio and 2 * ratio <= K.FACTOR
    ref.check(qr, "reverse order")


@pytest.mark.parametrize("n_iter", [1, 10])
@pytest.mark.parametrize("row", list(K.ROWS))
def test_table_seed_leaves_no_argmax_exception_to_the_reference(row, n_iter):
    """q32 against q64 excepts no pixel from the argmax rule (here at 23x31; 0 of 117 image checks over every case of
    tests/test_crf_params_gpu.py when the float32 oracle stands in for the kernels)."""
    for b in range(2):
        ref = K.table_ref(row, 23, 31, 5, n_iter, b)
        assert ref.excepted(ref.q32) == 0.0
        assert np.array_equal(ref.q32.argmax(0), ref.q64.argmax(0))
