"""csrc/dense_crf.hip on the MI355X against the float64 mode of tests/crf_oracle.py, under the bar of tests/crf_cases.py (kernel error
<= 4 x the float32 oracle's own error + 1e-6, argmax equal but for near-ties of the float64 result): every descriptor field away from
the reference's constants, iteration parity, the last descriptors the range check accepts, images of a batch independent of their
neighbours, batches past the launch grid's cap, probability maps that are no clean softmax, the group-width boundaries of C and
shapes that meet the scan block.  Keys and vertex counts of both lattices are the oracle's, bit for bit.

Largest err / e32 per group, measured on the MI355X (err = max|Q - q64|, e32 = max|q32 - q64| of the same case):
    parameter table, 1 iteration     0.86   (tight_xy, 23x31, blocks)
    parameter table, 10 iterations   3.64   (neg_w, 37x53, C = 27, noise: 2.40e-5 of a bar of 2.74e-5; then 2.80)
    range edges                      1.49   (pos_xy_std at its edge, a flat extreme colour; 1.25 on the corner-colour image)
    probability edges                1.07   (C = 17)
    geometry edges                   1.14   (16x32)
and, beyond the groups the bar was set for: grid cap 1.15, iteration parity 1.23.

With the softmax's expf, float sum and float division and the unary's logf these tests found one case over the bar, 10.30 at ten
iterations (test_parameter_table has the figures); the kernels now evaluate both in double and round once."""
import numpy as np
import pytest
import torch

import crf_cases as K
import crf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DEFAULT = K.ROWS["default"]


def _run(bgr, probs, n_iter, params, keep=False):
    """bgr uint8 [B, H, W, 3], probs float32 [B, C, H, W] -> Q as a device tensor (and the workspace and descriptor with keep)."""
    from stego_amd import capi
    B, C, H, W = probs.shape
    desc = capi.crf_desc(B, C, H, W, n_iter, *params)
    assert capi.crf_workspace_bytes(desc) > 0                 # accepted by the host check: nothing here is meant to be refused
    out = capi.crf_run(desc, torch.from_numpy(bgr).to(DEV), torch.from_numpy(np.ascontiguousarray(probs)).to(DEV), keep_workspace=keep)
    torch.cuda.synchronize()
    return (out[0], out[1], desc) if keep else out


def _check_keys(desc, ws, b, lats):
    from stego_amd import capi
    for which, lat in enumerate(lats):
        M, keys = capi.crf_lattice_info(desc, ws, b, which, max_keys=lat.M + 1)
        assert M == lat.M, (b, which, M, lat.M)
        np.testing.assert_array_equal(keys, lat.keys)


def _batch(pairs):
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _check_batch(bgr, probs, n_iter, params, what, keys=True):
    """Every image of one call against its own float64 / float32 oracle pair."""
    q, ws, desc = _run(bgr, probs, n_iter, params, keep=True)
    q = q.cpu().numpy()
    for b in range(len(bgr)):
        ref = K.Ref(bgr[b], probs[b], n_iter, params)
        ref.check(q[b], "%s image %d" % (what, b))
        if keys:
            _check_keys(desc, ws, b, ref.lat)


@pytest.mark.parametrize("n_iter", [1, 10])
@pytest.mark.parametrize("H,W,C", K.TABLE_SHAPES)
@pytest.mark.parametrize("row", list(K.ROWS))
def test_parameter_table(row, H, W, C, n_iter):
    """The case that moved the kernels' softmax to double: default constants, 23x31, C = 5, the noise image, ten iterations.  With
    expf, a float sum and a float division the kernels were 1.888e-5 from q64 against e32 1.833e-6 (bar 8.33e-6, ratio 10.3): 2.1e-7
    after the first iteration (0.91 x e32), then doubling per iteration - this image's mean-field has a mode that grows about 2.1 x
    per iteration, so each iteration's own rounding is what the result carries a hundredfold.  With the softmax (and the unary's
    log) in double, rounded once: 2.76e-6, ratio 1.50; every one-iteration case is at or below 0.86."""
    bgr, probs = K.table_inputs(H, W, C)                    # noise and gradient-plus-blocks, one call
    q, ws, desc = _run(bgr, probs, n_iter, K.ROWS[row], keep=True)
    q = q.cpu().numpy()
    for b, kind in enumerate(("noise", "blocks")):
        ref = K.table_ref(row, H, W, C, n_iter, b)
        ref.check(q[b], "table n_iter=%d %s %dx%d C=%d %s" % (n_iter, row, H, W, C, kind))
        _check_keys(desc, ws, b, ref.lat)


@pytest.mark.parametrize("n_iter", [2, 3])
def test_iteration_parity(n_iter):
    """The state s * Q is rewritten in place and the blur's two buffers alternate: an even and an odd count on one row."""
    bgr, probs = K.table_inputs(23, 31, 5)
    _check_batch(bgr, probs, n_iter, K.ROWS["neg_w"], "parity n_iter=%d" % n_iter, keys=False)


@pytest.mark.parametrize("field", K.STD_FIELDS)
def test_range_edges_on_the_device(field):
    """The smallest std the host check accepts (tests/test_crf_params_host.py: keys and neighbours fit the packed field there)."""
    H, W = 12, 16
    params = K.range_params(H, W, field)
    corner = K.inputs("corner", H, W, 3, seed=1)
    # and every position under each of the eight extreme colours: with bi_xy_std at its edge these reach neighbour coordinate 2030 of
    # 2047, the random corner image 1935
    flat = [(np.broadcast_to(np.array(c, np.uint8) * 255, (H, W, 3)).copy(), corner[1]) for c in np.ndindex(2, 2, 2)]
    bgr, probs = _batch([corner] + flat)
    _check_batch(bgr, probs, 2, params, "range %s=%.6g" % (field, K.smallest_accepted(H, W, field)[0]))


def _five(H, W, C):
    return _batch([K.inputs(kind, H, W, C, seed=20 + i) for i, kind in enumerate(("noise", "blocks", "noise", "corner", "blocks"))])


@pytest.mark.parametrize("H,W", [(9, 11), (23, 31)])
def test_batch_independence(H, W):
    """The Gaussian lattice is shared by the batch (stride 0), the bilateral one and every value buffer are per image."""
    bgr, probs = _five(H, W, 5)
    assert len({bgr[b].tobytes() for b in range(5)}) == 5
    together = _run(bgr, probs, O.MAX_ITER, DEFAULT)
    for b in range(5):
        alone = _run(bgr[b:b + 1], probs[b:b + 1], O.MAX_ITER, DEFAULT)
        assert torch.equal(together[b], alone[0]), b
    for b in range(1, 5):
        assert not torch.equal(together[b], together[0])


# two batch sizes past the cap's steps, each also with a C whose group width makes the cap bind: at C = 5 (128 rows per block) 9x11 needs 5 blocks
# of the 6 allowed and 4x5 needs one, so no grid-stride loop takes a second step; at C = 64 (16 rows per block) 9x11 asks for 38
# blocks and gets 6, at C = 17 (32 rows per block) 4x5 asks for 4 and gets 1
@pytest.mark.parametrize("B,H,W,C,n_iter", [(600, 9, 11, 5, 10), (4100, 4, 5, 3, 2), (600, 9, 11, 64, 2), (4100, 4, 5, 17, 2)])
def test_grid_cap(B, H, W, C, n_iter):
    """4096 / B blocks per image with grid-stride loops: a batch tiled from six distinct images; every copy is bitwise its first
    occurrence and the six meet the bar."""
    bgr6, probs6 = _batch([K.inputs(("noise", "blocks")[i % 2], H, W, C, seed=30 + i) for i in range(6)])
    idx = np.arange(B) % 6
    q = _run(bgr6[idx], probs6[idx], n_iter, DEFAULT)
    assert tuple(q.shape) == (B, C, H, W)
    assert torch.equal(q, q[:6][torch.from_numpy(idx).to(DEV)])
    q6 = q[:6].cpu().numpy()
    for b in range(6):
        K.Ref(bgr6[b], probs6[b], n_iter, DEFAULT).check(q6[b], "grid cap B=%d C=%d image %d" % (B, C, b))


def _edge_probs(kind, p):
    if kind == "zeros":                                      # exact zeros (the clip at 1e-5), rows still summing to 1
        z = np.where(p < 0.05, np.float32(0), p)
        out = (z / z.sum(0, keepdims=True)).astype(np.float32)
        assert (out == 0).mean() > 0.2
    elif kind == "one_hot":                                  # exact ones, -U = log 1e-5 elsewhere
        out = (np.arange(p.shape[0])[:, None, None] == p.argmax(0)[None]).astype(np.float32)
    elif kind == "half":                                     # rows sum to 0.5
        out = p * np.float32(0.5)
    else:                                                    # rows sum to 3, values above 1 meet the clip
        out = p * np.float32(3)
        assert (out > 1).mean() > 0.05
    return out


@pytest.mark.parametrize("kind", ["zeros", "one_hot", "half", "triple"])
def test_probability_edges(kind):
    bgr, p = K.inputs("noise", 9, 11, 5, seed=40)
    _check_batch(bgr[None], _edge_probs(kind, p)[None], O.MAX_ITER, DEFAULT, "prob %s" % kind, keys=False)


@pytest.mark.parametrize("C", [1, 4, 5, 16, 17, 64])
def test_group_width_boundaries(C):
    """C = 4 | 5, 16 | 17 and 64: the last C of one group width and the first of the next, the single label and the limit."""
    bgr, probs = _batch([K.inputs(kind, 9, 11, C, seed=50) for kind in ("noise", "blocks")])
    _check_batch(bgr, probs, O.MAX_ITER, DEFAULT, "prob C=%d" % C, keys=False)


@pytest.mark.parametrize("H,W", [(1, 64), (64, 1), (16, 32)])
def test_geometry_edges(H, W):
    """One row, one column, and 16x32, whose record counts 1536 and 3072 meet the 1024-position scan block (the bilateral one is
    three whole blocks)."""
    bgr, probs = _batch([K.inputs(kind, H, W, 5, seed=60) for kind in ("noise", "blocks")])
    _check_batch(bgr, probs, 2, DEFAULT, "geom %dx%d" % (H, W))
