"""The split-fp16 tile body on v_mfma_f32_16x16x32_f16 (bwd_tile_h_body, csrc/corr_bwd_tile.h) at the smallest shapes that reach every
way its operand path can go wrong: a lane's fragment is 8 points of a code row - ONE 16-byte block of the XOR-swizzled image, its halves
exchanged in the odd channel tiles - against 8 points of G (a 16-byte row read in gemm_dA, two transposing reads in gemm_dB; both with the
halves the other way round for the odd tiles).  Per shape: the training path (lists first) with scalar upstreams, the same with
STEGO_DEBUG_BWD 2048 (both sides normalised and stored at the end), and dense upstreams through corr_bwd_tile_h_kernel<nt, true>; each against
the fp64 oracle (the bar of tests/test_bwd_fused.py) and twice, bit for bit.  Helpers of tests/test_bwd_variants_gpu.py.  The device
tests need the MI355X; the seed condition below runs anywhere."""
import numpy as np
import pytest

import bwd_variant_cases as T
import test_bwd_variants_gpu as V

DBG_LATE_DB = 2048

# (B, C, H, W, K, S, n_neg), seed.  Seeds: the first of 1, 2, ... at which no cd element of the fp64 oracle lies within T.CLAMP_MARGIN of the
# clamp bound (twice the margin where a seed below 40 has it; see bwd_variant_cases: such an element may pass the clamp in fp32 and fail
# it in fp64); asserted below.
SHAPES = [
    ((2, 32, 8, 8, 8, 3, 1), 1),           # P = 9: less than one k block; one channel tile (mc = 0 only)                    margin 8.0e-04
    ((2, 32, 8, 8, 24, 6, 1), 1),          # P = 36: one full and one partial k block; mc 0 and 1: one exchanged-half fragment      6.6e-05
    ((2, 32, 12, 12, 40, 8, 2), 11),       # P = 64: exact blocks; three channel tiles                                              2.3e-05
    ((2, 32, 12, 12, 70, 11, 2), 56),      # P = 121, nt = 5: the training tile (117 128 cd elements: the first seed at the margin) 1.06e-05
    ((2, 384, 12, 12, 100, 6, 2), 3),      # nt = 7 in two groups: the late order and the new fragments together                    5.1e-05
    ((1, 32, 8, 8, 16, 5, 0), 1),          # no negatives: the intra tile (A is B) and one inter tile                               2.7e-05
]
IDS = ["P9-nt1", "P36-nt2", "P64-nt3", "P121-nt5", "P36-nt7-two-groups", "P25-intra"]


def _case(i, dense, debug):
    shape, seed = SHAPES[i]
    nt = T._nt(shape[4])
    kernels = ("tile_h<%d,true>" % nt, T._row(shape[3], shape[4])) if dense else ("tile_build<%d>" % nt, T._list(shape[4]))
    return T.Case("k32-%s%s%s" % (IDS[i], "-dense" if dense else "", "-late" if debug else ""), shape, "f16x3", dense, debug, "forward",
                  "default", seed, "random", kernels)


_FWD = {}


def _backwards(i, dense, debug):
    """(first call, second call, oracle) of a shape; one forward per (shape, upstreams), shared by the default and the late-dB run."""
    case = _case(i, dense, debug)
    d = T.make_inputs(case)
    if (i, dense) not in _FWD:
        _FWD.clear()                                  # one saved context alive at a time
        _FWD[(i, dense)] = V._Forward(case.shape, case.precision, V._cfg(case), d)
    fwd = _FWD[(i, dense)]
    return case, fwd.backward(debug), fwd.backward(debug), V._oracle(case, d)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_seeds_keep_every_cd_element_away_from_the_clamp_bound(i):
    from test_bwd_variants_host import _cd_margin
    m = _cd_margin(_case(i, False, 0))
    assert m >= T.CLAMP_MARGIN, (IDS[i], m)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_k32_tiles_scalar_upstreams_early_and_late_db(i):
    case, a, b, exp = _backwards(i, False, 0)
    print("K32 %s: max error / max|oracle| = %.3e" % (case.name, V._rel_err(a, exp)))
    V._check_against_oracle(case, a, exp)
    for x, y in zip(a, b):
        assert np.array_equal(x, y), case.name + ": not repeatable"
    late, la, lb, _ = _backwards(i, False, DBG_LATE_DB)
    V._check_against_oracle(late, la, exp)
    for x, y in zip(la, lb):
        assert np.array_equal(x, y), late.name + ": not repeatable"
    # the bound tests/test_bwd_fused.py uses between its two paths: the order of the two GEMMs and of the stores changes no sum
    for x, y, what in zip(a, la, ("d_code", "d_code_pos")):
        diff, scale = float(np.abs(x - y).max()), float(np.abs(x).max())
        print("K32 %s %s: early vs late dB %.3e of the largest entry" % (case.name, what, diff / scale))
        assert diff <= 4e-6 * scale, (case.name, what, diff, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_k32_tiles_dense_upstreams(i):
    case, a, b, exp = _backwards(i, True, 0)
    print("K32 %s: max error / max|oracle| = %.3e" % (case.name, V._rel_err(a, exp)))
    V._check_against_oracle(case, a, exp)
    for x, y in zip(a, b):
        assert np.array_equal(x, y), case.name + ": not repeatable"
