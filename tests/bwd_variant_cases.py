"""One table of backward cases for the correspondence loss: every kernel pair launch_corr_bwd() / launch_corr_bwd_lists() can dispatch
(csrc/corr_bwd_plan.h) and every limit of bwd_check, at the smallest shapes at which the variant can still go wrong.  Plain data, no torch:
tests/test_bwd_variants_host.py walks it against the plan header on the CPU (the kernel pair named in a row IS the plan's, the set the table
reaches IS the set the two units emit), tests/test_bwd_variants_gpu.py runs every row on the device against the fp64 oracle.

A row: name, shape (B, C, H, W, K, S, n_neg; helper rows: N, C, S1, S2, K, S2, 0), precision, dense upstreams, STEGO_DEBUG_BWD (host-side
path bits only: 32 band, 512 fp32 tiles, 1024 no lists - the ablation bits change results), mode ("forward" | "helper"), cfg ("default" |
"noclamp" = zero_clamp False), seed, input recipe, and the (tile kernel, unsample kernel) pair the row is there for.

Seeds: for cfg "default" the fp64 oracle's cd tensors have no element within CLAMP_MARGIN of a clamp bound (found by searching seeds with the
oracle on the CPU, asserted by the host test): an element that close may pass the clamp in fp32 and fail it in fp64, a whole term of a
gradient sum.  The B = 203 rows (812 000 cd elements) have no such seed among the first twelve; they exist for the unsample kernels, not for
the clamp mask, and run with zero_clamp False."""
from collections import namedtuple

Case = namedtuple("Case", "name shape precision dense debug mode cfg seed recipe kernels")
Refusal = namedtuple("Refusal", "name shape precision debug why")     # why: "bwd_check" (STEGO_ERR_UNSUPPORTED) | "no_kernel" (the plan is Invalid)

DBG_BAND, DBG_F32_TILES, DBG_NO_LISTS = 32, 512, 1024
ALLOWED_DEBUG_BITS = DBG_BAND | DBG_F32_TILES | DBG_NO_LISTS
RECIPES = ("random", "crowded_row", "one_image_negatives")
CLAMP_MARGIN = 1e-5          # four times the 2.5e-6 test_split_fp16_error_bound_on_adversarial_inputs allows the forward's cd

K_LIST = (8, 24, 40, 64, 65, 80, 81, 112, 128)

# seed per input set (shape, recipe, mode); cfg "default" sets: the first of seeds 1, 2, ... whose margin is comfortable
SEEDS = {}


def _nt(K):
    return (((K + 7) & ~7) + 15) // 16


def _C(K):
    return 192 if K > 72 else 32          # K > 72 exists on the fused forward only: channels-last ViT-width maps


def _list(K):
    return "list<1,0>" if K <= 64 else "list<1,1>" if K <= 80 else "list<2,0>"


def _row(W, K):
    return "row<%d,%d>" % (2 if W <= 32 else 4, 5 if _nt(K) <= 5 else 8)


def _seed(shape, recipe, mode):
    return SEEDS.get((shape, recipe, mode), 1)


def _case(name, shape, precision, dense, debug, kernels, mode="forward", cfg="default", recipe="random"):
    return Case(name, shape, precision, dense, debug, mode, cfg, _seed(shape, recipe, mode), recipe, kernels)


def _build():
    rows = []
    # ---- lists first: two bins, the second partial
    for K in K_LIST:
        shape = (3, _C(K), 6, 20, K, 5, 2)
        rows.append(_case("lists-f16x3-K%d" % K, shape, "f16x3", False, 0, ("tile_build<%d>" % _nt(K), _list(K))))
        if K <= 81:     # K = 81: F32 takes the split kernel
            rows.append(_case("lists-f32-K%d" % K, shape, "f32", False, 0,
                              ("tile32_build<%d>" % _nt(K) if K <= 80 else "tile_build<%d>" % _nt(K), _list(K))))
    rows.append(_case("lists-f16x3-K40-fp32tiles", (3, 32, 6, 20, 40, 5, 2), "f16x3", False, DBG_F32_TILES, ("tile32_build<3>", "list<1,0>")))
    # ---- tile + row: W alternates 20 / 40 down the K list (row<2|4, 5|8>)
    for i, K in enumerate(K_LIST):
        W = 40 if i % 2 else 20
        shape = (3, _C(K), 6, W, K, 5, 2)
        rows.append(_case("row-f16x3-K%d-W%d" % (K, W), shape, "f16x3", False, DBG_NO_LISTS, ("tile_h<%d,false>" % _nt(K), _row(W, K))))
        rows.append(_case("row-f16x3-K%d-W%d-dense" % (K, W), shape, "f16x3", True, 0, ("tile_h<%d,true>" % _nt(K), _row(W, K))))
        if K <= 80:
            rows.append(_case("row-f32-K%d-W%d" % (K, W), shape, "f32", False, DBG_NO_LISTS, ("tile_kernel<%d>" % _nt(K), _row(W, K))))
            rows.append(_case("row-f32-K%d-W%d-dense" % (K, W), shape, "f32", True, 0, ("tile_kernel<%d>" % _nt(K), _row(W, K))))
    rows.append(_case("row-f16x3-H65-dense", (2, 32, 65, 16, 8, 5, 1), "f16x3", True, 0, ("tile_h<1,true>", "row<2,5>")))
    # ---- row kernel, several passes of the 256-candidate item scan: 267 candidates, 266 of them items of image 0
    many = (52, 32, 8, 8, 8, 5, 5)
    rows.append(_case("row-passes-B52", many, "f16x3", False, DBG_NO_LISTS, ("tile_h<1,false>", "row<2,5>"), recipe="one_image_negatives"))
    rows.append(_case("row-passes-B52-dense", many, "f16x3", True, 0, ("tile_h<1,true>", "row<2,5>"), recipe="one_image_negatives"))
    # ---- the last accepted contribution count, 7 + 5 * 203 = 1022, 1021 of them on image 0: item table at its cap, lists from the overflow pool
    last = (203, 32, 8, 8, 16, 5, 5)
    rows.append(_case("contrib1022-lists", last, "f16x3", False, 0, ("tile_build<1>", "list<1,0>"), cfg="noclamp", recipe="one_image_negatives"))
    rows.append(_case("contrib1022-row", last, "f16x3", False, DBG_NO_LISTS, ("tile_h<1,false>", "row<2,5>"), cfg="noclamp", recipe="one_image_negatives"))
    rows.append(_case("contrib1022-band", last, "f16x3", False, DBG_BAND, ("tile_h<1,false>", "unsample_kernel"), cfg="noclamp", recipe="one_image_negatives"))
    # ---- band
    for prec in ("f16x3", "f32"):       # rt = 2, three bands, the last partial, both channel halves full (F32 at K = 128: the split kernel)
        rows.append(_case("band-%s-W66-K128" % prec, (2, 192, 5, 66, 128, 5, 1), prec, False, 0, ("tile_h<8,false>", "unsample_kernel")))
    rows.append(_case("band-f16x3-W70-K100", (2, 192, 5, 70, 100, 5, 1), "f16x3", False, 0, ("tile_h<7,false>", "unsample_kernel")))      # partial upper channel half
    rows.append(_case("band-f16x3-W70-K100-dense", (2, 192, 5, 70, 100, 5, 1), "f16x3", True, 0, ("tile_h<7,true>", "unsample_kernel")))
    rows.append(_case("band-f16x3-W192-K128", (2, 192, 3, 192, 128, 4, 1), "f16x3", False, 0, ("tile_h<8,false>", "unsample_kernel")))    # rt = 1 at W K 4 == UNS_BAND_BYTES
    for prec in ("f16x3", "f32"):       # 4 x 121 = 484 row-entries on one pixel row per round: the worklist overflows into LDS atomics
        rows.append(_case("band-%s-crowded" % prec, (2, 8, 3, 70, 8, 11, 2), prec, False, 0,
                          ("tile_h<1,false>" if prec == "f16x3" else "tile_kernel<1>", "unsample_kernel"), recipe="crowded_row"))
    rows.append(_case("band-f16x3-B70", (70, 8, 2, 66, 8, 3, 1), "f16x3", False, 0, ("tile_h<1,false>", "unsample_kernel"),
                      recipe="one_image_negatives"))          # a second ballot round of the contribution table
    # ---- helper() at its limits: K = 72, 128 points; dense upstreams on loss and cd; the fp32 tile kernel in either precision
    for prec in ("f16x3", "f32"):
        rows.append(_case("helper-%s-K72" % prec, (3, 48, 8, 16, 72, 16, 0), prec, True, 0, ("tile_kernel<5>", "row<2,5>"), mode="helper"))
    return rows


SEEDS.update({                                                          # min |cd| of the fp64 oracle (the clamp bound is 0)
    ((3, 32, 6, 20, 8, 5, 2), "random", "forward"): 2,                  # 1.1e-04
    ((3, 32, 6, 20, 24, 5, 2), "random", "forward"): 2,                 # 4.7e-05
    ((3, 32, 6, 20, 40, 5, 2), "random", "forward"): 1,                 # 7.3e-05
    ((3, 32, 6, 20, 64, 5, 2), "random", "forward"): 2,                 # 4.1e-05
    ((3, 32, 6, 20, 65, 5, 2), "random", "forward"): 1,                 # 3.1e-05
    ((3, 192, 6, 20, 80, 5, 2), "random", "forward"): 1,                # 1.0e-04
    ((3, 192, 6, 20, 81, 5, 2), "random", "forward"): 11,               # 3.8e-05
    ((3, 192, 6, 20, 112, 5, 2), "random", "forward"): 7,               # 3.2e-05
    ((3, 192, 6, 20, 128, 5, 2), "random", "forward"): 4,               # 3.4e-05
    ((3, 32, 6, 40, 24, 5, 2), "random", "forward"): 1,                 # 1.1e-04
    ((3, 32, 6, 40, 64, 5, 2), "random", "forward"): 1,                 # 3.5e-05
    ((3, 192, 6, 40, 80, 5, 2), "random", "forward"): 2,                # 1.3e-04
    ((3, 192, 6, 40, 112, 5, 2), "random", "forward"): 1,               # 6.5e-05
    ((2, 32, 65, 16, 8, 5, 1), "random", "forward"): 1,                 # 3.1e-04
    ((52, 32, 8, 8, 8, 5, 5), "one_image_negatives", "forward"): 9,     # 1.5e-05
    ((203, 32, 8, 8, 16, 5, 5), "one_image_negatives", "forward"): 5,   # 1.8e-06, the best of twelve seeds: zero_clamp False
    ((2, 192, 5, 66, 128, 5, 1), "random", "forward"): 1,               # 7.4e-05
    ((2, 192, 5, 70, 100, 5, 1), "random", "forward"): 1,               # 4.6e-05
    ((2, 192, 3, 192, 128, 4, 1), "random", "forward"): 1,              # 5.2e-05
    ((2, 8, 3, 70, 8, 11, 2), "crowded_row", "forward"): 11,            # 1.5e-05
    ((70, 8, 2, 66, 8, 3, 1), "one_image_negatives", "forward"): 5,     # 3.8e-05
    ((2, 192, 4, 193, 128, 5, 1), "random", "forward"): 2,              # 7.9e-05 (SURFACE)
    ((3, 48, 8, 16, 72, 16, 0), "random", "helper"): 100,               # 2.1e-05 (49152 elements: one seed in ~30 clears the margin)
})

CASES = _build()

REFUSALS = [
    Refusal("refused-contrib1027", (204, 32, 8, 8, 16, 5, 5), "f16x3", 0, "bwd_check"),           # n_sets + n_neg B = 1027 > 1024
    Refusal("refused-W193-K128", (2, 192, 4, 193, 128, 5, 1), "f16x3", 0, "bwd_check"),           # W K 4 = 98816 > UNS_BAND_BYTES
    Refusal("refused-fp32tiles-K81", (3, 192, 6, 20, 81, 5, 2), "f16x3", DBG_F32_TILES, "no_kernel"),     # six channel tiles have no fp32 kernel
]
AFTER_REFUSAL = "lists-f16x3-K8"         # a small case that must still give oracle gradients after the refusals

# the Python surface at the two refused shapes (ContrastiveCorrelationLoss.forward_explicit + backward(): generic_forward must take them)
SURFACE = [
    _case("surface-contrib1027", (204, 32, 8, 8, 16, 5, 5), "f16x3", False, 0, (), cfg="noclamp"),     # (816 000 cd elements: no seed with the margin)
    _case("surface-W193-K128", (2, 192, 4, 193, 128, 5, 1), "f16x3", False, 0, ()),
]


def twin(case):
    """The F32 row that differs from an F16X3 row in the precision alone (same inputs, path and upstreams), or None."""
    if case.precision != "f16x3":
        return None
    for c in CASES:
        if c.precision == "f32" and c._replace(name="", precision="", kernels=()) == case._replace(name="", precision="", kernels=()):
            return c
    return None


def make_inputs(case):
    """The row's inputs as numpy arrays (oracle.corr_oracle.synth_inputs + the recipe); helper rows: f1, f2, c1, c2.  Dense rows also carry
    "ups": seeded standard-normal upstreams on all six outputs (helper: on loss and cd)."""
    import numpy as np
    from oracle import corr_oracle as O
    B, C, H, W, K, S, n_neg = case.shape
    rng = np.random.default_rng(case.seed + 1000)
    if case.mode == "helper":
        r = np.random.default_rng(case.seed)
        d = dict(zip(("f1", "f2"), (r.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(2))))
        d.update(zip(("c1", "c2"), (r.standard_normal((B, K, H, W)).astype(np.float32) for _ in range(2))))
        n = (B, H, W, H, W)
        d["ups"] = [(rng.standard_normal(n) / (H * W) ** 2).astype(np.float32) for _ in range(2)]
        return d
    d = O.synth_inputs(B, C, H, W, K, S, n_neg, seed=case.seed)
    if case.recipe == "one_image_negatives":
        perms = np.zeros((n_neg, B), np.int64)
        perms[:, 0] = 1                          # (no fixed points: super_perm never maps b to b)
        d["perms"] = perms
    elif case.recipe == "crowded_row":
        for key in ("coords1", "coords2"):
            d[key][:B // 2, :, :, 1] = -2.0      # beyond the border: the first pixel row
            d[key][B // 2:, :, :, 1] = 1.7       # the last one
    else:
        assert case.recipe == "random"
    if case.dense:
        shapes = [(), (B, S, S, S, S), (), (B, S, S, S, S), (n_neg * B, S, S, S, S), (n_neg * B, S, S, S, S)]
        d["ups"] = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    return d
