"""One table of cases for the wide loss path (csrc/corr_wide.hip, cfg.feature_samples 12 .. 16) and the building blocks the generic path
reuses: every sampler instantiation launch_sample_panels2 can pick, the three prepared-operand GEMMs, both window counts of the backward's
GEMM kernel, gather and scatter, and the edges of the path, at the smallest shapes at which the variant can still go wrong.  Plain data, no
torch: tests/test_wide_variants_host.py walks it against csrc/corr_wide_plan.h on the CPU (the variants a row names ARE the plan's, the set
the table reaches IS the set the launchers can emit), tests/test_wide_variants_gpu.py runs every row on the device against the fp64 oracle.

A row (CASES): name, shape (B, C, H, W, K, S, n_neg), layout of the two feature maps and of the two code maps, input recipe, pointwise,
dense upstreams, cfg ("default" | "stab" = stabalize True: clamp to [0, 0.8] | "noclamp" = zero_clamp False), seed, and the variants the row
is there for: the three sampler launches "panels<VW1,VW2>" (anchors, positives, negatives), the fd GEMM, the window count and the backward
of the sampling.  PANELS: the stage cases of the one-map sampler and of the GEMM on prepared operands.

Layouts: "cl" channels-last, "nchw" contiguous, "slice1" / "slice2" the channels [1, 1 + C) / [2, 2 + C) of a channels-last buffer of C + 4
channels (a view whose first element is 4 / 8 bytes past a 16-byte boundary).

Seeds: for cfg "default" / "stab" the fp64 oracle's cd tensors have no element within CLAMP_MARGIN of a clamp bound (searched on the CPU, see
cd_margin; asserted by the host test): an element that close may pass the clamp in fp32 and fail it in fp64, a whole term of a gradient sum.
The exact zeros the "zeros" recipe makes on purpose are the one exception: a zero row's cd is 0 in any arithmetic.  Rows with too many cd
elements for a seed that clears the margin to be found (S = 16, or K >= 89 at two images) run with zero_clamp False, as the B = 203 rows of
bwd_variant_cases do."""
from collections import namedtuple

from bwd_variant_cases import CLAMP_MARGIN

Case = namedtuple("Case", "name shape flayout clayout recipe pointwise dense cfg seed variants")
PanelCase = namedtuple("PanelCase", "name C layout S vw gemm")      # one map: "panels<VW>"; gemm: the kernel dense_corr_panels takes at P = S * S

LAYOUTS = ("cl", "nchw", "slice1", "slice2")
RECIPES = ("random", "edges", "zeros", "image0")
CFGS = ("default", "stab", "noclamp")
FD_KERNELS = ("rowpair", "rowblock", "tile")
K_WINDOWS = (1, 8, 88, 89, 97, 127, 128)

# seed per input set (shape, recipe, cfg): filled by the search of cd_margin over seeds 1, 2, ...
SEEDS = {}


def facts(layout, C, H, W):
    """(stride_n, stride_c, stride_h, stride_w, byte offset of element 0 past a 256-byte boundary) of a [B, C, H, W] map in `layout`."""
    if layout == "nchw":
        return (C * H * W, H * W, W, 1, 0)
    Cb = C if layout == "cl" else C + 4
    return (H * W * Cb, 1, W * Cb, Cb, {"cl": 0, "slice1": 4, "slice2": 8}[layout])


def _vw(layout, C, H, W):
    """panel_vw of corr_wide_plan.h, restated for the table's own expectations only (the host test asks the header)."""
    sn, sc, sh, sw, off = facts(layout, C, H, W)
    for vw in (4, 2):
        if sc == 1 and C % vw == 0 and C <= 256 * vw and sn % vw == 0 and sh % vw == 0 and sw % vw == 0 and off % (4 * vw) == 0:
            return vw
    return 0


def _fd(C):
    return "rowpair" if C <= 128 else "rowblock" if C <= 384 else "tile"


def _case(name, shape, flayout="cl", clayout="cl", recipe="random", pointwise=True, dense=False, cfg="default"):
    B, C, H, W, K, S, n_neg = shape
    pair = "panels<%d,%d>" % (_vw(flayout, C, H, W), _vw(clayout, K, H, W))
    variants = (pair, "fd:" + _fd(C), "win:%d" % (1 if K <= 88 else 2), "bwd:" + ("gather" if H * W <= 4096 else "scatter"))
    return Case(name, shape, flayout, clayout, recipe, pointwise, dense, cfg, SEEDS.get((shape, recipe, cfg), 1), variants)


def _build():
    rows = []
    M = (2, 7, 9)                # B, H, W of the ordinary row: two images, an odd map
    def shp(C, K, S=12, n_neg=1, B=M[0], H=M[1], W=M[2]):
        return (B, C, H, W, K, S, n_neg)
    # ---- sampler widths: the nine two-map pairs, the two width limits, the two alignment rows
    rows.append(_case("vw42-C384-K70", shp(384, 70)))                                       # the reference's shape: row block fd
    rows.append(_case("vw42-C384-K70-dense", shp(384, 70), dense=True))
    rows.append(_case("vw44-C64-K24-S16", shp(64, 24, S=16), cfg="noclamp"))               # both point blocks full; row pair fd
    rows.append(_case("vw40-C384-K101", shp(384, 101), cfg="noclamp"))                     # odd K: scalar code side, two windows (56 + 45)
    rows.append(_case("vw24-C70-K24", shp(70, 24)))
    rows.append(_case("vw22-C134-K70", shp(134, 70)))                                       # row block fd at three chunks, the last of 6 channels
    rows.append(_case("vw20-C70-K1", shp(70, 1)))                                           # K = 1: cd is +-1
    rows.append(_case("vw04-C192nchw-K88", shp(192, 88), flayout="nchw"))                   # the last one-window K
    rows.append(_case("vw02-C65-K70", shp(65, 70)))                                         # odd C
    rows.append(_case("vw00-C128nchw-K89nchw", shp(128, 89), flayout="nchw", clayout="nchw", cfg="noclamp"))    # the first two-window K (48 + 41)
    rows.append(_case("vw0-C770-K8", shp(770, 8)))                                          # even, beyond the 512 channels of 8-byte loads; tile fd
    rows.append(_case("vw0-C1028-K127", shp(1028, 127, B=1)))                # % 4, beyond the 1024 channels of 16-byte loads
    rows.append(_case("align1-C384of388-K70", shp(384, 70), flayout="slice1"))              # base 4 bytes past: scalar loads
    rows.append(_case("align2-C384of388-K70", shp(384, 70), flayout="slice2"))              # base 8 bytes past: 8-byte loads
    # ---- fd kernels: row pair (64: above, 128), row block (134, 384: above), tile (392, 770: above); each without the pointwise shift too
    rows.append(_case("fd-C128-K8", shp(128, 8)))
    rows.append(_case("fd-C392-K8", shp(392, 8)))
    for C in (64, 128, 134, 384, 392, 770):
        rows.append(_case("fd-C%d-K8-nopointwise" % C, shp(C, 8), pointwise=False))
    # ---- code windows of the backward (1, 88, 89, 127: above)
    rows.append(_case("win-K8-stab", shp(64, 8), cfg="stab"))                               # both clamp bounds live
    rows.append(_case("win-K97-S16-dense", shp(192, 97, S=16), dense=True, cfg="noclamp"))  # windows of 56 and 41 channels, four full G tiles
    rows.append(_case("win-K128", shp(192, 128), cfg="noclamp"))
    rows.append(_case("win-K128-B1", shp(192, 128, B=1)))                                   # ... with the clamp mask live
    # ---- edges
    rows.append(_case("edge-nneg0", shp(64, 24, n_neg=0)))
    rows.append(_case("edge-nneg0-dense", shp(64, 24, n_neg=0), dense=True))
    rows.append(_case("edge-B1", shp(64, 24, B=1)))
    rows.append(_case("edge-image0", shp(64, 24, B=3, n_neg=2), recipe="image0"))
    rows.append(_case("edge-H1", shp(64, 24, H=1, W=9), recipe="edges"))
    rows.append(_case("edge-W1", shp(64, 24, H=9, W=1), recipe="edges"))
    rows.append(_case("edge-1x1", shp(64, 24, H=1, W=1), recipe="edges"))                    # every point samples the one pixel
    rows.append(_case("edge-coords", shp(64, 24, H=5, W=9), recipe="edges"))
    rows.append(_case("edge-coords-dense", shp(64, 24, H=5, W=9), recipe="edges", dense=True))
    rows.append(_case("edge-zeros", shp(64, 24), recipe="zeros"))
    rows.append(_case("edge-zeros-dense", shp(64, 24), recipe="zeros", dense=True))
    rows.append(_case("edge-S13", shp(64, 24, S=13)))                                       # 169 points: odd P (scalar w loads in the backward), 41 rows in the second block
    # ---- the scatter path: a map of more than 4096 pixels
    rows.append(_case("scatter-65x64", shp(16, 24, H=65, W=64)))
    rows.append(_case("scatter-65x64-dense", shp(16, 24, H=65, W=64), dense=True))
    return rows


SEEDS.update({                                                          # (shape, recipe, cfg): seed; the distance of the nearest cd element to a bound
    ((1, 1028, 7, 9, 127, 12, 1), 'random', 'default'): 3448,      # 2.7e-05
    ((1, 192, 7, 9, 128, 12, 1), 'random', 'default'): 1492,      # 2.1e-05
    ((1, 64, 7, 9, 24, 12, 1), 'random', 'default'): 190,      # 3.2e-05
    ((2, 128, 7, 9, 8, 12, 1), 'random', 'default'): 1865,      # 3.3e-05
    ((2, 134, 7, 9, 70, 12, 1), 'random', 'default'): 899,      # 1.1e-05
    ((2, 134, 7, 9, 8, 12, 1), 'random', 'default'): 1865,      # 3.3e-05
    ((2, 16, 65, 64, 24, 12, 1), 'random', 'default'): 4343,      # 2.4e-05
    ((2, 192, 7, 9, 88, 12, 1), 'random', 'default'): 4277,      # 1.2e-05
    ((2, 384, 7, 9, 70, 12, 1), 'random', 'default'): 899,      # 1.1e-05
    ((2, 384, 7, 9, 8, 12, 1), 'random', 'default'): 1865,      # 3.3e-05
    ((2, 392, 7, 9, 8, 12, 1), 'random', 'default'): 1865,      # 3.3e-05
    ((2, 64, 1, 1, 24, 12, 1), 'edges', 'default'): 1,      # 1.3e-01
    ((2, 64, 1, 9, 24, 12, 1), 'edges', 'default'): 4,      # 7.3e-05
    ((2, 64, 5, 9, 24, 12, 1), 'edges', 'default'): 1373,      # 3.3e-05
    ((2, 64, 7, 9, 24, 12, 0), 'random', 'default'): 835,      # 3.4e-05
    ((2, 64, 7, 9, 24, 12, 1), 'zeros', 'default'): 5402,      # 2.5e-05
    ((2, 64, 7, 9, 24, 13, 1), 'random', 'default'): 4034,      # 1.8e-05
    ((2, 64, 7, 9, 8, 12, 1), 'random', 'default'): 1865,      # 3.3e-05
    ((2, 64, 7, 9, 8, 12, 1), 'random', 'stab'): 3698,      # 3.5e-05
    ((2, 64, 9, 1, 24, 12, 1), 'edges', 'default'): 4,      # 6.0e-05
    ((2, 65, 7, 9, 70, 12, 1), 'random', 'default'): 899,      # 1.1e-05
    ((2, 70, 7, 9, 1, 12, 1), 'random', 'default'): 1,      # 1.0e+00
    ((2, 70, 7, 9, 24, 12, 1), 'random', 'default'): 646,      # 2.4e-05
    ((2, 770, 7, 9, 8, 12, 1), 'random', 'default'): 1865,      # 3.3e-05
    ((3, 64, 7, 9, 24, 12, 2), 'image0', 'default'): 5440,      # 1.5e-05
})

CASES = _build()

# ---- stage cases: the one-map sampler instantiations by every reason for a width, and the operands of the three GEMMs
PANELS = [
    PanelCase("one4-C64", 64, "cl", 12, 4, "rowpair"),
    PanelCase("one4-C128", 128, "cl", 16, 4, "rowpair"),
    PanelCase("one4-C384", 384, "cl", 12, 4, "rowblock"),
    PanelCase("one4-C392", 392, "cl", 12, 4, "tile"),
    PanelCase("one4-C1024", 1024, "cl", 12, 4, "tile"),              # the last 16-byte width: every lane's four vectors live
    PanelCase("one2-C70", 70, "cl", 12, 2, "rowpair"),
    PanelCase("one2-C134", 134, "cl", 12, 2, "rowblock"),
    PanelCase("one2-C510", 510, "cl", 12, 2, "tile"),                # the last 8-byte width short of a full chunk
    PanelCase("one2-slice2", 384, "slice2", 12, 2, "rowblock"),
    PanelCase("one0-C65", 65, "cl", 12, 0, "rowpair"),
    PanelCase("one0-C770", 770, "cl", 12, 0, "tile"),
    PanelCase("one0-C1028", 1028, "cl", 12, 0, "tile"),
    PanelCase("one0-nchw", 192, "nchw", 12, 0, "rowblock"),
    PanelCase("one0-slice1", 384, "slice1", 12, 0, "rowblock"),
]
PANEL_MAP = (2, 7, 9)            # B, H, W of the stage cases' maps


def edge_coords(rng, B, S, H, W):
    """Coordinates that mix interior points, exact +-1, exact pixel centres (where -1 + 2 i / (n - 1) is a float32: n - 1 a power of two) and
    values out to +-1.2, independently per axis."""
    import numpy as np
    def axis(n):
        kind = rng.integers(0, 20, (B, S, S))
        v = rng.random((B, S, S)) * 2 - 1                                              # interior
        v = np.where(kind < 3, np.where(rng.random((B, S, S)) < 0.5, -1.0, 1.0), v)     # exactly on the border
        if n > 1 and (n - 1) & (n - 2) == 0:
            v = np.where((kind >= 3) & (kind < 8), -1.0 + 2.0 * rng.integers(0, n, (B, S, S)) / (n - 1), v)      # pixel centres
        v = np.where(kind >= 15, (rng.random((B, S, S)) * 0.2 + 1.0) * np.where(rng.random((B, S, S)) < 0.5, -1.0, 1.0), v)      # beyond
        return v
    return np.stack([axis(W), axis(H)], axis=-1).astype(np.float32)


def make_codes(case):
    """The code side of a row's inputs (numpy): what cd, its clamp mask and the gradients' sparsity depend on."""
    import numpy as np
    B, C, H, W, K, S, n_neg = case.shape
    rng = np.random.default_rng(case.seed)
    d = dict(code=rng.standard_normal((B, K, H, W)).astype(np.float32), code_pos=rng.standard_normal((B, K, H, W)).astype(np.float32))
    if case.recipe == "edges":
        d["coords1"], d["coords2"] = edge_coords(rng, B, S, H, W), edge_coords(rng, B, S, H, W)
    else:
        d["coords1"] = (rng.random((B, S, S, 2)) * 2 - 1).astype(np.float32)
        d["coords2"] = (rng.random((B, S, S, 2)) * 2 - 1).astype(np.float32)
    if case.recipe == "image0":
        perms = np.zeros((n_neg, B), np.int64)        # every negative draws image 0 (image 0 itself draws 1: super_perm has no fixed points)
        perms[:, 0] = 1
    else:
        from oracle.corr_oracle import super_perm_from_randperm
        perms = np.stack([super_perm_from_randperm(rng.permutation(B)) for _ in range(n_neg)]).astype(np.int64) if n_neg else np.zeros((0, B), np.int64)
    d["perms"] = perms
    if case.recipe == "zeros":
        d["code"][0, :, 1:5, 2:7] = 0.0               # blocks of zero pixels: the points that fall inside sample exactly zero rows
        d["code_pos"][B - 1, :, 2:6, 0:5] = 0.0
    return d


def make_inputs(case):
    """The row's inputs as numpy arrays; dense rows also carry "ups": seeded standard-normal upstreams on all six outputs."""
    import numpy as np
    B, C, H, W, K, S, n_neg = case.shape
    d = make_codes(case)
    rf = np.random.default_rng(77000 + C)
    d["feats"] = rf.standard_normal((B, C, H, W)).astype(np.float32)
    d["feats_pos"] = rf.standard_normal((B, C, H, W)).astype(np.float32)
    if case.recipe == "zeros":
        d["feats"][B - 1, :, 0:4, 3:8] = 0.0
        d["feats_pos"][0, :, 3:7, 4:9] = 0.0
    if case.dense:
        rng = np.random.default_rng(case.seed + 1000)
        shapes = [(), (B, S, S, S, S), (), (B, S, S, S, S), (n_neg * B, S, S, S, S), (n_neg * B, S, S, S, S)]
        d["ups"] = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    return d


def clamp_bounds(cfg):
    return {"default": (0.0, None), "stab": (0.0, 0.8), "noclamp": (None, None)}[cfg]


def cd_margin(case, d=None):
    """The smallest distance of an element of the fp64 cd tensors to a clamp bound of the row's cfg (exact zeros excepted in the "zeros"
    recipe), from the code side alone: modules.py:369-373, :385, :336."""
    import numpy as np
    from oracle import corr_oracle as O
    d = d or make_codes(case)
    c, cp = d["code"].astype(np.float64), d["code_pos"].astype(np.float64)
    c1, c2 = d["coords1"].astype(np.float64), d["coords2"].astype(np.float64)
    a = O.norm(O.sample(c, c1))
    seconds = [a, O.norm(O.sample(cp, c2))] + [O.norm(O.sample(c[p], c2)) for p in d["perms"]]
    lo, hi = clamp_bounds(case.cfg)
    m = np.inf
    for b in seconds:
        cd = O.tensor_correlation(a, b)
        if case.recipe == "zeros":
            cd = cd[cd != 0.0]
        for bound in (lo, hi):
            if bound is not None and cd.size:
                m = min(m, float(np.abs(cd - bound).min()))
    return m
