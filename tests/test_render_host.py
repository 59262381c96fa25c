"""Coloured pictures without a GPU: the C ABI's surface and host checks (include/stego_render.h), the colormaps, the cluster -> class
vector and the torch chains against tests/golden/render_small.npz, which records what the reference's own functions return
(tools/make_render_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from stego_amd import capi, render
from stego_amd.metrics import DeviceUnsupervisedMetrics
from stego_amd.utils import UnsupervisedMetrics

A = 0x10000          # an aligned stand-in address: the checks reject before any pointer is read
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stego_render.h")).read()
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "render_small.npz"))
L, I, E, BL, R = capi.RENDER_LABELS, capi.RENDER_IMAGE, capi.RENDER_EDGES, capi.RENDER_BLEND, capi.RENDER_RESCALE


def _desc(**kw):
    d = dict(B=2, H=37, W=53, n_lut=27, label_dtype=capi.RENDER_I64, flags=L, alpha=0.5, label_strides=(37 * 53, 53, 1),
             out_strides=(37 * 53 * 3, 53 * 3))
    d.update(kw)
    return capi.render_desc(**d)


def _rc(desc, null=True):
    """stego_render with NULL pointers (the descriptor checks come first), or with stand-in addresses."""
    if null:
        return capi.render_raw(desc, None, None, None, None, None)
    return capi.render_raw(desc, capi.StegoMap(A, 3 * 37 * 53, 37 * 53, 53, 1), A, A, A, A)


def test_symbols_abi_and_error_constants():
    lib = capi.load()
    assert lib.stego_abi_version() == 7 == capi.ABI_VERSION
    for name in ("stego_image_range_workspace_bytes", "stego_image_range", "stego_render"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, HEADER), name
    names = ("SIZE", "LUT", "DTYPE", "FLAGS", "PARAM", "SELECT")
    for name in names:
        rc = getattr(capi, "RENDER_ERR_" + name)
        assert re.search(r"STEGO_ERR_RENDER_%s = %d\b" % (name, rc), HEADER), name
        assert lib.stego_error_string(rc).decode().startswith("render:"), rc
    assert len(re.findall(r"STEGO_ERR_RENDER_\w+ = \d+", HEADER)) == len(names)
    for name in ("IMAGE", "LABELS", "EDGES", "BLEND", "RESCALE", "I64", "I32", "U8"):
        assert re.search(r"STEGO_RENDER_%s = %d\b" % (name, getattr(capi, "RENDER_" + name)), HEADER), name
    assert re.search(r"#define STEGO_RENDER_MAX_LUT %d\b" % capi.RENDER_MAX_LUT, HEADER)


def test_descriptor_fields_follow_the_header():
    body = re.search(r"typedef struct StegoRenderDesc \{(.*?)\} StegoRenderDesc;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            fields += [(ctype, re.sub(r"\[\d+\]", "", n.strip()), re.findall(r"\[(\d+)\]", n)) for n in rest.split(",")]
    ctypes_of = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "uint8_t": ctypes.c_uint8, "int64_t": ctypes.c_int64}
    assert [n for _, n, _ in fields] == [n for n, _ in capi.StegoRenderDesc._fields_]
    for (ctype, name, dims), (_, have) in zip(fields, capi.StegoRenderDesc._fields_):
        want = ctypes_of[ctype] * int(dims[0]) if dims else ctypes_of[ctype]
        assert ctypes.sizeof(have) == ctypes.sizeof(want) and (have is want or have._type_ is ctypes_of[ctype]), name


@pytest.mark.parametrize("kw,rc", [
    (dict(B=0), capi.RENDER_ERR_SIZE), (dict(B=65536), capi.RENDER_ERR_SIZE),
    (dict(H=0), capi.RENDER_ERR_SIZE), (dict(H=32769), capi.RENDER_ERR_SIZE),
    (dict(W=0), capi.RENDER_ERR_SIZE), (dict(W=32769), capi.RENDER_ERR_SIZE),
    (dict(n_lut=0), capi.RENDER_ERR_LUT), (dict(n_lut=513), capi.RENDER_ERR_LUT),
    (dict(label_dtype=3), capi.RENDER_ERR_DTYPE), (dict(label_dtype=-1), capi.RENDER_ERR_DTYPE),
    (dict(flags=L | 32), capi.RENDER_ERR_FLAGS), (dict(flags=-1), capi.RENDER_ERR_FLAGS),
    (dict(flags=L | I | BL, alpha=-0.01), capi.RENDER_ERR_PARAM), (dict(flags=L | I | BL, alpha=1.01), capi.RENDER_ERR_PARAM),
    (dict(flags=L | I | BL, alpha=float("nan")), capi.RENDER_ERR_PARAM),
    (dict(flags=I, mean=(0.0, float("inf"), 0.0)), capi.RENDER_ERR_PARAM),
    (dict(flags=0), capi.RENDER_ERR_SELECT),                          # neither image nor labels
    (dict(flags=E), capi.RENDER_ERR_SELECT),
    (dict(flags=L | BL), capi.RENDER_ERR_SELECT), (dict(flags=I | BL), capi.RENDER_ERR_SELECT),      # BLEND without both
    (dict(flags=L | I), capi.RENDER_ERR_SELECT),                      # both without BLEND
    (dict(flags=I | E), capi.RENDER_ERR_SELECT),                      # EDGES without labels
    (dict(flags=L | R), capi.RENDER_ERR_SELECT),                      # RESCALE without an image, so without a range
])
def test_descriptor_checks_come_first(kw, rc):
    assert _rc(_desc(**kw)) == rc                  # with NULL pointers: the code is the descriptor's, nothing was enqueued
    assert _rc(_desc(**kw), null=False) == rc


def test_pointer_checks():
    lib = capi.load()
    assert lib.stego_render(None, None, A, A, A, A, None) == 1
    assert _rc(_desc()) == 1                                                       # valid descriptor, NULL pointers
    m = capi.StegoMap(A, 3 * 37 * 53, 37 * 53, 53, 1)
    assert capi.render_raw(_desc(flags=I | R), m, None, None, None, A) == 1        # RESCALE selected, no range
    assert capi.render_raw(_desc(flags=I), m, None, None, None, None) == 1         # no target
    assert capi.render_raw(_desc(), None, A, None, None, A) == 1                   # labels without a table
    assert capi.render_raw(_desc(), None, A + 4, A, None, A + 1) == 5              # int64 labels at 4 mod 8
    assert capi.render_raw(_desc(flags=I), capi.StegoMap(A + 2, 1, 1, 1, 1), None, None, None, A) == 5
    assert capi.render_raw(_desc(flags=I | R), m, None, None, A + 2, A) == 5
    # limits are inclusive, a skipped input's fields are not read: these stop at the misaligned labels / image
    assert capi.render_raw(_desc(B=65535, H=32768, W=32768, n_lut=512), None, A + 4, A, None, A + 3) == 5
    assert capi.render_raw(_desc(flags=I, n_lut=0, label_dtype=9), capi.StegoMap(A + 2, 1, 1, 1, 1), None, None, None, A) == 5


def test_image_range_checks():
    assert capi.image_range_workspace_bytes(_desc(flags=I)) >= 2 * 2 * 4
    assert capi.image_range_workspace_bytes(_desc(H=0)) == 0
    assert capi.image_range_raw(_desc(W=32769), None, None, None, 0) == capi.RENDER_ERR_SIZE
    assert capi.image_range_raw(_desc(std=(1.0, float("nan"), 1.0)), None, None, None, 0) == capi.RENDER_ERR_PARAM
    assert capi.image_range_raw(_desc(), None, None, None, 0) == 1
    m = capi.StegoMap(A, 3 * 37 * 53, 37 * 53, 53, 1)
    need = capi.image_range_workspace_bytes(_desc())
    assert capi.image_range_raw(_desc(), m, A, A, need - 1) == 4
    assert capi.image_range_raw(_desc(), m, A + 2, A, need) == 5
    # one workgroup per 2048 pixels, 1024 at the most, two floats each, rounded to 16 bytes
    assert capi.image_range_workspace_bytes(_desc(B=3, H=4800, W=4800)) == 3 * 1024 * 8
    assert capi.image_range_workspace_bytes(_desc(B=1, H=1, W=1)) == 16


def test_colormaps_equal_the_reference():
    pascal, city = render.pascal_label_colormap(), render.cityscapes_colormap()
    assert pascal.shape == (512, 3) and np.array_equal(pascal, GOLD["pascal"])
    assert city.shape == (28, 3) and np.array_equal(city, GOLD["cityscapes"])
    assert np.array_equal(render.label_cmap("cityscapes"), GOLD["cityscapes"])
    assert np.array_equal(render.label_cmap("cocostuff27"), GOLD["pascal"])
    assert np.array_equal(render.label_cmap("potsdam"), GOLD["pascal"])


def test_model_label_cmap():
    import types

    from stego_amd.train_segmentation import LitUnsupervisedSegmenter
    for name, key in (("cityscapes", "cityscapes"), ("cocostuff27", "pascal"), ("directory", "pascal")):
        holder = types.SimpleNamespace(cfg=types.SimpleNamespace(dataset_name=name))
        cmap = LitUnsupervisedSegmenter.label_cmap.fget(holder)
        assert isinstance(cmap, np.ndarray) and np.array_equal(cmap, GOLD[key])


@pytest.mark.parametrize("cls", [UnsupervisedMetrics, DeviceUnsupervisedMetrics])
@pytest.mark.parametrize("extra", [0, 2])
def test_map_clusters_equals_the_reference(cls, extra):
    stats = GOLD["stats_extra%d" % extra]
    m = cls("t/", stats.shape[1], extra, True)
    with pytest.raises(RuntimeError):
        m.cluster_to_class()                                  # no assignment before compute()
    m.stats = torch.from_numpy(stats.copy())
    m.compute()
    vec = m.cluster_to_class()
    assert vec.dtype == np.int64 and np.array_equal(vec, GOLD["vector_extra%d" % extra])
    clusters = torch.from_numpy(GOLD["clusters_extra%d" % extra])
    mapped = m.map_clusters(clusters)
    assert mapped.dtype == torch.int64 and np.array_equal(mapped.numpy(), GOLD["mapped_extra%d" % extra])
    if extra:
        assert (vec == -1).sum() == extra


def test_cluster_to_class_without_hungarian_is_identity():
    m = UnsupervisedMetrics("t/", 5, 0, False)
    assert np.array_equal(m.cluster_to_class(), np.arange(5))
    assert np.array_equal(m.map_clusters(torch.tensor([[4, 0], [2, 2]])).numpy(), [[4, 0], [2, 2]])


@pytest.mark.parametrize("i", [0, 1])
def test_torch_image_u8_against_prep_for_plot(i):
    img = torch.from_numpy(GOLD["img%d" % i])
    want = GOLD["plot%d" % i].astype(np.float64) * 255.0
    got = render.torch_image_u8(img).numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.abs(got.astype(np.float64) - np.floor(want)).max() <= 1
    assert np.array_equal(render.image_u8(img).numpy(), got)                       # a CPU tensor takes the torch chain
    assert np.array_equal(render.torch_image_u8(img.unsqueeze(0))[0].numpy(), got)
    plain = np.clip(GOLD["plot%d_norescale" % i].astype(np.float64), 0, 1) * 255.0
    got = render.torch_image_u8(img, rescale=False).numpy()
    assert np.abs(got.astype(np.float64) - np.floor(plain)).max() <= 1


def test_torch_image_u8_constant_image_is_zero():
    assert not render.torch_image_u8(torch.full((3, 4, 5), 0.7)).any()


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.int16, torch.uint8])
def test_torch_colorize_is_numpy_indexing(dtype):
    rng = np.random.default_rng(3)
    cmap = render.cityscapes_colormap()
    lab = rng.integers(0, 28, (2, 9, 11))
    if dtype != torch.uint8:
        lab[0, 2, 3] = lab[1, 8, 10] = -1
    want = cmap[lab].astype(np.uint8)
    t = torch.from_numpy(lab).to(dtype)
    got = render.torch_colorize(t, cmap)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    assert np.array_equal(render.colorize(t, cmap).numpy(), want)                  # a CPU tensor takes the torch chain
    assert np.array_equal(render.colorize(t[0], cmap).numpy(), want[0])
    out = torch.zeros(2, 9, 11, 3, dtype=torch.uint8)
    assert render.colorize(t, cmap, out=out) is out and np.array_equal(out.numpy(), want)


def test_torch_colorize_mapping_edges_and_blend():
    cmap = render.pascal_label_colormap()
    lab = torch.tensor([[0, 0, 1], [0, 2, 2], [3, 3, 3]])
    mapping = np.array([4, -1, 7, 600])                       # a class, none, a class, outside the colormap
    got = render.torch_colorize(lab, cmap, mapping=mapping).numpy()
    want = np.stack([cmap[4], cmap[-1], cmap[7], cmap[-1]]).astype(np.uint8)[lab.numpy()]
    assert np.array_equal(got, want)
    edge = np.array([[0, 1, 1], [1, 1, 1], [0, 0, 0]], dtype=bool)           # differs from the right or the lower neighbour
    got = render.torch_colorize(lab, cmap, edges=True, edge_color=(9, 8, 7)).numpy()
    assert np.array_equal(got[edge], np.tile(np.array([9, 8, 7], np.uint8), (edge.sum(), 1)))
    assert np.array_equal(got[~edge], cmap[lab.numpy()][~edge].astype(np.uint8))
    img = torch.linspace(-2, 2, 27).reshape(3, 3, 3)
    assert np.array_equal(render.torch_colorize(lab, cmap, image=img, alpha=1.0).numpy(), cmap[lab.numpy()].astype(np.uint8))
    plain = render.torch_image_u8(img, rescale=False, mean=render.IMAGENET_MEAN, std=render.IMAGENET_STD)
    assert np.array_equal(render.torch_colorize(lab, cmap, image=img, alpha=0.0).numpy(), plain.numpy())


def test_comparison_sheet_on_the_host():
    cmap = render.cityscapes_colormap()
    lab = torch.arange(2 * 4 * 5).reshape(2, 4, 5) % 27
    img = torch.randn(2, 3, 4, 5, generator=torch.Generator().manual_seed(0))
    sheet = render.comparison_sheet([{"image": img}, {"labels": lab, "cmap": cmap}], pad=2, background=(1, 2, 3))
    assert sheet.shape == (2 + 2 * (4 + 2), 2 + 2 * (5 + 2), 3) and sheet.dtype == torch.uint8
    panels = [render.image_u8(img), render.colorize(lab, cmap)]
    mask = torch.ones(sheet.shape[:2], dtype=torch.bool)
    for r in range(2):
        for b in range(2):
            y, x = 2 + r * 6, 2 + b * 7
            assert torch.equal(sheet[y:y + 4, x:x + 5], panels[r][b])
            mask[y:y + 4, x:x + 5] = False
    assert torch.equal(sheet[mask], torch.tensor([1, 2, 3], dtype=torch.uint8).expand(int(mask.sum()), 3))
