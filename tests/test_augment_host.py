"""The device-side augmentation and the fused aug-alignment loss without a GPU: the ctypes structures match include/stego_aug.h, every
host check of stego_augment / stego_aug_align returns its documented code before anything is launched, tests/aug_oracle.py agrees with
torch's own CPU operators where they exist, draw_aug_params draws the reference's distributions, the cases of tests/test_augment_gpu.py
are well conditioned (fp32 on the CPU uses at most a quarter of assert_close's allowance against float64), the torch chain is the
reference's composition (with the reference present), and the cfg.native_aug gate of my_app."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aug_oracle
from conftest import ROOT, assert_close, load_golden
from stego_amd import capi
from stego_amd.augment import (BRIGHTNESS, CONTRAST, HUE, NONE, SATURATION, crop_size, draw_aug_params, make_params, needs_torchvision,
                               params_table, torch_aug_alignment)
from test_augment_gpu import (AUG_CASES, GOLDEN_CASES, LOSS_BOUND, LOSS_CASES, allowance_used, aug_inputs, aug_reference, chain_grad,
                              loss_inputs, loss_reference)

A = 0x10000          # a 256-byte aligned stand-in address: the checks reject before any device pointer is read
BIG = 1 << 50        # a workspace size no descriptor needs
HEADER = open(os.path.join(ROOT, "include", "stego_aug.h")).read()


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    fields = []
    for line in body.splitlines():
        m = re.match(r"\s*(int32_t|float)\s+([^;]+);", line)
        if m:
            for n in m.group(2).split(","):
                arr = re.match(r"\s*(\w+)\[(\d+)\]", n)
                t = ctypes.c_int32 if m.group(1) == "int32_t" else ctypes.c_float
                fields.append((arr.group(1), t * int(arr.group(2))) if arr else (n.strip(), t))
    return fields


def test_library_exports_the_functions_and_the_structures_match_the_header():
    lib = capi.load()
    for name in ("stego_augment", "stego_augment_workspace_bytes", "stego_augment_check_params", "stego_augment_plan", "stego_aug_align",
                 "stego_aug_align_workspace_bytes", "stego_aug_align_plan"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, HEADER), name
    for cls, size in ((capi.StegoAugParams, 64), (capi.StegoAugDesc, 16), (capi.StegoAugAlignDesc, 28)):
        got = [(n, t._type_, t._length_) if hasattr(t, "_length_") else (n, t, 1) for n, t in cls._fields_]
        want = [(n, t._type_, t._length_) if hasattr(t, "_length_") else (n, t, 1) for n, t in _struct_fields(cls.__name__)]
        assert got == want, cls.__name__
        assert ctypes.sizeof(cls) == size == 4 * sum(f[2] for f in got), cls.__name__
    assert "sizeof(StegoAugParams) == 64" in HEADER
    for name, value in (("STEGO_ERR_AUG_SIZE", capi.AUG_ERR_SIZE), ("STEGO_ERR_AUG_PARAM", capi.AUG_ERR_PARAM),
                        ("STEGO_ERR_AUGALIGN_DIM", capi.AUGALIGN_ERR_DIM), ("STEGO_ERR_AUGALIGN_SIZE", capi.AUGALIGN_ERR_SIZE),
                        ("STEGO_AUG_BRIGHTNESS", BRIGHTNESS), ("STEGO_AUG_CONTRAST", CONTRAST), ("STEGO_AUG_SATURATION", SATURATION),
                        ("STEGO_AUG_HUE", HUE), ("STEGO_AUG_NONE", NONE)):
        assert re.search(r"%s = %d\b" % (name, value), HEADER), name
    for name, value in (("AUG_MAX_SIDE", capi.AUG_MAX_SIDE), ("AUG_MIN_RES", capi.AUG_MIN_RES), ("AUG_LAUNCHES", capi.AUG_LAUNCHES),
                        ("AUGALIGN_MAX_K", capi.AUGALIGN_MAX_K), ("AUGALIGN_MAX_SIDE", capi.AUGALIGN_MAX_SIDE),
                        ("AUGALIGN_LAUNCHES", capi.AUGALIGN_LAUNCHES)):
        assert re.search(r"#define STEGO_%s %d\b" % (name, value), HEADER), name
    assert lib.stego_abi_version() == 7                                  # the new symbols are additions
    for rc in (90, 91):
        assert lib.stego_error_string(rc).decode().startswith("augment:"), rc
    for rc in (92, 93):
        assert lib.stego_error_string(rc).decode().startswith("aug alignment:"), rc


# ---- stego_augment's host checks
H0, W0, R0 = 20, 28, 12


def _table(n=2, **kw):
    return params_table([make_params(H0, W0, **kw) for _ in range(n)])


def _aug_rc(desc=None, img=True, host=True, workspace_bytes=BIG, **kw):
    a = dict(params=A, img_aug=A, coord_aug=A, workspace=A)
    a.update(kw)
    desc = capi.aug_desc(2, H0, W0, R0) if desc is None else desc
    m = capi.StegoMap(A, 3 * H0 * W0, H0 * W0, W0, 1) if img is True else img
    return capi.augment_raw(desc, m, _table() if host is True else host, a["params"], a["img_aug"], a["coord_aug"], a["workspace"],
                            workspace_bytes)


@pytest.mark.parametrize("dims", [(0, 20, 28, 12), (65536, 20, 28, 12), (2, 0, 28, 12), (2, 2049, 28, 12), (2, 20, 0, 12), (2, 20, 2049, 12),
                                  (2, 20, 28, 2), (2, 20, 28, 2049)])
def test_augment_descriptor_checks(dims):
    desc = capi.aug_desc(*dims)
    assert _aug_rc(desc) == capi.AUG_ERR_SIZE
    assert capi.augment_workspace_bytes(desc) == 0
    assert capi.augment_plan(desc) == (capi.AUG_ERR_SIZE, [(0, 0)] * 2)
    assert capi.aug_check_params(desc, _table())[0] == capi.AUG_ERR_SIZE


BAD_RECORDS = [dict(flip=2), dict(flip=-1), dict(gray=2), dict(ch=0), dict(ch=H0 + 1), dict(cw=0), dict(cw=W0 + 1), dict(top=-1),
               dict(top=1), dict(top=5, ch=16), dict(left=-1), dict(left=9, cw=20), dict(order=(5, NONE, NONE, NONE)),
               dict(order=(-1, NONE, NONE, NONE)), dict(order=(CONTRAST, NONE, CONTRAST, NONE)), dict(order=(HUE, HUE, NONE, NONE)),
               dict(factors=(float("nan"), 1, 1, 0)), dict(factors=(1, float("inf"), 1, 0)), dict(factors=(-0.1, 1, 1, 0)),
               dict(factors=(1, -0.1, 1, 0)), dict(factors=(1, 1, -0.1, 0)), dict(factors=(1, 1, 1, 0.51)), dict(factors=(1, 1, 1, -0.51)),
               dict(blur_sigma=-0.5), dict(blur_sigma=float("nan")), dict(blur_sigma=float("inf"))]


@pytest.mark.parametrize("kw", BAD_RECORDS)
def test_an_invalid_record_is_refused_with_its_index(kw):
    table = params_table([make_params(H0, W0), make_params(H0, W0, **kw)])
    assert capi.aug_check_params(capi.aug_desc(2, H0, W0, R0), table) == (capi.AUG_ERR_PARAM, 1, False)
    assert _aug_rc(host=table) == capi.AUG_ERR_PARAM
    table[1].reserved, table[0].reserved = 0, 1
    assert capi.aug_check_params(capi.aug_desc(2, H0, W0, R0), table)[:2] == (capi.AUG_ERR_PARAM, 0)


def test_valid_records_and_the_contrast_flag():
    desc = capi.aug_desc(2, H0, W0, R0)
    assert capi.aug_check_params(desc, _table()) == (0, -1, False)
    assert capi.aug_check_params(desc, _table(order=(HUE, SATURATION, BRIGHTNESS, NONE), factors=(0, 0, 0, -0.5), gray=1, blur_sigma=3.0,
                                              flip=1, top=19, left=27, ch=1, cw=1)) == (0, -1, False)
    table = params_table([make_params(H0, W0), make_params(H0, W0, order=(NONE, NONE, NONE, CONTRAST))])
    assert capi.aug_check_params(desc, table) == (0, -1, True)
    assert capi.aug_check_params(desc, None)[0] == 1 and capi.aug_check_params(None, table)[0] == 1


@pytest.mark.parametrize("which", ["params", "img_aug", "coord_aug", "workspace"])
def test_augment_null_pointers(which):
    assert _aug_rc(**{which: None}) == 1                                 # STEGO_ERR_NULL


def test_augment_null_descriptor_image_and_table():
    assert capi.augment_raw(None, capi.StegoMap(A, 1, 1, 1, 1), _table(), A, A, A, A, BIG) == 1
    assert _aug_rc(img=None) == 1 and _aug_rc(img=capi.StegoMap(0, 1, 1, 1, 1)) == 1 and _aug_rc(host=None) == 1


def test_augment_workspace_and_alignment():
    n = capi.augment_workspace_bytes(capi.aug_desc(2, H0, W0, R0))
    assert n > 0
    assert _aug_rc(workspace_bytes=n - 1) == 4 and _aug_rc(workspace_bytes=0) == 4          # STEGO_ERR_WORKSPACE
    assert _aug_rc(img=capi.StegoMap(A + 2, 1, 1, 1, 1)) == 5                                # STEGO_ERR_ALIGN
    for which, off in (("params", 2), ("img_aug", 4), ("img_aug", 8), ("coord_aug", 4), ("workspace", 8)):
        assert _aug_rc(**{which: A + off}) == 5, which


@pytest.mark.parametrize("dims", [(2, 20, 28, 12), (32, 224, 224, 224), (65535, 2048, 2048, 2048), (1, 1, 1, 3), (3, 7, 2048, 33)])
def test_augment_plan_fits_lds_and_the_launch_limits(dims):
    rc, launches = capi.augment_plan(capi.aug_desc(*dims))
    assert rc == 0 and len(launches) == 2
    B, _, _, R = dims
    assert launches[0][1] == B * math.ceil(R / 8) and launches[1][1] == B * math.ceil(R / 64) * math.ceil(R / 16)
    for lds, wgs in launches:
        assert 0 < lds <= 64 * 1024 and 1 <= wgs < 2 ** 31
    assert math.ceil(R / 64) < 2 ** 16 and math.ceil(R / 16) < 2 ** 16 and B < 2 ** 16     # a three-dimensional grid inside HIP's limits
    assert capi.augment_workspace_bytes(capi.aug_desc(*dims)) >= 8 * launches[0][1]


def test_python_surface_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.augment(torch.zeros(2, 3, H0, W0), _table(), R0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.aug_align(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 3, 3), torch.zeros(1, 8, 8, 2))


# ---- stego_aug_align's host checks
def _align_desc(**kw):
    d = dict(B=2, K=70, h=28, w=28, S=28, Rh=224, Rw=224)
    d.update(kw)
    return capi.aug_align_desc(**d)


ALIGN_NAMES = ("code", "code_aug", "coord", "loss", "d_code", "d_code_aug", "workspace")
ALIGN_MAPS = ("code", "code_aug", "d_code", "d_code_aug")


def _align_rc(desc, workspace_bytes=BIG, **kw):
    a = dict.fromkeys(ALIGN_NAMES, A)
    for n in ALIGN_MAPS:
        a[n] = capi.StegoMap(A, 70 * 784, 784, 28, 1)
    a.update(kw)
    return capi.aug_align_raw(desc, *[a[n] for n in ALIGN_NAMES], workspace_bytes)


@pytest.mark.parametrize("kw,rc", [
    (dict(K=0), capi.AUGALIGN_ERR_DIM), (dict(K=129), capi.AUGALIGN_ERR_DIM),
    (dict(B=0), capi.AUGALIGN_ERR_SIZE), (dict(B=65536), capi.AUGALIGN_ERR_SIZE), (dict(h=0), capi.AUGALIGN_ERR_SIZE),
    (dict(h=257), capi.AUGALIGN_ERR_SIZE), (dict(w=0), capi.AUGALIGN_ERR_SIZE), (dict(w=257), capi.AUGALIGN_ERR_SIZE),
    (dict(S=0), capi.AUGALIGN_ERR_SIZE), (dict(S=257), capi.AUGALIGN_ERR_SIZE), (dict(Rh=0), capi.AUGALIGN_ERR_SIZE),
    (dict(Rh=2049), capi.AUGALIGN_ERR_SIZE), (dict(Rw=0), capi.AUGALIGN_ERR_SIZE), (dict(Rw=2049), capi.AUGALIGN_ERR_SIZE),
])
def test_aug_align_descriptor_checks(kw, rc):
    assert _align_rc(_align_desc(**kw)) == rc
    assert capi.aug_align_workspace_bytes(_align_desc(**kw)) == 0
    assert capi.aug_align_plan(_align_desc(**kw)) == (rc, [(0, 0)] * 2)


@pytest.mark.parametrize("which", [n for n in ALIGN_NAMES if not n.startswith("d_")])
def test_aug_align_null_pointers(which):
    assert _align_rc(_align_desc(), **{which: None}) == 1
    if which in ALIGN_MAPS:
        assert _align_rc(_align_desc(), **{which: capi.StegoMap(0, 1, 1, 1, 1)}) == 1


def test_aug_align_null_descriptor_and_optional_gradients():
    assert capi.aug_align_raw(None, capi.StegoMap(A, 1, 1, 1, 1), capi.StegoMap(A, 1, 1, 1, 1), A, A, None, None, A, BIG) == 1
    assert _align_rc(_align_desc(), d_code=capi.StegoMap(0, 1, 1, 1, 1)) == 1 and _align_rc(_align_desc(), d_code_aug=capi.StegoMap(0, 1, 1, 1, 1)) == 1
    # both gradients may be NULL: the call goes on to a later check (a misaligned loss pointer, STEGO_ERR_ALIGN)
    assert _align_rc(_align_desc(), d_code=None, d_code_aug=None, loss=A + 2) == 5


def test_aug_align_workspace_and_alignment():
    n = capi.aug_align_workspace_bytes(_align_desc())
    assert n >= 2 * 784 * (70 + 9) * 4
    assert _align_rc(_align_desc(), workspace_bytes=n - 1) == 4 and _align_rc(_align_desc(), workspace_bytes=0) == 4
    for which, off in (("code", 2), ("code_aug", 2), ("coord", 2), ("loss", 2), ("d_code", 2), ("d_code_aug", 2), ("workspace", 8)):
        bad = capi.StegoMap(A + off, 1, 1, 1, 1) if which in ALIGN_MAPS else A + off
        assert _align_rc(_align_desc(), **{which: bad}) == 5, which
    sizes = [capi.aug_align_workspace_bytes(_align_desc(B=B)) for B in (1, 2, 16, 32, 65535)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[3] <= 12 << 20, sizes


@pytest.mark.parametrize("kw", [dict(), dict(B=32), dict(B=65535, K=128, h=256, w=256, S=256, Rh=2048, Rw=2048),
                                dict(B=1, K=1, h=1, w=1, S=1, Rh=1, Rw=1), dict(B=3, K=33, h=7, w=5, S=6, Rh=48, Rw=48)])
def test_aug_align_plan_is_inside_the_launch_limits(kw):
    rc, launches = capi.aug_align_plan(_align_desc(**kw))
    d = _align_desc(**kw)
    assert rc == 0 and launches[0][1] == math.ceil(d.B * d.S * d.S / 4)
    assert launches[1][1] == min(d.B * math.ceil(d.h * d.w / 16), 1 << 18) + 1
    for lds, wgs in launches:
        assert lds <= 64 * 1024 and 1 <= wgs < 2 ** 31 and wgs * 256 < 2 ** 40


# ---- the oracle against torch's own CPU operators
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_geometry_is_flip_slice_interpolate(dtype):
    g = torch.Generator().manual_seed(1)
    img = torch.randn(3, 20, 28, generator=g).to(dtype)
    coord = aug_oracle.coord_image(20, 28, dtype)
    for name in ("geometry_12", "geometry_33"):
        _, table, R = aug_inputs(name)
        for rec in table:
            for src in (img, coord):
                want = torch.flip(src, dims=[2]) if rec.flip else src
                want = want[:, rec.top:rec.top + rec.ch, rec.left:rec.left + rec.cw]
                want = F.interpolate(want.unsqueeze(0), (R, R), mode="bilinear", align_corners=False).squeeze(0)
                got = aug_oracle.geometry(src, rec, R)
                # the weights carry the rounding of a source coordinate as large as the crop's side: eps * side, times the values' range
                assert (got - want).abs().max().item() <= 8 * torch.finfo(dtype).eps * max(rec.ch, rec.cw) * max(1.0, src.abs().max().item())


def test_oracle_blur_is_reflect_pad_and_conv2d():
    x = torch.rand(3, 17, 17, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    for sigma in (0.1, 0.7, 2.0):
        k = aug_oracle.blur_weights(sigma, torch.float64)
        assert abs(k.sum().item() - 1) < 1e-15 and torch.equal(k, k.flip(0))
        k2 = (k[:, None] * k[None, :]).expand(3, 1, 5, 5)
        want = F.conv2d(F.pad(x.unsqueeze(0), (2, 2, 2, 2), mode="reflect"), k2, groups=3).squeeze(0)
        assert (aug_oracle.blur(x, sigma) - want).abs().max().item() < 1e-14
    padded = F.pad(torch.arange(7.0).view(1, 1, 1, 7), (2, 2, 0, 0), mode="reflect").flatten().tolist()
    assert padded == [2, 1, 0, 1, 2, 3, 4, 5, 6, 5, 4]                   # -1 -> 1, -2 -> 2, R -> R - 2, R + 1 -> R - 3


def test_oracle_identity_and_the_operators_by_hand():
    sq = torch.rand(1, 3, 9, 9, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    out, coord = aug_oracle.augment(sq, [make_params(9, 9)], 9)
    assert torch.equal(out, sq) and torch.equal(coord[0], aug_oracle.coord_image(9, 9, torch.float64).permute(1, 2, 0))
    assert coord[0, 0, 0].tolist() == [-1, -1] and coord[0, 8, 0].tolist() == [1, -1]       # channel 0 is the row ramp
    x = torch.tensor([0.2, 0.6, 0.4], dtype=torch.float64).view(3, 1, 1)
    gray = 0.2989 * 0.2 + 0.587 * 0.6 + 0.114 * 0.4
    assert aug_oracle.photometric(x, make_params(1, 1, order=(BRIGHTNESS, NONE, NONE, NONE), factors=(1.5, 1, 1, 0))).flatten().tolist() == \
        pytest.approx([0.3, 0.9, 0.6])
    assert aug_oracle.photometric(x, make_params(1, 1, order=(SATURATION, NONE, NONE, NONE), factors=(1, 1, 0.0, 0))).flatten().tolist() == \
        pytest.approx([gray] * 3)
    assert aug_oracle.photometric(x, make_params(1, 1, order=(CONTRAST, NONE, NONE, NONE), factors=(1, 0.0, 1, 0))).flatten().tolist() == \
        pytest.approx([gray] * 3)
    assert aug_oracle.photometric(x, make_params(1, 1, gray=1)).flatten().tolist() == pytest.approx([gray] * 3)
    # hue: a shift of a third of the circle rotates the channels; a zero shift returns the pixel; a gray pixel stays
    assert aug_oracle.hue(x, 1.0 / 3.0).flatten().tolist() == pytest.approx([0.4, 0.2, 0.6])
    assert aug_oracle.hue(x, 0.0).flatten().tolist() == pytest.approx([0.2, 0.6, 0.4])
    assert aug_oracle.hue(torch.full((3, 1, 1), 0.3, dtype=torch.float64), 0.2).flatten().tolist() == pytest.approx([0.3] * 3)
    # contrast takes the mean as it is after the operators before it
    two = torch.tensor([[0.2, 0.8]], dtype=torch.float64).expand(3, 1, 2).reshape(3, 1, 2)
    got = aug_oracle.photometric(two, make_params(1, 2, order=(BRIGHTNESS, CONTRAST, NONE, NONE), factors=(0.5, 0.0, 1, 0)))
    assert got.flatten().tolist() == pytest.approx([0.9999 * 0.25] * 6)


# ---- the draws
def test_crop_size_by_hand():
    assert crop_size(10, 10, [0.85], [1.0]) == (9, 9, 0)                 # sqrt(85) = 9.22
    assert crop_size(5, 5, [0.25], [1.0]) == (2, 2, 0)                   # sqrt(6.25) = 2.5 -> 2: half to even, not 3
    assert crop_size(7, 7, [0.25], [1.0]) == (4, 4, 0)                   # sqrt(12.25) = 3.5 -> 4
    assert crop_size(10, 20, [0.9], [2.0]) == (9, 19, 0)                 # w = round(sqrt(360)) = 19, h = round(sqrt(90)) = 9
    assert crop_size(10, 12, [1.0, 0.9], [4.0 / 3.0, 1.0]) == (10, 10, 1)   # the first try is 13 wide: too wide; sqrt(108) = 10.39
    # a 10 x 100 image: every try is more than 10 rows high -> the centred fallback with the aspect clamped to 4 / 3
    fracs, aspects = [0.8 + 0.02 * i for i in range(10)], [0.75 + 0.05 * i for i in range(10)]
    assert crop_size(10, 100, fracs, aspects) == (10, 13, None)
    assert crop_size(100, 10, fracs, aspects) == (13, 10, None)
    assert crop_size(9, 9, [2.0] * 10, [1.0] * 10) == (9, 9, None)       # inside the aspect range: the whole image


def test_draws_reproduce_from_a_seed_and_pass_the_host_check():
    a = draw_aug_params(64, 40, 56, 32, torch.Generator().manual_seed(3))
    b = draw_aug_params(64, 40, 56, 32, torch.Generator().manual_seed(3))
    c = draw_aug_params(64, 40, 56, 32, torch.Generator().manual_seed(4))
    assert bytes(a) == bytes(b) != bytes(c)
    assert capi.aug_check_params(capi.aug_desc(64, 40, 56, 32), a)[:2] == (0, -1)
    with pytest.raises(ValueError, match="CPU torch.Generator"):
        draw_aug_params(1, 8, 8, 8, None)
    with pytest.raises(ValueError, match="error 90"):
        draw_aug_params(1, 8, 8, 2, torch.Generator().manual_seed(0))


def test_draws_follow_the_reference_distributions():
    n, H, W = 2000, 64, 48
    recs = draw_aug_params(n, H, W, 32, torch.Generator().manual_seed(7))
    f = np.array([list(r.factor) for r in recs])
    assert (f[:, :3] >= 0.7).all() and (f[:, :3] <= 1.3).all() and (np.abs(f[:, 3]) <= 0.1 + 1e-7).all()
    assert np.abs(f[:, :3].mean(0) - 1.0).max() < 0.02 and abs(f[:, 3].mean()) < 0.01 and f[:, :3].min() < 0.72 and f[:, :3].max() > 1.28
    assert all(sorted(r.order) == [0, 1, 2, 3] for r in recs)
    first = np.bincount([r.order[0] for r in recs], minlength=4) / n
    assert np.abs(first - 0.25).max() < 0.04                             # 4 sigma of a fair four-way draw is 0.039
    for got, p in ((np.mean([r.flip for r in recs]), 0.5), (np.mean([r.gray for r in recs]), 0.2),
                   (np.mean([r.blur_sigma > 0 for r in recs]), 0.5)):
        assert abs(got - p) < 4 * math.sqrt(p * (1 - p) / n), (got, p)
    sig = np.array([r.blur_sigma for r in recs if r.blur_sigma > 0])
    assert sig.min() >= 0.1 - 1e-7 and sig.max() <= 2.0 and sig.min() < 0.15 and sig.max() > 1.95
    area = np.array([r.ch * r.cw for r in recs]) / float(H * W)
    ratio = np.array([r.cw / r.ch for r in recs])
    assert area.min() > 0.77 and area.max() <= 1.0 and abs(area.mean() - 0.9) < 0.02      # rounding moves a side by half a pixel
    assert ratio.min() > 0.72 and ratio.max() < 1.39
    assert all(0 <= r.top <= H - r.ch and 0 <= r.left <= W - r.cw for r in recs)
    assert len({(r.top, r.left) for r in recs}) > 20


# ---- the conditioning of the GPU cases: fp32 on the CPU against the float64 reference
@pytest.mark.parametrize("name", sorted(AUG_CASES))
def test_gpu_augment_cases_are_well_conditioned(name):
    img, table, R = aug_inputs(name)
    ref = aug_reference(name)
    out32 = [t.numpy() for t in aug_oracle.augment(img, table, R, torch.float32)]
    used = [allowance_used(out32[0], ref[0]), allowance_used(out32[1], ref[1])]
    used += [max(allowance_used(out32[i][b], ref[i][b]) for b in range(len(table))) for i in (0, 1)]
    print("%s: fp32 uses %.4f (img_aug) %.4f (coord_aug) of the allowance; per image %.4f %.4f" % ((name,) + tuple(used)))
    assert max(used) <= 0.25, used


@pytest.mark.parametrize("case", sorted(LOSS_CASES))
def test_gpu_loss_cases_are_well_conditioned(case):
    ref = loss_reference(case)
    loss, d_code, d_code_aug, _ = chain_grad(*loss_inputs(case), torch.float32)
    used = (abs(loss - ref[0]) / (LOSS_BOUND * ref[3]), allowance_used(d_code, ref[1]), allowance_used(d_code_aug, ref[2]))
    print("case %d: torch fp32 uses %.4f (loss) %.4f (d_code) %.4f (d_code_aug) of the allowance" % ((case,) + used))
    assert max(used) <= 0.25, used


# ---- the torch chain and the golden file
def test_torch_chain_has_the_swapped_indices_and_the_flip_quirk():
    """With the coordinate image of the identity the sampled code is the code itself (channel 0, the row ramp, is read as x, and the
    permute of modules.sample swaps it back); the coordinate image of a horizontally flipped view looks the code up vertically flipped."""
    g = torch.Generator().manual_seed(1)
    code = torch.randn(2, 5, 6, 6, generator=g, dtype=torch.float64)
    ident = aug_oracle.coord_image(6, 6, torch.float64).permute(1, 2, 0).expand(2, -1, -1, -1)
    n = F.normalize(code, dim=1, eps=1e-10)
    assert abs(torch_aug_alignment(code, code, ident).item() + 1.0) < 1e-12
    flipped = aug_oracle.augment(torch.zeros(2, 3, 6, 6), [make_params(6, 6, flip=1)] * 2, 6)[1]
    assert abs(torch_aug_alignment(code, torch.flip(code, dims=[2]), flipped).item() + 1.0) < 1e-12
    assert torch_aug_alignment(code, torch.flip(code, dims=[3]), flipped).item() > -0.9
    assert n.shape == code.shape


def test_golden_file_holds_the_gpu_cases():
    g = load_golden("aug_align_small")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "aug_align_small.npz")) < 200 << 10
    for case in GOLDEN_CASES:
        p = "c%d_" % case
        ref = loss_reference(case)
        for a, e in zip((g[p + "code"], g[p + "code_aug"], g[p + "coord"]), loss_inputs(case)):
            assert a.dtype == np.float32 and np.array_equal(a, e.numpy())
        assert abs(float(g[p + "loss"]) - ref[0]) <= 1e-12 and abs(float(g[p + "scale"]) - ref[3]) <= 1e-12
        np.testing.assert_allclose(g[p + "d_code"], ref[1], rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(g[p + "d_code_aug"], ref[2], rtol=1e-9, atol=1e-15)


def test_with_the_reference_the_chain_is_its_composition_and_the_golden_regenerates():
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("the reference is not present")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_aug_golden
    R = ref_shim.load_reference_modules()
    for case in sorted(LOSS_CASES):
        code, code_aug, coord = (t.double() for t in loss_inputs(case))
        want, _ = make_aug_golden.reference_term(R, code, code_aug, coord)
        assert torch.equal(torch_aug_alignment(code, code_aug, coord), want)
    g, again = load_golden("aug_align_small"), make_aug_golden.golden_arrays(R)
    assert sorted(g) == sorted(again)
    for k in g:
        assert np.array_equal(g[k], again[k]), k


# ---- the gate
def test_native_aug_gate(tmp_path):
    from stego_amd.train_segmentation import load_config, my_app
    assert load_config().native_aug is False
    off = load_config(overrides=["aug_alignment_weight=0.5"])
    assert "aug_alignment_weight" in needs_torchvision(off) and "native_aug" in needs_torchvision(off)
    assert needs_torchvision(load_config(overrides=["aug_alignment_weight=0.5", "native_aug=True"])) is None
    assert needs_torchvision(load_config()) is None and needs_torchvision(load_config(overrides=["native_aug=True"])) is None
    from stego_amd.data import crop_dir
    cfg = load_config(overrides=["pytorch_data_dir=%s" % tmp_path, "aug_alignment_weight=0.5", "output_root=%s" % tmp_path])
    os.makedirs(os.path.join(crop_dir(str(tmp_path), cfg.dataset_name, cfg.crop_type, cfg.crop_ratio), "img", "train"))
    with pytest.raises(ValueError, match="native_aug"):
        my_app(cfg)


def test_cpu_tensors_take_the_torch_chain():
    from stego_amd.augment import _native_ok, aug_alignment_loss
    code, code_aug, coord = loss_inputs(4)
    code.requires_grad_(True)
    assert not _native_ok(code, code_aug, coord)
    got, want = aug_alignment_loss(code, code_aug, coord), torch_aug_alignment(code, code_aug, coord)
    assert torch.equal(got, want) and torch.equal(torch.autograd.grad(got, code)[0], torch.autograd.grad(want, code)[0])
