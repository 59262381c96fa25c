"""Sliding-window stitching without a GPU: every host check of stego_stitch_probe and stego_window_gather (include/stego_stitch.h)
returns its documented code before anything is launched, the window layout's closed form, the plan, and the Python surface's
refusals."""
import ctypes
import os
import re

import pytest
import torch

from stego_amd import capi
from stego_amd.segment import segment_large, window_origins

A = 0x10000          # a 256-byte aligned stand-in address: the checks reject before any pointer is read
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(**kw):
    d = dict(H=101, W=77, win=48, stride=24, T=12, K=70, hc=3, wc=3, n_lin=27, n_clu=29, lin_kind=capi.PROBE_LOG_PROBS,
             clu_kind=capi.PROBE_LOG_PROBS, alpha=2.0)
    d.update(kw)
    return capi.stitch_desc(**d)


def _map(addr=A):
    return capi.StegoMap(addr, 70 * 9, 9, 3, 1)


def _rc(desc, code=None, flip=None, lw=A, lb=A, cent=A, lo=A, co=A):
    return capi.stitch_probe_raw(desc, _map() if code is None else code, flip, lw, lb, cent, lo, co)


@pytest.mark.parametrize("kw,rc", [
    (dict(K=0), capi.STITCH_ERR_DIM), (dict(K=129), capi.STITCH_ERR_DIM),
    (dict(n_lin=0), capi.STITCH_ERR_DIM), (dict(n_lin=65), capi.STITCH_ERR_DIM),
    (dict(n_clu=0), capi.STITCH_ERR_DIM), (dict(n_clu=65), capi.STITCH_ERR_DIM),
    (dict(H=32769, T=1341 * 3), capi.STITCH_ERR_SIZE), (dict(W=32769, T=4 * 1365), capi.STITCH_ERR_SIZE),
    (dict(H=0), capi.STITCH_ERR_SIZE), (dict(win=0), capi.STITCH_ERR_SIZE),
    (dict(H=4096, W=4096, win=2049, stride=2049, T=4), capi.STITCH_ERR_SIZE),
    (dict(hc=0), capi.STITCH_ERR_SIZE), (dict(wc=65536), capi.STITCH_ERR_SIZE),
    (dict(H=47), capi.STITCH_ERR_LAYOUT), (dict(W=47), capi.STITCH_ERR_LAYOUT),             # win > H, win > W
    (dict(stride=23), capi.STITCH_ERR_LAYOUT),                                              # 2 * stride < win
    (dict(stride=49), capi.STITCH_ERR_LAYOUT), (dict(stride=0), capi.STITCH_ERR_LAYOUT),    # stride > win
    (dict(T=11), capi.STITCH_ERR_WINDOWS), (dict(T=13), capi.STITCH_ERR_WINDOWS), (dict(T=0), capi.STITCH_ERR_WINDOWS),
    (dict(lin_kind=4), capi.STITCH_ERR_OUTPUT), (dict(clu_kind=-1), capi.STITCH_ERR_OUTPUT),
    (dict(lin_kind=capi.PROBE_SKIP, clu_kind=capi.PROBE_SKIP), capi.STITCH_ERR_OUTPUT),
])
def test_descriptor_checks(kw, rc):
    assert _rc(_desc(**kw)) == rc


def test_limits_are_inclusive():
    """The largest canvas, window and label counts pass every descriptor check: the call then stops at a misaligned code pointer
    (STEGO_ERR_ALIGN), so nothing is launched."""
    bad = _map(A + 2)
    assert _rc(_desc(H=32768, W=32768, win=2048, stride=1024, T=31 * 31, K=128, n_lin=64, n_clu=64), code=bad) == 5
    assert _rc(_desc(H=48, W=48, T=1, K=1, n_lin=1, n_clu=1), code=bad) == 5
    assert _rc(_desc(stride=48, T=6), code=bad) == 5


def test_skipped_probe_ignores_its_labels_and_pointers():
    for n in (0, 27, 99, -1):
        assert _rc(_desc(lin_kind=capi.PROBE_SKIP, n_lin=n), code=_map(A + 2), lw=None, lb=None, lo=None) == 5
        assert _rc(_desc(clu_kind=capi.PROBE_SKIP, n_clu=n), code=_map(A + 2), cent=None, co=None) == 5
        assert capi.stitch_probe_plan(_desc(lin_kind=capi.PROBE_SKIP, n_lin=n))[0] > 0


@pytest.mark.parametrize("which", ["code", "flip", "lw", "lb", "cent", "lo", "co"])
def test_null_pointers(which):
    kw = {}
    if which == "code":
        kw["code"] = _map(0)
    elif which == "flip":
        kw["flip"] = _map(0)
    else:
        kw[which] = None
    assert _rc(_desc(), **kw) == 1                     # STEGO_ERR_NULL
    lib = capi.load()
    assert lib.stego_stitch_probe(None, ctypes.byref(_map()), None, A, A, A, A, A, None) == 1
    assert lib.stego_stitch_probe(ctypes.byref(_desc()), None, None, A, A, A, A, A, None) == 1


@pytest.mark.parametrize("which", ["code", "flip", "lw", "lb", "cent", "lo", "co"])
def test_misaligned_pointers(which):
    kw = {}
    if which == "code":
        kw["code"] = _map(A + 2)
    elif which == "flip":
        kw["flip"] = _map(A + 2)
    else:
        kw[which] = A + 2
    assert _rc(_desc(), **kw) == 5                     # STEGO_ERR_ALIGN


def test_argmax_output_needs_8_byte_alignment():
    assert _rc(_desc(lin_kind=capi.PROBE_ARGMAX), lo=A + 4) == 5
    assert _rc(_desc(clu_kind=capi.PROBE_ARGMAX), co=A + 4) == 5


def test_error_strings_and_symbols():
    lib = capi.load()
    header = open(os.path.join(ROOT, "include", "stego_stitch.h")).read()
    for rc in range(capi.STITCH_ERR_DIM, capi.STITCH_ERR_RANGE + 1):
        assert lib.stego_error_string(rc).decode().startswith("stitch:"), rc
        assert re.search(r"STEGO_ERR_STITCH_\w+ = %d\b" % rc, header), rc
    for name in ("stego_stitch_probe", "stego_stitch_probe_plan", "stego_window_gather"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, header), name


@pytest.mark.parametrize("args,origins", [((101, 48, 24), [0, 24, 48, 53]), ((77, 48, 24), [0, 24, 29]), ((100, 48, 48), [0, 48, 52]),
                                          ((48, 48, 24), [0])])
def test_window_origins(args, origins):
    assert window_origins(*args) == origins


def test_window_origins_properties():
    """Nothing padded, nothing dropped, at most three windows over a position, the last window ends at the edge."""
    for win in (1, 2, 7, 48):
        for stride in range((win + 1) // 2, win + 1):
            for L in range(win, 4 * win + 3):
                o = window_origins(L, win, stride)
                assert len(o) == 1 + -(-(L - win) // stride) and o[0] == 0 and o[-1] == L - win
                assert all(b > a for a, b in zip(o, o[1:]))
                cover = [sum(1 for x in o if x <= p < x + win) for p in range(L)]
                assert 1 <= min(cover) and max(cover) <= 3, (L, win, stride)
    for bad in ((47, 48, 24), (100, 48, 23), (100, 48, 49), (100, 0, 0)):
        with pytest.raises(ValueError):
            window_origins(*bad)


@pytest.mark.parametrize("layout", [(101, 77, 48, 24), (100, 130, 48, 32), (100, 93, 40, 40), (100, 96, 48, 48), (48, 48, 48, 24),
                                    (4800, 4800, 320, 160), (4800, 4800, 320, 320), (32768, 32768, 2048, 1024), (7, 9, 1, 1)])
def test_plan_counts_agree_with_window_origins(layout):
    H, W, win, stride = layout
    ny, nx = len(window_origins(H, win, stride)), len(window_origins(W, win, stride))
    lds, ty, tx, pny, pnx = capi.stitch_probe_plan(_desc(H=H, W=W, win=win, stride=stride, T=ny * nx, hc=max(win // 8, 1), wc=max(win // 8, 1)))
    assert (pny, pnx) == (ny, nx)
    assert 0 < lds <= 64 * 1024 and 1 <= ty * tx <= 256 and ty <= win and tx <= win, (lds, ty, tx)


@pytest.mark.parametrize("shape", [(40, 40, 320), (37, 53, 291), (40, 40, 24), (1, 1, 2048), (2048, 2048, 7), (65535, 3, 1), (3, 65535, 5)])
@pytest.mark.parametrize("K,n", [(70, 27), (128, 64), (1, 1)])
def test_plan_fits_lds(shape, K, n):
    hc, wc, win = shape
    lds, ty, tx, _, _ = capi.stitch_probe_plan(_desc(H=win + 5, W=win, win=win, stride=(win + 1) // 2, K=K, n_lin=n, n_clu=n, hc=hc, wc=wc))
    assert 0 < lds <= 64 * 1024, lds
    assert 1 <= ty * tx <= 256 and ty <= win and tx <= win, (ty, tx)


def test_plan_of_an_invalid_descriptor_is_zero():
    assert capi.stitch_probe_plan(_desc(K=0))[0] == 0
    assert capi.stitch_probe_plan(_desc(stride=23))[0] == 0
    assert capi.stitch_probe_plan(_desc(T=5))[0] > 0          # the plan does not look at T


def _gather_rc(layout=(101, 77, 48, 24), img=None, t0=0, n=12, out=A, out_flip=None):
    return capi.window_gather_raw(capi.window_layout(*layout), capi.StegoMap(A, 0, 101 * 77, 77, 1) if img is None else img, t0, n, out,
                                  out_flip)


def test_window_gather_checks():
    assert _gather_rc(layout=(32769, 77, 48, 24)) == capi.STITCH_ERR_SIZE
    assert _gather_rc(layout=(101, 77, 2049, 2049)) == capi.STITCH_ERR_SIZE
    assert _gather_rc(layout=(101, 47, 48, 24)) == capi.STITCH_ERR_LAYOUT
    assert _gather_rc(layout=(101, 77, 48, 23)) == capi.STITCH_ERR_LAYOUT
    assert _gather_rc(layout=(101, 77, 48, 49)) == capi.STITCH_ERR_LAYOUT
    assert _gather_rc(t0=-1) == capi.STITCH_ERR_RANGE
    assert _gather_rc(n=0) == capi.STITCH_ERR_RANGE
    assert _gather_rc(t0=1, n=12) == capi.STITCH_ERR_RANGE
    assert _gather_rc(layout=(32768, 32768, 48, 24), n=65536) == capi.STITCH_ERR_RANGE
    assert _gather_rc(img=capi.StegoMap(0, 0, 1, 1, 1)) == 1
    assert _gather_rc(out=None) == 1
    assert capi.load().stego_window_gather(None, None, 0, 1, A, None, None) == 1
    assert _gather_rc(img=capi.StegoMap(A + 2, 0, 1, 1, 1)) == 5
    assert _gather_rc(out=A + 2) == 5
    assert _gather_rc(out_flip=A + 2) == 5
    assert _gather_rc(t0=5, n=7, out=A + 4, out_flip=A + 8, img=capi.StegoMap(A + 6, 0, 1, 1, 1)) == 5     # every check before the launch


def test_python_surface_refuses_cpu_tensors_and_small_images():
    model = torch.nn.Module()
    with pytest.raises(RuntimeError, match="MI355X only"):
        segment_large(model, torch.zeros(3, 60, 70), 48)
    with pytest.raises(RuntimeError, match="MI355X only"):
        segment_large(model, torch.zeros(2, 3, 60, 70), 48, run_crf=False)
    for shape in ((3, 47, 70), (3, 60, 47), (1, 3, 40, 40)):
        with pytest.raises(ValueError, match=r"segment\(\)"):
            segment_large(model, torch.zeros(*shape), 48)
    with pytest.raises(ValueError):
        segment_large(model, torch.zeros(3, 60, 70), 48, stride=23)
    with pytest.raises(ValueError):
        segment_large(model, torch.zeros(4, 60, 70), 48)
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.window_gather(torch.zeros(3, 60, 70), 48, 24, 0, 1)
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.stitch_probe(torch.zeros(1, 4, 3, 3), None, torch.zeros(3, 4), torch.zeros(3), torch.zeros(3, 4), (48, 48), 48, 24,
                          "argmax", "argmax", 2.0)
