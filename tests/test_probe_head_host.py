"""The fused probe head without a GPU: every host check of stego_probe_head (include/stego_probe.h) returns its documented code
before anything is launched, the tile plan fits its LDS budget, and the Python surface refuses CPU tensors."""
import ctypes

import pytest
import torch

from stego_amd import capi

A = 0x10000          # a 256-byte aligned stand-in address: the checks reject before any pointer is read


def _desc(**kw):
    d = dict(B=2, K=70, h=40, w=40, H=320, W=320, n_lin=27, n_clu=27, lin_kind=capi.PROBE_LOG_PROBS, clu_kind=capi.PROBE_LOG_PROBS,
             alpha=2.0)
    d.update(kw)
    return capi.probe_desc(**d)


def _map(addr=A):
    return capi.StegoMap(addr, 70 * 1600, 1600, 40, 1)


def _rc(desc, code=None, flip=None, lw=A, lb=A, cent=A, lo=A, co=A):
    return capi.probe_head_raw(desc, _map() if code is None else code, flip, lw, lb, cent, lo, co)


@pytest.mark.parametrize("kw,rc", [
    (dict(K=0), capi.PROBE_ERR_DIM), (dict(K=129), capi.PROBE_ERR_DIM),
    (dict(n_lin=0), capi.PROBE_ERR_DIM), (dict(n_lin=65), capi.PROBE_ERR_DIM),
    (dict(n_clu=0), capi.PROBE_ERR_DIM), (dict(n_clu=65), capi.PROBE_ERR_DIM),
    (dict(H=2049), capi.PROBE_ERR_SIZE), (dict(W=2049), capi.PROBE_ERR_SIZE), (dict(H=0), capi.PROBE_ERR_SIZE),
    (dict(B=0), capi.PROBE_ERR_SIZE), (dict(B=65536), capi.PROBE_ERR_SIZE), (dict(h=0), capi.PROBE_ERR_SIZE),
    (dict(w=65536), capi.PROBE_ERR_SIZE),
    (dict(lin_kind=4), capi.PROBE_ERR_OUTPUT), (dict(clu_kind=-1), capi.PROBE_ERR_OUTPUT),
    (dict(lin_kind=capi.PROBE_SKIP, clu_kind=capi.PROBE_SKIP), capi.PROBE_ERR_OUTPUT),
])
def test_descriptor_checks(kw, rc):
    assert _rc(_desc(**kw)) == rc


def test_skipped_probe_ignores_its_labels_and_pointers():
    """A skipped probe's n and pointers are not checked.  Every call here still fails a later check (a misaligned code pointer,
    STEGO_ERR_ALIGN), so nothing is launched: reaching that check shows the skipped probe passed the ones before it.  The launch
    itself with a skipped probe is tests/test_probe_head_gpu.py::test_skipped_probe_reads_nothing_of_it."""
    for n in (0, 27, 99, -1):
        assert _rc(_desc(lin_kind=capi.PROBE_SKIP, n_lin=n), code=_map(A + 2), lw=None, lb=None, lo=None) == 5
        assert _rc(_desc(clu_kind=capi.PROBE_SKIP, n_clu=n), code=_map(A + 2), cent=None, co=None) == 5
        assert capi.probe_head_plan(_desc(lin_kind=capi.PROBE_SKIP, n_lin=n))[0] > 0


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
    assert capi.load().stego_probe_head(None, ctypes.byref(_map()), None, A, A, A, A, A, None) == 1


@pytest.mark.parametrize("kind", [capi.PROBE_LOG_PROBS, capi.PROBE_PROBS, capi.PROBE_ARGMAX])
def test_null_output_for_every_probe(kind):
    assert _rc(_desc(lin_kind=kind), lo=None) == 1
    assert _rc(_desc(clu_kind=kind), co=None) == 1
    assert _rc(_desc(lin_kind=kind, clu_kind=capi.PROBE_SKIP), lo=None, co=A) == 1
    assert _rc(_desc(lin_kind=capi.PROBE_SKIP, clu_kind=kind), lo=A, co=None) == 1


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
    assert _rc(_desc(lin_kind=capi.PROBE_ARGMAX, clu_kind=capi.PROBE_ARGMAX), lo=A + 8, co=A + 4) == 5


def test_error_strings():
    lib = capi.load()
    for rc in (capi.PROBE_ERR_DIM, capi.PROBE_ERR_SIZE, capi.PROBE_ERR_OUTPUT):
        assert lib.stego_error_string(rc).decode().startswith("probe head:"), rc


@pytest.mark.parametrize("shape", [(40, 40, 320, 320), (37, 53, 291, 419), (40, 40, 24, 24), (1, 1, 2048, 2048), (2048, 2048, 7, 2048),
                                   (65535, 3, 1, 1), (3, 65535, 5, 2048), (40, 40, 1, 1)])
@pytest.mark.parametrize("K,n", [(70, 27), (128, 64), (1, 1)])
def test_plan_fits_lds(shape, K, n):
    h, w, H, W = shape
    lds, ty, tx = capi.probe_head_plan(_desc(K=K, n_lin=n, n_clu=n, h=h, w=w, H=H, W=W))
    assert 0 < lds <= 64 * 1024, lds
    assert 1 <= ty * tx <= 256 and ty <= H and tx <= W, (ty, tx)


def test_plan_at_eval_shape():
    """16 images 40^2 -> 320^2: 4 x 64 output pixels per workgroup (one per thread)."""
    lds, ty, tx = capi.probe_head_plan(_desc())
    assert (ty, tx) == (4, 64)
    assert capi.probe_head_plan(_desc(K=0))[0] == 0


def test_python_surface_refuses_cpu_tensors():
    from stego_amd import segment
    model = torch.nn.Module()
    code = torch.zeros(1, 4, 5, 5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        segment.probe_head(model, code, None, (8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        segment.segment(model, torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        segment.probe_head(model, code, None, (8, 8), linear="logits")
