"""The fused CRF loss without a GPU: the ctypes descriptor matches the header, every host check of stego_crf_loss
(include/stego_crf_loss.h) returns its documented code before anything is launched, the plan fits the LDS of a compute unit at the
limits, featurizers.ContrastiveCRFLoss (draw, forward) and crf_loss.torch_crf_mean_loss reproduce what the reference's module computed
(tests/golden/crf_loss_small.npz, tools/make_crf_loss_golden.py), mean_loss on CPU tensors is the torch chain, and the cases of
tests/test_crf_loss_gpu.py are as well conditioned as that module says: torch's own fp32 chain passes their check with room."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_close, load_golden
from stego_amd import capi
from test_crf_loss_gpu import CASE8_BOUND, CASES, WELL_CONDITIONED, allowance_used, chain_grad, make_inputs, reference

A = 0x10000          # a 256-byte aligned stand-in address: the checks reject before any pointer is read
BIG = 1 << 50        # a workspace size no descriptor needs
SHIPPED = dict(alpha=0.5, beta=0.15, gamma=0.05, w1=10.0, w2=3.0, shift=0.0)


def _desc(**kw):
    d = dict(B=2, K=70, G=3, h=28, w=28, hg=224, wg=224, H=56, W=56, N=1000, flags=capi.CRFLOSS_NORMALIZE, **SHIPPED)
    d.update(kw)
    return capi.crf_loss_desc(**d)


def _map(addr=A):
    return capi.StegoMap(addr, 70 * 784, 784, 28, 1)


NAMES = ("guidance", "code", "coords", "loss", "per_image", "d_code", "workspace")
MAPS = ("guidance", "code", "d_code")


def _rc(desc, workspace_bytes=BIG, **kw):
    a = dict.fromkeys(NAMES, A)
    for n in MAPS:
        a[n] = _map()
    a.update(kw)
    return capi.crf_loss_raw(desc, *[a[n] for n in NAMES], workspace_bytes)


def test_library_exports_the_three_functions_and_the_descriptor_matches_the_header():
    lib = capi.load()
    for name in ("stego_crf_loss", "stego_crf_loss_workspace_bytes", "stego_crf_loss_plan"):
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    text = open(os.path.join(ROOT, "include", "stego_crf_loss.h")).read()
    body = re.search(r"typedef struct StegoCrfLossDesc \{(.*?)\} StegoCrfLossDesc;", text, re.S).group(1)
    fields = []
    for line in body.splitlines():
        m = re.match(r"\s*(int32_t|float)\s+([^;]+);", line)
        if m:
            fields += [(n.strip(), ctypes.c_int32 if m.group(1) == "int32_t" else ctypes.c_float) for n in m.group(2).split(",")]
    assert fields == list(capi.StegoCrfLossDesc._fields_)
    assert ctypes.sizeof(capi.StegoCrfLossDesc) == 4 * len(fields) == 68
    for name, value in (("STEGO_ERR_CRFLOSS_DIM", capi.CRFLOSS_ERR_DIM), ("STEGO_ERR_CRFLOSS_POINTS", capi.CRFLOSS_ERR_POINTS),
                        ("STEGO_ERR_CRFLOSS_SIZE", capi.CRFLOSS_ERR_SIZE), ("STEGO_ERR_CRFLOSS_PARAM", capi.CRFLOSS_ERR_PARAM),
                        ("STEGO_ERR_CRFLOSS_FLAGS", capi.CRFLOSS_ERR_FLAGS), ("STEGO_CRFLOSS_NORMALIZE", capi.CRFLOSS_NORMALIZE)):
        assert re.search(r"%s = %d\b" % (name, value), text), name
    for name, value in (("MAX_K", capi.CRFLOSS_MAX_K), ("MAX_G", capi.CRFLOSS_MAX_G), ("MAX_POINTS", capi.CRFLOSS_MAX_POINTS),
                        ("MAX_SIDE", capi.CRFLOSS_MAX_SIDE), ("LAUNCHES", capi.CRFLOSS_LAUNCHES)):
        assert re.search(r"#define STEGO_CRFLOSS_%s %d\b" % (name, value), text), name


@pytest.mark.parametrize("kw,rc", [
    (dict(K=0), capi.CRFLOSS_ERR_DIM), (dict(K=129), capi.CRFLOSS_ERR_DIM), (dict(G=0), capi.CRFLOSS_ERR_DIM), (dict(G=9), capi.CRFLOSS_ERR_DIM),
    (dict(N=0), capi.CRFLOSS_ERR_POINTS), (dict(N=4097), capi.CRFLOSS_ERR_POINTS),
    (dict(B=0), capi.CRFLOSS_ERR_SIZE), (dict(B=65536), capi.CRFLOSS_ERR_SIZE),
    (dict(h=0), capi.CRFLOSS_ERR_SIZE), (dict(w=2049), capi.CRFLOSS_ERR_SIZE), (dict(hg=2049), capi.CRFLOSS_ERR_SIZE),
    (dict(wg=0), capi.CRFLOSS_ERR_SIZE), (dict(H=0), capi.CRFLOSS_ERR_SIZE), (dict(W=2049), capi.CRFLOSS_ERR_SIZE),
    (dict(alpha=0.0), capi.CRFLOSS_ERR_PARAM), (dict(beta=-1.0), capi.CRFLOSS_ERR_PARAM), (dict(gamma=float("nan")), capi.CRFLOSS_ERR_PARAM),
    (dict(alpha=float("inf")), capi.CRFLOSS_ERR_PARAM), (dict(w1=float("inf")), capi.CRFLOSS_ERR_PARAM),
    (dict(w2=float("nan")), capi.CRFLOSS_ERR_PARAM), (dict(shift=float("-inf")), capi.CRFLOSS_ERR_PARAM),
    (dict(flags=2), capi.CRFLOSS_ERR_FLAGS), (dict(flags=-1), capi.CRFLOSS_ERR_FLAGS),
])
def test_descriptor_checks(kw, rc):
    assert _rc(_desc(**kw)) == rc
    assert capi.crf_loss_workspace_bytes(_desc(**kw)) == 0
    assert capi.crf_loss_plan(_desc(**kw)) == (rc, [(0, 0)] * 3)


@pytest.mark.parametrize("which", [n for n in NAMES if n not in ("per_image", "d_code")])
def test_null_pointers(which):
    assert _rc(_desc(), **{which: None}) == 1                                                  # STEGO_ERR_NULL
    if which in MAPS:
        assert _rc(_desc(), **{which: _map(0)}) == 1


def test_null_descriptor_and_optional_outputs():
    assert capi.crf_loss_raw(None, _map(), _map(), A, A, A, _map(), A, BIG) == 1
    assert _rc(_desc(), d_code=_map(0)) == 1                                                    # a d_code without data
    # per_image and d_code may be NULL: the call goes on to a later check (a misaligned loss pointer, STEGO_ERR_ALIGN)
    assert _rc(_desc(), per_image=None, d_code=None, loss=A + 2) == 5


def test_workspace_too_small():
    n = capi.crf_loss_workspace_bytes(_desc())
    assert n > 0
    assert _rc(_desc(), workspace_bytes=n - 1) == 4                                             # STEGO_ERR_WORKSPACE
    assert _rc(_desc(), workspace_bytes=0) == 4


@pytest.mark.parametrize("which,off", [("guidance", 2), ("code", 2), ("coords", 4), ("loss", 2), ("per_image", 2), ("d_code", 2),
                                       ("workspace", 8)])
def test_misaligned_pointers(which, off):
    assert _rc(_desc(), **{which: _map(A + off) if which in MAPS else A + off}) == 5           # STEGO_ERR_ALIGN


def test_error_strings():
    lib = capi.load()
    for rc in range(80, 85):
        assert lib.stego_error_string(rc).decode().startswith("CRF loss:"), rc


@pytest.mark.parametrize("kw", [dict(), dict(B=32), dict(K=128, G=8, N=4096, B=65535, h=2048, w=2048, hg=2048, wg=2048, H=2048, W=2048),
                                dict(K=1, G=1, N=1, B=1, h=1, w=1, hg=1, wg=1, H=1, W=1), dict(K=97, N=4096), dict(K=33, N=129),
                                dict(K=64, N=2049, h=2048, w=1)])
def test_plan_fits_lds_and_the_launch_limits(kw):
    rc, launches = capi.crf_loss_plan(_desc(**kw))
    assert rc == 0 and len(launches) == 3
    for (lds, wgs), threads in zip(launches, (1024, 256, 256)):
        assert 0 < lds <= 160 * 1024 and wgs >= 1, launches
        assert wgs < 2 ** 31 and wgs * threads < 2 ** 32, launches            # a one-dimensional grid inside HIP's limits


def test_plan_and_workspace_at_the_training_shape():
    """B = 32, K = 70, N = 1000: 512 workgroups of the pairs launch, two of which fit a compute unit's LDS; about 26 MB of workspace."""
    rc, launches = capi.crf_loss_plan(_desc(B=32))
    assert rc == 0 and launches[1][1] == 32 * 16 and launches[1][0] <= 160 * 1024 // 2, launches
    assert capi.crf_loss_workspace_bytes(_desc(B=32)) <= 28 << 20
    sizes = [capi.crf_loss_workspace_bytes(_desc(B=B)) for B in (1, 2, 3, 16, 32, 65535)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes


def test_python_surface_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.crf_loss(torch.zeros(1, 3, 8, 8), torch.zeros(1, 4, 4, 4), torch.zeros(2, 5, dtype=torch.int64), (8, 8), (1, 1, 1, 1, 1, 0))


# ---- the torch side against the reference's module
def _golden():
    g = load_golden("crf_loss_small")
    return g, torch.from_numpy(g["guidance"]), torch.from_numpy(g["code"]), torch.from_numpy(g["coords"])


def test_draw_reproduces_the_points_the_reference_drew():
    from stego_amd.featurizers import ContrastiveCRFLoss
    g, guidance, code, coords = _golden()
    m = ContrastiveCRFLoss(coords.shape[1], *g["params"])
    torch.manual_seed(int(g["draw_seed"]))
    drawn = m.draw(guidance.shape[2], guidance.shape[3], torch.device("cpu"))
    assert drawn.dtype == torch.int64 and torch.equal(drawn, coords)


def test_forward_and_the_torch_chain_reproduce_the_reference_means():
    from stego_amd.crf_loss import torch_crf_mean_loss
    from stego_amd.featurizers import ContrastiveCRFLoss
    g, guidance, code, coords = _golden()
    assert guidance.dtype == torch.float64
    m = ContrastiveCRFLoss(coords.shape[1], *g["params"])
    torch.manual_seed(int(g["draw_seed"]))
    out = m(guidance, code)
    assert tuple(out.shape) == (2, coords.shape[1], coords.shape[1])
    assert abs(out.mean().item() - float(g["mean"])) <= 1e-12 * abs(float(g["mean"]))
    np.testing.assert_allclose(out.mean(dim=(1, 2)).numpy(), g["per_image"], rtol=1e-12, atol=0)
    size = tuple(guidance.shape[2:])
    loss = torch_crf_mean_loss(guidance, code, coords, size, g["params"], normalize=False)
    assert abs(loss.item() - float(g["mean"])) <= 1e-12 * abs(float(g["mean"]))
    for b in range(2):
        one = torch_crf_mean_loss(guidance[b:b + 1], code[b:b + 1], coords, size, g["params"], normalize=False)
        assert abs(one.item() - float(g["per_image"][b])) <= 1e-12 * abs(float(g["per_image"][b]))


def test_mean_loss_on_cpu_tensors_is_the_torch_chain():
    from stego_amd.crf_loss import _native_ok, crf_mean_loss, torch_crf_mean_loss
    from stego_amd.featurizers import ContrastiveCRFLoss
    g = torch.Generator().manual_seed(1)
    img, code = torch.randn(2, 3, 16, 16, generator=g), torch.randn(2, 6, 4, 4, generator=g, requires_grad=True)
    params = (0.5, 0.15, 0.05, 10.0, 3.0, 0.1)
    m = ContrastiveCRFLoss(40, *params)
    for size, normalize in ((8, True), (None, False), ((6, 5), True)):
        grid = tuple(code.shape[2:]) if size is None else (size, size) if isinstance(size, int) else size
        torch.manual_seed(3)
        coords = m.draw(grid[0], grid[1], code.device)
        assert not _native_ok(img, code, coords, grid, params)
        want = torch_crf_mean_loss(img, code, coords, grid, params, normalize)
        (dw,) = torch.autograd.grad(want, code)
        torch.manual_seed(3)
        got = m.mean_loss(img, code, size=size, normalize=normalize)
        (dg,) = torch.autograd.grad(got, code)
        assert got.dim() == 0 and torch.equal(got, want) and torch.equal(dg, dw)
        assert torch.equal(crf_mean_loss(img, code, coords, grid, params, normalize), want)
    # the composition of training_step: the module on the resized maps
    from stego_amd.modules import norm
    from stego_amd.utils import resize
    torch.manual_seed(3)
    ref = m(resize(img, 8), norm(resize(code, 8))).mean()
    torch.manual_seed(3)
    assert torch.equal(m.mean_loss(img, code, size=8, normalize=True), ref)


# ---- the conditioning of the GPU cases (tests/test_crf_loss_gpu.py): torch's fp32 chain on the CPU against the float64 reference
@pytest.mark.parametrize("case", WELL_CONDITIONED)
def test_gpu_cases_are_well_conditioned(case):
    img, code, coords = make_inputs(case)
    ref = reference(case)
    loss, per_image, d_code = chain_grad(img, code, coords, CASES[case], torch.float32)
    used = (allowance_used(loss, ref[0]), allowance_used(per_image, ref[1]), allowance_used(d_code, ref[2]))
    print("case %d: torch fp32 uses %.3f (loss) %.3f (per_image) %.3f (d_code) of the allowance" % ((case,) + used))
    assert_close(loss, ref[0], what="loss")
    assert_close(d_code, ref[2], what="d_code")
    assert max(used[0], used[2]) <= 0.25, used


def test_shipped_case_torch_fp32_on_the_uncancelled_ruler():
    """Case 8: torch's fp32 chain stays below 5e-7 * max|e_raw| - the kernel's bound, 2e-6, leaves it room over the reference."""
    img, code, coords = make_inputs(8)
    ref = reference(8)
    e_raw = chain_grad(img, code, coords, CASES[8], torch.float64, detach_norm=True)[2]
    d32 = chain_grad(img, code, coords, CASES[8], torch.float32)[2]
    fig = float(np.abs(d32 - ref[2]).max() / np.abs(e_raw).max())
    print("case 8: torch fp32 max|a - e| = %.3e * max|e_raw|; max|e_raw| / max|e| = %.1f; allowance used %.2f" % (
        fig, float(np.abs(e_raw).max() / np.abs(ref[2]).max()), allowance_used(d32, ref[2])))
    assert fig <= 5e-7 < CASE8_BOUND
