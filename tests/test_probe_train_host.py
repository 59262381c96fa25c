"""The fused probe training call without a GPU: the library exports its three functions, every host check of stego_probe_train
(include/stego_probe_train.h) returns its documented code before anything is launched, the plan fits the LDS of a compute unit, the
workspace grows with the batch, and probe_losses on CPU tensors is the torch chain of training_step bit for bit."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from stego_amd import capi

A = 0x10000          # a 256-byte aligned stand-in address: the checks reject before any pointer is read
BIG = 1 << 40        # a workspace size no descriptor needs


def _desc(**kw):
    d = dict(B=2, K=70, h=28, w=28, H=224, W=224, n_lin=27, n_clu=27)
    d.update(kw)
    return capi.probe_train_desc(**d)


def _map(addr=A):
    return capi.StegoMap(addr, 70 * 784, 784, 28, 1)


NAMES = ("code", "label", "lin_w", "lin_b", "clusters", "losses", "n_valid", "d_lin_w", "d_lin_b", "d_clusters", "workspace")


def _rc(desc, workspace_bytes=BIG, **kw):
    a = dict.fromkeys(NAMES, A)
    a["code"] = _map()
    a.update(kw)
    return capi.probe_train_raw(desc, *[a[n] for n in NAMES], workspace_bytes)


def test_library_exports_the_three_functions():
    lib = capi.load()
    for name in ("stego_probe_train", "stego_probe_train_workspace_bytes", "stego_probe_train_plan"):
        assert hasattr(lib, name) and name in capi.SIGNATURES, name
    assert lib.stego_abi_version() == 7


@pytest.mark.parametrize("kw,rc", [
    (dict(K=0), capi.PTRAIN_ERR_DIM), (dict(K=129), capi.PTRAIN_ERR_DIM),
    (dict(n_lin=65), capi.PTRAIN_ERR_DIM), (dict(n_lin=-1), capi.PTRAIN_ERR_DIM),
    (dict(n_clu=65), capi.PTRAIN_ERR_DIM), (dict(n_clu=-1), capi.PTRAIN_ERR_DIM),
    (dict(H=2049), capi.PTRAIN_ERR_SIZE), (dict(W=2049), capi.PTRAIN_ERR_SIZE), (dict(H=0), capi.PTRAIN_ERR_SIZE),
    (dict(W=0), capi.PTRAIN_ERR_SIZE), (dict(B=0), capi.PTRAIN_ERR_SIZE), (dict(B=65536), capi.PTRAIN_ERR_SIZE),
    (dict(h=0), capi.PTRAIN_ERR_SIZE), (dict(w=65536), capi.PTRAIN_ERR_SIZE),
    (dict(n_lin=0, n_clu=0), capi.PTRAIN_ERR_PROBES),
])
def test_descriptor_checks(kw, rc):
    assert _rc(_desc(**kw)) == rc
    assert capi.probe_train_plan(_desc(**kw))[0] == 0
    assert capi.probe_train_workspace_bytes(_desc(**kw)) == 0


@pytest.mark.parametrize("which", NAMES)
def test_null_pointers(which):
    assert _rc(_desc(), **{which: _map(0) if which == "code" else None}) == 1                  # STEGO_ERR_NULL
    assert capi.load().stego_probe_train(None, ctypes.byref(_map()), *([A] * 11), BIG, None) == 1


def test_skipped_probe_needs_none_of_its_pointers():
    """The call still fails a later check (a misaligned code pointer, STEGO_ERR_ALIGN), so nothing is launched: reaching that check
    shows the skipped probe's NULL pointers passed the ones before it."""
    assert _rc(_desc(n_lin=0), code=_map(A + 2), label=None, lin_w=None, lin_b=None, d_lin_w=None, d_lin_b=None) == 5
    assert _rc(_desc(n_clu=0), code=_map(A + 2), clusters=None, d_clusters=None) == 5
    assert _rc(_desc(n_clu=0), clusters=None, d_clusters=None, d_lin_w=None) == 1


def test_workspace_too_small():
    n = capi.probe_train_workspace_bytes(_desc())
    assert n > 0
    assert _rc(_desc(), workspace_bytes=n - 1) == 4                                             # STEGO_ERR_WORKSPACE
    assert _rc(_desc(), workspace_bytes=0) == 4


@pytest.mark.parametrize("which,off", [("code", 2), ("label", 4), ("lin_w", 2), ("lin_b", 2), ("clusters", 2), ("losses", 2),
                                       ("n_valid", 4), ("d_lin_w", 2), ("d_lin_b", 2), ("d_clusters", 2), ("workspace", 4)])
def test_misaligned_pointers(which, off):
    assert _rc(_desc(), **{which: _map(A + off) if which == "code" else A + off}) == 5         # STEGO_ERR_ALIGN


def test_error_strings():
    lib = capi.load()
    for rc in (capi.PTRAIN_ERR_DIM, capi.PTRAIN_ERR_SIZE, capi.PTRAIN_ERR_PROBES):
        assert lib.stego_error_string(rc).decode().startswith("probe training:"), rc


@pytest.mark.parametrize("shape", [(28, 28, 224, 224), (40, 40, 320, 320), (5, 7, 37, 53), (12, 12, 8, 8), (1, 1, 2048, 2048),
                                   (2048, 2048, 7, 2048), (65535, 3, 1, 1), (3, 65535, 5, 2048), (65535, 65535, 2048, 2048),
                                   (1, 600, 1, 4), (2, 65535, 2, 3)])
@pytest.mark.parametrize("K,n_lin,n_clu", [(70, 27, 27), (128, 64, 64), (1, 1, 1), (128, 64, 0), (128, 0, 64), (33, 5, 7)])
def test_plan_fits_lds(shape, K, n_lin, n_clu):
    h, w, H, W = shape
    lds, wgs = capi.probe_train_plan(_desc(K=K, n_lin=n_lin, n_clu=n_clu, h=h, w=w, H=H, W=W))
    assert 0 < lds <= 160 * 1024, lds
    assert 1 <= wgs <= 768 + 256, wgs


def test_plan_at_the_training_shape():
    """32 images 28^2 -> 224^2, K = 70, 27 + 27 labels: three workgroups fit the 160 KiB of a compute unit."""
    lds, wgs = capi.probe_train_plan(_desc(B=32))
    assert lds <= 160 * 1024 // 3 and wgs == 768 + 256, (lds, wgs)


def test_workspace_is_monotone_in_the_batch():
    sizes = [capi.probe_train_workspace_bytes(_desc(B=B)) for B in (1, 2, 3, 4, 8, 16, 32, 64, 1024, 65535)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[0] < sizes[2], sizes
    small = [capi.probe_train_workspace_bytes(_desc(B=B, h=4, w=4, H=16, W=16)) for B in (1, 2, 3, 4, 5)]
    assert all(a < b for a, b in zip(small, small[1:])), small


def test_python_surface_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="MI355X only"):
        capi.probe_train(torch.zeros(1, 4, 5, 5), torch.zeros(1, 8, 8, dtype=torch.int64), torch.zeros(3, 4), torch.zeros(3), torch.zeros(3, 4))


def test_probe_losses_on_cpu_tensors_is_the_torch_chain_bitwise():
    """The fallback: losses and .grad equal what training_step's lines compute, bit for bit."""
    from stego_amd.featurizers import ClusterLookup
    from stego_amd.probe_train import probe_losses
    g = torch.Generator().manual_seed(3)
    code = torch.randn(2, 6, 4, 5, generator=g, requires_grad=True)
    label = torch.randint(-1, 8, (2, 16, 20), generator=g)
    torch.manual_seed(0)
    lin, clu = torch.nn.Conv2d(6, 7, (1, 1)), ClusterLookup(6, 9)

    def grads():
        out = [p.grad.clone() for p in (lin.weight, lin.bias, clu.clusters)]
        for p in (lin.weight, lin.bias, clu.clusters):
            p.grad = None
        return out

    # training_step's lines, written out
    detached_code = torch.clone(code.detach())
    logits = F.interpolate(lin(detached_code), label.shape[-2:], mode='bilinear', align_corners=False)
    valid = (label >= 0) & (label < 7)
    l0 = F.cross_entropy(logits, torch.where(valid, label, torch.full_like(label, -100)), ignore_index=-100)
    c0, _ = clu(detached_code, None)
    (l0 + c0).backward()
    want = grads()

    l1, c1 = probe_losses(code, label, lin, clu)
    assert l1.dim() == 0 and c1.dim() == 0
    (l1 + c1).backward()
    got = grads()
    assert torch.equal(l0, l1) and torch.equal(c0, c1) and code.grad is None
    for a, e in zip(got, want):
        assert torch.equal(a, e)
