"""CPU tests of the host layer (stego_amd/modules.py): RNG draw order, argument packing,
autograd wiring - using an oracle-backed double for the C-ABI backend - plus the C-ABI
library's load/export/error behaviour (no compute without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import oracle_backend
from conftest import ROOT, GoldenCase, assert_close, load_golden
from oracle import corr_oracle as O
from stego_amd import capi
from stego_amd import modules as M


@pytest.fixture
def oracle_backed(monkeypatch):
    monkeypatch.setattr(M, "_backend", oracle_backend)
    oracle_backend.calls.clear()
    return oracle_backend


def _cfg(**kw):
    c = O.CorrCfg()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_rng_draw_order_matches_reference_forward(oracle_backed):
    """Same seed on the same generator => same coords1, coords2, perm x3 as the reference's
    forward() (modules.py:366,367,383): outputs must equal the golden reference forward."""
    g = load_golden("seeded_e2e")
    cfg = _cfg(feature_samples=5, neg_samples=3)
    f, fp, c, cp = (torch.from_numpy(g[k]) for k in ("in_feats", "in_feats_pos", "in_code", "in_code_pos"))
    torch.manual_seed(123)
    out = M.ContrastiveCorrelationLoss(cfg)(f, fp, None, None, c, cp)
    names = ("pos_intra_loss", "pos_intra_cd", "pos_inter_loss", "pos_inter_cd", "neg_inter_loss", "neg_inter_cd")
    for name, o in zip(names, out):
        assert tuple(o.shape) == tuple(g[name].shape), name
        assert_close(o.numpy(), g[name], rtol=1e-4, what=name)
    # and the draws themselves
    torch.manual_seed(123)
    loss = M.ContrastiveCorrelationLoss(cfg)
    c1, c2 = loss.draw_coords(f, None, None)
    perms = torch.stack([M.super_perm(4, f.device) for _ in range(3)])
    np.testing.assert_array_equal(c1.numpy(), g["coords1"])
    np.testing.assert_array_equal(c2.numpy(), g["coords2"])
    np.testing.assert_array_equal(perms.numpy(), g["perms"])


def test_super_perm_known_answer():
    torch.manual_seed(1)
    rp = torch.randperm(8)
    torch.manual_seed(1)
    sp = M.super_perm(8, torch.device("cpu"))
    assert np.array_equal(O.super_perm_from_randperm(rp.numpy()), sp.numpy())
    assert not (sp == torch.arange(8)).any()


def test_autograd_wiring_train_weights(oracle_backed):
    c = GoldenCase("small_default")
    t = {k: torch.from_numpy(v) for k, v in c.inputs.items()}
    code = t["code"].clone().requires_grad_(True)
    code_pos = t["code_pos"].clone().requires_grad_(True)
    out = M.ContrastiveCorrelationLoss(c.cfg).forward_explicit(
        t["feats"], t["feats_pos"], code, code_pos, t["coords1"], t["coords2"], torch.from_numpy(c.perms))
    assert out[0].dim() == 0 and out[2].dim() == 0
    (0.67 * out[0] + 0.25 * out[2] + 0.63 * out[4].mean()).backward()
    assert oracle_backend.calls == ["corr_fwd", "corr_bwd"]
    assert_close(code.grad.numpy(), c.g["d_code_train"], rtol=1e-3, atol_frac=1e-3, what="d_code")
    assert_close(code_pos.grad.numpy(), c.g["d_code_pos_train"], rtol=1e-3, atol_frac=1e-3, what="d_code_pos")


def test_negative_loss_mean_comes_from_the_kernel(oracle_backed):
    """forward() hands the negative loss back as a tensor whose .mean() - all the reference's training step takes from it - is the
    scalar the forward launch computed, with a one-scalar upstream in the backward; any other use is the plain tensor's."""
    c = GoldenCase("small_default")
    t = {k: torch.from_numpy(v) for k, v in c.inputs.items()}

    def run(use):
        code = t["code"].clone().requires_grad_(True)
        code_pos = t["code_pos"].clone().requires_grad_(True)
        out = M.ContrastiveCorrelationLoss(c.cfg).forward_explicit(
            t["feats"], t["feats_pos"], code, code_pos, t["coords1"], t["coords2"], torch.from_numpy(c.perms))
        oracle_backend.last_neg_is_mean = None
        (0.67 * out[0] + 0.25 * out[2] + 0.63 * use(out[4])).backward()
        return out, code.grad.numpy(), code_pos.grad.numpy()

    out, g1, gp1 = run(lambda x: x.mean())                               # answered by the kernel's scalar
    assert oracle_backend.last_neg_is_mean is True
    _, g2, gp2 = run(lambda x: x.sum() / x.numel())                      # the plain tensor path (dense upstream)
    assert oracle_backend.last_neg_is_mean is False
    _, g3, gp3 = run(lambda x: 0.5 * x.mean() + 0.5 * torch.mean(torch.Tensor.as_subclass(x, torch.Tensor)))     # both at once
    for g, gp in ((g2, gp2), (g3, gp3)):
        assert_close(g1, g, rtol=1e-4, atol_frac=1e-5, what="d_code")
        assert_close(gp1, gp, rtol=1e-4, atol_frac=1e-5, what="d_code_pos")
    assert_close(g1, c.g["d_code_train"], rtol=1e-3, atol_frac=1e-3, what="d_code")
    x = out[4]
    assert isinstance(x, torch.Tensor) and x.mean().dim() == 0
    np.testing.assert_allclose(float(x.mean()), float(x.detach().numpy().mean()), rtol=1e-5)
    assert type(x + 1) is torch.Tensor and type(x.detach()) is torch.Tensor and type(x.reshape(-1)[:5]) is torch.Tensor
    # identity conversions (what a reader of the reference may put in front of .mean()) keep the shortcut: same scalar, mean upstream
    for conv in (lambda y: y.float(), lambda y: y.contiguous(), lambda y: y.reshape(-1), lambda y: y.view(-1), lambda y: y.flatten(),
                 lambda y: y.to(torch.float32)):
        _, gc, gpc = run(lambda y: conv(y).mean())
        assert oracle_backend.last_neg_is_mean is True
        np.testing.assert_array_equal(gc, g1)
        np.testing.assert_array_equal(gpc, gp1)
    assert type(x.double()) is torch.Tensor and x.double().mean().dtype == torch.float64        # (a real conversion: the plain tensor)
    assert type(torch.cat([x, x])) is torch.Tensor and x.mean(dim=0).shape == x.shape[1:]
    assert x.numel() == c.g["neg_inter_loss"].size


def test_autograd_wiring_general_upstream(oracle_backed):
    c = GoldenCase("small_stab")
    g = c.g
    t = {k: torch.from_numpy(v) for k, v in c.inputs.items()}
    code = t["code"].clone().requires_grad_(True)
    code_pos = t["code_pos"].clone().requires_grad_(True)
    out = M.ContrastiveCorrelationLoss(c.cfg).forward_explicit(
        t["feats"], t["feats_pos"], code, code_pos, t["coords1"], t["coords2"], torch.from_numpy(c.perms))
    u = {k: torch.from_numpy(g[k]) for k in ("u_neg_loss", "u_intra_cd", "u_inter_cd", "u_neg_cd")}
    total = 1.3 * out[0] - 0.7 * out[2] + (out[4].reshape(-1) * u["u_neg_loss"]).sum() + \
        (out[1].reshape(-1) * u["u_intra_cd"]).sum() + (out[3].reshape(-1) * u["u_inter_cd"]).sum() + \
        (out[5].reshape(-1) * u["u_neg_cd"]).sum()
    total.backward()
    assert_close(code.grad.numpy(), g["d_code_gen"], rtol=1e-3, atol_frac=1e-3, what="d_code_gen")
    assert_close(code_pos.grad.numpy(), g["d_code_pos_gen"], rtol=1e-3, atol_frac=1e-3, what="d_code_pos_gen")


def test_no_grad_inputs_skip_saved_state(oracle_backed):
    c = GoldenCase("small_noneg")
    t = {k: torch.from_numpy(v) for k, v in c.inputs.items()}
    out = M.ContrastiveCorrelationLoss(c.cfg).forward_explicit(
        t["feats"], t["feats_pos"], t["code"], t["code_pos"], t["coords1"], t["coords2"], None)
    assert not out[0].requires_grad
    assert tuple(out[4].shape) == (0, c.S, c.S, c.S, c.S)
    assert_close(out[0].numpy(), c.g["pos_intra_loss"], rtol=1e-3, atol_frac=1e-2)


def test_helper_wiring(oracle_backed):
    rng = np.random.default_rng(0)
    f1 = torch.from_numpy(rng.standard_normal((2, 6, 3, 4)).astype(np.float32))
    f2 = torch.from_numpy(rng.standard_normal((2, 6, 3, 4)).astype(np.float32))
    c1 = torch.from_numpy(rng.standard_normal((2, 5, 3, 4)).astype(np.float32)).requires_grad_(True)
    c2 = torch.from_numpy(rng.standard_normal((2, 5, 3, 4)).astype(np.float32)).requires_grad_(True)
    cfg = _cfg()
    loss, cd = M.ContrastiveCorrelationLoss(cfg).helper(f1, f2, c1, c2, 0.3)
    el, ecd, _ = O.helper(f1.numpy().astype(np.float64), f2.numpy().astype(np.float64),
                          c1.detach().numpy().astype(np.float64), c2.detach().numpy().astype(np.float64), 0.3, cfg)
    assert tuple(loss.shape) == (2, 3, 4, 3, 4)
    assert_close(loss.detach().numpy(), el, rtol=1e-4)
    assert_close(cd.detach().numpy(), ecd, rtol=1e-4)
    loss.mean().backward()
    assert c1.grad is not None and c2.grad is not None and torch.isfinite(c1.grad).all()


def test_real_backend_refuses_cpu_tensors():
    """No CPU fallback: the product path must fail loudly off-device."""
    cfg = _cfg(feature_samples=3, neg_samples=1)
    f = torch.randn(2, 8, 5, 5)
    c = torch.randn(2, 4, 5, 5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        M.ContrastiveCorrelationLoss(cfg)(f, f, None, None, c, c)
    with pytest.raises(RuntimeError, match="MI355X only"):
        M.ContrastiveCorrelationLoss(cfg).helper(f[:, :, :3, :3], f[:, :, :3, :3], c[:, :, :3, :3], c[:, :, :3, :3], .1)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(capi, "_lib", None)
    monkeypatch.setattr(capi._build, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="not built"):
        capi.load()


# ------------------------------------------------------------------ C ABI (no compute)
def _header_functions():
    names = set()
    inc = os.path.join(ROOT, "include")
    for h in sorted(os.listdir(inc)):
        if h.endswith(".h"):
            src = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, h)).read(), flags=re.S)
            names |= set(re.findall(r"\b(stego_[a-z_0-9]+)\s*\(", src))
    return sorted(names)


def test_library_exports_every_declared_symbol():
    lib = capi.load()
    names = _header_functions()
    assert "stego_corr_fwd" in names and "stego_corr_bwd" in names and "stego_vit_forward" in names
    for n in names:
        assert hasattr(lib, n), "libstego_corr.so does not export %s" % n
        assert n in capi.SIGNATURES, "capi.py has no signature for %s" % n
    assert lib.stego_abi_version() == 7


def test_library_validates_before_enqueueing():
    """Argument errors are detected on the host (safe to call without a GPU)."""
    lib = capi.load()
    cfg = _cfg()
    d = capi.make_desc(4, 384, 70, 28, 28, 11, 5, cfg, (.18, .12, .46))
    ws = lib.stego_corr_workspace_bytes(ctypes.byref(d))
    ctx = lib.stego_corr_saved_ctx_bytes(ctypes.byref(d))
    assert ws >= 4 * 6 * 128 * 68 * 4 + ctx and ctx >= 28 * 128 * (76 + 1 + 8) * 4     # anchor operand images + saved context
    args_null = [None] * 4 + [None] * 3 + [None] * 8 + [None, 0, None]
    assert lib.stego_corr_fwd(None, *args_null) == 1                      # STEGO_ERR_NULL
    assert lib.stego_corr_fwd(ctypes.byref(d), *args_null) == 1
    d12 = capi.make_desc(4, 384, 70, 28, 28, 12, 5, cfg, (.18, .12, .46))  # S*S = 144 > 128: the multi-launch path (csrc/corr_wide.hip) since round 5
    assert lib.stego_corr_fwd(ctypes.byref(d12), *args_null) == 1
    w16 = capi.make_desc(32, 384, 70, 28, 28, 16, 5, cfg, (.18, .12, .46))
    n_img, P = 7 * 32, 256
    assert lib.stego_corr_workspace_bytes(ctypes.byref(w16)) >= n_img * P * (384 + 70) * 4           # the operand images of both correlations
    assert lib.stego_corr_saved_ctx_bytes(ctypes.byref(w16)) >= n_img * P * (70 + 1) * 4             # the normalised code rows + 1 / |row|
    assert lib.stego_corr_bwd_workspace_bytes(ctypes.byref(w16)) >= 2 * n_img * P * 70 * 4
    w96 = capi.make_desc(4, 384, 96, 28, 28, 12, 5, cfg, (.18, .12, .46))                           # K > 88 beyond 128 points: two passes of the backward's GEMMs
    assert lib.stego_corr_fwd(ctypes.byref(w96), *args_null) == 1 and lib.stego_corr_workspace_bytes(ctypes.byref(w96)) > 0
    for bad in (capi.make_desc(4, 384, 70, 28, 28, 17, 5, cfg, (.18, .12, .46)),                    # S * S > 256
                capi.make_desc(4, 384, 130, 28, 28, 12, 5, cfg, (.18, .12, .46))):                  # K > 128
        assert lib.stego_corr_fwd(ctypes.byref(bad), *args_null) == 3     # STEGO_ERR_UNSUPPORTED
        assert lib.stego_corr_workspace_bytes(ctypes.byref(bad)) == 0
    d0 = capi.make_desc(0, 384, 70, 28, 28, 11, 5, cfg, (.18, .12, .46))
    assert lib.stego_corr_fwd(ctypes.byref(d0), *args_null) == 2          # STEGO_ERR_SHAPE
    assert b"unsupported" in lib.stego_error_string(3)
    assert lib.stego_error_string(0) == b"ok"


def test_deployment_flag_is_per_call_and_measurement_knobs_are_host_side():
    """ABI 3: "other kernels share the device" is a flag of the DESCRIPTOR (per call), set from cfg.shared_device, an explicit
    argument or the process default of capi.set_shared_device - never a side effect of a collective; stego_debug_set knobs are
    measurement switches (atomics, host state, no GPU needed), an index outside the table is refused; unknown flags are refused."""
    lib = capi.load()
    cfg = O.CorrCfg()
    mk = lambda **kw: capi.make_desc(4, 384, 70, 28, 28, 11, 5, cfg, (.18, .12, .46), **kw)
    assert mk().flags == 0 and mk(shared_device=True).flags == capi.FLAG_SHARED_DEVICE
    capi.set_shared_device(True)
    try:
        assert mk().flags == capi.FLAG_SHARED_DEVICE and mk(shared_device=False).flags == 0
        cfg.shared_device = False                      # the cfg key wins over the process default
        assert mk().flags == 0
    finally:
        capi.set_shared_device(False)
        del cfg.shared_device
    assert ctypes.sizeof(capi.StegoCorrDesc) == 15 * 4
    bad = mk()
    bad.flags = 2
    assert lib.stego_corr_workspace_bytes(ctypes.byref(bad)) == 0                     # unknown flag: unsupported descriptor
    assert sorted(capi.KNOBS.values()) == list(range(7)) and capi.KNOBS["STEGO_SHARED_DEVICE"] == 6
    assert lib.stego_debug_set(99, 1) == 2 and lib.stego_debug_set(-1, 1) == 2        # STEGO_ERR_SHAPE
    assert lib.stego_debug_occupy(0, 65536, 10, None) == 2                            # (argument check only: nothing is launched)


def test_allreduce_does_not_touch_the_library_state():
    """FlatGradReducer.allreduce_mean used to flip the process-wide shared-device knob on its first call (and never
    back).  The reducer no longer imports the binding at all."""
    import inspect
    from stego_amd import ddp
    assert "set_shared_device(" not in inspect.getsource(ddp.FlatGradReducer) and "import capi" not in inspect.getsource(ddp)


# ------------------------------------------------------------------ salience-guided coordinates (cfg.use_salience)
def test_salience_coords_follow_the_reference_draw_order():
    """modules.py:355-365 + sample_nonzero_locations :298-311: per image one randint over its non-zero salience pixels
    (or over the whole map if there are none), then rand, rand, rand(mask) - same generator, same order.  The expected
    values are restated from those lines; the restatement's draws equal what the reference function drew on the same maps
    after the same seed (tests/golden/salience_coords.npz, oracle/make_golden.py: salience_case)."""
    gold = load_golden("salience_coords")
    cfg = _cfg()
    cfg.use_salience = True
    cfg.feature_samples = 5
    B, H = 3, 12
    g = torch.Generator().manual_seed(3)
    sal = (torch.rand(B, H, H, generator=g) > 0.7).float()
    sal[1] = 0                                                   # an image without salient pixels: uniform randint fallback
    sal_pos = (torch.rand(B, H, H, generator=g) > 0.5).float()
    assert np.array_equal(sal.numpy(), gold["sal"]) and np.array_equal(sal_pos.numpy(), gold["sal_pos"])
    feats = torch.zeros(B, 4, 6, 6)
    loss = M.ContrastiveCorrelationLoss(cfg)

    torch.manual_seed(11)
    c1, c2 = loss.draw_coords(feats, sal, sal_pos)
    after = torch.rand(1)

    torch.manual_seed(11)
    shape = [B, 5, 5, 2]
    def snl(t, target_size):                                     # restatement of :298-311
        nz = torch.nonzero(t)
        coords = torch.zeros(target_size, dtype=nz.dtype)
        n = target_size[1] * target_size[2]
        for i in range(t.shape[0]):
            sel = nz[nz[:, 0] == i]
            pick = torch.randint(t.shape[1], size=(n, 2)) if sel.shape[0] == 0 else sel[torch.randint(len(sel), size=(n,)), 1:]
            coords[i] = pick.reshape(target_size[1], target_size[2], 2)
        return torch.flip(coords.to(torch.float32) / t.shape[1] * 2 - 1, dims=[-1])
    n1, n2 = snl(sal, shape), snl(sal_pos, shape)
    assert np.array_equal(n1.numpy(), gold["n1"]) and np.array_equal(n2.numpy(), gold["n2"])
    r1 = torch.rand(shape) * 2 - 1
    r2 = torch.rand(shape) * 2 - 1
    mask = (torch.rand(shape[:-1]) > .1).unsqueeze(-1).to(torch.float32)
    e1, e2 = n1 * mask + r1 * (1 - mask), n2 * mask + r2 * (1 - mask)
    assert torch.equal(c1, e1) and torch.equal(c2, e2)
    assert torch.equal(after, torch.rand(1))                     # generator left in the same state
    assert c1.min() >= -1 and c1.max() <= 1


def test_means_and_total_api_equal_the_reference_composition(oracle_backed):
    """ContrastiveCorrelationLoss.means() / .total(): the three loss means as one tensor (the forward kernel produces all of
    them) and their weighted sum as one dot product == train_segmentation.py:176-181 on forward()'s outputs, values and
    gradients, with the same draws."""
    c = GoldenCase("small_default")
    t = {k: torch.from_numpy(v) for k, v in c.inputs.items()}
    loss_fn = M.ContrastiveCorrelationLoss(c.cfg)
    code = t["code"].clone().requires_grad_(True)
    code_pos = t["code_pos"].clone().requires_grad_(True)
    torch.manual_seed(5)
    out = loss_fn(t["feats"], t["feats_pos"], None, None, code, code_pos)
    ref_total = 0.67 * out[0] + 0.25 * out[2] + 0.63 * out[4].mean()
    ref_total.backward()
    g1, g2 = code.grad.clone(), code_pos.grad.clone()
    code.grad = None
    code_pos.grad = None
    torch.manual_seed(5)
    total, means, icd, ecd, ncd = loss_fn.total(t["feats"], t["feats_pos"], None, None, code, code_pos, (0.67, 0.25, 0.63))
    assert means.shape == (3,) and not means.requires_grad
    assert_close(means.numpy(), np.array([float(out[0]), float(out[2]), float(out[4].mean())]), rtol=1e-5, what="means")
    assert abs(float(total) - float(ref_total)) < 1e-6 * max(1.0, abs(float(ref_total)))
    assert torch.equal(icd, out[1]) and torch.equal(ncd, out[5])
    total.backward()
    assert_close(code.grad.numpy(), g1.numpy(), rtol=1e-4, atol_frac=1e-5, what="d_code via total()")
    assert_close(code_pos.grad.numpy(), g2.numpy(), rtol=1e-4, atol_frac=1e-5, what="d_code_pos via total()")


def test_torch_glue_extension_is_built_and_bound_to_the_library():
    """stego_amd/lib/_stego_torchglue.so (csrc/torch_glue_ext.cpp, built by __graft_entry__.build()): loads next to the C-ABI library,
    resolves the entry points it calls (bind() checks the ABI version), and refuses host tensors like every other entry of the product."""
    import torch
    from stego_amd import capi, _build
    _build.build_torchglue()
    ext = capi.torchglue()
    assert ext is not None
    for name in ("bind", "philox_state", "ref_draws", "corr_loss", "head", "reset_workspaces"):
        assert hasattr(ext, name)
    x = torch.zeros(2, 8, 4, 4)
    desc = capi.make_desc(2, 8, 4, 4, 4, 2, 0, type("C", (), dict(pointwise=True, zero_clamp=True, stabalize=False))(), (0.1, 0.2, 0.3))
    with pytest.raises(RuntimeError, match="MI355X only"):
        ext.corr_loss(x, x, x[:, :4], x[:, :4], torch.zeros(2, 2, 2, 2), torch.zeros(2, 2, 2, 2), torch.zeros(0, 2, dtype=torch.long), bytes(desc), 0)


def test_lazy_loss_sum_contract_every_use_equals_the_plain_expression():
    """modules._LossScalar / _LazyLoss (the weighted sum of the three loss scalars the reference's training step writes,
    train_segmentation.py:178-181): what stays lazy is a closed list; everything else must be exactly the plain tensor expression."""
    import math
    import numpy as np
    import torch
    from stego_amd import modules as M

    x = torch.tensor([0.3, -1.2, 2.0], dtype=torch.float64, requires_grad=True)

    def family(lazy):
        o = [x[i] * 2.0 + 0.1 * i for i in range(3)]
        return M._lazy_scalars(*o) if lazy else o

    # (expression, stays lazy?)
    exprs = [
        (lambda a, b, c: (0.25 * b + 0.67 * a + 0.63 * c) * 1.5, True),        # the reference's line
        (lambda a, b, c: 0.25 * b.mean() + 0.67 * a.mean() + 0.63 * c.mean(), True),
        (lambda a, b, c: 0 + (a * 2 - b / 4) + (-c), True),
        (lambda a, b, c: a + b, True),
        (lambda a, b, c: torch.mul(2.0, a) - 3 * a, True),
        (lambda a, b, c: (a * 2) + 1.0, False),
        (lambda a, b, c: (a * 2) * torch.tensor(3.0, dtype=torch.float64), False),
        (lambda a, b, c: a * b, False),
        (lambda a, b, c: (a * 2) ** 2 + abs(b * -1) + 1 / (c * 2), False),
        (lambda a, b, c: torch.stack([0.5 * a, b * 2.0, c]).sum(), False),
        (lambda a, b, c: (2.0 * a).exp() + torch.sin(b * 0.5), False),
        (lambda a, b, c: 2 - a * 3, False),
        (lambda a, b, c: (a * 2).clamp(min=0.0) + (b * 2).detach(), False),
        (lambda a, b, c: a.exp(), False),
    ]
    for k, (f, stays_lazy) in enumerate(exprs):
        e = f(*family(True))
        r = f(*family(False))
        assert isinstance(e, M._LazyLoss) == stays_lazy, k
        assert math.isclose(float(e), float(r), rel_tol=1e-14, abs_tol=1e-15), k
        x.grad = None
        f(*family(True)).backward()
        g = x.grad.clone()
        x.grad = None
        f(*family(False)).backward()
        np.testing.assert_allclose(g.numpy(), x.grad.numpy(), rtol=1e-14, atol=1e-15, err_msg=str(k))
    # two forward calls never mix lazily; formatting, comparisons, numpy, item()
    a1, _, _ = family(True)
    _, b2, _ = family(True)
    assert isinstance(a1 * 2 + b2 * 2, torch.Tensor)
    e = (family(True)[0] * 2)
    assert ("%.4f" % e) == ("%.4f" % float(e)) and bool(e > 0) and np.asarray(e.detach()).shape == () and e.item() == float(e)
    assert isinstance(e.detach(), torch.Tensor) and not isinstance(e.detach(), M._LossScalar)
    # without cfg.lazy_loss_sums nothing is wrapped: test_default_forward_outputs_are_tensors below + tests/test_parity_gpu.py


def test_default_forward_outputs_are_tensors(monkeypatch):
    """VERDICT round 5 (weak 6) / train_segmentation.py:179-181,227: under the DEFAULT cfg the reference's training_step expression on the
    6-tuple of forward() is a torch.Tensor (the lazy wrappers are opt-in).  The native op is replaced by a stand-in with its output
    signature (8 outputs, csrc/torch_glue_ext.cpp) - this pins the host-side wrapping, not the kernels."""
    import torch
    from stego_amd import modules as M
    from oracle import corr_oracle as O
    B, C, H, W, K, S, n_neg = 2, 8, 5, 5, 4, 3, 2

    class FakeExt:
        @staticmethod
        def corr_loss(f, fp, c, cp, c1, c2, perms, desc, mode):
            s = (c.sum() + cp.sum()) * 1e-3
            cd = lambda n: torch.zeros(n, S, S, S, S) + s          # noqa: E731
            return (s * 1.0, cd(B), s * 2.0, cd(B), cd(n_neg * B), cd(n_neg * B), s * 3.0, torch.stack([s, s * 2.0, s * 3.0]))

    monkeypatch.setattr(M, "_native_autograd", lambda cfg: FakeExt)
    g = torch.Generator().manual_seed(0)
    f, fp = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    c, cp = torch.randn(B, K, H, W, generator=g, requires_grad=True), torch.randn(B, K, H, W, generator=g, requires_grad=True)
    coords = torch.rand(B, S, S, 2, generator=g) * 2 - 1
    perms = torch.stack([torch.roll(torch.arange(B), 1)] * n_neg)
    for lazy in (None, True):
        cfg = O.CorrCfg(feature_samples=S, neg_samples=n_neg)
        if lazy:
            cfg.lazy_loss_sums = True
        out = M.ContrastiveCorrelationLoss(cfg).forward_explicit(f, fp, c, cp, coords, coords, perms)
        assert all(isinstance(o, torch.Tensor) for o in out)
        loss = 0
        loss += (0.25 * out[2] + 0.67 * out[0] + 0.63 * out[4].mean()) * 1.0
        assert isinstance(loss, torch.Tensor) == (lazy is None)
        assert isinstance(loss, M._LazyLoss) == bool(lazy)
        if lazy is None:
            assert type(out[0]) is torch.Tensor and type(out[2]) is torch.Tensor and torch.is_tensor(loss)
        c.grad = cp.grad = None
        loss.backward()
        assert c.grad is not None and cp.grad is not None


def test_cached_upstream_constants_are_bounded_and_never_reallocated():
    """modules._LossFamily caches the device constants a lazy weighted sum hands to the backward; coefficients that change
    every step (scheduled loss weights) must not grow it without bound, and a cached tensor is never replaced by a new allocation (a
    captured graph may hold its address): at the bound the least recently used tensor is overwritten in place and re-keyed."""
    import torch
    from stego_amd import modules as M
    F = M._LossFamily
    old, F._const, F._pinned = (F._const, F._pinned), {}, set()
    try:
        like = torch.zeros((), dtype=torch.float32)
        first = F.const(0.5, like)
        ptr = first.data_ptr()
        seen = {ptr}
        for i in range(3 * F._CONST_MAX):
            t = F.const(1.0 + i, like)
            assert float(t) == 1.0 + i
            seen.add(t.data_ptr())
            v = F.const3((float(i), 0.25, 0.5), like)
            assert v.tolist() == [float(i), 0.25, 0.5] and v.shape == (3,)
        assert len(F._const) <= F._CONST_MAX and len(seen) <= F._CONST_MAX
        assert F.const(1.0 + 3 * F._CONST_MAX - 1, like) is F.const(1.0 + 3 * F._CONST_MAX - 1, like)      # a hit returns the same tensor
    finally:
        F._const, F._pinned = old


def test_the_selected_generator_restatement_is_reported_and_a_fallback_warns_once(caplog):
    """stego_ref_draws / stego_ref_dropout_masks restate ATen's generator arithmetic; the self-check that selects a
    variant (or keeps the torch calls) must say which - a torch upgrade may not silently return the step to dozens of tiny launches."""
    import logging
    import warnings
    from stego_amd import modules as M
    with caplog.at_level(logging.INFO, logger="stego_amd"):
        M._report_variant("the draws (test)", "stego_ref_draws", 3, "cost")
    assert any("variant 3 of stego_ref_draws" in r.getMessage() for r in caplog.records)
    M._REPORTED_FALLBACKS.discard(("the draws (test)", "stego_ref_draws"))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        M._report_variant("the draws (test)", "stego_ref_draws", -1, "~31 tiny launches per step instead of one")
        M._report_variant("the draws (test)", "stego_ref_draws", -1, "~31 tiny launches per step instead of one")
    assert len(rec) == 1 and "torch calls are kept" in str(rec[0].message) and "31 tiny launches" in str(rec[0].message)


@pytest.mark.parametrize("S,n_neg,pointwise,stab", [(12, 2, True, False), (13, 0, True, True), (5, 3, False, False)])
def test_generic_forward_as_one_batch_of_pair_sets_equals_the_oracle(S, n_neg, pointwise, stab):
    """generic_forward (what feature_samples > 11 or dim > 128 run on) computes all 2 + neg_samples pair-sets in ONE batch, the per-set
    means of modules.py:331-333 over a [sets, B, ...] view: forward values and the gradients into both code maps against the fp64
    restatement of the reference's loop (torch on CPU tensors: grid_sample + einsum - the same code the device path runs with the
    native dense kernel in place of the einsum)."""
    from oracle import corr_oracle as O
    B, C, H, W, K = 3, 16, 7, 6, 9
    d = O.synth_inputs(B, C, H, W, K, S, n_neg, seed=321 + S)
    cfg = O.CorrCfg(feature_samples=S, neg_samples=n_neg, pointwise=pointwise, stabalize=stab)
    t = {k: torch.from_numpy(np.asarray(d[k])) for k in ("feats", "feats_pos", "code", "code_pos", "coords1", "coords2")}
    perms = torch.from_numpy(np.asarray(d["perms"])) if n_neg else None
    code, code_pos = t["code"].clone().requires_grad_(True), t["code_pos"].clone().requires_grad_(True)
    out = M.ContrastiveCorrelationLoss(cfg).generic_forward(t["feats"], t["feats_pos"], code, code_pos, t["coords1"], t["coords2"], perms)
    ref = O.corr_loss_forward(d["feats"], d["feats_pos"], d["code"], d["code_pos"], d["coords1"], d["coords2"], d["perms"], cfg)
    assert_close(out[1].detach().numpy(), ref.pos_intra_cd, rtol=1e-4, atol_frac=1e-4, what="intra_cd")
    assert_close(out[3].detach().numpy(), ref.pos_inter_cd, rtol=1e-4, atol_frac=1e-4, what="inter_cd")
    assert abs(float(out[0].detach()) - float(ref.pos_intra_loss)) < 1e-5 + 1e-4 * abs(float(ref.pos_intra_loss))
    assert abs(float(out[2].detach()) - float(ref.pos_inter_loss)) < 1e-5 + 1e-4 * abs(float(ref.pos_inter_loss))
    assert tuple(out[4].shape) == (n_neg * B, S, S, S, S) and tuple(out[5].shape) == (n_neg * B, S, S, S, S)
    total = 0.67 * out[0] + 0.25 * out[2]
    g_nl = None
    if n_neg:
        assert_close(out[4].detach().numpy(), ref.neg_inter_loss, rtol=1e-4, atol_frac=1e-4, what="neg_loss")
        assert_close(out[5].detach().numpy(), ref.neg_inter_cd, rtol=1e-4, atol_frac=1e-4, what="neg_cd")
        total = total + 0.63 * out[4].mean()
        g_nl = np.full(ref.neg_inter_loss.shape, 0.63 / (n_neg * B * S ** 4))
    total.backward()
    dc, dcp = O.corr_loss_backward(d["feats"], d["feats_pos"], d["code"], d["code_pos"], d["coords1"], d["coords2"], d["perms"], cfg,
                                   0.67, 0.25, g_nl)
    assert_close(code.grad.numpy(), dc, rtol=1e-3, atol_frac=1e-3, what="d_code")
    assert_close(code_pos.grad.numpy(), dcp, rtol=1e-3, atol_frac=1e-3, what="d_code_pos")


def test_bench_denominators_are_the_contract_s_numbers():
    """The roofline fractions of bench.py divide by SURVEY.md 8(d)'s algorithmic bytes - every distinct tensor once, fp32.  The figures
    the round verdicts recomputed (113 671 436 B forward, 48 543 488 B backward at BASELINE config 2) are pinned here: a changed
    denominator would move every reported fraction without a kernel getting faster."""
    import bench
    B, C, H, W, K, S, n_neg = 32, 384, 28, 28, 70, 11, 5
    fwd = bench.algorithmic_bytes_fwd(B, C, H, W, K, S, n_neg)
    # inputs: two feature maps, two code maps, two coordinate sets, the permutations; outputs: cd of 2 + n_neg pair-sets, the negative loss
    # tensor, three scalars
    assert fwd == 4 * (2 * B * C * H * W + 2 * B * K * H * W + 2 * B * S * S * 2) + 8 * n_neg * B + 4 * (7 + 5) * B * S ** 4 + 12 == 113671436
    assert bench.algorithmic_bytes_bwd(B, K, H, W, S, n_neg) == 48543488
    assert bench.algorithmic_flops_fwd(B, C, K, S, n_neg) == 2 * 7 * B * S ** 4 * (C + K) == 2977862272
    assert bench.WORKLOADS["vits8_224"] == (384, 28, 28, 70) and bench.WORKLOADS["vitb8_320"] == (768, 40, 40, 70)
    assert bench.head_grad_numel(384, 70) == 384 * 70 + 70 + 384 * 384 + 384 + 384 * 70 + 70 + 70 * 27 + 27 + 27 * 70
    # round 5: the record explains itself - the fraction of the achievable HBM rate beside the fraction of the peak, where the `traffic`
    # constant comes from (a file of the builder's counter passes, not this run), the other arithmetic mode with its own forward roofline,
    # and for N > 1 what every rank saw and what the all-reduce costs on its own
    assert bench.HBM_PEAK == 8.0e12 and bench.HBM_ACHIEVABLE == 6.3e12
    src = open(bench.__file__).read()
    for key in ("frac_of_achievable", "traffic_source", 'alt["roofline"]', "ms_per_step_by_rank", "ms_per_step_rank_min", "ms_per_step_rank_max", "allreduce_us",
                '"feature_samples_16": wide', "--feature-samples"):          # (the multi-launch path of cfg.feature_samples 12 .. 16 in the same line)
        assert key in src, key
    import json
    tj = json.load(open(os.path.join(os.path.dirname(bench.__file__), "profiles", "traffic.json")))
    assert isinstance(tj["vits8_224_f16x3_B32"], int) and "_source" in tj


def test_the_product_never_imports_the_oracle():
    """The oracle is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import it; the package
    itself must fail loudly without the HIP library rather than fall back to a CPU restatement."""
    import ast
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in glob.glob(os.path.join(root, "stego_amd", "**", "*.py"), recursive=True):
        tree = ast.parse(open(path).read())
        for node in ast.walk(tree):
            names = []
            if isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            assert not any(n == "oracle" or n.startswith("oracle.") or n == "oracle_backend" for n in names), (path, names)
    # bench.py: the oracle appears in cpu_baseline() only; __graft_entry__: in smoke() only
    for fname, allowed in (("bench.py", "cpu_baseline"), ("__graft_entry__.py", "smoke")):
        tree = ast.parse(open(os.path.join(root, fname)).read())
        for fn in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.Module))]:
            body = fn.body if isinstance(fn, ast.Module) else []
            for node in (ast.walk(fn) if isinstance(fn, ast.FunctionDef) else body):
                if isinstance(node, (ast.Import, ast.ImportFrom)):
                    mod = node.module if isinstance(node, ast.ImportFrom) else node.names[0].name
                    if mod and (mod == "oracle" or mod.startswith("oracle.")):
                        assert isinstance(fn, ast.FunctionDef) and fn.name == allowed, (fname, getattr(fn, "name", "module level"))
