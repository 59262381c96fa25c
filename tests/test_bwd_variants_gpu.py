"""Every kernel pair the loss backward can dispatch and every limit of bwd_check, on the device against the fp64 oracle: one case per row
of tests/bwd_variant_cases.py (tests/test_bwd_variants_host.py proves on the CPU that each row reaches the pair it names and that the
table reaches every kernel corr_bwd.hip and corr_bwd_lists.hip emit).  One forward and the backwards of a row through the C ABI, in the
manner of tests/test_bwd_fused.py; helper rows through ContrastiveCorrelationLoss.helper.  Needs the MI355X."""
from ctypes import byref

import numpy as np
import pytest
import torch

import bwd_variant_cases as T
from conftest import assert_close
from oracle import corr_oracle as O
from stego_amd import capi
from stego_amd import modules as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHIFT = 0.31                                 # helper rows
PREC = {"f32": capi.PREC_F32, "f16x3": capi.PREC_F16X3}
BY_NAME = {c.name: c for c in T.CASES}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _cl(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _cfg(case):
    S, n_neg = case.shape[5:]
    cfg = O.CorrCfg(feature_samples=S, neg_samples=n_neg, zero_clamp=case.cfg != "noclamp")
    cfg.corr_precision = case.precision
    return cfg


def _poison(n_bytes):
    """A NaN-filled block of the workspace's size, allocated and freed: the backward's workspace (and whatever else the allocator recycles
    from it) starts out poisoned."""
    t = torch.full(((int(n_bytes) + 3) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    del t


_ORACLES = {}


def _oracle(case, d):
    """fp64 gradients of the row; computed once per (inputs, upstreams, cfg) and shared by the rows that differ in precision or path."""
    key = (case.shape, case.seed, case.recipe, case.dense, case.mode, case.cfg)
    if key not in _ORACLES:
        cfg = _cfg(case)
        if case.mode == "helper":
            f1, f2, c1, c2 = (d[k].astype(np.float64) for k in ("f1", "f2", "c1", "c2"))
            _, cd, fd = O.helper(f1, f2, c1, c2, SHIFT, cfg)
            res = O._helper_bwd_codes(c1, c2, fd, cd, SHIFT, cfg, d["ups"][0].astype(np.float64), d["ups"][1].astype(np.float64))
        else:
            B, C, H, W, K, S, n_neg = case.shape
            args = (d["feats"], d["feats_pos"], d["code"], d["code_pos"], d["coords1"], d["coords2"], d["perms"], cfg)
            if case.dense:
                u = d["ups"]
                res = O.corr_loss_backward(*args, float(u[0]), float(u[2]), u[4], g_intra_cd=u[1], g_inter_cd=u[3], g_neg_cd=u[5])
            else:
                g_nl = np.full((n_neg * B, S, S, S, S), 0.63 / max(n_neg * B * S ** 4, 1))
                res = O.corr_loss_backward(*args, 0.67, 0.25, g_nl)
        for r in res:
            r.setflags(write=False)
        _ORACLES[key] = res
    return _ORACLES[key]


class _Forward:
    """One forward of a row (or a refusal) through the C ABI, the saved context kept; backward() as often as wanted."""

    def __init__(self, shape, precision, cfg, d):
        B, C, H, W, K, S, n_neg = shape
        self.shape = shape
        self.desc = capi.make_desc(B, C, K, H, W, S, n_neg, cfg, (cfg.pos_intra_shift, cfg.pos_inter_shift, cfg.neg_inter_shift), PREC[precision])
        t = {k: _dev(v) for k, v in d.items() if k != "ups"}
        self.t = t
        self.ups = [_dev(u) for u in d["ups"]] if "ups" in d else None
        self.c, self.cp = _cl(t["code"]), _cl(t["code_pos"])
        self.perms = t["perms"] if n_neg else None
        out = capi.corr_fwd(self.desc, _cl(t["feats"]), _cl(t["feats_pos"]), self.c, self.cp, t["coords1"], t["coords2"], self.perms, True)
        self.lm, self.icd, self.ecd, self.nl, self.ncd, self.saved = out
        torch.cuda.synchronize()
        self.ws_bytes = int(capi.load().stego_corr_bwd_workspace_bytes(byref(self.desc)))

    def upstreams(self):
        """(g_intra, g_inter, g_neg_loss, g_intra_cd, g_inter_cd, g_neg_cd): dense tensors on all six outputs, or the scalars of training"""
        B, C, H, W, K, S, n_neg = self.shape
        if self.ups is not None:
            u = self.ups
            return u[0], u[2], (u[4] if n_neg else None), u[1], u[3], (u[5] if n_neg else None)
        gn = torch.full((1,), 0.63 / max(n_neg * B * S ** 4, 1), device=DEV).expand(n_neg * B, S, S, S, S) if n_neg else None
        return torch.tensor(0.67, device=DEV), torch.tensor(0.25, device=DEV), gn, None, None, None

    def backward(self, debug):
        gi, ge, gnl, gicd, gecd, gncd = self.upstreams()
        _poison(self.ws_bytes)
        capi.debug_set("STEGO_DEBUG_BWD", debug)
        try:
            dc, dcp = capi.corr_bwd(self.desc, self.c, self.cp, self.t["coords1"], self.t["coords2"], self.perms, self.saved,
                                    self.icd, self.ecd, self.ncd, gi, ge, gnl, gicd, gecd, gncd)
            torch.cuda.synchronize()
        finally:
            capi.debug_set("STEGO_DEBUG_BWD", 0)
        return dc.contiguous().cpu().numpy(), dcp.contiguous().cpu().numpy()


def _helper_backward(case, d):
    cfg = _cfg(case)
    N, C, S1, S2, K = case.shape[:5]
    desc = capi.make_desc(N, C, K, S1, S2, S2, 0, cfg, (SHIFT,) * 3, PREC[case.precision])
    tc1 = _dev(d["c1"]).requires_grad_(True)
    tc2 = _dev(d["c2"]).requires_grad_(True)
    loss, cd = M.ContrastiveCorrelationLoss(cfg).helper(_dev(d["f1"]), _dev(d["f2"]), tc1, tc2, SHIFT)
    total = (loss * _dev(d["ups"][0])).sum() + (cd * _dev(d["ups"][1])).sum()
    torch.cuda.synchronize()
    _poison(capi.load().stego_corr_helper_bwd_workspace_bytes(byref(desc)))
    capi.debug_set("STEGO_DEBUG_BWD", case.debug)
    try:
        total.backward()
        torch.cuda.synchronize()
    finally:
        capi.debug_set("STEGO_DEBUG_BWD", 0)
    return tc1.grad.cpu().numpy(), tc2.grad.cpu().numpy()


_RUNS = {}


def _run(case, cached=True):
    """(first call, second call, oracle) of a row; kept, so that an F16X3 row finds its F32 twin's figures."""
    if cached and case.name in _RUNS:
        return _RUNS[case.name]
    d = T.make_inputs(case)
    if case.mode == "helper":
        a, b = _helper_backward(case, d), _helper_backward(case, d)
    else:
        fwd = _Forward(case.shape, case.precision, _cfg(case), d)
        a, b = fwd.backward(case.debug), fwd.backward(case.debug)
    res = (a, b, _oracle(case, d))
    if cached:
        _RUNS[case.name] = res
    return res


def _rel_err(got, exp):
    return max(float(np.abs(g - e).max() / np.abs(e).max()) for g, e in zip(got, exp))


def _check_against_oracle(case, got, exp):
    for g, e, what in zip(got, exp, ("d_code", "d_code_pos") if case.mode == "forward" else ("d_c1", "d_c2")):
        assert np.isfinite(g).all(), (case.name, what)
        assert_close(g, e, rtol=1e-3, atol_frac=1e-3, what="%s %s" % (case.name, what))
        # a pixel no tap touches carries neither stale workspace nor another unit's row
        assert not g[e == 0].any(), (case.name, what, int(np.count_nonzero(g[e == 0])))


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_backward_variant_against_the_fp64_oracle(name):
    case = BY_NAME[name]
    a, b, exp = _run(case)
    err = _rel_err(a, exp)
    print("BWDVAR %s %s kernels %s + %s: max error / max|oracle| = %.3e" % (case.name, case.precision, case.kernels[0], case.kernels[1], err))
    _check_against_oracle(case, a, exp)
    if case.kernels[1] == "unsample_kernel":
        # the band appends row-entries in arrival order: fp32 rounding of the sums (test_backward_wide_map_fallback_...), nothing more
        scale = max(float(np.abs(e).max()) for e in exp)
        for x, y in zip(a, b):
            assert float(np.abs(x - y).max()) <= 1e-6 * scale, case.name
    else:
        for x, y in zip(a, b):
            assert np.array_equal(x, y), case.name + ": not repeatable"
    t = T.twin(case)
    if t is not None:
        # the bar of test_split_fp16_backward_error_stays_in_the_fp32_class
        err32 = _rel_err(_run(t)[0], exp)
        print("BWDVAR %s: F32 twin %s %.3e" % (case.name, t.name, err32))
        assert err <= 2.0 * err32 + 1e-6, (case.name, err, err32)


def _raw_bwd(fwd, debug, d_code, d_code_pos, ws):
    """stego_corr_bwd on buffers of the caller's: the return code, nothing raised."""
    gi, ge, gnl, _, _, _ = fwd.upstreams()
    capi.debug_set("STEGO_DEBUG_BWD", debug)
    try:
        rc = capi.load().stego_corr_bwd(byref(fwd.desc), capi._ptr(fwd.perms), capi._ptr(fwd.saved[0]), capi._ptr(fwd.saved[1]), capi._ptr(fwd.saved[2]),
                                        capi._ptr(fwd.icd), capi._ptr(fwd.ecd), capi._ptr(fwd.ncd), capi._ptr(gi), capi._ptr(ge), capi._ptr(gnl), 0,
                                        None, None, None, capi._ptr(d_code), capi._ptr(d_code_pos), capi._ptr(ws), ws.numel(), capi._stream())
        torch.cuda.synchronize()
    finally:
        capi.debug_set("STEGO_DEBUG_BWD", 0)
    return rc


def test_refused_backwards_raise_launch_nothing_and_leave_the_library_usable():
    for r in T.REFUSALS:
        B, C, H, W, K, S, n_neg = r.shape
        d = O.synth_inputs(B, C, H, W, K, S, n_neg, seed=1)
        fwd = _Forward(r.shape, r.precision, O.CorrCfg(feature_samples=S, neg_samples=n_neg), d)
        assert fwd.ws_bytes > 0                                   # check_desc takes the shape: the forward ran, the refusal is the backward's own
        with pytest.raises(RuntimeError, match="unsupported" if r.why == "bwd_check" else "libstego_corr error"):
            fwd.backward(r.debug)
        # nothing was launched: neither output nor the workspace is touched
        d_code = torch.full((B, H, W, K), -7.25, device=DEV)
        d_code_pos = torch.full((B, H, W, K), -7.25, device=DEV)
        ws = torch.full((fwd.ws_bytes,), 0x5A, dtype=torch.uint8, device=DEV)
        rc = _raw_bwd(fwd, r.debug, d_code, d_code_pos, ws)
        assert rc != 0, r.name
        if r.why == "bwd_check":
            assert "unsupported" in capi.load().stego_error_string(rc).decode()
        assert bool((d_code == -7.25).all()) and bool((d_code_pos == -7.25).all()) and bool((ws == 0x5A).all()), r.name
        del fwd, d_code, d_code_pos, ws
    case = BY_NAME[T.AFTER_REFUSAL]
    a, _, exp = _run(case, cached=False)
    _check_against_oracle(case, a, exp)


@pytest.mark.parametrize("name", [s.name for s in T.SURFACE])
def test_python_surface_takes_the_generic_path_where_the_backward_refuses(name):
    """forward_explicit + backward() at the two shapes bwd_check refuses: ContrastiveCorrelationLoss must not run the native forward and
    then raise inside backward(); it computes them on generic_forward() like every other shape the kernels do not cover."""
    s = [s for s in T.SURFACE if s.name == name][0]
    B, C, H, W, K, S, n_neg = s.shape
    assert not M.ContrastiveCorrelationLoss.fused_kernels_cover(B, C, K, H, W, S, torch.device(DEV), n_neg=n_neg)
    d = T.make_inputs(s)
    cfg = _cfg(s)
    t = {k: _dev(v) for k, v in d.items()}
    c = _cl(t["code"]).detach().requires_grad_(True)
    cp = _cl(t["code_pos"]).detach().requires_grad_(True)
    out = M.ContrastiveCorrelationLoss(cfg).forward_explicit(_cl(t["feats"]), _cl(t["feats_pos"]), c, cp, t["coords1"], t["coords2"], t["perms"])
    (0.67 * out[0] + 0.25 * out[2] + 0.63 * out[4].mean()).backward()
    torch.cuda.synchronize()
    exp = _oracle(s, d)
    for g, e, what in zip((c.grad, cp.grad), exp, ("d_code", "d_code_pos")):
        g = g.cpu().numpy()
        assert np.isfinite(g).all()
        assert_close(g, e, rtol=1e-3, atol_frac=1e-3, what="%s %s" % (name, what))
