"""The wide loss path (csrc/corr_wide.hip, cfg.feature_samples 12 .. 16) and the building blocks the generic path reuses, on the device
against fp64: (a) the operand images of every sampler instantiation, (b) the three GEMMs on prepared operands, (c) the adjoint and the
pointwise stages, (d) every row of tests/wide_variant_cases.py end to end through stego_corr_fwd / stego_corr_bwd on poisoned workspaces.
tests/test_wide_variants_host.py proves on the CPU that each row reaches the variants it names and that the table reaches every variant.

One rule throughout: the kernel's error against fp64 is at most twice the error of fp32 torch computing the same statement on the same
inputs, plus a floor that follows from the number formats and the data's scale (written at each use).  Needs the MI355X."""
from ctypes import byref, c_float

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wide_variant_cases as T
from conftest import assert_close
from oracle import corr_oracle as O
from oracle import torch_cpu_port as PORT
from stego_amd import capi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BY_NAME = {c.name: c for c in T.CASES}
PANEL_BY_NAME = {q.name: q for q in T.PANELS}
EPS_GROUP = 1e3          # gradients beyond this magnitude come from the eps branch of norm() (g / 1e-10): compared at their own scale


def _up256(v):
    return (int(v) + 255) // 256 * 256


def _layout(x, layout):
    """numpy [B, C, H, W] -> a device view of that shape with exactly the strides and the alignment of wide_variant_cases.facts(layout) - also
    where torch would report other strides for an axis of one element; the spare channels of a slice hold NaN."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    B, C, H, W = t.shape
    sn, sc, sh, sw, off = T.facts(layout, C, H, W)
    buf = torch.full((B * sn + 4,), float("nan"), dtype=torch.float32, device=DEV)
    v = buf.as_strided((B, C, H, W), (sn, sc, sh, sw), off // 4)
    v.copy_(t)
    assert v.stride() == (sn, sc, sh, sw) and v.data_ptr() % 256 == off, (layout, v.stride(), v.data_ptr() % 256)
    return v


def _decode(panels, row_scale, images, C, P):
    """[image][128-point block][64-channel chunk][hi | lo][128][72] fp16 -> (hi + lo [images, nb 128, NCH 64], the same times row_scale), fp64."""
    nb, nch = (P + 127) // 128, (C + 63) // 64
    h = panels.view(torch.float16).view(images, nb, nch, 2, 128, 72)[..., :64].double()
    raw = (h[:, :, :, 0] + h[:, :, :, 1]).permute(0, 1, 3, 2, 4).reshape(images, nb * 128, nch * 64)
    return raw, raw * row_scale.double().reshape(images, nb * 128, 1)


def _rows(x):
    """[N, C, S, S] -> channels-last rows [N, S * S, C]: point q = h S + w"""
    return np.ascontiguousarray(np.moveaxis(x, 1, -1)).reshape(x.shape[0], -1, x.shape[1])


def _sample32(t, coords, idx=None):
    """fp32 torch on the device: sample() of modules.py:287-288 as rows [N, P, C]"""
    n = t.shape[0] if idx is None else len(idx)
    src = t if idx is None else t[torch.as_tensor(idx, device=DEV)]
    co = coords[torch.arange(n, device=DEV) % coords.shape[0]]
    out = F.grid_sample(src, co.permute(0, 2, 1, 3), padding_mode="border", align_corners=True)
    return out.permute(0, 2, 3, 1).reshape(n, -1, t.shape[1])


def _sample64(x, coords, idx=None):
    n = x.shape[0] if idx is None else len(idx)
    src = x.astype(np.float64) if idx is None else x.astype(np.float64)[np.asarray(idx)]
    return O.sample(src, coords.astype(np.float64)[np.arange(n) % coords.shape[0]])


def _check_panel_rows(tag, raw, dec, P, C, ref_n, t32_n, zero_rows):
    """The decoded operand images of one map against the fp64 normalised rows ref_n [N, P, C]; t32_n: fp32 torch's.  Returns (err, e32)."""
    raw, dec = raw[:, :P].cpu().numpy(), dec[:, :P].cpu().numpy()
    assert np.isfinite(dec).all(), tag
    assert not raw[:, :, C:].any(), tag + ": channels C .. 64 NCH of a live row are exact zeros in both halves"
    mx = np.abs(raw).max(-1)
    assert (mx[~zero_rows] >= 0.5).all() and (mx[~zero_rows] <= 1.0).all(), tag + ": a live row's largest magnitude lies in [0.5, 1]"
    assert not dec[zero_rows].any(), tag + ": an exactly zero row decodes to zeros"
    err_row = np.abs(dec[:, :, :C] - ref_n).max(-1)
    e32 = float(np.abs(t32_n - ref_n).max())
    # the split's own bound (corr_common.h): |e| <= 2^-22 |x| per element, hi and lo together 2^-21 of the row's largest magnitude
    bar = 2.0 * e32 + 2.0 ** -21 * np.abs(ref_n).max(-1)
    assert (err_row <= bar).all(), (tag, float(err_row.max()), e32)
    return float(err_row.max()), e32


# ------------------------------------------------------------------------------------------------ (a) panels against fp64
def _panel_inputs(q):
    B, H, W = T.PANEL_MAP
    rng = np.random.default_rng(500 + q.C)
    x = rng.standard_normal((B, q.C, H, W)).astype(np.float32)
    x[1, :, 2:6, 3:8] = 0.0                                       # the points inside sample exactly zero rows
    coords = T.edge_coords(rng, B, q.S, H, W)
    return x, coords


@pytest.mark.parametrize("name", [q.name for q in T.PANELS])
def test_panels_of_every_one_map_instantiation_against_fp64(name):
    q = PANEL_BY_NAME[name]
    x, coords = _panel_inputs(q)
    B, C, P = x.shape[0], q.C, q.S * q.S
    t, co = _layout(x, q.layout), torch.from_numpy(coords).to(DEV)
    for idx, want_rows in ((None, False), ([1, 1, 0], True)):
        n = B if idx is None else len(idx)
        ps = capi.PanelSet(n, C, P, DEV)
        ps.panels.fill_(0xFF)
        ps.row_scale.view(torch.uint8).fill_(0xFF)
        rows_out = torch.full((n, P, C), float("nan"), device=DEV) if want_rows else None
        inv_out = torch.full((n, P), float("nan"), device=DEV) if want_rows else None
        capi.sample_panels(ps, 0, t, co, None if idx is None else torch.tensor(idx, device=DEV), True, rows_out, inv_out)
        torch.cuda.synchronize()
        s64 = _rows(_sample64(x, coords, idx))
        nrm = np.sqrt((s64 * s64).sum(-1))
        ref_n = s64 / np.maximum(nrm, 1e-10)[..., None]
        zero_rows = ~s64.any(-1)
        assert zero_rows.any() and not zero_rows.all()
        s32 = _sample32(t, co, idx)
        t32_n = F.normalize(s32, dim=2, eps=1e-10).double().cpu().numpy()
        raw, dec = _decode(ps.panels, ps.row_scale, n, C, P)
        err, e32 = _check_panel_rows(name, raw, dec, P, C, ref_n, t32_n, zero_rows)
        print("WIDEVAR %s panels<%d> index %s: max row error %.3e, fp32 torch %.3e" % (name, q.vw, idx is not None, err, e32))
        if want_rows:
            got, inv = rows_out.double().cpu().numpy(), inv_out.double().cpu().numpy()
            # one more fp32 rounding (row * 1 / norm) than the statement has: 2^-23 of the row's largest magnitude
            erow = np.abs(got - ref_n).max(-1)
            assert (erow <= 2.0 * e32 + 2.0 ** -23 * np.abs(ref_n).max(-1)).all(), (name, float(erow.max()), e32)
            inv64 = 1.0 / np.maximum(nrm, 1e-10)
            inv32 = (1.0 / s32.norm(dim=2).clamp_min(1e-10)).double().cpu().numpy()
            assert (inv[zero_rows] == np.float32(1e10)).all(), name + ": inv_out of an exactly zero row is 1e10"
            einv, e32inv = np.abs(inv / inv64 - 1).max(), np.abs(inv32 / inv64 - 1).max()
            assert einv <= 2.0 * e32inv + 2.0 ** -23, (name, einv, e32inv)
            print("WIDEVAR %s rows_out: max error %.3e (fp32 torch %.3e), inv_out relative %.3e (fp32 torch %.3e)" % (name, erow.max(), e32, einv, e32inv))


# ------------------------------------------------------------------------------------------------ (b) prepared-operand GEMM against fp64
def _encode(rows, poison):
    """fp32 rows [images, P, C] (CPU) -> a PanelSet holding them as stego_sample_panels would write them: every row times the power of two that
    puts its largest magnitude into [0.5, 1), split into fp16 hi + lo, zeros up to the end of the last chunk, 1 / scale beside it.  Rows
    P .. 128 nb - 1 and their scales: 0xFF bytes (NaN) when `poison`, zeros otherwise."""
    images, P, C = rows.shape
    nb, nch = (P + 127) // 128, (C + 63) // 64
    mx = rows.abs().amax(-1)
    rs = torch.where(mx > 0, torch.ldexp(torch.ones_like(mx), -torch.frexp(mx)[1]), torch.ones_like(mx))
    x = torch.zeros(images, nb * 128, nch * 64)
    x[:, :P, :C] = rows * rs[..., None]
    hi = x.half()
    lo = (x - hi.float()).half()
    buf = torch.full((images, nb, nch, 2, 128, 72), -1 if poison else 0, dtype=torch.int16).view(torch.float16)
    live = torch.zeros(nb * 128, dtype=torch.bool)
    live[:P] = True
    live = live.view(1, nb, 1, 128, 1).expand(images, nb, nch, 128, 64)
    for which, part in ((0, hi), (1, lo)):
        v = part.view(images, nb, 128, nch, 64).permute(0, 1, 3, 2, 4)            # [image][block][chunk][128][64]
        buf[:, :, :, which, :, :64][live] = v[live]
    scale = torch.full((images, nb * 128), float("nan") if poison else 0.0)
    scale[:, :P] = 1.0 / rs
    ps = capi.PanelSet(images, C, P, DEV)
    ps.panels.copy_(buf.view(torch.uint8).flatten().to(DEV))
    ps.row_scale.copy_(scale.to(DEV))
    return ps, (hi.double() + lo.double())[:, :P, :C] / rs.double()[..., None]


def _unit_rows(rng, images, P, C):
    x = rng.standard_normal((images, P, C))
    x /= np.sqrt((x * x).sum(-1, keepdims=True))
    x[0, 3] = 0.0                                                  # zero rows: scale 1, all-zero halves
    x[images - 1, P - 1] = 0.0
    return torch.from_numpy(x.astype(np.float32))


GEMM_CASES = [        # kernel, C, M, N
    ("rowpair", 128, 144, 255), ("rowpair", 70, 256, 129), ("rowpair", 64, 144, 100),
    ("rowblock", 384, 129, 256), ("rowblock", 134, 255, 144), ("rowblock", 64, 100, 144),
    ("tile", 392, 144, 129), ("tile", 770, 129, 255), ("tile", 392, 64, 144), ("tile", 1028, 256, 144),
]


@pytest.mark.parametrize("kernel,C,M,N", GEMM_CASES)
def test_prepared_operand_gemm_against_fp64_of_the_decoded_operands(kernel, C, M, N):
    nbA, nch = (M + 127) // 128, (C + 63) // 64
    assert kernel == ("rowpair" if nch <= 2 and nbA >= 2 else "rowblock" if nch <= 6 else "tile")        # (panel_gemm_plan; pinned by the host test)
    images_a, n_pairs = 2, 5
    rng = np.random.default_rng(C * 1000 + M)
    a32, b32 = _unit_rows(rng, images_a, M, C), _unit_rows(rng, n_pairs, N, C)
    pa, a64 = _encode(a32, True)
    pb, b64 = _encode(b32, True)
    assert torch.equal(a64.float().double(), a64) and torch.equal(b64.float().double(), b64)      # the decoded operands are fp32 numbers
    sel = torch.arange(n_pairs) % images_a
    ref = torch.matmul(a64[sel], b64.transpose(1, 2))
    y32 = torch.matmul(a64.float()[sel], b64.float().transpose(1, 2))        # the yardstick: torch's fp32 matmul (CPU) of the same operands
    out, rowsum = capi.dense_corr_panels(pa, images_a, pb, n_pairs, want_rowsum=True)
    out_only = capi.dense_corr_panels(pa, images_a, pb, n_pairs)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(rowsum).all(), "a poisoned pad row reached the output"
    assert torch.equal(out, out_only), "the product depends on whether the row sums are wanted"
    got = out.double().cpu()
    err, e32 = float((got - ref).abs().max()), float((y32.double() - ref).abs().max())
    assert err <= 2.0 * e32 + 1e-7 * float(ref.abs().max()), (kernel, C, M, N, err, e32)
    rs_ref = ref.sum(-1).reshape(-1)
    rs_err, rs_e32 = float((rowsum.double().cpu() - rs_ref).abs().max()), float((y32.sum(-1).reshape(-1).double() - rs_ref).abs().max())
    assert rs_err <= 2.0 * rs_e32 + 1e-7 * float(rs_ref.abs().max()), (kernel, C, M, N, rs_err, rs_e32)
    print("WIDEVAR gemm-%s C %d M %d N %d: max error %.3e (fp32 torch %.3e), row sums %.3e (fp32 torch %.3e)" % (kernel, C, M, N, err, e32, rs_err, rs_e32))
    # no output depends on the pad rows or their scales
    za, _ = _encode(a32, False)
    zb, _ = _encode(b32, False)
    out0, rowsum0 = capi.dense_corr_panels(za, images_a, zb, n_pairs, want_rowsum=True)
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and torch.equal(rowsum, rowsum0), "the outputs depend on the rows behind the last point"


# ------------------------------------------------------------------------------------------------ (c) adjoint and pointwise stages against fp64
SAMPLE_CASES = [("vec", 24, "cl"), ("vec-C1028", 1028, "cl"), ("scalar-odd", 65, "cl"), ("scalar-nchw", 24, "nchw"), ("scalar-align", 24, "slice1")]


def _groups(ref, zero_map=None):
    """The pixels whose own vector is zero receive the eps branch of norm() (g / 1e-10, ten orders of magnitude above the rest) from the
    rows that sample nothing else: they are compared at their own scale.  zero_map [B, C, H, W]: the map the gradient belongs to."""
    if zero_map is None:
        return [("all", np.ones(ref.shape, bool))]
    eps = np.broadcast_to(~zero_map.any(axis=1, keepdims=True), ref.shape)
    assert eps.any() and np.abs(ref[eps]).max() > EPS_GROUP > np.abs(ref[~eps]).max()
    return [("eps", eps), ("rest", ~eps)]


def _rule(tag, got, ref, y32, floor_frac, extra=0.0, zero_map=None):
    """kernel error <= 2 x fp32 torch's + floor_frac x the data's largest magnitude, per magnitude group; returns the figures"""
    out = []
    for gname, m in _groups(ref, zero_map):
        scale = float(np.abs(ref[m]).max()) if m.any() else 0.0
        err, e32 = float(np.abs(got - ref)[m].max()), float(np.abs(y32 - ref)[m].max())
        out.append((gname, err, e32, scale))
        assert err <= 2.0 * e32 + floor_frac * scale + extra, (tag, gname, err, e32, scale)
    return out


@pytest.mark.parametrize("name,C,layout", SAMPLE_CASES)
def test_sample_and_its_adjoint_against_fp64(name, C, layout):
    B, H, W, S = 2, 5, 9, 13
    rng = np.random.default_rng(40 + C)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    coords = T.edge_coords(rng, B, S, H, W)
    t, co = _layout(x, layout), torch.from_numpy(coords).to(DEV)
    for idx in (None, [1, 1, 0, 1]):
        n = B if idx is None else len(idx)
        ti = None if idx is None else torch.tensor(idx, device=DEV)
        got = capi.sample(t, co, ti)
        torch.cuda.synchronize()
        ref = _sample64(x, coords, idx)
        y32 = _sample32(t, co, idx).reshape(n, S, S, C).permute(0, 3, 1, 2).double().cpu().numpy()
        # a blend of four taps of weights <= 1 in fp32: a rounding per product and sum, 2^-22 of the largest input
        fig = _rule(name + " sample", got.double().cpu().numpy(), ref, y32, 2.0 ** -22)
        # the adjoint: atomic adds in any order - compared to rounding, with the same rule
        g = rng.standard_normal((n, C, S, S)).astype(np.float32)
        d = capi.sample_bwd(torch.from_numpy(g).to(DEV), t, co, ti)
        torch.cuda.synchronize()
        gi = O.sample_bwd((n, C, H, W), coords.astype(np.float64)[np.arange(n) % B], g.astype(np.float64))
        dref = np.zeros((B, C, H, W))
        np.add.at(dref, np.arange(n) if idx is None else np.asarray(idx), gi)
        leaf = t.detach().clone().requires_grad_(True)
        src = leaf if idx is None else leaf[ti]
        F.grid_sample(src, co[torch.arange(n, device=DEV) % B].permute(0, 2, 1, 3), padding_mode="border", align_corners=True).backward(torch.from_numpy(g).to(DEV))
        dgot = d.double().cpu().numpy()
        assert not dgot[dref == 0].any(), name + ": a pixel no tap touches got a gradient"
        # up to P N terms land on a border pixel: fp32 sums of them, 2^-22 of the largest sum per term order
        fig += _rule(name + " sample_bwd", dgot, dref, leaf.grad.double().cpu().numpy(), 2.0 ** -22)
        print("WIDEVAR %s index %s: %s" % (name, idx is not None, "; ".join("%s err %.3e fp32 torch %.3e" % f[:3] for f in fig)))


@pytest.mark.parametrize("name,C,layout", [("cl", 24, "cl"), ("nchw", 24, "nchw"), ("K1", 1, "cl"), ("K127", 127, "cl")])
def test_sample_bwd_rows_with_and_without_the_backward_of_norm_against_fp64(name, C, layout):
    M, H, W, S = 2, 5, 9, 13
    P = S * S
    rng = np.random.default_rng(60 + C)
    x = rng.standard_normal((M, C, H, W)).astype(np.float32)
    x[0, :, 0:3, 2:7] = 0.0                                     # zero rows: inv = 1e10, the eps branch
    coords = T.edge_coords(rng, M, S, H, W)
    co = torch.from_numpy(coords).to(DEV)
    for idx in (None, [1, 0, 0]):
        n = M if idx is None else len(idx)
        ti = None if idx is None else torch.tensor(idx, device=DEV)
        dest = np.arange(n) if idx is None else np.asarray(idx)
        s64 = _rows(_sample64(x, coords, idx))
        nrm = np.sqrt((s64 * s64).sum(-1))
        rows_n = (s64 / np.maximum(nrm, 1e-10)[..., None]).astype(np.float32)          # the kernel's inputs: what stego_sample_panels saves
        inv = (1.0 / np.maximum(nrm, 1e-10)).astype(np.float32)
        assert (inv == np.float32(1e10)).any()
        g = rng.standard_normal((n, P, C)).astype(np.float32)
        for with_norm in (False, True):
            d_map = _layout(np.zeros((M, C, H, W), np.float32), layout)
            capi.sample_bwd_rows(torch.from_numpy(g).to(DEV), d_map, co, ti,
                                 torch.from_numpy(rows_n).to(DEV) if with_norm else None, torch.from_numpy(inv).to(DEV) if with_norm else None)
            torch.cuda.synchronize()

            def statement(dt, tdev=None):
                """d rows = inv (g - rows_n <rows_n, g>), inv g on the eps branch (include/stego_corr.h); then the adjoint of the sampling"""
                if tdev is None:
                    gg, y, iv = g.astype(dt), rows_n.astype(dt), inv.astype(dt)
                    v = gg
                    if with_norm:
                        proj = np.where(iv > 0.99e10, 0.0, (y * gg).sum(-1))
                        v = iv[..., None] * (gg - y * proj[..., None])
                    gi = O.sample_bwd((n, C, H, W), coords.astype(dt)[np.arange(n) % M], np.moveaxis(v.reshape(n, S, S, C), -1, 1))
                    out = np.zeros((M, C, H, W), dt)
                    np.add.at(out, dest, gi)
                    return out
                gg, y, iv = (torch.from_numpy(a).to(DEV) for a in (g, rows_n, inv))
                v = gg
                if with_norm:
                    proj = torch.where(iv > 0.99e10, torch.zeros_like(iv), (y * gg).sum(-1))
                    v = iv[..., None] * (gg - y * proj[..., None])
                leaf = torch.zeros(M, C, H, W, device=DEV, requires_grad=True)
                src = leaf if idx is None else leaf[ti]
                F.grid_sample(src, co[torch.arange(n, device=DEV) % M].permute(0, 2, 1, 3), padding_mode="border",
                              align_corners=True).backward(v.reshape(n, S, S, C).permute(0, 3, 1, 2))
                return leaf.grad.double().cpu().numpy()

            ref, y32 = statement(np.float64), statement(None, True)
            got = d_map.double().cpu().numpy()
            assert np.isfinite(got).all() and not got[ref == 0].any(), name
            # fp32 sums of up to P N terms per pixel in any order (atomics): 2^-22 of the group's largest sum
            fig = _rule("%s rows norm %s" % (name, with_norm), got, ref, y32, 2.0 ** -22, zero_map=x if with_norm else None)
            print("WIDEVAR sample_bwd_rows-%s index %s norm %s: %s" % (name, idx is not None, with_norm,
                                                                      "; ".join("%s err %.3e fp32 torch %.3e (scale %.2e)" % f for f in fig)))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 169])
@pytest.mark.parametrize("pointwise", [True, False])
def test_pointwise_stages_against_fp64_with_cd_on_both_clamp_bounds(P, pointwise):
    n_sets, B = 4, 2
    cmin, cmax = 0.0, float(np.float32(0.8))                                 # (the bound the kernel compares with: 0.8f)
    shifts = (0.18, 0.12, 0.46)
    rng = np.random.default_rng(P)
    fd = (rng.standard_normal((n_sets, B, P, P)) * 0.3).astype(np.float32)
    cd = (rng.random((n_sets, B, P, P)) * 2 - 1).astype(np.float32)
    flat = cd.reshape(-1)
    k = max(1, flat.size // 7)
    where = rng.permutation(flat.size)
    f32 = np.float32
    flat[where[:k]] = f32(cmin)                                             # exactly on the bounds: the mask is inclusive
    flat[where[k:2 * k]] = f32(cmax)
    flat[where[2 * k:3 * k]] = np.nextafter(f32(cmax), f32(2))               # one ulp outside
    flat[where[3 * k:4 * k]] = f32(-1e-30)
    lib = capi.load()
    tfd, tcd = torch.from_numpy(fd).to(DEV), torch.from_numpy(cd).to(DEV)
    neg_loss, sums, rowsum, old_mean = capi.loss_pointwise_fwd(tfd, tcd, shifts, cmin, cmax, pointwise)
    g_neg = (rng.standard_normal((n_sets - 2, B, P, P))).astype(np.float32)
    g_sums = rng.standard_normal(n_sets).astype(np.float32)
    g_bc = f32(0.37)
    tg_neg, tg_sums, tg_bc = torch.from_numpy(g_neg).to(DEV), torch.from_numpy(g_sums).to(DEV), torch.full((1,), float(g_bc), device=DEV)
    g_cd = torch.full_like(tcd, float("nan"))
    capi._check(lib.stego_loss_pointwise_bwd(tfd.data_ptr(), tcd.data_ptr(), rowsum.data_ptr(), old_mean.data_ptr(), n_sets, B, P,
                                             (c_float * 3)(*shifts), cmin, cmax, 1 if pointwise else 0, tg_neg.data_ptr(), tg_bc.data_ptr(),
                                             tg_sums.data_ptr(), g_cd.data_ptr(), capi._stream()))
    torch.cuda.synchronize()

    def statement(xp, fdv, cdv, gn, gs, gb, sh):
        """modules.py:330-345 per pair-set and its backward towards cd, dense + broadcast + per-set upstreams together"""
        w = fdv
        if pointwise:
            w = (fdv - fdv.mean(-1, keepdims=True) if xp is np else fdv - fdv.mean(-1, keepdim=True))
            w = w + (fdv.mean((1, 2, 3), keepdims=True) if xp is np else fdv.mean((1, 2, 3), keepdim=True))
        w = w - sh
        loss = -(xp.clip(cdv, cmin, cmax) if xp is np else cdv.clamp(cmin, cmax)) * w
        up = gs.reshape(-1, 1, 1, 1) + xp.zeros_like(cdv)
        up[2:] = up[2:] + gn + gb
        mask = (cdv >= cmin) & (cdv <= cmax)
        return loss, -(w * mask) * up

    sh64 = np.asarray([shifts[0], shifts[1]] + [shifts[2]] * (n_sets - 2), np.float32).astype(np.float64).reshape(-1, 1, 1, 1)
    loss64, gcd64 = statement(np, fd.astype(np.float64), cd.astype(np.float64), g_neg.astype(np.float64), g_sums.astype(np.float64), float(g_bc), sh64)
    sh32 = torch.from_numpy(sh64.astype(np.float32)).to(DEV)
    loss32, gcd32 = statement(torch, tfd, tcd, tg_neg, tg_sums, tg_bc, sh32)
    # floors: w = fd - rowmean + old_mean - shift carries a rounding of each term (2^-24 of the largest, four terms), times |clamp(cd)| <= 1
    wscale = float(np.abs(fd).max()) + max(shifts)
    fl = 4 * 2.0 ** -24 * wscale
    e = float(np.abs(neg_loss.double().cpu().numpy() - loss64[2:]).max())
    e32 = float(np.abs(loss32[2:].double().cpu().numpy() - loss64[2:]).max())
    assert e <= 2.0 * e32 + fl, (P, pointwise, e, e32)
    # sums of B P P terms in fp32: the worst case of a chunked pairwise sum is (P / 64 + log2) roundings of the sum of the magnitudes
    s64, s32 = loss64.sum((1, 2, 3)), loss32.sum((1, 2, 3)).double().cpu().numpy()
    es, es32 = float(np.abs(sums.double().cpu().numpy() - s64).max()), float(np.abs(s32 - s64).max())
    assert es <= 2.0 * es32 + 2.0 ** -24 * (P / 64 + 26) * float(np.abs(loss64).sum((1, 2, 3)).max()) + fl * B * P * P, (P, pointwise, es, es32)
    got = g_cd.double().cpu().numpy()
    assert np.isfinite(got).all()
    assert not got[gcd64 == 0].any() and got[(cd == f32(cmin)) | (cd == f32(cmax))].all(), "the clamp's pass mask is inclusive on both bounds"
    eg, eg32 = float(np.abs(got - gcd64).max()), float(np.abs(gcd32.double().cpu().numpy() - gcd64).max())
    upscale = float(np.abs(g_neg).max() + np.abs(g_sums).max() + abs(g_bc))
    assert eg <= 2.0 * eg32 + (fl + 3 * 2.0 ** -24 * wscale) * upscale, (P, pointwise, eg, eg32)
    print("WIDEVAR pointwise P %d pointwise %s: loss %.3e (fp32 torch %.3e), sums %.3e (%.3e), d cd %.3e (%.3e)" % (P, pointwise, e, e32, es, es32, eg, eg32))


# ------------------------------------------------------------------------------------------------ (d) every table row end to end
def _cfg(case):
    S, n_neg = case.shape[5:]
    return O.CorrCfg(pointwise=case.pointwise, zero_clamp=case.cfg != "noclamp", stabalize=case.cfg == "stab", feature_samples=S, neg_samples=n_neg)


def _wide_offsets(lib, desc):
    """The forward workspace and the saved context of wide_geometry (csrc/corr_wide.hip), restated to find the operand images; the totals
    must be the library's, so a changed layout fails here and is not misread."""
    B, C, K, S, n_neg = desc.B, desc.C, desc.K, desc.S, desc.n_neg
    n_img, P = (2 + n_neg) * B, S * S
    nb = (P + 127) // 128
    fimg, cimg = int(lib.stego_panel_image_bytes(C, P)), int(lib.stego_panel_image_bytes(K, P))
    rows = n_img * P
    o = dict(fimg=fimg, cimg=cimg, n_img=n_img, P=P, nb=nb)
    o["c_inv"] = _up256(rows * K * 4)
    ctx_bytes = o["c_inv"] + _up256(rows * 4) + 2 * _up256(B * P * 8)
    off = 0
    for key, size in (("fpan", n_img * fimg), ("frs", n_img * nb * 128 * 4), ("cpan", n_img * cimg), ("crs", n_img * nb * 128 * 4),
                      ("rowsum", rows * 4), ("lrowsum", rows * 4), ("mean", 256), ("fd", rows * P * 4), ("ctx", ctx_bytes)):
        o[key] = off
        off += _up256(size)
    assert off + 256 == int(lib.stego_corr_workspace_bytes(byref(desc))) and ctx_bytes == int(lib.stego_corr_saved_ctx_bytes(byref(desc)))
    return o


class _Row:
    """One forward of a table row through stego_corr_fwd on buffers of the test's own, all of them poisoned; backward() as often as wanted."""

    def __init__(self, case):
        self.case = case
        B, C, H, W, K, S, n_neg = case.shape
        self.d = d = T.make_inputs(case)
        self.cfg = cfg = _cfg(case)
        self.desc = capi.make_desc(B, C, K, H, W, S, n_neg, cfg, (cfg.pos_intra_shift, cfg.pos_inter_shift, cfg.neg_inter_shift), capi.PREC_F16X3)
        self.lib = lib = capi.load()
        self.maps = [_layout(d["feats"], case.flayout), _layout(d["feats_pos"], case.flayout), _layout(d["code"], case.clayout),
                     _layout(d["code_pos"], case.clayout)]
        self.co1, self.co2 = torch.from_numpy(d["coords1"]).to(DEV), torch.from_numpy(d["coords2"]).to(DEV)
        self.perms = torch.from_numpy(d["perms"]).to(DEV) if n_neg else None
        nan = dict(dtype=torch.float32, device=DEV)
        P = S * S
        self.lm = torch.full((3,), float("nan"), **nan)
        self.icd, self.ecd = torch.full((B, P * P), float("nan"), **nan), torch.full((B, P * P), float("nan"), **nan)
        self.nl = torch.full((n_neg * B, P * P), float("nan"), **nan) if n_neg else None         # n_neg == 0: null pointers
        self.ncd = torch.full((n_neg * B, P * P), float("nan"), **nan) if n_neg else None
        self.saved_w = torch.full(((2 + n_neg) * B, P * P), float("nan"), **nan)
        self.saved_mean = torch.full((2 + n_neg,), float("nan"), **nan)
        self.ctx = torch.full((int(lib.stego_corr_saved_ctx_bytes(byref(self.desc))),), 0xFF, dtype=torch.uint8, device=DEV)
        self.ws = torch.full((int(lib.stego_corr_workspace_bytes(byref(self.desc))),), 0xFF, dtype=torch.uint8, device=DEV)
        assert self.ws.data_ptr() % 256 == 0 and self.ctx.data_ptr() % 256 == 0
        m = [capi._map(t) for t in self.maps]
        capi._check(lib.stego_corr_fwd(byref(self.desc), *[byref(x) for x in m], self.co1.data_ptr(), self.co2.data_ptr(), capi._ptr(self.perms),
                                       self.lm.data_ptr(), self.icd.data_ptr(), self.ecd.data_ptr(), capi._ptr(self.nl), capi._ptr(self.ncd),
                                       self.saved_w.data_ptr(), self.saved_mean.data_ptr(), self.ctx.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                       capi._stream()))
        torch.cuda.synchronize()
        self.bwd_ws_bytes = int(lib.stego_corr_bwd_workspace_bytes(byref(self.desc)))

    def upstreams(self, neg_is_mean=False):
        """(g_intra, g_inter, g_neg, stride, g_intra_cd, g_inter_cd, g_neg_cd): dense tensors on all six outputs, or the scalars of training"""
        B, C, H, W, K, S, n_neg = self.case.shape
        if self.case.dense:
            u = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in self.d["ups"]]
            return u[0], u[2], (u[4] if n_neg else None), 1, u[1], u[3], (u[5] if n_neg else None)
        gi, ge = torch.tensor(0.67, device=DEV), torch.tensor(0.25, device=DEV)
        if not n_neg:
            return gi, ge, None, 1, None, None, None
        if neg_is_mean:
            return gi, ge, torch.full((1,), 0.63, device=DEV), -1, None, None, None
        return gi, ge, torch.full((1,), 0.63 / (n_neg * B * S ** 4), device=DEV), 0, None, None, None

    def backward(self, neg_is_mean=False):
        B, C, H, W, K, S, n_neg = self.case.shape
        gi, ge, gn, stride, gicd, gecd, gncd = self.upstreams(neg_is_mean)
        d_code = torch.full((B, H, W, K), float("nan"), device=DEV)
        d_code_pos = torch.full((B, H, W, K), float("nan"), device=DEV)
        ws = torch.full((self.bwd_ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
        capi._check(self.lib.stego_corr_bwd(byref(self.desc), capi._ptr(self.perms), self.saved_w.data_ptr(), self.saved_mean.data_ptr(), self.ctx.data_ptr(),
                                            self.icd.data_ptr(), self.ecd.data_ptr(), capi._ptr(self.ncd), capi._ptr(gi), capi._ptr(ge), capi._ptr(gn), stride,
                                            capi._ptr(gicd), capi._ptr(gecd), capi._ptr(gncd), d_code.data_ptr(), d_code_pos.data_ptr(), ws.data_ptr(),
                                            ws.numel(), capi._stream()))
        torch.cuda.synchronize()
        return d_code.permute(0, 3, 1, 2).cpu().numpy(), d_code_pos.permute(0, 3, 1, 2).cpu().numpy()


def _oracle(case, d, cfg):
    B, C, H, W, K, S, n_neg = case.shape
    args = (d["feats"], d["feats_pos"], d["code"], d["code_pos"], d["coords1"], d["coords2"], d["perms"], cfg)
    fwd = O.corr_loss_forward(*args)
    if case.dense:
        u = d["ups"]
        bwd = O.corr_loss_backward(*args, float(u[0]), float(u[2]), u[4], g_intra_cd=u[1], g_inter_cd=u[3], g_neg_cd=u[5])
    else:
        bwd = O.corr_loss_backward(*args, 0.67, 0.25, np.full((n_neg * B, S, S, S, S), 0.63 / max(n_neg * B * S ** 4, 1)))
    return fwd, bwd


def _k1_scale_and_touched(case, d, cfg):
    """K = 1: a normalised row is +-1 and the backward of norm() projects every gradient to zero - the fp64 gradients are zero EVERYWHERE, by
    cancellation.  What rounding leaves of them is relative to the gradients in front of the projection: their largest magnitude (the
    oracle's backward with the projection taken out), and the pixels a tap touches at all."""
    B, C, H, W, K, S, n_neg = case.shape
    keep = O._normalize_bwd
    O._normalize_bwd = lambda t, g: g / np.maximum(np.sqrt((t * t).sum(axis=1, keepdims=True)), 1e-10)
    try:
        scale = max(float(np.abs(g).max()) for g in _oracle(case, d, cfg)[1])
    finally:
        O._normalize_bwd = keep
    one = np.ones((B, 1, S, S))
    t1 = O.sample_bwd((B, 1, H, W), d["coords1"].astype(np.float64), one)
    t2 = O.sample_bwd((B, 1, H, W), d["coords2"].astype(np.float64), one)
    for perm in d["perms"]:
        np.add.at(t1, perm, t2)
    return scale, (t1 > 0, t2 > 0)


def _torch32(case, d, cfg):
    """oracle/torch_cpu_port.py in float32 on the same inputs, forward and (autograd) backward with the row's upstreams: the yardstick"""
    B, C, H, W, K, S, n_neg = case.shape
    t = {k: torch.from_numpy(d[k]) for k in ("feats", "feats_pos", "coords1", "coords2")}
    code, code_pos = torch.from_numpy(d["code"]).requires_grad_(True), torch.from_numpy(d["code_pos"]).requires_grad_(True)
    out = PORT.corr_loss_torch_cpu(t["feats"], t["feats_pos"], code, code_pos, t["coords1"], t["coords2"], [torch.from_numpy(p) for p in d["perms"]], cfg)
    if case.dense:
        ups = [torch.from_numpy(np.ascontiguousarray(u)) for u in d["ups"]]
    else:
        ups = [torch.tensor(0.67), None, torch.tensor(0.25), None, torch.full_like(out[4], 0.63 / max(n_neg * B * S ** 4, 1)), None]
    total = sum((o * u).sum() for o, u in zip(out, ups) if u is not None and o.numel())
    total.backward()
    return [o.detach().double().numpy() for o in out], (code.grad.double().numpy(), code_pos.grad.double().numpy())


def _loss_scale(fwd, cfg):
    """mean |loss element| per pair-set kind: what an error of a returned mean is relative to"""
    lo, hi = O._clamp_bounds(cfg)
    shifts = (cfg.pos_intra_shift, cfg.pos_inter_shift)
    cds = (fwd.pos_intra_cd, fwd.pos_inter_cd)
    s = [float(np.abs(np.clip(cds[i], lo, hi) * (fwd.fd[i] - shifts[i])).mean()) for i in range(2)]
    return s + [float(np.abs(fwd.neg_inter_loss).mean()) if fwd.neg_inter_loss.size else 1.0]


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_wide_row_end_to_end_against_the_fp64_oracle(name):
    case = BY_NAME[name]
    B, C, H, W, K, S, n_neg = case.shape
    P = S * S
    row = _Row(case)
    d, cfg, lib = row.d, row.cfg, row.lib
    fwd, (dc, dcp) = _oracle(case, d, cfg)
    y_out, y_grad = _torch32(case, d, cfg)
    figs = []
    # (stego_corr_fwd_launches counts the kernels of corr_wide.hip itself: the row-sum launch behind the tile GEMM, which corr_wide_plan.h
    # counts too, is not among them)
    assert capi.corr_fwd_launches(row.desc, *row.maps) == (3 if n_neg else 2) + 5

    # ---- the operand images of the three sampler launches, straight from the poisoned workspace: sample_panels_kernel<VW1, VW2>
    o = _wide_offsets(lib, row.desc)
    n_img = o["n_img"]
    x = {k: d[k] for k in ("feats", "feats_pos", "code", "code_pos")}
    idx = [int(v) for v in d["perms"].reshape(-1)]
    srcs = [("feats", "code", "coords1", None), ("feats_pos", "code_pos", "coords2", None)] + ([("feats", "code", "coords2", idx)] if n_neg else [])
    t_dev = dict(zip(("feats", "feats_pos", "code", "code_pos"), row.maps))
    co_dev = {"coords1": row.co1, "coords2": row.co2}
    ref_rows = {0: [], 1: []}
    t32_rows = {0: [], 1: []}
    inv32 = []
    for fk, ck, cok, ix in srcs:
        for side, key in ((0, fk), (1, ck)):
            s64 = _rows(_sample64(x[key], d[cok], ix))
            ref_rows[side].append(s64)
            s32 = _sample32(t_dev[key], co_dev[cok], ix)
            t32_rows[side].append(F.normalize(s32, dim=2, eps=1e-10).double().cpu().numpy())
            if side == 1:
                inv32.append((1.0 / s32.norm(dim=2).clamp_min(1e-10)).double().cpu().numpy())
    for side, (pan, rs, img_bytes, ch, label) in enumerate((("fpan", "frs", o["fimg"], C, "features"), ("cpan", "crs", o["cimg"], K, "codes"))):
        s64 = np.concatenate(ref_rows[side])
        nrm = np.sqrt((s64 * s64).sum(-1))
        ref_n = s64 / np.maximum(nrm, 1e-10)[..., None]
        zero_rows = ~s64.any(-1)
        if case.recipe == "zeros":
            assert zero_rows.any(), name + ": the zero blocks catch no point"
        raw, dec = _decode(row.ws[o[pan]:o[pan] + n_img * img_bytes], row.ws[o[rs]:o[rs] + n_img * o["nb"] * 512].view(torch.float32), n_img, ch, P)
        err, e32 = _check_panel_rows("%s %s" % (name, label), raw, dec, P, ch, ref_n, np.concatenate(t32_rows[side]), zero_rows)
        figs.append("%s rows %.3e (fp32 torch %.3e)" % (label, err, e32))
        if side == 1:
            # the saved context: the codes' normalised fp32 rows and 1 / max(|row|, eps)
            cn = row.ctx[:n_img * P * K * 4].view(torch.float32).view(n_img, P, K).double().cpu().numpy()
            inv = row.ctx[o["c_inv"]:o["c_inv"] + n_img * P * 4].view(torch.float32).view(n_img, P).double().cpu().numpy()
            ecn = np.abs(cn - ref_n).max(-1)
            assert (ecn <= 2.0 * e32 + 2.0 ** -23 * np.abs(ref_n).max(-1)).all(), (name, float(ecn.max()), e32)
            assert (inv[zero_rows] == np.float32(1e10)).all()
            live = ~zero_rows
            einv, e32inv = np.abs(inv[live] * nrm[live] - 1).max(), np.abs(np.concatenate(inv32)[live] * nrm[live] - 1).max()
            assert einv <= 2.0 * e32inv + 2.0 ** -23, (name, einv, e32inv)

    # ---- the six outputs
    got = [float(row.lm[0]), row.icd.cpu().numpy().reshape(fwd.pos_intra_cd.shape), float(row.lm[1]), row.ecd.cpu().numpy().reshape(fwd.pos_inter_cd.shape),
           row.nl.cpu().numpy().reshape(fwd.neg_inter_loss.shape) if n_neg else np.zeros(fwd.neg_inter_loss.shape, np.float32),
           row.ncd.cpu().numpy().reshape(fwd.neg_inter_cd.shape) if n_neg else np.zeros(fwd.neg_inter_cd.shape, np.float32)]
    exp = fwd.as_tuple()
    scale = _loss_scale(fwd, cfg)
    for i, what in ((1, "pos_intra_cd"), (3, "pos_inter_cd"), (4, "neg_inter_loss"), (5, "neg_inter_cd")):
        if not exp[i].size:
            continue
        assert np.isfinite(got[i]).all(), (name, what)
        assert_close(got[i], exp[i], rtol=1e-3, atol_frac=1e-3, what="%s %s" % (name, what))
        m = float(np.abs(exp[i]).max())
        if m == 0.0:
            # (a map of one pixel whose negative has a negative cd: every loss element is -0 x w)
            assert not got[i].any(), (name, what)
            continue
        err, e32 = float(np.abs(got[i] - exp[i]).max()) / m, float(np.abs(y_out[i] - exp[i]).max()) / m
        figs.append("%s %.3e (%.3e)" % (what, err, e32))
        assert err <= 2.0 * e32 + 1e-6, (name, what, err, e32)
    for i, k, what in ((0, 0, "pos_intra_loss"), (2, 1, "pos_inter_loss")):
        err, e32 = abs(got[i] - float(exp[i])) / scale[k], abs(float(y_out[i]) - float(exp[i])) / scale[k]
        figs.append("%s %.3e (%.3e)" % (what, err, e32))
        assert abs(got[i] - float(exp[i])) <= 1e-3 * scale[k] + 1e-3 * abs(float(exp[i])), (name, what, got[i], float(exp[i]))
        assert err <= 2.0 * e32 + 1e-6, (name, what, err, e32)
    lm2 = float(row.lm[2])
    if n_neg and scale[2] == 0.0:
        assert lm2 == 0.0, (name, lm2)
    elif n_neg:
        e_mean = float(exp[4].mean())
        err, e32 = abs(lm2 - e_mean) / scale[2], abs(float(y_out[4].mean()) - e_mean) / scale[2]
        figs.append("neg mean %.3e (%.3e)" % (err, e32))
        assert err <= 2.0 * e32 + 1e-6, (name, "loss_means[2]", err, e32)
    else:
        assert lm2 == 0.0, "loss_means[2] is 0 when n_neg == 0 (include/stego_corr.h)"

    # ---- both gradients, on a poisoned workspace; twice
    a, b = row.backward(), row.backward()
    k1 = _k1_scale_and_touched(case, d, cfg) if K == 1 else None
    runs = [("", a)] + ([("mean-upstream ", row.backward(neg_is_mean=True))] if n_neg and not case.dense else [])
    for tag, g2 in runs:
        for g, e, y, what in zip(g2, (dc, dcp), y_grad, ("d_code", "d_code_pos")):
            assert np.isfinite(g).all(), (name, what)
            if k1 is not None:
                # y = x / |x| (two roundings), <y, g>, y <y, g> and the difference: at most eight roundings of the unprojected gradient, 2^-21 of it
                assert not e.any() and not g[~np.broadcast_to(k1[1][what == "d_code_pos"], g.shape)].any(), (name, what)
                err, e32 = float(np.abs(g).max()), float(np.abs(y).max())
                figs.append("%s%s |g| %.3e (fp32 torch %.3e; unprojected %.3e)" % (tag, what, err, e32, k1[0]))
                assert err <= 2.0 * e32 + 2.0 ** -21 * k1[0], (name, tag + what, err, e32, k1[0])
                continue
            # a pixel no tap touches carries neither stale workspace nor another image's row
            assert not g[e == 0].any(), (name, what, int(np.count_nonzero(g[e == 0])))
            zero_map = d["code" if what == "d_code" else "code_pos"] if case.recipe == "zeros" else None
            for gname, m in _groups(e, zero_map):
                assert_close(g[m], e[m], rtol=1e-3, atol_frac=1e-3, what="%s %s%s %s" % (name, tag, what, gname))
                s = float(np.abs(e[m]).max())
                err, e32 = float(np.abs(g - e)[m].max()) / s, float(np.abs(y - e)[m].max()) / s
                figs.append("%s%s[%s] %.3e (%.3e)" % (tag, what, gname, err, e32))
                assert err <= 2.0 * e32 + 1e-6, (name, tag + what, gname, err, e32)
    if case.variants[3] == "bwd:gather":
        for xg, yg in zip(a, b):
            assert np.array_equal(xg, yg), name + ": not repeatable"
    else:
        # the scatter adds with fp32 atomics in arrival order: rounding of the sums, nothing more
        for xg, yg, e in zip(a, b, (dc, dcp)):
            assert float(np.abs(xg - yg).max()) <= 1e-6 * float(np.abs(e).max()), name
    print("WIDEVAR %s %s: %s" % (name, " ".join(case.variants), "; ".join(figs)))
