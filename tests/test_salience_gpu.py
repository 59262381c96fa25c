"""The salience-guided coordinate draws on the MI355X: stego_salience_coords (include/stego_salience.h) against a torch restatement
bit for bit, and ContrastiveCorrelationLoss.draw() / forward() with cfg.native_salience."""
import types

import pytest
import torch

from stego_amd import capi
from stego_amd import modules as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ALMOST_ONE = 1.0 - 2.0 ** -24


def _masks(B, H, W, kind, seed):
    """uint8 [B, H, W] patterns, one per image (cycled): all zero, all ones, 30 % random, a single nonzero at the first pixel, one at
    the last, nonzeros only in the last (partial) 64-pixel chunk - or `kind` for the whole batch."""
    g = torch.Generator().manual_seed(seed)
    n = H * W
    m = torch.zeros(B, n, dtype=torch.uint8)
    kinds = ["random", "ones", "zeros", "first", "last", "tail"] if kind == "mixed" else [kind]
    for b in range(B):
        k = kinds[b % len(kinds)]
        if k == "ones":
            m[b] = 1
        elif k == "random":
            m[b] = (torch.rand(n, generator=g) < 0.3).to(torch.uint8) * 3          # any nonzero byte counts
        elif k == "first":
            m[b, 0] = 1
        elif k == "last":
            m[b, n - 1] = 255
        elif k == "tail":
            start = (n - 1) // 64 * 64
            m[b, start:] = (torch.rand(n - start, generator=g) < 0.5).to(torch.uint8)
            m[b, n - 1] = 1
    return m.reshape(B, H, W)


def _uniforms(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(2, B, S, S, 3, generator=g)
    u.view(-1)[0::7] = 0.0
    u.view(-1)[3::11] = ALMOST_ONE
    u[:, :, 0, 0, :] = 0.0
    u[:, :, -1, -1, :] = ALMOST_ONE
    u_mix = torch.rand(B, S, S, generator=g)
    flat = u_mix.view(-1)
    flat[0::5] = 0.1                                   # float32(0.1) itself: not > 0.1f, keeps reg
    flat[1::5] = torch.nextafter(torch.tensor(0.1), torch.tensor(1.0))
    flat[2::5] = torch.nextafter(torch.tensor(0.1), torch.tensor(0.0))
    reg1 = torch.rand(B, S, S, 2, generator=g) * 2 - 1
    reg2 = torch.rand(B, S, S, 2, generator=g) * 2 - 1
    assert float(u.max()) < 1.0
    return u, u_mix, reg1, reg2


def _restated(mask, u, u_mix, reg):
    """One side on the CPU: torch.nonzero(mask[b])[r] with the header's fp32 expressions for r and nz."""
    B, H, W = mask.shape
    S = u_mix.shape[1]
    fH = torch.tensor(float(H), dtype=torch.float32)
    out = torch.empty(B, S * S, 2, dtype=torch.float32)
    uu, mix, rr = u.reshape(B, S * S, 3), u_mix.reshape(B, S * S), reg.reshape(B, S * S, 2)
    for b in range(B):
        nz = torch.nonzero(mask[b])                                                   # row-major (y, x)
        c = nz.shape[0]
        if c > 0:
            r = torch.clamp((uu[b, :, 0] * torch.tensor(float(c), dtype=torch.float32)).to(torch.int32), max=c - 1).long()
            y, x = nz[r, 0], nz[r, 1]
        else:
            y = torch.clamp((uu[b, :, 1] * fH).to(torch.int32), max=H - 1).long()
            x = torch.clamp((uu[b, :, 2] * fH).to(torch.int32), max=H - 1).long()
        pick = torch.stack([x.to(torch.float32) / fH * 2 - 1, y.to(torch.float32) / fH * 2 - 1], -1)
        out[b] = torch.where((mix[b] > 0.1).unsqueeze(-1), pick, rr[b])
    return out.reshape(B, S, S, 2)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(m1, m2, S, seed):
    B = m1.shape[0]
    u, u_mix, reg1, reg2 = _uniforms(B, S, seed)
    dev = [t.to(DEV) for t in (m1, m2, u, u_mix, reg1, reg2)]
    c1, c2 = capi.salience_coords(*dev)
    d1, d2 = capi.salience_coords(*dev)
    torch.cuda.synchronize()
    assert c1.dtype == torch.float32 and tuple(c1.shape) == (B, S, S, 2) == tuple(c2.shape)
    assert torch.equal(_bits(c1), _bits(d1)) and torch.equal(_bits(c2), _bits(d2))           # repeat launches
    e1, e2 = _restated(m1, u[0], u_mix, reg1), _restated(m2, u[1], u_mix, reg2)
    assert torch.equal(_bits(c1.cpu()), _bits(e1))
    assert torch.equal(_bits(c2.cpu()), _bits(e2))
    kept = (u_mix > 0.1)
    assert bool(kept.any()) and bool((~kept).any())                                         # both sides of the mix occur


SHAPES = [(3, 8, 8, 2),            # one chunk
          (2, 24, 24, 11),         # nine chunks
          (2, 37, 53, 11),         # non-square, chunks crossing rows, a partial last chunk
          (4, 224, 224, 11),
          (1, 1024, 1024, 16)]     # the limit: 16384 chunks, 256 blocks of chunks


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.bool])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_salience_coords_equal_the_torch_restatement(shape, dtype):
    B, H, W, S = shape
    for kind in (["mixed"] if H * W > 2 ** 16 else ["mixed", "zeros", "ones", "first", "last", "tail"]):
        # side 1 and side 2 see different patterns for the same image
        m1 = _masks(max(B, 6) if kind == "mixed" and H * W <= 2 ** 16 else B, H, W, kind, 1)
        m2 = torch.roll(_masks(m1.shape[0], H, W, kind, 2), 1, 0)
        _check(m1.to(dtype), m2.to(dtype), S, 10 + H)
    if H * W > 2 ** 16:                       # the large shapes: each single pattern once, on one side, beside a random one
        for kind in ("zeros", "first", "last", "tail", "ones"):
            _check(_masks(B, H, W, kind, 3).to(dtype), _masks(B, H, W, "random", 4).to(dtype), S, 20 + H)


def test_an_empty_image_between_two_full_ones_and_torch_s_rule_for_nonzero():
    B, H, W, S = 3, 24, 24, 11
    m = torch.ones(B, H, W, dtype=torch.uint8)
    m[1] = 0
    _check(m, m.flip(0).contiguous(), S, 5)
    _check(m.float(), m.float(), S, 6)
    # a float mask: -0.0 is zero; 1e-30, a negative value and NaN are not
    f = torch.zeros(B, H, W)
    f[0] = -0.0
    f[0, 3, 5], f[0, 23, 23], f[0, 7, 0] = 1e-30, -2.5, float("nan")
    f[1] = -0.0                                                                      # no nonzero at all: the fallback
    f[2, 0, 0], f[2, 11, 13] = float("nan"), 1e-30
    assert torch.nonzero(f[0]).shape[0] == 3 and torch.nonzero(f[1]).shape[0] == 0 and torch.nonzero(f[2]).shape[0] == 2
    _check(f, f.roll(1, 0).contiguous(), S, 7)


def _cfg(**kw):
    cfg = types.SimpleNamespace(feature_samples=11, neg_samples=5, pointwise=True, zero_clamp=True, stabalize=False, use_salience=True,
                                native_salience=True, pos_intra_shift=0.18, pos_inter_shift=0.12, neg_inter_shift=0.46,
                                pos_intra_weight=0.67, pos_inter_weight=0.25, neg_inter_weight=0.63)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _salience(B, H, seed):
    g = torch.Generator().manual_seed(seed)
    s1 = (torch.rand(B, H, H, generator=g) > 0.9).float()
    s2 = (torch.rand(B, H, H, generator=g) > 0.6).float()
    s1[1] = 0
    return s1.to(DEV), s2.to(DEV)


def test_native_draw_picks_nonzero_pixels_or_keeps_reg_and_repeats_from_a_seed():
    B, H, S = 4, 28, 11
    loss = M.ContrastiveCorrelationLoss(_cfg())
    feats = torch.zeros(B, 8, H, H, device=DEV)
    s1, s2 = _salience(B, H, 0)
    torch.cuda.manual_seed(7)
    c1, c2, perms = loss.draw(feats, s1, s2)
    torch.cuda.manual_seed(7)
    d1, d2, perms2 = loss.draw(feats, s1, s2)
    assert torch.equal(_bits(c1), _bits(d1)) and torch.equal(_bits(c2), _bits(d2)) and torch.equal(perms, perms2)
    assert tuple(c1.shape) == (B, S, S, 2) and tuple(perms.shape) == (5, B)
    # the draws in the documented order: rand, rand (the reg coordinates), the randperms, u, u_mix
    torch.cuda.manual_seed(7)
    reg1 = torch.rand(B, S, S, 2, device=DEV) * 2 - 1
    reg2 = torch.rand(B, S, S, 2, device=DEV) * 2 - 1
    for _ in range(5):
        torch.randperm(B, device=DEV)
    u = torch.rand(2, B, S, S, 3, device=DEV)
    u_mix = torch.rand(B, S, S, device=DEV)
    n_reg = n_nz = 0
    for c, reg, sal, side in ((c1, reg1, s1, 0), (c2, reg2, s2, 1)):
        c, reg, sal = c.cpu(), reg.cpu(), sal.cpu()
        is_reg = (_bits(c) == _bits(reg)).all(-1)
        assert torch.equal(is_reg | (u_mix.cpu() > 0.1), torch.ones_like(is_reg))
        x = torch.round((c[..., 0] + 1) / 2 * H).long().clamp(0, H - 1)
        y = torch.round((c[..., 1] + 1) / 2 * H).long().clamp(0, H - 1)
        exact = (x.float() / H * 2 - 1 == c[..., 0]) & (y.float() / H * 2 - 1 == c[..., 1])
        on_nz = torch.stack([sal[b][y[b], x[b]] != 0 for b in range(B)]) & exact
        empty = (sal.reshape(B, -1) != 0).sum(1) == 0                     # an image without salient pixels: any pixel of the grid
        ok = is_reg | on_nz | (exact & empty[:, None, None])
        assert bool(ok.all()), side
        n_reg += int((is_reg & ~on_nz).sum())
        n_nz += int((on_nz & ~is_reg).sum())
    assert n_reg > 0 and n_nz > 0                                         # both kinds occur
    # the torch path the flag replaces draws from the same masks when the key is off: unchanged from the same seed
    off = M.ContrastiveCorrelationLoss(_cfg(native_salience=False))
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    a1, a2 = off.draw_coords(feats, s1, s2)
    raw = [torch.randperm(B, device=DEV, dtype=torch.long) for _ in range(5)]
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    b1, b2, bp = off.draw(feats, s1, s2)
    assert torch.equal(_bits(a1), _bits(b1)) and torch.equal(_bits(a2), _bits(b2)) and torch.equal(bp, M._unfix(torch.stack(raw)))


def test_native_draw_makes_no_host_synchronisation():
    B, H = 4, 28
    loss = M.ContrastiveCorrelationLoss(_cfg())
    feats = torch.zeros(B, 8, H, H, device=DEV)
    s1, s2 = _salience(B, H, 1)
    loss.draw(feats, s1, s2)                     # the library is loaded and the allocator warm
    torch.cuda.synchronize()
    # where this torch build reports synchronising calls (it must flag a known one, .item()), the draw makes none
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=DEV).sum().item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            loss.draw(feats, s1, s2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode honoured:", honoured)
    torch.cuda.synchronize()
    # captured in a graph: a host synchronisation inside the draw would invalidate the capture
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        loss.draw(feats, s1, s2)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        c1, c2, perms = loss.draw(feats, s1, s2)
    g.replay()
    torch.cuda.synchronize()
    first = (c1.clone(), c2.clone(), perms.clone())
    g.replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(c1).all()) and float(c1.abs().max()) <= 1.0 and float(c2.abs().max()) <= 1.0
    assert not torch.equal(first[0], c1)         # the generator moves on between replays
    assert tuple(perms.shape) == (5, B) and int(perms.min()) >= 0 and int(perms.max()) < B


def test_forward_with_native_salience_on_a_fused_shape():
    B, C, K, H, S = 4, 384, 70, 28, 11
    g = torch.Generator().manual_seed(0)
    feats, feats_pos = (torch.randn(B, C, H, H, generator=g).to(DEV) for _ in range(2))
    code = torch.randn(B, K, H, H, generator=g).to(DEV).requires_grad_(True)
    code_pos = torch.randn(B, K, H, H, generator=g).to(DEV).requires_grad_(True)
    s1, s2 = _salience(B, 224, 2)
    assert M.ContrastiveCorrelationLoss.fused_kernels_cover(B, C, K, H, H, S, device=DEV, n_neg=5)
    loss = M.ContrastiveCorrelationLoss(_cfg())
    torch.cuda.manual_seed(1)
    out = loss(feats, feats_pos, s1, s2, code, code_pos)
    assert len(out) == 6 and all(bool(torch.isfinite(o).all()) for o in out)
    (out[0].mean() + out[2].mean() + out[4].mean()).backward()
    assert bool(torch.isfinite(code.grad).all()) and bool(torch.isfinite(code_pos.grad).all())
