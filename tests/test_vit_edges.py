"""The native ViT forward (stego_amd/csrc/vit_forward.hip) at the shapes where its tiling can go wrong, against the fp64 evaluation
of the same torch module.  Everything goes through the product path, ``vit_native.NativeViT(model, precision).forward_tokens(img)``;
a stage is isolated by the WEIGHTS of a depth-1 model (MODES below), never by a hook into the library.

Edges (the smallest shapes that reach them):
  * attention key padding: ntok = 2, 3, 63, 64 (no padding), 65 (a key tile with one live key), 129 (a query block with one live query);
  * GEMM column tiles: N in {64, 128, 256, 320, 448, 704} ends in a partial 192-column tile that starts at row 64 of a weight panel,
    hidden / 32 chunk panels leave the GELU epilogue in the order {0,1,3} / {2,4,5} with out_nkc no multiple of 6;
  * row tiles: M and B*hw at, just below and just above 256; stale (NaN) scratch in the panel rows >= M; an image that straddles a tile;
  * the float-reciprocal row -> (image, token) split up to its guard B * ntok < 2^20 (host arithmetic, one forward at M = 2^20 - 4, and
    ntok = 83 / hw = 82, whose float32 reciprocals are rounded down: without the + 0.5 the first row of image 1 lands in image 0).

Bars.  None comes from the kernel under test:
  * f16x3: relative L2 error against fp64 at most 2 x the fp32 torch module's own + 1e-7, worst element at most 3 x + 1e-6 - the bars
    of tests/test_vit_native.py (split operands carry 22 bits where fp32 carries 24: beyond 4 x the mode is not fp32 class);
  * f16: relative L2 against the fp32 module below max(2e-3, 1.05 x torch's fp16 autocast of the same model).
Every case prints its figures before it asserts.
"""
import functools
import zlib

import numpy as np
import pytest
import torch

from stego_amd import dino_vit, vit_native

MODES = {                       # mode -> (attn.proj zeroed, mlp.fc2 zeroed): weight AND bias
    "embed": (True, True),      # im2col, patch GEMM + bias + pos rows, class row, final LayerNorm (F16X3: the all-zero-tensor packing scale)
    "attn": (False, True),      # + LN1 -> panels, QKV GEMM + scatter, attention, proj GEMM with the residual epilogue
    "mlp": (True, False),       # + LN2, FC1 + GELU -> panels, FC2 with the residual epilogue
    "full": (False, False),
}
PRECISIONS = ("f16x3", "f16")


def build_model(patch, D, hidden, mode, seed):
    """Depth-1 ViT with DINO-like magnitudes, so that every stage moves the output (the 0.02 init leaves both branches at a few
    per cent of the residual): noise on every vector and on the class token, position table x 10, patch filter x 3, qkv x 4,
    proj x 40, fc1 x 10, fc2 x 10."""
    torch.manual_seed(seed)
    m = dino_vit.VisionTransformer(img_size=(4 * patch,), patch_size=patch, embed_dim=D, depth=1, num_heads=D // 64, mlp_ratio=hidden / D).eval()
    blk = m.blocks[0]
    assert blk.mlp.fc1.out_features == hidden, (D, hidden, blk.mlp.fc1.out_features)      # int(D * ratio) truncates
    assert vit_native.supported(m)
    with torch.no_grad():
        for name, prm in m.named_parameters():
            if prm.dim() == 1 or name == "cls_token":
                prm.add_(0.05 * torch.randn_like(prm))
        m.pos_embed.mul_(10.0)
        m.patch_embed.proj.weight.mul_(3.0)
        blk.attn.qkv.weight.mul_(4.0)
        blk.attn.proj.weight.mul_(40.0)
        blk.mlp.fc1.weight.mul_(10.0)
        blk.mlp.fc2.weight.mul_(10.0)
        no_attn, no_mlp = MODES[mode]
        if no_attn:
            blk.attn.proj.weight.zero_()
            blk.attn.proj.bias.zero_()
        if no_mlp:
            blk.mlp.fc2.weight.zero_()
            blk.mlp.fc2.bias.zero_()
    return m


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def branch_figures(m64, img64):
    """fp64 diagnostics of one block: RMS(attention branch) / RMS(residual), RMS(MLP branch) / RMS(residual), mean softmax entropy (nats)."""
    blk = m64.blocks[0]
    x0 = m64.prepare_tokens(img64)
    a, attn, _ = blk.attn(blk.norm1(x0), need_attn=True)
    x1 = x0 + a
    f = blk.mlp(blk.norm2(x1))
    ent = float(-(attn * attn.clamp_min(1e-300).log()).sum(-1).mean())
    return _rms(a) / _rms(x0), _rms(f) / _rms(x1), ent


def assert_case_tests_something(mode, ntok, figs):
    ra, rm, ent = figs
    if mode in ("attn", "full"):
        assert ra >= 0.3, ("attention branch too small to matter", ra)
        if ntok >= 63:
            assert ent > 0.5, ("one-hot attention: a wrong key mask would not move the output", ent)
    if mode in ("mlp", "full"):
        assert rm >= 0.3, ("MLP branch too small to matter", rm)


def _double_of(model):
    m64 = dino_vit.VisionTransformer(img_size=(model.patch_embed.img_size,), patch_size=model.patch_embed.patch_size, embed_dim=model.embed_dim,
                                     depth=1, num_heads=model.blocks[0].attn.num_heads,
                                     mlp_ratio=model.blocks[0].mlp.fc1.out_features / model.embed_dim).to(model.pos_embed.device).double().eval()
    assert m64.blocks[0].mlp.fc1.out_features == model.blocks[0].mlp.fc1.out_features
    m64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    return m64


def _errs(got, ref64):
    d = got.double() - ref64
    return float(d.norm() / ref64.norm()), float(d.abs().max())


@functools.lru_cache(maxsize=None)
def _case(patch, D, hidden, H, W, B, mode):
    """Model, input and the three torch evaluations (fp64, fp32, fp16 autocast) of one case: computed once, shared, never written to."""
    seed = _seed(patch, D, hidden, H, W, B, mode)
    model = build_model(patch, D, hidden, mode, seed).cuda()
    img = torch.randn(B, 3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
    with torch.no_grad():
        m64 = _double_of(model)
        ref64 = m64.get_intermediate_feat(img.double(), n=1)[0][0]
        figs = branch_figures(m64, img.double())
        ref32 = model.get_intermediate_feat(img, n=1)[0][0]
        with torch.autocast("cuda", dtype=torch.float16):
            half = model.get_intermediate_feat(img, n=1)[0][0].float()
    return model, img, ref64, ref32, half, figs


def check_against_fp64(tag, got_by_precision, ref64, ref32, half):
    """Prints every figure, then asserts the bars of the module docstring for each precision."""
    err32, worst32 = _errs(ref32, ref64)
    failures = []
    for precision, got in got_by_precision.items():
        assert got.shape == ref64.shape, (tag, precision, got.shape, ref64.shape)
        finite = bool(torch.isfinite(got).all())
        if precision == "f16x3":
            err, worst = _errs(got, ref64)
            print("%s f16x3: err %.3e err32 %.3e ratio %.2f | worst %.3e worst32 %.3e ratio %.2f" %
                  (tag, err, err32, err / err32, worst, worst32, worst / worst32))
            ok = finite and err <= 2.0 * err32 + 1e-7 and worst <= 3.0 * worst32 + 1e-6
        else:
            err = float((got.double() - ref32.double()).norm() / ref32.double().norm())
            err_half = float((half.double() - ref32.double()).norm() / ref32.double().norm())
            print("%s f16: err vs fp32 %.3e autocast %.3e" % (tag, err, err_half))
            ok = finite and err < max(2e-3, 1.05 * err_half)
        if not ok:
            failures.append((precision, finite, err))
    assert not failures, (tag, failures)


# ------------------------------------------------------------------------------------------------- cases
# (patch, D, hidden, H, W, B): the edge each one reaches
TOKEN_EDGES = [
    (8, 128, 320, 8, 8, 1),         # ntok 2: one patch, hw = 1, M = 2
    (8, 128, 320, 8, 8, 5),         # ... M = 10
    (8, 128, 320, 8, 16, 3),        # ntok 3: 1/3 is inexact, M = 9
    (8, 128, 320, 16, 248, 4),      # ntok 63: M = 252, B*hw = 248
    (8, 128, 320, 16, 328, 4),      # ntok 83, hw 82: float32 1/83 and 1/82 are rounded DOWN, so m * (1 / n) < k at m = k n - the + 0.5 decides
    (8, 128, 320, 56, 72, 4),       # ntok 64: no key padding, M = 256 exactly
    (8, 128, 320, 72, 56, 4),
    (8, 128, 320, 64, 64, 4),       # ntok 65: second key tile holds one key, M = 260 (image 3 straddles the row tile), B*hw = 256 exactly
    (8, 128, 320, 64, 128, 2),      # ntok 129: second query block holds one query, third key tile one key, M = 258
    (16, 128, 320, 112, 144, 4),    # ntok 64 and 65 through the 768-wide im2col
    (16, 128, 320, 128, 128, 4),
]
WIDTH_EDGES = [(64, 64), (64, 320), (128, 320), (256, 1024), (320, 448), (448, 1792), (704, 2816)]      # last column tile partial
CASES = [c + (mode,) for c in TOKEN_EDGES for mode in ("attn", "full")]
CASES += [(8, D, hidden, 64, 64, 4, mode) for D, hidden in WIDTH_EDGES for mode in MODES]
CASES.append((8, 192, 768, 64, 64, 4, "full"))       # the aligned control
CASES = list(dict.fromkeys(CASES))                   # (128, 320) at 65 tokens is in both lists


def _id(c):
    return "p%d-D%d-h%d-%dx%d-B%d-%s" % c


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_native_vit_edge_shape_against_fp64(case):
    """Both precisions of one edge case against the bars of the module docstring.  Measured f16x3 err / err32 over all cases, by mode:
    embed 0.70 - 2.12 (1.8e-7 against a torch convolution at 8.5e-8: the 2^-22 operand split of the patch GEMM, inside the bar by its
    absolute term), attn 0.66 - 1.48, mlp 0.67 - 1.24, full 0.64 - 1.16; f16: 0.69 - 1.00 x the autocast error."""
    patch, D, hidden, H, W, B, mode = case
    model, img, ref64, ref32, half, figs = _case(*case)
    ntok = 1 + (H // patch) * (W // patch)
    print("%s: ntok %d M %d | attn/resid %.2f mlp/resid %.2f entropy %.2f" % (_id(case), ntok, B * ntok, *figs))
    assert_case_tests_something(mode, ntok, figs)
    got = {p: vit_native.NativeViT(model, precision=p).forward_tokens(img) for p in PRECISIONS}
    check_against_fp64(_id(case), got, ref64, ref32, half)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_stale_scratch_never_reaches_an_output(precision):
    """NativeViT keeps one workspace per device and reuses it across geometries; panel rows >= M are never written and only q / k / v^T
    are cleared.  After a 129-token forward the whole cached workspace is filled with 0xFF bytes (every half and every float a NaN)
    before each of a 2-, a 63- and a 65-token forward: each result is finite and bitwise what a fresh NativeViT gives."""
    model = _case(8, 128, 320, 64, 64, 4, "full")[0]
    nat = vit_native.NativeViT(model, precision=precision)
    dev = None
    later = [(8, 8, 5), (16, 248, 4), (64, 64, 4)]
    gen = torch.Generator("cuda").manual_seed(77)
    nat.forward_tokens(torch.randn(2, 3, 64, 128, device="cuda", generator=gen))        # 129 tokens
    imgs = [torch.randn(B, 3, H, W, device="cuda", generator=gen) for H, W, B in later]
    nat.forward_tokens(imgs[-1])                       # the largest workspace of the three: no later call replaces the poisoned buffer
    (dev, ws), = nat._ws.items()
    for img in imgs:
        nat._ws[dev].fill_(255)
        got = nat.forward_tokens(img)
        assert nat._ws[dev].data_ptr() == ws.data_ptr()                      # it ran in the poisoned buffer
        fresh = vit_native.NativeViT(model, precision=precision).forward_tokens(img)
        assert torch.isfinite(got).all(), tuple(img.shape)
        assert torch.equal(got, fresh), (tuple(img.shape), float((got - fresh).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_image_across_a_row_tile_is_batch_independent(precision):
    """65 tokens, B = 4: image 3 owns rows 195 .. 259, on both sides of the 256-row GEMM tile and of the 128-row panels."""
    model, img = _case(8, 128, 320, 64, 64, 4, "full")[:2]
    nat = vit_native.NativeViT(model, precision=precision)
    whole = nat.forward_tokens(img)
    for b in (3, 0):
        assert torch.equal(nat.forward_tokens(img[b:b + 1])[0], whole[b]), b


NEAR_LIMIT = (8, 64, 64, 16, 248, 16644)        # ntok 63: M = 1 048 572 = 2^20 - 4


@pytest.mark.gpu
def test_native_vit_near_the_row_limit_against_fp64():
    """The row -> (image, token) split by float reciprocal, the 32-bit buffer offsets of the residual epilogue and every grid at the
    largest M the library accepts (about 4 GB in all).  f16x3, mode full, against fp64 in chunks of images; the last 8 images bitwise
    against a B = 8 call on them."""
    patch, D, hidden, H, W, B = NEAR_LIMIT
    ntok = 1 + (H // patch) * (W // patch)
    assert B * ntok == (1 << 20) - 4
    seed = _seed(NEAR_LIMIT)
    model = build_model(patch, D, hidden, "full", seed).cuda()
    nat = vit_native.NativeViT(model)
    assert nat.shape_supported(B, H, W) and not nat.shape_supported(B + 1, H, W)
    img = torch.randn(B, 3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
    got = nat.forward_tokens(img)
    assert got.shape == (B, ntok, D) and torch.isfinite(got).all()
    tail = nat.forward_tokens(img[-8:])
    assert torch.equal(tail, got[-8:])
    num = num32 = den = 0.0
    worst = worst32 = 0.0
    with torch.no_grad():
        m64 = _double_of(model)
        figs = branch_figures(m64, img[:64].double())
        for s in range(0, B, 2048):
            x = img[s:s + 2048]
            r64 = m64.get_intermediate_feat(x.double(), n=1)[0][0]
            d = got[s:s + 2048].double() - r64
            d32 = model.get_intermediate_feat(x, n=1)[0][0].double() - r64
            num, num32, den = num + float(d.pow(2).sum()), num32 + float(d32.pow(2).sum()), den + float(r64.pow(2).sum())
            worst, worst32 = max(worst, float(d.abs().max())), max(worst32, float(d32.abs().max()))
    err, err32 = (num / den) ** 0.5, (num32 / den) ** 0.5
    print("near-limit: attn/resid %.2f mlp/resid %.2f entropy %.2f" % figs)
    print("near-limit f16x3: err %.3e err32 %.3e ratio %.2f | worst %.3e worst32 %.3e ratio %.2f" % (err, err32, err / err32, worst, worst32, worst / worst32))
    assert_case_tests_something("full", ntok, figs)
    assert err <= 2.0 * err32 + 1e-7, (err, err32)
    assert worst <= 3.0 * worst32 + 1e-6, (worst, worst32)


# ------------------------------------------------------------------------------------------------- host
def test_float_reciprocal_row_split_is_exact_below_the_guard():
    """The QKV scatter and the embed epilogue split a row index as b = (int)(((float)m + 0.5f) * (1.f / (float)n)) (n = ntok or hw),
    guarded by B * ntok < 2^20.  The expression is monotone in m, so for every n in [1, 2^20) the first and the last row of every
    image, m = k n and m = k n + n - 1 < 2^20, decide whether it equals m // n everywhere.  The same float32 arithmetic in numpy."""
    LIM = 1 << 20
    n = np.arange(1, LIM, dtype=np.int64)
    cnt = (LIM - 1) // n + 1                              # k = 0 .. (LIM - 1) // n: every k with k n < LIM
    nn = np.repeat(n, cnt)
    k = np.arange(nn.size, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    inv = (np.float32(1.0) / nn.astype(np.float32)).astype(np.float32)
    for m in (k * nn, k * nn + nn - 1):
        sel = m < LIM
        assert sel.sum() > 7_000_000
        got = ((m[sel].astype(np.float32) + np.float32(0.5)) * inv[sel]).astype(np.int32)
        assert got.dtype == np.int32 and ((m[sel].astype(np.float32) + np.float32(0.5)) * inv[sel]).dtype == np.float32
        bad = np.nonzero(got != k[sel])[0]
        assert bad.size == 0, (bad.size, nn[sel][bad[:5]], m[sel][bad[:5]])


def test_row_limit_flips_exactly_at_two_to_the_twenty():
    """shape_supported (stego_vit_workspace_bytes: check_desc) accepts B * ntok = 2^20 - 1 and refuses 2^20; (2^20 + 255) rows of 768
    floats - the last row a residual-epilogue lane can address, in bytes - fit the 32-bit buffer offset."""
    nat = vit_native.NativeViT(build_model(8, 64, 64, "full", 1))
    for H, W, ntok in ((8, 8, 2), (8, 16, 3), (32, 64, 33), (16, 248, 63), (56, 72, 64), (64, 64, 65)):
        assert 1 + (H // 8) * (W // 8) == ntok
        last = ((1 << 20) - 1) // ntok
        assert nat.shape_supported(last, H, W), (ntok, last)
        assert not nat.shape_supported(last + 1, H, W), (ntok, last + 1)
        if ((1 << 20) - 1) % ntok == 0:
            assert last * ntok == (1 << 20) - 1
    assert ((1 << 20) - 1) % 3 == 0 and ((1 << 20) - 1) % 33 == 0 and (1 << 20) % 64 == 0      # both sides of the flip are reached exactly
    assert nat.shape_supported(NEAR_LIMIT[5], 16, 248) and not nat.shape_supported(NEAR_LIMIT[5] + 1, 16, 248)
    assert ((1 << 20) + 255) * 768 * 4 < 1 << 32


def test_every_case_builds_on_the_host_and_names_its_edge():
    """The case list itself: every model is one the native path accepts with the stated hidden width, the token counts are the edges
    of the module docstring, and every width but the control ends in a partial 192-column tile."""
    ntoks = sorted({1 + (H // p) * (W // p) for p, _, _, H, W, _ in TOKEN_EDGES})
    assert ntoks == [2, 3, 63, 64, 65, 83, 129]
    assert {B * (1 + (H // p) * (W // p)) for p, _, _, H, W, B in TOKEN_EDGES} >= {2, 9, 252, 256, 258, 260}
    for D, hidden in WIDTH_EDGES:
        assert D % 192 and (hidden % 192 or (hidden // 32) % 6)
        build_model(8, D, hidden, "embed", 0)
    for n in (83, 82):                                  # the case whose row split fails without the rounding offset, in both epilogues
        assert int(np.float32(n) * (np.float32(1) / np.float32(n))) == 0 and int((np.float32(n) + np.float32(0.5)) * (np.float32(1) / np.float32(n))) == 1
    assert len(CASES) == len(set(CASES)) and 40 <= len(CASES) <= 60
