"""NativeViT.forward_keys (stego_vit_forward_keys, include/stego_vit.h): the last block's attention keys - the reference's
feat_type "KK", modules.py:98-101 - against the fp64 evaluation of the same torch module, and what DinoFeaturizer builds on them.

The reference is always ``get_intermediate_feat(img.double(), n=1)[2][0][1]`` of the fp64 twin, as [B, ntok, D] (channel head * 64 + d);
the models carry the magnitudes of tests/test_vit_edges.py::build_model in every block.  The bars are that file's, imported from it:
  * f16x3: relative L2 against fp64 at most 2 x the fp32 torch module's own error on the keys + 1e-7, worst element at most 3 x + 1e-6;
  * f16: relative L2 against the fp32 module's keys below max(2e-3, 1.05 x torch's fp16 autocast on the same keys).
Every case prints its figures before it asserts.

Edges: the K third starts at weight row D = row 0 or 64 of a 128-row panel; D % 192 != 0 ends in a partial column tile whose trailing
weight rows are V rows (or padding, D = 64) and must be dropped; M = B * ntok below, at and above the 256-row tile; depth 1 runs no
full block, depth 2 one."""
import functools

import pytest
import torch

from conftest import assert_close
from test_vit_edges import PRECISIONS, _errs, _seed, check_against_fp64
from stego_amd import capi, dino_vit, vit_native

pytestmark = pytest.mark.gpu


def build_model(patch, D, hidden, depth, seed):
    """tests/test_vit_edges.py::build_model (mode "full") at any depth: noise on every vector and on the class token, position table
    x 10, patch filter x 3 and in EVERY block qkv x 4, proj x 40, fc1 x 10, fc2 x 10."""
    torch.manual_seed(seed)
    m = dino_vit.VisionTransformer(img_size=(4 * patch,), patch_size=patch, embed_dim=D, depth=depth, num_heads=D // 64, mlp_ratio=hidden / D).eval()
    assert all(blk.mlp.fc1.out_features == hidden for blk in m.blocks) and len(m.blocks) == depth
    assert vit_native.supported(m)
    with torch.no_grad():
        for name, prm in m.named_parameters():
            if prm.dim() == 1 or name == "cls_token":
                prm.add_(0.05 * torch.randn_like(prm))
        m.pos_embed.mul_(10.0)
        m.patch_embed.proj.weight.mul_(3.0)
        for blk in m.blocks:
            blk.attn.qkv.weight.mul_(4.0)
            blk.attn.proj.weight.mul_(40.0)
            blk.mlp.fc1.weight.mul_(10.0)
            blk.mlp.fc2.weight.mul_(10.0)
    return m


def _double_of(model):
    blk = model.blocks[0]
    m64 = dino_vit.VisionTransformer(img_size=(model.patch_embed.img_size,), patch_size=model.patch_embed.patch_size, embed_dim=model.embed_dim,
                                     depth=len(model.blocks), num_heads=blk.attn.num_heads,
                                     mlp_ratio=blk.mlp.fc1.out_features / model.embed_dim).to(model.pos_embed.device).double().eval()
    assert m64.blocks[0].mlp.fc1.out_features == blk.mlp.fc1.out_features
    m64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    return m64


def _rows(t):
    """[B, heads, ntok, 64] (one third of the qkv tensor) -> [B, ntok, heads * 64]"""
    B, heads, ntok, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, ntok, heads * d)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@functools.lru_cache(maxsize=None)
def _case(patch, D, hidden, depth, H, W, B):
    """Model, input, the keys by the three torch evaluations (fp64, fp32, fp16 autocast) and the fp64 distances that make a wrong
    block or a wrong third visible: computed once, shared, never written to."""
    seed = _seed("keys", patch, D, hidden, depth, H, W, B)
    model = build_model(patch, D, hidden, depth, seed).cuda()
    img = torch.randn(B, 3, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
    with torch.no_grad():
        m64 = _double_of(model)
        qkvs = m64.get_intermediate_feat(img.double(), n=depth)[2]
        ref64 = _rows(m64.get_intermediate_feat(img.double(), n=1)[2][0][1])
        assert torch.equal(ref64, _rows(qkvs[-1][1]))
        figs = (_rel(_rows(qkvs[0][1]), ref64) if depth > 1 else None, _rel(_rows(qkvs[-1][0]), ref64), _rel(_rows(qkvs[-1][2]), ref64))
        ref32 = _rows(model.get_intermediate_feat(img, n=1)[2][0][1])
        with torch.autocast("cuda", dtype=torch.float16):
            half = _rows(model.get_intermediate_feat(img, n=1)[2][0][1]).float()
    return model, img, ref64, ref32, half, figs


def assert_case_can_fail(depth, figs):
    first, q, v = figs
    if depth > 1:
        assert first >= 0.3, ("the keys of block 0 are the keys of the last block: the wrong block would pass", first)
    assert q >= 0.5 and v >= 0.5, ("K is close to the Q or V third: a wrong column base or bias third would pass", q, v)


# (patch, D, hidden, depth, H, W, B)
DEPTH2 = [(8, D, hidden, 2, 64, 64, 4) for D, hidden in ((64, 64), (128, 320), (192, 768), (320, 448), (384, 1536))]      # ntok 65, M = 260
DEPTH1 = [(8, 128, 320, 1, 8, 8, 1), (8, 128, 320, 1, 8, 8, 5),      # ntok 2
          (8, 128, 320, 1, 56, 72, 4),                               # ntok 64, M = 256 exactly
          (8, 128, 320, 1, 64, 128, 2)]                              # ntok 129
HEADS12 = [(8, 768, 3072, 2, 16, 16, 2)]
PATCH16 = [(16, 128, 320, 2, 128, 128, 4)]
CASES = DEPTH2 + DEPTH1 + HEADS12 + PATCH16


def _id(c):
    return "p%d-D%d-h%d-L%d-%dx%d-B%d" % c


def test_the_case_list_reaches_both_panel_rows_and_both_kinds_of_last_tile():
    assert [(D % 128, D % 192 == 0) for _, D, _, _, _, _, _ in DEPTH2] == [(64, False), (0, False), (64, True), (64, False), (0, True)]
    assert sorted({1 + (H // p) * (W // p) for p, _, _, _, H, W, _ in DEPTH1}) == [2, 64, 129]
    assert all(B * (1 + (H // p) * (W // p)) == 260 for p, _, _, _, H, W, B in DEPTH2)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_native_keys_against_fp64(case):
    patch, D, hidden, depth, H, W, B = case
    model, img, ref64, ref32, half, figs = _case(*case)
    ntok = 1 + (H // patch) * (W // patch)
    print("%s: ntok %d M %d | fp64 rel. distance of K to block 0's K %s, to Q %.2f, to V %.2f" %
          (_id(case), ntok, B * ntok, "%.2f" % figs[0] if depth > 1 else "-", figs[1], figs[2]))
    assert_case_can_fail(depth, figs)
    got = {p: vit_native.NativeViT(model, precision=p).forward_keys(img) for p in PRECISIONS}
    assert all(g.shape == (B, ntok, D) for g in got.values())
    check_against_fp64(_id(case), got, ref64, ref32, half)
    check_against_fp64(_id(case) + " class row", {p: g[:, :1] for p, g in got.items()}, ref64[:, :1], ref32[:, :1], half[:, :1])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stale_scratch_never_reaches_the_keys(precision):
    """As tests/test_vit_edges.py::test_stale_scratch_never_reaches_an_output: the cached workspace full of 0xFF bytes before a 2-, a
    63- and a 65-token forward_keys; each result is finite and bitwise a fresh NativeViT's."""
    model = _case(8, 128, 320, 2, 64, 64, 4)[0]
    nat = vit_native.NativeViT(model, precision=precision)
    later = [(8, 8, 5), (16, 248, 4), (64, 64, 4)]
    gen = torch.Generator("cuda").manual_seed(78)
    nat.forward_keys(torch.randn(2, 3, 64, 128, device="cuda", generator=gen))        # 129 tokens
    imgs = [torch.randn(B, 3, H, W, device="cuda", generator=gen) for H, W, B in later]
    nat.forward_keys(imgs[-1])
    (dev, ws), = nat._ws.items()
    for img in imgs:
        nat._ws[dev].fill_(255)
        got = nat.forward_keys(img)
        assert nat._ws[dev].data_ptr() == ws.data_ptr()
        fresh = vit_native.NativeViT(model, precision=precision).forward_keys(img)
        assert torch.isfinite(got).all(), tuple(img.shape)
        assert torch.equal(got, fresh), (tuple(img.shape), float((got - fresh).abs().max()))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_keys_are_batch_independent_and_leave_the_token_forward_alone(precision):
    model, img = _case(8, 128, 320, 2, 64, 64, 4)[:2]
    nat = vit_native.NativeViT(model, precision=precision)
    before = nat.forward_tokens(img)
    whole = nat.forward_keys(img)
    for b in (3, 0):                                   # image 3: rows 195 .. 259, on both sides of the 256-row tile
        assert torch.equal(nat.forward_keys(img[b:b + 1])[0], whole[b]), b
    assert torch.equal(nat.forward_tokens(img), before)
    assert len(nat._packed) == 1 and len(nat._ws) == 1             # one blob, one workspace for both entry points


# ------------------------------------------------------------------------------------------------- featurizer
FZ_CASE = (8, 192, 768, 2, 64, 64, 4)          # ViT-S-like and tiny: 3 heads, C = 192


def _featurizer(feat_type="KK", **cfg_extra):
    """DinoFeaturizer(dim 70, nonlinear head, no dropout, cfg.native_backbone = True as configs/train_config.yml sets it) around the
    model of FZ_CASE."""
    import warnings
    from stego_amd import featurizers

    class C:
        dino_patch_size = 8; dino_feat_type = feat_type; model_type = "vit_tiny"; projection_type = "nonlinear"
        dropout = False; pretrained_weights = None; native_backbone = True
    for k, v in cfg_extra.items():
        setattr(C, k, v)
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fz = featurizers.DinoFeaturizer(70, C()).cuda().eval()
    fz.model = _case(*FZ_CASE)[0]
    return fz


def _as_rows(image_feat):
    B, C, h, w = image_feat.shape
    return image_feat.permute(0, 2, 3, 1).reshape(B, h * w, C)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_kk_featurizer_runs_the_native_keys_and_the_native_head(precision):
    model, img, ref64, ref32, half, figs = _case(*FZ_CASE)
    assert_case_can_fail(2, figs)
    fz = _featurizer(backbone_precision=precision)
    feats, code = fz(img)
    assert fz.backbone_path == "native"
    assert feats.shape == (4, 192, 8, 8) and feats.stride(1) == 1 and code.shape == (4, 70, 8, 8)
    check_against_fp64("featurizer KK", {precision: _as_rows(feats)}, ref64[:, 1:], ref32[:, 1:], half[:, 1:])
    # the torch branch of the same featurizer: the K third of the fp32 module's qkv tensor
    ft = _featurizer(native_backbone=False)
    feats_t, code_t = ft(img)
    assert ft.backbone_path == "torch" and feats_t.shape == feats.shape
    map64 = ref64[:, 1:].reshape(4, 8, 8, 192).permute(0, 3, 1, 2)
    d_nt, d_n, d_t = (float((a.double() - b.double()).norm()) for a, b in ((feats, feats_t), (feats, map64), (feats_t, map64)))
    print("featurizer KK %s: |native - torch| %.3e, |native - fp64| %.3e + |torch - fp64| %.3e" % (precision, d_nt, d_n, d_t))
    assert d_nt <= (d_n + d_t) * (1 + 1e-9)
    # the head: native kernels on the channels-last key map, against the torch head on the same map
    assert fz._native_head_ok(feats)
    with torch.no_grad():
        code_ref = fz._head(feats)
    assert code.stride(1) == 1
    assert_close(code.detach().cpu().numpy(), code_ref.cpu().numpy(), rtol=1e-3, atol_frac=1e-4, what="code (KK, native head)")
    # the class feature is the class row of the TOKENS whatever the feature type
    cls = fz(img, return_class_feat=True)
    assert fz.backbone_path == "native" and cls.shape == (4, 192, 1, 1)
    cls_feat = _featurizer("feat", backbone_precision=precision)(img, return_class_feat=True)
    assert torch.equal(cls, cls_feat)
    assert _errs(cls.reshape(4, 192), ref64[:, 0])[0] > 0.5            # ... and not the class token's key


def test_a_cfg_without_the_native_backbone_key_keeps_the_torch_keys():
    """'KK' ran on the fp32 torch module before the kernels had keys; a cfg object that does not carry `native_backbone` at all keeps
    that (tests/test_vit_native.py pins it), every cfg of load_config carries the key."""
    from stego_amd.train_segmentation import load_config
    assert load_config(overrides=["dino_feat_type=KK"]).native_backbone is True
    img = _case(*FZ_CASE)[1]
    fz = _featurizer()
    del type(fz.cfg).native_backbone
    assert not hasattr(fz.cfg, "native_backbone")
    feats, _ = fz(img)
    assert fz.backbone_path == "torch"
    fz.cfg.native_backbone = True
    native, _ = fz(img)
    assert fz.backbone_path == "native" and float((native - feats).norm() / feats.norm()) < 1e-5


def test_kk_token_cache_holds_the_keys_and_never_serves_the_class_feature():
    model, img = _case(*FZ_CASE)[:2]
    fz = _featurizer()
    direct = fz(img)[0]
    cache = fz.enable_token_cache(8, (64, 64), img.device)
    idx = torch.tensor([5, 1, 6, 2], device=img.device)
    first = fz(img, cache_index=idx)[0]
    assert cache.misses == 4 and fz.backbone_path == "native"
    fz.backbone_path = None
    second, code = fz(img, cache_index=idx)
    assert cache.misses == 4 and fz.backbone_path is None             # no backbone ran
    want = direct.half().float()
    assert second.stride(1) == 1 and torch.equal(second, want) and torch.equal(first, want)
    assert torch.equal(cache.tokens[idx][:, 1:].float(), _as_rows(want))
    assert fz._native_head_ok(second) and code.shape == (4, 70, 8, 8)
    cls = fz(img, return_class_feat=True, cache_index=idx)
    assert cache.misses == 4
    assert torch.equal(cls, _featurizer("feat")(img, return_class_feat=True))
    assert not torch.equal(cls.reshape(4, 192), cache.tokens[idx][:, 0].float())


def test_loss_on_kk_maps_takes_the_single_launch_forward():
    """The channels-last key maps (C = 192) go through the fused forward (one launch); a contiguous channels-first copy of the same maps
    takes the three-launch kernels.  Same values, 1e-3 relative."""
    from oracle import corr_oracle as O
    from stego_amd import modules as M
    img = _case(*FZ_CASE)[1]
    fz = _featurizer()
    B, C, K, H, W, S, n_neg = 4, 192, 70, 8, 8, 5, 2
    gen = torch.Generator("cuda").manual_seed(5)
    img_pos = torch.randn(img.shape, device="cuda", generator=gen)
    feats, code = fz(img)
    feats_pos, code_pos = fz(img_pos)
    code, code_pos = code.detach(), code_pos.detach()
    assert fz.backbone_path == "native" and all(t.stride(1) == 1 for t in (feats, feats_pos, code, code_pos))
    cfg = O.CorrCfg(feature_samples=S, neg_samples=n_neg)
    loss = M.ContrastiveCorrelationLoss(cfg)
    assert loss.fused_kernels_cover(B, C, K, H, W, S, feats.device, n_neg)
    desc = capi.make_desc(B, C, K, H, W, S, n_neg, cfg, (cfg.pos_intra_shift, cfg.pos_inter_shift, cfg.neg_inter_shift), capi.PREC_F16X3)
    assert capi.corr_fwd_launches(desc, feats, feats_pos, code, code_pos) == 1
    nchw = [t.contiguous() for t in (feats, feats_pos, code, code_pos)]
    assert all(t.stride(1) != 1 for t in nchw) and capi.corr_fwd_launches(desc, *nchw) == 3
    coords1 = torch.rand(B, S, S, 2, device="cuda", generator=gen) * 2 - 1
    coords2 = torch.rand(B, S, S, 2, device="cuda", generator=gen) * 2 - 1
    perms = torch.tensor([[1, 2, 3, 0], [2, 3, 0, 1]], device="cuda")
    with torch.no_grad():
        a = loss.forward_explicit(feats, feats_pos, code, code_pos, coords1, coords2, perms)
        b = loss.forward_explicit(*nchw, coords1, coords2, perms)
    scale = float(b[4].abs().mean())
    for i in (0, 2):
        print("loss[%d]: fused %.7f three-launch %.7f" % (i, float(a[i]), float(b[i])))
        assert abs(float(a[i]) - float(b[i])) <= 1e-3 * scale + 1e-3 * abs(float(b[i]))
    for i, what in ((1, "pos_intra_cd"), (3, "pos_inter_cd"), (4, "neg_inter_loss"), (5, "neg_inter_cd")):
        assert_close(a[i].cpu().numpy(), b[i].cpu().numpy(), rtol=1e-3, atol_frac=5e-4, what=what)
