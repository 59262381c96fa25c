"""the segmentation head (modules.py:108-116) on the hand-written kernels of include/stego_head.h against the
reference's convolution head with the same Dropout2d draws, forward and all six parameter gradients."""
import types

import numpy as np
import pytest
import torch

from conftest import assert_close
from stego_amd import capi
from stego_amd.featurizers import DinoFeaturizer
from stego_amd.train_segmentation import load_config

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _featurizer(arch, dim, proj, dropout, seed=0):
    cfg = load_config(overrides=["model_type=%s" % arch, "dino_patch_size=8", "dim=%d" % dim, "projection_type=%s" % proj,
                                 "dropout=%s" % dropout, "native_backbone=False"])
    torch.manual_seed(seed)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = DinoFeaturizer(dim, cfg).to(DEV)
    return net, cfg


def _reference_head_fp64(net, image_feat, masks):
    """modules.py:108-116 in double precision with explicit channel masks: conv1x1(x * m) = (x * m) W^T + b over the tokens.
    Also returns, for a nonlinear head, which hidden channels have a pre-activation within fp32 rounding of zero somewhere: the sign
    of such a value - hence relu' - is not defined at fp32 accuracy (fp32 torch and the kernels flip the same few), and one flipped
    (token, channel) moves that channel's row of cluster2[0]'s weight gradient by far more than any rounding error."""
    x = image_feat.double()
    m1, m2, m3 = [m.double().view(m.shape[0], -1, 1, 1) for m in masks]
    c1 = net.cluster1[0]
    conv = lambda c, t: torch.nn.functional.conv2d(t, c.weight.double(), c.bias.double())
    code = conv(c1, x * m1)
    ambiguous = None
    if net.proj_type == "nonlinear":
        pre = conv(net.cluster2[0], x * m2)
        ambiguous = (pre.detach().abs() < 1e-5).permute(1, 0, 2, 3).flatten(1).any(1)
        code = code + conv(net.cluster2[2], torch.relu(pre))
    return x * m3, code, ambiguous


_ARCH_C = {"vit_tiny": 192, "vit_small": 384, "vit_base": 768}
# head_gemm_kernel<true, EPI_BIAS_RELU, 1> (forward H) and <false, EPI_MASK_POS, 1> (backward dHpre): wide_blocks(C) == 1, C % 384 != 0
_NARROW_C = [("vit_tiny", 4, (28, 28), 70, "nonlinear")]
# head_wgrad_kernel (the non-transposing weight gradient): stego_head_bwd's wgrad takes it when HW < 32; and the forward's mask slots:
# n_slot = min(B, 127 / HW + 2) images per 128-row tile (9 at HW = 16, 7 at HW = 25, 6 at HW = 31), B large enough to fill them
_SHORT_MAPS = [(arch, B, hw, 70, "nonlinear") for arch in _ARCH_C for B, hw in ((24, (4, 4)), (16, (5, 5)), (12, (1, 31)))]
# code widths K (the N of the cluster1 / cluster2[2] GEMMs and of the dW1 / dW22 tiles) from one column to a full 128-column tile
_CODE_WIDTHS = [("vit_small", 2, (14, 14), K, proj) for K in (1, 27, 64, 128) for proj in ("linear", "nonlinear")]
# M = B * HW below one 128-row tile and not a multiple of it; the production batch 2B = 64 at 28 x 28
_ROW_COUNTS = [("vit_small", 3, (3, 11), 70, "nonlinear"), ("vit_small", 64, (28, 28), 70, "nonlinear")]


@pytest.mark.parametrize("arch,B,hw,dim,proj", [("vit_small", 4, (14, 14), 70, "nonlinear"), ("vit_small", 3, (9, 13), 70, "linear"),
                                                 ("vit_base", 2, (10, 10), 100, "nonlinear"), ("vit_small", 32, (28, 28), 70, "nonlinear")]
                         + _NARROW_C + _SHORT_MAPS + _CODE_WIDTHS + _ROW_COUNTS)
def test_native_head_matches_the_reference_head_with_the_same_dropout_draws(arch, B, hw, dim, proj):
    net, cfg = _featurizer(arch, dim, proj, True)
    net.train()
    C = net.n_feats
    g = torch.Generator(device=DEV).manual_seed(5)
    tokens = torch.randn(B, 1 + hw[0] * hw[1], C, device=DEV, generator=g)
    image_feat = tokens[:, 1:, :].reshape(B, hw[0], hw[1], C).permute(0, 3, 1, 2)       # what forward() hands the head (modules.py:97)
    up = torch.randn(B, dim, hw[0], hw[1], device=DEV, generator=g) / (hw[0] * hw[1])
    assert net._native_head_ok(image_feat)
    params = [p for n, p in net.named_parameters() if n.startswith("cluster")]

    def run(native):
        cfg.native_head = native
        for p in params:
            p.grad = None
        torch.manual_seed(77)
        if native:
            feats, code = net._head_native(image_feat)
        else:
            code = net._head(image_feat)
            feats = net.dropout(image_feat)
        (code * up).sum().backward()
        return feats.detach().clone(), code.detach().clone(), [p.grad.detach().clone() for p in params], torch.rand(2, device=DEV)

    f_n, c_n, g_n, r_n = run(True)
    f_t, c_t, g_t, r_t = run(False)
    assert torch.equal(r_n, r_t)                       # both consumed the generator alike
    assert torch.equal(f_n, f_t)                       # the returned dropout(image_feat): same mask, same product
    # masks as drawn (same seed, same calls), for the fp64 reference
    torch.manual_seed(77)
    masks = [net._feature_noise(image_feat).view(B, C) for _ in range(3 if proj == "nonlinear" else 1)]
    if proj != "nonlinear":
        masks = [masks[0], masks[0], net._feature_noise(image_feat).view(B, C)]
    if B > 1:                                          # distinct masks per image: a mask row taken from the wrong image shows
        for m in masks:
            assert len({tuple(r) for r in m.cpu().tolist()}) == B
    x64 = image_feat.double().requires_grad_(False)
    for p in params:
        p.grad = None
    f64, c64, ambiguous = _reference_head_fp64(net, x64, masks)
    net64_grads = torch.autograd.grad((c64 * up.double()).sum(), params, allow_unused=True)
    assert_close(c_n.cpu().numpy(), c64.detach().cpu().numpy(), rtol=1e-3, atol_frac=1e-4, what="code")
    err_n = float((c_n.double() - c64).abs().max())
    err_t = float((c_t.double() - c64).abs().max())
    assert err_n <= 2.0 * err_t + 1e-6, (err_n, err_t)           # the split-fp16 head is in the fp32 class of the torch head
    for b in range(B):                                           # ... image by image (each has its own mask rows)
        eb_n = float((c_n[b].double() - c64[b]).abs().max())
        eb_t = float((c_t[b].double() - c64[b]).abs().max())
        assert eb_n <= 2.0 * eb_t + 1e-6, (b, eb_n, eb_t)
    for (name, p), gn, gt, g64 in zip([(n, p) for n, p in net.named_parameters() if n.startswith("cluster")], g_n, g_t, net64_grads):
        if name.startswith("cluster2.0.") and ambiguous is not None and bool(ambiguous.any()):
            keep = ~ambiguous                     # rows of dW21 / entries of db21 whose relu' is well defined
            assert int(keep.sum()) >= 0.5 * keep.numel()
            gn, gt, g64 = gn[keep], gt[keep], g64[keep]
        assert_close(gn.cpu().numpy(), g64.detach().cpu().numpy(), rtol=1e-3, atol_frac=2e-4, what="grad %s" % (tuple(p.shape),))
        en, et = float((gn.double() - g64).abs().max()), float((gt.double() - g64).abs().max())
        assert en <= 3.0 * et + 1e-7 * float(g64.abs().max()) + 1e-12, (tuple(p.shape), en, et)


def test_native_head_in_eval_mode_and_bitwise_repeatable():
    net, cfg = _featurizer("vit_small", 70, "nonlinear", True)
    net.eval()
    B, hw, C = 5, (12, 12), 384
    tokens = torch.randn(B, 1 + 144, C, device=DEV)
    image_feat = tokens[:, 1:, :].reshape(B, 12, 12, C).permute(0, 3, 1, 2)
    with torch.no_grad():
        f1, c1 = net._head_native(image_feat)
        f2, c2 = net._head_native(image_feat)
        cfg.native_head = False
        ct = net._head(image_feat)
    assert f1.data_ptr() == image_feat.data_ptr()          # eval: nn.Dropout2d is the identity, the map itself is returned
    assert torch.equal(c1, c2)
    assert_close(c1.cpu().numpy(), ct.cpu().numpy(), rtol=1e-3, atol_frac=1e-4, what="code (eval)")


def test_head_argument_checks_need_no_launch():
    import ctypes
    lib = capi.load()
    d = capi.StegoHeadDesc(2, 49, 100, 70, 1, 100, 50 * 100)               # C not a multiple of 32
    assert lib.stego_head_fwd_workspace_bytes(ctypes.byref(d)) == 0
    d = capi.StegoHeadDesc(2, 49, 384, 70, 1, 384, 50 * 384)
    assert lib.stego_head_fwd_workspace_bytes(ctypes.byref(d)) >= 2 * 49 * 384 * 4
    assert lib.stego_head_fwd(ctypes.byref(d), *([None] * 14), 0, None) == 1   # STEGO_ERR_NULL


@pytest.mark.parametrize("B,C,n", [(64, 384, 3), (32, 384, 3), (4, 768, 2), (3, 96, 1)])
def test_one_launch_dropout_masks_are_the_torch_generator_s_bernoulli_draws(B, C, n):
    """stego_ref_dropout_masks against nn.Dropout2d's own draws (x.new_empty(B, C, 1, 1).bernoulli_(1 - p).div_(1 - p), n calls) from the
    same generator state over many seeds: every mask value equal, the generator left at the same offset - eagerly and replayed from a
    HIP graph (the captured launch reads the generator's graph-safe state)."""
    from stego_amd import capi, featurizers as FZ
    from stego_amd.modules import _device_generator
    net, cfg = _featurizer("vit_small", 70, "nonlinear", True)
    dev = torch.device(DEV)
    x = torch.zeros(B, C, 2, 2, device=dev)
    q = 1.0 - float(net.dropout.p)
    assert capi.torchglue() is not None
    v = FZ._mask_variant(net, x, n, q)
    assert v >= 0, "no variant of stego_ref_dropout_masks reproduces this torch build: DinoFeaturizer would keep the torch calls"
    gen = _device_generator(dev)
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    for seed in range(300):
        torch.manual_seed(4000 + seed)
        if seed % 3 == 1:
            torch.rand(5, device=dev)
        st = gen.get_state()
        want = torch.stack([net._feature_noise(x).view(-1) for _ in range(n)])
        off = gen.get_offset()
        gen.set_state(st)
        got = capi.ref_dropout_masks(gen, n, B * C, q, v, dev)
        assert gen.get_offset() == off
        bad += (got != want).sum()
    assert int(bad) == 0
    assert 0.05 < float((want == 0).float().mean()) < 0.16          # (p = 0.1 of the channels dropped)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = capi.ref_dropout_masks(gen, n, B * C, q, v, dev)
    for seed in range(10):
        torch.manual_seed(7000 + seed)
        st = gen.get_state()
        want = [torch.stack([net._feature_noise(x).view(-1) for _ in range(n)]) for _ in range(2)]
        off = gen.get_offset()
        gen.set_state(st)
        for k in range(2):
            g.replay()
            assert torch.equal(got, want[k])
        assert gen.get_offset() == off


def test_cached_tokens_arrive_converted_with_their_magnitude_word():
    """stego_tokens_from_cache (TokenCache.fetch on a HIP device): rows of the fp16 table as fp32 + the largest magnitude of the patch
    tokens (class token skipped) in one pass; the head run with that word (StegoHeadDesc.tokens_amax) is bitwise the head that scans
    the tokens itself."""
    from stego_amd import capi
    dev = torch.device(DEV)
    g = torch.Generator(device=dev).manual_seed(3)
    table = (torch.randn(10, 1 + 49, 384, device=dev, generator=g) * 3).half()
    table[:, 0, :] *= 50                                   # a class token larger than every patch token
    index = torch.tensor([7, 2, 2, 9], device=dev)
    out, amax = capi.tokens_from_cache(table, index, skip_rows=1)
    assert torch.equal(out, table[index].float())
    assert float(amax.view(torch.float32)) == float(table[index][:, 1:, :].float().abs().max())
    net, cfg = _featurizer("vit_small", 70, "nonlinear", True)
    net.eval()
    image_feat = out[:, 1:, :].reshape(4, 7, 7, 384).permute(0, 3, 1, 2)
    with torch.no_grad():
        f0, c0 = net._head_native(image_feat)
        f1, c1 = net._head_native(image_feat, amax)
    assert torch.equal(c0, c1) and torch.equal(f0, f1)


def test_cpp_head_function_is_the_python_one_bit_for_bit():
    """csrc/torch_glue_ext.cpp::HeadFn (default) against featurizers._NativeHeadFunction (cfg.native_autograd = False): same C ABI calls,
    so feats, code and the six parameter gradients are bitwise equal - training mode (masks, saved H) and eval mode."""
    from stego_amd import capi
    assert capi.torchglue() is not None and hasattr(capi.torchglue(), "head")
    net, cfg = _featurizer("vit_small", 70, "nonlinear", True)
    g = torch.Generator(device=DEV).manual_seed(9)
    tokens = torch.randn(6, 1 + 14 * 14, 384, device=DEV, generator=g)
    image_feat = tokens[:, 1:, :].reshape(6, 14, 14, 384).permute(0, 3, 1, 2)
    up = torch.randn(6, 70, 14, 14, device=DEV, generator=g) / 196
    params = [p for n, p in net.named_parameters() if n.startswith("cluster")]
    res = {}
    for native_autograd in (True, False):
        cfg.native_autograd = native_autograd
        rec = []
        for train in (True, False):
            net.train(train)
            for p in params:
                p.grad = None
            torch.manual_seed(5)
            feats, code = net._head_native(image_feat)
            (code * up).sum().backward()
            rec += [feats.detach().clone(), code.detach().clone()] + [p.grad.detach().clone() for p in params]
        res[native_autograd] = rec
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def _head_torch(tokens, masks, P, up, dtype):
    """modules.py:108-112 on the token matrix in `dtype`, with explicit channel masks: code, the six parameter gradients of
    sum(code * up), and cluster2[0]'s pre-activation."""
    x = tokens.to(dtype)
    m1, m2 = [m.to(dtype)[:, None, :] for m in masks[:2]]
    ps = [P[n].detach().to(dtype).requires_grad_(True) for n in ("w1", "b1", "w21", "b21", "w22", "b22")]
    w1, b1, w21, b21, w22, b22 = ps
    pre = (x * m2) @ w21.T + b21
    code = (x * m1) @ w1.T + b1 + torch.relu(pre) @ w22.T + b22
    return code.detach(), torch.autograd.grad((code * up.to(dtype)).sum(), ps), pre.detach()


def _head_params(C, K, seed, b21_shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    u = lambda *shape: (torch.rand(*shape, device=DEV, generator=g) * 2 - 1) / C ** 0.5       # Conv2d's default init range
    return dict(w1=u(K, C), b1=u(K), w21=u(C, C), b21=u(C) + b21_shift, w22=u(K, C), b22=u(K))


# operand-scale edges of head_scale (the power-of-two prescale taken from each operand's largest magnitude), through the C ABI:
# tokens x 1e-3 / x 1e3, all-zero tokens (scale word 0), a ReLU-dead hidden layer (H = 0, its scale word 0), one image masked out;
# at C = 384, HW = 49 (head_gemm_kernel<.., 3>, head_wgrad_tr_kernel) and C = 192, HW = 16 (NW = 1 GEMMs, head_wgrad_kernel, 9 slots)
@pytest.mark.parametrize("B,HW,C", [(6, 49, 384), (20, 16, 192)])
@pytest.mark.parametrize("edge", ["tokens_x1e-3", "tokens_x1e3", "zero_tokens", "relu_dead", "zero_mask_image"])
def test_native_head_operand_scale_edges_against_fp64(edge, B, HW, C):
    K = 70
    g = torch.Generator(device=DEV).manual_seed(HW + C)
    full = torch.randn(B, 1 + HW, C, device=DEV, generator=g)
    scale = {"tokens_x1e-3": 1e-3, "tokens_x1e3": 1e3, "zero_tokens": 0.0}.get(edge, 1.0)
    full *= scale
    tokens = full[:, 1:, :]                                            # the backbone's layout: the class token skipped by the view
    masks = [((torch.rand(B, C, device=DEV, generator=g) < 0.9).float() / 0.9).contiguous() for _ in range(3)]
    if edge == "zero_mask_image":
        for m in masks:
            m[1] = 0.0
    P = _head_params(C, K, seed=C, b21_shift=-1e3 if edge == "relu_dead" else 0.0)
    up = torch.randn(B, HW, K, device=DEV, generator=g) / HW
    code, feats, saved_h = capi.head_fwd(tokens, masks, P["w1"], P["b1"], P["w21"], P["b21"], P["w22"], P["b22"], True, True)
    grads = capi.head_bwd(tokens, masks, saved_h, P["w22"], up, K)
    torch.cuda.synchronize()
    c64, g64, pre64 = _head_torch(tokens, masks, P, up, torch.float64)
    c32, g32, _ = _head_torch(tokens, masks, P, up, torch.float32)
    if edge == "relu_dead":
        assert bool((pre64 < 0).all())
    assert torch.equal(feats, tokens * masks[2][:, None, :])           # the returned dropout(image_feat): the same fp32 product
    outs = [("code", code, c32, c64)] + [("grad %s" % n, a, t, r) for n, a, t, r in zip(("w1", "b1", "w21", "b21", "w22", "b22"),
                                                                                         grads, g32, g64)]
    ambiguous = (pre64.abs() < 1e-5 * max(1.0, float(pre64.abs().max()))).flatten(0, 1).any(0)       # relu' undefined at fp32 accuracy
    for name, got, t32, r64 in outs:
        assert bool(torch.isfinite(got).all()), name
        assert bool((got[r64 == 0] == 0).all()), (name, "not exactly zero where fp64 is")
        if name in ("grad w21", "grad b21") and bool(ambiguous.any()):
            keep = ~ambiguous
            assert int(keep.sum()) >= 0.5 * keep.numel()
            got, t32, r64 = got[keep], t32[keep], r64[keep]
        if name == "code":
            assert_close(got.cpu().numpy(), r64.cpu().numpy(), rtol=1e-3, atol_frac=1e-4, what=name)
            for b in range(B):
                en, et = float((got[b].double() - r64[b]).abs().max()), float((t32[b].double() - r64[b]).abs().max())
                assert en <= 2.0 * et + 1e-6 * max(1.0, scale), (name, b, en, et)
        else:
            assert_close(got.cpu().numpy(), r64.cpu().numpy(), rtol=1e-3, atol_frac=2e-4, what=name)
            en, et = float((got.double() - r64).abs().max()), float((t32.double() - r64).abs().max())
            assert en <= 3.0 * et + 1e-7 * float(r64.abs().max()) + 1e-12, (name, en, et)
    if edge == "zero_mask_image":                                      # image 1 sees no token: its code is the same for every token
        assert bool((feats[1] == 0).all())
        assert float((code[1] - code[1, :1]).abs().max()) == 0.0
