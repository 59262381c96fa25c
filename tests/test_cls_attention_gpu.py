"""Class-token attention maps and attention salience masks on the MI355X (csrc/vit_cls_attn.hip; include/stego_vit.h:
stego_vit_forward_attn, stego_attn_salience).

The attention: NativeViT.forward_tokens_attn against the fp64 twin's ``get_intermediate_feat(img.double(), n=1, need_attn=True)[1][0][:, :, 0, :]``
with the fp32 module and fp16 autocast beside it; models from tests/test_vit_keys_gpu.py::build_model, the comparison and its bars from
tests/test_vit_edges.py::check_against_fp64, both imported:
  * f16x3: relative L2 against fp64 at most 2 x the fp32 torch module's own error + 1e-7, worst element at most 3 x + 1e-6;
  * f16: relative L2 against the fp32 module below max(2e-3, 1.05 x torch's fp16 autocast).
Before it compares, every case asserts in fp64 that the class row is at least 0.3 (relative L2) away from the uniform row, from token 1's
attention row and - depth 2 - from block 0's class row: a no-op, a wrong query row or a wrong block would not pass.
The masks: stego_attn_salience on the synthetic inputs of tests/attn_salience_oracle.py against that oracle - masks and kept EQUAL, soft
within 1e-6 relative - and on the native attention of a ViT case.  Every case prints its figures before it asserts.
"""
import functools
import warnings

import numpy as np
import pytest
import torch

import attn_salience_oracle as O
from test_vit_edges import PRECISIONS, _seed, check_against_fp64
from test_vit_keys_gpu import _double_of, _featurizer, build_model
from stego_amd import salience, vit_native

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="DinoFeaturizer")


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _class_row(model, x):
    return model.get_intermediate_feat(x, n=1, need_attn=True)[1][0][:, :, 0, :]


@functools.lru_cache(maxsize=None)
def _case(patch, D, hidden, depth, H, W, B):
    """Model, input, the class row by the three torch evaluations (fp64, fp32, fp16 autocast) and the fp64 distances that make a no-op, a
    wrong query row or a wrong block visible: computed once, shared, never written to."""
    seed = _seed("class attention", patch, D, hidden, depth, H, W, B)
    model = build_model(patch, D, hidden, depth, seed).cuda()
    # (drawn on the host: the case - and its three distances, 0.36 at the least over the list, evaluated in fp64 on a CPU - is the same everywhere)
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)).cuda()
    with torch.no_grad():
        m64 = _double_of(model)
        attns = m64.get_intermediate_feat(img.double(), n=depth, need_attn=True)[1]
        ref64 = _class_row(m64, img.double())
        assert torch.allclose(ref64, attns[-1][:, :, 0, :], rtol=0, atol=1e-12)
        figs = (_rel(torch.full_like(ref64, 1.0 / ref64.shape[-1]), ref64), _rel(attns[-1][:, :, 1, :], ref64),
                _rel(attns[0][:, :, 0, :], ref64) if depth > 1 else None)
        ref32 = _class_row(model, img)
        with torch.autocast("cuda", dtype=torch.float16):
            half = _class_row(model, img).float()
    return model, img, ref64, ref32, half, figs


def assert_case_can_fail(figs):
    uniform, token1, block0 = figs
    assert uniform >= 0.3, ("the class row is the uniform row: a kernel that ignores q and k would pass", uniform)
    assert token1 >= 0.3, ("the class row is token 1's row: a wrong query row would pass", token1)
    assert block0 is None or block0 >= 0.3, ("block 0's class row is the last block's: the wrong block would pass", block0)


# (patch, D, hidden, depth, H, W, B)
CASES = [(8, 64, 64, 2, 64, 64, 4),            # 1 head, ntok 65 -> padded to 128
         (8, 128, 320, 2, 64, 64, 4),
         (8, 192, 768, 2, 64, 64, 4),
         (8, 384, 1536, 2, 64, 64, 4),         # 6 heads, one attention weight near 1
         (8, 128, 320, 1, 8, 8, 5),            # ntok 2, depth 1
         (8, 128, 320, 1, 56, 72, 4),          # ntok 64: no padding row at all
         (8, 128, 320, 1, 64, 128, 2),         # ntok 129
         (8, 768, 3072, 2, 16, 16, 2),         # 12 heads, ntok 5
         (16, 128, 320, 2, 128, 128, 4),       # patch 16
         (8, 128, 320, 2, 136, 136, 1),        # ntok 290: more tokens than threads in a workgroup
         (8, 128, 320, 2, 24, 40, 3)]          # ntok 16, h != w
MAIN = (8, 128, 320, 2, 64, 64, 4)


def _id(c):
    return "p%d-D%d-h%d-L%d-%dx%d-B%d" % c


def test_the_case_list_reaches_the_token_counts_it_names():
    assert [1 + (H // p) * (W // p) for p, _, _, _, H, W, _ in CASES] == [65, 65, 65, 65, 2, 64, 129, 5, 65, 290, 16]
    assert sorted({D // 64 for _, D, _, _, _, _, _ in CASES}) == [1, 2, 3, 6, 12]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_native_class_attention_against_fp64(case):
    patch, D, hidden, depth, H, W, B = case
    model, img, ref64, ref32, half, figs = _case(*case)
    ntok = 1 + (H // patch) * (W // patch)
    print("%s: ntok %d | fp64 rel. distance of the class row to uniform %.2f, to token 1's row %.2f, to block 0's class row %s | largest weight %.3f"
          % (_id(case), ntok, figs[0], figs[1], "%.2f" % figs[2] if depth > 1 else "-", float(ref64.max())))
    assert_case_can_fail(figs)
    got = {}
    for p in PRECISIONS:
        nat = vit_native.NativeViT(model, precision=p)
        tokens, attn = nat.forward_tokens_attn(img)
        assert attn.shape == (B, D // 64, ntok) and attn.dtype == torch.float32
        assert torch.equal(tokens, nat.forward_tokens(img)), p
        sums = attn.double().sum(-1)
        print("%s %s: row sums in [%.8f, %.8f]" % (_id(case), p, float(sums.min()), float(sums.max())))
        assert float((sums - 1).abs().max()) <= 1e-5 and float(attn.min()) >= 0, p          # a padding row in the sum fails this
        got[p] = attn
    check_against_fp64(_id(case), got, ref64, ref32, half)


@functools.lru_cache(maxsize=None)
def _long_case():
    """8282 tokens, one head, depth 1: the class row by hand from the three torch evaluations' q and k (softmax(q_cls . k / 8), the same
    definition), so that no [N, N] map is built."""
    patch, D, hidden, depth, H, W, B = 8, 64, 64, 1, 728, 728, 1
    seed = _seed("cls attention", "lds")
    model = build_model(patch, D, hidden, depth, seed).cuda()
    img = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed)).cuda()

    def row(m, x):
        qkv = m.get_intermediate_feat(x, n=1)[2][0]
        return ((qkv[0][:, :, :1] @ qkv[1].transpose(-2, -1)) * 0.125).softmax(-1)[:, :, 0, :]
    with torch.no_grad():
        ref64 = row(_double_of(model), img.double())
        ref32 = row(model, img)
        with torch.autocast("cuda", dtype=torch.float16):
            half = row(model, img).float()
    return model, img, ref64, ref32, half


@pytest.mark.parametrize("precision", PRECISIONS)
def test_more_tokens_than_logits_fit_in_lds(precision):
    """The kernel keeps 8192 logits in LDS and computes the others again in the sum and the store pass: 8282 tokens, the bars of
    check_against_fp64 on the whole row and on the 90 tokens beyond the LDS alone."""
    model, img, ref64, ref32, half = _long_case()
    ntok = ref64.shape[-1]
    assert ntok == 8282 > 8192
    uniform = _rel(torch.full_like(ref64, 1.0 / ntok), ref64)
    tail = float(ref64[..., 8192:].sum())
    print("ntok %d: fp64 rel. distance to uniform %.2f, mass of the tokens beyond 8192 %.5f (uniform: %.5f)" % (ntok, uniform, tail, 90 / ntok))
    assert uniform >= 0.3 and tail > 1e-4
    attn = vit_native.NativeViT(model, precision=precision).forward_tokens_attn(img)[1]
    assert float((attn.double().sum(-1) - 1).abs().max()) <= 1e-5
    check_against_fp64("8282 tokens", {precision: attn}, ref64, ref32, half)
    check_against_fp64("8282 tokens, beyond the LDS", {precision: attn[..., 8192:]}, ref64[..., 8192:], ref32[..., 8192:], half[..., 8192:])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_three_entry_points_interleave_on_one_object(precision):
    model, img = _case(*MAIN)[:2]
    nat = vit_native.NativeViT(model, precision=precision)
    fresh = lambda: vit_native.NativeViT(model, precision=precision)
    want_tokens, want_keys, want_attn = fresh().forward_tokens(img), fresh().forward_keys(img), fresh().forward_tokens_attn(img)
    for _ in range(2):
        assert torch.equal(nat.forward_tokens(img), want_tokens)
        assert torch.equal(nat.forward_keys(img), want_keys)
        tokens, attn = nat.forward_tokens_attn(img)
        assert torch.equal(tokens, want_attn[0]) and torch.equal(attn, want_attn[1]) and torch.equal(tokens, want_tokens)
    assert len(nat._packed) == 1 and len(nat._ws) == 1             # one blob, one workspace for the three entry points


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stale_scratch_never_reaches_the_attention(precision):
    """As tests/test_vit_keys_gpu.py: the cached workspace full of 0xFF bytes before a 2-, a 65- and a 290-token call; each result is
    finite and bitwise a fresh NativeViT's."""
    model = _case(*MAIN)[0]
    nat = vit_native.NativeViT(model, precision=precision)
    later = [(8, 8, 5), (64, 64, 4), (136, 136, 1)]
    gen = torch.Generator("cuda").manual_seed(79)
    imgs = [torch.randn(B, 3, H, W, device="cuda", generator=gen) for H, W, B in later]
    for img in imgs:
        nat.forward_tokens_attn(img)                   # the workspace has its final size: no later call replaces the poisoned buffer
    (dev, ws), = nat._ws.items()
    for img in imgs:
        nat._ws[dev].fill_(255)
        tokens, attn = nat.forward_tokens_attn(img)
        assert nat._ws[dev].data_ptr() == ws.data_ptr()
        f_tokens, f_attn = vit_native.NativeViT(model, precision=precision).forward_tokens_attn(img)
        assert torch.isfinite(attn).all() and torch.isfinite(tokens).all(), tuple(img.shape)
        assert torch.equal(attn, f_attn) and torch.equal(tokens, f_tokens), (tuple(img.shape), float((attn - f_attn).abs().max()))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_attention_is_batch_independent(precision):
    model, img = _case(*MAIN)[:2]
    nat = vit_native.NativeViT(model, precision=precision)
    whole = nat.forward_tokens_attn(img)[1]
    for b in (3, 0):                                   # image 3: rows 195 .. 259, on both sides of the 256-row tile
        assert torch.equal(nat.forward_tokens_attn(img[b:b + 1])[1][0], whole[b]), b


# ------------------------------------------------------------------------------------------------- salience
SYNTH = O.cases()


def _check_salience(tag, attn, h, w, patch, keep):
    """Native masks of a device attention against the oracle on the same numbers."""
    a = attn.cpu().numpy()
    soft, kept, mask, margin = O.salience(a, h, w, patch, keep)
    exact = O.exact_sums(a)
    print("%s: margin %.3e, exact sums %s, kept %s of %d" % (tag, margin.min(), exact, kept.reshape(len(kept), -1).sum(1).tolist(), h * w))
    assert margin.min() >= 1e-9 or exact, tag
    g_soft, g_mask = salience.attention_salience(attn, (h, w), patch, keep)
    assert g_mask.dtype == torch.uint8 and g_mask.shape == mask.shape and g_soft.shape == soft.shape
    g_mask, g_soft = g_mask.cpu().numpy(), g_soft.cpu().numpy().astype(np.float64)
    assert np.array_equal(g_mask[:, ::patch, ::patch] != 0, kept), tag
    assert np.array_equal(g_mask, mask), tag
    rel = np.abs(g_soft - soft) / np.maximum(soft, 1e-300)
    print("%s: soft worst relative error %.3e" % (tag, rel[soft > 0].max() if (soft > 0).any() else 0.0))
    assert (rel[soft > 0] <= 1e-6).all() and (g_soft[soft == 0] == 0).all(), tag


@pytest.mark.parametrize("name", sorted(SYNTH))
def test_native_salience_equals_the_oracle(name):
    attn, h, w, patch, keep = SYNTH[name]
    _check_salience(name, torch.from_numpy(attn).cuda(), h, w, patch, keep)


def test_per_head_masks_and_the_limit_of_the_native_call():
    attn, h, w, patch, keep = SYNTH["h != w, odd w, patch 8"]
    dev = torch.from_numpy(attn).cuda()
    B, heads, n1 = attn.shape
    _, mask = salience.attention_salience(dev, (h, w), patch, keep, per_head=True)
    assert np.array_equal(mask.cpu().numpy(), O.salience(attn.reshape(B * heads, 1, n1), h, w, patch, keep)[2])
    # beyond 4096 patches the torch restatement runs, on the device: the same masks (the margin is asserted)
    rng = np.random.default_rng(5)
    big = rng.random((1, 2, 1 + 65 * 64)).astype(np.float32)
    soft, kept, want, margin = O.salience(big, 65, 64, 8, 0.6)
    assert margin.min() >= 1e-9
    assert np.array_equal(salience.attention_salience(torch.from_numpy(big).cuda(), (65, 64), 8, 0.6)[1].cpu().numpy(), want)


@pytest.mark.parametrize("case", [MAIN, (16, 128, 320, 2, 128, 128, 4), (8, 128, 320, 2, 24, 40, 3)], ids=_id)
def test_native_attention_to_native_mask(case):
    patch, D, hidden, depth, H, W, B = case
    model, img = _case(*case)[:2]
    attn = vit_native.NativeViT(model).forward_tokens_attn(img)[1]
    _check_salience("chain " + _id(case), attn, H // patch, W // patch, patch, 0.6)


# ------------------------------------------------------------------------------------------------- featurizer and training
@pytest.mark.parametrize("feat_type", ["feat", "KK"])
def test_featurizer_returns_the_attention_of_the_same_pass(feat_type):
    from test_vit_keys_gpu import FZ_CASE, _case as keys_case
    model, img = keys_case(*FZ_CASE)[:2]
    fz = _featurizer(feat_type)
    feats, code, attn = fz(img, return_attention=True)
    assert fz.backbone_path == "native" and attn.shape == (4, 3, 65)
    plain_feats, plain_code = fz(img)
    assert torch.equal(feats, plain_feats) and torch.equal(code, plain_code)
    want = vit_native.NativeViT(model).forward_tokens_attn(img)[1]
    assert torch.equal(attn, want) and torch.equal(fz.class_attention(img), want) and fz.backbone_path == "native"
    with pytest.raises(ValueError, match="cache"):
        fz(img, return_attention=True, cache_index=torch.arange(4, device=img.device))
    # the torch module of the same featurizer: row 0 of its maps, the same thing to fp32
    ft = _featurizer(feat_type, native_backbone=False)
    t_attn = ft(img, return_attention=True)[2]
    assert ft.backbone_path == "torch" and _rel(t_attn, want) < 1e-4
    soft, mask = salience.image_salience(fz, img)
    assert soft.shape == (4, 8, 8) and mask.shape == (4, 64, 64) and mask.is_cuda


OV = ["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=4", "feature_samples=5", "neg_samples=2", "dim=10", "dropout=False",
      "use_salience=True", "salience_source=attention"]


@pytest.mark.parametrize("native_salience", [True, False])
def test_training_step_with_attention_salience(native_salience):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    cfg = load_config(overrides=OV + ["native_salience=%s" % native_salience])
    torch.manual_seed(0)
    m = LitUnsupervisedSegmenter(27, cfg).cuda()
    ds = SyntheticContrastiveDataset(4, 64, 27)
    batch = torch.utils.data.default_collate([ds[i] for i in range(4)])
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items() if k not in ("mask", "mask_pos")}
    seen = []
    total = m.contrastive_corr_loss_fn.total

    def spy(signal, signal_pos, sal, sal_pos, *rest):
        seen.append((sal, sal_pos))
        return total(signal, signal_pos, sal, sal_pos, *rest)
    m.contrastive_corr_loss_fn.total = spy
    for step in range(2):
        loss = m.training_step(batch, step)
        assert bool(torch.isfinite(loss)), step
    assert m.net.backbone_path == "native" and all(bool(torch.isfinite(v).all()) for v in m.logged.values() if torch.is_tensor(v))
    for sal in seen[0]:
        assert sal.shape == (4, 64, 64) and sal.dtype == (torch.uint8 if native_salience else torch.float32)
        assert int(sal.reshape(4, -1).sum(1).min()) >= 256                       # at least one patch per image


def test_the_attention_masks_add_no_host_synchronisation():
    """What salience_source = "attention" adds to a step - the backbone pass with the attention and the mask kernel - under torch's
    synchronisation check (where this build honours it) and captured in a graph, as tests/test_salience_gpu.py does for the draw."""
    from test_vit_keys_gpu import FZ_CASE, _case as keys_case
    img = keys_case(*FZ_CASE)[1]
    fz = _featurizer("feat")

    def added():
        feats, code, attn = fz(img, return_attention=True)
        return salience.attention_salience(attn, (8, 8), 8, 0.6)[1]
    eager = added().clone()                              # weights packed, workspace allocated, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").sum().item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            added()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("sync debug mode honoured:", honoured)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        added()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(g):
        mask = added()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(mask, eager)


def test_demo_writes_the_salience_mask_and_the_image_beside_it(tmp_path):
    import os
    from PIL import Image
    from stego_amd import demo_segmentation as D
    from stego_amd.data import image_transform
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    res = 64
    mcfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=%d" % res, "dim=70", "dropout=False"])
    torch.manual_seed(1)
    ck = tmp_path / "demo.ckpt"
    LitUnsupervisedSegmenter(27, mcfg).save_checkpoint(str(ck))
    d = tmp_path / "images"
    d.mkdir()
    rng = np.random.default_rng(2)
    for name, shape in (("wide.jpg", (70, 100, 3)), ("square.png", (64, 64, 3)), ("tall.png", (120, 66, 3))):
        Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8)).save(d / name)
    cfg = load_config(D.DEMO_CONFIG, overrides=["output_root=%s" % tmp_path, "model_path=%s" % ck, "image_dir=%s" % d, "experiment_name=t",
                                                "res=%d" % res, "batch_size=2", "num_workers=0", "run_crf=False", "save_salience=True"])
    written = D.my_app(cfg)
    out = os.path.join(str(tmp_path), "results", "predictions", "t")
    assert len(written) == 6 and sorted(os.listdir(out)) == ["cluster", "linear", "salience", "salience_sheet"]
    loaded = LitUnsupervisedSegmenter.load_from_checkpoint(str(ck)).eval().cuda()
    tf = image_transform(res, "center")
    names = sorted(os.listdir(d))
    img = torch.stack([tf(Image.open(d / n).convert("RGB")) for n in names]).cuda()
    want = salience.image_salience(loaded.net, img, keep=0.6)[1].cpu().numpy()
    for j, n in enumerate(names):
        stem = os.path.splitext(n)[0]
        png = Image.open(os.path.join(out, "salience", stem + ".png"))
        arr = np.asarray(png)
        assert png.mode == "L" and arr.shape == (res, res) and np.array_equal(arr, want[j] * 255) and 0 < want[j].sum() < res * res
        sheet = np.asarray(Image.open(os.path.join(out, "salience_sheet", stem + ".png")))
        assert sheet.shape == (res, 2 * res + 4, 3) and (sheet[:, res:res + 4] == 255).all()
        assert np.array_equal(sheet[:, res + 4:], np.repeat(arr[:, :, None], 3, axis=2))          # the mask, white on black
        assert sheet[:, :res].std() > 10                                                           # ... beside the image
