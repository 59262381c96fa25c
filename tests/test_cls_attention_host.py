"""Class-token attention maps and attention salience masks (include/stego_vit.h: stego_vit_forward_attn, stego_attn_salience) without a
GPU: the symbols and the ABI version, the argument checks - all before any device call, the pointers below are made-up addresses, never
dereferenced -, the torch restatement of the salience definition against the numpy oracle (tests/attn_salience_oracle.py), the torch
path of the attention (get_last_selfattention, DinoFeaturizer.class_attention / return_attention) and cfg.salience_source."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import attn_salience_oracle as O
import oracle_backend
from stego_amd import capi, dino_vit, featurizers, salience
from stego_amd import modules as M
from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config

warnings.filterwarnings("ignore", message="DinoFeaturizer")

OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_ALIGN = 0, 1, 2, 3, 4, 5      # include/stego_corr.h
FAKE = 0x7F0000001000            # 4 KiB aligned, non-null
CASES = O.cases()


def _desc(B=2, H=64, W=64, patch=8, D=128, depth=2, heads=2, hidden=320, precision=capi.VIT_F16X3):
    return capi.StegoVitDesc(B, H, W, patch, D, depth, heads, hidden, precision)


def _forward_attn(d, packed=FAKE, img=FAKE + 0x100000, out=FAKE + 0x200000, attn=FAKE + 0x400000, ws=FAKE + 0x300000, ws_bytes=None):
    lib = capi.load()
    if ws_bytes is None:
        ws_bytes = int(lib.stego_vit_workspace_bytes(ctypes.byref(d)))
    return int(lib.stego_vit_forward_attn(ctypes.byref(d), packed, img, out, attn, ws, ws_bytes, None))


def _salience(attn=FAKE, B=2, heads=3, h=4, w=5, patch=8, keep=0.6, soft=FAKE + 0x100000, mask=FAKE + 0x200000):
    return int(capi.load().stego_attn_salience(attn, B, heads, h, w, patch, keep, soft, mask, None))


def test_the_library_exports_both_entry_points_at_abi_7():
    lib = capi.load()
    assert lib.stego_abi_version() == 7 and capi.ABI_VERSION == 7
    header = open(capi._build.INCLUDE + "/stego_vit.h").read()
    for name in ("stego_vit_forward_attn", "stego_attn_salience"):
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value and name in capi.SIGNATURES and (name + "(") in header, name


def test_forward_attn_checks_its_arguments_before_any_device_call():
    d = _desc()
    assert _forward_attn(d, ws_bytes=0) == ERR_WORKSPACE
    for arg in ("packed", "img", "out", "attn", "ws"):
        assert _forward_attn(d, **{arg: None}) == ERR_NULL, arg
    assert _forward_attn(d, attn=FAKE + 0x400000 + 2) == ERR_ALIGN                  # the attention: 4 bytes
    assert _forward_attn(d, ws=FAKE + 0x300000 + 128, ws_bytes=1 << 40) == ERR_ALIGN
    assert _forward_attn(d, img=FAKE + 0x100000 + 4, ws_bytes=1 << 40) == ERR_ALIGN
    assert int(capi.load().stego_vit_forward_attn(None, FAKE, FAKE, FAKE, FAKE, FAKE, 0, None)) == ERR_NULL
    # a refused descriptor gets the token forward's code, and the descriptor is judged first
    for bad in (_desc(heads=3), _desc(patch=4), _desc(H=60), _desc(precision=2), _desc(B=0)):
        want = int(capi.load().stego_vit_forward(ctypes.byref(bad), FAKE, FAKE, FAKE, FAKE, 1 << 40, None))
        assert want in (ERR_SHAPE, ERR_UNSUPPORTED)
        assert _forward_attn(bad, ws_bytes=1 << 40) == want and _forward_attn(bad, attn=None, ws_bytes=0) == want


def test_salience_checks_its_arguments_before_any_device_call():
    assert _salience(attn=None) == ERR_NULL
    for keep in (0.0, -0.25, 1.5, float("nan")):
        assert _salience(keep=keep) == ERR_SHAPE, keep
    assert _salience(h=1, w=4097) == ERR_UNSUPPORTED and _salience(h=4097, w=4097) == ERR_UNSUPPORTED      # h * w > 4096
    assert _salience(patch=4) == ERR_UNSUPPORTED and _salience(patch=12) == ERR_UNSUPPORTED
    for dim in ("B", "heads", "h", "w"):
        assert _salience(**{dim: 0}) == ERR_SHAPE and _salience(**{dim: -1}) == ERR_SHAPE, dim
    assert _salience(attn=FAKE + 2) == ERR_ALIGN and _salience(soft=FAKE + 0x100000 + 2) == ERR_ALIGN
    assert _salience(mask=FAKE + 0x200000 + 8) == ERR_ALIGN                          # the mask leaves in 16-byte stores
    assert _salience(soft=None, mask=None) == OK                                     # nothing asked for: nothing enqueued


# ------------------------------------------------------------------------------------------------- the definition
def test_the_oracle_on_inputs_whose_answer_is_known():
    attn, h, w, patch, keep = CASES["uniform 8x8 keep 0.6"]
    soft, kept, mask, margin = O.salience(attn, h, w, patch, keep)
    assert kept.reshape(2, -1).sum(1).tolist() == [39, 39] and kept.reshape(2, -1)[:, :39].all()      # exact ties: the index decides
    assert abs(margin[0] - 0.00625) < 1e-6 and np.allclose(soft, 1 / 64) and mask.shape == (2, 64, 64)
    attn, h, w, patch, keep = CASES["keep 1e-6"]
    soft, kept, _, _ = O.salience(attn, h, w, patch, keep)
    flat = kept.reshape(len(kept), -1)
    assert (flat.sum(1) == 1).all() and (flat.argmax(1) == soft.reshape(len(kept), -1).argmax(1)).all()
    for name in ("keep 1.0", "keep 1.0, softmax"):
        attn, h, w, patch, keep = CASES[name]
        soft, kept, _, _ = O.salience(attn, h, w, patch, keep)
        assert np.array_equal(kept, soft > 0), name
    assert not O.salience(*CASES["keep 1.0"])[1].all()                             # ... and some patch has no mass there


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_synthetic_input_decides_clearly(name):
    """Equality with the oracle is demanded where its margin is at least 1e-9, or every sum is exact in any order: each input is one or
    the other, so no case is ever let off."""
    attn, h, w, patch, keep = CASES[name]
    margin = O.salience(attn, h, w, patch, keep)[3]
    print(name, "margin", margin.min(), "exact sums", O.exact_sums(attn))
    assert margin.min() >= 1e-9 or O.exact_sums(attn)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_torch_restatement_equals_the_oracle(name):
    attn, h, w, patch, keep = CASES[name]
    soft, kept, mask, _ = O.salience(attn, h, w, patch, keep)
    t_soft, t_mask = salience.torch_attention_salience(torch.from_numpy(attn), (h, w), patch, keep)
    assert t_mask.dtype == torch.uint8 and t_soft.dtype == torch.float32
    assert np.array_equal(t_mask.numpy(), mask)
    assert np.array_equal(t_soft.numpy(), soft.astype(np.float32))
    # the public call takes the restatement for a CPU tensor; per_head is the same call on [B * heads, 1, n]
    p_soft, p_mask = salience.attention_salience(torch.from_numpy(attn), (h, w), patch, keep)
    assert torch.equal(p_mask, t_mask) and torch.equal(p_soft, t_soft)
    B, heads, n1 = attn.shape
    h_soft, h_mask = salience.attention_salience(torch.from_numpy(attn), (h, w), patch, keep, per_head=True)
    want = O.salience(attn.reshape(B * heads, 1, n1), h, w, patch, keep)
    assert h_mask.shape[0] == B * heads and np.array_equal(h_mask.numpy(), want[2])


def test_attention_salience_refuses_what_the_definition_does_not_cover():
    attn = torch.from_numpy(CASES["one patch"][0])
    with pytest.raises(ValueError):
        salience.attention_salience(attn, (2, 2), 8)
    for keep in (0.0, 1.5):
        with pytest.raises(ValueError):
            salience.attention_salience(attn, (1, 1), 8, keep=keep)


# ------------------------------------------------------------------------------------------------- the torch path of the attention
def _featurizer(feat_type="feat"):
    class C:
        dino_patch_size = 16; dino_feat_type = feat_type; model_type = "vit_tiny"; projection_type = "nonlinear"
        dropout = False; pretrained_weights = None; native_backbone = True
    torch.manual_seed(3)
    return featurizers.DinoFeaturizer(70, C()).cpu().eval()


def test_get_last_selfattention_is_the_last_block_s_softmax():
    torch.manual_seed(5)
    model = dino_vit.VisionTransformer(img_size=(32,), patch_size=8, embed_dim=128, depth=2, num_heads=2, mlp_ratio=2.5).eval()
    img = torch.randn(3, 3, 32, 48)
    with torch.no_grad():
        attn = model.get_last_selfattention(img)
        feats, attns, qkvs = model.get_intermediate_feat(img, n=2, need_attn=True)
    assert attn.shape == (3, 2, 25, 25)
    assert float((attn.sum(-1) - 1).abs().max()) < 1e-5 and float(attn.min()) >= 0
    q, k = qkvs[-1][0], qkvs[-1][1]
    assert torch.allclose(attn, ((q @ k.transpose(-2, -1)) * 0.125).softmax(-1), atol=1e-6)
    assert torch.allclose(attn, attns[-1], atol=1e-6) and not torch.equal(attns[-1], attns[0])
    assert torch.equal(attn, model.get_intermediate_feat(img, n=1, need_attn=True)[1][0])


@pytest.mark.parametrize("feat_type", ["feat", "KK"])
def test_class_attention_on_a_cpu_model_is_row_0_of_the_torch_maps(feat_type):
    fz = _featurizer(feat_type)
    img = torch.randn(2, 3, 64, 48)
    with torch.no_grad():
        want = fz.model.get_last_selfattention(img)[:, :, 0, :]
    got = fz.class_attention(img)
    assert fz.backbone_path == "torch" and got.shape == (2, 3, 13) and torch.equal(got, want)
    feats, code, attn = fz(img, return_attention=True)
    assert torch.equal(attn, want)
    plain_feats, plain_code = fz(img)
    assert feats.shape == plain_feats.shape and torch.allclose(feats, plain_feats, atol=1e-4) and torch.allclose(code, plain_code, atol=1e-4)
    fz.enable_token_cache(4, (64, 48), "cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match="cache"):
        fz(img, return_attention=True, cache_index=torch.tensor([0, 1]))
    soft, mask = salience.image_salience(fz, img, keep=0.6)
    assert soft.shape == (2, 4, 3) and mask.shape == (2, 64, 48) and mask.dtype == torch.uint8
    assert np.array_equal(mask.numpy(), O.salience(want.numpy(), 4, 3, 16, 0.6)[2])


# ------------------------------------------------------------------------------------------------- training
TINY = ["model_type=vit_tiny", "dino_patch_size=16", "res=32", "batch_size=3", "feature_samples=3", "neg_samples=2", "dim=6", "max_steps=2"]


def test_the_config_ships_the_mask_source_and_refuses_attention_with_the_token_cache():
    cfg = load_config()
    assert cfg.salience_source == "mask" and cfg.salience_keep == 0.6 and cfg.use_salience is False
    from stego_amd.demo_segmentation import DEMO_CONFIG
    assert load_config(DEMO_CONFIG).save_salience is False
    with pytest.raises(ValueError, match="cache_backbone_tokens"):
        LitUnsupervisedSegmenter(27, load_config(overrides=TINY + ["salience_source=attention", "cache_backbone_tokens=True"]))
    with pytest.raises(ValueError, match="salience_source"):
        LitUnsupervisedSegmenter(27, load_config(overrides=TINY + ["salience_source=labels"]))


def test_a_training_step_draws_from_attention_masks_and_never_reads_the_batch_s():
    M._backend = oracle_backend
    try:
        cfg = load_config(overrides=TINY + ["use_salience=True", "salience_source=attention"])
        torch.manual_seed(0)
        m = LitUnsupervisedSegmenter(27, cfg).cpu()          # (the featurizer puts its backbone on a GPU where there is one)
        ds = SyntheticContrastiveDataset(6, cfg.res, 27, seed=0)
        batch = torch.utils.data.default_collate([ds[i] for i in range(cfg.batch_size)])
        batch.pop("mask", None)
        batch.pop("mask_pos", None)
        seen = []
        total = m.contrastive_corr_loss_fn.total

        def spy(signal, signal_pos, sal, sal_pos, *rest):
            seen.append((sal, sal_pos))
            return total(signal, signal_pos, sal, sal_pos, *rest)
        m.contrastive_corr_loss_fn.total = spy
        loss = m.training_step(batch, 0)
        assert torch.isfinite(loss) and len(seen) == 1
        for sal, img in zip(seen[0], (batch["img"], batch["img_pos"])):
            assert sal.shape == (3, 32, 32) and sal.dtype == torch.float32
            assert (sal.reshape(3, -1).sum(1) >= 256).all() and set(sal.unique().tolist()) <= {0.0, 1.0}      # at least one patch each
            want = salience.image_salience(m.net, img, keep=0.6)[1]
            assert torch.equal(sal, want.float())
    finally:
        M._backend = capi
