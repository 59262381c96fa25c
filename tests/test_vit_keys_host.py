"""stego_vit_forward_keys (include/stego_vit.h: the last block's attention keys, the reference's feat_type "KK") without a GPU:
the symbol and the ABI version, its argument checks - the same codes in the same order as stego_vit_forward, all of them before
any device call (the pointers below are made-up addresses, never dereferenced) - and the torch fallback of a "KK" featurizer on
the CPU."""
import ctypes

import pytest
import torch

from stego_amd import _build, capi, dino_vit

OK, ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, ERR_ALIGN = 0, 1, 2, 3, 4, 5      # include/stego_corr.h
FAKE = 0x7F0000001000            # 4 KiB aligned, non-null


def _desc(B=2, H=64, W=64, patch=8, D=128, depth=2, heads=2, hidden=320, precision=capi.VIT_F16X3):
    return capi.StegoVitDesc(B, H, W, patch, D, depth, heads, hidden, precision)


def _call(name, d, packed=FAKE, img=FAKE + 0x100000, out=FAKE + 0x200000, ws=FAKE + 0x300000, ws_bytes=None):
    lib = capi.load()
    if ws_bytes is None:
        ws_bytes = int(lib.stego_vit_workspace_bytes(ctypes.byref(d)))
    return int(getattr(lib, name)(ctypes.byref(d), packed, img, out, ws, ws_bytes, None))


def test_the_library_exports_the_keys_entry_point_at_abi_7():
    lib = capi.load()
    assert lib.stego_abi_version() == 7
    assert ctypes.cast(lib.stego_vit_forward_keys, ctypes.c_void_p).value


def test_argument_checks_return_before_any_device_call():
    d = _desc()
    assert int(capi.load().stego_vit_workspace_bytes(ctypes.byref(d))) > 0
    assert _call("stego_vit_forward_keys", d, ws_bytes=0) == ERR_WORKSPACE
    assert _call("stego_vit_forward_keys", d, out=None) == ERR_NULL
    assert _call("stego_vit_forward_keys", d, packed=None) == ERR_NULL
    assert _call("stego_vit_forward_keys", d, ws=FAKE + 0x300000 + 128) == ERR_ALIGN        # workspace: 256 bytes
    assert _call("stego_vit_forward_keys", d, img=FAKE + 0x100000 + 4) == ERR_ALIGN         # image: 16 bytes
    assert _call("stego_vit_forward_keys", _desc(depth=1), ws_bytes=0) == ERR_WORKSPACE      # depth 1 is a legal descriptor


def test_refused_descriptors_get_the_code_of_the_token_forward():
    ntok = 65
    assert (1 << 20) % 64 == 0
    cases = [_desc(heads=3),                                        # heads * 64 != D
             _desc(B=(1 << 20) // 64, H=56, W=72),                  # B * ntok = 2^20 (ntok 64)
             _desc(patch=4), _desc(H=60), _desc(D=832, heads=13), _desc(precision=2), _desc(B=0)]
    for d in cases:
        want = _call("stego_vit_forward", d, ws_bytes=1 << 40)
        assert want in (ERR_SHAPE, ERR_UNSUPPORTED), want
        assert _call("stego_vit_forward_keys", d, ws_bytes=1 << 40) == want
        assert _call("stego_vit_forward_keys", d, out=None, ws_bytes=0) == want           # the descriptor is judged first
    assert _call("stego_vit_forward_keys", _desc(heads=3)) == ERR_UNSUPPORTED
    assert _call("stego_vit_forward_keys", _desc(B=(1 << 20) // 64, H=56, W=72)) == ERR_UNSUPPORTED
    assert _call("stego_vit_forward_keys", _desc(B=((1 << 20) - 1) // ntok), ws_bytes=0) == ERR_WORKSPACE      # just inside the guard
    lib = capi.load()
    assert int(lib.stego_vit_forward_keys(None, FAKE, FAKE, FAKE, FAKE, 0, None)) == ERR_NULL


def test_every_width_keeps_the_key_columns_inside_the_packed_qkv_weight():
    """The K third's column tiles read weight rows [D, D + 192 * ceil(D / 192)); the packed QKV weight holds
    128 * ceil(192 * ceil(3 D / 192) / 128) rows (zero beyond 3 D).  The library checks this itself: no supported width is refused."""
    for D in range(64, 769, 64):
        last = D + 192 * -(-D // 192)
        have = 128 * -(-(192 * -(-3 * D // 192)) // 128)
        assert last <= have, (D, last, have)
        assert _call("stego_vit_forward_keys", _desc(D=D, heads=D // 64, hidden=D), ws_bytes=0) == ERR_WORKSPACE, D


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_the_keys_kernel_keeps_the_register_budget_of_the_gemm():
    """vit_keys_kernel is the GEMM tile of vit_gemm_kernel with another epilogue: like it, two 512-thread workgroups per CU
    (occupancy >= 4 waves per SIMD) and nothing spilled inside the k loop (tests/test_kernel_resources.py: at most 8 registers)."""
    kernels = _build.kernel_resources("vit_forward.hip")
    keys = {k: v for k, v in kernels.items() if "vit_keys_kernel" in k}
    assert len(keys) == 2, sorted(kernels)                       # two precisions
    for k, v in keys.items():
        assert v["Occupancy [waves/SIMD]"] >= 4 and v["VGPRs Spill"] <= 8, (k, v)


def test_kk_featurizer_on_the_cpu_keeps_the_torch_module_bit_for_bit():
    from stego_amd import featurizers

    class C:
        dino_patch_size = 16; dino_feat_type = "KK"; model_type = "vit_tiny"; projection_type = None
        dropout = False; pretrained_weights = None
    torch.manual_seed(3)
    fz = featurizers.DinoFeaturizer(70, C()).cpu().eval()
    img = torch.randn(2, 3, 64, 48)
    feats, code = fz(img)
    assert fz.backbone_path == "torch"
    with torch.no_grad():
        feat, _, qkv = fz.model.get_intermediate_feat(img, n=1)
        k = qkv[0][1, :, :, 1:, :]
        Bn, heads, _, d = k.shape
        want = k.reshape(Bn, heads, 4, 3, d).permute(0, 1, 4, 2, 3).reshape(Bn, heads * d, 4, 3)
    assert feats.shape == (2, 192, 4, 3) and torch.equal(feats, want) and code is feats
    cls = fz(img, return_class_feat=True)
    assert fz.backbone_path == "torch"
    assert torch.equal(cls, feat[0][:, :1, :].reshape(2, 1, 1, -1).permute(0, 3, 1, 2))
    assert isinstance(fz.model, dino_vit.VisionTransformer)
