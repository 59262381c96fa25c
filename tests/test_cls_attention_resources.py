"""Build-time guard for csrc/vit_cls_attn.hip: every kernel of the unit compiles for gfx950 with no VGPR / SGPR spills and no scratch,
and its static LDS stays within the 64 KB every kernel may use.

Today (VGPRs, LDS bytes): vit_cls_attn_kernel 62 (F16X3) / 58 (F16), 32 800 (8192 logits and the two reduction rounds);
attn_salience_kernel 27, 36 896 (4096 patch weights in fp64, their kept flags, one reduction round)."""
import pytest

from stego_amd import _build

KERNELS = ["vit_cls_attn_kernel", "attn_salience_kernel"]
INSTANCES = {"vit_cls_attn_kernel": 2, "attn_salience_kernel": 1}          # the attention kernel: F16X3 and F16


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_the_unit_has_exactly_these_kernels():
    kernels = _build.kernel_resources("vit_cls_attn.hip")
    assert len(kernels) == sum(INSTANCES.values()), sorted(kernels)
    for name in KERNELS:
        assert sum(("%d%s" % (len(name), name)) in k for k in kernels) == INSTANCES[name], (name, sorted(kernels))


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
@pytest.mark.parametrize("name", KERNELS)
def test_cls_attention_kernels_have_no_spills(name):
    kernels = _build.kernel_resources("vit_cls_attn.hip")
    found = [v for k, v in kernels.items() if ("%d%s" % (len(name), name)) in k]
    assert len(found) == INSTANCES[name]
    for v in found:
        print(name, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["LDS Size [bytes/block]"] <= 64 * 1024, (name, v)
