"""Build-time guard for csrc/feature_pca.hip: every kernel of the unit compiles for gfx950 with no VGPR / SGPR spills and no scratch,
and its static LDS stays within the 64 KB every kernel may use.

Today (VGPRs, LDS bytes): mean_partial 84, 24 576; mean_final 14, 0; gram 97, 35 328 (two staged sides of 64 tokens x 68 floats and
their means); gram_final 18, 0; eigen 200, 53 520 (Q [768][8] in fp64: one workgroup per group, two waves per SIMD by registers);
scores 64, 12 384; score_range 21, 96; paint 36, 12 288 (sixteen row stages of 768 bytes)."""
import pytest

from stego_amd import _build

KERNELS = ["mean_partial_kernel", "mean_final_kernel", "gram_kernel", "gram_final_kernel", "eigen_kernel", "scores_kernel",
           "score_range_kernel", "paint_kernel"]


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_the_unit_has_exactly_these_kernels():
    kernels = _build.kernel_resources("feature_pca.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name in KERNELS:
        assert sum(("%d%s" % (len(name), name)) in k for k in kernels) == 1, (name, sorted(kernels))


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
@pytest.mark.parametrize("name", KERNELS)
def test_feature_pca_kernels_have_no_spills(name):
    kernels = _build.kernel_resources("feature_pca.hip")
    v = [v for k, v in kernels.items() if ("%d%s" % (len(name), name)) in k][0]
    print(name, v)
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (name, v)
    assert v["LDS Size [bytes/block]"] <= 64 * 1024, (name, v)
