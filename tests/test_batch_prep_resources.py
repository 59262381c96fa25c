"""Build-time guard for csrc/batch_prep.hip: both instantiations of the batch-preparation kernel (16 pixels per lane with 16-byte
stores, and the one-pixel form for R % 4 != 0) compile without spills and keep the occupancy they have today."""
import pytest

from stego_amd import _build


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_batch_prep_kernel_has_no_spills():
    kernels = _build.kernel_resources("batch_prep.hip")
    prep = {k: v for k, v in kernels.items() if "batch_prep_kernel" in k}
    assert len(prep) == 2, sorted(kernels)
    for k, v in prep.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["Occupancy [waves/SIMD]"] >= 4, (k, v)          # 102 registers at 16 pixels per lane today
