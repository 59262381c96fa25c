"""Build-time guard for csrc/batch_prep_dir.hip and csrc/salience_draw.hip: both instantiations of the directory batch-preparation
kernel (16 pixels per lane with 16-byte stores, and the one-pixel form for R % 4 != 0) and both of the salience draw (float32 and
one-byte masks) compile for gfx950 without spills or scratch and keep the occupancy they have today."""
import pytest

from stego_amd import _build


def _no_spills(k, v):
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_dir_prep_kernel_has_no_spills():
    kernels = _build.kernel_resources("batch_prep_dir.hip")
    prep = {k: v for k, v in kernels.items() if "dir_prep_kernel" in k}
    assert len(prep) == 2 and not any("batch_prep_kernel" in k for k in kernels), sorted(kernels)
    for k, v in prep.items():
        _no_spills(k, v)
        vec = "ILi16E" in k
        assert v["Occupancy [waves/SIMD]"] >= (4 if vec else 8), (k, v)      # 106 registers at 16 pixels per lane today, 13 at one
        assert v["LDS Size [bytes/block]"] == 3 * 256 * 4, (k, v)


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_salience_draw_kernel_has_no_spills():
    kernels = _build.kernel_resources("salience_draw.hip")
    draw = {k: v for k, v in kernels.items() if "salience_draw_kernel" in k}
    assert len(draw) == 2, sorted(kernels)
    for k, v in draw.items():
        _no_spills(k, v)
        assert v["Occupancy [waves/SIMD]"] >= 8, (k, v)                      # 19 registers today; 1024 threads are 4 waves per SIMD
        assert v["LDS Size [bytes/block]"] <= 40 * 1024, (k, v)              # 35856 today: four workgroups of a compute unit's 160 KB
