"""Build-time guard for csrc/region_pool.hip: every kernel of the unit compiles for gfx950 with no VGPR / SGPR spills and no scratch, takes
only the 16 bytes of static LDS stego_region_pool_plan reports, and keeps the occupancy the design relies on: the pool kernel hides the
latency of its dependent loads (an id, then the cells of its taps) behind the other waves of the SIMD, so all three must stay at
8 waves a SIMD (at most 64 VGPRs).

Today (VGPRs): range 29, pool 44, finish 22."""
import pytest

from stego_amd import _build

KERNELS = ["region_pool_range_kernel", "region_pool_kernel", "region_pool_finish_kernel"]


def _of(name):
    return {k: v for k, v in _build.kernel_resources("region_pool.hip").items() if ("%d%s" % (len(name), name)) in k}


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_the_unit_has_exactly_these_kernels():
    kernels = _build.kernel_resources("region_pool.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name in KERNELS:
        assert len(_of(name)) == 1, (name, sorted(kernels))


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
@pytest.mark.parametrize("name", KERNELS)
def test_region_pool_kernels_have_no_spills_and_full_occupancy(name):
    for k, v in _of(name).items():
        print(k, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] == 16, (k, v)
        assert v["Occupancy [waves/SIMD]"] == 8 and v["VGPRs"] + v["AGPRs"] <= 64, (k, v)
