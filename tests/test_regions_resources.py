"""Build-time guard for csrc/regions.hip: every kernel of the unit compiles for gfx950 with no VGPR / SGPR spills and no scratch, and its
static LDS stays within the 64 KB every kernel may use (none of them takes dynamic LDS: stego_regions_plan reports the static bytes).

Today (VGPRs): tile 17 (12 KB of LDS: the tile's labels and parents), seam 14, flatten 14, scan 18, number 21, spread 8; table reset 10,
add 25, finish 10; votes reset 3, votes 47, relabel 13."""
import pytest

from stego_amd import _build

KERNELS = ["regions_tile_kernel", "regions_seam_kernel", "regions_flatten_kernel", "regions_scan_kernel", "regions_number_kernel",
           "regions_spread_kernel", "regions_table_reset_kernel", "regions_table_add_kernel", "regions_table_finish_kernel",
           "regions_votes_reset_kernel", "regions_votes_kernel", "regions_relabel_kernel"]


def _of(name):
    return {k: v for k, v in _build.kernel_resources("regions.hip").items() if ("%d%s" % (len(name), name)) in k}


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_the_unit_has_exactly_these_kernels():
    kernels = _build.kernel_resources("regions.hip")
    assert len(kernels) == len(KERNELS), sorted(kernels)
    for name in KERNELS:
        assert len(_of(name)) == 1, (name, sorted(kernels))


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
@pytest.mark.parametrize("name", KERNELS)
def test_regions_kernels_have_no_spills(name):
    for k, v in _of(name).items():
        print(k, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] <= 64 * 1024, (k, v)
