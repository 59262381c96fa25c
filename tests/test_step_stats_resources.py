"""Build-time guard for csrc/step_stats.hip: the one kernel of the step statistics compiles for gfx950 with no VGPR / SGPR spills and no
scratch, and its LDS is what its design declares: the 1549 threshold keys, one set of 1548 uint32 counters per wave and the few words
of the workgroup fold - 31 KB, so five workgroups share a compute unit."""
import pytest

from stego_amd import _build


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_step_stats_kernel_has_no_spills():
    kernels = _build.kernel_resources("step_stats.hip")
    assert len(kernels) == 1 and "step_stats_kernel" in next(iter(kernels)), sorted(kernels)     # one launch: one kernel
    waves, limits, buckets = 4, 1549, 1548
    declared = 4 * limits + 4 * waves * buckets                    # keys, per-wave counters
    for k, v in kernels.items():                   # today: 95 VGPRs, 31120 bytes of LDS, 5 waves per SIMD
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert declared <= v["LDS Size [bytes/block]"] <= declared + 256, (k, v, declared)     # + the fold's stage (28 bytes per wave) and a flag
        assert v["VGPRs"] <= 128 and v["Occupancy [waves/SIMD]"] >= 4, (k, v)
