"""Build-time guard for csrc/crf_loss.hip: every kernel of the fused CRF loss compiles for gfx950 with no VGPR / SGPR spills and no
scratch, and keeps the occupancy it has today.

Today (waves/SIMD from the compiler's register count): crf_prepare 8 (48 VGPRs), crf_finish 8 (24); crf_pairs<NT, backward> for
KP = 32 NT channels: <1, 1> 3 (150), <2, 1> 3 (166), <3, 1> 2 (207; K = 70, the training shape: two workgroups of four waves per
compute unit), <4, 1> 2 (243); forward only <1, 0> 4 (105), <2, 0> 3 (130), <3, 0> 3 (138), <4, 0> 3 (156)."""
import pytest

from stego_amd import _build

OCCUPANCY_FLOOR = {"crf_prepare": 8, "crf_finish": 8, "crf_pairsILi1ELb1E": 3, "crf_pairsILi2ELb1E": 3, "crf_pairsILi3ELb1E": 2,
                   "crf_pairsILi4ELb1E": 2, "crf_pairsILi1ELb0E": 4, "crf_pairsILi2ELb0E": 3, "crf_pairsILi3ELb0E": 3,
                   "crf_pairsILi4ELb0E": 3}


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_crf_loss_kernels_have_no_spills():
    kernels = _build.kernel_resources("crf_loss.hip")
    crf = {k: v for k, v in kernels.items() if "crf_" in k}
    assert len(crf) == len(OCCUPANCY_FLOOR), sorted(kernels)
    for k, v in crf.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        floor = [f for key, f in OCCUPANCY_FLOOR.items() if key in k]
        assert len(floor) == 1 and v["Occupancy [waves/SIMD]"] >= floor[0], (k, v)
