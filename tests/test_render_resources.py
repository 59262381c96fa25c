"""Build-time guard for csrc/render.hip: the three label-type instantiations of the render kernel and both range kernels compile for
gfx950 with no VGPR / SGPR spills and no scratch, and their static LDS (label tile, row stages, colour table) stays below the 64 KB
every kernel may use: 53 504 bytes with int64 labels (three workgroups per compute unit), 33 920 with int32 or uint8 labels.

Today: 94 / 152 / 48 VGPRs with int64 / int32 / uint8 labels (a thread's label and image loads are all in flight together)."""
import pytest

from stego_amd import _build

INSTANCES = {"labels_i64": "render_kernelIlE", "labels_i32": "render_kernelIiE", "labels_u8": "render_kernelIhE",
             "range_partial": "range_partial_kernel", "range_final": "range_final_kernel"}
TILE, STAGE, TABLE = 17 * 288, 16 * 768, 512 * 4


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
@pytest.mark.parametrize("inst", sorted(INSTANCES))
def test_render_kernels_have_no_spills(inst):
    kernels = _build.kernel_resources("render.hip")
    hits = [v for k, v in kernels.items() if INSTANCES[inst] in k]
    assert len(hits) == 1, (inst, sorted(kernels))
    v = hits[0]
    print(inst, v)
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (inst, v)
    if inst.startswith("labels"):
        assert v["LDS Size [bytes/block]"] == TILE * (8 if inst == "labels_i64" else 4) + STAGE + TABLE, (inst, v)
        assert v["Occupancy [waves/SIMD]"] >= 3, (inst, v)         # three workgroups per compute unit, by LDS and by registers
    else:
        assert v["LDS Size [bytes/block]"] <= 64, (inst, v)
