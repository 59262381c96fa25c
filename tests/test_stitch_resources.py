"""Build-time guard for csrc/stitch_probe.hip: every instantiation of the stitch kernel (8, 16 and 32 label slots with both probes in
one walk over the windows; 64 label slots with one probe each, as a loop-free launch for the pixels under one window and a walk for
the pixels under several) and the window gather compile for gfx950 with no VGPR / SGPR spills and no scratch, use dynamic LDS only,
and the plan that sizes that LDS stays within its 64 KiB budget.

Today: 96 / 158 / 198 VGPRs at 8 / 16 / 32 slots (5 / 3 / 2 waves per SIMD); at 64 slots 170 / 170 (one window) and 182 / 196
(several) for the linear / cluster probe, 2 waves."""
import pytest

from stego_amd import _build

LDS_BUDGET = 64 * 1024
INSTANCES = {"slots8": "stitch_probe_kernelILi8ELb1ELb1E", "slots16": "stitch_probe_kernelILi16ELb1ELb1E",
             "slots32": "stitch_probe_kernelILi32ELb1ELb1E", "slots64_linear_sole": "stitch_probe_kernelILi64ELb1ELb0ELi1E",
             "slots64_linear_blend": "stitch_probe_kernelILi64ELb1ELb0ELi2E", "slots64_cluster_sole": "stitch_probe_kernelILi64ELb0ELb1ELi1E",
             "slots64_cluster_blend": "stitch_probe_kernelILi64ELb0ELb1ELi2E", "gather": "window_gather_kernel"}


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_every_instantiation_is_there():
    kernels = _build.kernel_resources("stitch_probe.hip")
    assert sum("stitch_probe_kernel" in k for k in kernels) == 7 and sum("window_gather_kernel" in k for k in kernels) == 1, sorted(kernels)


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
@pytest.mark.parametrize("inst", sorted(INSTANCES))
def test_stitch_kernel_has_no_spills(inst):
    kernels = _build.kernel_resources("stitch_probe.hip")
    hits = [v for k, v in kernels.items() if INSTANCES[inst] in k]
    assert len(hits) == 1, (inst, sorted(kernels))
    v = hits[0]
    print(inst, v)
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (inst, v)
    assert v["LDS Size [bytes/block]"] == 0, (inst, v)                 # no static LDS: the plan's dynamic bytes are all there is


@pytest.mark.parametrize("K,n", [(70, 27), (128, 64), (16, 3), (1, 1)])
@pytest.mark.parametrize("hc,wc,win", [(40, 40, 320), (3, 3, 48), (5, 5, 40), (28, 28, 224), (2048, 2048, 7), (1, 1, 2048), (65535, 3, 2)])
def test_planned_lds_stays_within_budget(K, n, hc, wc, win):
    from stego_amd import capi
    desc = capi.stitch_desc(2 * win + 3, 3 * win + 1, win, (win + 1) // 2, 1, K, hc, wc, n, n, capi.PROBE_PROBS, capi.PROBE_PROBS, 2.0)
    lds, ty, tx, ny, nx = capi.stitch_probe_plan(desc)
    assert 0 < lds <= LDS_BUDGET, lds
    slots = 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64
    floats_per_px = ((K + 3) // 4 * 4 + 4) + 2 * slots + 4
    # the footprint of a ty x tx tile is at least one code pixel: the plan holds it, both masks and the copy of the parameters (64 floats)
    assert lds >= 4 * (floats_per_px + 4 * slots + 64)
    assert (lds - 4 * (4 * slots + 64)) % (4 * floats_per_px) == 0
