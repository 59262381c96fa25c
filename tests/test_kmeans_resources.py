"""Build-time guard for csrc/code_kmeans.hip: every kernel of the unit compiles for gfx950 with no VGPR / SGPR spills and no scratch,
and its static LDS stays within the 64 KB every kernel may use (the main launch's LDS is dynamic: stego_kmeans_plan reports it, and
tests/test_kmeans_host.py pins it below the 160 KB of a compute unit).

Today (VGPRs + AGPRs), strided / dense read: assign<1, *> 94 + 32 / 101 .. 151 + 32 (one centroid tile: one output tile of the sums per
wave; the dense read holds a tile's 4 * CT float4 per thread while they are in flight), assign<2, 1..2> 122 + 48 / 122 .. 129 + 48,
assign<2, 3..4> 184 + 64 / 204 .. 221 + 64 (two score tiles, two output tiles with their fp64 accumulators: one wave per SIMD with the
dense read, two without); finish 26, seed_weigh 38, seed_pick 30."""
import pytest

from stego_amd import _build

KERNELS = {"kmeans_assign_kernel": 16, "kmeans_finish_kernel": 1, "kmeans_seed_weigh_kernel": 1, "kmeans_seed_pick_kernel": 1}


def _of(name):
    return {k: v for k, v in _build.kernel_resources("code_kmeans.hip").items() if ("%d%s" % (len(name), name)) in k}


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
def test_the_unit_has_exactly_these_kernels():
    kernels = _build.kernel_resources("code_kmeans.hip")
    assert len(kernels) == sum(KERNELS.values()), sorted(kernels)
    for name, count in KERNELS.items():
        assert len(_of(name)) == count, (name, sorted(kernels))
    assert sorted(k[k.index("kernelI") + 6:k.index("EEEv")] for k in _of("kmeans_assign_kernel")) == \
        sorted("ILi%dELi%dELb%d" % (nt, ct, dense) for nt in (1, 2) for ct in (1, 2, 3, 4) for dense in (0, 1))
    # <centroid tiles, channel tiles, the dense channels-last read>


@pytest.mark.skipif(not _build.have_hipcc(), reason="needs hipcc")
@pytest.mark.parametrize("name", sorted(KERNELS))
def test_kmeans_kernels_have_no_spills(name):
    for k, v in _of(name).items():
        print(k, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] <= 64 * 1024, (k, v)
