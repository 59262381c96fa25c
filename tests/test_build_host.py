"""The build's own rules (stego_amd/_build.py) without a GPU and without a compiler: SOURCES lists what csrc/ holds, every header a
source includes is one the stale rule watches, an object goes stale when its source or any header does (for build() and for
build_asan()), and the parser of the compiler's resource remarks reads what hipcc prints."""
import glob
import os
import re

import pytest

from stego_amd import _build

WIDE_PLAN = os.path.join(_build.CSRC, "corr_wide_plan.h")     # the regression: included by three units, once missing from the hand-kept list

# hipcc's stderr for csrc/rec_loss.hip (-Rpass-analysis=kernel-resource-usage), cut down to two of its eight kernels
REC_LOSS_REMARKS = """\
stego_amd/csrc/rec_loss.hip:112:1: remark: Function Name: _ZN12_GLOBAL__N_19rec_tilesILi1EEEvNS_9RecParamsE [-Rpass-analysis=kernel-resource-usage]
  112 | {
      | ^
stego_amd/csrc/rec_loss.hip:112:1: remark:     TotalSGPRs: 76 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:112:1: remark:     VGPRs: 228 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:112:1: remark:     AGPRs: 16 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:112:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:112:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:112:1: remark:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:112:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:112:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:112:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:273:1: remark: Function Name: _ZN12_GLOBAL__N_110rec_finishILi1EEEvNS_9RecParamsEi [-Rpass-analysis=kernel-resource-usage]
  273 | {
      | ^
stego_amd/csrc/rec_loss.hip:273:1: remark:     TotalSGPRs: 68 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:273:1: remark:     VGPRs: 128 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:273:1: remark:     AGPRs: 32 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:273:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:273:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:273:1: remark:     Occupancy [waves/SIMD]: 3 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:273:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:273:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
stego_amd/csrc/rec_loss.hip:273:1: remark:     LDS Size [bytes/block]: 18952 [-Rpass-analysis=kernel-resource-usage]
"""


def test_sources_list_what_the_directory_holds(monkeypatch):
    assert sorted(_build.SOURCES) == sorted(os.path.basename(p) for p in glob.glob(os.path.join(_build.CSRC, "*.hip")))
    assert [os.path.basename(p) for p in _build.sources()] == _build.SOURCES          # the link order
    monkeypatch.setattr(_build, "SOURCES", _build.SOURCES + ["no_such_unit.hip"])
    with pytest.raises(RuntimeError, match="no_such_unit.hip"):
        _build.sources()


def test_every_included_header_is_tracked():
    tracked = {os.path.realpath(h) for h in _build._headers()}
    assert os.path.realpath(WIDE_PLAN) in tracked
    includers = glob.glob(os.path.join(_build.CSRC, "*.hip")) + glob.glob(os.path.join(_build.CSRC, "*.h"))
    seen = 0
    for path in includers:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+\.h)"', open(path).read(), flags=re.M):
            seen += 1
            assert os.path.realpath(os.path.join(os.path.dirname(path), inc)) in tracked, (path, inc)
    assert seen > 100                            # the pattern finds the includes: csrc/ has some 150 of them


@pytest.mark.parametrize("subdir", ["", "asan"], ids=["build", "build_asan"])          # build()'s object directory and build_asan()'s
def test_an_object_goes_stale_with_its_source_and_with_any_header(tmp_path, monkeypatch, subdir):
    monkeypatch.setattr(_build, "OBJ_DIR", str(tmp_path))
    odir = os.path.join(_build.OBJ_DIR, subdir)
    os.makedirs(odir, exist_ok=True)
    src = os.path.join(_build.CSRC, "corr_wide.hip")
    assert _build._obj_stale(src, odir)                      # no object yet
    obj = _build._obj(src, odir)
    open(obj, "w").close()
    deps = _build.sources() + _build._headers() + [_build.__file__]
    newest = max(os.stat(d).st_mtime_ns for d in deps)
    os.utime(obj, ns=(newest + 10 ** 9, newest + 10 ** 9))
    monkeypatch.setattr(_build, "LIB_PATH", obj)             # the library's own rule, build()'s first question: the same files but _build.py
    assert not _build._obj_stale(src, odir) and not _build.is_stale()
    for dep in [WIDE_PLAN, src, os.path.join(_build.INCLUDE, "stego_corr.h")]:
        st = os.stat(dep)
        try:
            os.utime(dep, ns=(st.st_atime_ns, newest + 2 * 10 ** 9))
            assert _build._obj_stale(src, odir) and _build.is_stale(), dep
        finally:
            os.utime(dep, ns=(st.st_atime_ns, st.st_mtime_ns))
        assert os.stat(dep).st_mtime_ns == st.st_mtime_ns and not _build._obj_stale(src, odir) and not _build.is_stale(), dep


def test_the_parser_reads_what_the_compiler_prints():
    figures = {"TotalSGPRs": 76, "VGPRs": 228, "AGPRs": 16, "ScratchSize [bytes/lane]": 0, "Occupancy [waves/SIMD]": 2, "SGPRs Spill": 0,
               "VGPRs Spill": 0, "LDS Size [bytes/block]": 0}
    assert _build.parse_resource_remarks(REC_LOSS_REMARKS) == {
        "_ZN12_GLOBAL__N_19rec_tilesILi1EEEvNS_9RecParamsE": figures,
        "_ZN12_GLOBAL__N_110rec_finishILi1EEEvNS_9RecParamsEi": dict(figures, TotalSGPRs=68, VGPRs=128, AGPRs=32, **{
            "Occupancy [waves/SIMD]": 3, "LDS Size [bytes/block]": 18952})}
    assert _build.parse_resource_remarks("") == {}
