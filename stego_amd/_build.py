"""Build libstego_corr.so (HIP kernels + C ABI) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting
``stego_amd/lib/libstego_corr.so`` is git-ignored but travels to the GPU box with the
repo snapshot.  No torch headers are involved: the library is plain C ABI.

Every source is compiled to its own object (``stego_amd/lib/obj/*.o``, in parallel, only when it or a header
changed) and the objects are linked into the one shared library: a one-kernel edit rebuilds in seconds.
The sources are listed (``SOURCES``: the link order); the headers are found (every ``*.h`` of ``csrc/`` and ``include/``).
"""
import functools
import glob
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
LIB_DIR = os.path.join(HERE, "lib")
OBJ_DIR = os.path.join(LIB_DIR, "obj")
LIB_PATH = os.path.join(LIB_DIR, "libstego_corr.so")
SOURCES = ["corr_sample.hip", "corr_fwd.hip", "corr_fused.hip", "corr_fused_odd.hip", "corr_fused_c192.hip", "corr_fused_half.hip", "corr_bwd.hip", "corr_bwd_lists.hip", "knn_topk.hip", "dense_corr.hip", "dense_stream.hip", "sample_sets.hip", "loss_pointwise.hip", "corr_wide.hip", "vit_forward.hip", "vit_cls_attn.hip", "host_util.hip", "draws.hip", "head_fused.hip", "dense_crf.hip", "batch_prep.hip", "batch_prep_dir.hip", "salience_draw.hip", "probe_head.hip", "probe_train.hip", "corr_pr.hip", "corr_heat.hip", "crf_loss.hip", "augment.hip", "confusion.hip", "optim_step.hip", "stitch_probe.hip", "rec_loss.hip", "render.hip", "step_stats.hip", "feature_pca.hip", "code_kmeans.hip", "regions.hip", "region_pool.hip", "c_api.hip"]
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
LDFLAGS = ["--offload-arch=gfx950", "-fPIC", "-shared"]
# the one torch C++ extension (host only, g++): the autograd function of the loss and the generator's graph-safe Philox state, over the C ABI
# measurement only (bench.py's roofline.frac_of_skeleton): the traffic skeleton of the fused forward, a stand-alone binary beside the library
SKELETON_SRC = os.path.join(HERE, "..", "tools", "ubench", "fused_skeleton.hip")
SKELETON_PATH = os.path.join(LIB_DIR, "fused_skeleton.bin")
TORCHGLUE_SRC = os.path.join(CSRC, "torch_glue_ext.cpp")
TORCHGLUE_PATH = os.path.join(LIB_DIR, "_stego_torchglue.so")


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def have_hipcc():
    """Whether this machine can compile the kernels at all: what the build-time guards of tests/ skip on."""
    return os.path.exists(HIPCC)


def _hipcc():
    if not have_hipcc():
        raise RuntimeError("hipcc not found (need ROCm with gfx950 support)")
    return HIPCC


def sources():
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    missing = [s for s in srcs if not os.path.exists(s)]
    if missing:
        raise RuntimeError("SOURCES names files that do not exist: " + ", ".join(missing))
    return srcs


def _headers():
    return sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(INCLUDE, "*.h")))


def _obj(src, odir=None):
    return os.path.join(odir or OBJ_DIR, os.path.splitext(os.path.basename(src))[0] + ".o")


def _obj_stale(src, odir=None):
    """An object is stale when its source, any header or this file is newer than it."""
    o = _obj(src, odir)
    if not os.path.exists(o):
        return True
    t = os.path.getmtime(o)
    return any(os.path.getmtime(d) > t for d in [src, os.path.abspath(__file__)] + _headers())


def is_stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(d) > t for d in sources() + _headers())


def _run(cmd, what, verbose):
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("%s failed:\n%s%s" % (what, res.stdout, res.stderr))
    return res.stderr


def _compile_objects(srcs, odir, flags, force, verbose):
    """Compile the stale ones of `srcs` (all of them with `force`) into `odir`, in parallel; returns the sources it compiled."""
    os.makedirs(odir, exist_ok=True)
    todo = [s for s in srcs if force or _obj_stale(s, odir)]

    def one(src):
        _run([_hipcc()] + flags + ["-c", src, "-o", _obj(src, odir) + ".tmp"], "hipcc on " + src, verbose)
        os.replace(_obj(src, odir) + ".tmp", _obj(src, odir))

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(todo)))) as ex:
        list(ex.map(one, todo))
    return todo


def _link(inputs, flags, out, verbose):
    _run([_hipcc()] + flags + inputs + ["-o", out + ".tmp"], "hipcc link", verbose)
    os.replace(out + ".tmp", out)
    return out


def build(force=False, verbose=False, extra_flags=(), out=None):
    """Compile every HIP source (objects cached per file) and link the shared library. Returns the library path.
    `extra_flags` (e.g. -DSTEGO_FUSED_TIMELINE) force a full rebuild into `out` without touching the object cache."""
    out = out or LIB_PATH
    if not force and not extra_flags and out == LIB_PATH and not is_stale():
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    srcs = sources()
    if extra_flags:                       # one-off variant build: everything in one go, no cache
        return _link(srcs, CFLAGS + list(extra_flags) + ["-shared"], out, False)
    _compile_objects(srcs, OBJ_DIR, CFLAGS, force, verbose)
    return _link([_obj(s) for s in srcs], LDFLAGS, out, verbose)


def build_torchglue(force=False, verbose=False):
    """Compile csrc/torch_glue_ext.cpp against the installed torch (pybind11 module, no device code) -> lib/_stego_torchglue.so."""
    deps = [TORCHGLUE_SRC, os.path.join(CSRC, "..", "..", "include", "stego_corr.h")]
    import sysconfig
    import torch
    stamp = TORCHGLUE_PATH + ".torch"          # the torch build the extension was compiled against: another one makes it stale
    built_for = open(stamp).read().strip() if os.path.exists(stamp) else ""
    if not force and os.path.exists(TORCHGLUE_PATH) and built_for == torch.__version__ and \
            all(os.path.getmtime(TORCHGLUE_PATH) >= os.path.getmtime(d) for d in deps):
        return TORCHGLUE_PATH
    from torch.utils import cpp_extension
    os.makedirs(LIB_DIR, exist_ok=True)
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [shutil.which("g++") or "g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           "-DTORCH_EXTENSION_NAME=_stego_torchglue", "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI)]
    cmd += ["-I" + d for d in cpp_extension.include_paths() + [os.path.join(rocm, "include"), sysconfig.get_paths()["include"]]]
    cmd += [TORCHGLUE_SRC, "-L" + tlib, "-Wl,-rpath," + tlib, "-lc10", "-lc10_hip", "-ltorch_cpu", "-ltorch_hip", "-ltorch", "-ltorch_python", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-ldl",
            "-o", TORCHGLUE_PATH + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("g++ failed on %s:\n%s%s" % (TORCHGLUE_SRC, res.stdout, res.stderr))
    os.replace(TORCHGLUE_PATH + ".tmp", TORCHGLUE_PATH)
    with open(stamp, "w") as f:
        f.write(torch.__version__)
    return TORCHGLUE_PATH


# ---- sanitizer build of the HOST side ("race / memory checkers"): the same sources, host code instrumented with
# AddressSanitizer + UndefinedBehaviorSanitizer (the device code is what the product ships: clang ignores -fsanitize for gfx950 without
# xnack+).  tests/test_asan_host.py runs the C-ABI's host logic - descriptor validation, geometry, error paths, the symbol table - through it.
ASAN_DIR = os.path.join(LIB_DIR, "asan")
ASAN_LIB_PATH = os.path.join(ASAN_DIR, "libstego_corr.so")
ASAN_FLAGS = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-shared-libsan", "-g", "-Wno-option-ignored"]


def asan_runtime():
    """The clang AddressSanitizer runtime to LD_PRELOAD into an uninstrumented python (None if this toolchain has none)."""
    hits = sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "lib", "llvm", "lib", "clang", "*", "lib", "linux",
                                         "libclang_rt.asan-x86_64.so")))
    return hits[-1] if hits else None


def build_asan(force=False, verbose=False):
    """lib/asan/libstego_corr.so: every source with ASAN_FLAGS (objects cached under lib/obj/asan)."""
    odir = os.path.join(OBJ_DIR, "asan")
    os.makedirs(ASAN_DIR, exist_ok=True)
    srcs = sources()
    if _compile_objects(srcs, odir, CFLAGS + ASAN_FLAGS, force, verbose) or not os.path.exists(ASAN_LIB_PATH):
        _link([_obj(s, odir) for s in srcs], LDFLAGS + ASAN_FLAGS, ASAN_LIB_PATH, verbose)
    return ASAN_LIB_PATH


def build_skeleton(force=False, verbose=False):
    """tools/ubench/fused_skeleton.hip -> stego_amd/lib/fused_skeleton.bin (git-ignored; travels with the snapshot like the library)."""
    src = os.path.abspath(SKELETON_SRC)
    if not os.path.exists(src):
        return None
    if not force and os.path.exists(SKELETON_PATH) and os.path.getmtime(SKELETON_PATH) >= os.path.getmtime(src):
        return SKELETON_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [_hipcc()] + CFLAGS[:3] + [src, "-o", SKELETON_PATH + ".tmp"]      # architecture, optimisation, standard: the library's
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    os.replace(SKELETON_PATH + ".tmp", SKELETON_PATH)
    return SKELETON_PATH


# ---- what the compiler reports per kernel (registers, spills, scratch, occupancy, LDS): the build-time guards of tests/ read it from here,
# so they see the compilation that ships (CFLAGS)
def parse_resource_remarks(text):
    """{mangled function name: {remark name: int}} from the stderr of a -Rpass-analysis=kernel-resource-usage compile."""
    kernels, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([^:]+): (\d+)\b", line)
        if m and name:
            kernels[name][m.group(1)] = int(m.group(2))
    return kernels


@functools.lru_cache(maxsize=None)
def kernel_resources(source_name):
    """The resource figures of every kernel of csrc/<source_name>, compiled with CFLAGS into a temporary directory (once per process).
    --cuda-device-only leaves out the host pass, which reports nothing: the table of all 35 sources is the same with and without it."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [_hipcc()] + CFLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, source_name),
                                     "-o", os.path.join(tmp, "unit.o")]
        return parse_resource_remarks(_run(cmd, "hipcc on " + source_name, False))


def kernel_resources_each(source_names):
    """[kernel_resources(s) for s in source_names], the units compiled side by side."""
    with ThreadPoolExecutor(max_workers=min(8, len(source_names))) as ex:
        return list(ex.map(kernel_resources, source_names))


if __name__ == "__main__":
    print(build(force=True, verbose=True))
    print(build_torchglue(force=True, verbose=True))
