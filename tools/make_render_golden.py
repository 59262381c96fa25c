"""Writes tests/golden/render_small.npz: what the reference's own plotting helpers return, for tests/test_render_host.py.

Build container only.  The reference's ``src/data.py`` and ``src/utils.py`` import torchvision, wget, torchmetrics and more at module
level, so they cannot be imported here and oracle/ref_shim.py (which loads ``src/modules.py``) does not reach them.  The definitions
this fixture needs are therefore cut out of the UNMODIFIED files with ``ast`` at generation time and executed in a namespace that
holds only numpy and torch: the two colormaps, ``UnNormalize`` / ``unnorm`` / ``prep_for_plot``, and ``UnsupervisedMetrics.map_clusters``
(bound to a plain object that carries ``n_classes``, ``extra_clusters`` and the ``assignments`` scipy returns for a seeded matrix).
Only the recorded arrays are written; no text of the reference is.

    python tools/make_render_golden.py
"""
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

SEED = 0
IMAGE_SHAPES = ((3, 7, 9), (3, 5, 16))
N_CLASSES = 5


def extract(path, names):
    """The top-level definitions `names` of the file (functions, classes, assignments to one name), compiled, in file order."""
    with open(path) as f:
        tree = ast.parse(f.read())
    keep = []
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
            keep.append(node)
        elif isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id in names:
            keep.append(node)
    found = {n.name if hasattr(n, "name") else n.targets[0].id for n in keep}
    assert found == set(names), sorted(set(names) - found)
    return compile(ast.Module(body=keep, type_ignores=[]), path, "exec")


def method(path, cls, name):
    """One method of a top-level class of the file, as a plain function."""
    with open(path) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.ClassDef) and node.name == cls:
            for sub in node.body:
                if isinstance(sub, ast.FunctionDef) and sub.name == name:
                    ns = {"np": np, "torch": torch}
                    exec(compile(ast.Module(body=[sub], type_ignores=[]), path, "exec"), ns)
                    return ns[name]
    raise KeyError("%s.%s" % (cls, name))


def images():
    rng = np.random.default_rng(SEED)
    return [(rng.standard_normal(s) * 1.2 + 0.1).astype(np.float32) for s in IMAGE_SHAPES]


def cluster_case(extra):
    """A seeded confusion matrix [n + extra, n], its Hungarian assignment, and cluster ids that use every row."""
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(SEED + 1 + extra)
    stats = rng.integers(0, 1000, (N_CLASSES + extra, N_CLASSES)).astype(np.int64)
    rows, cols = linear_sum_assignment(stats, maximize=True)
    clusters = rng.permutation(np.repeat(np.arange(N_CLASSES + extra), 3)).reshape(3, -1).astype(np.int64)
    return stats, rows, cols, clusters


def main():
    if not ref_shim.available():
        raise RuntimeError("the reference is not present: this tool runs in the build container only")
    src = ref_shim.REFERENCE_SRC
    out = {}

    ns = {"np": np}
    exec(extract(os.path.join(src, "data.py"), ["bit_get", "create_pascal_label_colormap", "create_cityscapes_colormap"]), ns)
    out["pascal"] = np.asarray(ns["create_pascal_label_colormap"]()).astype(np.int64)
    out["cityscapes"] = np.asarray(ns["create_cityscapes_colormap"]()).astype(np.int64)

    import torch.nn.functional as F
    ns = {"np": np, "torch": torch, "F": F}
    exec(extract(os.path.join(src, "utils.py"), ["UnNormalize", "unnorm", "prep_for_plot"]), ns)
    for i, img in enumerate(images()):
        out["img%d" % i] = img
        out["plot%d" % i] = ns["prep_for_plot"](torch.from_numpy(img)).numpy()
        out["plot%d_norescale" % i] = ns["prep_for_plot"](torch.from_numpy(img), rescale=False).numpy()
        assert out["plot%d" % i].dtype == np.float32 and out["plot%d" % i].shape == (img.shape[1], img.shape[2], 3)

    map_clusters = method(os.path.join(src, "utils.py"), "UnsupervisedMetrics", "map_clusters")
    for extra in (0, 2):
        stats, rows, cols, clusters = cluster_case(extra)
        holder = types.SimpleNamespace(n_classes=N_CLASSES, extra_clusters=extra, assignments=(rows, cols))
        mapped = map_clusters(holder, torch.from_numpy(clusters)).numpy()
        vector = map_clusters(holder, torch.arange(N_CLASSES + extra)).numpy()
        out["stats_extra%d" % extra] = stats
        out["clusters_extra%d" % extra] = clusters
        out["mapped_extra%d" % extra] = mapped.astype(np.int64)
        out["vector_extra%d" % extra] = vector.astype(np.int64)

    path = os.path.join(ROOT, "tests", "golden", "render_small.npz")
    np.savez_compressed(path, **out)
    print("%s %d bytes: %s" % (path, os.path.getsize(path), ", ".join(sorted(out))))


if __name__ == "__main__":
    main()
