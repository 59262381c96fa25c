"""Writes tests/golden/corr_heatmaps_small.npz: seeded inputs and what the reference's get_heatmaps chain
(src/plot_dino_correspondence.py:45-56) computes from them in fp32, for the self and the KNN target and three output sizes.

Build container only: the UNMODIFIED reference's ``sample`` is imported through oracle/ref_shim.py and composed with torch's own
``F.normalize`` and ``F.interpolate`` the way get_heatmaps composes them (plot_dino_correspondence.py itself imports hydra,
pytorch_lightning and matplotlib.animation at module level and needs a device, so it cannot be imported here).
tests/test_heatmaps_host.py pins tests/corr_heatmap_oracle.py against the file.

    python tools/make_heatmap_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

C, H_MAP, W_MAP = 24, 6, 5
SIZES = ((17, 13), (6, 5), (1, 7))
SEED = 0


def inputs():
    rng = np.random.default_rng(SEED)
    feats1 = rng.standard_normal((1, C, H_MAP, W_MAP)).astype(np.float32)
    feats2 = (feats1 + 0.7 * rng.standard_normal((1, C, H_MAP, W_MAP))).astype(np.float32)
    feats1[0, :, 3:5, 0:2] = 0.0                                         # a zero region: the eps branch of F.normalize
    feats2[0, :, 0, 4] = 0.0
    points = np.array([[0.31, -0.44],                                    # a generic point
                       [-0.75, 0.4],                                     # inside the zero region (pixel x = 0.5, y = 3.5)
                       [1.3, -0.2],                                      # beyond the border: clamped
                       [-1.0, 1.0]], dtype=np.float32).reshape(1, 4, 1, 2)       # a corner
    return feats1, feats2, points


def reference(feats1, feats2, points):
    R = ref_shim.load_reference_modules()
    f1, f2, q = (torch.from_numpy(x) for x in (feats1, feats2, points))
    out = {}
    with torch.no_grad():
        s = R.sample(f1, q)
        for name, ft in (("intra", f1), ("inter", f2)):
            attn = torch.einsum("nchw,ncij->nhwij", F.normalize(s, dim=1), F.normalize(ft, dim=1))
            attn -= attn.mean([3, 4], keepdims=True)
            attn = attn.clamp(0).squeeze(0)
            for size in SIZES:
                out["%s_%dx%d" % (name, size[0], size[1])] = F.interpolate(attn, size, mode="bilinear", align_corners=True).squeeze(0).numpy()
    return out


def main():
    feats1, feats2, points = inputs()
    res = reference(feats1, feats2, points)
    assert all(v.dtype == np.float32 for v in res.values())
    assert not res["intra_6x5"][1].any() and res["intra_6x5"][0].any()     # the query inside the zero region: a heatmap of zeros
    out = os.path.join(ROOT, "tests", "golden", "corr_heatmaps_small.npz")
    np.savez_compressed(out, feats1=feats1, feats2=feats2, points=points, sizes=np.array(SIZES, dtype=np.int64), **res)
    print("%s %d bytes: %s" % (out, os.path.getsize(out), ", ".join(sorted(res))))


if __name__ == "__main__":
    main()
