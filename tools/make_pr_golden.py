"""Writes tests/golden/corr_pr_small.npz: seeded inputs and what the UNMODIFIED reference computes from them for the
label co-occurrence PR curves (src/plot_pr_curves.py:108-121, get_net_fd): the fp32 feature correlation ``fd`` and label
correlation ``ld`` of every pair of sample points.

Build container only: the reference's ``sample`` / ``norm`` / ``tensor_correlation`` are imported through oracle/ref_shim.py and
composed the way get_net_fd composes them (plot_pr_curves.py itself imports pytorch_lightning, seaborn and hydra at module level
and cannot be imported here).  tests/test_corr_pr_host.py pins tests/corr_pr_oracle.py against the file.

    python tools/make_pr_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim  # noqa: E402

B, C, HF, HL, S, N_CLASSES, BLOCK = 2, 24, 12, 48, 5, 6, 8
BAND = 2e-3          # no impure pair may have a label correlation this close to 1 (tests/test_corr_pr_host.py asserts it)


def inputs(seed):
    rng = np.random.default_rng(seed)
    feats1 = rng.standard_normal((B, C, HF, HF)).astype(np.float32)
    feats2 = rng.standard_normal((B, C, HF, HF)).astype(np.float32)
    feats1[0, :, 4:8, 4:8] = 0.0                                        # a zero region: the eps branch of norm()
    blocks = rng.integers(-1, N_CLASSES, (2, B, HL // BLOCK, HL // BLOCK))     # -1: unlabeled regions
    label1, label2 = [np.repeat(np.repeat(b, BLOCK, 1), BLOCK, 2).astype(np.int64) for b in blocks]
    coords1 = (rng.random((B, S, S, 2)) * 2 - 1).astype(np.float32)
    coords2 = (rng.random((B, S, S, 2)) * 2 - 1).astype(np.float32)
    coords1[0, 0, 0] = (0.0, 0.0)                                        # inside the zero region (pixel 5.5, 5.5)
    coords1[1, 0, 1] = (1.3, -0.2)                                       # beyond the border: clamped
    coords2[0, 1, 0] = (-1.0, 1.0)                                       # a corner
    coords2[1, 2, 2] = (-1.7, 2.5)
    return feats1, feats2, label1, label2, coords1, coords2


def reference(feats1, feats2, label1, label2, coords1, coords2):
    R = ref_shim.load_reference_modules()
    t = [torch.from_numpy(x) for x in (feats1, feats2, label1, label2, coords1, coords2)]
    with torch.no_grad():
        s1, s2 = R.sample(t[0], t[4]), R.sample(t[1], t[5])
        l1 = R.sample(F.one_hot(t[2] + 1, N_CLASSES + 1).to(torch.float).permute(0, 3, 1, 2), t[4])
        l2 = R.sample(F.one_hot(t[3] + 1, N_CLASSES + 1).to(torch.float).permute(0, 3, 1, 2), t[5])
        fd = R.tensor_correlation(R.norm(s1), R.norm(s2))
        ld = R.tensor_correlation(l1, l2)
    return fd.numpy(), ld.numpy()


def main():
    import corr_pr_oracle as P
    for seed in range(100):
        d = inputs(seed)
        o = P.net_fd(d[0], d[1], d[2], d[3], d[4], d[5], N_CLASSES)
        if not ((o["ld"] > 1 - BAND) & ~o["target"]).any() and o["target"].sum() >= 50:
            break
    else:
        raise SystemExit("no seed keeps every impure pair out of the band")
    fd, ld = reference(*d)
    assert fd.dtype == np.float32 and ld.dtype == np.float32
    out = os.path.join(ROOT, "tests", "golden", "corr_pr_small.npz")
    np.savez_compressed(out, feats1=d[0], feats2=d[1], label1=d[2].astype(np.int16), label2=d[3].astype(np.int16), coords1=d[4], coords2=d[5],
                        fd=fd, ld=ld, meta=np.array([N_CLASSES, seed], dtype=np.int64))
    print("seed %d: %d pairs, %d positive, %d truncated to 0 by ld.to(int64); %s %d bytes"
          % (seed, ld.size, int(o["target"].sum()), int((o["target"] & (ld < 1)).sum()), out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
