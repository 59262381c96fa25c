"""Writes tests/golden/aug_align_small.npz: for two of the small loss cases of tests/test_augment_gpu.py (GOLDEN_CASES) the float32
inputs, and in float64 the aug-alignment term (train_segmentation.py:189-198 of the reference), its gradients to code and code_aug
and the mean |cosine| term the loss scalar is judged by.

Build container only: `sample` and `norm` are the UNMODIFIED reference's (src/modules.py:275-288, imported through
oracle/ref_shim.py); its `resize` (src/utils.py:61-62, a module this image cannot import) is the one F.interpolate call written out
here.  tests/test_augment_host.py regenerates the file's numbers with the reference present; tests/test_augment_gpu.py holds the
kernel to them.

    python tools/make_aug_golden.py
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


def reference_term(R, code, code_aug, coord):
    """(loss, per-pixel cosine terms [B, S, S]) with the reference's own sample and norm."""
    ds = F.interpolate(coord.permute(0, 3, 1, 2), (code_aug.shape[2], code_aug.shape[2]), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    terms = torch.einsum("bkhw,bkhw->bhw", R.norm(R.sample(code, ds)), R.norm(code_aug))
    return -terms.mean(), terms


def golden_arrays(R):
    from test_augment_gpu import GOLDEN_CASES, loss_inputs
    out = {}
    for case in GOLDEN_CASES:
        code, code_aug, coord = loss_inputs(case)
        x, y = code.double().requires_grad_(True), code_aug.double().requires_grad_(True)
        loss, terms = reference_term(R, x, y, coord.double())
        loss.backward()
        p = "c%d_" % case
        out.update({p + "code": code.numpy(), p + "code_aug": code_aug.numpy(), p + "coord": coord.numpy(),
                    p + "loss": loss.detach().numpy(), p + "d_code": x.grad.numpy(), p + "d_code_aug": y.grad.numpy(),
                    p + "scale": terms.detach().abs().mean().numpy()})
    return out


def main():
    arrays = golden_arrays(ref_shim.load_reference_modules())
    path = os.path.join(ROOT, "tests", "golden", "aug_align_small.npz")
    np.savez_compressed(path, **arrays)
    print("%s %d bytes: %s" % (path, os.path.getsize(path), ", ".join("%s %.17g" % (k, float(v)) for k, v in arrays.items() if k.endswith("loss"))))


if __name__ == "__main__":
    main()
