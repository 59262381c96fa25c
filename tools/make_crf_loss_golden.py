"""Writes tests/golden/crf_loss_small.npz: seeded float64 inputs, the points the reference's ContrastiveCRFLoss (src/modules.py:437-469)
drew for them and the mean of its [B, N, N] output, overall and per image.

Build container only: the UNMODIFIED reference module is imported through oracle/ref_shim.py.  The module draws its points inside
forward, from torch's global generator: the tool seeds it, repeats the module's two randint calls to record the points, seeds it again
and calls the module, which therefore draws the same points.  tests/test_crf_loss_host.py pins featurizers.ContrastiveCRFLoss (draw,
forward) and crf_loss.torch_crf_mean_loss against the file.

    python tools/make_crf_loss_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

B, K, G, H, W, N = 2, 5, 3, 8, 8, 50
PARAMS = (0.5, 0.15, 0.05, 10.0, 3.0, 0.1)          # alpha, beta, gamma, w1, w2, shift
SEED, DRAW_SEED = 11, 12


def main():
    R = ref_shim.load_reference_modules()
    g = torch.Generator().manual_seed(SEED)
    guidance = torch.randn(B, G, H, W, generator=g, dtype=torch.float64)
    code = torch.randn(B, K, H, W, generator=g, dtype=torch.float64)
    module = R.ContrastiveCRFLoss(N, *PARAMS)
    torch.manual_seed(DRAW_SEED)
    coords = torch.cat([torch.randint(0, H, size=[1, N]), torch.randint(0, W, size=[1, N])], 0)
    torch.manual_seed(DRAW_SEED)
    with torch.no_grad():
        out = module(guidance, code)
    assert out.dtype == torch.float64 and tuple(out.shape) == (B, N, N)
    path = os.path.join(ROOT, "tests", "golden", "crf_loss_small.npz")
    np.savez_compressed(path, guidance=guidance.numpy(), code=code.numpy(), coords=coords.numpy(), params=np.array(PARAMS),
                        draw_seed=np.array(DRAW_SEED), mean=out.mean().numpy(), per_image=out.mean(dim=(1, 2)).numpy())
    print("%s %d bytes: mean %.17g" % (path, os.path.getsize(path), float(out.mean())))


if __name__ == "__main__":
    main()
