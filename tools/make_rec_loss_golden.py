"""Writes tests/golden/rec_loss_small.npz: seeded float64 code, feats and decoder parameters, and the reconstruction loss the
reference's own lines (src/train_segmentation.py:183-187) give for them.

Build container only: `norm` is the UNMODIFIED reference function, imported through oracle/ref_shim.py; the decoder is the
nn.Conv2d(dim, n_feats, 1) the reference's LitUnsupervisedSegmenter builds.  tests/test_rec_loss_host.py pins tests/rec_oracle.py and
rec_loss.torch_rec_loss against the file.

    python tools/make_rec_loss_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

B, K, C, H, W = 2, 5, 12, 4, 3
SEED = 21


def main():
    R = ref_shim.load_reference_modules()
    g = torch.Generator().manual_seed(SEED)
    code = torch.randn(B, K, H, W, generator=g, dtype=torch.float64)
    feats = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    weight = torch.randn(C, K, generator=g, dtype=torch.float64) / K ** 0.5
    bias = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    decoder = torch.nn.Conv2d(K, C, (1, 1)).double()
    with torch.no_grad():
        decoder.weight.copy_(weight.reshape(C, K, 1, 1))
        decoder.bias.copy_(bias)
        loss = -(R.norm(decoder(code)) * R.norm(feats)).sum(1).mean()
    assert loss.dtype == torch.float64 and loss.dim() == 0
    path = os.path.join(ROOT, "tests", "golden", "rec_loss_small.npz")
    np.savez_compressed(path, code=code.numpy(), feats=feats.numpy(), weight=weight.numpy(), bias=bias.numpy(), loss=loss.numpy())
    print("%s %d bytes: loss %.17g" % (path, os.path.getsize(path), float(loss)))


if __name__ == "__main__":
    main()
