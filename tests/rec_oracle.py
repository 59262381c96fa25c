"""The reconstruction loss of include/stego_rec.h restated in numpy float64, formula by formula: the loss and the three gradients for a
unit upstream.  tests/test_rec_loss_host.py holds it against torch's float64 autograd of stego_amd.rec_loss.torch_rec_loss."""
import numpy as np

EPS = 1e-10


def rec_loss(code, feats, weight, bias):
    """code [B, K, h, w], feats [B, C, h, w], weight [C, K], bias [C] -> (loss, d_code [B, K, h, w], d_weight [C, K], d_bias [C])."""
    code, feats = np.asarray(code, dtype=np.float64), np.asarray(feats, dtype=np.float64)
    weight, bias = np.asarray(weight, dtype=np.float64).reshape(feats.shape[1], code.shape[1]), np.asarray(bias, dtype=np.float64)
    B, K, h, w = code.shape
    C = feats.shape[1]
    x = code.transpose(0, 2, 3, 1).reshape(-1, K)                       # tokens over (b, y, x)
    f = feats.transpose(0, 2, 3, 1).reshape(-1, C)
    T = x.shape[0]
    r = x @ weight.T + bias
    nr_raw = np.sqrt((r * r).sum(1))
    nr, nf = np.maximum(nr_raw, EPS), np.maximum(np.sqrt((f * f).sum(1)), EPS)
    c = (r * f).sum(1) / (nr * nf)
    loss = -c.sum() / T
    proj = (nr_raw >= EPS).astype(np.float64) * c                       # torch's clamp_min rule: the projection vanishes below eps
    g = -(f / nf[:, None] - proj[:, None] * r / nr[:, None]) / nr[:, None] / T
    d_code = (g @ weight).reshape(B, h, w, K).transpose(0, 3, 1, 2)
    return loss, d_code, g.T @ x, g.sum(0)
