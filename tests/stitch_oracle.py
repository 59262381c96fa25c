"""Float64 restatement of stego_stitch_probe (include/stego_stitch.h) with torch on the CPU: per window the reference's torch chain
(flip average, F.interpolate bilinear with align_corners=False, the linear probe, the cluster probe's cosine), then the tent blend of
the windows' logits on the canvas and the log-softmax."""
import torch
import torch.nn.functional as F

from stego_amd.segment import window_origins


def window_logits(code, code_flip, lin_w, lin_b, cent, win, alpha=2.0):
    """Both probes' logits of every window at (win, win), float64: ([T, n_lin, win, win], [T, n_clu, win, win]).  `cent` is used as
    given (the kernel takes L2-normalised centroids)."""
    c = code.detach().double().cpu()
    if code_flip is not None:
        c = (c + code_flip.detach().double().cpu().flip(dims=[3])) / 2
    c = F.interpolate(c, (win, win), mode="bilinear", align_corners=False)
    lin = torch.einsum("tkhw,nk->tnhw", c, lin_w.detach().double().cpu()) + lin_b.detach().double().cpu()[None, :, None, None]
    clu = alpha * torch.einsum("tkhw,nk->tnhw", F.normalize(c, dim=1), cent.detach().double().cpu())
    return lin, clu


def tent_weights(win):
    u = torch.arange(win, dtype=torch.float64)
    t = torch.minimum(u + 1, win - u)
    return t[:, None] * t[None, :]


def blend(logits, H, W, win, stride):
    """[T, n, win, win] window logits -> [n, H, W]: sum of a^_t logits_t over the covering windows, a^ = a / sum of a."""
    oys, oxs = window_origins(H, win, stride), window_origins(W, win, stride)
    assert logits.shape[0] == len(oys) * len(oxs)
    a = tent_weights(win)
    total = torch.zeros(H, W, dtype=torch.float64)
    for oy in oys:
        for ox in oxs:
            total[oy:oy + win, ox:ox + win] += a
    out = torch.zeros(logits.shape[1], H, W, dtype=torch.float64)
    for iy, oy in enumerate(oys):
        for ix, ox in enumerate(oxs):
            out[:, oy:oy + win, ox:ox + win] += (a / total[oy:oy + win, ox:ox + win]) * logits[iy * len(oxs) + ix]
    return out


def cover(H, W, win, stride):
    """How many windows cover each canvas pixel, int64 [H, W]."""
    n = torch.zeros(H, W, dtype=torch.int64)
    for oy in window_origins(H, win, stride):
        for ox in window_origins(W, win, stride):
            n[oy:oy + win, ox:ox + win] += 1
    return n


def stitch_log_probs(code, code_flip, lin_w, lin_b, cent, size, win, stride, alpha=2.0):
    """-> (linear, cluster) log-probabilities on the canvas, float64 [n, H, W]."""
    H, W = size
    lin, clu = window_logits(code, code_flip, lin_w, lin_b, cent, win, alpha)
    return torch.log_softmax(blend(lin, H, W, win, stride), 0), torch.log_softmax(blend(clu, H, W, win, stride), 0)


def top2_gap(log_probs):
    """The gap between the largest and the second largest value per pixel, [H, W]."""
    v = log_probs.topk(2, dim=0).values
    return v[0] - v[1]
