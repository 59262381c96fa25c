"""The definition of stego_attn_salience (include/stego_vit.h) in numpy float64, and the synthetic inputs both test files share.

Per image, from the float32 attention [B, heads, 1 + h*w]:
    m_i     = sum over the heads, in head order, of attn[b, head, 1 + i]
    T       = sum_i m_i in index order
    ahead_i = sum of m_j over the patches before i in the order (m descending, index ascending on ties): np.lexsort((index, -m)) and an
              exclusive np.cumsum in that order
    kept_i  = ahead_i < (double)(float)keep * T
    soft    = m / T,  mask = kept replicated over patch x patch pixels
margin = min_i |ahead_i - keep * T| / T per image: how far the nearest decision is from flipping.  An implementation that adds in another
order moves ahead_i and T by float64 rounding (1e-16 relative); where the margin is above 1e-9 its kept must EQUAL this one's.  Where
every m is a small multiple of a power of two (`exact_sums`), all sums are exact in every order and equality holds at any margin.
"""
import numpy as np


def salience(attn, h, w, patch, keep):
    """-> soft float64 [B, h, w], kept bool [B, h, w], mask uint8 [B, h*patch, w*patch], margin float64 [B]."""
    attn = np.asarray(attn)
    assert attn.dtype == np.float32 and attn.ndim == 3 and attn.shape[2] == 1 + h * w
    B, heads, _ = attn.shape
    n = h * w
    keep64 = float(np.float32(keep))
    soft = np.empty((B, n))
    kept = np.empty((B, n), dtype=bool)
    margin = np.empty(B)
    for b in range(B):
        m = np.zeros(n)
        for hd in range(heads):
            m = m + attn[b, hd, 1:].astype(np.float64)
        T = np.cumsum(m)[-1]                                  # sequential: index order
        order = np.lexsort((np.arange(n), -m))
        sorted_m = m[order]
        ahead = np.empty(n)
        ahead[order] = np.cumsum(sorted_m) - sorted_m         # exclusive, in the order
        kept[b] = ahead < keep64 * T
        soft[b] = m / T
        margin[b] = np.abs(ahead - keep64 * T).min() / T
    kept = kept.reshape(B, h, w)
    mask = np.repeat(np.repeat(kept.astype(np.uint8), patch, axis=1), patch, axis=2)
    return soft.reshape(B, h, w), kept, mask, margin


def exact_sums(attn):
    """True when every patch weight is a multiple of 2^-8 below 2^8: any sum of up to 2^36 of them is exact in float64 in any order."""
    a = np.asarray(attn, dtype=np.float64)[:, :, 1:] * 256.0
    return bool((a == np.round(a)).all() and (np.abs(a) < 65536).all())


def _softmax_like(rng, B, heads, n):
    x = rng.standard_normal((B, heads, 1 + n)) * 2.0
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _quantised(rng, B, heads, n, zeros=False):
    """Multiples of 1 / 256 from a handful of levels: many exact ties, within a head and between the sums of heads."""
    a = rng.integers(0 if zeros else 1, 6, size=(B, heads, 1 + n)).astype(np.float32) / 256.0
    if zeros:
        a[:, :, 1 + n // 3] = 0.0
        a[0, :, 1:1 + max(1, n // 2)] = 0.0
    return a


def cases():
    """name -> (attn, h, w, patch, keep): the synthetic inputs of the issue's list."""
    rng = np.random.default_rng(20240611)
    out = {}
    out["uniform 8x8 keep 0.6"] = (np.full((2, 1, 65), np.float32(1.0 / 65), dtype=np.float32), 8, 8, 8, 0.6)
    out["quantised ties, 1 head"] = (_quantised(rng, 3, 1, 7 * 9), 7, 9, 8, 0.6)
    out["quantised ties, 12 heads"] = (_quantised(rng, 2, 12, 6 * 5), 6, 5, 16, 0.45)
    out["one patch"] = (_softmax_like(rng, 3, 2, 1), 1, 1, 8, 0.6)
    out["4096 patches"] = (_softmax_like(rng, 2, 6, 4096), 64, 64, 8, 0.6)
    out["h != w, odd w, patch 8"] = (_softmax_like(rng, 3, 6, 5 * 13), 5, 13, 8, 0.6)
    out["h != w, patch 16"] = (_softmax_like(rng, 2, 3, 9 * 4), 9, 4, 16, 0.7)
    out["keep 1.0"] = (_quantised(rng, 2, 3, 6 * 6, zeros=True), 6, 6, 8, 1.0)
    out["keep 1.0, softmax"] = (_softmax_like(rng, 2, 6, 28 * 28), 28, 28, 8, 1.0)
    out["keep 1e-6"] = (_softmax_like(rng, 4, 6, 28 * 28), 28, 28, 8, 1e-6)
    out["exact zeros"] = (_quantised(rng, 3, 2, 10 * 3, zeros=True), 10, 3, 16, 0.6)
    return out
