"""torch restatement of the semantics of include/stego_aug.h (torchvision's tensor operators: hflip, resized_crop, ColorJitter's four
adjust_* functions, rgb_to_grayscale, gaussian_blur), with the dtype as a parameter: float64 is the reference of the GPU tests, float32
shows what the precision of the format costs.  Records are StegoAugParams (stego_amd.augment.make_params)."""
import torch
import torch.nn.functional as F


def axis(n_out, crop, dtype):
    """(i0, i1, lambda of i1) of the bilinear resize crop -> n_out, align_corners=False: the rule of the header."""
    d = torch.arange(n_out, dtype=dtype)
    src = (torch.tensor(float(crop), dtype=dtype) / n_out * (d + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(crop - 1)
    i1 = i0 + (i0 < crop - 1).long()
    return i0, i1, src - i0.to(dtype)


def geometry(img, rec, R):
    """img [C, H, W] -> [C, R, R]: the resized crop of the (flipped) image."""
    W = img.shape[2]
    y0, y1, ly = axis(R, rec.ch, img.dtype)
    x0, x1, lx = axis(R, rec.cw, img.dtype)
    r0, r1, c0, c1 = rec.top + y0, rec.top + y1, rec.left + x0, rec.left + x1
    if rec.flip:
        c0, c1 = W - 1 - c0, W - 1 - c1
    ly, lx = ly[None, :, None], lx[None, None, :]
    p = lambda r, c: img[:, r][:, :, c]
    return (1 - ly) * ((1 - lx) * p(r0, c0) + lx * p(r0, c1)) + ly * ((1 - lx) * p(r1, c0) + lx * p(r1, c1))


def gray(x):
    return (0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]).unsqueeze(0)


def blend(a, b, f):
    return (f * a + (1 - f) * b).clamp(0, 1)


def hue(x, f):
    r, g, b = x[0], x[1], x[2]
    maxc, minc = x.max(0).values, x.min(0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = (h + f) % 1.0
    v = maxc
    i = torch.floor(h * 6.0)
    ff = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * ff)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - ff))).clamp(0, 1)
    pick = lambda options: torch.stack(options).gather(0, i.unsqueeze(0)).squeeze(0)
    return torch.stack([pick([v, q, p, p, t, v]), pick([t, v, v, q, p, p]), pick([p, p, t, v, v, q])])


def blur_weights(sigma, dtype):
    x = torch.arange(-2, 3, dtype=dtype)
    pdf = torch.exp(-0.5 * (x / sigma) ** 2)
    return pdf / pdf.sum()


def blur(x, sigma):
    k = blur_weights(sigma, x.dtype)
    R = x.shape[-1]
    p = F.pad(x.unsqueeze(0), (2, 2, 2, 2), mode="reflect").squeeze(0)
    rows = sum(k[i] * p[:, :, i:i + R] for i in range(5))
    return sum(k[i] * rows[:, i:i + R, :] for i in range(5))


def photometric(x, rec):
    for op in rec.order:
        if op == 0:
            x = blend(x, torch.zeros_like(x), rec.factor[0])
        elif op == 1:
            x = blend(x, gray(x).mean(), rec.factor[1])
        elif op == 2:
            x = blend(x, gray(x), rec.factor[2])
        elif op == 3:
            x = hue(x, rec.factor[3])
    if rec.gray:
        x = gray(x).expand(3, -1, -1)
    if rec.blur_sigma > 0:
        x = blur(x, rec.blur_sigma)
    return x


def coord_image(H, W, dtype):
    """The reference's coordinate image (data.py:530-532): channel 0 the row ramp, channel 1 the column ramp."""
    return torch.stack(torch.meshgrid(torch.linspace(-1, 1, H, dtype=dtype), torch.linspace(-1, 1, W, dtype=dtype), indexing="ij"))


def augment(img, records, R, dtype=torch.float64):
    """img [B, 3, H, W], B records -> (img_aug [B, 3, R, R], coord_aug [B, R, R, 2]) computed in `dtype` on the CPU."""
    img = img.detach().cpu().to(dtype)
    coord = coord_image(img.shape[2], img.shape[3], dtype)
    out, cout = [], []
    for b, rec in enumerate(records):
        out.append(photometric(geometry(img[b], rec, R), rec))
        cout.append(geometry(coord, rec, R).permute(1, 2, 0))
    return torch.stack(out), torch.stack(cout)
