"""Dense feature correspondence (tensor_correlation, reference modules.py:283-284) on the HIP
kernel through the C ABI, against the reference's golden vector and a float64 einsum."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "primitives.npz")


def _ref(a, b, normalize):
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    if normalize:                                     # norm(): F.normalize(dim=1, eps=1e-10), modules.py:275-276
        a = a / np.maximum(np.sqrt((a * a).sum(1, keepdims=True)), 1e-10)
        b = b / np.maximum(np.sqrt((b * b).sum(1, keepdims=True)), 1e-10)
    return np.einsum("nchw,ncij->nhwij", a, b)


def test_reference_golden_tensor_correlation():
    from stego_amd import modules as M
    g = np.load(GOLD)
    out = M.tensor_correlation(torch.from_numpy(g["a"]).to(DEV), torch.from_numpy(g["b"]).to(DEV))
    assert tuple(out.shape) == g["corr"].shape
    np.testing.assert_allclose(out.cpu().numpy(), g["corr"], rtol=1e-5, atol=1e-6)
    # with autograd the reference einsum is used, same numbers
    a = torch.from_numpy(g["a"]).to(DEV).requires_grad_(True)
    np.testing.assert_allclose(M.tensor_correlation(a, torch.from_numpy(g["b"]).to(DEV)).detach().cpu().numpy(), g["corr"],
                               rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape", [
    (2, 384, 28, 28, 28, 28, True),      # ViT-S/8 at 224^2: the [B, 784, 784] correspondence, cosine
    (1, 768, 40, 40, 40, 40, True),      # ViT-B/8 at 320^2
    (3, 70, 5, 9, 11, 3, False),         # unequal maps, C straddling the 64-wide chunk, raw dot products
    (2, 5, 1, 1, 2, 200, False),         # 1-pixel map against a wide one
])
@pytest.mark.parametrize("layout", ["cl", "nchw"])
def test_dense_corr_matches_float64_einsum(shape, layout):
    from stego_amd import capi
    B, C, H1, W1, H2, W2, normalize = shape
    rng = np.random.default_rng(B * C + H1)
    a = rng.standard_normal((B, C, H1, W1)).astype(np.float32)
    b = rng.standard_normal((B, C, H2, W2)).astype(np.float32)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    if layout == "cl":
        ta = ta.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        tb = tb.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    out = capi.dense_corr(ta, tb, normalize=normalize).cpu().numpy()
    ref = _ref(a, b, normalize)
    scale = np.abs(ref).mean()
    np.testing.assert_allclose(out, ref, rtol=1e-3, atol=2e-5 * max(scale, 1e-3) + 1e-6)
    if normalize and (H1, W1) == (H2, W2):
        self_sim = capi.dense_corr(ta, ta, normalize=True).cpu().numpy().reshape(B, H1 * W1, H1 * W1)
        np.testing.assert_allclose(np.diagonal(self_sim, axis1=1, axis2=2), 1.0, atol=2e-6)      # unit self-similarity
        np.testing.assert_allclose(self_sim, self_sim.transpose(0, 2, 1), atol=1e-6)              # symmetric


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [
    (3, 192, 14, 14, 14, 14, True),      # three chunks (an odd count), one whole block of B + a tail of 68 pixels
    (2, 136, 9, 13, 7, 11, False),       # the last chunk holds 8 channels; 117 rows (a partial row block), 77 columns: a tail only, N % 4 = 1 (scalar stores)
    (9, 328, 12, 12, 20, 20, True),      # two groups of images; 144 rows (a block + 16), 400 columns (three blocks + 16), five chunks + 8 channels
    (1, 72, 16, 16, 16, 16, True),       # two chunks, exactly two blocks, no tail
    (2, 256, 3, 50, 50, 3, False),       # 150 x 150, N % 4 = 2
])
def test_dense_stream_kernel_shapes(shape):
    """csrc/dense_stream.hip (channels-last maps, 64 < C <= 384, C % 8 == 0) on the shapes its special cases exist for, against fp64."""
    from stego_amd import capi
    B, C, H1, W1, H2, W2, normalize = shape
    rng = np.random.default_rng(B * C + H1 + 7)
    a = (rng.standard_normal((B, C, H1, W1)) * rng.uniform(0.2, 5.0, (B, 1, H1, W1))).astype(np.float32)      # pixel norms vary
    b = (rng.standard_normal((B, C, H2, W2)) * rng.uniform(0.2, 5.0, (B, 1, H2, W2))).astype(np.float32)
    ta = torch.from_numpy(a).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    tb = torch.from_numpy(b).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    out = capi.dense_corr(ta, tb, normalize=normalize).cpu().numpy()
    ref = _ref(a, b, normalize)
    scale = np.abs(ref).mean()
    np.testing.assert_allclose(out, ref, rtol=1e-3, atol=2e-5 * max(scale, 1e-3) + 1e-6)
    err = np.abs(out - ref).max() / max(np.abs(ref).max(), 1e-30)
    assert err < 2e-6, err                                                                      # fp32 class, not just the north-star bar


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1e-7, 1.0, 1e6])
def test_dense_stream_raw_products_any_magnitude(scale):
    """The streaming kernel's fp16 staging (a power of two per pixel from dense_stats_kernel) on tiny and huge raw maps."""
    from stego_amd import capi
    rng = np.random.default_rng(5)
    a = (rng.standard_normal((2, 96, 6, 7)) * scale).astype(np.float32)
    b = (rng.standard_normal((2, 96, 5, 4)) * scale).astype(np.float32)
    ta = torch.from_numpy(a).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    tb = torch.from_numpy(b).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    out = capi.dense_corr(ta, tb).cpu().numpy()
    ref = _ref(a, b, False)
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).mean())


@pytest.mark.parametrize("scale", [1e-7, 1.0, 1e6])
def test_dense_corr_raw_products_any_magnitude(scale):
    """Without norm() the products are raw: the fp16 staging must not lose tiny maps or overflow on huge ones."""
    from stego_amd import capi
    rng = np.random.default_rng(3)
    a = (rng.standard_normal((2, 96, 6, 7)) * scale).astype(np.float32)
    b = (rng.standard_normal((2, 96, 5, 4)) * scale).astype(np.float32)
    out = capi.dense_corr(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy()
    ref = _ref(a, b, False)
    np.testing.assert_allclose(out, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).mean())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 64, 7, 9, 5, 6), (3, 384, 28, 28, 28, 28), (1, 70, 11, 11, 20, 20)])
def test_tensor_correlation_gradients_run_on_the_native_kernel(shape):
    """modules.tensor_correlation with autograd (reference modules.py:283-284: the einsum is differentiable there): both
    adjoints are the dense-correspondence kernel on strided views; compared with autograd through the reference's einsum."""
    import torch
    from stego_amd import modules as M
    N, C, H1, W1, H2, W2 = shape
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randn(N, C, H1, W1, device="cuda", generator=g)
    b = torch.randn(N, H2, W2, C, device="cuda", generator=g).permute(0, 3, 1, 2)       # a channels-last view, as DINO emits
    up = torch.randn(N, H1, W1, H2, W2, device="cuda", generator=g)
    a1, b1 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = M.tensor_correlation(a1, b1)
    assert out.grad_fn is not None and "DenseCorr" in type(out.grad_fn).__name__
    (out * up).sum().backward()
    a2, b2 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = torch.einsum("nchw,ncij->nhwij", a2, b2)
    (ref * up.double()).sum().backward()
    for got, want in ((out, ref), (a1.grad, a2.grad), (b1.grad, b2.grad)):
        err = (got.double() - want).abs().max() / want.abs().max()
        assert float(err) < 2e-6, float(err)


def _cl_map(x):
    """A channels-last HIP copy of the NCHW numpy map, as a [B, C, H, W] view."""
    return torch.from_numpy(x).to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _varied(rng, B, C, H, W):
    return (rng.standard_normal((B, C, H, W)) * rng.uniform(0.2, 5.0, (B, 1, H, W))).astype(np.float32)      # pixel norms vary


def _fp32_class_err(out, ref):
    return float(np.abs(out - ref).max() / max(np.abs(ref).max(), 1e-30))


# dense_rowblock_kernel<false> (A consumed in place, B prepared): launch_dense_corr takes it for channels-last maps with C % 8 == 0 and
# NCH <= 6 that the stream kernel does not take, i.e. C <= 64 (here) or B rows not dense (the cropped view below)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("C", [8, 32, 64])
def test_dense_rowblock_kernel_narrow_channels(C, normalize):
    """C in {8, 32, 64} (one partial / one whole 64-channel chunk); 117 x 77 pixels: a partial row block and a partial column block."""
    from stego_amd import capi
    B, H1, W1, H2, W2 = 2, 9, 13, 7, 11
    rng = np.random.default_rng(C + 11 * normalize)
    a, b = _varied(rng, B, C, H1, W1), _varied(rng, B, C, H2, W2)
    out = capi.dense_corr(_cl_map(a), _cl_map(b), normalize=normalize).cpu().numpy()
    ref = _ref(a, b, normalize)
    np.testing.assert_allclose(out, ref, rtol=1e-3, atol=2e-5 * max(np.abs(ref).mean(), 1e-3) + 1e-6)
    assert _fp32_class_err(out, ref) < 2e-6                            # the fp32-class bar of test_dense_stream_kernel_shapes


# dense_rowblock_kernel<false> through the cropped-view condition: C = 384 (the stream kernel's width) but b.sh != W2 * b.sw
@pytest.mark.parametrize("normalize", [True, False])
def test_dense_rowblock_kernel_cropped_b_view(normalize):
    from stego_amd import capi
    B, C = 2, 384
    rng = np.random.default_rng(21 + normalize)
    a, b = _varied(rng, B, C, 14, 14), _varied(rng, B, C, 16, 17)
    tb = _cl_map(b)[:, :, 1:-1, 2:-1]
    assert tb.stride(2) != tb.shape[3] * tb.stride(3) and tb.stride(1) == 1
    out = capi.dense_corr(_cl_map(a), tb, normalize=normalize).cpu().numpy()
    ref = _ref(a, b[:, :, 1:-1, 2:-1], normalize)
    np.testing.assert_allclose(out, ref, rtol=1e-3, atol=2e-5 * max(np.abs(ref).mean(), 1e-3) + 1e-6)
    assert _fp32_class_err(out, ref) < 2e-6


# one input through all three channels-last kernels: dense_stream (default), dense_rowblock_kernel<false> (STEGO_DEBUG bit 21) and
# dense_prep_kernel + dense_tile_kernel (STEGO_DEBUG 8192)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("C", [136, 384])
def test_dense_corr_every_kernel_on_one_input(C, normalize):
    from stego_amd import capi
    base = int(os.environ.get("STEGO_DEBUG", "0"))
    B, H1, W1, H2, W2 = 3, 9, 13, 12, 12
    rng = np.random.default_rng(C + normalize)
    a, b = _varied(rng, B, C, H1, W1), _varied(rng, B, C, H2, W2)
    ta, tb = _cl_map(a), _cl_map(b)
    ref = _ref(a, b, normalize)
    outs = {}
    try:
        for name, bits in (("stream", 0), ("rowblock", 1 << 21), ("tile", 8192)):
            capi.debug_set("STEGO_DEBUG", (base & ~((1 << 21) | 8192)) | bits)
            outs[name] = capi.dense_corr(ta, tb, normalize=normalize).cpu().numpy()
    finally:
        capi.debug_set("STEGO_DEBUG", base)
    for name, out in outs.items():
        np.testing.assert_allclose(out, ref, rtol=1e-3, atol=2e-5 * max(np.abs(ref).mean(), 1e-3) + 1e-6, err_msg=name)
        assert _fp32_class_err(out, ref) < 2e-6, (name, _fp32_class_err(out, ref))


# ---------------------------------------------------------------------------------------------------------------------------------------
# The stream kernel's 32-bit byte offsets (csrc/dense_stream.hip: load_rows, store_rows).  dense_corr_kernel (csrc/dense_corr.hip) sends a
# call there only while an image's output is at most 2^32 bytes and (N - 1) * 4 * b.stride_w + 4 * C <= 2^32; beyond either the maps go to
# the row-block kernel, whose addresses are 64-bit.  Each case asks stego_dense_corr_kernel FIRST and launches only if the answer is the
# expected one: a shape beyond a limit is never run through the stream kernel (no debug bit selects it either - bits 8192 and 1 << 21 only
# lead away from it).  B = 1, C = 72: the narrowest width the stream kernel takes.
_LIMIT_C = 72


def _stream_b_stride_limit(N, C):
    """Largest b.stride_w (a multiple of 4: 16-byte aligned pixels) with (N - 1) * 4 * stride_w + 4 * C <= 2^32."""
    return ((2 ** 32 - 4 * C) // (4 * (N - 1))) // 4 * 4


def _block_close(out, a_rows, b_rows, normalize, what):
    """out [R, Q] (fp32, device) against the fp64 product of a_rows [R, C] and b_rows [Q, C], computed on the device; the two bars of
    test_dense_stream_kernel_shapes."""
    a64, b64 = a_rows.double(), b_rows.double()
    if normalize:                                     # norm(): F.normalize(dim=1, eps=1e-10), modules.py:275-276
        a64 = a64 / a64.norm(dim=1, keepdim=True).clamp_min(1e-10)
        b64 = b64 / b64.norm(dim=1, keepdim=True).clamp_min(1e-10)
    ref = a64 @ b64.T
    diff = (out.double() - ref).abs()
    assert bool(torch.isfinite(out).all()), what
    scale = float(ref.abs().mean())
    tol = 1e-3 * ref.abs() + (2e-5 * max(scale, 1e-3) + 1e-6)                      # assert_allclose(rtol=1e-3, atol=2e-5 * max(scale, 1e-3) + 1e-6)
    worst = float((diff - tol).max())
    err = float(diff.max()) / max(float(ref.abs().max()), 1e-30)                  # _fp32_class_err
    print("%s: max |out - ref| / max |ref| = %.3g, worst margin to the allclose bar = %.3g" % (what, err, worst))
    assert worst <= 0.0, (what, worst)
    assert err < 2e-6, (what, err)


@pytest.mark.parametrize("H1,W1,normalize,expect", [
    (217, 151, True, "stream"),        # M = 32767: 2^32 - 131072 bytes of output per image, the last row pair ends 131072 bytes under the limit
    (257, 128, False, "rowblock"),     # M = 32896: 4.3 GB; rows 32768 .. 32895 begin at byte offsets >= 2^32
])
def test_dense_corr_output_at_the_stream_kernels_offset_limit(H1, W1, normalize, expect):
    from stego_amd import capi
    C, H2, W2 = _LIMIT_C, 128, 256
    M, N = H1 * W1, H2 * W2
    rng = np.random.default_rng(M)
    ta, tb = _cl_map(_varied(rng, 1, C, H1, W1)), _cl_map(_varied(rng, 1, C, H2, W2))
    assert capi.dense_corr_kernel(ta, tb) == expect                  # the guard: nothing is launched on a surprise
    assert (4 * M * N <= 2 ** 32) == (expect == "stream")
    out = capi.dense_corr(ta, tb, normalize=normalize).view(M, N)
    a_rows, b_rows = ta[0].permute(1, 2, 0).reshape(M, C), tb[0].permute(1, 2, 0).reshape(N, C)
    cross = 2 ** 32 // (4 * N)                                       # the first row whose byte offset row * N * 4 does not fit 32 bits
    mid = max(0, min(cross - 128, M - 256))
    for name, r0, r1 in (("first rows", 0, 256), ("rows around 2^32 bytes", mid, mid + 256), ("last rows", M - 128, M)):
        _block_close(out[r0:r1], a_rows[r0:r1], b_rows, normalize, "%d x %d, %s [%d, %d)" % (M, N, name, r0, r1))


@pytest.mark.parametrize("over,normalize,expect", [
    (True, True, "rowblock"),          # stride_w = 262400: pixel 4095 lies 4095 * 4 * 262400 = 4.298e9 > 2^32 bytes behind pixel 0
    (False, False, "stream"),          # the largest 16-byte aligned pixel stride under the limit: the last pixel's last byte ends < 2^32
])
def test_dense_corr_b_pixel_stride_at_the_stream_kernels_offset_limit(over, normalize, expect):
    """B is a 64 x 64 map of 72 channels whose pixels lie `stride_w` floats apart: channels [:72] of a [1, 4096, stride_w] buffer (1.07e9
    elements: under the 2^31 of a map view).  Only the view is filled."""
    from stego_amd import capi
    C, H1, W1, H2, W2 = _LIMIT_C, 16, 16, 64, 64
    M, N = H1 * W1, H2 * W2
    sw = 262400 if over else _stream_b_stride_limit(N, C)
    assert sw % 4 == 0 and ((N - 1) * 4 * sw + 4 * C > 2 ** 32) == over
    assert over or (N - 1) * 4 * (sw + 4) + 4 * C > 2 ** 32            # ... and the next aligned stride is over it
    rng = np.random.default_rng(sw)
    ta = _cl_map(_varied(rng, 1, C, H1, W1))
    buf = torch.empty(1, H2, W2, sw, dtype=torch.float32, device=DEV)
    tb = buf[..., :C].permute(0, 3, 1, 2)
    tb.copy_(torch.from_numpy(_varied(rng, 1, C, H2, W2)).to(DEV))
    assert tb.stride() == (N * sw, 1, W2 * sw, sw)
    assert capi.dense_corr_kernel(ta, tb) == expect                  # the guard: nothing is launched on a surprise
    out = capi.dense_corr(ta, tb, normalize=normalize).view(M, N)
    a_rows, b_rows = ta[0].permute(1, 2, 0).reshape(M, C), tb[0].permute(1, 2, 0).reshape(N, C)
    for name, q0 in (("first", 0), ("middle", N // 2 - 64), ("last", N - 128)):
        _block_close(out[:, q0:q0 + 128], a_rows, b_rows[q0:q0 + 128], normalize, "stride_w %d, %s B pixels [%d, %d)" % (sw, name, q0, q0 + 128))
