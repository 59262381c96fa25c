"""Which kernel the dense correlation takes (stego_dense_corr_kernel -> dense_corr_kernel, csrc/dense_corr.hip: the one predicate
launch_dense_corr itself asks): host arithmetic on strides and dimensions, asked here without a GPU through ctypes with map pointers that
are never dereferenced.  The stream kernel (csrc/dense_stream.hip) forms 32-bit unsigned byte offsets; its two limits are pinned at the
last value under, the first value over and a value far over each."""
import ctypes
import os

import pytest

from stego_amd import capi

STREAM, ROWBLOCK, TILE = 0, 1, 2
ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_ALIGN = 1, 2, 3, 5
FAKE = 0x7f0000000000            # 16-byte aligned, never read


def _cl(C, H, W, sw=None, data=FAKE):
    """Channels-last [*, C, H, W]: pixels `sw` floats apart (default: dense, sw = C)."""
    sw = C if sw is None else sw
    return capi.StegoMap(data, H * W * sw, 1, W * sw, sw)


def _nchw(C, H, W, data=FAKE):
    return capi.StegoMap(data, C * H * W, H * W, W, 1)


def _kernel(a, b, B, C, H1, W1, H2, W2):
    return capi.load().stego_dense_corr_kernel(ctypes.byref(a), ctypes.byref(b), B, C, H1, W1, H2, W2)


def _cl_pair(B, C, H1, W1, H2, W2):
    return _kernel(_cl(C, H1, W1), _cl(C, H2, W2), B, C, H1, W1, H2, W2)


def _nchw_pair(B, C, H1, W1, H2, W2):
    return _kernel(_nchw(C, H1, W1), _nchw(C, H2, W2), B, C, H1, W1, H2, W2)


@pytest.fixture
def debug_knob():
    base = int(os.environ.get("STEGO_DEBUG", "0"))
    capi.debug_set("STEGO_DEBUG", base & ~((1 << 21) | 8192))
    yield lambda bits: capi.debug_set("STEGO_DEBUG", (base & ~((1 << 21) | 8192)) | bits)
    capi.debug_set("STEGO_DEBUG", base)


def test_the_shapes_of_the_gpu_tests_take_the_kernels_their_comments_name(debug_knob):
    """tests/test_dense_corr.py, test by test."""
    # test_dense_stream_kernel_shapes, test_dense_stream_raw_products_any_magnitude: "csrc/dense_stream.hip (channels-last, 64 < C <= 384, C % 8 == 0)"
    for shape in ((3, 192, 14, 14, 14, 14), (2, 136, 9, 13, 7, 11), (9, 328, 12, 12, 20, 20), (1, 72, 16, 16, 16, 16), (2, 256, 3, 50, 50, 3),
                  (2, 96, 6, 7, 5, 4)):
        assert _cl_pair(*shape) == STREAM, shape
    # test_dense_corr_matches_float64_einsum: ViT-S/8 channels-last is the stream kernel's own case; C = 768 has twelve chunks, C = 70 and
    # C = 5 no 16-byte pixels, NCHW maps no channels-last pixels at all: the tile kernel
    assert _cl_pair(2, 384, 28, 28, 28, 28) == STREAM
    for shape in ((1, 768, 40, 40, 40, 40), (3, 70, 5, 9, 11, 3), (2, 5, 1, 1, 2, 200)):
        assert _cl_pair(*shape) == TILE, shape
    for shape in ((2, 384, 28, 28, 28, 28), (1, 768, 40, 40, 40, 40), (3, 70, 5, 9, 11, 3), (2, 5, 1, 1, 2, 200), (2, 96, 6, 7, 5, 4)):
        assert _nchw_pair(*shape) == TILE, shape
    # test_dense_rowblock_kernel_narrow_channels: "dense_rowblock_kernel<false> ... C <= 64"
    for C in (8, 32, 64):
        assert _cl_pair(2, C, 9, 13, 7, 11) == ROWBLOCK, C
    # test_dense_rowblock_kernel_cropped_b_view: b = a 16 x 17 map's [1:-1, 2:-1], so b.stride_h = 17 C != W2 * C
    C = 384
    crop = capi.StegoMap(FAKE + 4 * C * (17 + 2), 16 * 17 * C, 1, 17 * C, C)
    assert _kernel(_cl(C, 14, 14), crop, 2, C, 14, 14, 14, 14) == ROWBLOCK
    # test_dense_corr_every_kernel_on_one_input: stream by default, bit 21 the row-block kernel, 8192 the tile kernel
    for C in (136, 384):
        for bits, want in ((0, STREAM), (1 << 21, ROWBLOCK), (8192, TILE), (8192 | (1 << 21), TILE)):
            debug_knob(bits)
            assert _cl_pair(3, C, 9, 13, 12, 12) == want, (C, bits)
    # test_tensor_correlation_gradients_run_on_the_native_kernel: an NCHW a against a channels-last b
    debug_knob(0)
    assert _kernel(_nchw(384, 28, 28), _cl(384, 28, 28), 3, 384, 28, 28, 28, 28) == TILE


def test_what_keeps_a_call_from_the_stream_kernel_today_still_does(debug_knob):
    assert _cl_pair(1, 72, 16, 16, 16, 16) == STREAM
    assert _cl_pair(1, 64, 16, 16, 16, 16) == ROWBLOCK                 # C <= 64: one chunk
    assert _cl_pair(1, 76, 16, 16, 16, 16) == TILE                     # C % 8 != 0 (16-byte pixels, but the kernels convert 8 channels a lane)
    assert _cl_pair(1, 70, 16, 16, 16, 16) == TILE                     # C % 4 != 0
    assert _cl_pair(1, 392, 16, 16, 16, 16) == TILE                    # seven chunks
    assert _nchw_pair(1, 72, 16, 16, 16, 16) == TILE
    assert _kernel(_cl(72, 16, 16), _nchw(72, 16, 16), 1, 72, 16, 16, 16, 16) == TILE
    assert _kernel(_cl(72, 16, 16, data=FAKE + 4), _cl(72, 16, 16), 1, 72, 16, 16, 16, 16) == TILE      # pixels not 16-byte aligned
    padded = capi.StegoMap(FAKE, 16 * 20 * 72, 1, 20 * 72, 72)         # rows of 16 pixels, 20 apart: pixel p is not at p * stride_w
    assert _kernel(_cl(72, 16, 16), padded, 1, 72, 16, 16, 16, 16) == ROWBLOCK
    assert _kernel(padded, _cl(72, 16, 16), 1, 72, 16, 16, 16, 16) == STREAM                            # (the A side is addressed by h and w)
    for bits, want in ((8192, TILE), (1 << 21, ROWBLOCK)):
        debug_knob(bits)
        assert _cl_pair(1, 72, 16, 16, 16, 16) == want


def test_stream_kernel_output_limit_is_2_to_32_bytes_per_image(debug_knob):
    """store_rows: ordo + k * rowp + 4 * njp * TP in unsigned - the largest offset stored to is 4 * M * N - 16."""
    C = 72
    assert _cl_pair(1, C, 217, 151, 128, 256) == STREAM                # 2^32 - 131072 bytes (the GPU test's shape)
    assert _cl_pair(1, C, 128, 256, 128, 256) == STREAM                # exactly 2^32 bytes: the last 16-byte store begins at 2^32 - 16
    assert _cl_pair(1, C, 1, 32769, 128, 256) == ROWBLOCK              # one row more
    assert _cl_pair(1, C, 257, 128, 128, 256) == ROWBLOCK              # 4.3 GB (the GPU test's shape)
    assert _cl_pair(1, C, 181, 181, 181, 181) == STREAM                # two square maps: 181^4 * 4 = 2^32 - 1834812 bytes ...
    assert _cl_pair(1, C, 182, 182, 182, 182) == ROWBLOCK              # ... and 182^4 * 4 = 4.39e9
    assert _cl_pair(1, C, 256, 256, 256, 256) == ROWBLOCK              # 2^34 bytes
    assert _cl_pair(1, C, 4096, 4096, 16, 16) == ROWBLOCK              # 2^34 bytes, the largest A map
    assert _cl_pair(1, C, 1, 64, 1024, 2048) == STREAM                 # M * N = 2^27, a long B map: N * C * 4 = 2^29 * 1.125 bytes
    for B in (2, 9, 65535):                                            # the limit is per image
        assert _cl_pair(B, C, 128, 256, 128, 256) == STREAM and _cl_pair(B, C, 1, 32769, 128, 256) == ROWBLOCK


def test_stream_kernel_b_offset_limit_is_2_to_32_bytes(debug_knob):
    """load_rows: min(p, N - 1) * (4 * stride_w) + 4 * channel in unsigned - the last byte read lies at (N - 1) * 4 * stride_w + 4 * C - 1."""
    C, H2, W2 = 72, 64, 64
    N = H2 * W2

    def k(sw, C=C, H2=H2, W2=W2):
        return _kernel(_cl(C, 16, 16), _cl(C, H2, W2, sw=sw), 1, C, 16, 16, H2, W2)

    sw_max = ((2 ** 32 - 4 * C) // (4 * (N - 1))) // 4 * 4
    assert sw_max == 262204 and (N - 1) * 4 * sw_max + 4 * C <= 2 ** 32 < (N - 1) * 4 * (sw_max + 4) + 4 * C
    assert k(sw_max) == STREAM
    assert k(sw_max + 4) == ROWBLOCK
    assert k(262400) == ROWBLOCK                                       # the GPU test's stride
    # far over: a map view holds less than 2^31 elements (to_mapv), so no accepted B offset reaches 2^33 bytes - the largest one ...
    sw_far = ((2 ** 31 - 2 - (C - 1)) // (N - 1)) // 4 * 4
    assert (N - 1) * 4 * sw_far > 2 ** 33 - 2 ** 22 and k(sw_far) == ROWBLOCK
    assert k(sw_far + 4) == -ERR_UNSUPPORTED                           # ... and the first one the argument check refuses, as stego_dense_corr does
    # dense maps reach the limit as well: N * C in (2^30, 2^31)
    assert k(384, C=384, H2=1024, W2=2048) == STREAM                  # 2^21 pixels: 3 * 2^30 bytes
    assert k(384, C=384, H2=1366, W2=2047) == STREAM                  # (N - 1) * 1536 + 1536 = 4294966272 <= 2^32
    assert k(384, C=384, H2=2731, W2=1024) == ROWBLOCK                # N = 2796544: 1024 bytes over
    assert k(384, C=384, H2=2048, W2=2048) == ROWBLOCK                # 6.4e9 bytes
    # one pixel: no stride enters an address
    assert _kernel(_cl(C, 16, 16), capi.StegoMap(FAKE, 4, 1, 2 ** 30, 2 ** 30), 1, C, 16, 16, 1, 1) == STREAM


def test_argument_checks_are_those_of_stego_dense_corr_and_the_fallbacks_have_their_own_limits(debug_knob):
    a, b = _cl(72, 16, 16), _cl(72, 16, 16)
    lib = capi.load()
    assert lib.stego_dense_corr_kernel(None, ctypes.byref(b), 1, 72, 16, 16, 16, 16) == -ERR_NULL
    assert _kernel(a, capi.StegoMap(None, 1, 1, 1, 1), 1, 72, 16, 16, 16, 16) == -ERR_NULL
    assert _kernel(a, b, 0, 72, 16, 16, 16, 16) == -ERR_SHAPE and _kernel(a, b, 1, 72, 16, 0, 16, 16) == -ERR_SHAPE
    assert _kernel(a, b, 65536, 72, 16, 16, 16, 16) == -ERR_UNSUPPORTED
    assert _cl_pair(1, 8, 4096, 4097, 1, 1) == -ERR_UNSUPPORTED        # H * W > 2^24
    assert _kernel(_cl(72, 16, 16, data=FAKE + 2), b, 1, 72, 16, 16, 16, 16) == -ERR_ALIGN
    assert _kernel(a, capi.StegoMap(FAKE, 1, 1, -1, 1), 1, 72, 16, 16, 16, 16) == -ERR_UNSUPPORTED       # negative stride
    # the tile kernel's row blocks of A are the grid's y dimension (<= 65535); the row-block kernel's are part of its x dimension
    assert _nchw_pair(1, 3, 65535, 128, 1, 1) == TILE
    assert _nchw_pair(1, 3, 65536, 128, 1, 1) == -ERR_UNSUPPORTED
    assert _cl_pair(1, 8, 65536, 128, 1, 1) == ROWBLOCK
    # every kernel's x grid is images x blocks, formed in int
    assert _cl_pair(65535, 8, 256, 128, 1, 1) == ROWBLOCK              # 65536 * 256 blocks
    assert _cl_pair(65535, 8, 4096, 4096, 1, 1) == -ERR_UNSUPPORTED    # 65536 * 2^17 = 2^33 blocks
    assert b"dense correlation" in lib.stego_error_string(ERR_UNSUPPORTED)
    # stego_dense_corr answers the same before it touches a pointer's target or the device (a non-NULL output and workspace of enough bytes)
    na, nb = _nchw(3, 65536, 128), _nchw(3, 1, 1)
    ws = lib.stego_dense_corr_workspace_bytes(1, 3, 65536, 128, 1, 1)
    assert ws > 0
    assert lib.stego_dense_corr(ctypes.byref(na), ctypes.byref(nb), 1, 3, 65536, 128, 1, 1, 0, FAKE, FAKE, ws, None) == ERR_UNSUPPORTED
