// Coloured segmentation pictures (include/stego_render.h): the range of the un-normalised image and the one-launch render of label
// colours, the image, or the image under the label colours into packed uint8 RGB at a byte-strided target.
//
// stego_render.  A workgroup renders ROWS rows of one image times one CHUNK: 768 bytes of every row counted from the row's own
// 16-byte aligned address A_r = row address & ~15, so chunk c of row r is the aligned global range [A_r + 768 c, A_r + 768 (c + 1)).
// The pixels of a row that a chunk holds therefore shift by up to 15 bytes from row to row (the target's strides have byte
// alignment only), and a pixel that straddles two chunks is computed by both.
//   1. the label tile: rows y0 .. y0 + ROWS (one halo row), columns 256 c - 16 .. 256 c + 271 (the chunk's pixels of every row
//      alignment, and one halo column), 16 bytes per lane where the row is dense and aligned, as stored (int64 stays int64: the
//      edge rule compares what is stored), all loads of a lane issued before the first is used;
//   2. the pixels, four per lane and step with their image values loaded together, three bytes each into the row's 768-byte stage
//      in LDS at the byte's place in the chunk;
//   3. the stage leaves as 16-byte stores of aligned addresses; a 16-byte piece that the row covers only in part - the row's head
//      and tail - leaves as byte stores of the covered bytes.  Nothing outside the B x H x 3W panel bytes is written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/stego_render.h"
#include "host_util.h"
#include "rgb_rows.h"

using namespace stego;

// The header's arithmetic is a sequence of individually rounded operations (the reference's mul_ then add_; the blend's two products
// and their sum).  HIP's __fmul_rn / __fadd_rn are plain operators, defined in a header that is compiled with the default
// -ffp-contract=fast, and fuse: the arithmetic below uses the operators themselves, with contraction off for the whole unit.
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int PIX_BATCH = 4;             // pixels of a lane whose image values are in flight together
constexpr int TILE_BACK = 16;            // the label tile starts 16 columns in front of 256 c: a 16-byte boundary for every label type
constexpr int TILE_W = CPIX + 2 * TILE_BACK;
constexpr int RANGE_MAX_WG = 1024;       // workgroups per image of the range's first launch
constexpr int RANGE_PIX_PER_WG = 2048;

struct RenderParams {
    StegoMap img;
    const void* labels;
    const uint8_t* lut;
    const float* range;
    uint8_t* out;
    int64_t lsn, lsh, lsw;               // label strides, elements
    int64_t osn, osh;                    // target strides, bytes
    int B, H, W, n_lut, flags;
    float alpha;
    float mean[3], std[3];
    uint32_t ignore_rgb, edge_rgb;       // R | G << 8 | B << 16
};

struct RangeParams {
    StegoMap img;
    float* partial;                      // [B][nwg][2]
    float* range;                        // [B][2]
    int B, H, W, nwg;
    float mean[3], std[3];
};

// x * std + mean as two rounded operations (the reference's mul_ then add_)
__device__ __forceinline__ float unnormalise(float x, float s, float m)
{
    const float scaled = x * s;
    return scaled + m;
}

template <class LT>
__global__ __launch_bounds__(TPB) void render_kernel(const RenderParams p)
{
    using ST = typename std::conditional<std::is_same<LT, int64_t>::value, int64_t, int32_t>::type;
    constexpr int VEC = 16 / (int)sizeof(LT);
    __shared__ __attribute__((aligned(16))) ST tile[(ROWS + 1) * TILE_W];
    __shared__ __attribute__((aligned(16))) uint8_t stage[ROWS * CHUNK];
    __shared__ uint32_t lut[STEGO_RENDER_MAX_LUT];

    const int t = threadIdx.x;
    const int c = blockIdx.x, y0 = blockIdx.y * ROWS, b = blockIdx.z;
    const bool has_img = p.flags & STEGO_RENDER_IMAGE, has_lab = p.flags & STEGO_RENDER_LABELS;
    const bool edges = p.flags & STEGO_RENDER_EDGES, blend = p.flags & STEGO_RENDER_BLEND, rescale = p.flags & STEGO_RENDER_RESCALE;
    const int tile_x0 = c * CPIX - TILE_BACK;

    if (has_lab) {
        for (int i = t; i < p.n_lut; i += TPB)
            lut[i] = (uint32_t)p.lut[3 * i] | ((uint32_t)p.lut[3 * i + 1] << 8) | ((uint32_t)p.lut[3 * i + 2] << 16);
        const LT* lab = static_cast<const LT*>(p.labels) + (int64_t)b * p.lsn;
        // every load of the thread is issued before the first is used: the tile costs one trip to memory, not one per step
        constexpr int ITEMS = TILE_W / VEC, N_ITEMS = (ROWS + 1) * ITEMS, STEPS = (N_ITEMS + TPB - 1) / TPB;
        u32x4 q[STEPS];
        int how[STEPS];                                                  // 0: nothing to load, 1: loaded as 16 bytes, 2: by element
#pragma unroll
        for (int k = 0; k < STEPS; ++k) {
            const int i = t + k * TPB;
            const int r = i / ITEMS, x = tile_x0 + (i - r * ITEMS) * VEC, y = y0 + r;
            how[k] = 0;
            q[k] = u32x4{0u, 0u, 0u, 0u};
            if (i >= N_ITEMS || y >= p.H || x + VEC <= 0 || x >= p.W) continue;      // (never read: every read below tests y and x first)
            const LT* src = lab + (int64_t)y * p.lsh + (int64_t)x * p.lsw;
            how[k] = 2;
            if (p.lsw == 1 && x >= 0 && x + VEC <= p.W && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
                q[k] = *reinterpret_cast<const u32x4*>(src);
                how[k] = 1;
            }
        }
#pragma unroll
        for (int k = 0; k < STEPS; ++k) {
            if (how[k] == 0) continue;
            const int i = t + k * TPB;
            const int r = i / ITEMS, x = tile_x0 + (i - r * ITEMS) * VEC, y = y0 + r;
            ST* dst = tile + r * TILE_W + (x - tile_x0);
            if (how[k] == 1) {
                union { u32x4 q; LT e[VEC]; } u;
                u.q = q[k];
#pragma unroll
                for (int e = 0; e < VEC; ++e) dst[e] = (ST)u.e[e];
            } else {
                const LT* src = lab + (int64_t)y * p.lsh + (int64_t)x * p.lsw;
                for (int e = 0; e < VEC; ++e)
                    if (x + e >= 0 && x + e < p.W) dst[e] = (ST)src[(int64_t)e * p.lsw];
            }
        }
    }
    __syncthreads();

    float lo = 0.f, span = 0.f;
    if (rescale) {
        lo = p.range[2 * b];
        span = p.range[2 * b + 1] - lo;
    }
    const float wi = 1.f - p.alpha;
    uint8_t* const out_b = p.out + (int64_t)b * p.osn;
    const int pix_x0 = c * CPIX - PIX_BACK;
    // PIX_BATCH pixels per step, their image values loaded before the first is used
    constexpr int N_PIX = ROWS * PIX_SPAN;
    for (int base = t; base < N_PIX; base += PIX_BATCH * TPB) {
        float val[PIX_BATCH][3];
        bool live[PIX_BATCH];
#pragma unroll
        for (int u = 0; u < PIX_BATCH; ++u) {
            const int i = base + u * TPB;
            const int r = i / PIX_SPAN, x = pix_x0 + (i - r * PIX_SPAN), y = y0 + r;
            live[u] = false;
            val[u][0] = val[u][1] = val[u][2] = 0.f;
            if (i >= N_PIX || y >= p.H || x < 0 || x >= p.W) continue;
            const int at = pixel_place(out_b + (int64_t)y * p.osh, x, c);
            if (at + 2 < 0 || at >= CHUNK) continue;
            live[u] = true;
            if (has_img) {
                const float* src = p.img.data + (int64_t)b * p.img.stride_n + (int64_t)y * p.img.stride_h + (int64_t)x * p.img.stride_w;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) val[u][ch] = src[(int64_t)ch * p.img.stride_c];
            }
        }
#pragma unroll
        for (int u = 0; u < PIX_BATCH; ++u) {
            if (!live[u]) continue;
            const int i = base + u * TPB;
            const int r = i / PIX_SPAN, x = pix_x0 + (i - r * PIX_SPAN), y = y0 + r;
            const int at = pixel_place(out_b + (int64_t)y * p.osh, x, c);
            uint32_t rgb = 0;
            if (has_lab) {
                const ST* row = tile + r * TILE_W + (x - tile_x0);
                const ST l = row[0];
                rgb = (l >= 0 && l < (ST)p.n_lut) ? lut[(int)l] : p.ignore_rgb;
                if (edges && ((x + 1 < p.W && row[1] != l) || (y + 1 < p.H && row[TILE_W] != l))) rgb = p.edge_rgb;
            }
            uint32_t px = rgb;
            if (has_img) {
                px = 0;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float v = unnormalise(val[u][ch], p.std[ch], p.mean[ch]);
                    if (rescale)
                        v = span == 0.f ? 0.f : (v - lo) / span;
                    else
                        v = fminf(fmaxf(v, 0.f), 1.f);
                    if (blend) {
                        const float under = wi * v, over = p.alpha * ((float)((rgb >> (8 * ch)) & 255u) / 255.f);
                        v = under + over;
                    }
                    px |= to_level(v) << (8 * ch);
                }
            }
            put_pixel(stage + r * CHUNK, at, px);
        }
    }
    __syncthreads();
    store_rows<TPB>(out_b, p.osh, stage, c, y0, p.H, p.W);
}

__device__ __forceinline__ void wave_min_max(float& lo, float& hi)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, m));
        hi = fmaxf(hi, __shfl_xor(hi, m));
    }
}

// the minimum and maximum of one (lo, hi) per thread over the workgroup, valid in thread 0
__device__ __forceinline__ void block_min_max(float& lo, float& hi, float* red)
{
    wave_min_max(lo, hi);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[2 * wave] = lo;
        red[2 * wave + 1] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < TPB / 64; ++w) {
            lo = fminf(lo, red[2 * w]);
            hi = fmaxf(hi, red[2 * w + 1]);
        }
}

__global__ __launch_bounds__(TPB) void range_partial_kernel(const RangeParams p)
{
    __shared__ float red[2 * TPB / 64];
    const int b = blockIdx.y;
    const int64_t HW = (int64_t)p.H * p.W;
    const float* img = p.img.data + (int64_t)b * p.img.stride_n;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < HW; i += (int64_t)p.nwg * TPB) {
        const int y = (int)(i / p.W), x = (int)(i - (int64_t)y * p.W);
        const float* src = img + (int64_t)y * p.img.stride_h + (int64_t)x * p.img.stride_w;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float v = unnormalise(src[(int64_t)ch * p.img.stride_c], p.std[ch], p.mean[ch]);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    block_min_max(lo, hi, red);
    if (threadIdx.x == 0) {
        float* dst = p.partial + 2 * ((int64_t)b * p.nwg + blockIdx.x);
        dst[0] = lo;
        dst[1] = hi;
    }
}

__global__ __launch_bounds__(TPB) void range_final_kernel(const RangeParams p)
{
    __shared__ float red[2 * TPB / 64];
    const int b = blockIdx.x;
    const float* src = p.partial + 2 * (int64_t)b * p.nwg;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < p.nwg; i += TPB) {
        lo = fminf(lo, src[2 * i]);
        hi = fmaxf(hi, src[2 * i + 1]);
    }
    block_min_max(lo, hi, red);
    if (threadIdx.x == 0) {
        p.range[2 * b] = lo;
        p.range[2 * b + 1] = hi;
    }
}

int check_size(const StegoRenderDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->B < 1 || d->B > 65535 || d->H < 1 || d->H > STEGO_STITCH_MAX_SIDE || d->W < 1 || d->W > STEGO_STITCH_MAX_SIDE)
        return STEGO_ERR_RENDER_SIZE;
    return STEGO_OK;
}

int check_unnorm(const StegoRenderDesc* d)
{
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(d->mean[c]) || !std::isfinite(d->std[c])) return STEGO_ERR_RENDER_PARAM;
    return STEGO_OK;
}

int check_desc(const StegoRenderDesc* d)
{
    int rc = check_size(d);
    if (rc != STEGO_OK) return rc;
    const int f = d->flags;
    const int all = STEGO_RENDER_IMAGE | STEGO_RENDER_LABELS | STEGO_RENDER_EDGES | STEGO_RENDER_BLEND | STEGO_RENDER_RESCALE;
    if (f & ~all) return STEGO_ERR_RENDER_FLAGS;
    const bool img = f & STEGO_RENDER_IMAGE, lab = f & STEGO_RENDER_LABELS;
    if (!img && !lab) return STEGO_ERR_RENDER_SELECT;
    if (((f & STEGO_RENDER_BLEND) != 0) != (img && lab)) return STEGO_ERR_RENDER_SELECT;
    if ((f & STEGO_RENDER_EDGES) && !lab) return STEGO_ERR_RENDER_SELECT;
    if ((f & STEGO_RENDER_RESCALE) && !img) return STEGO_ERR_RENDER_SELECT;
    if (lab) {
        if (d->n_lut < 1 || d->n_lut > STEGO_RENDER_MAX_LUT) return STEGO_ERR_RENDER_LUT;
        if (d->label_dtype != STEGO_RENDER_I64 && d->label_dtype != STEGO_RENDER_I32 && d->label_dtype != STEGO_RENDER_U8)
            return STEGO_ERR_RENDER_DTYPE;
    }
    if ((f & STEGO_RENDER_BLEND) && !(d->alpha >= 0.f && d->alpha <= 1.f)) return STEGO_ERR_RENDER_PARAM;
    if (img && (rc = check_unnorm(d)) != STEGO_OK) return rc;
    return STEGO_OK;
}

int range_workgroups(const StegoRenderDesc* d)
{
    const int64_t n = ((int64_t)d->H * d->W + RANGE_PIX_PER_WG - 1) / RANGE_PIX_PER_WG;
    return (int)(n < RANGE_MAX_WG ? n : RANGE_MAX_WG);
}

struct RangeLayout {
    size_t partial, total;
};

RangeLayout range_layout(const StegoRenderDesc* d)
{
    WsLayout ws;
    RangeLayout l;
    l.partial = ws.take((size_t)d->B * range_workgroups(d) * 2 * sizeof(float), 16);
    l.total = ws.total(16);
    return l;
}

uint32_t pack_rgb(const uint8_t* c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

}  // namespace

extern "C" size_t stego_image_range_workspace_bytes(const StegoRenderDesc* desc)
{
    if (check_size(desc) != STEGO_OK || check_unnorm(desc) != STEGO_OK) return 0;
    return range_layout(desc).total;
}

extern "C" int stego_image_range(const StegoRenderDesc* desc, const StegoMap* image, float* range, void* workspace, size_t workspace_bytes,
                                 stego_stream_t stream)
{
    int rc = check_size(desc);
    if (rc == STEGO_OK) rc = check_unnorm(desc);
    if (rc != STEGO_OK) return rc;
    if (!image || !image->data || !range || !workspace) return STEGO_ERR_NULL;
    const RangeLayout lay = range_layout(desc);
    if (workspace_bytes < lay.total) return STEGO_ERR_WORKSPACE;
    if (!aligned(image->data, 4) || !aligned(range, 4) || !aligned(workspace, 4)) return STEGO_ERR_ALIGN;
    RangeParams p{};
    p.img = *image;
    p.partial = at<float>(workspace, lay.partial);
    p.range = range;
    p.B = desc->B;
    p.H = desc->H;
    p.W = desc->W;
    p.nwg = range_workgroups(desc);
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = desc->mean[c];
        p.std[c] = desc->std[c];
    }
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_first<range_partial_kernel>(dim3((unsigned)p.nwg, (unsigned)p.B), TPB, 0, s, p);
    if (e == hipSuccess) e = launch_next<range_final_kernel>(dim3((unsigned)p.B), TPB, 0, s, p);
    return hip_rc(e);
}

extern "C" int stego_render(const StegoRenderDesc* desc, const StegoMap* image, const void* labels, const uint8_t* lut, const float* range,
                            uint8_t* out, stego_stream_t stream)
{
    const int rc = check_desc(desc);
    if (rc != STEGO_OK) return rc;
    const int f = desc->flags;
    const bool img = f & STEGO_RENDER_IMAGE, lab = f & STEGO_RENDER_LABELS, resc = f & STEGO_RENDER_RESCALE;
    if (!out || (img && (!image || !image->data)) || (lab && (!labels || !lut)) || (resc && !range)) return STEGO_ERR_NULL;
    const size_t lab_size = desc->label_dtype == STEGO_RENDER_I64 ? 8 : desc->label_dtype == STEGO_RENDER_I32 ? 4 : 1;
    if ((img && !aligned(image->data, 4)) || (resc && !aligned(range, 4)) || (lab && !aligned(labels, lab_size))) return STEGO_ERR_ALIGN;
    RenderParams p{};
    if (img) p.img = *image;
    p.labels = lab ? labels : nullptr;
    p.lut = lab ? lut : nullptr;
    p.range = resc ? range : nullptr;
    p.out = out;
    p.lsn = desc->label_stride_n;
    p.lsh = desc->label_stride_h;
    p.lsw = desc->label_stride_w;
    p.osn = desc->out_stride_n;
    p.osh = desc->out_stride_h;
    p.B = desc->B;
    p.H = desc->H;
    p.W = desc->W;
    p.n_lut = lab ? desc->n_lut : 0;
    p.flags = f;
    p.alpha = desc->alpha;
    for (int c = 0; c < 3; ++c) {
        p.mean[c] = desc->mean[c];
        p.std[c] = desc->std[c];
    }
    p.ignore_rgb = pack_rgb(desc->ignore_rgb);
    p.edge_rgb = pack_rgb(desc->edge_rgb);
    // a row's bytes start up to 15 bytes behind its aligned address: chunks of 3 W + 15 bytes at the most
    const dim3 grid((unsigned)((3 * desc->W + 15 + CHUNK - 1) / CHUNK), (unsigned)((desc->H + ROWS - 1) / ROWS), (unsigned)desc->B);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int dtype = lab ? desc->label_dtype : STEGO_RENDER_I32;
    hipError_t e;
    if (dtype == STEGO_RENDER_I64)
        e = launch_first<render_kernel<int64_t>>(grid, TPB, 0, s, p);
    else if (dtype == STEGO_RENDER_I32)
        e = launch_first<render_kernel<int32_t>>(grid, TPB, 0, s, p);
    else
        e = launch_first<render_kernel<uint8_t>>(grid, TPB, 0, s, p);
    return hip_rc(e);
}
