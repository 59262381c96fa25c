// The fused Adam step (include/stego_optim.h): every trainable tensor of every optimizer in one launch, step counters on the device.
//
// A streaming kernel over four fp32 arrays that is bound by launch latency, not by bytes (0.8 MB of parameters at ViT-S), so the one
// design goal is ONE launch: no table-building kernel in front, no counter kernel behind.
//
// Work split: a segment (one parameter tensor) is cut into chunks of STEGO_ADAM_CHUNK = 1024 elements, numbered through all segments;
// workgroup b of 256 threads takes chunks b, b + grid, ...  The chunk -> segment map is a scan over the table's counts: the trainer
// has 9 segments, the records are workgroup-uniform scalar loads from one or two cache lines, and a second table (chunk -> segment)
// would be one more thing the caller has to keep in step with the first.
//
// Alignment: ddp.FlatGradReducer packs gradients without padding, so a 70-element bias leaves every tensor behind it off 16-byte
// alignment.  Per chunk the kernel looks at the four addresses it is about to touch (chunk starts are multiples of 4 KB inside a
// segment, so this is the segment's alignment): all four 16-byte aligned -> one float4 per lane and array, the last count % 4
// elements one lane each; otherwise one float per lane and round.  Both paths run the same per-element arithmetic.
//
// Step counters: every wave reads steps[g] before it touches its chunk.  After its last chunk a workgroup meets at a barrier, then
// one lane draws a ticket (agent-scope atomic add behind a release fence).  The workgroup that draws the last ticket knows that every
// other workgroup has read its counters: it alone writes steps[g] + 1 for the active groups and zeroes the ticket for the next call.
// Nothing is handed from one workgroup to another, so no acquire is needed anywhere.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/stego_optim.h"
#include "host_util.h"

namespace {

constexpr int TPB = 256;
constexpr int CHUNK = STEGO_ADAM_CHUNK;
static_assert(CHUNK == 4 * TPB, "the 16-byte path moves one float4 per lane");

struct AdamParams {
    const StegoAdamSegment* segs;
    float* grads;
    float* m;
    float* v;
    int32_t* steps;
    unsigned* ticket;
    int32_t n_seg, n_groups, n_chunks, zero;
    StegoAdamGroup groups[STEGO_ADAM_MAX_GROUPS];
};

struct Scalars {
    float w1, beta2, w2, step_size, bc2_sqrt, eps;    // w1 = 1 - beta1, w2 = 1 - beta2
};

// beta^t by squaring, in double (t >= 1)
__device__ inline double ipow(double b, unsigned t)
{
    double r = 1.0;
    for (; t; t >>= 1) {
        if (t & 1) r *= b;
        b *= b;
    }
    return r;
}

__device__ inline void adam(float g, float& m, float& v, float& p, const Scalars& s)
{
    m = m + s.w1 * (g - m);
    v = s.beta2 * v + s.w2 * g * g;
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p - s.step_size * (m / denom);
}

__global__ __launch_bounds__(TPB) void adam_step_kernel(AdamParams p)
{
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < p.n_chunks; c += gridDim.x) {
        // the segment of chunk c: `first` is the number of chunks of the segments before it
        int s = 0, first = 0;
        int64_t count = 0;
        for (; s < p.n_seg; ++s) {
            count = p.segs[s].count;
            const int nc = (int)((count + CHUNK - 1) / CHUNK);
            if (c < first + nc) break;
            first += nc;
        }
        if (s >= p.n_seg) break;                                  // (a device table that disagrees with the host's: touch nothing)
        const StegoAdamSegment sg = p.segs[s];
        const int g = sg.group;
        if (g < 0 || g >= p.n_groups || !p.groups[g].active) continue;
        const StegoAdamGroup grp = p.groups[g];
        const int32_t done = p.steps[g];
        const unsigned t = (unsigned)(done < 0 ? 0 : done) + 1u;

        const int64_t off = (int64_t)(c - first) * CHUNK;
        const int n = (int)(count - off < CHUNK ? count - off : CHUNK);
        float* const P = static_cast<float*>(sg.param) + off;
        float* const G = p.grads + sg.grad_offset + off;
        float* const M = p.m + sg.state_offset + off;
        float* const V = p.v + sg.state_offset + off;
        const bool wide = ((reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(M) |
                            reinterpret_cast<uintptr_t>(V)) & 15) == 0;

        // the loads first: the double-precision scalars below are computed while they are in flight
        float4 g4, m4, v4, p4;
        float g1 = 0.f, m1 = 0.f, v1 = 0.f, p1 = 0.f;
        const int q = n >> 2;                                      // whole float4 of the chunk
        const int tail = 4 * q + tid;                              // the 16-byte path's one-by-one elements: lanes 0 .. n % 4 - 1
        const bool has4 = wide && tid < q, has1 = wide && tail < n;
        if (has4) {
            g4 = reinterpret_cast<const float4*>(G)[tid];
            m4 = reinterpret_cast<const float4*>(M)[tid];
            v4 = reinterpret_cast<const float4*>(V)[tid];
            p4 = reinterpret_cast<const float4*>(P)[tid];
        }
        if (has1) {
            g1 = G[tail];
            m1 = M[tail];
            v1 = V[tail];
            p1 = P[tail];
        }

        Scalars sc;
        {
            const double bc1 = 1.0 - ipow(grp.beta1, t), bc2 = 1.0 - ipow(grp.beta2, t);
            sc.w1 = (float)(1.0 - grp.beta1);
            sc.beta2 = (float)grp.beta2;
            sc.w2 = (float)(1.0 - grp.beta2);
            sc.step_size = (float)(grp.lr / bc1);
            sc.bc2_sqrt = (float)sqrt(bc2);
            sc.eps = (float)grp.eps;
        }

        if (wide) {
            if (has4) {
                adam(g4.x, m4.x, v4.x, p4.x, sc);
                adam(g4.y, m4.y, v4.y, p4.y, sc);
                adam(g4.z, m4.z, v4.z, p4.z, sc);
                adam(g4.w, m4.w, v4.w, p4.w, sc);
                reinterpret_cast<float4*>(M)[tid] = m4;
                reinterpret_cast<float4*>(V)[tid] = v4;
                reinterpret_cast<float4*>(P)[tid] = p4;
                if (p.zero) reinterpret_cast<float4*>(G)[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            if (has1) {
                adam(g1, m1, v1, p1, sc);
                M[tail] = m1;
                V[tail] = v1;
                P[tail] = p1;
                if (p.zero) G[tail] = 0.f;
            }
        } else {
#pragma unroll
            for (int r = 0; r < CHUNK / TPB; ++r) {
                const int i = r * TPB + tid;
                if (i < n) {
                    const float gi = G[i];
                    float mi = M[i], vi = V[i], pi = P[i];
                    adam(gi, mi, vi, pi, sc);
                    M[i] = mi;
                    V[i] = vi;
                    P[i] = pi;
                    if (p.zero) G[i] = 0.f;
                }
            }
        }
    }

    // every wave of this workgroup has read its counters; the workgroup that draws the last ticket advances them
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const unsigned drawn = __hip_atomic_fetch_add(p.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (drawn == gridDim.x - 1) {
            for (int g = 0; g < p.n_groups; ++g) {
                if (!p.groups[g].active) continue;
                const int32_t done = p.steps[g];
                p.steps[g] = done < 0 ? 1 : done < INT32_MAX ? done + 1 : done;
            }
            __hip_atomic_store(p.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

using stego::aligned;
using stego::hip_rc;

// Everything that can be checked without the buffers: the descriptor, then the table.  *n_chunks: the chunks of all segments.
int check(const StegoAdamDesc* d, const StegoAdamSegment* segs, int64_t* n_chunks)
{
    if (!d || !segs) return STEGO_ERR_NULL;
    if (d->n_segments < 1 || d->n_segments > STEGO_ADAM_MAX_SEGMENTS || d->n_groups < 1 || d->n_groups > STEGO_ADAM_MAX_GROUPS)
        return STEGO_ERR_OPTIM_COUNT;
    if (d->zero_grads != 0 && d->zero_grads != 1) return STEGO_ERR_OPTIM_FLAGS;
    bool any = false;
    for (int g = 0; g < d->n_groups; ++g) {
        if (d->groups[g].active != 0 && d->groups[g].active != 1) return STEGO_ERR_OPTIM_FLAGS;
        any = any || d->groups[g].active;
    }
    if (!any) return STEGO_ERR_OPTIM_FLAGS;
    for (int g = 0; g < d->n_groups; ++g) {
        const StegoAdamGroup& q = d->groups[g];
        if (!q.active) continue;
        if (!(q.beta1 >= 0.0 && q.beta1 < 1.0) || !(q.beta2 >= 0.0 && q.beta2 < 1.0)) return STEGO_ERR_OPTIM_PARAM;
        if (!std::isfinite(q.lr) || q.lr < 0.0 || !std::isfinite(q.eps) || q.eps < 0.0) return STEGO_ERR_OPTIM_PARAM;
    }
    int64_t total = 0, chunks = 0;
    for (int s = 0; s < d->n_segments; ++s) {
        const StegoAdamSegment& sg = segs[s];
        if (!sg.param) return STEGO_ERR_NULL;
        if (sg.count < 1 || sg.group < 0 || sg.group >= d->n_groups) return STEGO_ERR_OPTIM_SEGMENT;
        if (sg.count >= STEGO_ADAM_MAX_ELEMS) return STEGO_ERR_OPTIM_COUNT;
        if (sg.grad_offset < 0 || sg.grad_offset > d->grad_elems - sg.count || sg.state_offset < 0 ||
            sg.state_offset > d->state_elems - sg.count)
            return STEGO_ERR_OPTIM_SEGMENT;
        total += sg.count;                                        // < 256 * 2^31
        chunks += (sg.count + CHUNK - 1) / CHUNK;
    }
    if (total >= STEGO_ADAM_MAX_ELEMS) return STEGO_ERR_OPTIM_COUNT;
    *n_chunks = chunks;
    return STEGO_OK;
}

inline int32_t grid_for(int64_t n_chunks) { return (int32_t)(n_chunks < STEGO_ADAM_MAX_GRID ? n_chunks : STEGO_ADAM_MAX_GRID); }

}  // namespace

extern "C" int stego_adam_plan(const StegoAdamDesc* desc, const StegoAdamSegment* segments_host, int32_t* grid, int32_t* chunk,
                               int64_t* n_chunks)
{
    int64_t chunks = 0;
    const int rc = check(desc, segments_host, &chunks);
    if (rc != STEGO_OK) return rc;
    if (grid) *grid = grid_for(chunks);
    if (chunk) *chunk = CHUNK;
    if (n_chunks) *n_chunks = chunks;
    return STEGO_OK;
}

extern "C" int stego_adam_step(const StegoAdamDesc* desc, const StegoAdamSegment* segments_host, const StegoAdamSegment* segments,
                               float* grads, float* exp_avg, float* exp_avg_sq, int32_t* steps, uint32_t* ticket, stego_stream_t stream)
{
    if (!desc || !segments_host || !segments || !grads || !exp_avg || !exp_avg_sq || !steps || !ticket) return STEGO_ERR_NULL;
    int64_t chunks = 0;
    const int rc = check(desc, segments_host, &chunks);
    if (rc != STEGO_OK) return rc;
    if (!aligned(segments, 8) || !aligned(grads, 4) || !aligned(exp_avg, 4) || !aligned(exp_avg_sq, 4) || !aligned(steps, 4) ||
        !aligned(ticket, 4))
        return STEGO_ERR_ALIGN;
    for (int s = 0; s < desc->n_segments; ++s)
        if (!aligned(segments_host[s].param, 4)) return STEGO_ERR_ALIGN;

    AdamParams p{};
    p.segs = segments;
    p.grads = grads;
    p.m = exp_avg;
    p.v = exp_avg_sq;
    p.steps = steps;
    p.ticket = ticket;
    p.n_seg = desc->n_segments;
    p.n_groups = desc->n_groups;
    p.n_chunks = (int32_t)chunks;                                 // < 2^21 + 256
    p.zero = desc->zero_grads;
    for (int g = 0; g < STEGO_ADAM_MAX_GROUPS; ++g) p.groups[g] = desc->groups[g];
    return hip_rc(stego::launch_first<adam_step_kernel>(grid_for(chunks), TPB, 0, static_cast<hipStream_t>(stream), p));
}
