// Device-side step statistics (include/stego_stats.h): up to four fp32 tensors read once, one record into a ring, one launch.
//
// Work split: a tensor is cut into chunks of STEGO_STATS_CHUNK = 4096 elements; workgroup b of 256 threads takes chunks b, b + grid, ...
// of the first tensor, then of the second, and so on, so that at any time its LDS histograms belong to one tensor.  The grid is the
// largest chunk count of the call's tensors (at most STEGO_STATS_MAX_GRID): at the trainer's shapes (B * S^4 and neg_samples * B * S^4
// values, 115 and 572 chunks at B = 32) every workgroup reads at most one chunk of each tensor.
//
// Alignment: neg_inter_cd is cd[2:].flatten(0, 1), a view at an element offset.  Chunk starts are multiples of 16 KB inside a tensor, so a
// tensor whose base is 16-byte aligned moves one float4 per lane and round and finishes its last count % 4 elements one lane each; any
// other tensor moves one float per lane and round.  Both paths run the same per-element code.
//
// Exactness: every compare is an integer compare of ORDERED KEYS (the bits of a float mapped so that the integer order is the float
// order, -0.0 and +0.0 on the same key); the 1549 thresholds are a compile-time table of such keys, copied to LDS.  The bucket of a
// value is a guess from its exponent and mantissa bits (a piecewise-linear log2, off by at most one bucket) that two loops then move until
// key[j] <= key(x) < key[j + 1]: the guess only decides how many steps they take, never the answer.
//
// The histogram: cd values of a trained model sit in a few dozen buckets, so the lanes of a wave mostly agree.  Every wave has its own
// 1548 uint32 counters in LDS (no contention between waves), and per 64 values a wave first adds per distinct bucket (confusion.hip's
// wave_count: the first pending lane's bucket goes to every lane, a ballot finds the lanes that hold it, one lane adds their number) for
// at most AGG_ROUNDS buckets; lanes still pending then add for themselves.  One bucket holding everything costs one add per 64 values,
// a spread over hundreds of buckets costs AGG_ROUNDS scalar rounds and then nearly conflict-free adds.  After a tensor's last chunk the
// workgroup adds its non-zero counters onto the call's gathering area in the workspace with 32-bit global atomics.
//
// Sums: every thread adds its values in the order it reads them, in fp64 (the square by an fp64 fma of the exactly converted value);
// block_fold folds a workgroup in one fixed tree (a butterfly per wave, the waves in order); thread 0 stores the workgroup's partial.  After the ticket (release before it, acquire
// in the workgroup that draws the last one) that workgroup folds the partials of all workgroups in index order through the same tree,
// writes the record, moves the gathered counts into the slot with atomic exchanges that leave zeros behind, and advances the step.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/stego_stats.h"
#include "host_util.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int CHUNK = STEGO_STATS_CHUNK;
constexpr int ROUNDS4 = CHUNK / (4 * TPB);         // float4 per lane and chunk
constexpr int ROUNDS1 = CHUNK / TPB;               // floats per lane and chunk on the 4-byte path
constexpr int NB = STEGO_STATS_BUCKETS;
constexpr int NL = STEGO_STATS_LIMITS;
constexpr int MAXT = STEGO_STATS_MAX_TENSORS;
constexpr int MAXS = STEGO_STATS_MAX_SCALARS;
constexpr int MAXG = STEGO_STATS_MAX_GRID;
constexpr int AGG_ROUNDS = 4;
constexpr int HALF = (NL - 1) / 2;                 // 774 limits on either side of 0
static_assert(CHUNK == 16 * TPB && MAXG % TPB == 0 && NL == 2 * HALF + 1 && NB == NL - 1, "the loops below assume this");

// ---- the edges, at compile time: the same table on the host (stego_step_stats_edges) and on the device
struct Edges {
    double limit[NL];
    float thr[NL];
    int key[NL];
    int n_pos;                                     // how many limits the loop made (HALF, checked below)
};

constexpr int ordered_key(uint32_t bits)
{
    // float order as integer order: non-negative floats keep their bits, negative ones count down from 0 (so -0.0 == +0.0 == 0)
    return (bits >> 31) ? (int)(0u - (bits & 0x7fffffffu)) : (int)bits;
}

constexpr float ceil_f32(double d)                 // the smallest float32 >= d (d != 0, far from the ends of the float range)
{
    float f = (float)d;
    if ((double)f < d) {
        const uint32_t b = __builtin_bit_cast(uint32_t, f);
        f = __builtin_bit_cast(float, f > 0.f ? b + 1u : b - 1u);
    }
    return f;
}

constexpr Edges make_edges()
{
    Edges e{};
    double pos[HALF + 8] = {};
    int n = 0;
    for (double v = 1e-12; v < 1e20 && n < HALF + 8; v *= 1.1) pos[n++] = v;
    e.n_pos = n;
    for (int i = 0; i < HALF; ++i) {
        e.limit[HALF - 1 - i] = -pos[i];
        e.limit[HALF + 1 + i] = pos[i];
    }
    e.limit[HALF] = 0.0;
    for (int i = 0; i < NL; ++i) {
        e.thr[i] = i == HALF ? 0.f : ceil_f32(e.limit[i]);
        e.key[i] = ordered_key(__builtin_bit_cast(uint32_t, e.thr[i]));
    }
    return e;
}

constexpr Edges EDGES = make_edges();
static_assert(EDGES.n_pos == HALF, "TensorBoard's loop makes 774 positive limits");

struct KeyTable {
    int key[NL];
};
constexpr KeyTable make_keys()
{
    KeyTable k{};
    for (int i = 0; i < NL; ++i) k.key[i] = EDGES.key[i];
    return k;
}
__device__ const KeyTable D_KEYS = make_keys();

// the bucket guess: log2|x| ~ bits * 2^-23 - 127 (never above the true value, at most 0.086 below), position = (log2|x| - log2 1e-12) / log2 1.1
constexpr float LOG2_STEP = 0.13750352374993502f;                        // log2(1.1)
constexpr float GUESS_A = 1.1920928955078125e-07f / LOG2_STEP;           // 2^-23 / log2(1.1)
constexpr float GUESS_B = (127.f - 39.863137138648355f) / LOG2_STEP - 0.3f;      // ... centred on the approximation's error

// ---- workspace: per-workgroup partials (tensor-major, MAXG per tensor) and the gathering area of the bucket counts
struct WsPlan {
    size_t sum, sum_sq, n_finite, n_nan, n_out, kmin, kmax, hist, bytes;
};
inline WsPlan ws_plan()
{
    stego::WsLayout l;
    WsPlan w;
    w.sum = l.take(sizeof(double) * MAXT * MAXG, 16);
    w.sum_sq = l.take(sizeof(double) * MAXT * MAXG, 16);
    w.n_finite = l.take(sizeof(uint32_t) * MAXT * MAXG, 16);
    w.n_nan = l.take(sizeof(uint32_t) * MAXT * MAXG, 16);
    w.n_out = l.take(sizeof(uint32_t) * MAXT * MAXG, 16);
    w.kmin = l.take(sizeof(int) * MAXT * MAXG, 16);
    w.kmax = l.take(sizeof(int) * MAXT * MAXG, 16);
    w.hist = l.take(sizeof(uint32_t) * MAXT * NB, 16);
    w.bytes = l.total(16);
    return w;
}

struct State {
    long long step;
    unsigned ticket;
    unsigned reserved;
};
static_assert(sizeof(State) == 16, "include/stego_stats.h says 16 bytes");

struct RecordLayout {
    int32_t bytes, step, with_hist, n_tensors, tensors, tensor_stride, scalars, hist, hist_stride;
};
// a tensor's block of the record
constexpr int T_N_FINITE = 0, T_N_NAN = 8, T_N_OUT = 16, T_SUM = 24, T_SUM_SQ = 32, T_MIN = 40, T_MAX = 44, T_BYTES = 48;

inline RecordLayout record_layout(int n_tensors, int n_scalars)
{
    stego::WsLayout l;
    RecordLayout r;
    r.step = (int32_t)l.take(8, 8);
    r.with_hist = (int32_t)l.take(4, 4);
    r.n_tensors = (int32_t)l.take(4, 4);
    r.tensors = (int32_t)l.take((size_t)T_BYTES * n_tensors, 8);
    r.tensor_stride = T_BYTES;
    r.scalars = (int32_t)l.take(sizeof(float) * n_scalars, 4);
    r.hist = (int32_t)l.take(sizeof(uint32_t) * NB * n_tensors, 8);
    r.hist_stride = (int32_t)(sizeof(uint32_t) * NB);
    r.bytes = (int32_t)l.total(16);
    return r;
}

struct StatsParams {
    const float* tensor[MAXT];
    long long count[MAXT];
    const uint32_t* scalar[MAXS];
    char* ring;
    State* state;
    double* ws_sum;                // the workspace's regions (ws_plan)
    double* ws_sum_sq;
    unsigned* ws_fin;
    unsigned* ws_nan;
    unsigned* ws_out;
    int* ws_kmin;
    int* ws_kmax;
    unsigned* ws_hist;
    RecordLayout rec;
    int32_t n_tensors, n_scalars, with_hist, ring_slots;
};

struct Acc {
    double sum, sum_sq;
    unsigned n_finite, n_nan, n_out;
    int kmin, kmax;
};

// One add per distinct bucket of the wave for the first AGG_ROUNDS distinct buckets, one add per lane after that.  Every lane of the
// wave calls this (converged); bucket < 0: the lane counts nothing.
__device__ inline void wave_count(unsigned* hist, int bucket, int lane)
{
    unsigned long long pending = __ballot(bucket >= 0);
    for (int r = 0; r < AGG_ROUNDS && pending; ++r) {
        const int lead = __builtin_amdgcn_readfirstlane(__builtin_ctzll(pending));
        const int k = __builtin_amdgcn_readlane(bucket, lead);
        const unsigned long long same = __ballot(bucket == k);
        if (lane == lead) atomicAdd(hist + k, (unsigned)__popcll(same));
        pending &= ~same;
    }
    if ((pending >> lane) & 1ull) atomicAdd(hist + bucket, 1u);
}

// keys[j] <= key < keys[j + 1] for a key inside [keys[0], keys[NL - 1])
__device__ inline int find_bucket(const int* keys, uint32_t bits, int key)
{
    const float pos = (float)(bits & 0x7fffffffu) * GUESS_A - GUESS_B;
    int p = (int)floorf(pos);
    p = p < -1 ? -1 : p > HALF - 1 ? HALF - 1 : p;
    int j = (bits >> 31) ? HALF - 2 - p : HALF + 1 + p;
    j = j < 0 ? 0 : j > NB - 1 ? NB - 1 : j;
    while (key < keys[j]) --j;                 // key >= keys[0]: stops at 0 at the latest
    while (key >= keys[j + 1]) ++j;            // key < keys[NL - 1]: stops at NB - 1 at the latest
    return j;
}

__device__ inline void take(float x, bool valid, bool with_hist, Acc& a, const int* keys, int key_lo, int key_hi, unsigned* hist, int lane)
{
    int bucket = -1;
    if (valid) {
        const uint32_t bits = __float_as_uint(x), mag = bits & 0x7fffffffu;
        if (mag > 0x7f800000u) {
            ++a.n_nan;
        } else if (mag == 0x7f800000u) {
            ++a.n_out;
        } else {
            const int key = ordered_key(bits);
            const double d = (double)x;
            ++a.n_finite;
            a.sum += d;
            a.sum_sq = fma(d, d, a.sum_sq);
            a.kmin = key < a.kmin ? key : a.kmin;
            a.kmax = key > a.kmax ? key : a.kmax;
            if (key < key_lo || key >= key_hi) ++a.n_out;
            else if (with_hist) bucket = find_bucket(keys, bits, key);
        }
    }
    if (with_hist) wave_count(hist, bucket, lane);      // (workgroup-uniform: every lane of the wave is here)
}

// The chunks of one tensor that this workgroup reads.  A chunk is GROUPS rounds of four values per lane, all loaded before the first is
// used, then taken by ONE rolled loop whose body holds the per-value code four times: the kernel runs every instruction a few times per
// workgroup, so its time is the time to fetch its code, and a fully unrolled chunk (66 copies of the per-value code) was twice as slow
// as the three .mean() launches it replaces.  Round r of the 16-byte path is the float4 at index r * TPB + tid, the extra last round the
// one-by-one tail; round r of the 4-byte path is elements (4 r + j) * TPB + tid, j = 0 .. 3.
__device__ inline void read_tensor(const float* base, long long count, bool with_hist, Acc& a, const int* keys, unsigned* hist)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int key_lo = keys[0], key_hi = keys[NL - 1];
    const bool wide = (reinterpret_cast<uintptr_t>(base) & 15) == 0;
    const long long n_chunks = (count + CHUNK - 1) / CHUNK;
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const long long off = c * CHUNK;
        const int n = (int)(count - off < CHUNK ? count - off : CHUNK);
        const float* const P = base + off;
        const int q = n >> 2;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 v0 = zero, v1 = zero, v2 = zero, v3 = zero, v4 = zero;
        if (wide) {
            const float4* const P4 = reinterpret_cast<const float4*>(P);
            if (tid < q) v0 = P4[tid];
            if (TPB + tid < q) v1 = P4[TPB + tid];
            if (2 * TPB + tid < q) v2 = P4[2 * TPB + tid];
            if (3 * TPB + tid < q) v3 = P4[3 * TPB + tid];
            if (4 * q + tid < n) v4.x = P[4 * q + tid];
        } else {
#define STEGO_STATS_LOAD4(v, r)                                                  \
            if ((4 * (r) + 0) * TPB + tid < n) v.x = P[(4 * (r) + 0) * TPB + tid];   \
            if ((4 * (r) + 1) * TPB + tid < n) v.y = P[(4 * (r) + 1) * TPB + tid];   \
            if ((4 * (r) + 2) * TPB + tid < n) v.z = P[(4 * (r) + 2) * TPB + tid];   \
            if ((4 * (r) + 3) * TPB + tid < n) v.w = P[(4 * (r) + 3) * TPB + tid];
            STEGO_STATS_LOAD4(v0, 0)
            STEGO_STATS_LOAD4(v1, 1)
            STEGO_STATS_LOAD4(v2, 2)
            STEGO_STATS_LOAD4(v3, 3)
#undef STEGO_STATS_LOAD4
        }
        const int rounds = wide && (n & 3) ? ROUNDS4 + 1 : ROUNDS4;
#pragma unroll 1
        for (int r = 0; r < rounds; ++r) {
            bool ok0, ok1, ok2, ok3;
            if (wide) {
                ok0 = r < ROUNDS4 ? r * TPB + tid < q : 4 * q + tid < n;
                ok1 = ok2 = ok3 = r < ROUNDS4 && ok0;
            } else {
                ok0 = (4 * r + 0) * TPB + tid < n;
                ok1 = (4 * r + 1) * TPB + tid < n;
                ok2 = (4 * r + 2) * TPB + tid < n;
                ok3 = (4 * r + 3) * TPB + tid < n;
            }
            take(v0.x, ok0, with_hist, a, keys, key_lo, key_hi, hist, lane);
            take(v0.y, ok1, with_hist, a, keys, key_lo, key_hi, hist, lane);
            take(v0.z, ok2, with_hist, a, keys, key_lo, key_hi, hist, lane);
            take(v0.w, ok3, with_hist, a, keys, key_lo, key_hi, hist, lane);
            v0 = v1;
            v1 = v2;
            v2 = v3;
            v3 = v4;
        }
    }
}

// A workgroup's Acc folded into thread 0's copy: the same butterfly in every lane of a wave (fp adds commute, so every lane holds the
// same bits), the four waves' results through `stage` in wave order.  One fixed tree; two barriers.
struct Stage {
    double sum[WAVES], sum_sq[WAVES];
    unsigned n_finite[WAVES], n_nan[WAVES], n_out[WAVES];
    int kmin[WAVES], kmax[WAVES];
};

__device__ inline Acc block_fold(Acc a, Stage* stage)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        a.sum += __shfl_xor(a.sum, m);
        a.sum_sq += __shfl_xor(a.sum_sq, m);
        a.n_finite += __shfl_xor(a.n_finite, m);
        a.n_nan += __shfl_xor(a.n_nan, m);
        a.n_out += __shfl_xor(a.n_out, m);
        const int lo = __shfl_xor(a.kmin, m), hi = __shfl_xor(a.kmax, m);
        a.kmin = lo < a.kmin ? lo : a.kmin;
        a.kmax = hi > a.kmax ? hi : a.kmax;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        stage->sum[w] = a.sum;
        stage->sum_sq[w] = a.sum_sq;
        stage->n_finite[w] = a.n_finite;
        stage->n_nan[w] = a.n_nan;
        stage->n_out[w] = a.n_out;
        stage->kmin[w] = a.kmin;
        stage->kmax[w] = a.kmax;
    }
    __syncthreads();
    Acc t{stage->sum[0], stage->sum_sq[0], stage->n_finite[0], stage->n_nan[0], stage->n_out[0], stage->kmin[0], stage->kmax[0]};
#pragma unroll
    for (int i = 1; i < WAVES; ++i) {
        t.sum += stage->sum[i];
        t.sum_sq += stage->sum_sq[i];
        t.n_finite += stage->n_finite[i];
        t.n_nan += stage->n_nan[i];
        t.n_out += stage->n_out[i];
        t.kmin = stage->kmin[i] < t.kmin ? stage->kmin[i] : t.kmin;
        t.kmax = stage->kmax[i] > t.kmax ? stage->kmax[i] : t.kmax;
    }
    __syncthreads();                             // the stage may be written again
    return t;
}

__device__ inline float key_to_float(int key)
{
    return __uint_as_float(key >= 0 ? (uint32_t)key : (0x80000000u | (0u - (uint32_t)key)));
}

__global__ __launch_bounds__(TPB) void step_stats_kernel(StatsParams p)
{
    __shared__ int keys[NL];
    __shared__ unsigned hist[WAVES * NB];
    __shared__ Stage stage;
    __shared__ int last;
    const int tid = threadIdx.x;
    const bool with_hist = p.with_hist != 0;
    for (int i = tid; i < NL; i += TPB) keys[i] = D_KEYS.key[i];
    if (with_hist)
        for (int i = tid; i < WAVES * NB; i += TPB) hist[i] = 0u;
    __syncthreads();

    double* const ws_sum = p.ws_sum;
    double* const ws_sum_sq = p.ws_sum_sq;
    unsigned* const ws_fin = p.ws_fin;
    unsigned* const ws_nan = p.ws_nan;
    unsigned* const ws_out = p.ws_out;
    int* const ws_kmin = p.ws_kmin;
    int* const ws_kmax = p.ws_kmax;
    unsigned* const ws_hist = p.ws_hist;
    unsigned* const my_hist = hist + (tid >> 6) * NB;

    for (int t = 0; t < p.n_tensors; ++t) {
        Acc a{0.0, 0.0, 0u, 0u, 0u, INT32_MAX, INT32_MIN};
        read_tensor(p.tensor[t], p.count[t], with_hist, a, keys, my_hist);
        const Acc w = block_fold(a, &stage);          // (its barriers are behind every wave's last add to its counters)
        const int slot = t * MAXG + blockIdx.x;
        if (tid == 0) {
            ws_sum[slot] = w.sum;
            ws_sum_sq[slot] = w.sum_sq;
            ws_fin[slot] = w.n_finite;
            ws_nan[slot] = w.n_nan;
            ws_out[slot] = w.n_out;
            ws_kmin[slot] = w.kmin;
            ws_kmax[slot] = w.kmax;
        }
        if (with_hist && p.count[t] > (long long)blockIdx.x * CHUNK) {      // (a workgroup without a chunk of this tensor counted nothing)
            for (int i = tid; i < NB; i += TPB) {
                unsigned v = 0u;
#pragma unroll
                for (int k = 0; k < WAVES; ++k) {
                    v += hist[k * NB + i];
                    hist[k * NB + i] = 0u;
                }
                if (v) atomicAdd(ws_hist + t * NB + i, v);
            }
            __syncthreads();
        }
    }

    // publish: every wave's stores and atomics have left, then one lane releases and draws the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned drawn = __hip_atomic_fetch_add(&p.state->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = drawn == gridDim.x - 1 ? 1 : 0;
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // the last workgroup: fold, write the record, move the counts, advance the step
    const long long step = p.state->step;                      // written by the last workgroup of the launch before only
    const long long slot_of_step = step % p.ring_slots;         // (a state that was never zeroed must not lead outside the ring)
    char* const rec = p.ring + (size_t)(slot_of_step < 0 ? slot_of_step + p.ring_slots : slot_of_step) * (size_t)p.rec.bytes;
    const int grid = (int)gridDim.x;
    for (int t = 0; t < p.n_tensors; ++t) {
        Acc a{0.0, 0.0, 0u, 0u, 0u, INT32_MAX, INT32_MIN};
        for (int b = tid; b < grid; b += TPB) {                // index order per thread, then the tree
            const int slot = t * MAXG + b;
            a.sum += __hip_atomic_load(ws_sum + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.sum_sq += __hip_atomic_load(ws_sum_sq + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.n_finite += __hip_atomic_load(ws_fin + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.n_nan += __hip_atomic_load(ws_nan + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.n_out += __hip_atomic_load(ws_out + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int lo = __hip_atomic_load(ws_kmin + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int hi = __hip_atomic_load(ws_kmax + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.kmin = lo < a.kmin ? lo : a.kmin;
            a.kmax = hi > a.kmax ? hi : a.kmax;
        }
        const Acc w = block_fold(a, &stage);
        char* const tb = rec + p.rec.tensors + t * p.rec.tensor_stride;
        if (tid == 0) {
            *reinterpret_cast<long long*>(tb + T_N_FINITE) = (long long)w.n_finite;
            *reinterpret_cast<long long*>(tb + T_N_NAN) = (long long)w.n_nan;
            *reinterpret_cast<long long*>(tb + T_N_OUT) = (long long)w.n_out;
            *reinterpret_cast<double*>(tb + T_SUM) = w.sum;
            *reinterpret_cast<double*>(tb + T_SUM_SQ) = w.sum_sq;
            *reinterpret_cast<float*>(tb + T_MIN) = w.n_finite ? key_to_float(w.kmin) : __uint_as_float(0x7f800000u);
            *reinterpret_cast<float*>(tb + T_MAX) = w.n_finite ? key_to_float(w.kmax) : __uint_as_float(0xff800000u);
        }
        if (with_hist) {
            unsigned* const out = reinterpret_cast<unsigned*>(rec + p.rec.hist + (size_t)t * p.rec.hist_stride);
            for (int i = tid; i < NB; i += TPB) out[i] = atomicExch(ws_hist + t * NB + i, 0u);      // ... and zero for the next call
        }
    }
    if (tid < p.n_scalars) reinterpret_cast<uint32_t*>(rec + p.rec.scalars)[tid] = *p.scalar[tid];      // bit for bit
    if (tid == 0) {
        *reinterpret_cast<long long*>(rec + p.rec.step) = step;
        *reinterpret_cast<int32_t*>(rec + p.rec.with_hist) = p.with_hist;
        *reinterpret_cast<int32_t*>(rec + p.rec.n_tensors) = p.n_tensors;
        p.state->step = step + 1;
        __hip_atomic_store(&p.state->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

using stego::aligned;
using stego::hip_rc;

// the descriptor alone
int check(const StegoStatsDesc* d)
{
    if (!d) return STEGO_ERR_NULL;
    if (d->n_tensors < 1 || d->n_tensors > MAXT || d->n_scalars < 0 || d->n_scalars > MAXS) return STEGO_ERR_STATS_COUNT;
    for (int t = 0; t < d->n_tensors; ++t)
        if (d->counts[t] < 0 || d->counts[t] >= STEGO_STATS_MAX_ELEMS) return STEGO_ERR_STATS_COUNT;
    if (d->ring_slots < 1 || d->ring_slots > STEGO_STATS_MAX_SLOTS) return STEGO_ERR_STATS_RING;
    if (d->with_hist != 0 && d->with_hist != 1) return STEGO_ERR_STATS_FLAGS;
    return STEGO_OK;
}

int32_t grid_for(const StegoStatsDesc* d)
{
    int64_t chunks = 1;
    for (int t = 0; t < d->n_tensors; ++t) {
        const int64_t c = (d->counts[t] + CHUNK - 1) / CHUNK;
        chunks = c > chunks ? c : chunks;
    }
    return (int32_t)(chunks < MAXG ? chunks : MAXG);
}

}  // namespace

extern "C" int stego_step_stats_edges(double* limits, float* thresholds)
{
    for (int i = 0; i < NL; ++i) {
        if (limits) limits[i] = EDGES.limit[i];
        if (thresholds) thresholds[i] = EDGES.thr[i];
    }
    return STEGO_OK;
}

extern "C" int stego_step_stats_plan(const StegoStatsDesc* desc, StegoStatsPlan* plan)
{
    if (!plan) return STEGO_ERR_NULL;
    const int rc = check(desc);
    if (rc != STEGO_OK) return rc;
    const RecordLayout r = record_layout(desc->n_tensors, desc->n_scalars);
    StegoStatsPlan q{};
    q.grid = grid_for(desc);
    q.chunk = CHUNK;
    q.record_bytes = r.bytes;
    q.off_step = r.step;
    q.off_with_hist = r.with_hist;
    q.off_n_tensors = r.n_tensors;
    q.off_tensors = r.tensors;
    q.tensor_stride = r.tensor_stride;
    q.t_n_finite = T_N_FINITE;
    q.t_n_nan = T_N_NAN;
    q.t_n_out = T_N_OUT;
    q.t_sum = T_SUM;
    q.t_sum_sq = T_SUM_SQ;
    q.t_min = T_MIN;
    q.t_max = T_MAX;
    q.off_scalars = r.scalars;
    q.off_hist = r.hist;
    q.hist_stride = r.hist_stride;
    q.ring_bytes = (int64_t)r.bytes * desc->ring_slots;
    q.state_bytes = sizeof(State);
    q.workspace_bytes = (int64_t)ws_plan().bytes;
    *plan = q;
    return STEGO_OK;
}

extern "C" int stego_step_stats(const StegoStatsDesc* desc, const float* const* tensors, const float* const* scalars, void* ring,
                                void* state, void* workspace, stego_stream_t stream)
{
    if (!desc || !tensors || !ring || !state || !workspace) return STEGO_ERR_NULL;
    if (desc->n_scalars > 0 && !scalars) return STEGO_ERR_NULL;
    const int rc = check(desc);
    if (rc != STEGO_OK) return rc;
    for (int t = 0; t < desc->n_tensors; ++t)
        if (desc->counts[t] > 0 && !tensors[t]) return STEGO_ERR_NULL;
    for (int s = 0; s < desc->n_scalars; ++s)
        if (!scalars[s]) return STEGO_ERR_NULL;
    if (!aligned(ring, 8) || !aligned(state, 8) || !aligned(workspace, 8)) return STEGO_ERR_ALIGN;
    for (int t = 0; t < desc->n_tensors; ++t)
        if (!aligned(tensors[t], 4)) return STEGO_ERR_ALIGN;
    for (int s = 0; s < desc->n_scalars; ++s)
        if (!aligned(scalars[s], 4)) return STEGO_ERR_ALIGN;

    StatsParams p{};
    for (int t = 0; t < desc->n_tensors; ++t) {
        p.tensor[t] = tensors[t];
        p.count[t] = desc->counts[t];
    }
    for (int s = 0; s < desc->n_scalars; ++s) p.scalar[s] = reinterpret_cast<const uint32_t*>(scalars[s]);
    p.ring = static_cast<char*>(ring);
    p.state = static_cast<State*>(state);
    const WsPlan w = ws_plan();
    p.ws_sum = stego::at<double>(workspace, w.sum);
    p.ws_sum_sq = stego::at<double>(workspace, w.sum_sq);
    p.ws_fin = stego::at<unsigned>(workspace, w.n_finite);
    p.ws_nan = stego::at<unsigned>(workspace, w.n_nan);
    p.ws_out = stego::at<unsigned>(workspace, w.n_out);
    p.ws_kmin = stego::at<int>(workspace, w.kmin);
    p.ws_kmax = stego::at<int>(workspace, w.kmax);
    p.ws_hist = stego::at<unsigned>(workspace, w.hist);
    p.rec = record_layout(desc->n_tensors, desc->n_scalars);
    p.n_tensors = desc->n_tensors;
    p.n_scalars = desc->n_scalars;
    p.with_hist = desc->with_hist;
    p.ring_slots = desc->ring_slots;
    return hip_rc(stego::launch_first<step_stats_kernel>(grid_for(desc), TPB, 0, static_cast<hipStream_t>(stream), p));
}
