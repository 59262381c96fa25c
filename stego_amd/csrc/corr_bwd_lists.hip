// Lists first: the training path of the loss backward (forward() semantics, scalar upstreams, maps up to 64 x 64; the dispatch and the
// other paths: corr_bwd.hip; workspace layout and limits: corr_bwd_plan.h).
// corr_bwd_tile_build_kernel (split-fp16 tiles) / corr_bwd_tile32_build_kernel (fp32 tiles) + corr_unsample_list_kernel.  The row kernel
// of corr_bwd.hip spends three dependent load rounds per unit (perms -> items, tap words -> worklist, DT rows) of which only the last needs the
// tile kernel's output.  Here the first two run BESIDE the tiles, in the same launch: with B = 32 the 224 tile workgroups leave 32
// CUs free, and B "builder" workgroups at the front of the grid turn perms + the forward's tap tables into the entry list of every
// (destination, image, pixel row, 16-pixel bin) unit - which DT rows land there, with which weights.  The second launch is then ONE
// wave per unit pair: its lists arrive in one load (fixed slots), every DT row of the unit is in flight at once (16-byte loads), the
// rows are accumulated as one-hot GEMMs on the f32 MFMA in registers, and the pixels leave as 16-byte stores.  One wave per unit, the
// list order fixed by a stable counting sort: no atomics on data, no reduction between waves, bitwise repeatable.
// (A version with the unsample INSIDE the same launch, handing the DT rows over through device counters, was measured slower than the
// kernel boundary it removed: profiles/r04b_bwd_one_launch_attempt.txt.)
#include <type_traits>

#include "corr_bwd_plan.h"
#include "corr_bwd_tile.h"
#include "corr_common.h"
#include "host_util.h"
#include "launchers.h"

namespace stego {

typedef unsigned int bu32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t bf_rsrc(const void* p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// ---- builder role: the entry lists of destination images bi, bi + n_build, ... (dest 0 = orig_code with its anchor and negative
// items, dest 1 = orig_code_pos with its one item, handled together).  A stable counting sort of the (item, point, tap row) sequence
// by list key, in LDS: wave w owns the item halves w, w + 8, ...; counts per (wave, key), a block-wide prefix, then every element
// takes its slot with a returning LDS add on its wave's OWN counter - lanes of one instruction that hit the same counter are
// served in an order the hardware fixes (no other wave touches it), so the lists come out the same launch after launch.
template <int NW>        // waves of the workgroup: 8 beside the split-fp16 tiles, 4 beside the fp32 ones
__device__ __forceinline__ void bwd_builder_role(const BwdParams& prm, const int bi, unsigned char* smem)
{
    int2* items = reinterpret_cast<int2*>(smem + BFS_ITEMS);
    unsigned* hist = reinterpret_cast<unsigned*>(smem + BFS_HIST);
    unsigned* ovf = reinterpret_cast<unsigned*>(smem + BFS_OVF);
    unsigned* scan = reinterpret_cast<unsigned*>(smem + BFS_SCAN);
    int* misc = reinterpret_cast<int*>(smem + BFS_MISC);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int B = prm.B, P = prm.P, H = prm.H, W = prm.W, ldk = prm.LDK;
    const int MT = (W + 15) >> 4;
    const int side_elems = TP * ldk;
    const unsigned EPI = (unsigned)UL_POINT_ENTRIES * (unsigned)P;      // entry slots per item: two rows, at most two bins each
    const unsigned light0 = (unsigned)(B * H * MT) * UL_SLOT0;       // byte offset of the dest-1 slots
    const __amdgpu_buffer_rsrc_t pool = bf_rsrc(prm.upool, prm.upool_bytes);
    const __amdgpu_buffer_rsrc_t slots = bf_rsrc(prm.uslots, prm.uslots_bytes);
    unsigned long long* ts = reinterpret_cast<unsigned long long*>(prm.dt + (size_t)prm.n_sets * B * 2 * side_elems) + 2048 + 2 * bi;
    const bool stamp_on = (prm.debug & BWD_DBG_STAMPS) && tid == 0 && bi < 512;
    if (stamp_on) ts[0] = __builtin_amdgcn_s_memrealtime();
    unsigned* myhist = hist + wave * BF_NKEY;

    for (int j = bi; j < B; j += prm.n_build) {
        __syncthreads();                                     // the previous image's LDS tables are dead
        // ---- items of dest 0 (the anchor's own tiles, then the negatives whose perm picked image j: modules.py:385), then dest 1's one item
        if (wave == 0) {
            const int n_own = prm.n_sets;
            for (int u = lane; u < n_own; u += 64) items[u] = make_int2(j, ((u * B + j) * 2 + 0) * side_elems);
            int n_seen = 0, below = 0;
            const int n_negc = prm.n_neg * B;
            for (int t0 = 0; t0 < n_negc; t0 += 64) {
                const int t = t0 + lane;
                const long long pv = t < n_negc ? prm.perms[t] : -1;
                const bool m = (int)pv == j && t < n_negc;
                const unsigned long long mask = __ballot(m);
                const int s = 2 * B + t;
                if (m) items[n_own + n_seen + lane_prefix(mask)] = make_int2(s, (s * 2 + 1) * side_elems);
                n_seen += __builtin_popcountll(mask);
                below += __builtin_popcountll(__ballot(t < n_negc && (int)pv < j));
            }
            const int n0 = n_own + n_seen;
            if (lane == 0) {
                items[n0] = make_int2(B + j, ((B + j) * 2 + 1) * side_elems);
                misc[0] = n0;
                misc[1] = (int)(EPI * (unsigned)(prm.n_sets * j + below));          // overflow slabs: room for every entry of the image
                misc[2] = (int)(EPI * (unsigned)(prm.n_sets * B + n_negc + j));
            }
        }
        for (int i = tid; i < NW * BF_NKEY; i += (64 * NW)) hist[i] = 0u;
        __syncthreads();
        const int n0 = misc[0], n_ih = 2 * (n0 + 1);         // item halves: 64 points each
        const unsigned slab0 = (unsigned)misc[1], slab1 = (unsigned)misc[2];
        // the (<= 4) list keys of a point: tap rows y0 and y0 + 1 (a clamped lower row carries zero weights: no entry), in each
        // the bin of x0 and - when x0 is the last pixel of its bin - the bin of x0 + 1
        auto point_keys = [&](int dest, int q, int wd, int (&key)[4]) {
            const int y0 = wd >> 16, x0 = wd & 0xffff;
            const int b0 = x0 >> 4, b1 = (x0 & 15) == 15 && b0 + 1 < MT ? b0 + 1 : -1;
            const bool v = q < P;
            const int r0 = (dest * H + y0) * BF_MAXMT, r1 = r0 + BF_MAXMT;
            key[0] = v ? r0 + b0 : -1;
            key[1] = v && b1 >= 0 ? r0 + b1 : -1;
            key[2] = v && y0 + 1 < H ? r1 + b0 : -1;
            key[3] = v && y0 + 1 < H && b1 >= 0 ? r1 + b1 : -1;
        };
        // ---- pass 0: counts per (wave, key)
        for (int ih0 = wave; ih0 < n_ih; ih0 += 4 * NW) {
            int wd[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ih = min(ih0 + u * NW, n_ih - 1), it = ih >> 1, q = (ih & 1) * 64 + lane;
                wd[u] = reinterpret_cast<const int*>(prm.tapyx + (size_t)items[it].x * TP + q)[0];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ih = ih0 + u * NW;
                if (ih < n_ih) {                             // uniform
                    int key[4];
                    point_keys((ih >> 1) >= n0, (ih & 1) * 64 + lane, wd[u], key);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (key[c] >= 0) __hip_atomic_fetch_add(myhist + key[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();
        // ---- prefix: thread t owns the keys t KPT .. t KPT + KPT - 1.  A list's first UL_CAP entries live in the unit's slot, the rest in
        // the image's overflow slab (lists in key order per destination); inside a list the waves come in order
        {
            constexpr int KPT = BF_NKEY / (64 * NW);
            const int kd1 = H * BF_MAXMT;                    // first key of dest 1
            unsigned c[KPT][NW], tot[KPT], over[KPT], osum = 0u;
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const int key = tid * KPT + i;
                tot[i] = 0u;
#pragma unroll
                for (int w = 0; w < NW; ++w) { c[i][w] = hist[w * BF_NKEY + key]; tot[i] += c[i][w]; }
                const unsigned cap = key >= kd1 ? UL_CAP1 : UL_CAP0;
                over[i] = tot[i] > cap ? tot[i] - cap : 0u;
                osum += over[i];
            }
            unsigned inc = osum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = (unsigned)__shfl_up((int)inc, d, 64);
                if (lane >= d) inc += o;
            }
            if (lane == 63) scan[wave] = inc;
            __syncthreads();
            unsigned base = inc - osum;
#pragma unroll
            for (int w = 0; w < NW; ++w) base += w < wave ? scan[w] : 0u;
            unsigned kb[KPT];                                // overflow entries in front of each of my keys
#pragma unroll
            for (int i = 0; i < KPT; ++i) { kb[i] = base; base += over[i]; }
#pragma unroll
            for (int i = 0; i < KPT; ++i)
                if (tid * KPT + i == kd1) scan[NW] = kb[i];  // dest 1's overflow restarts in its own slab
            __syncthreads();
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const int key = tid * KPT + i;
                const bool d1 = key >= kd1;
                const unsigned ostart = d1 ? slab1 + (kb[i] - scan[NW]) : slab0 + kb[i];
                ovf[key] = ostart;
                const int rm = key - (d1 ? kd1 : 0), m = rm & (BF_MAXMT - 1);     // rm = row * BF_MAXMT + bin
                if (key < 2 * kd1 && m < MT) {
                    const unsigned ui = (unsigned)((j * H + (rm >> BF_MAXMT_LOG2)) * MT + m);
                    __builtin_amdgcn_raw_buffer_store_b128(bu32x4{tot[i], ostart, 0u, 0u}, slots, d1 ? light0 + ui * UL_SLOT1 : ui * UL_SLOT0, 0, 0);
                }
                unsigned run = 0u;                           // list-relative running positions per (wave, key)
#pragma unroll
                for (int w = 0; w < NW; ++w) { hist[w * BF_NKEY + key] = run; run += c[i][w]; }
            }
        }
        __syncthreads();
        // ---- pass 1: every element takes its position and leaves its entry {DT row, x0, weight left, weight right}
        const int kd1 = H * BF_MAXMT;
        for (int ih0 = wave; ih0 < n_ih; ih0 += 4 * NW) {
            int wd[4];
            float4 w4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ih = min(ih0 + u * NW, n_ih - 1), it = ih >> 1, q = (ih & 1) * 64 + lane;
                const size_t e = (size_t)items[it].x * TP + q;
                wd[u] = reinterpret_cast<const int*>(prm.tapyx + e)[0];
                w4[u] = prm.tapw[e];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ih = ih0 + u * NW;
                if (ih < n_ih) {                             // uniform
                    const int it = ih >> 1, q = (ih & 1) * 64 + lane;
                    const bool d1 = it >= n0;
                    int key[4];
                    point_keys(d1, q, wd[u], key);
                    bu32x4 ent;
                    ent[0] = (unsigned)(items[it].y + q * ldk);
                    ent[1] = (unsigned)(wd[u] & 0xffff);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (key[c] >= 0) {
                            const unsigned pos = __hip_atomic_fetch_add(myhist + key[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            ent[2] = __builtin_bit_cast(unsigned, c >= 2 ? w4[u].z : w4[u].x);
                            ent[3] = __builtin_bit_cast(unsigned, c >= 2 ? w4[u].w : w4[u].y);
                            const int rm = key[c] - (d1 ? kd1 : 0);
                            const unsigned ui = (unsigned)((j * H + (rm >> BF_MAXMT_LOG2)) * MT + (rm & (BF_MAXMT - 1)));
                            const unsigned cap = d1 ? UL_CAP1 : UL_CAP0;
                            if (pos < cap) __builtin_amdgcn_raw_buffer_store_b128(ent, slots, (d1 ? light0 + ui * UL_SLOT1 : ui * UL_SLOT0) + (unsigned)UL_ENTRY_BYTES * (1u + pos), 0, 0);
                            else __builtin_amdgcn_raw_buffer_store_b128(ent, pool, (ovf[key[c]] + (pos - cap)) * (unsigned)UL_ENTRY_BYTES, 0, 0);
                        }
                }
            }
        }
    }
    if (stamp_on) ts[1] = __builtin_amdgcn_s_memrealtime();
}

template <int NT>
__global__ void __launch_bounds__(HW_THREADS) corr_bwd_tile_build_kernel(const BwdParams prm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int w = blockIdx.x;
    if (w < prm.n_build) bwd_builder_role<HW_WAVES>(prm, w, smem);
    else bwd_tile_h_body<NT, false>(prm, w - prm.n_build, smem);
}

// the same beside the exact-fp32 tiles (F32 mode): 256-thread workgroups, four builder waves
template <int NT>
__global__ void __launch_bounds__(NTHREADS) corr_bwd_tile32_build_kernel(const BwdParams prm)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int w = blockIdx.x;
    if (w < prm.n_build) bwd_builder_role<NTHREADS / 64>(prm, w, smem);
    else bwd_tile_body<NT>(prm, w - prm.n_build, smem);
}

// ---- second launch: wave k takes the pair of units {dest 0, dest 1} x (image, row, bin) k
// Channels: NQ x 64 as 16-byte loads (lane l16 holds channels 64 qd + 4 l16 .. + 3: accumulator tile 4 qd + c is channel 64 qd + 4 l16 + c,
// so a pixel leaves as one 16-byte store per lane), + TAIL 16-channel tiles as 4-byte loads (channel 64 NQ + l16).
template <int NQ, int TAIL>
__global__ void __launch_bounds__(64 * UL_WAVES) corr_unsample_list_kernel(const BwdParams prm)
{
    constexpr int NA = 4 * NQ + TAIL;                        // accumulator tiles
    constexpr int EG0 = (UL_CAP0 + 1) / 4, EG1 = (UL_CAP1 + 1) / 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int B = prm.B, H = prm.H, W = prm.W, K = prm.K, ldk = prm.LDK;
    const int MT = (W + 15) >> 4;
    const int n_pairs = B * H * MT;
    // every unit of image j on XCD j % 8 (block b runs on XCD b % 8: observed, used for speed only): the builder of image j and the tiles
    // of anchor j ran there, and plain stores leave their lines in that L2 across the kernel boundary (measured -1 us per step)
    int k;
    {
        const int upi = H * MT, wpi = (upi + UL_WAVES - 1) / UL_WAVES;
        const int x = blockIdx.x & 7, sl = blockIdx.x >> 3;
        const int j = (sl / wpi) * 8 + x, u = (sl % wpi) * UL_WAVES + wave;
        if (j >= B || u >= upi) return;
        k = j * upi + u;
    }
    if (k >= n_pairs) return;
    const int l16 = lane & 15, k4 = lane >> 4;
    const __amdgpu_buffer_rsrc_t pool = bf_rsrc(prm.upool, prm.upool_bytes);
    const __amdgpu_buffer_rsrc_t slots = bf_rsrc(prm.uslots, prm.uslots_bytes);
    const __amdgpu_buffer_rsrc_t dtr = bf_rsrc(prm.dt, prm.dt_bytes);
    const unsigned light0 = (unsigned)n_pairs * UL_SLOT0;
    unsigned long long* ts = reinterpret_cast<unsigned long long*>(prm.dt + (size_t)prm.n_sets * B * 2 * TP * ldk) + 2 * blockIdx.x;
    const bool stamp_on = (prm.debug & BWD_DBG_STAMPS) && threadIdx.x == 0 && blockIdx.x < 1024;
    if (stamp_on) ts[0] = __builtin_amdgcn_s_memrealtime();
    const int m = k % MT, jr = k / MT;                       // jr = image * H + row

    // both slots in one round: lane 0 the header, lane i entry i - 1
    bu32x4 s0 = __builtin_amdgcn_raw_buffer_load_b128(slots, (unsigned)k * UL_SLOT0 + (unsigned)UL_ENTRY_BYTES * lane, 0, 0);
    bu32x4 s1 = __builtin_amdgcn_raw_buffer_load_b128(slots, light0 + (unsigned)k * UL_SLOT1 + (unsigned)UL_ENTRY_BYTES * (lane & UL_CAP1), 0, 0);
    const unsigned n0 = __builtin_amdgcn_readfirstlane(s0[0]), o0 = __builtin_amdgcn_readfirstlane(s0[1]);
    const unsigned n1 = __builtin_amdgcn_readfirstlane(s1[0]), o1 = __builtin_amdgcn_readfirstlane(s1[1]);

    f32x4 acc[2][NA];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[u][a] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the DT rows of NG groups of 4 entries held by the lanes first .. first + n - 1 of `ent` (group g, lane group k4: entry 4 g + k4)
    struct Rows { f32x4 q[NQ]; float t[TAIL > 0 ? TAIL : 1]; };
    auto issue = [&](const bu32x4& ent, int first, int n, auto& rows, auto ng_tag) {
        constexpr int NG = decltype(ng_tag)::value;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (4 * g < n) {                                  // uniform: groups beyond the list issue nothing
                const int e = min(4 * g + k4, n - 1);
                const unsigned row = (unsigned)__shfl((int)ent[0], first + e, 64);
#pragma unroll
                for (int qd = 0; qd < NQ; ++qd)
                    rows[g].q[qd] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(dtr, (row + 64u * qd + 4u * l16) * 4u, 0, 0));
#pragma unroll
                for (int t = 0; t < TAIL; ++t)
                    rows[g].t[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dtr, (row + (unsigned)min(64 * NQ + 16 * t + l16, ldk - 1)) * 4u, 0, 0));
            }
        }
    };
    auto consume = [&](const bu32x4& ent, int first, int n, auto& rows, f32x4 (&ac)[NA], auto ng_tag) {
        constexpr int NG = decltype(ng_tag)::value;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (4 * g < n) {                                  // uniform
                const int e = min(4 * g + k4, n - 1);
                const int x0 = __shfl((int)ent[1], first + e, 64);
                float wa = __builtin_bit_cast(float, __shfl((int)ent[2], first + e, 64));
                float wb = __builtin_bit_cast(float, __shfl((int)ent[3], first + e, 64));
                if (4 * g + k4 >= n) { wa = 0.f; wb = 0.f; }
                const int dx = 16 * m + l16 - x0;
                const float a = dx == 0 ? wa : (dx == 1 ? wb : 0.f);
#pragma unroll
                for (int qd = 0; qd < NQ; ++qd)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        ac[4 * qd + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, rows[g].q[qd][c], ac[4 * qd + c], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < TAIL; ++t)
                    ac[4 * NQ + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, rows[g].t[t], ac[4 * NQ + t], 0, 0, 0);
            }
        }
    };
    {
        Rows r0[EG0], r1[EG1];
        const int c0 = (int)min(n0, (unsigned)UL_CAP0), c1 = (int)min(n1, (unsigned)UL_CAP1);
        issue(s0, 1, c0, r0, std::integral_constant<int, EG0>());
        issue(s1, 1, c1, r1, std::integral_constant<int, EG1>());
        __builtin_amdgcn_sched_barrier(0);                   // every DT row is in flight before the first use waits
        consume(s0, 1, c0, r0, acc[0], std::integral_constant<int, EG0>());
        consume(s1, 1, c1, r1, acc[1], std::integral_constant<int, EG1>());
    }
    // lists longer than their slot (a few percent of the units at the training shape): 64 entries per round from the overflow slab
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int rest = u ? (int)n1 - UL_CAP1 : (int)n0 - UL_CAP0;
        const unsigned ob = u ? o1 : o0;
        for (int e0 = 0; e0 < rest; e0 += 64) {
            const int n = min(64, rest - e0);
            const bu32x4 ent = __builtin_amdgcn_raw_buffer_load_b128(pool, (ob + (unsigned)(e0 + min(lane, n - 1))) * (unsigned)UL_ENTRY_BYTES, 0, 0);
            Rows r[16];
            issue(ent, 0, n, r, std::integral_constant<int, 16>());
            __builtin_amdgcn_sched_barrier(0);
            consume(ent, 0, n, r, acc[u], std::integral_constant<int, 16>());
        }
    }
    // acc[u][a][reg] is pixel 16 m + 4 k4 + reg of row jr of destination u; channel 64 qd + 4 l16 + c (a = 4 qd + c), 64 NQ + 16 t + l16 (tail)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        float* out = (u == 0 ? prm.d_code : prm.d_code_pos) + (size_t)jr * W * K;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int x = 16 * m + 4 * k4 + reg;
            if (x < W) {
                float* px = out + (size_t)x * K;
#pragma unroll
                for (int qd = 0; qd < NQ; ++qd) {
                    const int ch = 64 * qd + 4 * l16;
                    const f32x4 v = f32x4{acc[u][4 * qd][reg], acc[u][4 * qd + 1][reg], acc[u][4 * qd + 2][reg], acc[u][4 * qd + 3][reg]};
                    if (ch + 3 < K) {
                        typedef f32x4 f32x4_a4 __attribute__((aligned(4)));
                        __builtin_nontemporal_store(v, reinterpret_cast<f32x4_a4*>(px + ch));
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (ch + c < K) __builtin_nontemporal_store(v[c], px + ch + c);
                    }
                }
#pragma unroll
                for (int t = 0; t < TAIL; ++t) {
                    const int ch = 64 * NQ + 16 * t + l16;
                    if (ch < K) __builtin_nontemporal_store(acc[u][4 * NQ + t][reg], px + ch);
                }
            }
        }
    }
    if (stamp_on) ts[1] = __builtin_amdgcn_s_memrealtime();
}

hipError_t launch_corr_bwd_lists(const BwdParams& prm, const BwdPlan& pl, hipStream_t stream)
{
    {
        const dim3 grid(pl.tile.grid), block(pl.tile.block);
        // channel tiles of 16: the split kernel has 1 .. 8 (anything else: 8), its fp32 twin 1 .. 5 (anything else: 5)
        const hipError_t e = pl.split
            ? with_const<1, 2, 3, 4, 5, 6, 7, 8>(pl.nt, [&](auto N) { return launch<corr_bwd_tile_build_kernel<N()>>(grid, block, pl.tile.lds, stream, prm); })
            : with_const<1, 2, 3, 4, 5>(pl.nt, [&](auto N) { return launch<corr_bwd_tile32_build_kernel<N()>>(grid, block, pl.tile.lds, stream, prm); });
        if (e != hipSuccess) return e;
    }
    const dim3 grid(pl.uns.grid), block(pl.uns.block);
    if (pl.nq == 1 && pl.tail == 0) return launch<corr_unsample_list_kernel<1, 0>>(grid, block, pl.uns.lds, stream, prm);
    if (pl.nq == 1) return launch<corr_unsample_list_kernel<1, 1>>(grid, block, pl.uns.lds, stream, prm);
    return launch<corr_unsample_list_kernel<2, 0>>(grid, block, pl.uns.lds, stream, prm);
}

}  // namespace stego
