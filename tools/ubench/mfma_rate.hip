// Micro-benchmark: how long does ONE fp16 MFMA take?
// (a) v_mfma_f32_32x32x16_f16 in the shapes the fused forward issues it:
//   one MFMA wave per SIMD (4 per workgroup, + 8 waves parked at a barrier as the gather team of a self-correlation tile is),
//   NACC independent accumulator chains, operands from registers (no LDS), N instructions per wave, on G workgroups (1 .. every CU).
// (b) the two 16x16 forms the backward's tile GEMMs can use, v_mfma_f32_16x16x16_f16 (K = 16) and v_mfma_f32_16x16x32_f16 (K = 32):
//   back to back from registers, one or two waves per SIMD (the tile body runs two), NACC accumulator chains, on one workgroup and on
//   every CU; ns per instruction and per FLOP (an instruction is 2 x 16 x 16 x K FLOP).
// Prints ns per MFMA per SIMD from s_memrealtime (100 MHz) inside the kernel and from HIP events around it.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/mfma_rate.hip -o tools/ubench/bin/mfma_rate
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int NACC, bool LDSREAD>
__global__ void __launch_bounds__(768) mfma_kernel(float* sink, unsigned long long* stamps, int iters)
{
    __shared__ __attribute__((aligned(16))) unsigned char lds[32768];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 8192; i += 768) reinterpret_cast<float*>(lds)[i] = (float)(i & 7) * 0.01f;
    __syncthreads();
    if (wave >= 4) { __syncthreads(); return; }          // parked, as a gather team without a gather
    f32x16 acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[a][e] = 0.f;
    f16x8 av, bv;
#pragma unroll
    for (int e = 0; e < 8; ++e) { av[e] = (_Float16)(0.001f * (lane + e)); bv[e] = (_Float16)(0.002f * (lane - e)); }
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
        if constexpr (LDSREAD) {
            // 12 fragment reads + 12 MFMAs: one feature stage of the half kernel
            f16x8 f[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) f[k] = *reinterpret_cast<const f16x8*>(lds + ((k * 1024 + (lane & 31) * 64 + ((lane >> 5) + 2 * (it & 1)) * 16) & 32767));
#pragma unroll
            for (int k = 0; k < 12; ++k) acc[k % NACC] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[k], f[(k + 5) % 12], acc[k % NACC], 0, 0, 0);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) acc[k % NACC] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv, acc[k % NACC], 0, 0, 0);
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < NACC; ++a) s += acc[a][lane & 15];
    if (s == 123.456f) sink[0] = s;
    if (lane == 0) stamps[blockIdx.x * 4 + wave] = t1 - t0;
    __syncthreads();
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

template <int KF, int NACC>         // KF = 16 or 32: the instruction's K
__global__ void __launch_bounds__(512) mfma16_kernel(float* sink, unsigned long long* stamps, int iters, int active)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (wave >= active) return;                           // `active` waves issue: 4 = one per SIMD, 8 = two
    f32x4 acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    f16x8 av, bv;
#pragma unroll
    for (int e = 0; e < 8; ++e) { av[e] = (_Float16)(0.001f * (lane + e)); bv[e] = (_Float16)(0.002f * (lane - e)); }
    const f16x4 a4 = f16x4{av[0], av[1], av[2], av[3]}, b4 = f16x4{bv[0], bv[1], bv[2], bv[3]};
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            if constexpr (KF == 16) acc[k % NACC] = __builtin_amdgcn_mfma_f32_16x16x16f16(a4, b4, acc[k % NACC], 0, 0, 0);
            else acc[k % NACC] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bv, acc[k % NACC], 0, 0, 0);
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < NACC; ++a) s += acc[a][lane & 3];
    if (s == 123.456f) sink[0] = s;
    if (lane == 0) stamps[blockIdx.x * 8 + wave] = t1 - t0;
}

template <int KF, int NACC>
static void run16(int active, int grid, int iters, float* sink, unsigned long long* stamps)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> ms;
    CK(hipMemset(stamps, 0, (size_t)grid * 8 * 8));
    for (int r = 0; r < 6; ++r) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((mfma16_kernel<KF, NACC>), dim3(grid), dim3(512), 0, 0, sink, stamps, iters, active);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float t;
        CK(hipEventElapsedTime(&t, e0, e1));
        if (r > 1) ms.push_back(t);
    }
    std::vector<unsigned long long> all((size_t)grid * 8), h;
    CK(hipMemcpy(all.data(), stamps, all.size() * 8, hipMemcpyDeviceToHost));
    for (int g = 0; g < grid; ++g)
        for (int w = 0; w < active; ++w) h.push_back(all[(size_t)g * 8 + w]);
    std::sort(h.begin(), h.end());
    std::sort(ms.begin(), ms.end());
    // a SIMD issues for active / 4 waves: time per instruction on the SIMD = wave time / (instructions of its waves)
    const double n = 12.0 * iters * (active / 4);
    const double ns = h[h.size() / 2] * 10.0 / n, flop = 2.0 * 16 * 16 * KF;
    printf("v_mfma_f32_16x16x%d_f16, %d chains, %d wave(s)/SIMD  grid %3d: %6.2f ns per MFMA per SIMD (median wave; slowest %6.2f), %7.3f ps per FLOP, kernel by events %7.1f us\n",
           KF, NACC, active / 4, grid, ns, h.back() * 10.0 / n, ns * 1e3 / flop, ms[ms.size() / 2] * 1e3);
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
}

template <int NACC, bool L>
static void run(const char* name, int grid, int iters, float* sink, unsigned long long* stamps)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> ms;
    std::vector<unsigned long long> h((size_t)grid * 4);
    for (int r = 0; r < 6; ++r) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((mfma_kernel<NACC, L>), dim3(grid), dim3(768), 0, 0, sink, stamps, iters);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float t;
        CK(hipEventElapsedTime(&t, e0, e1));
        if (r > 1) ms.push_back(t);
    }
    CK(hipMemcpy(h.data(), stamps, h.size() * 8, hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end());
    std::sort(ms.begin(), ms.end());
    const double n = 12.0 * iters;
    printf("%-44s grid %3d: in-kernel %6.1f ns per MFMA (median wave; slowest %6.1f), kernel by events %7.1f us\n", name, grid,
           h[h.size() / 2] * 10.0 / n, h.back() * 10.0 / n, ms[ms.size() / 2] * 1e3);
}

int main()
{
    float* sink; unsigned long long* stamps;
    CK(hipMalloc(&sink, 64)); CK(hipMalloc(&stamps, 1024 * 8 * 8));
    // ---- the 16x16 forms of the backward's tile GEMMs (a tile wave issues 60 .. 120 per GEMM on 5 chains)
    for (int iters : {10, 1000}) {
        printf("---- 16x16 forms: %d x 12 MFMAs per wave, operands in registers\n", iters);
        for (int grid : {1, 256})
            for (int active : {4, 8}) {
                run16<16, 1>(active, grid, iters, sink, stamps);
                run16<32, 1>(active, grid, iters, sink, stamps);
                run16<16, 4>(active, grid, iters, sink, stamps);
                run16<32, 4>(active, grid, iters, sink, stamps);
            }
    }
    for (int iters : {15, 150, 1500}) {
        printf("---- %d stages of 12 MFMAs per wave\n", iters);
        for (int grid : {1, 8, 256}) {
            run<2, false>("registers, 2 chains", grid, iters, sink, stamps);
            run<4, false>("registers, 4 chains", grid, iters, sink, stamps);
            run<2, true>("12 ds_read_b128 + 12 MFMA per stage, 2 chains", grid, iters, sink, stamps);
            run<4, true>("12 ds_read_b128 + 12 MFMA per stage, 4 chains", grid, iters, sink, stamps);
        }
    }
    return 0;
}
