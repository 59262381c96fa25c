// Every host function that one translation unit of the library defines and another calls (corr_wide.h has the wide path's own).  The
// defining unit and the callers include this header, so a signature that drifts fails where it is compiled, not when the library is loaded.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/stego_corr.h"
#include "corr_bwd_plan.h"
#include "corr_common.h"

namespace stego {

// corr_sample.hip, corr_fwd.hip
hipError_t launch_corr_sample(const SampleParams& prm, int precision, hipStream_t stream);
hipError_t launch_corr_tile(const CorrParams& prm, int precision, hipStream_t stream);
hipError_t launch_corr_finalize(const CorrParams& prm, hipStream_t stream);
// corr_fused.hip, and the launch functions of its sibling units (corr_fused_odd.hip, corr_fused_c192.hip, corr_fused_half.hip)
bool fused_supported(const FusedParams& prm, int precision);
hipError_t launch_corr_fused(const FusedParams& prm, int precision, size_t sync_bytes, bool prepared, bool shared_device, hipStream_t stream,
                             hipEvent_t* ev /* null or [4]: before the memset, before / after the kernel, end */);
hipError_t prepare_corr_fused(const FusedParams& prm, size_t sync_bytes, hipStream_t stream);
hipError_t launch_fused_odd(const FusedParams& prm, int precision, dim3 grid, dim3 block, int lds, hipStream_t stream);
hipError_t launch_fused_c192(const FusedParams& prm, int precision, dim3 grid, dim3 block, int lds, hipStream_t stream);
hipError_t launch_fused_half(const FusedParams& prm, int precision, hipStream_t stream);
// corr_bwd.hip: plans the backward (corr_bwd_plan.h) and launches it; corr_bwd_lists.hip: the launches of a lists-first plan
hipError_t launch_corr_bwd(const BwdParams& prm, hipStream_t stream);
hipError_t launch_corr_bwd_lists(const BwdParams& prm, const BwdPlan& plan, hipStream_t stream);
// draws.hip
hipError_t launch_fast_draws(const long long* seed, long long n_coord, int n_neg, int B, float* c1, float* c2, long long* perms,
                             hipStream_t stream);
hipError_t launch_finish_draws(const float* u1, const float* u2, long long n_coord, const long long* const* raw, int n_neg,
                               int B, float* c1, float* c2, long long* perms, hipStream_t stream);
hipError_t launch_ref_draws(unsigned long long seed, unsigned long long offset, const long long* seed_ptr, const long long* offset_ptr,
                            int variant, long long n_coord, int n_neg, int B,
                            int cus, int threads_per_cu, float* c1, float* c2, long long* perms, hipStream_t stream);
unsigned long long ref_draws_advance(long long n_coord, int n_neg, int B, int variant, int cus, int threads_per_cu);
unsigned long long ref_masks_advance(long long numel, int n_masks, int variant, int cus, int threads_per_cu);
hipError_t launch_ref_masks(unsigned long long seed, unsigned long long offset, const long long* seed_ptr, const long long* offset_ptr,
                            int variant, int n_masks, long long numel, float keep_prob, int cus, int threads_per_cu, float* out,
                            hipStream_t stream);
// dense_corr.hip, dense_stream.hip
size_t dense_workspace_bytes(int B, int C, int M, int N);
size_t dense_panel_image_bytes(int C, int P);
// which kernel launch_dense_corr takes for these maps (STEGO_DENSE_*), or -1: none of them is correct there.  debug: knob(KNOB_DEBUG).
// Host arithmetic on strides and dimensions only: no map data is read, nothing is launched.
int dense_corr_kernel(const MapV& a, const MapV& b, int B, int C, int H1, int W1, int H2, int W2, int debug);
hipError_t launch_dense_corr(const MapV& a, const MapV& b, int B, int C, int H1, int W1, int H2, int W2, int normalize,
                             float* out, void* ws, hipStream_t stream);
hipError_t launch_dense_corr_panels(const void* imgA, const float* rsA, int imagesA, const void* imgB, const float* rsB, int B, int C, int M, int N,
                                    float* out, float* rowsum, hipStream_t stream);
hipError_t launch_dense_corr_panels_seg(const void* imgA, const float* rsA, int imagesA, const void* imgB, const float* rsB, int B, int C, int M, int N,
                                        float* out, float* out1, float* out2, int seg, float* rowsum, hipStream_t stream);
hipError_t launch_dense_stream(const MapV& a, const MapV& b, int B, int C, int H1, int W1, int H2, int W2, int normalize, float* out, void* ws,
                               hipStream_t stream);
// loss_pointwise.hip
hipError_t launch_rowsum(const float* x, float* out, long long rows, int P, hipStream_t stream);
// sample_sets.hip
hipError_t launch_sample_panels2(const StegoMap* map, int C, void* panels, float* row_scale, float* rows_out, float* inv_out,
                                 const StegoMap* map2, int C2, void* panels2, float* row_scale2, float* rows_out2, float* inv_out2,
                                 const long long* index, int N, int H, int W, const float* coords, int n_coords, int S, int normalize,
                                 hipStream_t stream);
hipError_t launch_sample_scatter(const float* g_rows, const float* rows_n, const float* inv, const StegoMap* d_map, const long long* index, int N, int C,
                                 int H, int W, const float* coords, int n_coords, int S, const float* extra, int n_extra, long long extra_stride,
                                 hipStream_t stream);
// knn_topk.hip
size_t knn_workspace_bytes(long long N, int D, int k, long long q_count);
hipError_t launch_knn(const float* X, long long N, int D, long long ldx, int k, int normalize, long long q_begin,
                      long long q_count, long long* out_idx, float* out_val, void* ws, hipStream_t stream);

}  // namespace stego
