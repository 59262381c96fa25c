// The launcher of csrc/vit_cls_attn.hip for stego_vit_forward_attn (csrc/vit_forward.hip): the class token's attention row of the block
// whose Q and K the workspace holds.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace stego {
namespace vit {

// q, k: [B][heads][ntok_pad][64] halves as EPI_QKV leaves them (q pre-scaled by log2(e) / 8; x3: the lo plane `plane` halves further);
// attn_out: fp32 [B][heads][ntok].  One launch on `stream`.
hipError_t launch_cls_attn(const _Float16* q, const _Float16* k, size_t plane, int ntok, int ntok_pad, int heads, int B, bool x3,
                           float* attn_out, hipStream_t stream);

}  // namespace vit
}  // namespace stego
