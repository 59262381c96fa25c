// The C = 192 instantiations of corr_fused_kernel (vit_tiny; even and odd K) and their launch function.
#include "corr_fused_kernel.h"
#include "launchers.h"

namespace stego {

// C = 192: six feature stages, at least two code chunks (c_api.hip: geometry) - there is no NKC = 1 kernel to fall back on
hipError_t launch_fused_c192(const FusedParams& prm, int precision, dim3 grid, dim3 block, int lds, hipStream_t stream)
{
    return (prm.K & 1) ? launch_fused_nkc<2, true, true, 2, 3, 4>(prm, precision, grid, block, lds, stream)
                       : launch_fused_nkc<2, false, true, 2, 3, 4>(prm, precision, grid, block, lds, stream);
}

}  // namespace stego
