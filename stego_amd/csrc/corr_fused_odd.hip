// The odd-K instantiations of corr_fused_kernel (C = 384 / 768) and their launch function.
#include "corr_fused_kernel.h"
#include "launchers.h"

namespace stego {

hipError_t launch_fused_odd(const FusedParams& prm, int precision, dim3 grid, dim3 block, int lds, hipStream_t stream)
{
    return prm.C == 384 ? launch_fused_nkc<3, true, false, 1, 2, 3, 4>(prm, precision, grid, block, lds, stream)
                        : launch_fused_nkc<6, true, false, 1, 2, 3, 4>(prm, precision, grid, block, lds, stream);
}

}  // namespace stego
