// The few constants of the correspondence loss that host-only code needs as well (plain C++, no HIP include): corr_common.h brings
// them to the kernels, corr_bwd_plan.h to the backward's plan and its stand-alone test.
#pragma once
#include <cstddef>

namespace stego {

constexpr int TP = 128;        // sample points per side, padded (S*S <= 128)
constexpr int NTHREADS = 256;  // 4 wave64 (the gather team size everywhere)

enum { PREC_F32 = 0, PREC_F16X3 = 1 };

constexpr size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace stego
