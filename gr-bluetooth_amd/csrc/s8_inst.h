// s8_inst.h -- the int8-input instantiations of the kernels that read the input stream (kernels.hip.h "Input formats").
//
// They are compiled in a translation unit of their own (s8_kernels.hip): btgpu.hip sees them as explicit instantiation
// DECLARATIONS (extern template) and only takes their addresses through bank_launch.h's helpers, exact_rows_pick<kInS8> and
// its own ddc_direct_kernel launches.  One list, two uses: BTGPU_S8_INSTANTIATE defined -> definitions, else declarations.
// A launch helper that picks an int8 kernel missing from this list fails at link time, not at run time.
#pragma once
#include "kernels.hip.h"
#include "pfb100.hip.h"
#include "pfb100f.hip.h"
#include "pfbm.hip.h"
#include "pfbg.hip.h"
#include "exact.hip.h"
#include "exact_dense.hip.h"
#include "exact_narrow.hip.h"
#include "ddc_mfma.hip.h"

namespace btgpu {

#ifdef BTGPU_S8_INSTANTIATE
#define BTGPU_S8_KERNEL(...) template __global__ void __VA_ARGS__;   // (the only symbols the library exports: s8_kernels.map)
#else
#define BTGPU_S8_KERNEL(...) extern template __global__ void __VA_ARGS__;
#endif

// direct-form bank: DIRECT channelizer and squelch, segmented rates, the staged squelch's direct stage 1
BTGPU_S8_KERNEL(ddc_direct_kernel_s8<2>(const float2 *, long long, long long, int, int, int, const float2 *, const float2 *, int,
                                            const double *, float2 *, long long, long long, int, int, long long))
// 100-bin bank, runs of tiles (launch_channel_bank's default forms)
BTGPU_S8_KERNEL(pfb100f_kernel_s8<256, true, 10, 255>(PfbParams))
BTGPU_S8_KERNEL(pfb100f_kernel_s8<256, true, 10, 231>(PfbParams))
BTGPU_S8_KERNEL(pfb100f_kernel_s8<256, false, 10, 227>(PfbParams))
// 100-bin bank, one tile per workgroup: fused (the run kernel's fallback), channel bank alone, stand-alone squelch stage 1
BTGPU_S8_KERNEL(pfb100_kernel_s8<7, 1, 26, true, true, 256, true>(PfbParams))
BTGPU_S8_KERNEL(pfb100_kernel_s8<7, 1, 26, false, true, 256, true>(PfbParams))
BTGPU_S8_KERNEL(pfb100_kernel_s8<7, 1, 26, true, true, 256, false>(PfbParams))
BTGPU_S8_KERNEL(pfb100_kernel_s8<7, 1, 26, false, true, 256, false>(PfbParams))
BTGPU_S8_KERNEL(pfb100_kernel_s8<15, 5, 10, false, false, 256, false>(PfbParams))
// small-M banks (launch_channel_bank_m, launch_noise_bank_m)
BTGPU_S8_KERNEL(pfbm_kernel_s8<false, true, 8, 7, true, true>(PfbmParams))
BTGPU_S8_KERNEL(pfbm_kernel_s8<false, true, 8, 7, true, false>(PfbmParams))
BTGPU_S8_KERNEL(pfbm_kernel_s8<true, true, 8, 7, true, false>(PfbmParams))
BTGPU_S8_KERNEL(pfbm_kernel_s8<false, true, 8, 7, false, false>(PfbmParams))
BTGPU_S8_KERNEL(pfbm_kernel_s8<true, true, 20, 7, false, false>(PfbmParams))
BTGPU_S8_KERNEL(pfbm_kernel_s8<true, true, 0, 0, false, false>(PfbmParams))
BTGPU_S8_KERNEL(pfbm_kernel_s8<false, true, 0, 0, false, false>(PfbmParams))
BTGPU_S8_KERNEL(pfbm_kernel_s8<false, false, 8, 15, true, false>(PfbmParams))
BTGPU_S8_KERNEL(pfbm_kernel_s8<false, false, 8, 15, false, false>(PfbmParams))
BTGPU_S8_KERNEL(pfbm_kernel_s8<false, false, 0, 0, false, false>(PfbmParams))
// general-M bank, DFT on the matrix pipe (launch_channel_bank_g, launch_noise_bank_g)
BTGPU_S8_KERNEL(pfbg_kernel_s8<true, true>(PfbgParams))
BTGPU_S8_KERNEL(pfbg_kernel_s8<false, true>(PfbgParams))
BTGPU_S8_KERNEL(pfbg_kernel_s8<false, false>(PfbgParams))
// exact rows: every decimation exact_rows_pick serves
#define BTGPU_S8_EX(n) BTGPU_S8_KERNEL(exact_rows_kernel_s8<n>(ExactParams, const float2 *))
BTGPU_S8_EX(2) BTGPU_S8_EX(3) BTGPU_S8_EX(4) BTGPU_S8_EX(5) BTGPU_S8_EX(6) BTGPU_S8_EX(7) BTGPU_S8_EX(8) BTGPU_S8_EX(9)
BTGPU_S8_EX(10) BTGPU_S8_EX(11) BTGPU_S8_EX(12) BTGPU_S8_EX(13) BTGPU_S8_EX(14) BTGPU_S8_EX(15) BTGPU_S8_EX(16) BTGPU_S8_EX(17)
BTGPU_S8_EX(18) BTGPU_S8_EX(19) BTGPU_S8_EX(20) BTGPU_S8_EX(21) BTGPU_S8_EX(22) BTGPU_S8_EX(23) BTGPU_S8_EX(24) BTGPU_S8_EX(25)
BTGPU_S8_EX(50)
#undef BTGPU_S8_EX
// exact rows, dense form: one kernel for every decimation
BTGPU_S8_KERNEL(exact_dense_kernel_s8<0>(ExactParams, const float2 *))
// exact rows, narrow form: one kernel per number of matrix instructions in a tap block (D <= 8)
BTGPU_S8_KERNEL(exact_narrow_kernel_s8<1>(ExactParams, const float2 *))
BTGPU_S8_KERNEL(exact_narrow_kernel_s8<2>(ExactParams, const float2 *))
BTGPU_S8_KERNEL(exact_narrow_kernel_s8<3>(ExactParams, const float2 *))
BTGPU_S8_KERNEL(exact_narrow_kernel_s8<4>(ExactParams, const float2 *))
// direct-form bank on the matrix pipe (BTGPU_FLAG_DIRECT_MFMA)
BTGPU_S8_KERNEL(ddc_mfma_kernel_s8<0>(DdcMfmaParams))
#undef BTGPU_S8_KERNEL

}  // namespace btgpu
