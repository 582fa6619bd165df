// jk_helpers.hpp -- device helpers the J/K streams share (kern_fock.hip, kern_cphf.hip): wave reductions and the
// packed-pair index.
#pragma once
#include <hip/hip_runtime.h>

namespace mqc {

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Wave sum through the DPP lane network: quad swaps, half-row and row mirrors, then the two row broadcasts -- 18 VALU
// instructions and no LDS round trip (a shuffle is two ds_bpermute_b32 per step and a wait for each).  The total is
// valid in lanes 48..63 only.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_take(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWMASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWMASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_top(double v)
{
    v += dpp_take<0xB1, 0xf>(v);        // quad_perm [1, 0, 3, 2]
    v += dpp_take<0x4E, 0xf>(v);        // quad_perm [2, 3, 0, 1]
    v += dpp_take<0x141, 0xf>(v);       // row_half_mirror
    v += dpp_take<0x140, 0xf>(v);       // row_mirror: every lane of a row of 16 holds the row's sum
    v += dpp_take<0x142, 0xa>(v);       // row_bcast15 into rows 1 and 3
    v += dpp_take<0x143, 0xc>(v);       // row_bcast31 into rows 2 and 3: row 3 holds the wave's sum
    return v;
}

__device__ __forceinline__ void unpack_pair(int idx, int& k, int& l)
{
    k = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
    while ((k + 1) * (k + 2) / 2 <= idx) ++k;
    while (k * (k + 1) / 2 > idx) --k;
    l = idx - k * (k + 1) / 2;
}

}  // namespace mqc
