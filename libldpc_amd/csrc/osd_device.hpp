// osd_device.hpp — what the two ordered-statistics kernels (kernels_osd.hip, kernels_osd_syndrome.hip) share on the device:
// the typed element widened exactly, its reliability, and the integer sum of a wave.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace ldpc_amd
{

// element i of the typed input, widened exactly (Args: OsdArgs or OsdSyndromeArgs)
template <class Args>
__device__ __forceinline__ double osd_widen(const Args &a, uint64_t i)
{
    switch (a.llr_type) // (uniform)
    {
    case kLlrF64: return static_cast<const double *>(a.llr)[i];
    case kLlrF32: return static_cast<double>(static_cast<const float *>(a.llr)[i]);
    case kLlrF16: return static_cast<double>(static_cast<const _Float16 *>(a.llr)[i]);
    default: return static_cast<double>(static_cast<const int8_t *>(a.llr)[i]);
    }
}

// min(floor(|w| * 4096), 2^31 - 1); a NaN gives 0.  The product is exact or infinite: a power of two
__device__ __forceinline__ uint32_t osd_reliability(double w)
{
    const double s = fabs(w) * 4096.0;
    return !(s == s) ? 0u : s >= 2147483647.0 ? kOsdQMax : static_cast<uint32_t>(s);
}

__device__ __forceinline__ int64_t osd_wave_sum(int64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
        const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint64_t>(v)), o, 64));
        const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint64_t>(v) >> 32), o, 64));
        v += static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
    }
    return v;
}

} // namespace ldpc_amd
