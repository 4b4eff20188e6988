// kernels_convert.hip — the two conversions around ldpc_hip_decode_batch_typed (include/ldpc_amd.h), both grid-stride:
//   widen_llr_kernel   typed LLRs (binary32, binary16, int8) -> the binary64 array W every decoder takes.  binary32 and
//                      binary16 widen exactly (NaN stays NaN, infinities, signed zeros and subnormals are kept); an int8 k
//                      becomes fl((double) k * step), one rounding.  (Fixed-point layered min-sum reads typed LLRs itself:
//                      kernels_layered_fixed_direct.hip.)
//   pack_hard_kernel   decision bytes [n][nc] -> words [n][ceil(nc / 32)], bit c & 31 of word c >> 5 = hard[c], the unused
//                      high bits of a frame's last word zero.  One wave takes 64 columns of a frame — a byte per lane,
//                      coalesced — and a ballot is its two words.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace ldpc_amd
{

namespace
{
constexpr int kConvThreads = 256;
constexpr uint64_t kConvMaxBlocks = 1 << 15; // (grid-stride beyond that: 256 CUs x a few dozen blocks)

template <typename T>
__global__ __launch_bounds__(kConvThreads) void widen_llr_kernel(const T *__restrict__ src, double scale, uint64_t count, double *__restrict__ dst)
{
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kConvThreads;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kConvThreads + threadIdx.x; i < count; i += stride)
    {
        if constexpr (sizeof(T) == 1)
            dst[i] = static_cast<double>(src[i]) * scale; // (exact conversion, one rounded product)
        else
            dst[i] = static_cast<double>(src[i]);
    }
}

__global__ __launch_bounds__(kConvThreads) void pack_hard_kernel(const uint8_t *__restrict__ hard, uint64_t n, uint32_t nc, uint32_t *__restrict__ bits)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t chunks_per_frame = (nc + 63u) / 64u, words_per_frame = (nc + 31u) / 32u;
    const uint64_t chunks = n * chunks_per_frame; // one wave each
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kConvThreads / 64);
    for (uint64_t w = static_cast<uint64_t>(blockIdx.x) * (kConvThreads / 64) + threadIdx.x / 64; w < chunks; w += waves) // (wave-uniform)
    {
        const uint64_t frame = w / chunks_per_frame, k = w % chunks_per_frame;
        const uint64_t c = 64 * k + lane;
        const bool one = c < nc && hard[frame * nc + c] != 0;
        const uint64_t mask = __ballot(one);
        uint32_t *row = bits + frame * words_per_frame;
        if (lane == 0)
            row[2 * k] = static_cast<uint32_t>(mask);
        if (lane == 32 && 2 * k + 1 < words_per_frame)
            row[2 * k + 1] = static_cast<uint32_t>(mask >> 32);
    }
}

unsigned conv_blocks(uint64_t items_per_block_unit)
{
    return static_cast<unsigned>(items_per_block_unit < kConvMaxBlocks ? (items_per_block_unit ? items_per_block_unit : 1) : kConvMaxBlocks);
}
} // namespace

int launch_widen_llr(const void *src, int type, double step, uint64_t count, double *dst, void *stream)
{
    if (count == 0)
        return hipSuccess;
    if (!src || !dst)
        return hipErrorInvalidValue;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(conv_blocks((count + kConvThreads - 1) / kConvThreads)), block(kConvThreads);
    switch (type)
    {
    case kLlrF32: hipLaunchKernelGGL(widen_llr_kernel<float>, grid, block, 0, s, static_cast<const float *>(src), 1.0, count, dst); break;
    case kLlrF16: hipLaunchKernelGGL(widen_llr_kernel<_Float16>, grid, block, 0, s, static_cast<const _Float16 *>(src), 1.0, count, dst); break;
    case kLlrI8: hipLaunchKernelGGL(widen_llr_kernel<int8_t>, grid, block, 0, s, static_cast<const int8_t *>(src), step, count, dst); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

int launch_pack_hard(const uint8_t *hard, uint64_t n, int nc, uint32_t *bits, void *stream)
{
    if (n == 0)
        return hipSuccess;
    if (!hard || !bits || nc <= 0)
        return hipErrorInvalidValue;
    const uint64_t chunks = n * ((static_cast<uint64_t>(nc) + 63) / 64);
    const dim3 grid(conv_blocks((chunks + kConvThreads / 64 - 1) / (kConvThreads / 64))), block(kConvThreads);
    hipLaunchKernelGGL(pack_hard_kernel, grid, block, 0, static_cast<hipStream_t>(stream), hard, n, static_cast<uint32_t>(nc), bits);
    return hipGetLastError();
}

} // namespace ldpc_amd
