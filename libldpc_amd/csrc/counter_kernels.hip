// counter_kernels.hip — the counter-based noise mode's own launches (device_philox.hpp): the raw generator words
// (ldpc_hip_philox) and the encoder's info words.  The channel itself is computed inside the decode launches' prologues.
#include <hip/hip_runtime.h>

#include "device_philox.hpp"
#include "kernels.hpp"

namespace ldpc_amd
{

namespace
{

__global__ __launch_bounds__(256) void philox_kernel(uint32_t k0, uint32_t k1, uint32_t tag, uint64_t frame, uint32_t first_block,
                                                     uint64_t n_blocks, uint32_t *out)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_blocks)
        return;
    const uint4 w = philox_block(k0, k1, frame, first_block + static_cast<uint32_t>(i), tag);
    reinterpret_cast<uint4 *>(out)[i] = w;
}

// one thread per (frame, 64-bit info word): word w of frame f = 32-bit words 2 (w % 2), 2 (w % 2) + 1 of block w / 2 (tag 2)
__global__ __launch_bounds__(256) void encode_info_counter_kernel(uint32_t k0, uint32_t k1, uint64_t frame0, uint64_t n, int kc,
                                                                  int words, uint64_t *prefix)
{
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n * static_cast<uint64_t>(words))
        return;
    const uint64_t f = t / static_cast<uint64_t>(words);
    const int w = static_cast<int>(t - f * static_cast<uint64_t>(words));
    const uint4 b = philox_block(k0, k1, frame0 + f, static_cast<uint32_t>(w / 2), kTagInfo);
    uint64_t v = (w & 1) ? (static_cast<uint64_t>(b.w) << 32 | b.z) : (static_cast<uint64_t>(b.y) << 32 | b.x);
    const int left = kc - 64 * w; // (info bits from kc on are zero)
    if (left < 64)
        v &= (1ull << left) - 1;
    prefix[t] = v;
}

} // namespace

int launch_philox(uint64_t seed, uint32_t tag, uint64_t frame, uint32_t first_block, uint64_t n_blocks, uint32_t *out, void *stream)
{
    if (n_blocks == 0)
        return hipSuccess;
    if (!out || n_blocks > (1ull << 32) - first_block)
        return hipErrorInvalidValue;
    const uint64_t groups = (n_blocks + 255) / 256;
    hipLaunchKernelGGL(philox_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), tag, frame, first_block, n_blocks, out);
    return hipGetLastError();
}

int launch_encode_info_counter(uint64_t seed, uint64_t frame0, uint64_t n, int kc, int words, uint64_t *prefix, void *stream)
{
    if (n == 0)
        return hipSuccess;
    if (!prefix || kc <= 0 || words != (kc + 63) / 64)
        return hipErrorInvalidValue;
    const uint64_t groups = (n * static_cast<uint64_t>(words) + 255) / 256;
    hipLaunchKernelGGL(encode_info_counter_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), frame0, n, kc, words, prefix);
    return hipGetLastError();
}

} // namespace ldpc_amd
