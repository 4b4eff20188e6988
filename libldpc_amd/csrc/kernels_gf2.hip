// kernels_gf2.hip — the GF(2) work of the batch interface's transmit side and its check (include/ldpc_amd.h,
// ldpc_hip_encode_batch / ldpc_hip_syndrome_batch / ldpc_hip_bit_errors_batch).  Bit rows are packed as hard_bits is: bit
// i & 31 of word i >> 5, the unused high bits of a row's last word zero on output and ignored on input.
//   gf2_encode_kernel<T>   codeword = info x G as a matrix product over packed words.  A wave takes 64 consecutive columns, a
//                          column per lane; the lane keeps T words of its column's mask in registers, the frame's
//                          information words are wave-uniform and arrive through the scalar path, a codeword bit is the
//                          parity of XOR_w (info[w] & mask[w]), and one ballot of the 64 parities is the frame's two output
//                          words.  kGf2FrameTile frames share the registers' masks; when the information word has more than
//                          T words the kernel walks it in chunks of T, a partial XOR per frame of the tile, the parity after
//                          the last chunk.  Byte information is packed in front by launch_pack_hard (kernels_convert.hip).
//   gf2_syndrome_kernel    a frame's word staged packed in LDS (bytes packed by ballot on the way in), a check node per
//                          thread XORs the bits at its row's columns (row CSR of H), a ballot is two syndrome words, the
//                          weight is the population count summed over the frame's waves.
//   gf2_bit_errors_kernel  a wave per frame: 64 columns at a time, (a ^ b) & the transmitted-position mask, population count.
// No kernel returns in front of a ballot: lanes beyond nc / mc take part and contribute 0.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"

namespace ldpc_amd
{

namespace
{
constexpr int kGf2Threads = 256;

// ---- encoder ----
// The information row is read word by word (32-bit scalar loads): the row stride ceil(kc / 32) is odd for many kc, so no
// wider alignment holds.  Every read stays inside the row: T <= words (the launcher picks it so), and where T does not
// divide `words` the last chunk's window is moved back to end at the row's end, the mask words it has seen already zeroed.
template <int T>
__global__ __launch_bounds__(kGf2Threads) void gf2_encode_kernel(Gf2EncodeArgs a)
{
    constexpr int F = kGf2FrameTile;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kGf2Threads + threadIdx.x; // < mask_cols: the table is padded with zero columns
    const uint32_t k = static_cast<uint32_t>(j >> 6);                                 // the wave's group of 64 columns
    const uint32_t words = a.words, out_words = (a.nc + 31u) / 32u;
    const uint64_t f_begin = static_cast<uint64_t>(blockIdx.y) * kGf2FramesPerBlock;
    const uint64_t f_end = f_begin + kGf2FramesPerBlock < a.n ? f_begin + kGf2FramesPerBlock : a.n;
    const bool single = words == static_cast<uint32_t>(T);
    uint32_t m[T];
    if (single) // the whole column mask stays in registers for every frame of the block
    {
#pragma unroll
        for (int t = 0; t < T; ++t)
            m[t] = a.mask[static_cast<uint64_t>(t) * a.mask_cols + j];
    }
    for (uint64_t f0 = f_begin; f0 < f_end; f0 += F) // (wave-uniform)
    {
        uint32_t acc[F];
#pragma unroll
        for (int f = 0; f < F; ++f)
            acc[f] = 0;
        for (uint32_t done = 0; done < words; done += T)
        {
            const uint32_t base = done + T <= words ? done : words - T; // the last window ends at the row's end
            if (!single)
            {
#pragma unroll
                for (int t = 0; t < T; ++t)
                {
                    const uint32_t v = a.mask[static_cast<uint64_t>(base + t) * a.mask_cols + j];
                    m[t] = base + t >= done ? v : 0u;
                }
            }
#pragma unroll
            for (int f = 0; f < F; ++f)
            {
                const uint64_t frame = f0 + f < a.n ? f0 + f : a.n - 1; // (a ragged tile reads its last frame again)
                const auto u = uniform_table(a.info + frame * words + base);
                uint32_t x = acc[f];
#pragma unroll
                for (int t = 0; t < T; ++t)
                    x ^= u[t] & m[t];
                acc[f] = x;
            }
        }
#pragma unroll
        for (int f = 0; f < F; ++f)
        {
            const uint64_t frame = f0 + f;
            const bool one = (__popc(acc[f]) & 1) != 0; // (columns from G.cols on have empty masks: 0)
            const uint64_t vote = __ballot(one);
            if (frame < a.n) // (wave-uniform)
            {
                if (a.codeword && j < a.nc)
                    a.codeword[frame * a.nc + j] = one ? 1 : 0;
                if (a.codeword_bits)
                {
                    uint32_t *row = a.codeword_bits + frame * out_words;
                    if (lane == 0 && 2 * k < out_words)
                        row[2 * k] = static_cast<uint32_t>(vote);
                    if (lane == 32 && 2 * k + 1 < out_words)
                        row[2 * k + 1] = static_cast<uint32_t>(vote >> 32);
                }
            }
        }
    }
}

// ---- syndrome ----
// WPF waves share a frame (256 / (64 WPF) frames per workgroup).  lds: per frame slot ceil(nc / 64) * 2 words.
template <int WPF, bool BYTES>
__global__ __launch_bounds__(kGf2Threads) void gf2_syndrome_kernel(Gf2SyndromeArgs a)
{
    extern __shared__ uint32_t gf2_lds[];
    constexpr uint32_t kPer = 64u * WPF, kSlots = kGf2Threads / kPer;
    __shared__ uint32_t weight_sum[kSlots];
    const uint32_t lane = threadIdx.x & 63u, slot = threadIdx.x / kPer, t = threadIdx.x % kPer, wave = t >> 6;
    const uint32_t chunks = (a.nc + 63u) / 64u, in_words = (a.nc + 31u) / 32u, out_words = (a.mc + 31u) / 32u;
    uint32_t *word = gf2_lds + static_cast<size_t>(slot) * 2u * chunks;
    const uint64_t per_pass = static_cast<uint64_t>(gridDim.x) * kSlots;
    for (uint64_t first = static_cast<uint64_t>(blockIdx.x) * kSlots; first < a.n; first += per_pass) // (the same trips for every thread)
    {
        const uint64_t frame = first + slot;
        const bool live = frame < a.n; // (uniform over the frame's waves)
        if (t == 0)
            weight_sum[slot] = 0;
        if (live)
        {
            if constexpr (BYTES)
            {
                const uint8_t *src = static_cast<const uint8_t *>(a.word) + frame * a.nc;
                for (uint32_t c0 = 64u * wave; c0 < a.nc; c0 += kPer) // (wave-uniform: every lane votes)
                {
                    const uint32_t c = c0 + lane;
                    const uint64_t vote = __ballot(c < a.nc && src[c] != 0);
                    if (lane == 0)
                        word[c0 >> 5] = static_cast<uint32_t>(vote);
                    if (lane == 32)
                        word[(c0 >> 5) + 1] = static_cast<uint32_t>(vote >> 32);
                }
            }
            else
            {
                const uint32_t *src = static_cast<const uint32_t *>(a.word) + frame * in_words;
                for (uint32_t i = t; i < in_words; i += kPer)
                    word[i] = src[i]; // (bits from nc on: no row of H reads them)
            }
        }
        __syncthreads();
        if (live)
        {
            uint32_t weight = 0;
            for (uint32_t r0 = 64u * wave; r0 < a.mc; r0 += kPer)
            {
                const uint32_t r = r0 + lane;
                uint32_t s = 0;
                if (r < a.mc)
                    for (uint32_t p = a.row_ptr[r], e = a.row_ptr[r + 1]; p < e; ++p)
                    {
                        const uint32_t c = a.row_col[p];
                        s ^= word[c >> 5] >> (c & 31u);
                    }
                s &= 1u;
                const uint64_t vote = __ballot(s != 0);
                weight += static_cast<uint32_t>(__popcll(vote));
                if (a.syndrome && r < a.mc)
                    a.syndrome[frame * a.mc + r] = static_cast<uint8_t>(s);
                if (a.syndrome_bits)
                {
                    uint32_t *row = a.syndrome_bits + frame * out_words;
                    if (lane == 0)
                        row[r0 >> 5] = static_cast<uint32_t>(vote);
                    if (lane == 32 && (r0 >> 5) + 1 < out_words)
                        row[(r0 >> 5) + 1] = static_cast<uint32_t>(vote >> 32);
                }
            }
            if (a.weight)
            {
                if constexpr (WPF == 1)
                {
                    if (lane == 0)
                        a.weight[frame] = weight;
                }
                else if (lane == 0)
                    atomicAdd(&weight_sum[slot], weight); // (the wave's count is wave-uniform: one lane adds it)
            }
        }
        __syncthreads();
        if (WPF > 1 && live && a.weight && t == 0)
            a.weight[frame] = weight_sum[slot];
        if (WPF > 1)
            __syncthreads(); // (the next pass zeroes the sum)
    }
}

// ---- bit errors ----
// 64 columns of an operand as one wave-uniform 64-bit value: bytes by ballot, packed words through the scalar path
template <bool BYTES>
__device__ __forceinline__ uint64_t gf2_columns(const void *rows, uint64_t frame, uint32_t nc, uint32_t words, uint32_t chunk, uint32_t lane)
{
    if constexpr (BYTES)
    {
        const uint32_t c = 64u * chunk + lane;
        return __ballot(c < nc && static_cast<const uint8_t *>(rows)[frame * nc + c] != 0);
    }
    else
    {
        const auto w = uniform_table(static_cast<const uint32_t *>(rows) + frame * words);
        const uint64_t lo = w[2 * chunk];
        const uint64_t hi = 2 * chunk + 1 < words ? w[2 * chunk + 1] : 0u;
        return lo | (hi << 32);
    }
}

template <bool A_BYTES, bool B_BYTES>
__global__ __launch_bounds__(kGf2Threads) void gf2_bit_errors_kernel(Gf2BitErrorArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t frame = static_cast<uint64_t>(blockIdx.x) * (kGf2Threads / 64) + wave;
    if (frame >= a.n) // (wave-uniform: the whole wave leaves)
        return;
    const uint32_t chunks = (a.nc + 63u) / 64u, words = (a.nc + 31u) / 32u;
    const auto tx = uniform_table(a.tx_mask);
    uint32_t count = 0;
    for (uint32_t k = 0; k < chunks; ++k)
    {
        const uint64_t x = gf2_columns<A_BYTES>(a.a, frame, a.nc, words, k, lane) ^ gf2_columns<B_BYTES>(a.b, frame, a.nc, words, k, lane);
        count += static_cast<uint32_t>(__popcll(x & tx[k])); // (the mask has no bit from nc on; wave-uniform, so no wave sum)
    }
    if (lane == 0)
        a.bit_errors[frame] = count;
}
} // namespace

int gf2_encode_chunk_words(uint32_t words)
{
    int t = 1;
    while (t < kGf2MaxChunkWords && 2u * t <= words)
        t *= 2;
    return t;
}

int launch_gf2_encode(const Gf2EncodeArgs &a, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    if (!a.info || !a.mask || a.nc == 0 || a.words == 0 || a.mask_cols % kGf2Threads || a.mask_cols < a.nc ||
        a.n > static_cast<uint64_t>(kGf2FramesPerBlock) * 65535u)
        return hipErrorInvalidValue;
    if (!a.codeword && !a.codeword_bits)
        return hipSuccess;
    const dim3 grid(static_cast<unsigned>(a.mask_cols / kGf2Threads), static_cast<unsigned>((a.n + kGf2FramesPerBlock - 1) / kGf2FramesPerBlock));
    const dim3 block(kGf2Threads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (gf2_encode_chunk_words(a.words))
    {
    case 1: hipLaunchKernelGGL(gf2_encode_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(gf2_encode_kernel<2>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(gf2_encode_kernel<4>, grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL(gf2_encode_kernel<8>, grid, block, 0, s, a); break;
    case 16: hipLaunchKernelGGL(gf2_encode_kernel<16>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(gf2_encode_kernel<kGf2MaxChunkWords>, grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

int launch_gf2_syndrome(const Gf2SyndromeArgs &a, int format, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    if (!a.word || !a.row_ptr || !a.row_col || a.nc == 0 || (format != kBitsU8 && format != kBitsPacked32))
        return hipErrorInvalidValue;
    if (!a.syndrome && !a.syndrome_bits && !a.weight)
        return hipSuccess;
    const int wpf = gf2_syndrome_waves_per_frame(a.nc);
    const uint32_t slots = kGf2Threads / (64 * wpf);
    const size_t lds = static_cast<size_t>(slots) * gf2_syndrome_frame_lds_bytes(a.nc);
    if (lds > kGf2SyndromeMaxLds)
        return hipErrorInvalidValue;
    const uint64_t blocks = (a.n + slots - 1) / slots;
    const dim3 grid(static_cast<unsigned>(blocks < (1u << 20) ? blocks : (1u << 20))), block(kGf2Threads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool bytes = format == kBitsU8;
    if (wpf == 1)
    {
        if (bytes)
            hipLaunchKernelGGL((gf2_syndrome_kernel<1, true>), grid, block, lds, s, a);
        else
            hipLaunchKernelGGL((gf2_syndrome_kernel<1, false>), grid, block, lds, s, a);
    }
    else
    {
        if (bytes)
            hipLaunchKernelGGL((gf2_syndrome_kernel<4, true>), grid, block, lds, s, a);
        else
            hipLaunchKernelGGL((gf2_syndrome_kernel<4, false>), grid, block, lds, s, a);
    }
    return hipGetLastError();
}

int launch_gf2_bit_errors(const Gf2BitErrorArgs &a, int a_format, int b_format, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    const auto known = [](int f) { return f == kBitsU8 || f == kBitsPacked32; };
    if (!a.a || !a.b || !a.tx_mask || !a.bit_errors || a.nc == 0 || !known(a_format) || !known(b_format) ||
        a.n > (1ull << 31))
        return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.n + kGf2Threads / 64 - 1) / (kGf2Threads / 64))), block(kGf2Threads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool ab = a_format == kBitsU8, bb = b_format == kBitsU8;
    if (ab && bb)
        hipLaunchKernelGGL((gf2_bit_errors_kernel<true, true>), grid, block, 0, s, a);
    else if (ab)
        hipLaunchKernelGGL((gf2_bit_errors_kernel<true, false>), grid, block, 0, s, a);
    else if (bb)
        hipLaunchKernelGGL((gf2_bit_errors_kernel<false, true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((gf2_bit_errors_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

} // namespace ldpc_amd
