// kernels_channel.hip — channel and demapper of the batch interface (include/ldpc_amd.h, ldpc_hip_channel_batch): codeword
// bits of frames that stay on the device in, LLRs in the element type the decoder reads out.  The noise is the counter mode's
// (device_philox.hpp, used as it stands): for binary signalling a frame's LLRs are, bit for bit, those of the stream's
// channel prologue (device_channel.hpp, channel_init) under the same seed and frame index.
//   channel_kernel<M, T, BSC>  M bits per symbol (AWGN: 2^M-ASK, Gray-labelled, max-log demapper in binary64; BSC: M = 1), T the
//                              element type of the LLRs (kernels.hpp, LlrType): the conversion is in the type, not a branch
//                              per element.  ONE LANE = ONE PHILOX BLOCK of a frame: four symbols, 4 M transmitted bits.  It
//                              reads its bits (bytes through bit_pos, or out of the packed word), writes its LLRs to the bits'
//                              columns and its four received values.  Behind the frame's block lanes come the lanes of the
//                              columns the channel does not write (punctured, unconnected: +0.0; shortened: the channel's
//                              value), one column each, so that every element of a wanted output is written exactly once in
//                              one launch.  Adjacent lanes write adjacent memory wherever bit_pos is consecutive; with M = 1 a
//                              lane's four values leave in one store of four elements where they are consecutive and aligned.
// No LDS, no scratch; lane = global thread index, frame = lane / work (32-bit: the launcher keeps n * work below 2^31).
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "device_philox.hpp"
#include "kernels.hpp"

namespace ldpc_amd
{

namespace
{
constexpr int kChannelThreads = 256;

template <int T>
struct LlrElem;
template <>
struct LlrElem<kLlrF64> { using type = double; };
template <>
struct LlrElem<kLlrF32> { using type = float; };
template <>
struct LlrElem<kLlrF16> { using type = _Float16; };
template <>
struct LlrElem<kLlrI8> { using type = int8_t; };

// L in the element type T.  kLlrF32: one rounding to nearest-even; kLlrF16: the binary32 value rounded again; kLlrI8:
// clamp(rint(fl(L * inv)), -qmax, +qmax), the clamp in binary64, a NaN gives 0 (kernels_qms.hip, qms_quantize)
template <int T>
__device__ __forceinline__ typename LlrElem<T>::type llr_elem(double L, double inv, int qmax)
{
#pragma clang fp contract(off)
    if constexpr (T == kLlrF64)
        return L;
    else if constexpr (T == kLlrF32)
        return static_cast<float>(L);
    else if constexpr (T == kLlrF16)
    {
        const float f = static_cast<float>(L);
        return static_cast<_Float16>(f);
    }
    else
    {
        const double x = __builtin_rint(L * inv);
        const double q = static_cast<double>(qmax);
        const int v = x >= q ? qmax : (x <= -q ? -qmax : (x == x ? static_cast<int>(x) : 0));
        return static_cast<int8_t>(v);
    }
}

template <int T>
__device__ __forceinline__ void store_llr(void *dst, uint64_t idx, double L, double inv, int qmax)
{
    static_cast<typename LlrElem<T>::type *>(dst)[idx] = llr_elem<T>(L, inv, qmax);
}

// the four values of a lane's block at dst[idx[k]], k < count: one store of four elements where they are consecutive and the
// first one's address is a multiple of the four's size (h.txt: every block of every frame), else one store each
template <int T>
__device__ __forceinline__ void store_block(void *dst, const uint64_t (&idx)[4], const double (&L)[4], uint32_t count, double inv, int qmax)
{
    using E = typename LlrElem<T>::type;
    typedef E E4 __attribute__((ext_vector_type(4)));
    E *const p = static_cast<E *>(dst) + idx[0];
    if (count == 4 && idx[1] == idx[0] + 1 && idx[2] == idx[0] + 2 && idx[3] == idx[0] + 3 &&
        reinterpret_cast<uintptr_t>(p) % (4 * sizeof(E)) == 0)
    {
        E4 v;
        v.x = llr_elem<T>(L[0], inv, qmax), v.y = llr_elem<T>(L[1], inv, qmax), v.z = llr_elem<T>(L[2], inv, qmax), v.w = llr_elem<T>(L[3], inv, qmax);
        *reinterpret_cast<E4 *>(p) = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (static_cast<uint32_t>(k) < count)
            static_cast<E *>(dst)[idx[k]] = llr_elem<T>(L[k], inv, qmax);
}

// bit `col` of the frame's codeword (wave-uniform format; a null codeword is all zero)
__device__ __forceinline__ int codeword_bit(const ChannelArgs &a, uint64_t frame, uint32_t col)
{
    if (!a.codeword)
        return 0;
    if (a.codeword_format == kBitsU8)
        return static_cast<const uint8_t *>(a.codeword)[frame * a.nc + col] != 0 ? 1 : 0;
    const uint32_t words = (a.nc + 31u) / 32u;
    return static_cast<int>((static_cast<const uint32_t *>(a.codeword)[frame * words + (col >> 5)] >> (col & 31u)) & 1u);
}

template <int M, int T, bool BSC>
__global__ __launch_bounds__(kChannelThreads) void channel_kernel(ChannelArgs a)
{
#pragma clang fp contract(off)
    static_assert(M >= 1 && M <= kChannelMaxBitsPerSymbol && (!BSC || M == 1), "bits per symbol");
    constexpr int kLevels = 1 << M;
    const uint64_t g64 = static_cast<uint64_t>(blockIdx.x) * kChannelThreads + threadIdx.x;
    if (g64 >= a.n * a.work)
        return;
    const uint32_t g = static_cast<uint32_t>(g64);
    const uint32_t row = g / a.work, w = g - row * a.work;
    const uint64_t frame = row;
    if (w >= a.blocks) // a column the channel does not write
    {
        if (a.llr)
        {
            const uint32_t e = a.other[w - a.blocks];
            store_llr<T>(a.llr, frame * a.nc + (e & ~kChannelShortened), (e & kChannelShortened) ? a.shorten : 0.0, a.inv, a.qmax);
        }
        return;
    }
    const uint32_t nct = a.nct, S = a.symbols;
    const uint4 blk = philox_block(a.key[0], a.key[1], a.frame0 + frame, w, BSC ? kTagDraw : kTagAwgn);
    if constexpr (M == 1) // binary signalling, AWGN and BSC: the operations of channel_init
    {
        const uint32_t count = nct - 4u * w < 4u ? nct - 4u * w : 4u; // (4 w < S = nct)
        float2 p0{0.f, 0.f}, p1{0.f, 0.f};
        if constexpr (!BSC)
            p0 = box_muller(blk.x, blk.y), p1 = box_muller(blk.z, blk.w);
        uint64_t at[4], rat[4];
        double rcv[4], L[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const uint32_t i = 4u * w + k;
            const bool live = static_cast<uint32_t>(k) < count;
            const uint32_t col = live ? static_cast<uint32_t>(a.bit_pos[i]) : 0u;
            const int xb = live ? codeword_bit(a, frame, col) : 0;
            at[k] = frame * a.nc + col, rat[k] = frame * S + i;
            if constexpr (BSC)
            {
                const int y = xb ^ (counter_hit(word_of(blk, k), a.eps) ? 1 : 0);
                rcv[k] = static_cast<double>(1 - 2 * y);
                L[k] = a.delta * rcv[k];
            }
            else
            {
                const double noise = static_cast<double>(pick_normal(p0, p1, k)) * a.sigma + 0.0;
                const double xs = static_cast<double>(1 - 2 * xb);
                rcv[k] = noise + xs;
                L[k] = 2 * rcv[k] / a.sigma2;
            }
        }
        if (a.received)
            store_block<kLlrF64>(a.received, rat, rcv, count, 1.0, 1);
        if (a.llr)
            store_block<T>(a.llr, at, L, count, a.inv, a.qmax);
    }
    else
    {
        const float2 p0 = box_muller(blk.x, blk.y), p1 = box_muller(blk.z, blk.w);
        {
            // the constellation through the scalar path (wave-uniform), and the transmitted level by the lane's own index
            const auto lv = uniform_table(a.level);
            double level[kLevels];
#pragma unroll
            for (int j = 0; j < kLevels; ++j)
                level[j] = lv[j];
            const double two_sigma2 = 2 * a.sigma2;
#pragma unroll 1
            for (int k = 0; k < 4; ++k)
            {
                const uint32_t s = 4u * w + k;
                if (s >= S)
                    break;
                // the symbol's label: its M bits, the first most significant; a bit beyond nct - 1 counts as 0
                uint32_t col[M], label = 0;
#pragma unroll
                for (int q = 0; q < M; ++q)
                {
                    const uint32_t i = static_cast<uint32_t>(M) * s + q;
                    col[q] = i < nct ? static_cast<uint32_t>(a.bit_pos[i]) : 0xFFFFFFFFu;
                    label = (label << 1) | (i < nct ? static_cast<uint32_t>(codeword_bit(a, frame, col[q])) : 0u);
                }
                const uint32_t j = label ^ (label >> 1) ^ (label >> 2) ^ (label >> 3); // inverse Gray code: j ^ (j >> 1) == label
                const double noise = static_cast<double>(pick_normal(p0, p1, k)) * a.sigma + 0.0;
                const double y = noise + a.level[j];
                if (a.received)
                    a.received[frame * S + s] = y;
                if (!a.llr)
                    continue;
                double d[kLevels];
#pragma unroll
                for (int t = 0; t < kLevels; ++t)
                {
                    const double e = y - level[t];
                    d[t] = e * e;
                }
#pragma unroll
                for (int q = 0; q < M; ++q)
                {
                    // D0 / D1: the smallest distance over the levels whose label has bit q (first bit most significant) 0 / 1
                    double D0 = 0.0, D1 = 0.0;
                    bool have0 = false, have1 = false;
#pragma unroll
                    for (int t = 0; t < kLevels; ++t)
                    {
                        const int bit = ((t ^ (t >> 1)) >> (M - 1 - q)) & 1;
                        if (bit)
                            D1 = have1 ? (d[t] < D1 ? d[t] : D1) : d[t], have1 = true;
                        else
                            D0 = have0 ? (d[t] < D0 ? d[t] : D0) : d[t], have0 = true;
                    }
                    if (col[q] != 0xFFFFFFFFu)
                        store_llr<T>(a.llr, frame * a.nc + col[q], (D1 - D0) / two_sigma2, a.inv, a.qmax);
                }
            }
        }
    }
}

template <int M, bool BSC>
int launch_typed(const ChannelArgs &a, int type, dim3 grid, hipStream_t s)
{
    const dim3 block(kChannelThreads);
    switch (type)
    {
    case kLlrF64: hipLaunchKernelGGL((channel_kernel<M, kLlrF64, BSC>), grid, block, 0, s, a); break;
    case kLlrF32: hipLaunchKernelGGL((channel_kernel<M, kLlrF32, BSC>), grid, block, 0, s, a); break;
    case kLlrF16: hipLaunchKernelGGL((channel_kernel<M, kLlrF16, BSC>), grid, block, 0, s, a); break;
    case kLlrI8: hipLaunchKernelGGL((channel_kernel<M, kLlrI8, BSC>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
} // namespace

int launch_channel(const ChannelArgs &a, int bits_per_symbol, int llr_type, void *stream)
{
    if (a.n == 0 || (!a.llr && !a.received))
        return hipSuccess;
    const bool bsc = a.channel == 2;
    const int m = bits_per_symbol;
    if ((a.channel != 1 && !bsc) || m < 1 || m > kChannelMaxBitsPerSymbol || (bsc && m != 1) || !a.bit_pos || a.nc == 0 ||
        (a.n_other && !a.other) || (m > 1 && !a.level) || (a.codeword && !bits_format_known(a.codeword_format)) ||
        a.symbols != (a.nct + m - 1) / m || a.blocks != (a.symbols + 3) / 4 || a.work != a.blocks + a.n_other || a.work == 0 ||
        a.n * a.work >= (1ull << 31))
        return hipErrorInvalidValue;
    const uint64_t lanes = a.n * a.work;
    const dim3 grid(static_cast<unsigned>((lanes + kChannelThreads - 1) / kChannelThreads));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (bsc)
        return launch_typed<1, true>(a, llr_type, grid, s);
    switch (m)
    {
    case 1: return launch_typed<1, false>(a, llr_type, grid, s);
    case 2: return launch_typed<2, false>(a, llr_type, grid, s);
    case 3: return launch_typed<3, false>(a, llr_type, grid, s);
    default: return launch_typed<4, false>(a, llr_type, grid, s);
    }
}

} // namespace ldpc_amd
