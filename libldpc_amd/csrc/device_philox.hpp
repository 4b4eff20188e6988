// device_philox.hpp — the counter-based noise of the opt-in NON-PARITY noise mode (include/ldpc_amd.h, ldpc_hip_set_noise).
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11): key (seed & 0xFFFFFFFF,
// seed >> 32), counter (block, frame & 0xFFFFFFFF, frame >> 32, tag).  A frame's noise is a pure function of (seed, frame
// index since stream_begin, bit index): no stream position, no jump-ahead, nothing exchanged between ranks.
//   AWGN (tag 0)      transmitted bit i: normal i % 4 of block i / 4 — two Box–Muller pairs per block, binary32 hardware
//                     log / sqrt / sin / cos; u = (w + 0.5) / 2^32 >= 2^-33 bounds a pair's radius by sqrt(66 ln 2) = 6.764
//   BSC / BEC (tag 1) transmitted bit i: word i % 4 of block i / 4, flipped / erased when (w + 0.5) / 2^32 < eps (binary64, exact)
//   encoder (tag 2)   info bit j: bit j % 32 of word (j / 32) % 4 of block j / 128
// The key is wave-uniform (scalar registers); only the block and frame words vary per lane.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace ldpc_amd
{

enum CounterTag : uint32_t
{
    kTagAwgn = 0,
    kTagDraw = 1, // BSC / BEC
    kTagInfo = 2, // encoder info bits
    kTagFlip = 3, // bit flipping: the draw of column v in round t is word v % 4 of block t * ceil(nc / 4) + v / 4
    kTagRelay = 4, // relay decoding's gamma table (drawn on the host side, binding.py relay_gammas): row l is frame l,
                   // column v word v % 4 of block v / 4
};

__host__ __device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r)
    {
        if (r > 0)
            k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0, p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
        const uint32_t hi0 = static_cast<uint32_t>(p0 >> 32), lo0 = static_cast<uint32_t>(p0);
        const uint32_t hi1 = static_cast<uint32_t>(p1 >> 32), lo1 = static_cast<uint32_t>(p1);
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
    }
    return uint4{c0, c1, c2, c3};
}

// block b of frame f (f: index since stream_begin) under tag
__device__ __forceinline__ uint4 philox_block(uint32_t k0, uint32_t k1, uint64_t frame, uint32_t b, uint32_t tag)
{
    return philox4x32_10(b, static_cast<uint32_t>(frame), static_cast<uint32_t>(frame >> 32), tag, k0, k1);
}

// One Box–Muller pair from two words (binary32): u = (w0 + 0.5) / 2^32, t = w1 / 2^32 revolutions;
// n0 = sqrt(-2 ln u) cos 2 pi t, n1 = sqrt(-2 ln u) sin 2 pi t.  (v_log_f32 is log2, v_sin / v_cos take revolutions.)
__device__ __forceinline__ float2 box_muller(uint32_t w0, uint32_t w1)
{
    const float u = __builtin_fmaf(static_cast<float>(w0), 0x1p-32f, 0x1p-33f); // (the product is exact: one rounding)
    const float t = static_cast<float>(w1) * 0x1p-32f;
    const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u)); // -2 ln u = -2 ln 2 log2 u
    return float2{r * __builtin_amdgcn_cosf(t), r * __builtin_amdgcn_sinf(t)};
}

// normal k (0..3) of a block's words (one pair evaluated)
__device__ __forceinline__ float counter_normal(const uint4 &w, int k)
{
    const float2 p = box_muller(k < 2 ? w.x : w.z, k < 2 ? w.y : w.w);
    return (k & 1) ? p.y : p.x;
}
// normal k of a block whose two pairs are evaluated already
__device__ __forceinline__ float pick_normal(const float2 &p0, const float2 &p1, int k)
{
    return k == 0 ? p0.x : (k == 1 ? p0.y : (k == 2 ? p1.x : p1.y));
}

__device__ __forceinline__ uint32_t word_of(const uint4 &w, int k) { return k == 0 ? w.x : (k == 1 ? w.y : (k == 2 ? w.z : w.w)); }

// (w + 0.5) / 2^32 < eps, exactly
__device__ __forceinline__ bool counter_hit(uint32_t w, double eps) { return (static_cast<double>(w) + 0.5) * 0x1p-32 < eps; }

// The noise sources a channel prologue is compiled for: the reference's stream only (every parity kernel: exactly its own
// code, no branch it does not need), the counter-based modes only (the counter-mode instantiations of the hot kernels), or
// both behind a runtime branch on a.mode (the kernels that serve few frames: lists, redo launches, other residencies).
enum NoiseKinds : int
{
    kNoiseStream = 0,
    kNoiseCounter = 1,
    kNoiseAny = 2,
};
template <int NK>
__device__ __forceinline__ bool counter_mode(const DecodeArgs &a)
{
    return NK == kNoiseCounter || (NK == kNoiseAny && (a.mode == kModeAwgnCtr || a.mode == kModeBscCtr));
}

} // namespace ldpc_amd
