// kernels_layered_fixed_impl.hpp — what the two translation units of fixed-point layered min-sum share: the quantizer and the
// check node here, and in kernels_layered_fixed_body.inc everything a frame does once its totals T[nc] stand in LDS (the
// sweeps, the syndrome check, the epilogue).
// kernels_layered_fixed.hip holds the instantiations that stage the binary64 channel LLRs in LDS first (every channel and
// noise mode), kernels_layered_fixed_direct.hip those that quantize typed LLRs straight from memory
// (ldpc_hip_decode_batch_typed).  Only the prologue, the LDS layout and the launch size differ between them.
#pragma once

#include <hip/hip_runtime.h>

#include "device_channel.hpp"
#include "device_math.hpp"
#include "kernels.hpp"
#include "launch_lds.hpp"

namespace ldpc_amd
{

namespace
{
constexpr int kLfThreads = 64; // one wave per workgroup, so that a CU takes as many frames as its LDS holds

// the frame's LDS is written as binary64 and read back as int16 and 32-bit words: these types alias everything
typedef int16_t __attribute__((may_alias)) lds_i16;
typedef uint32_t __attribute__((may_alias)) lds_u32;
typedef double __attribute__((may_alias)) lds_f64;

// clamp(rint(fl(llr * inv)), -qmax, +qmax), the clamp in binary64 (an infinity or 99999.9 saturates); rint is round-half-
// to-even; a NaN gives 0 (kernels_qms.hip, qms_quantize: the same quantizer)
__device__ __forceinline__ int lf_quantize(double llr, double inv, int qmax)
{
#pragma clang fp contract(off)
    const double x = __builtin_rint(llr * inv);
    const double q = static_cast<double>(qmax);
    return x >= q ? qmax : (x <= -q ? -qmax : (x == x ? static_cast<int>(x) : 0));
}

__device__ __forceinline__ int lf_clamp(int x, int m) // (a maximum and a minimum)
{
    const int lo = x < -m ? -m : x;
    return lo > m ? m : lo;
}
// -1 where bit j of x is set, else 0 (one signed one-bit field extract)
__device__ __forceinline__ int lf_bit_mask(uint32_t x, int j) { return -static_cast<int>((x >> j) & 1u); }
// a where mask is -1, b where it is 0
__device__ __forceinline__ int lf_sel(int mask, int a, int b) { return (a & mask) | (b & ~mask); }

__device__ __forceinline__ uint32_t vn_of(const uint32_t (&pk)[4], int j) { return (j & 1) ? pk[j >> 1] >> 16 : pk[j >> 1] & 0xFFFFu; }

// one check node of degree D on this lane: T = the frame's totals, pk = its neighbours' VN ranks (two per word), rec = its
// record
template <int D>
__device__ __forceinline__ void cn_layered_fixed(lds_i16 *T, lds_u32 *rec, const uint8_t *lut, const uint32_t (&pk)[4], int qmax, int pmax)
{
    // Written without a comparison per edge: a compare that feeds a select costs the pair and the wait between them, and the
    // kernel is bound by the instructions it issues (17 waves on a CU keep the LDS latency covered).  Masks are 0 or -1:
    // (x ^ mask) - mask negates under the mask, sel() picks by it; the minimum, the runner-up and the argmin come from
    // KEYS |u| << 3 | j (the smallest key holds the smallest |u| and an edge that has it).
    const uint32_t o = *rec;
    const int o_rest = static_cast<int>(o & 127u), o_arg = static_cast<int>((o >> 7) & 127u);
    const uint32_t o_hot = 1u << ((o >> 14) & 7u); // bit argmin
    const int o_neg = static_cast<int>(o >> 17);
    uint32_t n[D];
    int t[D];
#pragma unroll
    for (int j = 0; j < D; ++j)
        n[j] = vn_of(pk, j);
    uint32_t key1 = 127u << 3, key2 = 127u << 3; // (|u| <= qmax <= 127)
    int signs = 0, sx = 0;
#pragma unroll
    for (int j = 0; j < D; ++j)
    {
        const int mo = lf_sel(lf_bit_mask(o_hot, j), o_arg, o_rest);
        const int neg = lf_bit_mask(o_neg, j);
        const int m = (mo ^ neg) - neg;
        t[j] = static_cast<int>(T[n[j]]) - m; // what the neighbour says without this node's last message: exact
        const int u = lf_clamp(t[j], qmax); // ... at message width
        const int s = u >> 31;              // -1 where u < 0 (an integer zero is not negative)
        const uint32_t key = static_cast<uint32_t>((u ^ s) - s) << 3 | static_cast<uint32_t>(j);
        signs |= s & (1 << j), sx ^= s;
        const uint32_t hi = key > key1 ? key : key1;
        key1 = key < key1 ? key : key1;
        key2 = hi < key2 ? hi : key2;
    }
    const int r_rest = lut[key1 >> 3], r_arg = lut[key2 >> 3];
    const uint32_t k = key1 & 7u, hot = 1u << k;
    const int out_signs = (signs ^ sx) & ((1 << D) - 1); // edge j: negative iff an odd number of the others is
#pragma unroll
    for (int j = 0; j < D; ++j)
    {
        const int mo = lf_sel(lf_bit_mask(hot, j), r_arg, r_rest);
        const int neg = lf_bit_mask(out_signs, j);
        T[n[j]] = static_cast<int16_t>(lf_clamp(t[j] + ((mo ^ neg) - neg), pmax));
    }
    *rec = static_cast<uint32_t>(r_rest) | static_cast<uint32_t>(r_arg) << 7 | k << 14 | static_cast<uint32_t>(out_signs) << 17;
}

template <int D>
__device__ __forceinline__ uint32_t cn_parity_fixed(const lds_i16 *T, const uint32_t (&pk)[4])
{
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < D; ++j)
        p ^= static_cast<uint32_t>(T[vn_of(pk, j)] <= 0); // decoder.cpp:58: out <= 0 decides 1
    return p;
}

// the correction table of the launch arguments into the frame's LDS, four magnitudes per lane
__device__ __forceinline__ void lf_load_lut(const LayeredFixedArgs &q, uint8_t *lut, int lane)
{
    if (lane < 32) // (a select chain over the launch arguments: indexing them by a lane's number would put them in scratch)
    {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i)
            w = lane == i ? q.lut[i] : w;
        reinterpret_cast<lds_u32 *>(lut)[lane] = w;
    }
}

} // namespace

} // namespace ldpc_amd
