// selftest.hip — the device arithmetic of detmath.h / device_cn.hpp evaluated element by element, so that tests can
// hold it against values computed by glibc's libm and by extended-precision host arithmetic (tests/test_gpu_math.py)
// instead of against the same header compiled for the host.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_cn.hpp"
#include "device_math.hpp"
#include "kernels.hpp"

namespace ldpc_amd
{

namespace
{

template <int D>
__device__ void cn_ratio_rows(uint64_t i, const double *a, double *out)
{
    double v[D];
#pragma unroll
    for (int j = 0; j < D; ++j)
        v[j] = a[i * D + j];
    cn_ratio<D>(v);
#pragma unroll
    for (int j = 0; j < D; ++j)
        out[i * D + j] = v[j];
}

template <int D>
__device__ void cn_shared_rows(uint64_t i, const double *a, double *out)
{
    double v[D];
#pragma unroll
    for (int j = 0; j < D; ++j)
        v[j] = a[i * D + j];
    uint32_t escaped = 0;
    cn_ratio<D, D != 6, D == 6>(v, &escaped, &escaped);
#pragma unroll
    for (int j = 0; j < D; ++j)
        out[i * D + j] = DM_RATIO_ESCAPED(escaped) ? __builtin_nan("") : v[j];
}

template <int D>
__device__ void cn_llr_rows(uint64_t i, const double *a, double *out)
{
    double v[D];
#pragma unroll
    for (int j = 0; j < D; ++j)
        v[j] = a[i * D + j];
    cn_core<D, false>(v);
#pragma unroll
    for (int j = 0; j < D; ++j)
        out[i * D + j] = v[j];
}

// one node of the fused form with its class as literals, as the kernels' cnf_call has them (kernels_fused.hip)
template <int D, unsigned FLIP, bool LEAF, bool SHARED>
__device__ __forceinline__ uint32_t cnf_node(double (&v)[D], uint32_t &lb, double &tot)
{
    if constexpr (D == 2)
        return dm_cnf2(v, FLIP);
    else if constexpr (D == 3)
        return dm_cnf3(v, FLIP, LEAF, SHARED, &lb, &tot);
    else
        return dm_cnf4(v, FLIP, LEAF, SHARED, &lb, &tot);
}

// rows {v_0 .. v_{D-1}, flip | leaf << 4, 0} -> {m_0 .. m_{D-1}, leaf_bit, leaf_tot} (kernels.hpp, kMathCnf2); the classes are
// the nineteen fused_rule.h admits: flipped inputs last among the message inputs, the leaf (its rho_ch) last of all
template <int D, bool SHARED>
__device__ void cnf_rows(uint64_t i, const double *a, double *out)
{
    constexpr int W = D + 2;
    const double nan = __builtin_nan("");
    double v[D];
#pragma unroll
    for (int j = 0; j < D; ++j)
        v[j] = a[i * W + j];
    const unsigned mode = static_cast<unsigned>(a[i * W + D]);
    uint32_t lb = 0, h = 0xFFFFFFFFu; // an unknown class: the row comes back as NaN
    double tot = nan;
#define CNF_CLASS(flip, leaf) \
    case (flip) | ((leaf) << 4): h = cnf_node<D, flip, leaf, SHARED>(v, lb, tot); break;
    if constexpr (D == 2)
        switch (mode)
        {
            CNF_CLASS(0u, 0) CNF_CLASS(2u, 0) CNF_CLASS(3u, 0)
        default: break;
        }
    else if constexpr (D == 3)
        switch (mode)
        {
            CNF_CLASS(0u, 0) CNF_CLASS(4u, 0) CNF_CLASS(6u, 0) CNF_CLASS(7u, 0)
            CNF_CLASS(0u, 1) CNF_CLASS(2u, 1) CNF_CLASS(3u, 1)
        default: break;
        }
    else
        switch (mode)
        {
            CNF_CLASS(0u, 0) CNF_CLASS(8u, 0) CNF_CLASS(12u, 0) CNF_CLASS(14u, 0) CNF_CLASS(15u, 0)
            CNF_CLASS(0u, 1) CNF_CLASS(4u, 1) CNF_CLASS(6u, 1) CNF_CLASS(7u, 1)
        default: break;
        }
#undef CNF_CLASS
    const bool over = h >= DM_FUSED_P_HI;
#pragma unroll
    for (int j = 0; j < D; ++j)
        out[i * W + j] = over ? nan : v[j];
    out[i * W + D] = over ? nan : static_cast<double>(lb);
    out[i * W + D + 1] = over ? nan : tot;
}

// the range predicates of detmath.h as a bit mask, in the order tests/test_gpu_math.py lists them
__device__ double predicate_mask(double x)
{
    const uint32_t hi = dm_hi(x);
    unsigned m = 0;
    m |= static_cast<unsigned>(dm_ratio_out_of_range(x) != 0) << 0;
    m |= static_cast<unsigned>(DM_RATIO_ESCAPED(dm_ratio_key(x))) << 1;
    m |= static_cast<unsigned>(dm_box_escaped(hi, hi) != 0) << 2;
    m |= static_cast<unsigned>(DM_SHARED_OVERFLOW(hi)) << 3;
    m |= static_cast<unsigned>(hi >= DM_FUSED_P_HI) << 4;
    m |= static_cast<unsigned>(DM_HANDOVER_DUE(dm_handover_key(x))) << 5;
    m |= static_cast<unsigned>(dm_ratio_llr_refused(x) != 0) << 6;
    m |= static_cast<unsigned>(dm_llr_tiny(__builtin_fabs(x)) != 0) << 7;
    return static_cast<double>(m);
}

__global__ __launch_bounds__(256) void math_selftest_kernel(int fn, uint64_t n, const double *a, const double *b, double *out)
{
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n)
        return;
    switch (fn)
    {
    case kMathExp: out[i] = dm_exp(a[i]); break;
    case kMathLog: out[i] = dm_log(a[i]); break;
    case kMathBoxplus: out[i] = box_jacobian(a[i], b[i]); break; // what the kernels call: dm_boxplus + its short cut
    case kMathRatioDiv: out[i] = dm_ratio_div(a[i], b[i]); break;
    case kMathRatioRho: out[i] = dm_ratio_rho(a[i], b[i]); break;
    case kMathRatioLambda: out[i] = dm_ratio_lambda(a[i], b[i]); break;
    case kMathECombine: out[i] = dm_e_combine(a[i], b[i]); break;
    case kMathExpClamped: out[i] = dm_exp_clamped(a[i]); break;
    case kMathBoxplusExp: out[i] = dm_boxplus_exp(a[i]); break;
    case kMathBoxplusLog: out[i] = dm_boxplus_log(a[i]); break;
    case kMathCnRatio3: cn_ratio_rows<3>(i, a, out); break;
    case kMathCnRatio4: cn_ratio_rows<4>(i, a, out); break;
    case kMathCnRatio5: cn_ratio_rows<5>(i, a, out); break;
    case kMathCnRatio6: cn_ratio_rows<6>(i, a, out); break;
    case kMathCnRatio8: cn_ratio_rows<8>(i, a, out); break;
    case kMathCnLlr4: cn_llr_rows<4>(i, a, out); break;
    case kMathCnLlr6: cn_llr_rows<6>(i, a, out); break;
    case kMathCnRatio3s: cn_shared_rows<3>(i, a, out); break;
    case kMathCnRatio4s: cn_shared_rows<4>(i, a, out); break;
    case kMathCnRatio6s: cn_shared_rows<6>(i, a, out); break;
    case kMathCnf2: cnf_rows<2, true>(i, a, out); break;
    case kMathCnf3: cnf_rows<3, true>(i, a, out); break;
    case kMathCnf4: cnf_rows<4, true>(i, a, out); break;
    case kMathCnf3d: cnf_rows<3, false>(i, a, out); break;
    case kMathCnf4d: cnf_rows<4, false>(i, a, out); break;
    case kMathCnLlr3: cn_llr_rows<3>(i, a, out); break;
    case kMathCnLlr5: cn_llr_rows<5>(i, a, out); break;
    case kMathCnLlr16: cn_llr_rows<16>(i, a, out); break;
    case kMathPredicates: out[i] = predicate_mask(a[i]); break;
    default: break;
    }
}

// operands a = 2^ea * ma, b = 2^eb * mb with ea, eb in [-500, 500] and random mantissas: a, b, a/b inside 2^-+1001
__global__ __launch_bounds__(256) void division_selftest_kernel(uint64_t n, uint64_t seed, unsigned long long *mismatches)
{
    unsigned long long bad = 0;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull)
    {
        uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull ^ seed;
        auto next = [&] {
            x ^= x >> 12, x ^= x << 25, x ^= x >> 27;
            return x * 0x2545F4914F6CDD1Dull;
        };
        auto operand = [&] {
            const uint64_t m = next() >> 12, e = 1023 - 500 + (next() >> 33) % 1001;
            return dm_from_bits((e << 52) | m);
        };
        const double a = operand(), b = operand();
        volatile double bv = b; // keep the compiler from folding the two forms together
        bad += dm_bits(dm_ratio_div(a, b)) != dm_bits(a / bv);
        // dm_div_by (detmath.h): numerators of either sign up to 2^8 over divisors in [2^-7, 2^7] with THEIR correctly rounded
        // reciprocal (here: the device's own IEEE division, which is correctly rounded) — the channel's 2 y / sigma^2
        const uint64_t m2 = next() >> 12, e2 = 1023 - 7 + (next() >> 33) % 15;
        const double d = dm_from_bits((e2 << 52) | m2);
        volatile double dv = d;
        const double rcp = 1.0 / dv;
        const uint64_t m3 = next() >> 12, e3 = 1023 - 60 + (next() >> 33) % 69, s3 = next() >> 63;
        const double num = dm_from_bits((s3 << 63) | (e3 << 52) | m3);
        bad += dm_bits(dm_div_by(num, d, rcp)) != dm_bits(num / dv);
    }
    if (bad)
        atomicAdd(mismatches, bad);
}

} // namespace

int math_selftest_width(int fn)
{
    switch (fn)
    {
    case kMathCnRatio3: case kMathCnRatio3s: case kMathCnLlr3: return 3;
    case kMathCnRatio4: case kMathCnLlr4: case kMathCnRatio4s: case kMathCnf2: return 4;
    case kMathCnRatio5: case kMathCnLlr5: case kMathCnf3: case kMathCnf3d: return 5;
    case kMathCnRatio6: case kMathCnLlr6: case kMathCnRatio6s: case kMathCnf4: case kMathCnf4d: return 6;
    case kMathCnRatio8: return 8;
    case kMathCnLlr16: return 16;
    default: return fn >= 0 && fn < kMathCount ? 1 : 0;
    }
}

int launch_math_selftest(int fn, uint64_t n, const double *a, const double *b, double *out, void *stream)
{
    if (n == 0)
        return hipSuccess;
    const unsigned blocks = static_cast<unsigned>((n + 255) / 256);
    hipLaunchKernelGGL(math_selftest_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), fn, n, a, b, out);
    return hipGetLastError();
}

int launch_division_selftest(uint64_t n, uint64_t seed, unsigned long long *mismatches, void *stream)
{
    if (n == 0)
        return hipSuccess;
    const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, 8192));
    hipLaunchKernelGGL(division_selftest_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), n, seed,
                       mismatches);
    return hipGetLastError();
}

} // namespace ldpc_amd
