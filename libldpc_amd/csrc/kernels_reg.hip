// kernels_reg.hip — register-resident BP / min-sum decoder for codes whose messages do not fit LDS four
// frames at a time (BASELINE config 4: (3,6)-regular n=8192, 196 KB of fp64 messages per frame).
//
// One workgroup of NT threads decodes one frame (NT = 512: two frames per CU, so that one frame's LDS
// exchange overlaps the other's arithmetic; NT = 1024: one).  The frame's messages live in the register file:
// thread (wave, lane) owns the check nodes of CN blocks k*(NT/64) + wave (k < KC) and holds their KC x MAXD messages
// in m[k][j] for the whole decode, so the check-node pass — 80 % of the arithmetic — touches no memory at all.
// The variable-node side is reached through an LDS mailbox laid out VN-block-major: CN threads scatter c2v,
// VN threads read their column contiguously ([position][lane]: conflict-free), form the APP in column file
// order, write v2c and the hard decision back in place, CN threads gather.  A code whose edges exceed the
// mailbox (160 KB = 18 176 entries of 8+1 bytes) is exchanged in rounds of VN blocks.  Input LLRs and per-VN
// hard decisions sit in device memory (read / written once per VN per iteration, coalesced).
//
// Same arithmetic, same order as the LDS-resident kernel (kernels.hip) and as the reference:
//   decode loop src/decoding/decoder.cpp:11-78, CN recursion :31-44 (device_cn.hpp), VN sum :50-56 in column
//   file order, syndrome src/decoding/decoder.h:47-64, channels src/sim/channel.cpp (device_channel.hpp).
#include <hip/hip_runtime.h>

#include <utility>

#include "device_channel.hpp"
#include "device_cn.hpp"
#include "device_math.hpp"
#include "kernels.hpp"
#include "launch_lds.hpp"

namespace ldpc_amd
{

namespace
{

// (the shared-reciprocal form of detmath.h belongs to the LDS-resident decoder: its range check rides on that kernel's
// check-node-first loop; here every output is divided separately)
// SH6: first launch of three — check nodes of degree 6 share reciprocals (detmath.h, dm_cn6_shared); their products' range
// check joins `escaped`, voted on after the variable-node pass that follows
template <bool MINSUM, bool RATIO, int MAXD, bool SH6, bool CORR = false>
__device__ __forceinline__ void cn_regs(double (&m)[MAXD], int degree, uint32_t *escaped, MsCorr c = MsCorr{1.0, 0.0})
{
    // wave-uniform degree: one fully unrolled recursion per width
#define LDPC_CASE(D)                         \
    case D:                                  \
    {                                        \
        double v[D];                         \
        _Pragma("unroll") for (int j = 0; j < D; ++j) v[j] = m[j]; \
        if constexpr (RATIO)                 \
            cn_ratio<D, false, SH6>(v, nullptr, escaped); \
        else                                 \
            cn_core<D, MINSUM, CORR>(v, c);  \
        _Pragma("unroll") for (int j = 0; j < D; ++j) m[j] = v[j]; \
        break;                               \
    }
    switch (degree)
    {
        LDPC_CASE(2)
        LDPC_CASE(3)
    default:
        if constexpr (MAXD >= 4)
            switch (degree)
            {
                LDPC_CASE(4)
            default:
                if constexpr (MAXD >= 6)
                    switch (degree)
                    {
                        LDPC_CASE(5)
                        LDPC_CASE(6)
                    default:
                        if constexpr (MAXD >= 8)
                            switch (degree)
                            {
                                LDPC_CASE(7)
                                LDPC_CASE(8)
                            default: break;
                            }
                        break;
                    }
                break;
            }
        break;
    }
#undef LDPC_CASE
}

// RATIO: the likelihood-ratio form of the sum-product iteration, exactly as in kernels.hip (v2c = rho, c2v = lambda,
// input LLRs kept as lambda; frames that leave the representable box go to a.redo_list).
template <bool MINSUM, bool WANT_LLR, int NT, int KC, int MAXD, bool RATIO, bool SH6 = false>
__global__ __launch_bounds__(NT) void decode_reg_kernel(const DecodeArgs a, const DevRegPlan R)
{
    constexpr bool CORR = false;
#include "kernels_reg_body.inc"
}

// corrected min-sum (device_cn.hpp, MsCorr; NON-PARITY): the min-sum kernel with the correction on every check node's inputs
template <bool WANT_LLR, int NT, int KC, int MAXD>
__global__ __launch_bounds__(NT) void decode_reg_msc_kernel(const DecodeArgs a, const DevRegPlan R)
{
    constexpr bool MINSUM = true, RATIO = false, SH6 = false, CORR = true;
#include "kernels_reg_body.inc"
}

using RegKernel = void (*)(const DecodeArgs, const DevRegPlan);

// the kernel of a stage (null: none here).  The first ratio launch shares the reciprocals of degree-6 check nodes (SH6); the
// second, over its list, divides every output separately.
template <bool WANT_LLR, int NT, int KC, int MAXD>
RegKernel reg_kernel_of(Stage stage, bool min_sum, bool ms_correct)
{
    switch (stage)
    {
    case Stage::kWhole:
        if (min_sum)
            return ms_correct ? decode_reg_msc_kernel<WANT_LLR, NT, KC, MAXD> : decode_reg_kernel<true, WANT_LLR, NT, KC, MAXD, false>;
        [[fallthrough]];
    case Stage::kLlrRedo:
        return decode_reg_kernel<false, WANT_LLR, NT, KC, MAXD, false>;
    case Stage::kRatioFirst:
        return decode_reg_kernel<false, WANT_LLR, NT, KC, MAXD, true, MAXD >= 6>;
    case Stage::kRatioSeparate:
        return decode_reg_kernel<false, WANT_LLR, NT, KC, MAXD, true>;
    default:
        return nullptr;
    }
}

template <int NT, int KC, int MAXD>
int launch_reg(const DecodeArgs &a, const DevRegPlan &r, Stage stage, bool min_sum, void *stream)
{
    if (!stage_args_ok(a, stage) || (min_sum && stage != Stage::kWhole))
        return hipErrorInvalidValue;
    const RegKernel k = a.llr_out ? reg_kernel_of<true, NT, KC, MAXD>(stage, min_sum, a.ms_correct)
                                  : reg_kernel_of<false, NT, KC, MAXD>(stage, min_sum, a.ms_correct);
    if (!k)
        return hipErrorInvalidValue;
    const uint32_t lds = r.mb_doubles * 9u;
    return launch_with_lds(k, dim3(static_cast<unsigned>(a.n_frames)), dim3(NT), lds, stream, a, r);
}

} // namespace

int launch_decode_reg(const DecodeArgs &a, const DevRegPlan &r, Stage stage, bool min_sum, void *stream)
{
    if (a.n_frames == 0)
        return hipSuccess;
    if (!a.ws_llr || !a.ws_hb)
        return hipErrorInvalidValue;
#define LDPC_TILE(N, K, D)                      \
    if (r.nt == N && r.kc == K && r.maxd == D)  \
        return launch_reg<N, K, D>(a, r, stage, min_sum, stream);
    LDPC_TILE(512, 8, 6)
    LDPC_TILE(512, 16, 4)
    LDPC_TILE(512, 4, 8)
    LDPC_TILE(1024, 4, 6)
    LDPC_TILE(1024, 8, 4)
    LDPC_TILE(1024, 2, 8)
#undef LDPC_TILE
    return hipErrorInvalidValue;
}

} // namespace ldpc_amd
