// kernels_layered_ms.hip — opt-in NON-PARITY LAYERED (row-serial) schedule of min-sum decoding ("BP_MS" with
// ldpc_hip_set_min_sum_schedule(LDPC_HIP_MS_SCHEDULE_LAYERED); include/ldpc_amd.h states the arithmetic).  Plain, normalized
// and offset min-sum (ldpc_hip_set_min_sum_correction) in binary64: no transcendental, every operation rounded once, so
// every output bit follows from the schedule and is held against a numpy mirror bit for bit
// (tests/layered_minsum_ref.py).  The reference's schedule is flooding (decoder.cpp:22-76): the results are not its own.
//
// Mapping as in kernels_layered.hip: ONE WAVE = ONE FRAME, a sweep is the sequence of STEPS of build_layer_plan (plan.cpp),
// a step is up to 64 check nodes of equal degree that share no variable node, one per lane; the steps need no barrier (a
// wave's LDS operations execute in order) and a step's neighbour table is fetched one step ahead.
//
// What LDS holds per frame:
//   * the totals T[nc], binary64 — the array the channel writes its LLRs into IS the totals array, no conversion pass;
//   * per check node a RECORD instead of its D messages.  The outputs of a min-sum check node take two magnitudes only:
//     every edge but the one that holds the smallest input gets f(min1), that edge gets f(min2), f the correction.  The
//     record is {f(min1), f(min2), one word: argmin position in bits 0..2, the D output sign bits from bit 3 on}; message j
//     is (j == argmin ? f(min2) : f(min1)) with sign bit j — exactly the message a full array would hold (where two inputs
//     tie for the minimum, min2 == min1 and either argmin gives the same values).  20 bytes per check node whatever its
//     degree, laid out [field][lane] within a step (consecutive lanes, consecutive banks) over the step's REAL check nodes
//     (rounded up to an even number, which keeps every step 8-byte aligned): h.txt 29 KB per frame, five frames per CU; the
//     n = 8192 (3,6) code 144 KB, one.
//
// Iteration count returned: sweeps completed before the sweep whose syndrome check passed (the reference's convention,
// decoder.cpp:21-22,74-77); the syndrome of the current decisions is taken after every sweep.
#include <hip/hip_runtime.h>

#include "device_channel.hpp"
#include "device_cn.hpp"
#include "device_math.hpp"
#include "kernels.hpp"
#include "launch_lds.hpp"

namespace ldpc_amd
{

namespace
{
constexpr int kLmsThreads = 64; // one wave per workgroup, so that a CU takes as many frames as its LDS holds

// max(fl(fl(scale * m) - offset), +0.0) of a non-negative magnitude (device_cn.hpp, ms_correct; (1, 0) returns m)
__device__ __forceinline__ double lms_correct(double m, MsCorr c)
{
#pragma clang fp contract(off)
    const double t = m * c.scale;
    const double r = t - c.offset;
    return r > 0.0 ? r : 0.0;
}

__device__ __forceinline__ uint32_t vn_of(const uint32_t (&pk)[4], int j) { return (j & 1) ? pk[j >> 1] >> 16 : pk[j >> 1] & 0xFFFFu; }

// one check node of degree D on this lane: T = the frame's totals, pk = its neighbours' VN ranks (two per word), rec = the
// step's records ([field][lane], `cnt` lanes per field: two fields of 8 bytes, one of 4)
template <int D>
__device__ __forceinline__ void cn_layered_ms(double *T, unsigned char *rec, uint32_t cnt, int lane, const uint32_t (&pk)[4], MsCorr c)
{
    double *mag_rest = reinterpret_cast<double *>(rec) + lane;
    double *mag_arg = mag_rest + cnt;
    uint32_t *word = reinterpret_cast<uint32_t *>(rec + 16 * cnt) + lane;
    const double o_rest = *mag_rest, o_arg = *mag_arg;
    const uint32_t o_w = *word;
    uint32_t n[D];
    double t[D];
#pragma unroll
    for (int j = 0; j < D; ++j)
        n[j] = vn_of(pk, j);
    double min1 = __builtin_huge_val(), min2 = __builtin_huge_val();
    uint32_t k = 0, signs = 0, sx = 0;
#pragma unroll
    for (int j = 0; j < D; ++j)
    {
        const double mo = (o_w & 7u) == static_cast<uint32_t>(j) ? o_arg : o_rest;
        const double m = dm_from_bits(dm_bits(mo) | (static_cast<uint64_t>((o_w >> (3 + j)) & 1u) << 63));
        t[j] = T[n[j]] - m; // what the neighbour says without this node's last message
        const double a = __builtin_fabs(t[j]);
        const uint32_t s = static_cast<uint32_t>(dm_bits(t[j]) >> 63);
        signs |= s << j, sx ^= s;
        const bool lt = a < min1;
        min2 = lt ? min1 : (a < min2 ? a : min2);
        k = lt ? static_cast<uint32_t>(j) : k;
        min1 = lt ? a : min1;
    }
    const double r_rest = lms_correct(min1, c), r_arg = lms_correct(min2, c);
    const uint32_t out_signs = signs ^ (sx ? (1u << D) - 1u : 0u); // edge j: XOR of the other edges' sign bits
#pragma unroll
    for (int j = 0; j < D; ++j)
    {
        const double mo = k == static_cast<uint32_t>(j) ? r_arg : r_rest;
        const double m = dm_from_bits(dm_bits(mo) | (static_cast<uint64_t>((out_signs >> j) & 1u) << 63));
        T[n[j]] = t[j] + m;
    }
    *mag_rest = r_rest, *mag_arg = r_arg, *word = k | out_signs << 3;
}

template <int D>
__device__ __forceinline__ uint32_t cn_parity_ms(const double *T, const uint32_t (&pk)[4])
{
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < D; ++j)
        p ^= static_cast<uint32_t>(T[vn_of(pk, j)] <= 0.0); // decoder.cpp:58: out <= 0 decides 1
    return p;
}

template <bool WANT_LLR>
__global__ __launch_bounds__(kLmsThreads) void decode_layered_ms_kernel(const DecodeArgs a, const DevLayerPlan L)
{
    extern __shared__ double lds_d[];
    const DevPlan &P = a.plan;
    const int nc = P.nc;
    const int lane = threadIdx.x;
    const uint64_t frame = blockIdx.x;
    if (frame >= a.n_frames)
        return;
    double *T = lds_d;
    unsigned char *records = reinterpret_cast<unsigned char *>(T + nc);
    const uint8_t *cw = a.codeword ? a.codeword + frame * nc : nullptr;
    const MsCorr corr{a.ms_scale, a.ms_offset};

    channel_init<64, kNoiseAny>(a, frame, T, lane); // binary64 channel + LLR initialisation, as everywhere (one wave's worth)
    __builtin_amdgcn_wave_barrier();
    if (a.llr_in_dump)
    {
        double *o = a.llr_in_dump + frame * nc;
        for (int r = lane; r < nc; r += 64)
            o[P.rank_col[r]] = T[r];
    }
    {
        uint32_t *z = reinterpret_cast<uint32_t *>(records);
        for (uint32_t i = lane; i < L.record_bytes / 4; i += 64)
            z[i] = 0; // every message +0.0: magnitudes 0, argmin 0, no sign bit
    }
    __builtin_amdgcn_wave_barrier();

    // the step's neighbour table one step AHEAD (kernels_layered.hip)
    const auto steps = uniform_table(reinterpret_cast<const uint32_t *>(L.steps));
    const auto rec_off = uniform_table(L.rec_off);
    const uint32_t *table = L.vn4 + lane;
    auto fetch = [&](uint32_t s, uint32_t (&pk)[4]) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
            pk[w] = table[(s * 4 + w) * 64];
    };
    uint32_t I = 0;
    uint32_t nxt[4];
    fetch(0, nxt);
    while (I < a.iterations)
    {
        for (uint32_t s = 0; s < L.n_steps; ++s)
        {
            uint32_t cur[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
            fetch(s + 1 < L.n_steps ? s + 1 : 0, nxt); // (the sweep's last step fetches the first one's)
            const uint32_t cd = steps[2 * s + 1], ro = rec_off[s];
            const int count = cd & 0xFFFF, degree = cd >> 16;
            const uint32_t cnt = (count + 1u) & ~1u; // lanes per field of the step's records
            if (lane < count)
            {
                unsigned char *rec = records + ro;
                switch (degree) // wave-uniform
                {
                case 2: cn_layered_ms<2>(T, rec, cnt, lane, cur, corr); break;
                case 3: cn_layered_ms<3>(T, rec, cnt, lane, cur, corr); break;
                case 4: cn_layered_ms<4>(T, rec, cnt, lane, cur, corr); break;
                case 5: cn_layered_ms<5>(T, rec, cnt, lane, cur, corr); break;
                case 6: cn_layered_ms<6>(T, rec, cnt, lane, cur, corr); break;
                case 7: cn_layered_ms<7>(T, rec, cnt, lane, cur, corr); break;
                case 8: cn_layered_ms<8>(T, rec, cnt, lane, cur, corr); break;
                default: break;
                }
            }
            __builtin_amdgcn_wave_barrier(); // (LDS operations of a wave execute in order; this only stops the compiler)
        }
        // syndrome of the decisions after this sweep (decoder.cpp:66-72)
        if (a.early_term)
        {
            uint32_t bad = 0;
            for (uint32_t s = 0; s < L.n_steps; ++s)
            {
                uint32_t cur[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
                fetch(s + 1 < L.n_steps ? s + 1 : 0, nxt);
                const uint32_t cd = steps[2 * s + 1];
                const int count = cd & 0xFFFF, degree = cd >> 16;
                if (lane < count)
                {
                    switch (degree)
                    {
                    case 2: bad |= cn_parity_ms<2>(T, cur); break;
                    case 3: bad |= cn_parity_ms<3>(T, cur); break;
                    case 4: bad |= cn_parity_ms<4>(T, cur); break;
                    case 5: bad |= cn_parity_ms<5>(T, cur); break;
                    case 6: bad |= cn_parity_ms<6>(T, cur); break;
                    case 7: bad |= cn_parity_ms<7>(T, cur); break;
                    case 8: bad |= cn_parity_ms<8>(T, cur); break;
                    default: break;
                    }
                }
            }
            if (__ballot(bad != 0) == 0)
                break;
        }
        ++I;
    }
    if (lane == 0 && a.iters)
        a.iters[frame] = I;
    const bool ran = a.iterations > 0;
    uint8_t *h = a.hard ? a.hard + frame * nc : nullptr;
    for (int r = lane; r < nc; r += 64)
    {
        const double x = T[r];
        const uint8_t bit = ran ? static_cast<uint8_t>(x <= 0.0) : 0; // mCO is still zero-initialised when no iteration ran
        if (h)
            h[P.rank_col[r]] = bit;
        if constexpr (WANT_LLR)
            a.llr_out[frame * nc + P.rank_col[r]] = ran ? x : 0.0;
    }
    if (a.bit_errors)
    {
        int err = 0;
        for (int i = lane; i < P.n_bitpos; i += 64)
        {
            const int est = ran ? static_cast<int>(T[P.tx_rank[i]] <= 0.0) : 0;
            const int tx = cw ? static_cast<int>(cw[P.bit_pos[i]]) : 0;
            err += est != tx;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            err += __shfl_xor(err, o, 64);
        if (lane == 0)
            a.bit_errors[frame] = static_cast<uint32_t>(err);
    }
}
} // namespace

int launch_decode_layered_ms(const DecodeArgs &a, const DevLayerPlan &L, void *stream)
{
    if (a.n_frames == 0)
        return hipSuccess;
    if (!L.steps || !L.rec_off || L.region_bytes_ms == 0 || L.region_bytes_ms > kCuLdsBytes || a.n_frames > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    void (*k)(const DecodeArgs, const DevLayerPlan) = a.llr_out ? decode_layered_ms_kernel<true> : decode_layered_ms_kernel<false>;
    return launch_with_lds(k, dim3(static_cast<unsigned>(a.n_frames)), dim3(kLmsThreads), L.region_bytes_ms, stream, a, L);
}

} // namespace ldpc_amd
