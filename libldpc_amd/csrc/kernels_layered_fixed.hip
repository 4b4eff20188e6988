// kernels_layered_fixed.hip — opt-in NON-PARITY FIXED-POINT LAYERED min-sum decoding ("BP_MS" with
// ldpc_hip_set_min_sum_layered_fixed(msg_bits, app_bits, step); include/ldpc_amd.h states the arithmetic).  The decoder that
// LDPC hardware implements: the layered (row-serial) schedule on a saturating integer datapath, messages of q = 2..8 bits and
// a wider a-posteriori total of p <= 16 bits per column.  Everything after the one quantization of the channel LLRs is integer
// arithmetic, so every output bit follows from the contract and is held against a numpy mirror bit for bit
// (tests/layered_fixed_minsum_ref.py).  The reference has no such decoder (decoder.cpp:22-76 is flooding, binary64).
//
// Mapping as in kernels_layered_ms.hip: ONE WAVE = ONE FRAME, a sweep is the sequence of STEPS of build_layer_plan (plan.cpp),
// a step is up to 64 check nodes of equal degree that share no variable node, one per lane; the steps need no barrier (a
// wave's LDS operations execute in order) and a step's neighbour table is fetched one step ahead.
//
// What LDS holds per frame (plan.hpp, layered_fixed_region_bytes):
//   * first the nc binary64 channel LLRs, written by channel_init as everywhere (all channel and noise modes);
//   * then, over the same bytes: the totals T[nc], int16 (the wave quantizes the LLRs IN PLACE, below); behind them, from
//     the next multiple of 4, per check node ONE 32-bit RECORD instead of its D messages.  The outputs of a min-sum check
//     node take two magnitudes only: every edge but the one that holds the smallest input gets lut[min1], that edge gets
//     lut[min2].  The record is lut[min1] in bits 0..6, lut[min2] in bits 7..13, the argmin position in bits 14..16 and the
//     D output sign bits from bit 17 on; message j is (j == argmin ? lut[min2] : lut[min1]) with sign bit j — exactly the
//     message a full array would hold (where two inputs tie for the minimum, min2 == min1 and either argmin gives the same
//     values).  Records are laid out [lane] within a step, the step's real check nodes rounded up to an even number (the
//     slots of plan.hpp, layered_ms_records: rec_off / 20 is the step's first slot);
//   * behind the larger of the two, the correction table, 128 bytes.
// h.txt: 9 344 bytes per frame, 17 frames per CU; the n = 8192 (3,6) code 65 664, two.
//
// Iteration count returned: sweeps completed before the sweep whose syndrome check passed (the reference's convention,
// decoder.cpp:21-22,74-77); the syndrome of the current decisions is taken after every sweep.
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

template <bool WANT_LLR>
__global__ __launch_bounds__(kLfThreads) void decode_layered_fixed_kernel(const DecodeArgs a, const DevLayerPlan L, const LayeredFixedArgs q)
{
    extern __shared__ double lds_d[];
    const DevPlan &P = a.plan;
    const int nc = P.nc;
    const int lane = threadIdx.x;
    const uint64_t frame = blockIdx.x;
    if (frame >= a.n_frames)
        return;
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds_d);
    const uint32_t rec_slots = L.record_bytes / 20; // (layered_ms_records: 20 bytes per slot there, one word here)
    lds_i16 *T = reinterpret_cast<lds_i16 *>(lds);
    lds_u32 *records = reinterpret_cast<lds_u32 *>(lds + layered_fixed_records_off(nc));
    uint8_t *lut = lds + layered_fixed_lut_off(rec_slots, nc);
    const uint8_t *cw = a.codeword ? a.codeword + frame * nc : nullptr;
    const int qmax = q.qmax, pmax = q.pmax;

    channel_init<64, kNoiseAny>(a, frame, lds_d, lane); // binary64 channel + LLR initialisation, as everywhere (one wave's worth)
    if (lane < 32) // (a select chain over the launch arguments: indexing them by a lane's number would put them in scratch)
    {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i)
            w = lane == i ? q.lut[i] : w;
        reinterpret_cast<lds_u32 *>(lut)[lane] = w; // (behind the binary64 area)
    }
    __syncthreads(); // (one wave: orders the compiler and the LDS queue, costs nothing)
    // The LLRs become the totals IN PLACE.  Chunk k = columns 64 k .. 64 k + 63: every lane reads its binary64 value (bytes
    // 512 k + 8 lane ..), then every lane writes its int16 (bytes 128 k + 2 lane ..) — one load instruction of the whole wave
    // before one store instruction, the store's value depending on the load's.  The int16 image of chunk k lies in bytes
    // [128 k, 128 k + 128), inside [512 (k / 4), 512 (k / 4) + 512): binary64 values of chunk k / 4 <= k, all read already;
    // chunks after k read from byte 512 (k + 1) > 128 k + 128 on.  In the last chunk of a column count that is no multiple of
    // 64 the lanes beyond nc neither read nor write: the bytes they would have written hold no column.
    {
        const lds_f64 *llr = reinterpret_cast<const lds_f64 *>(lds);
        double *o = a.llr_in_dump ? a.llr_in_dump + frame * nc : nullptr;
        for (int r = lane; r < nc; r += 64)
        {
            const double x = llr[r];
            if (o)
                o[P.rank_col[r]] = x; // (llr_in stays the unquantized value)
            T[r] = static_cast<int16_t>(lf_quantize(x, q.inv, qmax));
        }
    }
    __syncthreads(); // the binary64 area is free
    for (uint32_t i = lane; i < rec_slots; i += 64)
        records[i] = 0; // every message 0: magnitudes 0, argmin 0, no sign bit
    __syncthreads();

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
            const uint32_t cd = steps[2 * s + 1], ro = rec_off[s] / 20;
            const int count = cd & 0xFFFF, degree = cd >> 16;
            if (lane < count)
            {
                lds_u32 *rec = records + ro + lane;
                switch (degree) // wave-uniform
                {
                case 2: cn_layered_fixed<2>(T, rec, lut, cur, qmax, pmax); break;
                case 3: cn_layered_fixed<3>(T, rec, lut, cur, qmax, pmax); break;
                case 4: cn_layered_fixed<4>(T, rec, lut, cur, qmax, pmax); break;
                case 5: cn_layered_fixed<5>(T, rec, lut, cur, qmax, pmax); break;
                case 6: cn_layered_fixed<6>(T, rec, lut, cur, qmax, pmax); break;
                case 7: cn_layered_fixed<7>(T, rec, lut, cur, qmax, pmax); break;
                case 8: cn_layered_fixed<8>(T, rec, lut, cur, qmax, pmax); break;
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
                    case 2: bad |= cn_parity_fixed<2>(T, cur); break;
                    case 3: bad |= cn_parity_fixed<3>(T, cur); break;
                    case 4: bad |= cn_parity_fixed<4>(T, cur); break;
                    case 5: bad |= cn_parity_fixed<5>(T, cur); break;
                    case 6: bad |= cn_parity_fixed<6>(T, cur); break;
                    case 7: bad |= cn_parity_fixed<7>(T, cur); break;
                    case 8: bad |= cn_parity_fixed<8>(T, cur); break;
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
        const int x = T[r];
        if (h)
            h[P.rank_col[r]] = ran ? static_cast<uint8_t>(x <= 0) : 0; // mCO is still zero-initialised when no iteration ran
        if constexpr (WANT_LLR)
            a.llr_out[frame * nc + P.rank_col[r]] = ran ? static_cast<double>(x) * q.step : 0.0;
    }
    if (a.bit_errors)
    {
        int err = 0;
        for (int i = lane; i < P.n_bitpos; i += 64)
        {
            const int est = ran ? static_cast<int>(T[P.tx_rank[i]] <= 0) : 0;
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

int launch_decode_layered_fixed(const DecodeArgs &a, const DevLayerPlan &L, const LayeredFixedArgs &q, void *stream)
{
    if (a.n_frames == 0)
        return hipSuccess;
    const uint64_t nc = a.plan.nc > 0 ? static_cast<uint64_t>(a.plan.nc) : 0;
    const size_t region = layered_fixed_region_bytes(L.record_bytes / 20, nc);
    if (!L.steps || !L.vn4 || !L.rec_off || L.record_bytes == 0 || L.record_bytes % 20 != 0 || nc == 0 || nc > 0xFFFF || region > kCuLdsBytes ||
        q.qmax < 1 || q.qmax > 127 || q.pmax < q.qmax || q.pmax > 32767 || a.n_frames > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    void (*k)(const DecodeArgs, const DevLayerPlan, const LayeredFixedArgs) =
        a.llr_out ? decode_layered_fixed_kernel<true> : decode_layered_fixed_kernel<false>;
    return launch_with_lds(k, dim3(static_cast<unsigned>(a.n_frames)), dim3(kLfThreads), static_cast<uint32_t>(region), stream, a, L, q);
}

} // namespace ldpc_amd
