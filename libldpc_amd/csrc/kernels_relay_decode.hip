// kernels_relay_decode.hip — quantized min-sum WITH MEMORY, run as a RELAY OF LEGS, toward a given syndrome (include/ldpc_amd.h,
// ldpc_hip_relay_decode_batch states the arithmetic): the message-passing decoder of degenerate codes (quantum LDPC, surface
// codes), where plain min-sum swings between equal-weight solutions.  Each column's prior for an iteration is its input
// mixed with its own previous total, by a strength gamma[leg][column] / 64 that may be negative; every leg starts from the
// totals the last one left; every word that meets the syndrome is priced by the inputs it contradicts and the cheapest is
// kept.  Everything after the one quantization of the input is integer arithmetic: every output bit follows from the contract
// and is held against a numpy mirror (tests/relay_decode_ref.py).
//
// ONE BODY, templated on the threads that share a frame, on the tables of DevQmsPlan (read from global memory):
//   THREADS = 256  a workgroup per frame; its passes are separated by workgroup barriers, the stop test is the pair of vote
//                  words of kernels_syndrome_decode.hip, a sum goes through four partial sums in LDS;
//   THREADS = 64   a wave per frame, kRelayWaveFrames frames to a workgroup and NO workgroup barrier: the LDS operations of
//                  a wave execute in order (kernels_bit_flip.hip), the stop test is a ballot, a sum six exchanges.  A wave
//                  whose frame lies beyond the batch leaves at once.
// What LDS holds per frame (kernels.hpp, relay_decode_lds_bytes): the frame of kernels_syndrome_decode.hip in its order —
// messages, totals A[nc], table + votes + partial sums, syndrome bits in table order, the quantized inputs L[nc] by rank —
// and behind it the kept word, a bit per column in COLUMN order.
//   leg        every slot of a column is set to clamp(Lambda) (a leg starts with all check-node messages 0), A stays.
//   iteration  the check-node pass of the parent; then ONE variable-node pass that forms, from the A it is about to
//              overwrite, this iteration's prior Lambda, the new total A = Lambda + the sum of the messages, and from that
//              new total the next iteration's prior and messages.  No array of Lambda, no further pass.
//   solution   only in an iteration that met s: the cost by a reduction; if it is strictly below the kept one, the word
//              through the column map by a ballot per 64 columns.
// The gamma of the leg is read from global memory by rank through DevPlan::rank_col; all frames share the row.
// No static LDS, nothing that depends on timing.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch_lds.hpp"

namespace ldpc_amd
{

namespace
{
// clamp(rint(fl(w * inv)), -qmax, +qmax), the clamp in binary64; a NaN gives 0 (kernels_syndrome_decode.hip, sd_quantize:
// the same quantizer)
__device__ __forceinline__ int rl_quantize(double w, double inv, int qmax)
{
#pragma clang fp contract(off)
    const double x = __builtin_rint(w * inv);
    const double q = static_cast<double>(qmax);
    return x >= q ? qmax : (x <= -q ? -qmax : (x == x ? static_cast<int>(x) : 0));
}

// element i of the typed input as its quantized value; an int8 k counts steps: clamp(k)
__device__ __forceinline__ int rl_load(const RelayDecodeArgs &a, uint64_t i)
{
    switch (a.llr_type) // (uniform)
    {
    case kLlrF64: return rl_quantize(static_cast<const double *>(a.llr)[i], a.inv, a.qmax);
    case kLlrF32: return rl_quantize(static_cast<double>(static_cast<const float *>(a.llr)[i]), a.inv, a.qmax);
    case kLlrF16: return rl_quantize(static_cast<double>(static_cast<const _Float16 *>(a.llr)[i]), a.inv, a.qmax);
    default:
    {
        const int k = static_cast<const int8_t *>(a.llr)[i];
        return k > a.qmax ? a.qmax : (k < -a.qmax ? -a.qmax : k);
    }
    }
}

__device__ __forceinline__ int rl_byte_of(uint32_t word, int b) { return static_cast<int>(static_cast<int8_t>(word >> (8 * b))); }
__device__ __forceinline__ int rl_bit(const uint32_t *words, int i) { return static_cast<int>((words[i >> 5] >> (i & 31)) & 1u); }
__device__ __forceinline__ int rl_clamp(int v, int m) { return v > m ? m : (v < -m ? -m : v); }

// what separates two passes over a frame's LDS: a workgroup barrier, or — one wave — only the compiler kept from moving
// LDS operations across (the hardware executes a wave's in order)
template <int THREADS>
__device__ __forceinline__ void rl_sync()
{
    if constexpr (THREADS == 64)
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    else
        __syncthreads();
}

// the sum of x over the frame's threads, in every one of them.  `part` [THREADS / 64] is read after one barrier; the caller
// keeps another barrier between two sums
template <int THREADS>
__device__ __forceinline__ uint32_t rl_sum(uint32_t x, uint32_t *part, int lane, int wave)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        x += __shfl_xor(x, o, 64);
    if constexpr (THREADS == 64)
        return x;
    else
    {
        if (lane == 0)
            part[wave] = x;
        __syncthreads();
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w)
            s += part[w];
        return s;
    }
}

// the prior of a column: Lambda = clamp(L + d, +-32767), d = g (A - L) / 64 rounded half away from zero
__device__ __forceinline__ int rl_prior(int g, int A, int L)
{
    const int p = g * (A - L);
    const int m = ((p < 0 ? -p : p) + 32) >> 6;
    return rl_clamp(L + (p < 0 ? -m : m), 32767);
}

// the gamma of rank r in this leg's row (null: zero), clamped to +-64
__device__ __forceinline__ int rl_gamma(const int8_t *row, const uint32_t *rank_col, int r)
{
    return row ? rl_clamp(static_cast<int>(row[rank_col[r]]), 64) : 0;
}

// the start of a leg: every check-node message counts as 0, so every message of a column becomes clamp(Lambda); A stays
template <int THREADS>
__device__ __forceinline__ void rl_leg_start(const DevQmsPlan &Q, const RelayDecodeArgs &a, const int8_t *grow, int nc, int tid, const int8_t *L,
                                             int8_t *msg, const int32_t *A)
{
    for (int r = tid; r < nc; r += THREADS)
    {
        const int8_t v = static_cast<int8_t>(rl_clamp(rl_prior(rl_gamma(grow, a.rank_col, r), A[r], L[r]), a.qmax));
        const uint32_t b = Q.vn_start[r], e = Q.vn_start[r + 1];
        for (uint32_t i = b; i < e; ++i)
            msg[Q.vn_slot[i]] = v;
    }
}

// variable nodes: this iteration's prior from the total the last one left, the new total, and from the new total the next
// iteration's prior and messages
template <int THREADS>
__device__ __forceinline__ void rl_vn_pass(const DevQmsPlan &Q, const RelayDecodeArgs &a, const int8_t *grow, int nc, int tid, const int8_t *L,
                                           int8_t *msg, int32_t *A)
{
    const int qmax = a.qmax;
    for (int r = tid; r < nc; r += THREADS)
    {
        const uint32_t b = Q.vn_start[r], e = Q.vn_start[r + 1];
        const int g = rl_gamma(grow, a.rank_col, r), l = L[r];
        int sum = 0;
        for (uint32_t i = b; i < e; ++i)
            sum += msg[Q.vn_slot[i]];
        const int total = rl_prior(g, A[r], l) + sum;
        A[r] = total;
        const int next = rl_prior(g, total, l) + sum;
        for (uint32_t i = b; i < e; ++i)
        {
            const uint32_t s = Q.vn_slot[i];
            msg[s] = static_cast<int8_t>(rl_clamp(next - msg[s], qmax));
        }
    }
}

// check nodes: message j := +-lut[the smallest |message| of the others], negative iff (the others that are < 0) + the check
// node's syndrome bit is odd (kernels_syndrome_decode.hip, sd_cn_pass: the same pass)
template <int THREADS>
__device__ __forceinline__ void rl_cn_pass(const DevQmsPlan &Q, int mc, int tid, int8_t *msg, const uint8_t *lut, const uint32_t *syn)
{
    for (int c = tid; c < mc; c += THREADS)
    {
        const uint2 d = *reinterpret_cast<const uint2 *>(Q.cn_desc + 2 * c);
        uint32_t *row = reinterpret_cast<uint32_t *>(msg + d.x);
        const int deg = static_cast<int>(d.y), words = (deg + 3) >> 2;
        int min1 = 127, min2 = 127, arg = 0, par = rl_bit(syn, c);
        for (int w = 0; w < words; ++w)
        {
            const uint32_t x = row[w];
#pragma unroll
            for (int b = 0; b < 4; ++b)
            {
                const int k = 4 * w + b;
                if (k >= deg)
                    break;
                const int v = rl_byte_of(x, b);
                const int m = v < 0 ? -v : v;
                par ^= static_cast<int>(v < 0);
                const bool lt = m < min1;
                min2 = lt ? min1 : (m < min2 ? m : min2);
                arg = lt ? k : arg;
                min1 = lt ? m : min1;
            }
        }
        const int r_rest = lut[min1], r_arg = lut[min2];
        for (int w = 0; w < words; ++w)
        {
            const uint32_t x = row[w];
            uint32_t y = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
            {
                const int k = 4 * w + b;
                if (k >= deg)
                    break; // (the padding stays zero)
                const int mag = k == arg ? r_arg : r_rest;
                const bool neg = (par ^ static_cast<int>(rl_byte_of(x, b) < 0)) != 0;
                y |= (static_cast<uint32_t>(neg ? -mag : mag) & 0xFFu) << (8 * b);
            }
            row[w] = y;
        }
    }
}

// this thread's check nodes whose XOR of the decisions A <= 0 over the row differs from the syndrome bit
template <int THREADS>
__device__ __forceinline__ uint32_t rl_unmet(const DevQmsPlan &Q, int mc, int tid, const int32_t *A, const uint32_t *syn)
{
    uint32_t bad = 0;
    for (int c = tid; c < mc; c += THREADS)
    {
        const uint2 d = *reinterpret_cast<const uint2 *>(Q.cn_desc + 2 * c);
        const uint16_t *vn = Q.cn_vn + d.x;
        int p = rl_bit(syn, c);
        for (uint32_t k = 0; k < d.y; ++k)
            p ^= static_cast<int>(A[vn[k]] <= 0);
        bad += static_cast<uint32_t>(p);
    }
    return bad;
}

// the decisions A <= 0 in column order, packed by a ballot per 64 columns, to `out` [words] (LDS or global memory)
template <int THREADS>
__device__ __forceinline__ void rl_pack(const RelayDecodeArgs &a, int nc, int lane, int wave, const int32_t *A, uint32_t *out)
{
    for (int base = 64 * wave; base < nc; base += THREADS) // (wave-uniform)
    {
        const int c = base + lane;
        const bool one = c < nc && A[a.col_rank[c]] <= 0;
        const uint64_t m = __ballot(one);
        if (lane == 0)
        {
            const uint32_t w = static_cast<uint32_t>(base) >> 5;
            out[w] = static_cast<uint32_t>(m);
            if (w + 1 < a.words)
                out[w + 1] = static_cast<uint32_t>(m >> 32);
        }
    }
}

template <int THREADS>
__global__ __launch_bounds__(256) void relay_decode_kernel(const RelayDecodeArgs a, const DevQmsPlan Q)
{
    extern __shared__ uint4 rl_lds[];
    const int nc = static_cast<int>(a.nc), mc = static_cast<int>(a.mc);
    // the thread's place among those of its frame, and the frame
    const int lane = threadIdx.x & 63;
    const int group_wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int wave = THREADS == 64 ? 0 : group_wave, tid = THREADS == 64 ? lane : static_cast<int>(threadIdx.x);
    const uint64_t frame = THREADS == 64 ? static_cast<uint64_t>(blockIdx.x) * kRelayWaveFrames + group_wave : blockIdx.x;
    if (frame >= a.n) // (THREADS == 64: no workgroup barrier below, the other waves do not wait)
        return;
    unsigned char *lds = reinterpret_cast<unsigned char *>(rl_lds) + (THREADS == 64 ? static_cast<size_t>(group_wave) * a.frame_bytes : 0);
    int8_t *msg = reinterpret_cast<int8_t *>(lds);
    int32_t *A = reinterpret_cast<int32_t *>(lds + syndrome_decode_round16(Q.slots));
    uint8_t *lut = reinterpret_cast<uint8_t *>(A) + syndrome_decode_round16(4 * static_cast<size_t>(nc));
    uint32_t *vote = reinterpret_cast<uint32_t *>(lut + 128); // [2], used in turn: iteration k of the frame votes in word k & 1
    uint32_t *part = vote + 4;                                // [4]: a wave's share of a sum
    uint32_t *syn = reinterpret_cast<uint32_t *>(lut + kSyndromeDecodeSideBytes);
    int8_t *L = reinterpret_cast<int8_t *>(syn) + syndrome_decode_round16(4 * static_cast<size_t>(a.syn_words));
    uint32_t *kept = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(L) + syndrome_decode_round16(static_cast<size_t>(nc)));

    {
        uint32_t *z = reinterpret_cast<uint32_t *>(msg);
        for (uint32_t i = tid; i < Q.slots / 4; i += THREADS)
            z[i] = 0;
        if (tid < 32) // (a select chain over the launch arguments: indexing them by a lane's number would put them in scratch)
        {
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 32; ++i)
                w = tid == i ? a.lut[i] : w;
            reinterpret_cast<uint32_t *>(lut)[tid] = w;
        }
        else if (tid < 40)
            vote[tid - 32] = 0;
        const uint64_t at = a.shared_llr ? 0 : frame * a.nc;
        for (int c = tid; c < nc; c += THREADS) // before leg 0, A := L
        {
            const int q = rl_load(a, at + static_cast<uint64_t>(c));
            const uint32_t r = a.col_rank[c];
            L[r] = static_cast<int8_t>(q);
            A[r] = q;
        }
        // the syndrome: check node c of the tables is row cn_row[c] of the caller's
        for (int base = 64 * wave; base < mc; base += THREADS) // (wave-uniform)
        {
            const int c = base + lane;
            bool one = false;
            if (c < mc && a.syndrome)
            {
                const uint32_t row = a.cn_row[c];
                if (a.syndrome_format == kBitsU8)
                    one = static_cast<const uint8_t *>(a.syndrome)[frame * a.mc + row] != 0;
                else
                    one = ((static_cast<const uint32_t *>(a.syndrome)[frame * a.syn_words + (row >> 5)] >> (row & 31u)) & 1u) != 0;
            }
            const uint64_t m = __ballot(one);
            if (lane == 0)
            {
                const uint32_t w = static_cast<uint32_t>(base) >> 5;
                syn[w] = static_cast<uint32_t>(m);
                if (w + 1 < a.syn_words)
                    syn[w + 1] = static_cast<uint32_t>(m >> 32);
            }
        }
    }
    rl_sync<THREADS>();

    // (all of these are the same in every thread of the frame)
    uint32_t iters = 0, solutions = 0, best_leg = kRelayNone, best_cost = kRelayNone, tick = 0;
    for (uint32_t leg = 0; leg < a.legs && solutions < a.stop_after; ++leg)
    {
        const int8_t *grow = a.gamma ? a.gamma + static_cast<size_t>(leg) * a.nc : nullptr;
        const uint32_t T = leg == 0 ? a.first_iterations : a.leg_iterations;
        rl_leg_start<THREADS>(Q, a, grow, nc, tid, L, msg, A);
        rl_sync<THREADS>();
        uint32_t i = 0;
        bool met = false;
        while (i < T)
        {
            rl_cn_pass<THREADS>(Q, mc, tid, msg, lut, syn);
            rl_sync<THREADS>();
            rl_vn_pass<THREADS>(Q, a, grow, nc, tid, L, msg, A);
            rl_sync<THREADS>();
            const uint32_t bad = rl_unmet<THREADS>(Q, mc, tid, A, syn);
            const bool wave_bad = __ballot(bad != 0) != 0;
            if constexpr (THREADS == 64)
                met = !wave_bad;
            else
            {
                // a wave with an unmet check node raises this iteration's word; thread 0 clears the other word for the next
                // iteration (read last an iteration ago, two barriers back)
                if (wave_bad && lane == 0)
                    vote[tick & 1] = 1;
                if (tid == 0)
                    vote[(tick + 1) & 1] = 0;
                __syncthreads();
                met = vote[tick & 1] == 0;
                ++tick;
            }
            if (met)
                break;
            ++i;
        }
        iters += i; // (i == T for a leg that never met s)
        if (met)
        {
            ++solutions;
            // the cost: the inputs the word contradicts
            uint32_t mine = 0;
            for (int r = tid; r < nc; r += THREADS)
            {
                const int l = L[r];
                if ((A[r] <= 0) != (l <= 0))
                    mine += static_cast<uint32_t>(l < 0 ? -l : l);
            }
            const uint32_t cost = rl_sum<THREADS>(mine, part, lane, wave);
            if (best_leg == kRelayNone || cost < best_cost)
            {
                best_leg = leg, best_cost = cost;
                rl_pack<THREADS>(a, nc, lane, wave, A, kept);
            }
        }
    }
    rl_sync<THREADS>(); // (the kept word, written by the first lanes of the waves, is read below by others)

    if (tid == 0)
    {
        if (a.iters)
            a.iters[frame] = iters;
        if (a.solutions)
            a.solutions[frame] = solutions;
        if (a.best_leg)
            a.best_leg[frame] = best_leg;
        if (a.cost)
            a.cost[frame] = best_cost;
    }
    if (best_leg != kRelayNone) // (uniform) the kept word meets s
    {
        if (a.hard_bits)
            for (uint32_t w = tid; w < a.words; w += THREADS)
                a.hard_bits[frame * a.words + w] = kept[w];
        if (a.weight && tid == 0)
            a.weight[frame] = 0;
    }
    else // the decisions of the last iteration run
    {
        if (a.hard_bits)
            rl_pack<THREADS>(a, nc, lane, wave, A, a.hard_bits + frame * a.words);
        if (a.weight)
        {
            const uint32_t bad = rl_sum<THREADS>(rl_unmet<THREADS>(Q, mc, tid, A, syn), part, lane, wave);
            if (tid == 0)
                a.weight[frame] = bad;
        }
    }
}
} // namespace

int launch_relay_decode(const RelayDecodeArgs &a, const DevQmsPlan &Q, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    if (!Q.cn_desc || !Q.cn_vn || !Q.vn_start || !Q.vn_slot || (Q.slots & 3u) || a.qmax < 1 || a.qmax > 127 || a.nc == 0 || a.nc > 0xFFFFu ||
        a.mc == 0 || a.words != (a.nc + 31) / 32 || a.syn_words != (a.mc + 31) / 32 || !a.col_rank || !a.rank_col || !a.cn_row || !a.llr ||
        llr_type_bytes(a.llr_type) == 0 || (a.syndrome && !bits_format_known(a.syndrome_format)) || a.legs < 1 || a.legs > 256 ||
        a.first_iterations < 1 || a.first_iterations > 0xFFFFu || a.leg_iterations < 1 || a.leg_iterations > 0xFFFFu || a.stop_after < 1 ||
        a.stop_after > a.legs || a.frame_bytes != relay_decode_lds_bytes(Q.slots, a.nc, a.mc) || a.n > (1ull << 20))
        return hipErrorInvalidValue;
    if (a.form == kRelayFormGroup)
    {
        if (a.frame_bytes > kCuLdsBytes)
            return hipErrorInvalidValue;
        return launch_with_lds(relay_decode_kernel<256>, dim3(static_cast<unsigned>(a.n)), dim3(256), a.frame_bytes, stream, a, Q);
    }
    if (a.form == kRelayFormWave)
    {
        if (static_cast<size_t>(kRelayWaveFrames) * a.frame_bytes > kCuLdsBytes)
            return hipErrorInvalidValue;
        const uint64_t groups = (a.n + kRelayWaveFrames - 1) / kRelayWaveFrames;
        return launch_with_lds(relay_decode_kernel<64>, dim3(static_cast<unsigned>(groups)), dim3(kRelayWaveFrames * 64),
                               kRelayWaveFrames * a.frame_bytes, stream, a, Q);
    }
    return hipErrorInvalidValue;
}

} // namespace ldpc_amd
