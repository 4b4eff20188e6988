// kernels_syndrome_decode_layered.hip — fixed-point layered min-sum decoding of the batch interface TOWARD A GIVEN SYNDROME
// (include/ldpc_amd.h, ldpc_hip_syndrome_decode_layered_batch states the arithmetic): the row-serial schedule and the integer
// datapath of kernels_layered_fixed.hip (int16 totals, one 32-bit record per check node, the 128-byte correction table) with
// the two changes of kernels_syndrome_decode.hip: a check node's sign parity starts at its syndrome bit, and the stop test
// asks for the syndrome s instead of zero.  Everything after the one quantization of the input is integer arithmetic: every
// output bit follows from the contract and is held against a numpy mirror (tests/syndrome_decode_layered_ref.py).
//
// ONE WAVE = ONE FRAME = ONE WORKGROUP, on the tables of DevLayerPlan (steps, vn4, rec_off), as
// decode_layered_fixed_direct_kernel.  What LDS holds per frame is exactly what that kernel holds (plan.hpp,
// layered_fixed_direct_region_bytes): the totals T[nc], int16; from the next multiple of 4 one 32-bit record per check-node
// slot; behind the records the correction table.  THE SYNDROME TAKES NO ROOM: a record uses bits 0..24 (two magnitudes, the
// argmin, eight signs), and bit 31 is the check node's right-hand side s[c], set when the records are initialised and kept
// by every rewrite.  The sign rule reads it back with the record (all output signs flip where it is set), the stop test and
// the weight compare a row's parity with it.
//   prologue   the frame's elements read in place in their own type, column order (coalesced; int8 a dword per lane from the
//              first 4-byte boundary of the row on), quantized, stored at the column's rank.  No binary64 staging.  Then, step
//              by step, lane l fetches the syndrome bit of the step's l-th check node through the one table this kernel adds
//              (step, lane) -> file row, and writes it as the record's first value.
//   sweeps     kernels_layered_fixed_body.inc with the check node below: the neighbour table fetched one step ahead.
//   epilogue   a lane per column: the total through the column map, llr_out coalesced, the packed decisions by a ballot per
//              64 columns; the weight = one parity pass over the final decisions, a popcount of ballots (0 without the pass
//              where the stop test has just passed).
// The check node and the sweeps are written out here instead of being shared with kernels_layered_fixed_body.inc: a change to
// that text moves the register allocation of the two kernels that include it.
#include "kernels_layered_fixed_impl.hpp"

namespace ldpc_amd
{

namespace
{
// cn_layered_fixed (kernels_layered_fixed_impl.hpp) with the right-hand side in bit 31 of the record: edge j is negative iff
// (the number of the others that are negative) + s is odd
template <int D>
__device__ __forceinline__ void cn_sdl(lds_i16 *T, lds_u32 *rec, const uint8_t *lut, const uint32_t (&pk)[4], int qmax, int pmax)
{
    const uint32_t o = *rec;
    const int o_rest = static_cast<int>(o & 127u), o_arg = static_cast<int>((o >> 7) & 127u);
    const uint32_t o_hot = 1u << ((o >> 14) & 7u); // bit argmin
    const uint32_t o_neg = o >> 17;                // (bits 0..7 are read: the syndrome bit sits at 14 here)
    const int flip = static_cast<int>(o) >> 31;    // -1 where s = 1
    uint32_t n[D];
    int t[D];
#pragma unroll
    for (int j = 0; j < D; ++j)
        n[j] = vn_of(pk, j);
    uint32_t key1 = 127u << 3, key2 = 127u << 3; // (|u| <= qmax <= 127)
    int signs = 0, sx = flip;
#pragma unroll
    for (int j = 0; j < D; ++j)
    {
        const int mo = lf_sel(lf_bit_mask(o_hot, j), o_arg, o_rest);
        const int neg = lf_bit_mask(o_neg, j);
        const int m = (mo ^ neg) - neg;
        t[j] = static_cast<int>(T[n[j]]) - m; // what the neighbour says without this node's last message: exact
        const int u = lf_clamp(t[j], qmax);   // ... at message width
        const int s = u >> 31;                // -1 where u < 0 (an integer zero is not negative)
        const uint32_t key = static_cast<uint32_t>((u ^ s) - s) << 3 | static_cast<uint32_t>(j);
        signs |= s & (1 << j), sx ^= s;
        const uint32_t hi = key > key1 ? key : key1;
        key1 = key < key1 ? key : key1;
        key2 = hi < key2 ? hi : key2;
    }
    const int r_rest = lut[key1 >> 3], r_arg = lut[key2 >> 3];
    const uint32_t k = key1 & 7u, hot = 1u << k;
    const int out_signs = (signs ^ sx) & ((1 << D) - 1);
#pragma unroll
    for (int j = 0; j < D; ++j)
    {
        const int mo = lf_sel(lf_bit_mask(hot, j), r_arg, r_rest);
        const int neg = lf_bit_mask(out_signs, j);
        T[n[j]] = static_cast<int16_t>(lf_clamp(t[j] + ((mo ^ neg) - neg), pmax));
    }
    *rec = static_cast<uint32_t>(r_rest) | static_cast<uint32_t>(r_arg) << 7 | k << 14 | static_cast<uint32_t>(out_signs) << 17 |
           (o & kSdlSyndromeBit);
}

// 1 where the XOR of the decisions over the check node's row differs from its syndrome bit
template <int D>
__device__ __forceinline__ uint32_t cn_unmet_sdl(const lds_i16 *T, const lds_u32 *rec, const uint32_t (&pk)[4])
{
    return cn_parity_fixed<D>(T, pk) ^ (*rec >> 31);
}

// a row of binary64, binary32 or binary16 elements, column order, quantized to the totals at the columns' ranks.  One wave
// walks the whole row (18 trips for 1 152 columns), so the loads of four trips are issued before the first is used: a trip
// at a time 8 192 binary64 frames of 8 192 columns took 3.94 ms per call, this way 3.30 (profiles/README.md)
template <class E>
__device__ __forceinline__ void sdl_quantize_row(const E *src, int nc, int lane, const uint32_t *col_rank, lds_i16 *T, double inv, int qmax)
{
    int c = lane;
    for (; c + 192 < nc; c += 256)
    {
        E x[4];
        uint32_t r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            x[u] = src[c + 64 * u], r[u] = col_rank[c + 64 * u];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            T[r[u]] = static_cast<int16_t>(lf_quantize(static_cast<double>(x[u]), inv, qmax));
    }
    for (; c < nc; c += 64)
        T[col_rank[c]] = static_cast<int16_t>(lf_quantize(static_cast<double>(src[c]), inv, qmax));
}

__global__ __launch_bounds__(kLfThreads) void syndrome_decode_layered_kernel(const SyndromeDecodeLayeredArgs a, const DevLayerPlan L)
{
    extern __shared__ double lds_d[];
    const int nc = static_cast<int>(a.nc);
    const int lane = threadIdx.x;
    const uint64_t frame = blockIdx.x;
    if (frame >= a.n)
        return;
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds_d);
    const uint32_t rec_slots = L.record_bytes / 20;
    lds_i16 *T = reinterpret_cast<lds_i16 *>(lds);
    lds_u32 *records = reinterpret_cast<lds_u32 *>(lds + layered_fixed_records_off(a.nc));
    uint8_t *lut = lds + layered_fixed_records_off(a.nc) + 4 * static_cast<size_t>(rec_slots);
    const int qmax = a.q.qmax, pmax = a.q.pmax;
    const uint32_t *col_rank = a.col_rank;
    const uint64_t row_at = a.shared_llr ? 0 : frame * a.nc; // the frame's first element

    lf_load_lut(a.q, lut, lane);
    if (a.llr_type == kLlrI8) // (the type is uniform)
    {
        const int8_t *src = static_cast<const int8_t *>(a.llr) + row_at;
        auto put = [&](int c, int k) { T[col_rank[c]] = static_cast<int16_t>(lf_clamp(k, qmax)); };
        int head = static_cast<int>((4 - (reinterpret_cast<uintptr_t>(src) & 3)) & 3); // bytes before the first whole word
        head = head < nc ? head : nc;
        const int words = (nc - head) >> 2;
        if (lane < head)
            put(lane, src[lane]);
        const uint32_t *src4 = reinterpret_cast<const uint32_t *>(src + head);
        for (int i = lane; i < words; i += 64)
        {
            const uint32_t w = src4[i];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                put(head + 4 * i + b, static_cast<int8_t>(w >> (8 * b)));
        }
        for (int c = head + 4 * words + lane; c < nc; c += 64)
            put(c, src[c]);
    }
    else if (a.llr_type == kLlrF16)
        sdl_quantize_row(static_cast<const _Float16 *>(a.llr) + row_at, nc, lane, col_rank, T, a.q.inv, qmax);
    else if (a.llr_type == kLlrF32)
        sdl_quantize_row(static_cast<const float *>(a.llr) + row_at, nc, lane, col_rank, T, a.q.inv, qmax);
    else
        sdl_quantize_row(static_cast<const double *>(a.llr) + row_at, nc, lane, col_rank, T, a.q.inv, qmax);
    for (uint32_t i = lane; i < rec_slots; i += 64)
        records[i] = 0; // every message 0: magnitudes 0, argmin 0, no sign bit; s = 0
    __syncthreads(); // (one wave: orders the compiler and the LDS queue)

    const auto steps = uniform_table(reinterpret_cast<const uint32_t *>(L.steps));
    const auto rec_off = uniform_table(L.rec_off);
    if (a.syndrome) // the right-hand sides: lane l of step s holds the check node of file row step_row[s][l]
    {
        for (uint32_t s = 0; s < L.n_steps; ++s)
        {
            const uint32_t count = steps[2 * s + 1] & 0xFFFFu, ro = rec_off[s] / 20;
            if (static_cast<uint32_t>(lane) < count)
            {
                const uint32_t row = a.step_row[s * 64 + lane]; // < mc
                bool one;
                if (a.syndrome_format == kBitsU8)
                    one = static_cast<const uint8_t *>(a.syndrome)[frame * a.mc + row] != 0;
                else
                    one = ((static_cast<const uint32_t *>(a.syndrome)[frame * a.syn_words + (row >> 5)] >> (row & 31u)) & 1u) != 0;
                records[ro + lane] = one ? kSdlSyndromeBit : 0u;
            }
        }
        __syncthreads();
    }

    // the step's neighbour table one step AHEAD (kernels_layered.hip)
    const uint32_t *table = L.vn4 + lane;
    auto fetch = [&](uint32_t s, uint32_t (&pk)[4]) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
            pk[w] = table[(s * 4 + w) * 64];
    };
    // this lane's check node of every step: 1 where its test fails on the decisions T <= 0; walks the table as a sweep does
    uint32_t nxt[4];
    auto unmet_pass = [&](auto &&seen) {
        for (uint32_t s = 0; s < L.n_steps; ++s)
        {
            uint32_t cur[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
            fetch(s + 1 < L.n_steps ? s + 1 : 0, nxt);
            const uint32_t cd = steps[2 * s + 1], ro = rec_off[s] / 20;
            const int count = cd & 0xFFFF, degree = cd >> 16;
            uint32_t bad = 0;
            if (lane < count)
            {
                const lds_u32 *rec = records + ro + lane;
                switch (degree) // wave-uniform
                {
                case 2: bad = cn_unmet_sdl<2>(T, rec, cur); break;
                case 3: bad = cn_unmet_sdl<3>(T, rec, cur); break;
                case 4: bad = cn_unmet_sdl<4>(T, rec, cur); break;
                case 5: bad = cn_unmet_sdl<5>(T, rec, cur); break;
                case 6: bad = cn_unmet_sdl<6>(T, rec, cur); break;
                case 7: bad = cn_unmet_sdl<7>(T, rec, cur); break;
                case 8: bad = cn_unmet_sdl<8>(T, rec, cur); break;
                default: break;
                }
            }
            seen(bad);
        }
    };
    uint32_t I = 0;
    bool met = false; // the stop test has passed on the totals as they stand
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
                case 2: cn_sdl<2>(T, rec, lut, cur, qmax, pmax); break;
                case 3: cn_sdl<3>(T, rec, lut, cur, qmax, pmax); break;
                case 4: cn_sdl<4>(T, rec, lut, cur, qmax, pmax); break;
                case 5: cn_sdl<5>(T, rec, lut, cur, qmax, pmax); break;
                case 6: cn_sdl<6>(T, rec, lut, cur, qmax, pmax); break;
                case 7: cn_sdl<7>(T, rec, lut, cur, qmax, pmax); break;
                case 8: cn_sdl<8>(T, rec, lut, cur, qmax, pmax); break;
                default: break;
                }
            }
            __builtin_amdgcn_wave_barrier(); // (LDS operations of a wave execute in order; this only stops the compiler)
        }
        if (a.early_term) // the decisions after this sweep against s
        {
            uint32_t bad = 0;
            unmet_pass([&](uint32_t b) { bad |= b; });
            if (__ballot(bad != 0) == 0)
            {
                met = true;
                break;
            }
        }
        ++I;
    }
    if (lane == 0 && a.iters)
        a.iters[frame] = I;
    // a lane per column: the total through the column map, the decisions of 64 columns by a ballot
    for (int base = 0; base < nc; base += 64)
    {
        const int c = base + lane;
        bool one = false;
        if (c < nc)
        {
            const int x = T[col_rank[c]];
            one = x <= 0;
            if (a.llr_out)
                a.llr_out[frame * a.nc + static_cast<uint64_t>(c)] = static_cast<double>(x) * a.q.step;
        }
        const uint64_t m = __ballot(one);
        if (a.hard_bits && lane == 0)
        {
            const uint32_t w = static_cast<uint32_t>(base) >> 5;
            uint32_t *h = a.hard_bits + frame * a.words;
            h[w] = static_cast<uint32_t>(m);
            if (w + 1 < a.words)
                h[w + 1] = static_cast<uint32_t>(m >> 32);
        }
    }
    if (a.weight) // (uniform)
    {
        uint32_t unmet = 0;
        if (!met)
            unmet_pass([&](uint32_t b) { unmet += static_cast<uint32_t>(__popcll(__ballot(b != 0))); });
        if (lane == 0)
            a.weight[frame] = unmet;
    }
}
} // namespace

int launch_syndrome_decode_layered(const SyndromeDecodeLayeredArgs &a, const DevLayerPlan &L, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    if (!L.steps || !L.vn4 || !L.rec_off || L.n_steps == 0 || L.record_bytes == 0 || L.record_bytes % 20 != 0 || a.nc == 0 || a.nc > 0xFFFFu ||
        a.mc == 0 || a.words != (a.nc + 31) / 32 || a.syn_words != (a.mc + 31) / 32 || a.q.qmax < 1 || a.q.qmax > 127 || a.q.pmax < a.q.qmax ||
        a.q.pmax > 32767 || !a.col_rank || !a.step_row || !a.llr || llr_type_bytes(a.llr_type) == 0 ||
        (a.syndrome && !bits_format_known(a.syndrome_format)) || a.lds_bytes != layered_fixed_direct_region_bytes(L.record_bytes / 20, a.nc) ||
        a.lds_bytes > kCuLdsBytes || a.n > (1ull << 20))
        return hipErrorInvalidValue;
    return launch_with_lds(syndrome_decode_layered_kernel, dim3(static_cast<unsigned>(a.n)), dim3(kLfThreads), a.lds_bytes, stream, a, L);
}

} // namespace ldpc_amd
