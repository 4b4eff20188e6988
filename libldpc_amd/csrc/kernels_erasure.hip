// kernels_erasure.hip — the erasure channel and the genie-free erasure decoder of the batch interface (include/ldpc_amd.h,
// ldpc_hip_erasure_channel_batch / ldpc_hip_erasure_decode_batch): received words with holes in them in, what peeling recovers
// out.  Bit rows are packed as hard_bits is.  The stream's erasure kernels (kernels_bec.hip) compare every message with the
// transmitted bit; nothing here knows it.
//   erasure_channel_kernel  ONE LANE = ONE OUTPUT WORD of a frame: 32 columns.  The lane walks them with the Philox block of
//                           the last transmitted index in registers (device_philox.hpp, tag 1: the BEC draw of the counter
//                           mode), so where bit_pos is consecutive a block is computed once, by the lane whose word holds its
//                           four columns; every output word is written exactly once, whole, with no atomic and no LDS.
//   erasure_decode_kernel   one workgroup = 32 consecutive frames, bit f of every LDS word = frame f.  A flooding erasure
//                           decoder without a genie needs no per-edge message: per pass a check node publishes two words,
//                             ONE = "exactly one of my columns is erased" = c0 & ~c1 (c0: one or more, c1: two or more),
//                             VAL = ONE & the XOR of my known columns' values (V & E = 0 throughout, so the XOR runs over V),
//                           and an erased column leaves E when some check node of it says ONE, taking the OR of their VAL.
//                           State per group: E[nc] V[nc] ONE[mc] VAL[mc] — 17 KB for h.txt where the message form takes 52.
//     prologue   frame-major packed rows -> column slices by ballot: lanes = frames, the two halves of a wave take two column
//                words, ballot b is the slice of column b of both; no staging buffer, each row word is read once.
//     pass       check-node chunks, barrier, column chunks (kernels.hpp: 64 lanes, coalesced index lists, uniform trip count;
//                columns of degree >= 8 on four lanes each), a wave-OR of what is left and of what moved, one vote, barrier.
//                Each E / V word has one writer; the votes are the only LDS atomics.
//     epilogue   the same ballot transpose back, population counts for `unresolved`.
// The chunk descriptors sit in LDS (a broadcast read per chunk and pass, no scalar load from device memory inside the passes);
// the index lists are read through the vector cache, 128 bytes per wave and trip.
#include <hip/hip_runtime.h>

#include "device_philox.hpp"
#include "kernels.hpp"
#include "launch_lds.hpp"
#include "plan.hpp"

namespace ldpc_amd
{

namespace
{
constexpr int kErasureChannelThreads = 256;
constexpr int kErasureWaves = kErasureThreads / 64;
using word_t = uint32_t;

__global__ __launch_bounds__(kErasureChannelThreads) void erasure_channel_kernel(ErasureChannelArgs a)
{
    const uint64_t g64 = static_cast<uint64_t>(blockIdx.x) * kErasureChannelThreads + threadIdx.x;
    if (g64 >= a.n * a.words)
        return;
    const uint32_t g = static_cast<uint32_t>(g64);
    const uint32_t row = g / a.words, w = g - row * a.words;
    const uint64_t frame = row;
    word_t cw = 0;
    const bool bytes = a.codeword_format == kBitsU8; // (uniform)
    if (a.codeword && a.word_bits && !bytes)
        cw = static_cast<const uint32_t *>(a.codeword)[frame * a.words + w];
    const uint8_t *src = static_cast<const uint8_t *>(a.codeword) + frame * a.nc + 32u * w;
    uint4 blk{0, 0, 0, 0};
    uint32_t have = 0xFFFFFFFFu; // the block in `blk` (no index reaches 2^32 / 4)
    word_t erased = 0, live = 0;
#pragma unroll 4
    for (uint32_t b = 0; b < 32; ++b)
    {
        const uint32_t t = a.col_tx[b * a.words + w];
        if (t == kErasureColPad)
            continue;
        live |= 1u << b;
        if (bytes && a.codeword && a.word_bits)
            cw |= static_cast<word_t>(src[b] != 0 ? 1 : 0) << b;
        if (t == kErasureColKnown)
            continue;
        bool hit = true; // kErasureColErased
        if (t != kErasureColErased)
        {
            if ((t >> 2) != have)
            {
                have = t >> 2;
                blk = philox_block(a.key[0], a.key[1], a.frame0 + frame, have, kTagDraw);
            }
            hit = counter_hit(word_of(blk, static_cast<int>(t & 3u)), a.eps);
        }
        erased |= static_cast<word_t>(hit ? 1 : 0) << b;
    }
    if (a.erased_bits)
        a.erased_bits[frame * a.words + w] = erased;
    if (a.word_bits)
        a.word_bits[frame * a.words + w] = cw & live & ~erased;
}

__device__ __forceinline__ word_t erasure_wave_or(word_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v |= static_cast<word_t>(__shfl_xor(static_cast<int>(v), o, 64));
    return v;
}

// Two 32 x 32 bit transposes per wave, one per half: lane l returns y with bit j of y = bit (l & 31) of the x of lane
// (l & 32) + j.  Ballot j is bit j of every lane's x; the lane whose index is j keeps its half of it.  (Its own inverse: rows
// of frames to column slices on the way in, slices to rows on the way out.)  Every lane of the wave must call it.
__device__ __forceinline__ word_t transpose_halves(word_t x, uint32_t lane)
{
    word_t y = 0;
#pragma unroll 4 // (unrolled whole, the 32 ballots of two transposes in flight spill scalar registers)
    for (uint32_t j = 0; j < 32; ++j)
    {
        const uint64_t m = __ballot(((x >> j) & 1u) != 0);
        const word_t mine = lane < 32 ? static_cast<word_t>(m) : static_cast<word_t>(m >> 32);
        y = (lane & 31u) == j ? mine : y;
    }
    return y;
}

// (eight waves per SIMD: 64 registers, so that registers never hold the occupancy below what the small LDS footprint allows)
__global__ __launch_bounds__(kErasureThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void erasure_decode_kernel(const ErasureDecodeArgs a)
{
    extern __shared__ word_t erasure_lds[];
    const uint32_t nc = a.nc, mc = a.mc, W = a.words, chunks = a.cn_chunks + a.vn_chunks;
    word_t *E = erasure_lds, *V = E + nc + 1, *ONE = V + nc + 1, *VAL = ONE + mc + 1;
    uint32_t *desc = VAL + mc + 1;
    word_t *still = desc + 2 * chunks, *changed = still + 2;
    uint32_t *left = changed + 2; // [32]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t f0 = static_cast<uint64_t>(blockIdx.x) * kErasureFrames;
    const uint32_t nf = static_cast<uint32_t>(a.n - f0 < kErasureFrames ? a.n - f0 : kErasureFrames); // frames of this group
    const word_t valid = nf == kErasureFrames ? ~word_t(0) : ((word_t(1) << nf) - 1);
    const uint32_t pairs = (W + 1) / 2;

    if (tid < kErasureVoteWords)
        still[tid] = 0;
    if (tid == 0)
        E[nc] = 0, V[nc] = 0, ONE[mc] = 0, VAL[mc] = 0;
    for (uint32_t i = tid; i < 2 * chunks; i += kErasureThreads)
        desc[i] = a.desc[i];
    // ---- rows of frames -> column slices.  A frame beyond the group reads nothing and votes 0 ----
    for (uint32_t p = wave; p < pairs; p += kErasureWaves) // (wave-uniform: every lane ballots)
    {
        const uint32_t w = 2 * p + (lane >> 5), f = lane & 31u;
        word_t xe = 0, xv = 0;
        if (f < nf && w < W)
        {
            const uint64_t at = (f0 + f) * W + w;
            xe = a.erased[at], xv = a.word[at];
        }
        const word_t se = transpose_halves(xe, lane), sv = transpose_halves(xv, lane);
        const uint32_t col = 32u * w + f; // (as a destination: slice of column 32 w + (lane & 31))
        if (col < nc)
            E[col] = se, V[col] = sv & ~se;
    }
    __syncthreads();

    const bool early = (a.flags & kErasureEarlyTerm) != 0, stalled = (a.flags & kErasureStopStalled) != 0;
    word_t act = a.iterations > 0 ? valid : 0; // frames still decoding (uniform)
    uint32_t my_iters = 0;                      // thread f < 32: iteration count of frame f
    for (uint32_t I = 0; I < a.iterations && act; ++I)
    {
        // ---- check nodes: ONE and VAL from E and V ----
        for (uint32_t k = wave; k < a.cn_chunks; k += kErasureWaves)
        {
            const uint32_t off = __builtin_amdgcn_readfirstlane(desc[2 * k]);
            const uint32_t trips = __builtin_amdgcn_readfirstlane(desc[2 * k + 1]);
            const uint16_t *idx = a.cn_entries + off + lane;
            word_t c0 = 0, c1 = 0, xa = 0;
#pragma unroll 4
            for (uint32_t j = 0; j < trips; ++j)
            {
                const uint32_t c = idx[64u * j];
                const word_t e = E[c];
                c1 |= c0 & e;
                c0 |= e;
                xa ^= V[c];
            }
            const uint32_t q = 64u * k + lane;
            if (q < mc)
            {
                const word_t one = c0 & ~c1;
                ONE[q] = one, VAL[q] = one & xa;
            }
        }
        __syncthreads();
        // ---- columns: an erased column with a check node that says ONE takes the OR of their VAL ----
        word_t any_e = 0, any_set = 0;
        for (uint32_t k = wave; k < a.vn_chunks; k += kErasureWaves)
        {
            const uint32_t off = __builtin_amdgcn_readfirstlane(desc[2 * (a.cn_chunks + k)]);
            const uint32_t d1 = __builtin_amdgcn_readfirstlane(desc[2 * (a.cn_chunks + k) + 1]);
            const uint32_t trips = d1 & ~kErasureWideChunk;
            const uint16_t *idx = a.vn_entries + off + lane;
            const uint32_t col = a.vn_col[64u * k + lane];
            word_t res = 0, val = 0;
#pragma unroll 4
            for (uint32_t j = 0; j < trips; ++j)
            {
                const uint32_t q = idx[64u * j];
                res |= ONE[q];
                val |= VAL[q];
            }
            bool writer = col < nc;
            if (d1 & kErasureWideChunk) // (uniform) four lanes per column: combine the quad, its first lane writes
            {
#pragma unroll
                for (int o = 1; o <= 2; o <<= 1)
                {
                    res |= static_cast<word_t>(__shfl_xor(static_cast<int>(res), o, 64));
                    val |= static_cast<word_t>(__shfl_xor(static_cast<int>(val), o, 64));
                }
                writer = writer && (lane & 3u) == 0;
            }
            if (writer)
            {
                const word_t e = E[col];
                const word_t set = e & res & act; // frames that have stopped keep their outputs
                const word_t ne = e & ~set;
                if (set)
                    E[col] = ne, V[col] |= val & set;
                any_e |= ne;
                any_set |= set;
            }
        }
        any_e = erasure_wave_or(any_e), any_set = erasure_wave_or(any_set);
        if (lane == 0)
        {
            if (any_e)
                atomicOr(&still[I & 1], any_e);
            if (any_set)
                atomicOr(&changed[I & 1], any_set);
        }
        __syncthreads();
        const word_t holds = still[I & 1], moved = changed[I & 1];
        if (tid == 0)
            still[(I + 1) & 1] = 0, changed[(I + 1) & 1] = 0; // (next written after the next pass's first barrier)
        // iters: with early termination the passes that left an erasure, else the passes the frame ran
        if (tid < kErasureFrames)
            my_iters += static_cast<uint32_t>(((early ? act & holds : act) >> tid) & 1u);
        act &= (early ? holds : ~word_t(0)) & (stalled ? moved : ~word_t(0));
    }
    __syncthreads();

    if (tid < nf && a.iters)
        a.iters[f0 + tid] = my_iters;
    // ---- column slices -> rows of frames; what is left of E, counted ----
    uint32_t count = 0;
    for (uint32_t p = wave; p < pairs; p += kErasureWaves)
    {
        const uint32_t w = 2 * p + (lane >> 5), f = lane & 31u;
        const uint32_t col = 32u * w + f;
        const word_t re = transpose_halves(col < nc ? E[col] : 0, lane); // (columns from nc on: the padding bits are 0)
        const word_t rv = transpose_halves(col < nc ? V[col] : 0, lane);
        if (f < nf && w < W)
        {
            const uint64_t at = (f0 + f) * W + w;
            if (a.erased_out)
                a.erased_out[at] = re;
            if (a.word_out)
                a.word_out[at] = rv;
            count += static_cast<uint32_t>(__popc(re));
        }
    }
    if (a.unresolved)
    {
        if (count)
            atomicAdd(&left[lane & 31u], count);
        __syncthreads();
        if (tid < nf)
            a.unresolved[f0 + tid] = left[tid];
    }
}
} // namespace

int launch_erasure_channel(const ErasureChannelArgs &a, void *stream)
{
    if (a.n == 0 || (!a.word_bits && !a.erased_bits))
        return hipSuccess;
    if (!a.col_tx || a.nc == 0 || a.words != (a.nc + 31u) / 32u || (a.codeword && !bits_format_known(a.codeword_format)) ||
        a.n * a.words >= (1ull << 31))
        return hipErrorInvalidValue;
    const uint64_t lanes = a.n * a.words;
    const dim3 grid(static_cast<unsigned>((lanes + kErasureChannelThreads - 1) / kErasureChannelThreads)), block(kErasureChannelThreads);
    hipLaunchKernelGGL(erasure_channel_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError();
}

int launch_erasure_decode(const ErasureDecodeArgs &a, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    const uint64_t groups = (a.n + kErasureFrames - 1) / kErasureFrames;
    if (!a.word || !a.erased || !a.desc || !a.cn_entries || !a.vn_entries || !a.vn_col || a.nc == 0 || a.nc > 65535u || a.mc > 65535u ||
        a.words != (a.nc + 31u) / 32u || a.cn_chunks != (a.mc + 63u) / 64u || (a.flags & ~(kErasureEarlyTerm | kErasureStopStalled)) ||
        a.lds_bytes != erasure_lds_bytes(a.nc, a.mc, a.cn_chunks + a.vn_chunks) || a.lds_bytes > kCuLdsBytes || groups >= (1ull << 31))
        return hipErrorInvalidValue;
    return launch_with_lds(erasure_decode_kernel, dim3(static_cast<unsigned>(groups)), dim3(kErasureThreads), a.lds_bytes, stream, a);
}

} // namespace ldpc_amd
