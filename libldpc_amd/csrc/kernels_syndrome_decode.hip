// kernels_syndrome_decode.hip — quantized (fixed-point) min-sum decoding of the batch interface TOWARD A GIVEN SYNDROME
// (include/ldpc_amd.h, ldpc_hip_syndrome_decode_batch states the arithmetic): which word with H x = s fits these LLRs, for
// the s the caller holds — syndrome-based source coding, reconciliation, every syndrome-measuring decoder.  The iteration is
// that of kernels_qms.hip (one byte per message, a check node's messages padded to whole words, 32-bit totals, the 128-byte
// correction table, the vote words) with two changes: a check node's sign parity starts at its syndrome bit, and the stop
// test asks for the syndrome s instead of zero.  Everything after the one quantization of the input is integer arithmetic:
// every output bit follows from the contract and is held against a numpy mirror (tests/syndrome_decode_ref.py).
//
// ONE WORKGROUP (256 threads) = ONE FRAME, on the tables of DevQmsPlan (read from global memory: all frames share them).
// What LDS holds per frame (kernels.hpp, syndrome_decode_lds_bytes; every part starts on 16 bytes): the messages; the
// totals A[nc]; the table, two vote words and four partial sums; the frame's syndrome, bit c = check node c in the ORDER OF
// THE TABLES (Plan::cn_rank_row maps it to the row the caller's bit sits at); L[nc], the quantized inputs as bytes.
//   prologue   a thread per COLUMN reads the element in place in its own type (coalesced), quantizes it and stores the
//              byte at the column's rank; a thread per check node fetches its syndrome bit, a wave's ballot is two words.
//   epilogue   a thread per column again: the total through the column map, llr_out coalesced, the packed decisions by a
//              ballot per 64 columns; the weight = the check nodes whose test fails on those decisions, a wave reduction
//              and four partial sums.
// No binary64 area, no static LDS, nothing that depends on timing.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch_lds.hpp"

namespace ldpc_amd
{

namespace
{
constexpr int kSdThreads = 256;

// clamp(rint(fl(w * inv)), -qmax, +qmax), the clamp in binary64 (an infinity or 99999.9 saturates); rint is round-half-
// to-even; a NaN gives 0 (kernels_qms.hip, qms_quantize: the same quantizer)
__device__ __forceinline__ int sd_quantize(double w, double inv, int qmax)
{
#pragma clang fp contract(off)
    const double x = __builtin_rint(w * inv);
    const double q = static_cast<double>(qmax);
    return x >= q ? qmax : (x <= -q ? -qmax : (x == x ? static_cast<int>(x) : 0));
}

// element i of the typed input as its quantized value; an int8 k counts steps: clamp(k)
__device__ __forceinline__ int sd_load(const SyndromeDecodeArgs &a, uint64_t i)
{
    switch (a.llr_type) // (uniform)
    {
    case kLlrF64: return sd_quantize(static_cast<const double *>(a.llr)[i], a.inv, a.qmax);
    case kLlrF32: return sd_quantize(static_cast<double>(static_cast<const float *>(a.llr)[i]), a.inv, a.qmax);
    case kLlrF16: return sd_quantize(static_cast<double>(static_cast<const _Float16 *>(a.llr)[i]), a.inv, a.qmax);
    default:
    {
        const int k = static_cast<const int8_t *>(a.llr)[i];
        return k > a.qmax ? a.qmax : (k < -a.qmax ? -a.qmax : k);
    }
    }
}

__device__ __forceinline__ int sd_byte_of(uint32_t word, int b) { return static_cast<int>(static_cast<int8_t>(word >> (8 * b))); }
__device__ __forceinline__ int sd_bit(const uint32_t *words, int i) { return static_cast<int>((words[i >> 5] >> (i & 31)) & 1u); }

// variable nodes: A = L + the sum of the node's messages (exact), each message replaced by clamp(A - message)
__device__ __forceinline__ void sd_vn_pass(const DevQmsPlan &Q, int nc, int tid, const int8_t *L, int8_t *msg, int32_t *A, int qmax)
{
    for (int r = tid; r < nc; r += kSdThreads)
    {
        const uint32_t b = Q.vn_start[r], e = Q.vn_start[r + 1];
        int acc = L[r];
        for (uint32_t i = b; i < e; ++i)
            acc += msg[Q.vn_slot[i]];
        A[r] = acc;
        for (uint32_t i = b; i < e; ++i)
        {
            const uint32_t s = Q.vn_slot[i];
            const int v = acc - msg[s];
            msg[s] = static_cast<int8_t>(v > qmax ? qmax : (v < -qmax ? -qmax : v));
        }
    }
}

// check nodes: message j := +-lut[the smallest |message| of the others], negative iff (the others that are < 0) + the check
// node's syndrome bit is odd
__device__ __forceinline__ void sd_cn_pass(const DevQmsPlan &Q, int mc, int tid, int8_t *msg, const uint8_t *lut, const uint32_t *syn)
{
    for (int c = tid; c < mc; c += kSdThreads)
    {
        const uint2 d = *reinterpret_cast<const uint2 *>(Q.cn_desc + 2 * c);
        uint32_t *row = reinterpret_cast<uint32_t *>(msg + d.x);
        const int deg = static_cast<int>(d.y), words = (deg + 3) >> 2;
        int min1 = 127, min2 = 127, arg = 0, par = sd_bit(syn, c);
        for (int w = 0; w < words; ++w)
        {
            const uint32_t x = row[w];
#pragma unroll
            for (int b = 0; b < 4; ++b)
            {
                const int k = 4 * w + b;
                if (k >= deg)
                    break;
                const int v = sd_byte_of(x, b);
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
                const bool neg = (par ^ static_cast<int>(sd_byte_of(x, b) < 0)) != 0;
                y |= (static_cast<uint32_t>(neg ? -mag : mag) & 0xFFu) << (8 * b);
            }
            row[w] = y;
        }
    }
}

// this thread's check nodes whose XOR of the decisions A <= 0 over the row differs from the syndrome bit
__device__ __forceinline__ int sd_unmet(const DevQmsPlan &Q, int mc, int tid, const int32_t *A, const uint32_t *syn)
{
    int bad = 0;
    for (int c = tid; c < mc; c += kSdThreads)
    {
        const uint2 d = *reinterpret_cast<const uint2 *>(Q.cn_desc + 2 * c);
        const uint16_t *vn = Q.cn_vn + d.x;
        int p = sd_bit(syn, c);
        for (uint32_t k = 0; k < d.y; ++k)
            p ^= static_cast<int>(A[vn[k]] <= 0);
        bad += p;
    }
    return bad;
}

__global__ __launch_bounds__(kSdThreads) void syndrome_decode_kernel(const SyndromeDecodeArgs a, const DevQmsPlan Q)
{
    extern __shared__ uint4 sd_lds[];
    const int nc = static_cast<int>(a.nc), mc = static_cast<int>(a.mc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t frame = blockIdx.x;
    if (frame >= a.n)
        return;
    unsigned char *lds = reinterpret_cast<unsigned char *>(sd_lds);
    int8_t *msg = reinterpret_cast<int8_t *>(lds);
    int32_t *A = reinterpret_cast<int32_t *>(lds + syndrome_decode_round16(Q.slots));
    uint8_t *lut = reinterpret_cast<uint8_t *>(A) + syndrome_decode_round16(4 * static_cast<size_t>(nc));
    uint32_t *vote = reinterpret_cast<uint32_t *>(lut + 128); // [2], used in turn: iteration I votes in word I & 1
    uint32_t *part = vote + 4;                                // [4]: a wave's share of the weight
    uint32_t *syn = reinterpret_cast<uint32_t *>(lut + kSyndromeDecodeSideBytes);
    int8_t *L = reinterpret_cast<int8_t *>(syn) + syndrome_decode_round16(4 * static_cast<size_t>(a.syn_words));
    const int qmax = a.qmax;

    {
        uint32_t *z = reinterpret_cast<uint32_t *>(msg);
        for (uint32_t i = tid; i < Q.slots / 4; i += kSdThreads)
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
        for (int c = tid; c < nc; c += kSdThreads)
            L[a.col_rank[c]] = static_cast<int8_t>(sd_load(a, at + static_cast<uint64_t>(c)));
        // the syndrome: check node c of the tables is row cn_row[c] of the caller's
        for (int base = 64 * wave; base < mc; base += kSdThreads) // (wave-uniform)
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
    __syncthreads();
    sd_vn_pass(Q, nc, tid, L, msg, A, qmax); // over all-zero messages: A = L, v2c = L
    __syncthreads();

    uint32_t I = 0;
    while (I < a.iterations)
    {
        sd_cn_pass(Q, mc, tid, msg, lut, syn);
        __syncthreads();
        sd_vn_pass(Q, nc, tid, L, msg, A, qmax);
        __syncthreads();
        if (a.early_term)
        {
            const int bad = sd_unmet(Q, mc, tid, A, syn);
            // a wave with an unmet check node raises this iteration's word; thread 0 clears the other word for the next
            // iteration (read last an iteration ago, two barriers back)
            const bool wave_bad = __ballot(bad != 0) != 0;
            if (wave_bad && lane == 0)
                vote[I & 1] = 1;
            if (tid == 0)
                vote[(I + 1) & 1] = 0;
            __syncthreads();
            if (vote[I & 1] == 0)
                break;
        }
        ++I;
    }
    if (tid == 0 && a.iters)
        a.iters[frame] = I;
    // a thread per column: the total through the column map, the decisions of 64 columns by a ballot
    for (int base = 64 * wave; base < nc; base += kSdThreads) // (wave-uniform)
    {
        const int c = base + lane;
        bool one = false;
        if (c < nc)
        {
            const int x = A[a.col_rank[c]];
            one = x <= 0;
            if (a.llr_out)
                a.llr_out[frame * a.nc + static_cast<uint64_t>(c)] = static_cast<double>(x) * a.step;
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
        int bad = sd_unmet(Q, mc, tid, A, syn);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            bad += __shfl_xor(bad, o, 64);
        if (lane == 0)
            part[wave] = static_cast<uint32_t>(bad);
        __syncthreads();
        if (tid == 0)
            a.weight[frame] = part[0] + part[1] + part[2] + part[3];
    }
}
} // namespace

int launch_syndrome_decode(const SyndromeDecodeArgs &a, const DevQmsPlan &Q, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    if (!Q.cn_desc || !Q.cn_vn || !Q.vn_start || !Q.vn_slot || (Q.slots & 3u) || a.qmax < 1 || a.qmax > 127 || a.nc == 0 || a.nc > 0xFFFFu ||
        a.mc == 0 || a.words != (a.nc + 31) / 32 || a.syn_words != (a.mc + 31) / 32 || !a.col_rank || !a.cn_row || !a.llr ||
        llr_type_bytes(a.llr_type) == 0 || (a.syndrome && !bits_format_known(a.syndrome_format)) ||
        a.lds_bytes != syndrome_decode_lds_bytes(Q.slots, a.nc, a.mc) || a.lds_bytes > kCuLdsBytes || a.n > (1ull << 20))
        return hipErrorInvalidValue;
    return launch_with_lds(syndrome_decode_kernel, dim3(static_cast<unsigned>(a.n)), dim3(kSdThreads), a.lds_bytes, stream, a, Q);
}

} // namespace ldpc_amd
