// kernels_qms.hip — opt-in NON-PARITY QUANTIZED (fixed-point) min-sum decoding ("BP_MS" with
// ldpc_hip_set_min_sum_quantization(bits, step); include/ldpc_amd.h states the arithmetic).  Messages of 2..8 bits on a
// saturating integer datapath, the reference's flooding schedule, early stop and iteration count.  Everything after the
// one quantization of the channel LLRs is integer arithmetic, so every output bit follows from the contract and is held
// against a numpy mirror bit for bit (tests/quantized_minsum_ref.py).  The reference computes in binary64
// (decoder.cpp:22-76): the results are not its own.
//
// ONE WORKGROUP (256 threads) = ONE FRAME.  What LDS holds per frame (plan.hpp, qms_region_bytes):
//   * first the nc binary64 channel LLRs, written by channel_init as everywhere (all channel and noise modes), and behind
//     them L[nc], one byte each: the LLRs quantized once;
//   * then, over the binary64 area: the messages, ONE BYTE per edge, a check node's messages consecutive and padded to a
//     whole number of words (c2v overwrites v2c in place and back); the totals A[nc], 32 bits each (the decisions are read
//     off them); the correction table, 128 bytes; two words for the workgroup's vote.
// One iteration: a thread per check node reads its row a WORD at a time (rows start on a word: no sub-dword access in this
// pass; neighbouring threads hold rows of equal degree), takes min1, min2, argmin and the sign parity, reads the row again
// and writes the c2v words; barrier; a thread per variable node gathers its bytes, stores the total and writes the
// saturated v2c bytes back; barrier; with early termination the syndrome of the decisions and a workgroup vote.  No
// binary64 and no per-thread array inside the loop, any check-node and variable-node degree.  The graph tables are read
// from global memory: all frames share them.
//
// Iteration count returned: the index of the iteration whose decisions passed the syndrome check (the reference's
// convention, decoder.cpp:21-22,74-77), otherwise `iterations`.
#include <hip/hip_runtime.h>

#include "device_channel.hpp"
#include "kernels.hpp"
#include "launch_lds.hpp"

namespace ldpc_amd
{

namespace
{
constexpr int kQmsThreads = 256;

// clamp(rint(fl(llr * inv)), -qmax, +qmax), the clamp in binary64 (an infinity or 99999.9 saturates); rint is round-half-
// to-even; a NaN gives 0
__device__ __forceinline__ int qms_quantize(double llr, double inv, int qmax)
{
#pragma clang fp contract(off)
    const double x = __builtin_rint(llr * inv);
    const double q = static_cast<double>(qmax);
    return x >= q ? qmax : (x <= -q ? -qmax : (x == x ? static_cast<int>(x) : 0));
}

__device__ __forceinline__ int byte_of(uint32_t word, int b) { return static_cast<int>(static_cast<int8_t>(word >> (8 * b))); }

// variable nodes: A = L + the sum of the node's messages (exact), each message replaced by clamp(A - message)
__device__ __forceinline__ void qms_vn_pass(const DevQmsPlan &Q, int nc, int tid, const int8_t *L, int8_t *msg, int32_t *A, int qmax)
{
    for (int r = tid; r < nc; r += kQmsThreads)
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

// check nodes: message j := +-lut[the smallest |message| of the others], negative iff an odd number of the others is < 0
__device__ __forceinline__ void qms_cn_pass(const DevQmsPlan &Q, int mc, int tid, int8_t *msg, const uint8_t *lut)
{
    for (int c = tid; c < mc; c += kQmsThreads)
    {
        const uint2 d = *reinterpret_cast<const uint2 *>(Q.cn_desc + 2 * c);
        uint32_t *row = reinterpret_cast<uint32_t *>(msg + d.x);
        const int deg = static_cast<int>(d.y), words = (deg + 3) >> 2;
        int min1 = 127, min2 = 127, arg = 0, par = 0;
        for (int w = 0; w < words; ++w)
        {
            const uint32_t x = row[w];
#pragma unroll
            for (int b = 0; b < 4; ++b)
            {
                const int k = 4 * w + b;
                if (k >= deg)
                    break;
                const int v = byte_of(x, b);
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
                const bool neg = (par ^ static_cast<int>(byte_of(x, b) < 0)) != 0;
                y |= (static_cast<uint32_t>(neg ? -mag : mag) & 0xFFu) << (8 * b);
            }
            row[w] = y;
        }
    }
}

template <bool WANT_LLR>
__global__ __launch_bounds__(kQmsThreads) void decode_qms_kernel(const DecodeArgs a, const DevQmsPlan Q, const QmsArgs q)
{
    extern __shared__ double lds_d[];
    const DevPlan &P = a.plan;
    const int nc = P.nc, mc = P.mc;
    const int tid = threadIdx.x;
    const uint64_t frame = blockIdx.x;
    if (frame >= a.n_frames)
        return;
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds_d);
    int8_t *msg = reinterpret_cast<int8_t *>(lds);
    int32_t *A = reinterpret_cast<int32_t *>(lds + Q.slots);
    uint8_t *lut = lds + Q.slots + 4 * static_cast<uint32_t>(nc);
    uint32_t *vote = reinterpret_cast<uint32_t *>(lut + 128); // [2], used in turn: iteration I votes in word I & 1
    int8_t *L = reinterpret_cast<int8_t *>(lds + Q.work_bytes);
    const uint8_t *cw = a.codeword ? a.codeword + frame * nc : nullptr;
    const int qmax = q.qmax;

    channel_init<kQmsThreads, kNoiseAny>(a, frame, lds_d, tid); // binary64 channel + LLR initialisation, as everywhere
    __syncthreads();
    {
        double *o = a.llr_in_dump ? a.llr_in_dump + frame * nc : nullptr;
        for (int r = tid; r < nc; r += kQmsThreads)
        {
            const double x = lds_d[r];
            if (o)
                o[P.rank_col[r]] = x; // (llr_in stays the unquantized value)
            L[r] = static_cast<int8_t>(qms_quantize(x, q.inv, qmax));
        }
    }
    __syncthreads(); // the binary64 area is free
    {
        uint32_t *z = reinterpret_cast<uint32_t *>(msg);
        for (uint32_t i = tid; i < Q.slots / 4; i += kQmsThreads)
            z[i] = 0;
        if (tid < 32) // (a select chain over the launch arguments: indexing them by a lane's number would put them in scratch)
        {
            uint32_t w = 0;
#pragma unroll
            for (int i = 0; i < 32; ++i)
                w = tid == i ? q.lut[i] : w;
            reinterpret_cast<uint32_t *>(lut)[tid] = w;
        }
        else if (tid < 34)
            vote[tid - 32] = 0;
    }
    __syncthreads();
    qms_vn_pass(Q, nc, tid, L, msg, A, qmax); // over all-zero messages: v2c = L
    __syncthreads();

    uint32_t I = 0;
    while (I < a.iterations)
    {
        qms_cn_pass(Q, mc, tid, msg, lut);
        __syncthreads();
        qms_vn_pass(Q, nc, tid, L, msg, A, qmax);
        __syncthreads();
        if (a.early_term) // syndrome of the decisions A <= 0 (decoder.cpp:58,66-72)
        {
            int bad = 0;
            for (int c = tid; c < mc; c += kQmsThreads)
            {
                const uint2 d = *reinterpret_cast<const uint2 *>(Q.cn_desc + 2 * c);
                const uint16_t *vn = Q.cn_vn + d.x;
                int p = 0;
                for (uint32_t k = 0; k < d.y; ++k)
                    p ^= static_cast<int>(A[vn[k]] <= 0);
                bad |= p;
            }
            // a wave with an unsatisfied check node raises this iteration's word; thread 0 clears the other word for the
            // next iteration (read last an iteration ago, two barriers back)
            const bool wave_bad = __ballot(bad != 0) != 0;
            if (wave_bad && (tid & 63) == 0)
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
    const bool ran = a.iterations > 0;
    uint8_t *h = a.hard ? a.hard + frame * nc : nullptr;
    for (int r = tid; r < nc; r += kQmsThreads)
    {
        const int x = A[r];
        if (h)
            h[P.rank_col[r]] = ran ? static_cast<uint8_t>(x <= 0) : 0; // mCO is still zero-initialised when no iteration ran
        if constexpr (WANT_LLR)
            a.llr_out[frame * nc + P.rank_col[r]] = ran ? static_cast<double>(x) * q.step : 0.0;
    }
    if (a.bit_errors)
    {
        int err = 0;
        for (int i = tid; i < P.n_bitpos; i += kQmsThreads)
        {
            const int est = ran ? static_cast<int>(A[P.tx_rank[i]] <= 0) : 0;
            const int tx = cw ? static_cast<int>(cw[P.bit_pos[i]]) : 0;
            err += est != tx;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            err += __shfl_xor(err, o, 64);
        int *part = reinterpret_cast<int *>(lut); // (the table has served: every thread is past the loop's last barrier)
        if ((tid & 63) == 0)
            part[tid >> 6] = err;
        __syncthreads();
        if (tid == 0)
        {
            int sum = 0;
            for (int w = 0; w < kQmsThreads / 64; ++w)
                sum += part[w];
            a.bit_errors[frame] = static_cast<uint32_t>(sum);
        }
    }
}
} // namespace

int launch_decode_qms(const DecodeArgs &a, const DevQmsPlan &Q, const QmsArgs &q, void *stream)
{
    if (a.n_frames == 0)
        return hipSuccess;
    const uint64_t nc = static_cast<uint64_t>(a.plan.nc);
    if (!Q.cn_desc || !Q.cn_vn || !Q.vn_start || !Q.vn_slot || (Q.slots & 3u) || q.qmax < 1 || q.qmax > 127 || a.plan.nc <= 0 ||
        nc > 0xFFFF || Q.work_bytes < 8 * nc || Q.work_bytes < Q.slots + 4 * nc + 144 || Q.region_bytes < Q.work_bytes + nc ||
        Q.region_bytes > kCuLdsBytes || a.n_frames > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    void (*k)(const DecodeArgs, const DevQmsPlan, const QmsArgs) = a.llr_out ? decode_qms_kernel<true> : decode_qms_kernel<false>;
    return launch_with_lds(k, dim3(static_cast<unsigned>(a.n_frames)), dim3(kQmsThreads), Q.region_bytes, stream, a, Q, q);
}

} // namespace ldpc_amd
