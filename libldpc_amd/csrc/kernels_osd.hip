// kernels_osd.hip — ordered-statistics decoding of the batch interface (include/ldpc_amd.h, ldpc_hip_osd_batch): the codeword
// that agrees with the hard decisions on the most reliable independent positions, and the best of the first single flips
// among them.  ONE WORKGROUP = ONE FRAME; the frame's whole check matrix over GF(2) lives in LDS (layout: kernels.hpp).
//   load       the elements are read in place in their own type and widened exactly; a wave's ballot is a 64-bit word of the
//              decisions z; the reliabilities q go into the region the matrix takes later, as sort keys.
//   codeword   one thread per check node walks its list in H and XORs z.  A frame whose z is a codeword leaves here.
//   order      the rank of column c is the number of columns with a smaller (q, c): a thread counts it over all keys (every
//              lane reads the same key: a broadcast) and writes order[rank] = c.  After the barrier the keys are dead.
//   build      a thread clears its rows and toggles one bit per listed column — an entry listed twice cancels.
//   eliminate  Gauss-Jordan over the columns in the order, as in kernels_erasure_solve.hip: thread t owns the rows t, t + T,
//              ...; per column every thread offers its first unused row with that bit, the first of the wave by ballots,
//              across waves by one LDS atomicMin per wave into one of three vote words used in turn; ONE barrier; the owner
//              marks the pivot row and notes the column in the row's side word, every other row with the bit takes the pivot
//              row XORed in.  A column without a pivot costs the vote only: it joins K, and thread 0 moves it to the front
//              of the order (position |K| so far <= the position just read, so nothing unread is overwritten).
//   order 0    the reduced row of pivot column p holds p, no other solved column and its part over K: x0[p] = the parity of
//              that part ANDed with z.  The owner sets the bit, reads q[p] again and leaves (q[p], p, x0[p] != z[p]) in the
//              side word; the metric and the flips of x0 are sums by LDS atomics.
//   candidates a wave per candidate j (the t-th column of K): flipping j flips the pivot of every row with bit j, so
//              metric(x_j) = metric(x0) + q[j] + the sum over those rows of +q (agreed with z) or -q (did not).  Rows are strided
//              over the lanes, sums are integer wave reductions; a wave keeps its first best, the workgroup the best of those
//              by (metric, t).  The winner is applied to the word by LDS atomics.
// Results go out by ordinary vector stores; nothing here depends on timing: minima, XORs and integer sums only.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch_lds.hpp"
#include "osd_device.hpp"
#include "plan.hpp"

namespace ldpc_amd
{

namespace
{
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
// the 32-bit scalars: [0..2] the pivot votes, then
constexpr int kOsdOdd = 3, kOsdFlips0 = 4;
constexpr uint64_t kOsdDiffers = 1ull << 48; // side word: q in bits 0..31, the pivot column in 32..47, x0 != z there in 48

__global__ __launch_bounds__(kOsdMaxThreads) void osd_kernel(const OsdArgs a)
{
    extern __shared__ uint64_t osd_lds[];
    const uint32_t nc = a.nc, mc = a.mc, nw = static_cast<uint32_t>(osd_row_words(nc)), S = static_cast<uint32_t>(osd_stride(nc));
    uint64_t *rows = osd_lds;
    uint32_t *key = reinterpret_cast<uint32_t *>(osd_lds); // [nc], until the matrix is built
    uint64_t *Z = rows + osd_matrix_bytes(nc, mc) / 8, *P = Z + nw, *X = P + nw; // [nw] each
    uint64_t *sum64 = X + nw;                                                  // [0] metric(x0), [1 + wave] the wave's best metric
    uint32_t *scal = reinterpret_cast<uint32_t *>(sum64 + 1 + kOsdMaxThreads / 64); // [16]
    uint32_t *best_t = scal + 16, *best_flips = best_t + kOsdMaxThreads / 64;   // [16] each: 328 bytes of kOsdSideBytes
    uint16_t *order = reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(sum64) + kOsdSideBytes); // [nc]
    uint32_t *X32 = reinterpret_cast<uint32_t *>(X);
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = T >> 6;
    const uint64_t at = static_cast<uint64_t>(blockIdx.x) * nc;

    // ---- load ----
    for (uint32_t base = 64u * wave; base < 64u * nw; base += T) // (wave-uniform)
    {
        const uint32_t c = base + lane;
        bool one = false;
        if (c < nc)
        {
            const double w = osd_widen(a, at + c);
            key[c] = osd_reliability(w);
            one = w <= 0.0; // (a NaN: 0)
        }
        const uint64_t m = __ballot(one);
        if (lane == 0)
            Z[base >> 6] = m, P[base >> 6] = 0;
    }
    if (tid < 16)
        scal[tid] = tid < 3 ? kNoRow : 0;
    if (tid == 0)
        sum64[0] = 0;
    __syncthreads();
    // ---- codeword ----
    bool odd = false;
    for (uint32_t r = tid; r < mc; r += T)
    {
        uint32_t s = 0;
        for (uint32_t q = a.row_ptr[r], end = a.row_ptr[r + 1]; q < end; ++q)
        {
            const uint32_t c = a.row_col[q];
            s ^= static_cast<uint32_t>(Z[c >> 6] >> (c & 63u)) & 1u;
        }
        odd = odd || s != 0;
    }
    if (odd)
        atomicOr(&scal[kOsdOdd], 1u);
    __syncthreads();
    uint32_t status = kOsdCodeword, flips = 0, column = kOsdNoColumn;
    uint64_t metric = 0;
    const uint32_t *word = reinterpret_cast<const uint32_t *>(Z);
    if (scal[kOsdOdd]) // (uniform, as every branch on the votes and the sums below)
    {
        // ---- order ----
        for (uint32_t c = tid; c < nc; c += T)
        {
            const uint32_t k = key[c];
            uint32_t rank = 0;
            for (uint32_t o = 0; o < nc; ++o)
            {
                const uint32_t ko = key[o];
                rank += (ko < k || (ko == k && o < c)) ? 1u : 0u;
            }
            order[rank] = static_cast<uint16_t>(c);
        }
        __syncthreads();
        // ---- build ----
        for (uint32_t r = tid; r < mc; r += T)
        {
            uint64_t *row = rows + static_cast<size_t>(r) * S;
            for (uint32_t w = 0; w < S; ++w)
                row[w] = 0;
            for (uint32_t q = a.row_ptr[r], end = a.row_ptr[r + 1]; q < end; ++q)
            {
                const uint32_t c = a.row_col[q];
                row[c >> 6] ^= 1ull << (c & 63u);
            }
        }
        __syncthreads();
        // ---- eliminate ----
        uint32_t used = 0, kept = 0; // bit k: my row tid + k T is a pivot row; |K| so far
        const uint32_t rows_per_thread = (mc + T - 1u) / T;
        for (uint32_t i = 0; i < nc; ++i)
        {
            const uint32_t c = order[i], wj = c >> 6, bj = c & 63u;
            uint32_t best = kNoRow;
            for (uint32_t k = 0, row = tid; k < rows_per_thread; ++k, row += T) // (uniform: every lane ballots)
            {
                const bool offer = row < mc && !((used >> k) & 1u) && ((rows[static_cast<size_t>(row) * S + wj] >> bj) & 1u);
                if (const uint64_t m = __ballot(offer))
                {
                    best = row - lane + static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
                    break;
                }
            }
            if (lane == 0 && best != kNoRow)
                atomicMin(&scal[i % 3u], best);
            __syncthreads();
            const uint32_t p = scal[i % 3u];
            if (tid == 0)
                scal[(i + 2u) % 3u] = kNoRow; // (read last before this barrier, voted on next after the next one)
            if (p == kNoRow)
            {
                if (tid == 0)
                    order[kept] = static_cast<uint16_t>(c); // (kept <= i: every thread has read that position)
                ++kept;
                continue;
            }
            if (tid == 0)
                P[wj] |= 1ull << bj;
            const uint64_t *pivot = rows + static_cast<size_t>(p) * S;
            for (uint32_t k = 0, row = tid; row < mc; ++k, row += T)
            {
                uint64_t *mine = rows + static_cast<size_t>(row) * S;
                if (!((mine[wj] >> bj) & 1u))
                    continue;
                if (row == p)
                {
                    used |= 1u << k;
                    mine[nw] = c; // (the side word: nobody else reads it before the barrier behind the loop)
                    continue;
                }
#pragma unroll 4
                for (uint32_t w = 0; w < nw; ++w)
                    if (const uint64_t x = pivot[w]) // (the same for every lane: a zero word costs its broadcast read only)
                        mine[w] ^= x;
            }
        }
        __syncthreads();
        // ---- order 0 ----
        for (uint32_t w = tid; w < nw; w += T)
            X[w] = Z[w] & ~P[w];
        __syncthreads();
        for (uint32_t k = 0, row = tid; row < mc; ++k, row += T)
        {
            uint64_t *mine = rows + static_cast<size_t>(row) * S;
            if (!((used >> k) & 1u))
                continue; // (all zero, the side word too)
            const uint32_t c = static_cast<uint32_t>(mine[nw]);
            uint32_t parity = 0;
            for (uint32_t w = 0; w < nw; ++w)
                parity ^= static_cast<uint32_t>(__popcll(mine[w] & Z[w] & ~P[w]));
            parity &= 1u;
            const bool differs = parity != (static_cast<uint32_t>(Z[c >> 6] >> (c & 63u)) & 1u);
            const uint32_t q = osd_reliability(osd_widen(a, at + c));
            if (parity)
                atomicOr(&X32[c >> 5], 1u << (c & 31u));
            mine[nw] = q | (static_cast<uint64_t>(c) << 32) | (differs ? kOsdDiffers : 0);
            if (differs)
            {
                atomicAdd(reinterpret_cast<unsigned long long *>(&sum64[0]), static_cast<unsigned long long>(q));
                atomicAdd(&scal[kOsdFlips0], 1u);
            }
        }
        __syncthreads();
        // ---- candidates ----
        const uint64_t metric0 = sum64[0];
        const uint32_t tried = a.candidates < kept ? a.candidates : kept;
        uint64_t bm = metric0;
        uint32_t bt = kNoRow, bf = 0;
        for (uint32_t t = wave; t < tried; t += waves) // (wave-uniform)
        {
            const uint32_t j = order[t], wj = j >> 6, bj = j & 63u;
            int64_t d = 0, f = 0;
            for (uint32_t row = lane; row < mc; row += 64u)
            {
                const uint64_t *r = rows + static_cast<size_t>(row) * S;
                if (!((r[wj] >> bj) & 1u))
                    continue;
                const uint64_t side = r[nw];
                const int64_t q = static_cast<int64_t>(side & 0xFFFFFFFFull);
                d += (side & kOsdDiffers) ? -q : q;
                f += (side & kOsdDiffers) ? -1 : 1;
            }
            d = osd_wave_sum(d), f = osd_wave_sum(f);
            const uint64_t m = metric0 + osd_reliability(osd_widen(a, at + j)) + static_cast<uint64_t>(d);
            if (m < bm)
                bm = m, bt = t, bf = static_cast<uint32_t>(f + 1);
        }
        if (lane == 0)
            sum64[1 + wave] = bm, best_t[wave] = bt, best_flips[wave] = bf;
        __syncthreads();
        metric = metric0, flips = scal[kOsdFlips0], status = kOsdOrder0;
        uint32_t wt = kNoRow, wf = 0;
        for (uint32_t v = 0; v < waves; ++v)
        {
            const uint64_t m = sum64[1 + v];
            const uint32_t t = best_t[v];
            if (t != kNoRow && (m < metric || (m == metric && t < wt)))
                metric = m, wt = t, wf = best_flips[v];
        }
        if (wt != kNoRow)
        {
            column = order[wt], flips += wf, status = kOsdReprocessed;
            const uint32_t wj = column >> 6, bj = column & 63u;
            if (tid == 0)
                atomicXor(&X32[column >> 5], 1u << (column & 31u));
            for (uint32_t row = tid; row < mc; row += T)
            {
                const uint64_t *r = rows + static_cast<size_t>(row) * S;
                if (!((r[wj] >> bj) & 1u))
                    continue;
                const uint32_t c = static_cast<uint32_t>(r[nw] >> 32) & 0xFFFFu;
                atomicXor(&X32[c >> 5], 1u << (c & 31u));
            }
            __syncthreads();
        }
        word = X32;
    }
    if (a.word_out)
        for (uint32_t w = tid; w < a.words; w += T)
            a.word_out[static_cast<uint64_t>(blockIdx.x) * a.words + w] = word[w];
    if (tid == 0)
    {
        if (a.flips)
            a.flips[blockIdx.x] = flips;
        if (a.metric)
            a.metric[blockIdx.x] = metric;
        if (a.flipped_column)
            a.flipped_column[blockIdx.x] = column;
        if (a.status)
            a.status[blockIdx.x] = status;
    }
}
} // namespace

int launch_osd(const OsdArgs &a, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    if (!a.llr || !a.row_ptr || !a.row_col || llr_type_bytes(a.llr_type) == 0 || a.nc == 0 || a.nc > 0xFFFFu || a.mc == 0 ||
        a.words != (a.nc + 31u) / 32u || a.threads == 0 || a.threads % 64u || a.threads > kOsdMaxThreads ||
        a.mc > static_cast<uint64_t>(kOsdRowsPerThread) * a.threads || a.lds_bytes != osd_lds_bytes(a.nc, a.mc) || a.lds_bytes > kCuLdsBytes ||
        a.n > (1ull << 20))
        return hipErrorInvalidValue;
    return launch_with_lds(osd_kernel, dim3(static_cast<unsigned>(a.n)), dim3(a.threads), a.lds_bytes, stream, a);
}

} // namespace ldpc_amd
