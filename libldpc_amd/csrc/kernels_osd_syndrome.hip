// kernels_osd_syndrome.hip — ordered-statistics decoding TOWARD A GIVEN SYNDROME with a bounded order-2 sweep (include/ldpc_amd.h,
// ldpc_hip_osd_syndrome_batch): the word x with M x = s that agrees with the hard decisions z on the most reliable independent
// positions, the best of the first single flips among them, and the best of all pairs among the first `pair_depth` of them.
// The shape of kernels_osd.hip — ONE WORKGROUP = ONE FRAME, the frame's whole check matrix over GF(2) in LDS, the same load,
// order, build, pivot votes and candidate search — and what is new:
//   right-hand side   every row carries the bit r = s + M z in bit 63 of its side word (tests/golden/h.txt has no spare bit in
//              its matrix words and no room for a further word per row).  The unknown is e = x + z: M e = r, and order 0 is
//              e = 0 on K.  During the elimination the side word is used as two 32-bit halves: the owner of a pivot row notes
//              the column in the LOW half, every row that takes the pivot row XORed in — pivot rows of earlier columns too —
//              takes the HIGH half along, which holds nothing but the bit.  Nobody writes the half another thread reads.
//   met        the first exit asks for M z = s (every r zero) instead of M z = 0; each thread keeps the r of its rows as a
//              mask until the matrix is built (the region holds the sort keys until then).
//   infeasible a row without a pivot is all zero after the elimination; its r set means s is outside the column space of M.
//   order 0    e0 at the pivot column of a row = the row's r: no parity over the row is needed.  The side word becomes
//              (q of the pivot column, the column in bits 32..47, r in bit 63): r is also "x0 differs from z there".
//   pairs      a wave per pair (t1, t2), the pairs dealt to the waves in lexicographic order.  Flipping K[t1] and K[t2] flips
//              the pivot of every row that holds exactly one of the two:
//                  metric = metric(x0) + q[j1] + q[j2] + the sum over the rows with (bit j1 XOR bit j2) of +q (r = 0) or -q.
//              The direct form: it is the single's loop with one more broadcast-free LDS read and an XOR per row, it needs
//              no table of single scores and no order between the single and the pair stage (pair_depth may exceed
//              candidates).  Rows are strided over the lanes: lane l reads word wj of row l, addresses 8 S l bytes apart with
//              S odd, so the 32 lanes of a half wave cover the 64 banks once — no conflict (ds_read_b64 banks by
//              (address / 4) mod 64).  The loop bounds and the pair's indices are wave-uniform: scalar registers and branches.
//              q[j1], q[j2] come from LDS (the first 256 of K, filled once), not from the typed input again.
//              Only the metric is summed per candidate; the winner's flips are counted once, while it is applied.
//   winner     first best by (metric, e), e = t for a single, min(candidates, |K|) + the pair's rank otherwise: within a wave
//              e only grows, so a strict comparison keeps the first; across waves (metric, e) is compared.
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
constexpr int kMiss = 3, kFlips0 = 4, kNoSolution = 5;
constexpr uint64_t kRhs = 1ull << 63; // side word: q in bits 0..31, the pivot column in 32..47, the right-hand side in 63
constexpr uint32_t kWaves = kOsdMaxThreads / 64;

__global__ __launch_bounds__(kOsdMaxThreads) void osd_syndrome_kernel(const OsdSyndromeArgs a)
{
    extern __shared__ uint64_t osd_syndrome_lds[];
    const uint32_t nc = a.nc, mc = a.mc, nw = static_cast<uint32_t>(osd_row_words(nc)), S = static_cast<uint32_t>(osd_stride(nc));
    uint64_t *rows = osd_syndrome_lds;
    uint32_t *key = reinterpret_cast<uint32_t *>(osd_syndrome_lds); // [nc], until the matrix is built
    uint64_t *Z = rows + osd_matrix_bytes(nc, mc) / 8, *P = Z + nw, *X = P + nw; // [nw] each
    uint64_t *sum64 = X + nw;                                                  // [0] metric(x0), [1 + wave] the wave's best metric
    uint32_t *scal = reinterpret_cast<uint32_t *>(sum64 + 1 + kWaves);         // [16]
    uint32_t *best_e = scal + 16, *best_a = best_e + kWaves, *best_b = best_a + kWaves; // 392 bytes so far
    uint32_t *qk = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(sum64) + 512);                               // [kOsdMaxPairDepth]
    uint16_t *order = reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(sum64) + kOsdSyndromeSideBytes);          // [nc]
    uint32_t *X32 = reinterpret_cast<uint32_t *>(X);
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = T >> 6;
    const uint64_t frame = blockIdx.x, at = frame * nc;

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
    // ---- met: r = s + M z of my rows tid + k T, bit k ----
    uint32_t rhs = 0;
    for (uint32_t k = 0, r = tid; r < mc; ++k, r += T)
    {
        uint32_t s = 0;
        if (a.syndrome) // (uniform)
            s = a.syndrome_format == kBitsU8 ? (static_cast<const uint8_t *>(a.syndrome)[frame * mc + r] != 0 ? 1u : 0u)
                                             : (static_cast<const uint32_t *>(a.syndrome)[frame * a.syn_words + (r >> 5)] >> (r & 31u)) & 1u;
        for (uint32_t q = a.row_ptr[r], end = a.row_ptr[r + 1]; q < end; ++q)
        {
            const uint32_t c = a.row_col[q];
            s ^= static_cast<uint32_t>(Z[c >> 6] >> (c & 63u)) & 1u;
        }
        rhs |= s << k;
    }
    if (rhs)
        atomicOr(&scal[kMiss], 1u);
    __syncthreads();
    uint32_t status = kOsdCodeword, flips = 0, column1 = kOsdNoColumn, column2 = kOsdNoColumn;
    uint64_t metric = 0;
    const uint32_t *word = reinterpret_cast<const uint32_t *>(Z);
    if (scal[kMiss]) // (uniform, as every branch on the votes, the flags and the sums below)
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
        for (uint32_t k = 0, r = tid; r < mc; ++k, r += T)
        {
            uint64_t *row = rows + static_cast<size_t>(r) * S;
            for (uint32_t w = 0; w < S; ++w)
                row[w] = 0;
            for (uint32_t q = a.row_ptr[r], end = a.row_ptr[r + 1]; q < end; ++q)
            {
                const uint32_t c = a.row_col[q];
                row[c >> 6] ^= 1ull << (c & 63u);
            }
            if ((rhs >> k) & 1u)
                row[nw] = kRhs;
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
            const uint32_t *pivot_rhs = reinterpret_cast<const uint32_t *>(pivot + nw) + 1; // (the high half: the bit alone)
            for (uint32_t k = 0, row = tid; row < mc; ++k, row += T)
            {
                uint64_t *mine = rows + static_cast<size_t>(row) * S;
                if (!((mine[wj] >> bj) & 1u))
                    continue;
                uint32_t *side = reinterpret_cast<uint32_t *>(mine + nw);
                if (row == p)
                {
                    used |= 1u << k;
                    side[0] = c; // (the low half: the others read the high half of this row, which stays)
                    continue;
                }
#pragma unroll 4
                for (uint32_t w = 0; w < nw; ++w)
                    if (const uint64_t x = pivot[w]) // (the same for every lane: a zero word costs its broadcast read only)
                        mine[w] ^= x;
                if (const uint32_t x = *pivot_rhs) // (uniform, as the zero words)
                    side[1] ^= x;
            }
        }
        __syncthreads();
        // ---- order 0: x0 = z + e0, e0 = r at the pivot columns and 0 on K ----
        const uint32_t depth = a.pair_depth < kept ? a.pair_depth : kept;
        for (uint32_t w = tid; w < nw; w += T)
            X[w] = Z[w];
        for (uint32_t t = tid; t < depth; t += T)
            qk[t] = osd_reliability(osd_widen(a, at + order[t]));
        __syncthreads();
        for (uint32_t k = 0, row = tid; row < mc; ++k, row += T)
        {
            uint64_t *mine = rows + static_cast<size_t>(row) * S;
            const bool one = (mine[nw] & kRhs) != 0;
            if (!((used >> k) & 1u))
            {
                if (one) // (the row is all zero: 0 = 1)
                    atomicOr(&scal[kNoSolution], 1u);
                continue;
            }
            const uint32_t c = static_cast<uint32_t>(mine[nw]);
            const uint32_t q = osd_reliability(osd_widen(a, at + c));
            mine[nw] = q | (static_cast<uint64_t>(c) << 32) | (one ? kRhs : 0);
            if (one)
            {
                atomicXor(&X32[c >> 5], 1u << (c & 31u));
                atomicAdd(reinterpret_cast<unsigned long long *>(&sum64[0]), static_cast<unsigned long long>(q));
                atomicAdd(&scal[kFlips0], 1u);
            }
        }
        __syncthreads();
        if (scal[kNoSolution])
            status = kOsdInfeasible;
        else
        {
            // ---- candidates: the singles, then the pairs ----
            const uint64_t metric0 = sum64[0];
            const uint32_t tried = a.candidates < kept ? a.candidates : kept;
            uint64_t bm = metric0;
            uint32_t be = kNoRow, ba = kNoRow, bb = kNoRow;
            for (uint32_t t = wave; t < tried; t += waves) // (wave-uniform)
            {
                const uint32_t j = order[t], wj = j >> 6, bj = j & 63u;
                int64_t d = 0;
                for (uint32_t row = lane; row < mc; row += 64u)
                {
                    const uint64_t *r = rows + static_cast<size_t>(row) * S;
                    if (!((r[wj] >> bj) & 1u))
                        continue;
                    const uint64_t side = r[nw];
                    const int64_t q = static_cast<int64_t>(side & 0xFFFFFFFFull);
                    d += (side & kRhs) ? -q : q;
                }
                d = osd_wave_sum(d);
                const uint64_t m = metric0 + osd_reliability(osd_widen(a, at + j)) + static_cast<uint64_t>(d);
                if (m < bm)
                    bm = m, be = t, ba = t, bb = kNoRow;
            }
            // pair (t1, t1 + 1 + pos), the wave's next in lexicographic order; e = tried + its rank
            for (uint32_t t1 = 0, pos = wave, e = tried + wave; t1 + 1u < depth;) // (wave-uniform)
            {
                const uint32_t width = depth - 1u - t1;
                if (pos >= width)
                {
                    pos -= width, ++t1;
                    continue;
                }
                const uint32_t t2 = t1 + 1u + pos;
                const uint32_t j1 = order[t1], w1 = j1 >> 6, b1 = j1 & 63u, j2 = order[t2], w2 = j2 >> 6, b2 = j2 & 63u;
                int64_t d = 0;
                for (uint32_t row = lane; row < mc; row += 64u)
                {
                    const uint64_t *r = rows + static_cast<size_t>(row) * S;
                    if (!(((r[w1] >> b1) ^ (r[w2] >> b2)) & 1u))
                        continue;
                    const uint64_t side = r[nw];
                    const int64_t q = static_cast<int64_t>(side & 0xFFFFFFFFull);
                    d += (side & kRhs) ? -q : q;
                }
                d = osd_wave_sum(d);
                const uint64_t m = metric0 + qk[t1] + qk[t2] + static_cast<uint64_t>(d);
                if (m < bm)
                    bm = m, be = e, ba = t1, bb = t2;
                pos += waves, e += waves;
            }
            if (lane == 0)
                sum64[1 + wave] = bm, best_e[wave] = be, best_a[wave] = ba, best_b[wave] = bb;
            __syncthreads();
            metric = metric0, status = kOsdOrder0;
            uint32_t we = kNoRow, wa = kNoRow, wb = kNoRow;
            for (uint32_t v = 0; v < waves; ++v)
            {
                const uint64_t m = sum64[1 + v];
                const uint32_t e = best_e[v];
                if (e != kNoRow && (m < metric || (m == metric && e < we)))
                    metric = m, we = e, wa = best_a[v], wb = best_b[v];
            }
            if (we != kNoRow)
            {
                const bool pair = wb != kNoRow;
                column1 = order[wa], column2 = pair ? order[wb] : kOsdNoColumn;
                status = pair ? kOsdReprocessedPair : kOsdReprocessed;
                const uint32_t w1 = column1 >> 6, b1 = column1 & 63u, w2 = pair ? column2 >> 6 : 0u, b2 = pair ? column2 & 63u : 0u;
                if (tid == 0)
                {
                    atomicXor(&X32[column1 >> 5], 1u << (column1 & 31u));
                    if (pair)
                        atomicXor(&X32[column2 >> 5], 1u << (column2 & 31u));
                }
                uint32_t more = 0; // the flips the winner adds to those of x0 at my rows' pivots, mod 2^32
                for (uint32_t row = tid; row < mc; row += T)
                {
                    const uint64_t *r = rows + static_cast<size_t>(row) * S;
                    uint64_t bit = r[w1] >> b1;
                    if (pair)
                        bit ^= r[w2] >> b2;
                    if (!(bit & 1u))
                        continue;
                    const uint32_t c = static_cast<uint32_t>(r[nw] >> 32) & 0xFFFFu;
                    atomicXor(&X32[c >> 5], 1u << (c & 31u));
                    more += (r[nw] & kRhs) ? 0xFFFFFFFFu : 1u;
                }
                if (more)
                    atomicAdd(&scal[kFlips0], more);
                __syncthreads();
                flips = scal[kFlips0] + (pair ? 2u : 1u);
            }
            else
                flips = scal[kFlips0];
            word = X32;
        }
    }
    if (a.word_out)
        for (uint32_t w = tid; w < a.words; w += T)
            a.word_out[frame * a.words + w] = word[w];
    if (tid == 0)
    {
        if (a.flips)
            a.flips[frame] = flips;
        if (a.metric)
            a.metric[frame] = metric;
        if (a.flipped_columns)
            a.flipped_columns[2 * frame] = column1, a.flipped_columns[2 * frame + 1] = column2;
        if (a.status)
            a.status[frame] = status;
    }
}
} // namespace

int launch_osd_syndrome(const OsdSyndromeArgs &a, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    if (!a.llr || !a.row_ptr || !a.row_col || llr_type_bytes(a.llr_type) == 0 || (a.syndrome && !bits_format_known(a.syndrome_format)) ||
        a.nc == 0 || a.nc > 0xFFFFu || a.mc == 0 || a.words != (a.nc + 31u) / 32u || a.syn_words != (a.mc + 31u) / 32u ||
        a.pair_depth > kOsdMaxPairDepth || a.threads == 0 || a.threads % 64u || a.threads > kOsdMaxThreads ||
        a.mc > static_cast<uint64_t>(kOsdRowsPerThread) * a.threads || a.lds_bytes != osd_syndrome_lds_bytes(a.nc, a.mc) ||
        a.lds_bytes > kCuLdsBytes || a.n > (1ull << 20))
        return hipErrorInvalidValue;
    return launch_with_lds(osd_syndrome_kernel, dim3(static_cast<unsigned>(a.n)), dim3(a.threads), a.lds_bytes, stream, a);
}

} // namespace ldpc_amd
