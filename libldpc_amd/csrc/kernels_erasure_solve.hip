// kernels_erasure_solve.hip — maximum-likelihood erasure decoding of the batch interface (include/ldpc_amd.h,
// ldpc_hip_erasure_solve_batch): every erased bit that the parity checks determine, where peeling (kernels_erasure.hip) stops
// at the first stopping set.  ONE WORKGROUP = ONE FRAME; the frame's linear system over GF(2) lives in LDS from the first
// word to the last.
//   load       E and V = word & ~E (the padding bits cleared); wave 0 counts the unknowns in front of every word of E, so
//              that the unknown index of an erased column c is pre[c / 32] + popcount(E[c / 32] below c).  A frame over the cap
//              leaves here, as it came.
//   rows       one thread per check node walks its list in H: does it list an erased column (a ballot per 64 check nodes
//              keeps the mask), and the XOR of its known columns.  A check node without an erased column and with XOR 1 makes
//              the frame inconsistent.  A frame without erasures leaves here: status 0 iff its syndrome is zero.
//   build      the check nodes that list an erased column get consecutive rows (count of the mask in front of them); a thread
//              clears its row, toggles one bit per listed erased column — an entry listed twice cancels — and sets the
//              right-hand side.  Row stride: kernels.hpp.
//   eliminate  Gauss-Jordan.  Thread t owns the rows t, t + T, ...; only the pivot row is ever read by others.  Per unknown j:
//              every thread offers its first unused row with bit j, the first of the wave by ballots, across waves by one
//              LDS atomicMin per wave; ONE barrier; the owner marks the pivot row used, every other row with bit j takes the
//              pivot row XORed in (a broadcast read, an 8-byte read and an 8-byte write per word).  The vote has three slots
//              in turn, so that clearing the next but one needs no second barrier.  The pivot row is not written in the
//              step that reads it, and its owner's next write to it comes after the next barrier.
//   results    after the last column an unused row has no unknown left: it is inconsistent if its right-hand side is 1.  A
//              row with exactly one unknown determines it (whatever order the pivots came in: the unit vector of a column
//              lies in the row space iff the reduced form holds it as a row).  Determined columns leave E and take their
//              value by LDS atomics on the two packed rows, which are then stored as they stand.
// Results go out by ordinary vector stores; nothing here depends on timing: minima, ORs and counts only.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "launch_lds.hpp"
#include "plan.hpp"

namespace ldpc_amd
{

namespace
{
constexpr uint32_t kNoRow = 0xFFFFFFFFu;
// the scalars: [0..2] the pivot votes, then
constexpr int kSolveBad = 3, kSolveRows = 4, kSolveDetermined = 5;

// dst[i] = count(0) + ... + count(i - 1) for i < items, by one wave (every lane calls it); returns the sum of all
template <typename Count>
__device__ __forceinline__ uint32_t solve_wave_prefix(uint32_t items, uint32_t lane, uint32_t *dst, Count count)
{
    uint32_t carry = 0;
    for (uint32_t base = 0; base < items; base += 64) // (uniform)
    {
        const uint32_t i = base + lane;
        const uint32_t x = i < items ? count(i) : 0;
        uint32_t sum = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1)
        {
            const uint32_t below = static_cast<uint32_t>(__shfl_up(static_cast<int>(sum), o, 64));
            sum += lane >= static_cast<uint32_t>(o) ? below : 0;
        }
        if (i < items)
            dst[i] = carry + sum - x;
        carry += static_cast<uint32_t>(__shfl(static_cast<int>(sum), 63, 64));
    }
    return carry;
}

__global__ __launch_bounds__(kErasureSolveMaxThreads) void erasure_solve_kernel(const ErasureSolveArgs a)
{
    extern __shared__ uint64_t solve_lds[];
    const uint32_t W = a.words, mc = a.mc, groups = (mc + 63) / 64;
    uint64_t *rows = solve_lds, *rowmask = rows + static_cast<size_t>(a.rows) * erasure_solve_stride(a.cap); // [groups]
    uint32_t *rowpre = reinterpret_cast<uint32_t *>(rowmask + groups);                                       // [groups]
    uint32_t *E = rowpre + groups, *V = E + W, *pre = V + W, *scal = pre + W + 1, *ucol = scal + kErasureSolveScalars; // ucol[cap]
    const uint32_t tid = threadIdx.x, T = blockDim.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6), waves = T >> 6;
    const uint64_t at = static_cast<uint64_t>(blockIdx.x) * W;

    // ---- load ----
    for (uint32_t w = tid; w < W; w += T)
    {
        const uint32_t live = (w == W - 1 && (a.nc & 31u)) ? (1u << (a.nc & 31u)) - 1u : ~0u;
        const uint32_t e = a.erased[at + w] & live;
        E[w] = e, V[w] = a.word[at + w] & live & ~e;
    }
    if (tid < kErasureSolveScalars)
        scal[tid] = tid < 3 ? kNoRow : 0;
    __syncthreads();
    if (wave == 0)
    {
        const uint32_t total = solve_wave_prefix(W, lane, pre, [&](uint32_t i) { return static_cast<uint32_t>(__popc(E[i])); });
        if (lane == 0)
            pre[W] = total;
    }
    __syncthreads();
    const uint32_t nE = pre[W];
    uint32_t status = kErasureTooLarge, rank = 0, determined = 0;
    if (nE <= a.cap) // (uniform, as every branch on nE, rank and the votes below)
    {
        // ---- rows: which check nodes list an erased column; the syndrome of those that list none ----
        bool bad = false;
        for (uint32_t g = wave; g < groups; g += waves)
        {
            const uint32_t r = 64u * g + lane;
            uint32_t listed = 0, rhs = 0;
            if (r < mc)
                for (uint32_t q = a.row_ptr[r], end = a.row_ptr[r + 1]; q < end; ++q)
                {
                    const uint32_t c = a.row_col[q], bit = 1u << (c & 31u);
                    listed |= E[c >> 5] & bit;
                    rhs ^= (V[c >> 5] & bit) != 0 ? 1u : 0u;
                }
            const uint64_t m = __ballot(listed != 0);
            if (lane == 0)
                rowmask[g] = m;
            bad = bad || (listed == 0 && rhs != 0);
        }
        if (bad)
            atomicOr(&scal[kSolveBad], 1u);
        __syncthreads();
        if (nE > 0)
        {
            // ---- number the rows and the unknowns ----
            if (wave == 0)
            {
                const uint32_t total = solve_wave_prefix(groups, lane, rowpre, [&](uint32_t i) { return static_cast<uint32_t>(__popcll(rowmask[i])); });
                if (lane == 0)
                    scal[kSolveRows] = total;
            }
            for (uint32_t w = tid; w < W; w += T)
            {
                uint32_t j = pre[w];
                for (uint32_t e = E[w]; e; e &= e - 1)
                    ucol[j++] = 32u * w + static_cast<uint32_t>(__ffs(static_cast<int>(e)) - 1);
            }
            __syncthreads();
            const uint32_t used_rows = scal[kSolveRows]; // <= a.rows: each of at most cap erased columns is listed by at most d check nodes
            const uint32_t s = static_cast<uint32_t>(erasure_solve_stride(nE)); // <= the stride of the cap
            // ---- build ----
            for (uint32_t g = wave; g < groups; g += waves)
            {
                const uint64_t m = rowmask[g];
                if (!((m >> lane) & 1u))
                    continue;
                const uint32_t r = 64u * g + lane;
                uint64_t *row = rows + static_cast<size_t>(rowpre[g] + static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)))) * s;
                for (uint32_t w = 0; w < s; ++w)
                    row[w] = 0;
                uint32_t rhs = 0;
                for (uint32_t q = a.row_ptr[r], end = a.row_ptr[r + 1]; q < end; ++q)
                {
                    const uint32_t c = a.row_col[q], bit = 1u << (c & 31u), e = E[c >> 5];
                    if (e & bit)
                    {
                        const uint32_t j = pre[c >> 5] + static_cast<uint32_t>(__popc(e & (bit - 1u)));
                        row[j >> 6] ^= 1ull << (j & 63u);
                    }
                    else
                        rhs ^= (V[c >> 5] & bit) != 0 ? 1u : 0u;
                }
                row[nE >> 6] ^= static_cast<uint64_t>(rhs) << (nE & 63u);
            }
            __syncthreads();
            // ---- eliminate ----
            uint32_t used = 0; // bit k: my row tid + k T is a pivot row
            const uint32_t rows_per_thread = (used_rows + T - 1u) / T;
            for (uint32_t j = 0; j < nE; ++j)
            {
                const uint32_t wj = j >> 6, bj = j & 63u;
                // the wave's first unused row with bit j: rows grow with k and, inside one k, with the lane — a ballot per k
                uint32_t best = kNoRow;
                for (uint32_t k = 0, row = tid; k < rows_per_thread; ++k, row += T) // (uniform: every lane ballots)
                {
                    const bool offer = row < used_rows && !((used >> k) & 1u) && ((rows[static_cast<size_t>(row) * s + wj] >> bj) & 1u);
                    if (const uint64_t m = __ballot(offer))
                    {
                        best = row - lane + static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
                        break;
                    }
                }
                if (lane == 0 && best != kNoRow)
                    atomicMin(&scal[j % 3u], best);
                __syncthreads();
                const uint32_t p = scal[j % 3u];
                if (tid == 0)
                    scal[(j + 2u) % 3u] = kNoRow; // (read last before this barrier, voted on next after the next one)
                if (p == kNoRow)
                    continue;
                ++rank;
                const uint64_t *pivot = rows + static_cast<size_t>(p) * s;
                for (uint32_t k = 0, row = tid; row < used_rows; ++k, row += T)
                {
                    uint64_t *mine_row = rows + static_cast<size_t>(row) * s;
                    if (!((mine_row[wj] >> bj) & 1u))
                        continue;
                    if (row == p)
                    {
                        used |= 1u << k;
                        continue;
                    }
#pragma unroll 4
                    for (uint32_t w = 0; w < s; ++w)
                        if (const uint64_t x = pivot[w]) // (the same for every lane: a zero word costs its broadcast read only)
                            mine_row[w] ^= x;
                }
            }
            // ---- results: every thread reads its own rows only ----
            const auto summary = [&](uint32_t row, uint32_t &unknown, uint32_t &rhs) {
                const uint64_t *r = rows + static_cast<size_t>(row) * s;
                uint32_t count = 0;
                for (uint32_t w = 0; 64u * w < nE; ++w)
                {
                    const uint64_t x = nE - 64u * w >= 64u ? r[w] : r[w] & ((1ull << (nE - 64u * w)) - 1ull);
                    if (x)
                        unknown = 64u * w + static_cast<uint32_t>(__ffsll(static_cast<long long>(x)) - 1);
                    count += static_cast<uint32_t>(__popcll(x));
                }
                rhs = static_cast<uint32_t>((r[nE >> 6] >> (nE & 63u)) & 1u);
                return count;
            };
            bad = false;
            for (uint32_t row = tid; row < used_rows; row += T)
            {
                uint32_t unknown = 0, rhs = 0;
                bad = bad || (summary(row, unknown, rhs) == 0 && rhs != 0);
            }
            if (bad)
                atomicOr(&scal[kSolveBad], 1u);
            __syncthreads();
            if (!scal[kSolveBad])
            {
                uint32_t found = 0;
                for (uint32_t row = tid; row < used_rows; row += T)
                {
                    uint32_t unknown = 0, rhs = 0;
                    if (summary(row, unknown, rhs) != 1)
                        continue;
                    const uint32_t c = ucol[unknown], bit = 1u << (c & 31u);
                    atomicAnd(&E[c >> 5], ~bit);
                    if (rhs)
                        atomicOr(&V[c >> 5], bit);
                    ++found;
                }
                if (found)
                    atomicAdd(&scal[kSolveDetermined], found);
            }
            __syncthreads();
            determined = scal[kSolveDetermined];
        }
        status = scal[kSolveBad] ? kErasureInconsistent : determined == nE ? kErasureSolved : kErasurePartial;
    }
    for (uint32_t w = tid; w < W; w += T)
    {
        if (a.erased_out)
            a.erased_out[at + w] = E[w];
        if (a.word_out)
            a.word_out[at + w] = V[w];
    }
    if (tid == 0)
    {
        if (a.unresolved)
            a.unresolved[blockIdx.x] = nE - determined;
        if (a.rank)
            a.rank[blockIdx.x] = rank;
        if (a.status)
            a.status[blockIdx.x] = status;
    }
}
} // namespace

int launch_erasure_solve(const ErasureSolveArgs &a, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    if (!a.word || !a.erased || !a.row_ptr || !a.row_col || a.nc == 0 || a.words != (a.nc + 31u) / 32u || a.cap == 0 || a.cap > a.nc ||
        a.rows > a.mc || a.threads == 0 || a.threads % 64u || a.threads > kErasureSolveMaxThreads ||
        a.rows > static_cast<uint64_t>(kErasureSolveRowsPerThread) * a.threads || a.lds_bytes != erasure_solve_lds_bytes(a.nc, a.mc, a.cap, a.rows) ||
        a.lds_bytes > kCuLdsBytes || a.n >= (1ull << 31))
        return hipErrorInvalidValue;
    return launch_with_lds(erasure_solve_kernel, dim3(static_cast<unsigned>(a.n)), dim3(a.threads), a.lds_bytes, stream, a);
}

} // namespace ldpc_amd
