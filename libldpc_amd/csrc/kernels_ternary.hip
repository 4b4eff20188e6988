// kernels_ternary.hip — opt-in NON-PARITY TERNARY min-sum decoding (Gallager's Algorithm E; "BP_MS" with
// ldpc_hip_set_min_sum_ternary(weight); include/ldpc_amd.h states the arithmetic).  Messages in {-1, 0, +1}, the reference's
// flooding schedule, syndrome early stop and iteration count.  All of it is integer work, so every output bit follows from
// the contract and is held against a numpy mirror bit for bit (tests/ternary_ref.py).  The reference computes in binary64
// (decoder.cpp:22-76): the results are not its own.
//
// BIT-SLICED like the erasure decoder (kernels_bec.hip): one workgroup of 512 threads decodes THIRTY-TWO consecutive frames,
// bit f of every word is frame f, `valid` masks a short last group.  A message is two words, Z ("is zero") and S ("is
// negative"), S & Z = 0 throughout; a lane that visits a node updates it for all 32 frames:
//   check node, edge j     zero if another input is zero, else the product of the others: the erasure decoder's rule with
//                          E -> Z and V -> S (zeros counted up to two bitwise, the signs XORed);
//   variable node          A = w r + the sum of the inputs, kept as a bit-sliced two's complement number (one plane per
//                          bit; an input adds or subtracts one by a ripple through the planes; as many planes as the node's
//                          degree and w need, 3..7).  Five masks are read off A — [A >= 2], [A = 1], [A = 0], [A = -1],
//                          [A <= -2] — and every output sgn(A - input) is six bitwise operations on them;
//                          hard = [A < 0] | [A = 0] & ~[r = +1];
//   syndrome               the decisions sit in one word per column (H); a check node reads its neighbours' through the
//                          u16 table slot -> variable-node rank, built in the prologue from the plan's slot table;
//   early termination      per frame: a frame whose decisions pass stops counting, and its H and A words are frozen (written
//                          under the mask `act`) while the group goes on; its messages run on, nobody reads them.
// Layout in LDS (plan.hpp, ternary_lds_bytes): 64 words of votes and error counts, MZ[nnz] MS[nnz] (check-node-major slots
// as in DevPlan; the area is at least 8 nc bytes: the channel prologue stages a frame's binary64 LLRs there), RP[nc] RN[nc]
// (r = +1, r = -1), H[nc], — only where llr_out is wanted — the planes of A, `planes` x nc words, then the two u16 tables.
// The work lists of a wave sit in the lanes of a few registers (v_readlane), as in the erasure kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "device_channel.hpp"
#include "kernels.hpp"
#include "launch_lds.hpp"

namespace ldpc_amd
{

namespace
{

constexpr int kTernThreads = 512, kTernWaves = kTernThreads / 64;
constexpr int kTernFrames = kTernaryFrames;
constexpr int kTernMaxPlanes = 7; // |A| <= 56 + 7
using word_t = uint32_t;

__device__ __forceinline__ word_t wave_or(word_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v |= static_cast<word_t>(__shfl_xor(static_cast<int>(v), o, 64));
    return v;
}

// bit f of the result = bit_of_frame(f) for the group's frames, 0 beyond them (kernels_bec.hip)
template <class F>
__device__ __forceinline__ word_t slice(int nf, word_t valid, F bit_of_frame)
{
    word_t w = 0;
#pragma unroll 8
    for (int f = 0; f < kTernFrames; ++f)
        w |= static_cast<word_t>(bit_of_frame(f < nf ? f : nf - 1) ? 1 : 0) << f;
    return w & valid;
}

// One variable node for 32 frames with NP planes of A (NP >= 3, |w| + degree < 2^(NP-1)).  idx: the node's slots, `count`
// apart.  Returns the decisions; A[k] = plane k of A, sign-extended to kTernMaxPlanes.
template <int NP>
__device__ __forceinline__ word_t tern_vn(word_t *MZ, word_t *MS, const uint16_t *idx, int count, int degree, word_t rp, word_t rn,
                                          uint32_t w, word_t (&A)[kTernMaxPlanes])
{
    word_t d[NP];
    const uint32_t nw = 0u - w;
#pragma unroll
    for (int k = 0; k < NP; ++k)
        d[k] = ((w >> k) & 1u ? rp : 0u) | ((nw >> k) & 1u ? rn : 0u);
    for (int p = 0; p < degree; ++p)
    {
        const uint32_t s = idx[p * count];
        const word_t n = MS[s];
        word_t m = ~MZ[s]; // the frames whose input is not zero: +1 where ~n, -1 where n
#pragma unroll
        for (int k = 0; k < NP; ++k)
        {
            const word_t old = d[k];
            d[k] = old ^ m;
            m &= old ^ n; // the carry of an increment goes on where the bit was 1, the borrow of a decrement where it was 0
        }
    }
    const word_t neg = d[NP - 1];
    word_t hi = d[1], all = d[0] & d[1];
#pragma unroll
    for (int k = 2; k < NP - 1; ++k)
        hi |= d[k], all &= d[k];
    const word_t small = ~neg & ~hi;
    const word_t G2 = ~neg & hi, E1 = small & d[0], E0 = small & ~d[0], Em1 = neg & all, L2 = neg & ~all;
    for (int p = 0; p < degree; ++p)
    {
        const uint32_t s = idx[p * count];
        const word_t z = MZ[s], n = MS[s];
        const word_t pin = ~z & ~n;
        const word_t pos = G2 | (E1 & ~pin) | (E0 & n);
        const word_t ng = L2 | (Em1 & ~n) | (E0 & pin);
        MZ[s] = ~(pos | ng), MS[s] = ng;
    }
#pragma unroll
    for (int k = 0; k < kTernMaxPlanes; ++k)
        A[k] = k < NP ? d[k < NP ? k : 0] : neg;
    return L2 | Em1 | (E0 & ~rp);
}

// LLR: the instantiation that keeps the planes of A for llr_out
template <bool LLR>
__global__ __launch_bounds__(kTernThreads) void decode_ternary_kernel(const DecodeArgs a, const TernaryArgs t)
{
    extern __shared__ double lds_d[];
    const DevPlan &P = a.plan;
    const int nnz = P.nnz, nc = P.nc, nct = P.nct;
    const int planes = t.planes;
    word_t *ldsw = reinterpret_cast<word_t *>(lds_d);
    word_t *still = ldsw;                                   // [2]
    uint32_t *errs = ldsw + 2;                              // [32]
    double *stage = lds_d + kTernaryHeadWords / 2;          // a frame's LLRs, over the message area
    word_t *MZ = ldsw + kTernaryHeadWords, *MS = MZ + nnz;
    word_t *RP = MZ + ternary_message_words(nnz, nc), *RN = RP + nc, *H = RN + nc;
    word_t *AP = H + nc; // [planes][nc], LLR only
    uint16_t *slot = reinterpret_cast<uint16_t *>(AP + (LLR ? static_cast<size_t>(planes) * nc : 0));
    uint16_t *crank = slot + nnz;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t f0 = static_cast<uint64_t>(blockIdx.x) * kTernFrames;
    const int nf = static_cast<int>(std::min<uint64_t>(kTernFrames, a.n_frames - f0)); // frames of this group
    const word_t valid = nf == kTernFrames ? ~word_t(0) : ((word_t(1) << nf) - 1);
    const uint8_t *cw = a.codeword ? a.codeword + f0 * nc : nullptr;

    if (tid < 2)
        still[tid] = 0;
    if (tid < kTernFrames)
        errs[tid] = 0;
    for (int e = tid; e < nnz; e += kTernThreads)
        slot[e] = static_cast<uint16_t>(P.vn_slot[e]);
    for (int r = tid; r < nc; r += kTernThreads)
    {
        RP[r] = 0, RN[r] = 0, H[r] = 0;
        if constexpr (LLR)
            for (int k = 0; k < planes; ++k)
                AP[static_cast<size_t>(k) * nc + r] = 0;
    }
    __syncthreads();

    // ---- channel: r = the sign of the frame's decoder input ----
    const bool bsc = a.mode == kModeBsc || a.mode == kModeBscCtr;
    if (bsc && !a.llr_in_dump)
    {
        // the BSC's LLRs are +-delta: the signs straight from the draws, a word of 32 frames at a time (the erasure
        // kernel's route; same values as channel_init: delta * (1 - 2 y), shortened columns delta, the others 0)
        const word_t dpos = a.delta > 0.0 ? valid : 0, dneg = a.delta < 0.0 ? valid : 0;
        const word_t spos = a.shorten_llr > 0.0 ? valid : 0, sneg = a.shorten_llr < 0.0 ? valid : 0;
        for (int r = tid; r < nc; r += kTernThreads)
            if (P.rank_kind[r] == 2)
                RP[r] = spos, RN[r] = sneg;
        auto put = [&](int i, word_t flip) {
            word_t y = flip;
            if (cw)
            {
                const uint8_t *c = cw + P.bit_pos[i];
                y ^= slice(nf, valid, [&](int f) { return c[static_cast<size_t>(f) * nc] != 0; });
            }
            const uint32_t r = P.tx_rank[i];
            RP[r] = (dpos & ~y) | (dneg & y), RN[r] = (dneg & ~y) | (dpos & y);
        };
        if (a.mode == kModeBscCtr)
        {
            for (int b = tid; 4 * b < nct; b += kTernThreads)
            {
                word_t fl[4] = {0, 0, 0, 0};
                for (int f = 0; f < nf; ++f)
                {
                    const uint4 w = philox_block(a.ctr_key[0], a.ctr_key[1], a.ctr_frame0 + f0 + f, static_cast<uint32_t>(b), kTagDraw);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        fl[k] |= static_cast<word_t>(counter_hit(word_of(w, k), a.eps) ? 1 : 0) << f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * b + k < nct)
                        put(4 * b + k, fl[k]);
            }
        }
        else
        {
            const uint64_t *raw = a.raw + f0 * static_cast<uint64_t>(nct);
            const double eps = a.eps;
            for (int i = tid; i < nct; i += kTernThreads)
                put(i, slice(nf, valid, [&](int f) { return canonical(raw[static_cast<size_t>(f) * nct + i]) < eps; }));
        }
        __syncthreads();
    }
    else
    {
        // every other source (given LLRs, AWGN, a dump of llr_in wanted): the binary64 channel as everywhere, frame by frame
        // into the staging area, and the signs taken into bit f
        for (int f = 0; f < nf; ++f)
        {
            channel_init<kTernThreads, kNoiseAny>(a, f0 + f, stage, tid);
            __syncthreads();
            double *o = a.llr_in_dump ? a.llr_in_dump + (f0 + f) * nc : nullptr;
            for (int r = tid; r < nc; r += kTernThreads)
            {
                const double x = stage[r];
                if (o)
                    o[P.rank_col[r]] = x; // (llr_in stays the binary64 value)
                RP[r] |= static_cast<word_t>(x > 0.0 ? 1 : 0) << f; // (+-0 and NaN: neither)
                RN[r] |= static_cast<word_t>(x < 0.0 ? 1 : 0) << f;
            }
            __syncthreads();
        }
    }
    // ---- v2c = r, and the table slot -> rank ----
    for (int b = wave; b < P.n_vn_blocks; b += kTernWaves)
    {
        const auto d = uniform_table(reinterpret_cast<const uint32_t *>(P.vn_blocks + b));
        const uint32_t idx_off = d[0], first = d[1], cd = d[2];
        const int count = static_cast<int>(cd & 0xFFFFu), degree = static_cast<int>(cd >> 16);
        if (lane < count)
        {
            const word_t rp = RP[first + lane], rn = RN[first + lane];
            for (int p = 0; p < degree; ++p)
            {
                const uint32_t s = slot[idx_off + lane + p * count];
                MZ[s] = ~(rp | rn), MS[s] = rn;
                crank[s] = static_cast<uint16_t>(first + lane);
            }
        }
    }
    __syncthreads();

    // the wave's work in the lanes of a few registers (lane k: its k-th item), read back as scalars in the passes
    uint32_t c_off = 0, c_cd = 0, v_off = 0, v_first = 0, v_cd = 0;
    int n_cn = 0, n_vn = 0;
    for (int b = wave; b < P.n_cn_blocks; b += kTernWaves, ++n_cn)
    {
        const auto d = uniform_table(reinterpret_cast<const uint32_t *>(P.cn_blocks + b));
        if (lane == n_cn)
            c_off = d[0], c_cd = d[1];
    }
    for (int b = wave; b < P.n_vn_blocks; b += kTernWaves, ++n_vn)
    {
        const auto d = uniform_table(reinterpret_cast<const uint32_t *>(P.vn_blocks + b));
        if (lane == n_vn)
            v_off = d[0], v_first = d[1], v_cd = d[2];
    }
    const uint32_t w = static_cast<uint32_t>(t.weight);
    word_t act = a.iterations > 0 ? valid : 0; // frames still decoding (uniform)
    uint32_t my_iters = 0;                      // thread f < 32: iteration count of frame f
    for (uint32_t I = 0; I < a.iterations && act; ++I)
    {
        // ---- check nodes ----
        for (int k = 0; k < n_cn; ++k)
        {
            const uint32_t off = __builtin_amdgcn_readlane(c_off, k), cd = __builtin_amdgcn_readlane(c_cd, k);
            const int count = static_cast<int>(cd & 0xFFFFu), degree = static_cast<int>(cd >> 16);
            if (lane < count)
            {
                word_t *mz = MZ + off + lane, *ms = MS + off + lane;
                // up to eight inputs stay in registers between the two sweeps (wave-uniform degree: the guards are scalar)
                auto small = [&]<int D>(std::integral_constant<int, D>) {
                    word_t z[D], s[D], c0 = 0, c1 = 0, xa = 0;
#pragma unroll
                    for (int j = 0; j < D; ++j)
                        z[j] = mz[j * count], s[j] = ms[j * count];
#pragma unroll
                    for (int j = 0; j < D; ++j)
                    {
                        c1 |= c0 & z[j];
                        c0 |= z[j];
                        xa ^= s[j];
                    }
#pragma unroll
                    for (int j = 0; j < D; ++j)
                    {
                        const word_t alone = ~c1 & (~c0 | z[j]); // no OTHER input is zero
                        mz[j * count] = ~alone;
                        ms[j * count] = (xa ^ s[j]) & alone;
                    }
                };
                switch (degree)
                {
                case 2: small(std::integral_constant<int, 2>{}); break;
                case 3: small(std::integral_constant<int, 3>{}); break;
                case 4: small(std::integral_constant<int, 4>{}); break;
                case 5: small(std::integral_constant<int, 5>{}); break;
                case 6: small(std::integral_constant<int, 6>{}); break;
                case 7: small(std::integral_constant<int, 7>{}); break;
                case 8: small(std::integral_constant<int, 8>{}); break;
                default:
                {
                    word_t c0 = 0, c1 = 0, xa = 0;
                    for (int j = 0; j < degree; ++j)
                    {
                        const word_t z = mz[j * count];
                        c1 |= c0 & z;
                        c0 |= z;
                        xa ^= ms[j * count];
                    }
                    for (int j = 0; j < degree; ++j)
                    {
                        const word_t z = mz[j * count], s = ms[j * count];
                        const word_t alone = ~c1 & (~c0 | z);
                        mz[j * count] = ~alone;
                        ms[j * count] = (xa ^ s) & alone;
                    }
                }
                }
            }
        }
        __syncthreads();
        // ---- variable nodes ----
        for (int k = 0; k < n_vn; ++k)
        {
            const uint32_t idx_off = __builtin_amdgcn_readlane(v_off, k), first = __builtin_amdgcn_readlane(v_first, k),
                           cd = __builtin_amdgcn_readlane(v_cd, k);
            const int count = static_cast<int>(cd & 0xFFFFu), degree = static_cast<int>(cd >> 16);
            // planes of A for this block: |A| <= degree + w < 2^(np - 1)
            const int np = std::max(3, 33 - __builtin_clz(static_cast<uint32_t>(degree) + w));
            if (lane < count)
            {
                const int r = static_cast<int>(first) + lane;
                const word_t rp = RP[r], rn = RN[r];
                const uint16_t *idx = slot + idx_off + lane;
                word_t A[kTernMaxPlanes], hard;
                switch (np)
                {
                case 3: hard = tern_vn<3>(MZ, MS, idx, count, degree, rp, rn, w, A); break;
                case 4: hard = tern_vn<4>(MZ, MS, idx, count, degree, rp, rn, w, A); break;
                case 5: hard = tern_vn<5>(MZ, MS, idx, count, degree, rp, rn, w, A); break;
                case 6: hard = tern_vn<6>(MZ, MS, idx, count, degree, rp, rn, w, A); break;
                default: hard = tern_vn<7>(MZ, MS, idx, count, degree, rp, rn, w, A); break;
                }
                H[r] = (H[r] & ~act) | (hard & act); // frames that have finished keep their outputs
                if constexpr (LLR)
                {
#pragma unroll
                    for (int q = 0; q < kTernMaxPlanes; ++q)
                        if (q < planes)
                        {
                            word_t *ap = AP + static_cast<size_t>(q) * nc + r;
                            *ap = (*ap & ~act) | (A[q] & act);
                        }
                }
            }
        }
        __syncthreads();
        word_t on = act;
        if (a.early_term)
        {
            // ---- syndrome of the decisions: the frames with an unsatisfied check node go on ----
            word_t bad = 0;
            for (int k = 0; k < n_cn; ++k)
            {
                const uint32_t off = __builtin_amdgcn_readlane(c_off, k), cd = __builtin_amdgcn_readlane(c_cd, k);
                const int count = static_cast<int>(cd & 0xFFFFu), degree = static_cast<int>(cd >> 16);
                if (lane < count)
                {
                    const uint16_t *cr = crank + off + lane;
                    word_t x = 0;
                    for (int j = 0; j < degree; ++j)
                        x ^= H[cr[j * count]];
                    bad |= x;
                }
            }
            bad = wave_or(bad);
            if (lane == 0 && bad)
                atomicOr(&still[I & 1], bad);
            __syncthreads();
            on = act & still[I & 1]; // (the same word for every thread: the vote is uniform)
            if (tid == 0)
                still[(I + 1) & 1] = 0; // (next written after the next iteration's second barrier)
        }
        if (tid < kTernFrames)
            my_iters += static_cast<uint32_t>((on >> tid) & 1);
        act = on;
    }
    __syncthreads();

    if (tid < nf && a.iters)
        a.iters[f0 + tid] = my_iters;
    // (no iteration ran: H and the planes of A still hold their initial zeros)
    if (a.hard)
    {
        uint8_t *h = a.hard + f0 * nc;
        for (int r = tid; r < nc; r += kTernThreads)
        {
            const word_t hb = H[r];
            uint8_t *d = h + P.rank_col[r];
            for (int f = 0; f < nf; ++f)
                d[static_cast<size_t>(f) * nc] = static_cast<uint8_t>((hb >> f) & 1);
        }
    }
    if constexpr (LLR)
    {
        double *o = a.llr_out + f0 * nc;
        for (int r = tid; r < nc; r += kTernThreads)
        {
            word_t pl[kTernMaxPlanes]; // sign-extended: the planes beyond the last repeat it
#pragma unroll
            for (int q = 0; q < kTernMaxPlanes; ++q)
                pl[q] = AP[static_cast<size_t>(q < planes ? q : planes - 1) * nc + r];
            double *d = o + P.rank_col[r];
            for (int f = 0; f < nf; ++f)
            {
                int v = 0;
#pragma unroll
                for (int q = 0; q < kTernMaxPlanes - 1; ++q)
                    v |= static_cast<int>((pl[q] >> f) & 1u) << q;
                v -= static_cast<int>((pl[kTernMaxPlanes - 1] >> f) & 1u) << (kTernMaxPlanes - 1);
                d[static_cast<size_t>(f) * nc] = static_cast<double>(v);
            }
        }
    }
    if (a.bit_errors)
    {
        // the words of the transmitted positions (decision xor transmitted bit) go to the message array, which has served;
        // then the threads count them frame by frame
        word_t *ew = MZ;
        for (int i = tid; i < P.n_bitpos; i += kTernThreads)
        {
            word_t x = 0;
            if (cw)
            {
                const uint8_t *c = cw + P.bit_pos[i];
                x = slice(nf, valid, [&](int f) { return c[static_cast<size_t>(f) * nc] != 0; });
            }
            ew[i] = (H[P.tx_rank[i]] ^ x) & valid;
        }
        __syncthreads();
        // thread (part, f): frame f over every 16th position
        uint32_t n = 0;
        const int fr = tid & (kTernFrames - 1), part = tid / kTernFrames, parts = kTernThreads / kTernFrames;
        for (int i = part; i < P.n_bitpos; i += parts)
            n += static_cast<uint32_t>((ew[i] >> fr) & 1);
        if (n)
            atomicAdd(&errs[fr], n);
        __syncthreads();
        if (tid < nf)
            a.bit_errors[f0 + tid] = errs[tid];
    }
}

} // namespace

int launch_decode_ternary(const DecodeArgs &a, const TernaryArgs &t, void *stream)
{
    static_assert(sizeof(CnBlock) == 8 && sizeof(VnBlock) == 12, "block descriptors are read as 2 / 3 scalar words");
    static_assert(kTernaryMaxVnDegree + 7 < (1 << (kTernMaxPlanes - 1)), "A fits its planes");
    if (a.n_frames == 0)
        return hipSuccess;
    const DevPlan &p = a.plan;
    const bool llr = a.llr_out != nullptr;
    // (a wave's work list lives in the 64 lanes of a register: blocks / 8 <= 64; the error count's words reuse the messages)
    if (p.nc <= 0 || p.nc > 0xFFFF || p.nnz <= 0 || p.nnz > 0xFFFF || p.n_cn_blocks > 64 * kTernWaves || p.n_vn_blocks > 64 * kTernWaves ||
        static_cast<size_t>(p.n_bitpos) > ternary_message_words(p.nnz, p.nc) || t.weight < 1 || t.weight > 7 || t.planes < 3 ||
        t.planes > kTernMaxPlanes || !p.cn_blocks || !p.vn_blocks || !p.vn_slot ||
        ternary_lds_bytes(p.nnz, p.nc, t.planes, true) > kCuLdsBytes)
        return hipErrorInvalidValue;
    const uint64_t groups = (a.n_frames + kTernFrames - 1) / kTernFrames;
    if (groups > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    void (*k)(const DecodeArgs, const TernaryArgs) = llr ? decode_ternary_kernel<true> : decode_ternary_kernel<false>;
    return launch_with_lds(k, dim3(static_cast<unsigned>(groups)), dim3(kTernThreads),
                           static_cast<uint32_t>(ternary_lds_bytes(p.nnz, p.nc, t.planes, llr)), stream, a, t);
}

} // namespace ldpc_amd
