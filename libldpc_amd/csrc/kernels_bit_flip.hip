// kernels_bit_flip.hip — gradient-descent bit flipping of the batch interface TOWARD A GIVEN SYNDROME (include/ldpc_amd.h,
// ldpc_hip_bit_flip_batch states the arithmetic): GDBF with soft reliabilities and multi-bit flipping, and PGDBF on the
// counter generator (device_philox.hpp, tag 3).  Everything after the one quantization of the input is integer arithmetic:
// every output bit follows from the contract and is held against a numpy mirror (tests/bit_flip_ref.py).
//
// ONE WAVE = ONE FRAME, up to kBitFlipMaxFrames frames to a workgroup (kernels.hpp, bit_flip_group_frames), and no workgroup
// barrier anywhere: a wave whose frame lies beyond the batch leaves at once, the others never wait for it.  What LDS holds
// per frame (kernels.hpp, bit_flip_lds_bytes; every part starts on 16 bytes): the nc quantized inputs, a byte each (sign = y,
// magnitude = r); the word x, a bit per column; the unmet checks u, a bit per check node, twice — U, what the round reads,
// and V, what its flips leave for the next round.
//   prologue   the frame's elements read in place in their own type, column order (coalesced), quantized to the byte; the
//              word x = y by a ballot per 64 columns; then a lane per check node: s[c] XOR the row's bits of x, a ballot per
//              64 check nodes, written to V.  This is the only walk of the row -> columns table.
//   round      V is copied to U with a popcount on the way (the stop test is a ballot over "this lane saw a set bit", the
//              weight the sum of the counts).  Walk 1, a lane per column through the column -> rows table: P from the bits of
//              U, the lane's maximum, then the wave's by six exchanges.  Walk 2, only in the lanes whose own maximum reaches
//              Pmax - margin: P again, and a candidate flips its bit of x and the bits of its check nodes in V (LDS
//              atomics: several lanes meet in a word; an entry listed twice toggles twice).  u is never formed from x again.
//   epilogue   the words of x are the packed decisions.
// P is formed twice instead of being kept: a 32-bit P per column would be three quarters of a frame's LDS, and the LDS a
// frame takes decides how many waves a CU holds.
#include "device_philox.hpp"
#include "launch_lds.hpp"

namespace ldpc_amd
{

namespace
{
constexpr int kBfNone = -(1 << 30); // below every penalty (|P| <= 255 * the entries of a column + 127)

// clamp(rint(fl(w * inv)), -qmax, +qmax), the clamp in binary64; a NaN gives 0 (kernels_syndrome_decode.hip, sd_quantize:
// the same quantizer)
__device__ __forceinline__ int bf_quantize(double w, double inv, int qmax)
{
#pragma clang fp contract(off)
    const double x = __builtin_rint(w * inv);
    const double q = static_cast<double>(qmax);
    return x >= q ? qmax : (x <= -q ? -qmax : (x == x ? static_cast<int>(x) : 0));
}

// the LDS operations of one wave execute in order; this keeps the compiler from moving them across
__device__ __forceinline__ void bf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t bf_bit(const uint32_t *words, uint32_t i) { return (words[i >> 5] >> (i & 31u)) & 1u; }

// a row of elements, column order, quantized to the bytes Q; x = (Q <= 0) packed by a ballot per 64 columns
template <class E>
__device__ __forceinline__ void bf_prologue(const BitFlipArgs &a, const E *src, int lane, int8_t *Q, uint32_t *X)
{
    const int nc = static_cast<int>(a.nc);
    for (int base = 0; base < nc; base += 64)
    {
        const int c = base + lane;
        bool one = false;
        if (c < nc)
        {
            int q;
            if constexpr (sizeof(E) == 1)
            {
                const int k = src[c];
                q = k > a.qmax ? a.qmax : (k < -a.qmax ? -a.qmax : k);
            }
            else
                q = bf_quantize(static_cast<double>(src[c]), a.inv, a.qmax);
            Q[c] = static_cast<int8_t>(q);
            one = q <= 0;
        }
        const uint64_t m = __ballot(one);
        if (lane == 0)
        {
            const uint32_t w = static_cast<uint32_t>(base) >> 5;
            X[w] = static_cast<uint32_t>(m);
            if (w + 1 < a.words)
                X[w + 1] = static_cast<uint32_t>(m >> 32);
        }
    }
}

// P[c] = w U[c] + (x[c] != y[c] ? +r[c] : -r[c])
__device__ __forceinline__ int bf_penalty(const BitFlipArgs &a, uint32_t c, const int8_t *Q, const uint32_t *X, const uint32_t *U)
{
    const uint32_t b = a.col_ptr[c], e = a.col_ptr[c + 1];
    int unmet = 0;
    for (uint32_t i = b; i < e; ++i)
        unmet += static_cast<int>(bf_bit(U, a.col_row[i]));
    const int q = Q[c];
    const uint32_t y = q <= 0 ? 1u : 0u;
    const int r = q < 0 ? -q : q;
    return a.check_weight * unmet + (bf_bit(X, c) != y ? r : -r);
}

__global__ __launch_bounds__(kBitFlipMaxFrames * 64) void bit_flip_kernel(const BitFlipArgs a)
{
    extern __shared__ double lds_d[];
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t frame = static_cast<uint64_t>(blockIdx.x) * a.group_frames + wave;
    if (wave >= a.group_frames || frame >= a.n) // (no barrier below: the other waves of the group do not wait)
        return;
    const uint32_t nc = a.nc, mc = a.mc;
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds_d) + static_cast<size_t>(wave) * a.frame_bytes;
    int8_t *Q = reinterpret_cast<int8_t *>(lds);
    uint32_t *X = reinterpret_cast<uint32_t *>(lds + bit_flip_round16(nc));
    uint32_t *U = X + bit_flip_round16(4 * static_cast<size_t>(a.words)) / 4;
    uint32_t *V = U + bit_flip_round16(4 * static_cast<size_t>(a.syn_words)) / 4;

    const uint64_t row_at = a.shared_llr ? 0 : frame * nc; // the frame's first element
    switch (a.llr_type)                                   // (uniform)
    {
    case kLlrF64: bf_prologue(a, static_cast<const double *>(a.llr) + row_at, lane, Q, X); break;
    case kLlrF32: bf_prologue(a, static_cast<const float *>(a.llr) + row_at, lane, Q, X); break;
    case kLlrF16: bf_prologue(a, static_cast<const _Float16 *>(a.llr) + row_at, lane, Q, X); break;
    default: bf_prologue(a, static_cast<const int8_t *>(a.llr) + row_at, lane, Q, X); break;
    }
    bf_wave_sync();
    // u = s XOR H x, a lane per check node, into V
    for (uint32_t base = 0; base < mc; base += 64)
    {
        const uint32_t r = base + lane;
        uint32_t par = 0;
        if (r < mc)
        {
            if (a.syndrome)
            {
                if (a.syndrome_format == kBitsU8)
                    par = static_cast<const uint8_t *>(a.syndrome)[frame * mc + r] != 0 ? 1u : 0u;
                else
                    par = (static_cast<const uint32_t *>(a.syndrome)[frame * a.syn_words + (r >> 5)] >> (r & 31u)) & 1u;
            }
            const uint32_t b = a.row_ptr[r], e = a.row_ptr[r + 1];
            for (uint32_t i = b; i < e; ++i)
                par ^= bf_bit(X, a.row_col[i]);
        }
        const uint64_t m = __ballot(par != 0);
        if (lane == 0)
        {
            const uint32_t w = base >> 5;
            V[w] = static_cast<uint32_t>(m);
            if (w + 1 < a.syn_words)
                V[w + 1] = static_cast<uint32_t>(m >> 32);
        }
    }
    bf_wave_sync();

    uint32_t t = 0, unmet = 0; // unmet: this lane's share of the weight
    for (;;)
    {
        unmet = 0;
        for (uint32_t i = lane; i < a.syn_words; i += 64)
        {
            const uint32_t w = V[i];
            U[i] = w;
            unmet += static_cast<uint32_t>(__popc(w));
        }
        bf_wave_sync();
        if (__ballot(unmet != 0) == 0 || t == a.iterations)
            break;
        // walk 1: the largest penalty of the frame
        int mine = kBfNone;
        for (uint32_t c = lane; c < nc; c += 64)
        {
            const int p = bf_penalty(a, c, Q, X, U);
            mine = p > mine ? p : mine;
        }
        int pmax = mine;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
        {
            const int other = __shfl_xor(pmax, off, 64);
            pmax = other > pmax ? other : pmax;
        }
        const int bar = pmax - a.margin;
        // walk 2: the candidates flip
        if (mine >= bar)
        {
            const uint32_t block0 = t * a.draw_blocks;
            for (uint32_t c = lane; c < nc; c += 64)
            {
                if (bf_penalty(a, c, Q, X, U) < bar)
                    continue;
                if (a.flip_threshold != kBitFlipEveryCandidate)
                {
                    const uint4 w = philox_block(a.k0, a.k1, a.first_frame + frame, block0 + (c >> 2), kTagFlip);
                    if (word_of(w, static_cast<int>(c & 3u)) >= a.flip_threshold)
                        continue;
                }
                atomicXor(&X[c >> 5], 1u << (c & 31u));
                const uint32_t b = a.col_ptr[c], e = a.col_ptr[c + 1];
                for (uint32_t i = b; i < e; ++i)
                {
                    const uint32_t r = a.col_row[i];
                    atomicXor(&V[r >> 5], 1u << (r & 31u));
                }
            }
        }
        bf_wave_sync();
        ++t;
    }

    if (a.iters && lane == 0)
        a.iters[frame] = t;
    if (a.weight) // (uniform)
    {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            unmet += __shfl_xor(unmet, off, 64);
        if (lane == 0)
            a.weight[frame] = unmet;
    }
    if (a.hard_bits)
    {
        uint32_t *h = a.hard_bits + frame * a.words;
        for (uint32_t i = lane; i < a.words; i += 64)
            h[i] = X[i];
    }
}
} // namespace

int launch_bit_flip(const BitFlipArgs &a, void *stream)
{
    if (a.n == 0)
        return hipSuccess;
    if (a.nc == 0 || a.nc > 0xFFFFu || a.mc == 0 || a.mc > 0xFFFFu || a.words != (a.nc + 31) / 32 || a.syn_words != (a.mc + 31) / 32 ||
        a.iterations > 0xFFFFu || a.qmax < 1 || a.qmax > 127 || a.check_weight < 1 || a.check_weight > 255 || a.margin < 0 ||
        a.margin > 0xFFFF || a.draw_blocks != (a.nc + 3) / 4 || !a.row_ptr || !a.row_col || !a.col_ptr || !a.col_row || !a.llr ||
        llr_type_bytes(a.llr_type) == 0 || (a.syndrome && !bits_format_known(a.syndrome_format)) ||
        a.frame_bytes != bit_flip_lds_bytes(a.nc, a.mc) || a.group_frames != bit_flip_group_frames(a.frame_bytes) ||
        static_cast<size_t>(a.group_frames) * a.frame_bytes > 160 * 1024 || a.n > (1ull << 20))
        return hipErrorInvalidValue;
    const uint64_t groups = (a.n + a.group_frames - 1) / a.group_frames;
    return launch_with_lds(bit_flip_kernel, dim3(static_cast<unsigned>(groups)), dim3(a.group_frames * 64), a.group_frames * a.frame_bytes,
                           stream, a);
}

} // namespace ldpc_amd
