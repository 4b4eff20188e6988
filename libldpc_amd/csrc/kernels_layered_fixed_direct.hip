// kernels_layered_fixed_direct.hip — fixed-point layered min-sum (kernels_layered_fixed.hip) on TYPED LLRs given in memory:
// binary32, binary16 or int8 (include/ldpc_amd.h, ldpc_hip_decode_batch_typed).  The decoder quantizes its input once and
// never looks at the binary64 value again, so these instantiations do not stage it: the prologue reads the frame's typed
// values from memory in column order (coalesced), widens each to binary64 W — exactly, every one of these types is a
// subset of binary64 — quantizes W and stores the total at the column's rank.  Everything after that is the shared text of
// kernels_layered_fixed_body.inc, so the outputs are those of the staged form on W bit for bit.
//
// What LDS holds per frame (plan.hpp, layered_fixed_direct_region_bytes): the totals T[nc], int16; from the next multiple of
// 4 one 32-bit record per check-node slot; behind the records the correction table, 128 bytes.  No 8 nc bytes of binary64:
// h.txt 6 528 bytes instead of 9 344 (25 frames per CU instead of 17), the n = 8192 (3,6) code 32 896 instead of 65 664 (four
// instead of two).
//
// int8 values ARE the quantized values: k stands for W = fl(k * step), and lf_quantize(W, fl(1 / step)) == clamp(k, -Qmax,
// +Qmax) for every int8 k and every step the setter takes (the two roundings are off by less than 2^-51 relative, rint returns
// k; tests/test_typed_batch_host.py checks all 256 k against 200 011 steps).  They are read a dword per lane from the first
// 4-byte boundary of the frame's row on; a row starts at byte frame * nc of the batch, at any alignment.
#include "kernels_layered_fixed_impl.hpp"

namespace ldpc_amd
{

namespace
{
template <bool WANT_LLR>
__global__ __launch_bounds__(kLfThreads) void decode_layered_fixed_direct_kernel(const DecodeArgs a, const DevLayerPlan L, const LayeredFixedArgs q,
                                                                                 const TypedLlrArgs t)
{
    extern __shared__ double lds_d[];
    const DevPlan &P = a.plan;
    const int nc = P.nc;
    const int lane = threadIdx.x;
    const uint64_t frame = blockIdx.x;
    if (frame >= a.n_frames)
        return;
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds_d);
    const uint32_t rec_slots = L.record_bytes / 20;
    lds_i16 *T = reinterpret_cast<lds_i16 *>(lds);
    lds_u32 *records = reinterpret_cast<lds_u32 *>(lds + layered_fixed_records_off(nc));
    uint8_t *lut = lds + layered_fixed_records_off(nc) + 4 * static_cast<size_t>(rec_slots);
    const uint8_t *cw = a.codeword ? a.codeword + frame * nc : nullptr;
    const int qmax = q.qmax, pmax = q.pmax;
    const uint32_t *col_rank = P.col_rank;
    double *o = a.llr_in_dump ? a.llr_in_dump + frame * nc : nullptr; // (llr_in is W, in column order)

    lf_load_lut(q, lut, lane);
    if (t.type == kLlrI8)
    {
        const int8_t *src = static_cast<const int8_t *>(t.llr) + frame * nc;
        auto put = [&](int c, int k) {
            if (o)
                o[c] = static_cast<double>(k) * q.step;
            T[col_rank[c]] = static_cast<int16_t>(lf_clamp(k, qmax));
        };
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
    else if (t.type == kLlrF16)
    {
        const _Float16 *src = static_cast<const _Float16 *>(t.llr) + frame * nc;
        for (int c = lane; c < nc; c += 64)
        {
            const double x = static_cast<double>(src[c]);
            if (o)
                o[c] = x;
            T[col_rank[c]] = static_cast<int16_t>(lf_quantize(x, q.inv, qmax));
        }
    }
    else
    {
        const float *src = static_cast<const float *>(t.llr) + frame * nc;
        for (int c = lane; c < nc; c += 64)
        {
            const double x = static_cast<double>(src[c]);
            if (o)
                o[c] = x;
            T[col_rank[c]] = static_cast<int16_t>(lf_quantize(x, q.inv, qmax));
        }
    }
    __syncthreads(); // (one wave: orders the compiler and the LDS queue)
#include "kernels_layered_fixed_body.inc"
}
} // namespace

int launch_decode_layered_fixed_direct(const DecodeArgs &a, const DevLayerPlan &L, const LayeredFixedArgs &q, const TypedLlrArgs &t,
                                       void *stream)
{
    if (a.n_frames == 0)
        return hipSuccess;
    const uint64_t nc = a.plan.nc > 0 ? static_cast<uint64_t>(a.plan.nc) : 0;
    const size_t region = layered_fixed_direct_region_bytes(L.record_bytes / 20, nc);
    if (!L.steps || !L.vn4 || !L.rec_off || L.record_bytes == 0 || L.record_bytes % 20 != 0 || nc == 0 || nc > 0xFFFF || region > kCuLdsBytes ||
        q.qmax < 1 || q.qmax > 127 || q.pmax < q.qmax || q.pmax > 32767 || a.n_frames > 0x7FFFFFFFull || !t.llr || !a.plan.col_rank ||
        (t.type != kLlrF32 && t.type != kLlrF16 && t.type != kLlrI8))
        return hipErrorInvalidValue;
    void (*k)(const DecodeArgs, const DevLayerPlan, const LayeredFixedArgs, const TypedLlrArgs) =
        a.llr_out ? decode_layered_fixed_direct_kernel<true> : decode_layered_fixed_direct_kernel<false>;
    return launch_with_lds(k, dim3(static_cast<unsigned>(a.n_frames)), dim3(kLfThreads), static_cast<uint32_t>(region), stream, a, L, q, t);
}

} // namespace ldpc_amd
