// kernels_layered_fixed.hip — opt-in NON-PARITY FIXED-POINT LAYERED min-sum decoding ("BP_MS" with
// ldpc_hip_set_min_sum_layered_fixed(msg_bits, app_bits, step); include/ldpc_amd.h states the arithmetic).  The decoder that
// LDPC hardware implements: the layered (row-serial) schedule on a saturating integer datapath, messages of q = 2..8 bits and
// a wider a-posteriori total of p <= 16 bits per column.  Everything after the one quantization of the channel LLRs is integer
// arithmetic, so every output bit follows from the contract and is held against a numpy mirror bit for bit
// (tests/layered_fixed_minsum_ref.py).  The reference has no such decoder (decoder.cpp:22-76 is flooding, binary64).
//
// Mapping as in kernels_layered_ms.hip: ONE WAVE = ONE FRAME, a sweep is the sequence of STEPS of build_layer_plan (plan.cpp),
// a step is up to 64 check nodes of equal degree that share no variable node, one per lane; the steps need no barrier (a
// wave's LDS operations execute in order) and a step's neighbour table is fetched one step ahead.
//
// What LDS holds per frame (plan.hpp, layered_fixed_region_bytes):
//   * first the nc binary64 channel LLRs, written by channel_init as everywhere (all channel and noise modes);
//   * then, over the same bytes: the totals T[nc], int16 (the wave quantizes the LLRs IN PLACE, below); behind them, from
//     the next multiple of 4, per check node ONE 32-bit RECORD instead of its D messages.  The outputs of a min-sum check
//     node take two magnitudes only: every edge but the one that holds the smallest input gets lut[min1], that edge gets
//     lut[min2].  The record is lut[min1] in bits 0..6, lut[min2] in bits 7..13, the argmin position in bits 14..16 and the
//     D output sign bits from bit 17 on; message j is (j == argmin ? lut[min2] : lut[min1]) with sign bit j — exactly the
//     message a full array would hold (where two inputs tie for the minimum, min2 == min1 and either argmin gives the same
//     values).  Records are laid out [lane] within a step, the step's real check nodes rounded up to an even number (the
//     slots of plan.hpp, layered_ms_records: rec_off / 20 is the step's first slot);
//   * behind the larger of the two, the correction table, 128 bytes.
// h.txt: 9 344 bytes per frame, 17 frames per CU; the n = 8192 (3,6) code 65 664, two.
//
// The typed batch call (ldpc_hip_decode_batch_typed) has a form of its own without the binary64 area: h.txt 6 528 bytes and 25
// frames per CU (kernels_layered_fixed_direct.hip).  What the two share is kernels_layered_fixed_impl.hpp and
// kernels_layered_fixed_body.inc.
//
// Iteration count returned: sweeps completed before the sweep whose syndrome check passed (the reference's convention,
// decoder.cpp:21-22,74-77); the syndrome of the current decisions is taken after every sweep.
#include "kernels_layered_fixed_impl.hpp" // the quantizer and the check node (shared with the direct form)

namespace ldpc_amd
{

namespace
{
template <bool WANT_LLR>
__global__ __launch_bounds__(kLfThreads) void decode_layered_fixed_kernel(const DecodeArgs a, const DevLayerPlan L, const LayeredFixedArgs q)
{
    extern __shared__ double lds_d[];
    const DevPlan &P = a.plan;
    const int nc = P.nc;
    const int lane = threadIdx.x;
    const uint64_t frame = blockIdx.x;
    if (frame >= a.n_frames)
        return;
    unsigned char *lds = reinterpret_cast<unsigned char *>(lds_d);
    const uint32_t rec_slots = L.record_bytes / 20; // (layered_ms_records: 20 bytes per slot there, one word here)
    lds_i16 *T = reinterpret_cast<lds_i16 *>(lds);
    lds_u32 *records = reinterpret_cast<lds_u32 *>(lds + layered_fixed_records_off(nc));
    uint8_t *lut = lds + layered_fixed_lut_off(rec_slots, nc);
    const uint8_t *cw = a.codeword ? a.codeword + frame * nc : nullptr;
    const int qmax = q.qmax, pmax = q.pmax;

    channel_init<64, kNoiseAny>(a, frame, lds_d, lane); // binary64 channel + LLR initialisation, as everywhere (one wave's worth)
    if (lane < 32) // (a select chain over the launch arguments: indexing them by a lane's number would put them in scratch)
    {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 32; ++i)
            w = lane == i ? q.lut[i] : w;
        reinterpret_cast<lds_u32 *>(lut)[lane] = w; // (behind the binary64 area)
    }
    __syncthreads(); // (one wave: orders the compiler and the LDS queue, costs nothing)
    // The LLRs become the totals IN PLACE.  Chunk k = columns 64 k .. 64 k + 63: every lane reads its binary64 value (bytes
    // 512 k + 8 lane ..), then every lane writes its int16 (bytes 128 k + 2 lane ..) — one load instruction of the whole wave
    // before one store instruction, the store's value depending on the load's.  The int16 image of chunk k lies in bytes
    // [128 k, 128 k + 128), inside [512 (k / 4), 512 (k / 4) + 512): binary64 values of chunk k / 4 <= k, all read already;
    // chunks after k read from byte 512 (k + 1) > 128 k + 128 on.  In the last chunk of a column count that is no multiple of
    // 64 the lanes beyond nc neither read nor write: the bytes they would have written hold no column.
    {
        const lds_f64 *llr = reinterpret_cast<const lds_f64 *>(lds);
        double *o = a.llr_in_dump ? a.llr_in_dump + frame * nc : nullptr;
        for (int r = lane; r < nc; r += 64)
        {
            const double x = llr[r];
            if (o)
                o[P.rank_col[r]] = x; // (llr_in stays the unquantized value)
            T[r] = static_cast<int16_t>(lf_quantize(x, q.inv, qmax));
        }
    }
    __syncthreads(); // the binary64 area is free
#include "kernels_layered_fixed_body.inc"
}
} // namespace

int launch_decode_layered_fixed(const DecodeArgs &a, const DevLayerPlan &L, const LayeredFixedArgs &q, void *stream)
{
    if (a.n_frames == 0)
        return hipSuccess;
    const uint64_t nc = a.plan.nc > 0 ? static_cast<uint64_t>(a.plan.nc) : 0;
    const size_t region = layered_fixed_region_bytes(L.record_bytes / 20, nc);
    if (!L.steps || !L.vn4 || !L.rec_off || L.record_bytes == 0 || L.record_bytes % 20 != 0 || nc == 0 || nc > 0xFFFF || region > kCuLdsBytes ||
        q.qmax < 1 || q.qmax > 127 || q.pmax < q.qmax || q.pmax > 32767 || a.n_frames > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    void (*k)(const DecodeArgs, const DevLayerPlan, const LayeredFixedArgs) =
        a.llr_out ? decode_layered_fixed_kernel<true> : decode_layered_fixed_kernel<false>;
    return launch_with_lds(k, dim3(static_cast<unsigned>(a.n_frames)), dim3(kLfThreads), static_cast<uint32_t>(region), stream, a, L, q);
}

} // namespace ldpc_amd
