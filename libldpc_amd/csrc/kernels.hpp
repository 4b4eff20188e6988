// kernels.hpp — host-visible launch interface of the HIP kernels (the .hip files of this directory).
#pragma once

#include <cstddef>
#include <cstdint>

#include "plan.hpp"

namespace ldpc_amd
{

// Device copy of Plan: all pointers are device pointers owned by the engine.
struct DevPlan
{
    int nc, mc, nnz, nct;
    int n_bitpos;
    int n_cn_blocks, n_vn_blocks;
    int cn_work_stride, vn_work_stride;
    const CnBlock *cn_blocks;
    const VnBlock *vn_blocks;
    const uint32_t *vn_slot;
    const uint32_t *cn_work;
    const uint32_t *vn_work;
    const CnBlock *cn_work_desc; // [kDecodeWaves][cn_desc_stride], count 0 = none
    int cn_desc_stride;
    const uint32_t *vn_work_desc; // [kDecodeWaves][vn_work_stride + 1][4], count 0 = none
    const uint32_t *vn_packed;    // [kDecodeWaves][16][64] register-held slot indices as the lanes keep them (plan.hpp), or null
    const uint32_t *col_rank;
    const uint32_t *rank_col;
    const uint32_t *tx_rank;
    const uint8_t *rank_kind;
    const uint32_t *rank_slot0;
    const int *bit_pos; // [n_bitpos] transmitted index -> column
    uint32_t lds_bytes;
};

enum ChannelMode : int
{
    kModeLlr = 0,  // LLRs given per frame (C-ABI decode, shared.cpp:47-65)
    kModeAwgn = 1, // fused channel_awgn::simulate + calculate_llrs (channel.cpp:62-93)
    kModeBsc = 2,  // fused channel_bsc (channel.cpp:129-162)
    // opt-in NON-PARITY counter-based noise (device_philox.hpp): the frame's noise from (ctr_key, ctr_frame0 + frame, bit)
    kModeAwgnCtr = 3, // AWGN normals
    kModeBscCtr = 4,  // BSC draws
};

struct DecodeArgs
{
    DevPlan plan;
    uint32_t iterations;
    int early_term;
    int mode;
    uint64_t n_frames;
    // kModeLlr
    const double *llr_in; // [n_frames][nc], column order
    // kModeAwgn: the two normals (bit patterns of y*mult, x*mult) of every accepted polar pair of the stream, as the noise
    // generator left them: one SLAB per generator chunk, compacted inside the slab in stream order (rng_kernels.hip,
    // polar_slab_kernel).  slab_cum[j] = pairs in the slabs before j (slab_cum[0] = 0, n_slabs + 1 entries, followed by four
    // entries of 2^64-1); the pair with
    // stream index q sits in the slab j with slab_cum[j] <= q - pair_origin < slab_cum[j+1], at
    // pairs[j * slab_words + 2 * (q - pair_origin - slab_cum[j])].  Normal g = frame*nct + i comes from pair g>>1.
    const uint64_t *pairs;
    const uint64_t *slab_cum;
    uint64_t slab_words;      // 64-bit words per slab (2 x the pairs a chunk can hold)
    uint32_t n_slabs;
    float slab_pairs_inv;     // 1 / (expected pairs per slab): first guess of the slab of a frame
    uint64_t pair_origin;     // stream index of the first pair of slab 0
    uint64_t normal_base;     // index of this batch's first normal in the stream
    int pairs_buffer;         // host bookkeeping: which of the engine's two slab buffers `pairs` points into
    double sigma, sigma2; // sqrt(sigma2), sigma2 = 10^(-snr/10)
    double inv_sigma2;    // 1 / sigma2, correctly rounded (host division): detmath.h, dm_div_by
    double shorten_llr;   // 99999.9 (AWGN) or delta (BSC)
    // kModeBsc: raw draws, one per transmitted bit: raw[frame*nct + i]
    const uint64_t *raw;
    double eps, delta;
    // transmitted codeword per frame [n_frames][nc] (nullptr = all-zero codeword)
    const uint8_t *codeword;
    // outputs (any may be nullptr)
    uint32_t *iters;
    uint32_t *bit_errors;
    uint8_t *hard;        // [n_frames][nc]
    double *llr_out;      // [n_frames][nc]
    double *llr_in_dump;  // [n_frames][nc]
    // memory-resident decoder only: per-frame state in device memory instead of LDS
    double *ws_msg;  // [n_frames][nnz]
    double *ws_llr;  // [n_frames][nc]
    uint8_t *ws_hb;  // [n_frames][nnz]
    double *ws_scr;  // [n_frames][2 nnz] scratch of check nodes wider than 16 (nullptr when the code has none);
                     // totals-form register kernel: [n_frames][(nv0 + nv1) * nt] channel terms of the variable nodes
    // sum-product in likelihood-ratio form (detmath.h), the lists of a launch's Stage (below): a stage that hands frames on
    // appends the frames it could not finish to redo_list[atomicAdd(redo_count)]; a stage that reads a list decodes exactly
    // those frames (block b takes frame redo_list_in[b], b < *redo_count_in; kListChain: a small grid walks the list)
    uint32_t *redo_list;
    uint32_t *redo_count;
    // unused, kept in place: moving or removing a host-only member of this struct changed the compiler's register allocation
    // and scratch use of dozens of kernel instantiations that take it by value (the static_asserts below hold the layout)
    int ratio_separate;
    const uint32_t *redo_list_in;
    const uint32_t *redo_count_in;
    // hand-over (kHandoverFirst -> kHandoverResume; detmath.h "Hand-over"): redo_iter[pos] = iteration the frame
    // redo_list[pos] resumes at in the LLR domain (0xFFFFFFFF: decode it from scratch), ws_handover[pos][nnz] = its c2v
    // messages as the ratio form left them (lambda, a decision in the sign bit), in message-slot order
    uint32_t *redo_iter;
    const uint32_t *redo_iter_in;
    double *ws_handover;
    int handover_llr; // ws_handover holds the c2v messages as LLRs already (the fused form's hand-over), not as lambda
    uint64_t *phase_trace; // debug builds with -DLDPC_AMD_PHASE_TRACE only: [2048 frames of mid-launch][4 waves][8 values]
    // kModeAwgnCtr / kModeBscCtr: Philox key (seed & 0xFFFFFFFF, seed >> 32) and the stream index of the batch's frame 0
    uint32_t ctr_key[2];
    uint64_t ctr_frame0;
    // opt-in NON-PARITY corrected min-sum (device_cn.hpp, MsCorr): a min-sum launch with ms_correct set takes the corrected
    // instantiations, whose check nodes output max(fl(fl(ms_scale * m) - ms_offset), +0.0) with the sign of plain min-sum
    int ms_correct;
    double ms_scale, ms_offset;
};
// the kernels take DecodeArgs by value and their register allocation follows its layout: no member moves
static_assert(sizeof(DecodeArgs) == 512 && offsetof(DecodeArgs, plan) == 0 && offsetof(DecodeArgs, iterations) == 168 &&
                  offsetof(DecodeArgs, redo_list) == 392 && offsetof(DecodeArgs, ratio_separate) == 408 &&
                  offsetof(DecodeArgs, redo_list_in) == 416 && offsetof(DecodeArgs, ms_correct) == 488 &&
                  offsetof(DecodeArgs, ms_offset) == 504,
              "DecodeArgs: layout changed");

// What one decode launch is for.  A batch takes one to three launches (engine.hpp, decode_stages); the
// stage says which form runs and which lists the launch reads and writes.
enum class Stage : int
{
    kWhole,          // no list: min-sum, the LLR-domain sum-product from scratch, the fast / layered modes
    kRatioFirst,     // list out: ratio form over the batch, early termination on
    kRatioSeparate,  // lists in and out: ratio form again, every check-node output divided separately (not LDS-resident)
    kListChain,      // list in: separately divided ratio form, then the LLR domain, frame by frame (LDS-resident)
    kLlrRedo,        // list in: the listed frames from scratch in the LLR domain
    kHandoverFirst,  // list out + redo_iter, ws_handover: ratio form without early termination (LDS-resident)
    kHandoverResume, // list in + redo_iter_in, ws_handover, handover_llr: the LLR domain resuming those frames
};
constexpr bool stage_writes_list(Stage s) { return s == Stage::kRatioFirst || s == Stage::kRatioSeparate || s == Stage::kHandoverFirst; }
constexpr bool stage_reads_list(Stage s)
{
    return s == Stage::kRatioSeparate || s == Stage::kListChain || s == Stage::kLlrRedo || s == Stage::kHandoverResume;
}
constexpr bool stage_is_handover(Stage s) { return s == Stage::kHandoverFirst || s == Stage::kHandoverResume; }
// every launcher's one check of the arguments: the pointers the stage needs are there, and the stages of the ratio form
// (iterations to run; early termination on, or the hand-over without it) are what the arguments describe
inline bool stage_args_ok(const DecodeArgs &a, Stage s)
{
    if (stage_writes_list(s) && (!a.redo_list || !a.redo_count))
        return false;
    if (stage_reads_list(s) && (!a.redo_list_in || !a.redo_count_in))
        return false;
    if (stage_is_handover(s) && (!a.ws_handover || !(s == Stage::kHandoverFirst ? a.redo_iter : a.redo_iter_in)))
        return false;
    return s == Stage::kWhole || (a.iterations > 0 && stage_is_handover(s) == !a.early_term);
}

// device copy of RegPlan (register-resident decoder, kernels_reg.hip)
struct DevRegPlan
{
    int nt, kc, maxd, rounds;
    uint32_t mb_doubles;
    const uint32_t *cn_edge;
    const uint8_t *cn_deg;
    const uint8_t *cn_cnt;
    const RegVnBlock *vn_blocks;
    const uint32_t *round_first;
};

// device copy of Reg2Plan (register-resident decoder, second form: kernels_reg2.hip)
struct DevReg2Plan
{
    int nt, kc, maxd, nv0, nv1;
    uint32_t neutral, lds_entries;
    int uniform_cn; // every check-node block has maxd edges
    int uniform_vn; // every variable-node block is full, of degree 3, at the affine offsets below
    // round r: column position 0 of block q = i * (nt/64) + wave at entry vn_affine[r][0] + vn_affine[r][1] * q (+ lane),
    // positions 1.. at [2] + [3] * q (+ 64 per position), the total at [4] + [5] * q
    uint32_t vn_affine[2][6];
    const uint32_t *edge_w;
    const uint8_t *cn_deg;
    const Reg2VnBlock *vn_blocks;
    const uint32_t *vn_rank;
};

// device copy of FusedPlan (fused form of the likelihood-ratio iteration: kernels_fused.hip)
struct DevFusedPlan
{
    int n_slots, vnb, cnl, calls_stride;
    int has_shortened;
    int need_lambda; // a column that is transmitted or shortened has three or more edges: the prologue stages lambda_ch too
    int wide_exclusive;
    uint32_t vn_prog[kDecodeWaves]; // plan.hpp, FusedPlan::vn_prog
    uint32_t lds_bytes;          // dynamic LDS per frame: the message slots, or the staging area of the prologue if larger
    const FusedCall *leaf_calls; // [kDecodeWaves][kFusedLeafCalls]
    const FusedCall *calls;      // [kDecodeWaves][calls_stride]
    const uint32_t *vn_desc;     // [kDecodeWaves][kFusedVnSlots][4]
    const uint32_t *vn_slot;
    const uint32_t *lane_tab;    // [kDecodeWaves][kFusedLaneRows][64]
    const uint32_t *ho_map;      // [n_slots] (plan.hpp, FusedPlan::ho_map)
    int program;                 // plan.hpp, FusedPlan::program (read by the host side of the launch only: it selects the kernel)
};
// the fused family on the LDS-resident decoder's plan: kRatioFirst, kHandoverFirst (separately divided outputs; the messages
// are handed over as LLRs: handover_llr for the resuming launch) and kWhole = min-sum without early termination
int launch_decode_fused(const DecodeArgs &a, const DevFusedPlan &f, Stage stage, void *stream);

// BEC (u8 erasure alphabet, decoder.cpp:91-192 + channel.cpp:199-229)
struct BecArgs
{
    DevPlan plan;
    uint32_t iterations;
    int early_term;
    int deg1_compat; // 1: erased degree-1 VN emits 0 (what the reference's out-of-bounds read yields)
    uint64_t n_frames;
    const uint64_t *raw; // raw[frame*nct + i], nullptr when symbols are given
    double eps;
    const uint8_t *symbols;  // [n_frames][nc] channel LLR alphabet {0,1,'E'} (when raw == nullptr)
    const uint8_t *codeword; // [n_frames][nc] or nullptr
    uint32_t *iters;
    uint32_t *bit_errors;
    uint8_t *hard;
    double *llr_out;     // symbol values 0, 1, 'E' widened to double
    double *llr_in_dump;
    uint8_t *ws;         // per-frame state in device memory (codes whose bec_state_bytes() exceed LDS), else nullptr
    // counter-based noise (device_philox.hpp; raw == nullptr, symbols == nullptr): erasures from (ctr_key, ctr_frame0 + frame, bit)
    int counter;
    uint32_t ctr_key[2];
    uint64_t ctr_frame0;
};

// bytes of a frame's state in the byte-per-message erasure kernel (bec_kernel, kernels_bec.hip): msg[nnz], sym[nc], lout[nc],
// each array from a 16-byte boundary.  Beyond kCuLdsBytes the state lives in device memory (BecArgs::ws)
constexpr uint32_t bec_state_bytes(int nnz, int nc)
{
    return static_cast<uint32_t>(((nnz + 15) / 16) * 16 + 2 * (((nc + 15) / 16) * 16));
}
// the erasure decoder (kernels_bec.hip): bit-sliced, 32 frames per workgroup, where that state fits LDS, else bec_kernel
int launch_bec(const BecArgs &a, void *stream);

// All launchers enqueue on `stream` (hipStream_t passed as void*) and return a hipError_t as int.
// LDS-resident decoder; llr_mode: 0 input LLRs in LDS, 2 in registers (needs plan.vn_work_stride <= 8 and no isolated
// variable node)
int launch_decode_lds(const DecodeArgs &a, Stage stage, bool min_sum, int max_cn_degree, int llr_mode, void *stream);
// memory-resident variant for codes whose messages do not fit LDS (a.ws_* must be set); occupancy_lds
// bytes of dynamic LDS are requested only to bound the number of resident frames per CU
int launch_decode_mem(const DecodeArgs &a, Stage stage, bool min_sum, int max_cn_degree, uint32_t occupancy_lds, void *stream);
// register-resident decoder: a.ws_llr [n][nc] doubles and a.ws_hb [n][nc] bytes must be set
int launch_decode_reg(const DecodeArgs &a, const DevRegPlan &r, Stage stage, bool min_sum, void *stream);
// register-resident decoder, second form (same workspace requirements)
int launch_decode_reg2(const DecodeArgs &a, const DevReg2Plan &r, Stage stage, bool min_sum, void *stream);
// opt-in non-parity fast mode (kernels_fast.hip): sum-product with binary32 messages; a.ws_hb [n][nc] must be set
bool fast_mode_supported(const DevPlan &p, int max_cn_degree);
int launch_decode_fast(const DecodeArgs &a, int max_cn_degree, void *stream);
// opt-in non-parity layered schedule (kernels_layered.hip): device copy of LayerPlan (plan.hpp)
struct DevLayerPlan
{
    const uint32_t *steps; // [n_steps][2]: offset into vn / the message array, count | degree << 16
    const uint32_t *vn4;   // [(step * 4 + w) * 64 + lane]: VN ranks of edges 2w, 2w+1 of the step's lane-th check node (16 bits each)
    uint32_t n_steps, slots;
    uint32_t region_bytes, region_bytes_half; // LDS per frame with binary32 / binary16 messages
    // layered min-sum (kernels_layered_ms.hip): byte offset of each step's check-node records behind the frame's totals
    // (plan.hpp, layered_ms_records), their size in all, and the frame's LDS: 8 nc bytes of totals + the records
    const uint32_t *rec_off; // [n_steps]
    uint32_t record_bytes, region_bytes_ms;
};
int launch_decode_layered(const DecodeArgs &a, const DevLayerPlan &L, bool half_messages, void *stream);
// opt-in non-parity layered schedule of min-sum (kernels_layered_ms.hip): binary64 totals, compressed check-node records;
// the correction of a.ms_scale / a.ms_offset always applies ((1, 0) is plain min-sum, bit for bit)
int launch_decode_layered_ms(const DecodeArgs &a, const DevLayerPlan &L, void *stream);
// opt-in non-parity quantized (fixed-point) min-sum (kernels_qms.hip; include/ldpc_amd.h,
// ldpc_hip_set_min_sum_quantization): device copy of QmsPlan (plan.hpp) and the frame's LDS
struct DevQmsPlan
{
    const uint32_t *cn_desc;  // [mc][2]: byte offset of the check node's first slot (a multiple of 4), its degree
    const uint16_t *cn_vn;    // [slots]
    const uint32_t *vn_start; // [nc + 1]
    const uint32_t *vn_slot;  // [nnz]
    uint32_t slots;           // message bytes of a frame (a multiple of 4)
    uint32_t work_bytes;      // plan.hpp, qms_work_bytes: the quantized channel values sit behind it
    uint32_t region_bytes;    // plan.hpp, qms_region_bytes
};
// what the host works out for one launch: the quantizer and the correction table.  The kernel never sees the correction's
// scale and offset (a.ms_scale / a.ms_offset are not read), only lut[m] for the magnitudes m = 0..qmax, four per word
struct QmsArgs
{
    double step, inv; // the LLR step and fl(1 / step)
    int32_t qmax;     // 2^(bits - 1) - 1, 1..127
    int32_t pad;
    uint32_t lut[32];
};
int launch_decode_qms(const DecodeArgs &a, const DevQmsPlan &Q, const QmsArgs &q, void *stream);
// opt-in non-parity fixed-point layered min-sum (kernels_layered_fixed.hip; include/ldpc_amd.h,
// ldpc_hip_set_min_sum_layered_fixed) on the layered plan's tables (steps, vn4, rec_off / 20 = a step's first record slot).
// The quantizer, the two saturation limits and the correction table of one launch: as for QmsArgs the kernel never sees the
// correction's scale and offset, only lut[m] for m = 0..qmax, four per word
struct LayeredFixedArgs
{
    double step, inv; // the LLR step and fl(1 / step)
    int32_t qmax;     // 2^(msg_bits - 1) - 1, 1..127
    int32_t pmax;     // 2^(app_bits - 1) - 1, qmax..32767
    uint32_t lut[32];
};
int launch_decode_layered_fixed(const DecodeArgs &a, const DevLayerPlan &L, const LayeredFixedArgs &q, void *stream);
// typed LLRs of the batch call (include/ldpc_amd.h, ldpc_hip_decode_batch_typed: LDPC_HIP_LLR_*)
enum LlrType : int
{
    kLlrF64 = 0,
    kLlrF32 = 1,
    kLlrF16 = 2, // IEEE binary16
    kLlrI8 = 3,  // k stands for fl(k * step) of the fixed-point mode in force
};
constexpr size_t llr_type_bytes(int type) { return type == kLlrF64 ? 8 : type == kLlrF32 ? 4 : type == kLlrF16 ? 2 : type == kLlrI8 ? 1 : 0; }
// the typed input of a launch, beside DecodeArgs (whose layout does not move): [n_frames][nc] elements of `type`, column order
struct TypedLlrArgs
{
    const void *llr;
    int32_t type; // kLlrF32, kLlrF16 or kLlrI8
    int32_t pad;
};
// fixed-point layered min-sum reading typed LLRs itself (kernels_layered_fixed_direct.hip): a.llr_in is not read, no binary64
// LLRs are staged in LDS (plan.hpp, layered_fixed_direct_region_bytes); the outputs are those of launch_decode_layered_fixed
// on the widened values, a.llr_in_dump included
int launch_decode_layered_fixed_direct(const DecodeArgs &a, const DevLayerPlan &L, const LayeredFixedArgs &q, const TypedLlrArgs &t,
                                       void *stream);
// kernels_convert.hip: dst[i] = src[i] widened to binary64 (kLlrF32, kLlrF16: exact) or fl((double) src[i] * step) (kLlrI8),
// i < count; bits[f][ceil(nc / 32)] = the decision bytes hard[f][nc] packed, bit c & 31 of word c >> 5, unused bits zero
int launch_widen_llr(const void *src, int type, double step, uint64_t count, double *dst, void *stream);
int launch_pack_hard(const uint8_t *hard, uint64_t n, int nc, uint32_t *bits, void *stream);

// ---- GF(2) work on frames of bits (kernels_gf2.hip; include/ldpc_amd.h, ldpc_hip_encode_batch / _syndrome_batch /
// _bit_errors_batch).  A row of L bits is bytes (non-zero = 1) or packed as hard_bits is, ceil(L / 32) words ----
enum BitsFormat : int
{
    kBitsU8 = 0,
    kBitsPacked32 = 1,
};
constexpr bool bits_format_known(int f) { return f == kBitsU8 || f == kBitsPacked32; }
constexpr size_t bits_row_bytes(int format, uint64_t bits) { return format == kBitsU8 ? bits : 4 * ((bits + 31) / 32); }
// the encoder: a lane keeps at most kGf2MaxChunkWords words of its column's mask in registers and walks a longer information
// word in chunks of that many; kGf2FrameTile frames share them, kGf2FramesPerBlock frames a workgroup's 256 columns
constexpr int kGf2MaxChunkWords = 32, kGf2FrameTile = 16, kGf2FramesPerBlock = 64;
// the chunk T of a code with `words` information words: the largest power of two <= min(words, kGf2MaxChunkWords), so that
// every window of T words lies inside the row
int gf2_encode_chunk_words(uint32_t words);
struct Gf2EncodeArgs
{
    uint32_t nc, words;       // words = ceil(kc / 32)
    uint64_t mask_cols;       // nc rounded up to a multiple of 256
    const uint32_t *mask;     // [words][mask_cols]: word w of column j's mask over the information word (zero columns beyond G.cols)
    const uint32_t *info;     // [n][words] packed information bits (the bits from kc on are not read: no mask has them)
    uint8_t *codeword;        // [n][nc] or nullptr
    uint32_t *codeword_bits;  // [n][ceil(nc / 32)] or nullptr
    uint64_t n;               // at most 65535 * kGf2FramesPerBlock
};
int launch_gf2_encode(const Gf2EncodeArgs &a, void *stream);
// the syndrome: one wave per frame (four frames per workgroup) up to kGf2SyndromeWaveCols columns, four waves per frame beyond;
// the frame's packed word in LDS, 8 bytes per 64 columns
constexpr uint32_t kGf2SyndromeWaveCols = 4096;
constexpr size_t kGf2SyndromeMaxLds = 64 * 1024;
constexpr int gf2_syndrome_waves_per_frame(uint32_t nc) { return nc <= kGf2SyndromeWaveCols ? 1 : 4; }
constexpr size_t gf2_syndrome_frame_lds_bytes(uint32_t nc) { return 8 * ((static_cast<size_t>(nc) + 63) / 64); }
struct Gf2SyndromeArgs
{
    uint32_t nc, mc;
    const uint32_t *row_ptr;  // [mc + 1] row CSR of H, entries in file order (a repeated entry counts twice)
    const uint32_t *row_col;  // [nnz]
    const void *word;         // [n][nc] bytes or [n][ceil(nc / 32)] words
    uint8_t *syndrome;        // [n][mc] or nullptr
    uint32_t *syndrome_bits;  // [n][ceil(mc / 32)] or nullptr
    uint32_t *weight;         // [n] or nullptr
    uint64_t n;
};
int launch_gf2_syndrome(const Gf2SyndromeArgs &a, int format, void *stream);
struct Gf2BitErrorArgs
{
    uint32_t nc;
    const uint64_t *tx_mask;  // [ceil(nc / 64)]: bit c & 63 of word c >> 6 set where column c is transmitted
    const void *a, *b;        // [n][nc] bytes or [n][ceil(nc / 32)] words, each in its own format
    uint32_t *bit_errors;     // [n]
    uint64_t n;               // at most 2^31
};
int launch_gf2_bit_errors(const Gf2BitErrorArgs &a, int a_format, int b_format, void *stream);

// ---- channel and demapper for frames of bits (kernels_channel.hip; include/ldpc_amd.h, ldpc_hip_channel_batch): codeword bits
// in, LLRs of element type `llr_type` out, the noise that of the counter mode (device_philox.hpp).  One lane owns one Philox
// block of a frame: four symbols of m bits; the columns the channel does not write (punctured, shortened, unconnected) are
// filled by further lanes of the same launch ----
constexpr int kChannelMaxBitsPerSymbol = 4;
constexpr uint32_t kChannelShortened = 0x80000000u; // ChannelArgs::other: the column is shortened (else it gets +0.0)
struct ChannelArgs
{
    uint32_t nc, nct;
    uint32_t symbols;         // S = ceil(nct / m)
    uint32_t blocks;          // ceil(S / 4): the lanes of a frame that own a Philox block
    uint32_t n_other;         // columns the channel does not write
    uint32_t work;            // blocks + n_other: lanes per frame
    const int *bit_pos;       // [nct] transmitted index -> column
    const uint32_t *other;    // [n_other] column | kChannelShortened
    const double *level;      // [2^m] the constellation, m >= 2 only (built on the host)
    const void *codeword;     // [n][nc] bytes or [n][ceil(nc / 32)] words, nullptr = all zero
    int32_t codeword_format;  // BitsFormat
    int32_t channel;          // 1 AWGN, 2 BSC
    void *llr;                // [n][nc] of llr_type, or nullptr
    double *received;         // [n][S], or nullptr
    uint32_t key[2];          // Philox key (seed low, seed high)
    uint64_t frame0;          // row f is frame frame0 + f of the noise
    double sigma, sigma2;     // AWGN
    double eps, delta;        // BSC
    double shorten;           // the LLR of a shortened column: 99999.9 / delta
    double inv;               // kLlrI8: fl(1 / step)
    int32_t qmax;             // kLlrI8: 2^(q_bits - 1) - 1
    int32_t pad;
    uint64_t n;               // n * work < 2^31
};
int launch_channel(const ChannelArgs &a, int bits_per_symbol, int llr_type, void *stream);

// ---- erasure channel and genie-free erasure decoder for frames of bits (kernels_erasure.hip; include/ldpc_amd.h,
// ldpc_hip_erasure_channel_batch / ldpc_hip_erasure_decode_batch).  Rows are packed as hard_bits is ----
// the channel: one lane owns one output word (32 columns) of one frame and writes it once; col_tx says what each column is
constexpr uint32_t kErasureColErased = 0xFFFFFFFFu; // punctured: always erased
constexpr uint32_t kErasureColKnown = 0xFFFFFFFEu;  // neither transmitted nor punctured: carries the codeword's bit
constexpr uint32_t kErasureColPad = 0xFFFFFFFDu;    // beyond nc: both output bits 0
struct ErasureChannelArgs
{
    uint32_t nc, words;       // words = ceil(nc / 32)
    const uint32_t *col_tx;   // [32][words]: column 32 w + b at [b * words + w]: its index among the transmitted bits, or one of the three marks
    const void *codeword;     // [n][nc] bytes or [n][words] words, nullptr = all zero
    int32_t codeword_format;  // BitsFormat
    int32_t pad;
    uint32_t *word_bits;      // [n][words] or nullptr
    uint32_t *erased_bits;    // [n][words] or nullptr
    uint32_t key[2];          // Philox key (seed low, seed high)
    uint64_t frame0;          // row f is frame frame0 + f of the noise
    double eps;
    uint64_t n;               // n * words < 2^31
};
int launch_erasure_channel(const ErasureChannelArgs &a, void *stream);
// the decoder: one workgroup of kErasureThreads decodes kErasureFrames consecutive frames, bit f of every LDS word is frame f.
// The graph as work for whole waves, built once per context (engine.cpp, erasure_tables): a CHUNK is 64 lanes' worth of nodes
// and `trips` entries per lane, entry j of lane l at entries[offset + 64 j + l] (adjacent lanes read adjacent indices); a
// lane with fewer edges is padded with the index of a word that is always zero (column nc / check node mc).
//   check-node chunks   64 check nodes (sorted by degree; which check node a lane holds does not matter to any output), the
//                       entries are columns;
//   column chunks       64 columns of degree < kErasureWideDegree, or 16 columns of degree >= kErasureWideDegree on four lanes
//                       each (lane 4 i + s takes the edges s, s + 4, ...), the entries are check-node slots; vn_col names the
//                       lane's column (nc = none).  Every column 0..nc-1 is named by exactly one lane with s == 0.
// desc[2 k], desc[2 k + 1] = {offset, trips | kErasureWideChunk} of chunk k, the check-node chunks first
constexpr int kErasureFrames = 32, kErasureThreads = 512, kErasureWideDegree = 8;
constexpr uint32_t kErasureWideChunk = 0x80000000u;
constexpr uint32_t kErasureVoteWords = 36; // still[2], changed[2], unresolved counts[32]
// LDS of one group (include/ldpc_amd.h, ldpc_hip_erasure_lds_bytes): E[nc + 1] V[nc + 1] (the last word of each the zero
// word), ONE[mc + 1] VAL[mc + 1] (likewise), the chunk descriptors and the votes
constexpr size_t erasure_lds_bytes(size_t nc, size_t mc, size_t chunks)
{
    return (4 * (2 * (nc + 1) + 2 * (mc + 1)) + 8 * chunks + 4 * kErasureVoteWords + 15) / 16 * 16;
}
enum ErasureFlags : int
{
    kErasureEarlyTerm = 1,
    kErasureStopStalled = 2,
};
struct ErasureDecodeArgs
{
    uint32_t nc, mc, words;      // words = ceil(nc / 32)
    uint32_t cn_chunks, vn_chunks;
    uint32_t iterations;
    int32_t flags;               // ErasureFlags
    uint32_t lds_bytes;          // erasure_lds_bytes(nc, mc, cn_chunks + vn_chunks)
    const uint32_t *desc;        // [2 (cn_chunks + vn_chunks)]
    const uint16_t *cn_entries;  // columns, <= nc
    const uint16_t *vn_entries;  // check-node slots, <= mc
    const uint16_t *vn_col;      // [64 vn_chunks]
    const uint32_t *word;        // [n][words]
    const uint32_t *erased;      // [n][words]
    uint32_t *word_out;          // [n][words] or nullptr
    uint32_t *erased_out;        // [n][words] or nullptr
    uint32_t *iters;             // [n] or nullptr
    uint32_t *unresolved;        // [n] or nullptr
    uint64_t n;                  // at most 2^31 - 1 groups
};
int launch_erasure_decode(const ErasureDecodeArgs &a, void *stream);

// ---- maximum-likelihood erasure decoding of frames of bits (kernels_erasure_solve.hip; include/ldpc_amd.h,
// ldpc_hip_erasure_solve_batch): one workgroup eliminates one frame's system over GF(2), all of it in LDS ----
// A row of the augmented matrix is `stride` 64-bit words: bit j < |E| = unknown j (the erased columns in column order), bit
// |E| = the right-hand side.  stride = ceil((cap + 1) / 64) made odd: a thread walks one row, and the rows of 32 adjacent
// threads then start on 32 different pairs of banks for the 8-byte reads and on 16 for each 16-lane group of the 8-byte
// writes.  A frame uses the stride of its own |E|, never more.  `rows` bounds the check nodes that list an erased column.
constexpr uint32_t kErasureSolveMaxThreads = 1024, kErasureSolveScalars = 16, kErasureSolveRowsPerThread = 32;
constexpr uint32_t kErasureSolved = 0, kErasurePartial = 1, kErasureInconsistent = 2, kErasureTooLarge = 3;
constexpr size_t erasure_solve_stride(size_t cap) { return ((cap + 1 + 63) / 64) | 1; }
constexpr size_t erasure_solve_rows(size_t mc, size_t cap, size_t max_column_degree) { return mc < cap * max_column_degree ? mc : cap * max_column_degree; }
// LDS of one frame (include/ldpc_amd.h, ldpc_hip_erasure_solve_lds_bytes): the matrix; per 64 check nodes the mask of those
// with an erased column and their count so far; E, V and the unknowns in front of each word of E; the column of every
// unknown; the votes
constexpr size_t erasure_solve_lds_bytes(size_t nc, size_t mc, size_t cap, size_t rows)
{
    return (8 * rows * erasure_solve_stride(cap) + 12 * ((mc + 63) / 64) + 4 * (3 * ((nc + 31) / 32) + 1) + 4 * cap + 4 * kErasureSolveScalars + 15) / 16 * 16;
}
struct ErasureSolveArgs
{
    uint32_t nc, mc, words;   // words = ceil(nc / 32)
    uint32_t cap;             // 1 <= cap <= nc: a frame with more erased columns is returned as it came
    uint32_t rows;            // erasure_solve_rows(mc, cap, largest column degree)
    uint32_t threads;         // a multiple of 64, <= kErasureSolveMaxThreads, rows <= kErasureSolveRowsPerThread * threads
    uint32_t lds_bytes;       // erasure_solve_lds_bytes(nc, mc, cap, rows)
    const uint32_t *row_ptr;  // [mc + 1]: the rows of H as the library loaded it, repeated entries included
    const uint32_t *row_col;  // columns, < nc
    const uint32_t *word;     // [n][words]
    const uint32_t *erased;   // [n][words]
    uint32_t *word_out;       // [n][words] or nullptr
    uint32_t *erased_out;     // [n][words] or nullptr
    uint32_t *unresolved;     // [n] or nullptr
    uint32_t *rank;           // [n] or nullptr
    uint32_t *status;         // [n] or nullptr
    uint64_t n;               // < 2^31
};
int launch_erasure_solve(const ErasureSolveArgs &a, void *stream);

// ---- ordered-statistics decoding of frames of LLRs (kernels_osd.hip; include/ldpc_amd.h, ldpc_hip_osd_batch): one
// workgroup reduces one frame's whole check matrix over GF(2) in LDS, in the order of the frame's reliabilities ----
// A row is `stride` 64-bit words: bit c of the first ceil(nc / 64) = the entry of column c, then at least one word beside
// them, which after the elimination holds what the candidate search reads of the row's pivot column (its reliability, its
// index, whether order 0 flips it).  stride = (ceil(nc / 64) + 1) made odd, for the banks (erasure_solve_stride).
constexpr uint32_t kOsdMaxThreads = 1024, kOsdRowsPerThread = 32, kOsdSideBytes = 384;
constexpr uint32_t kOsdCodeword = 0, kOsdOrder0 = 1, kOsdReprocessed = 2, kOsdNoColumn = 0xFFFFFFFFu, kOsdQMax = 0x7FFFFFFFu;
constexpr size_t osd_row_words(size_t nc) { return (nc + 63) / 64; }
constexpr size_t osd_stride(size_t nc) { return (osd_row_words(nc) + 1) | 1; }
// the region the matrix shares with the sort keys (4 bytes a column, gone before the matrix is built)
constexpr size_t osd_matrix_bytes(size_t nc, size_t mc)
{
    return 8 * mc * osd_stride(nc) > (4 * nc + 7) / 8 * 8 ? 8 * mc * osd_stride(nc) : (4 * nc + 7) / 8 * 8;
}
// LDS of one frame (include/ldpc_amd.h, ldpc_hip_osd_lds_bytes): the matrix; the decisions z, the solved set P and the word
// being built as masks over the columns; the order (16 bits a column); votes, sums and one best candidate per wave
constexpr size_t osd_lds_bytes(size_t nc, size_t mc)
{
    return (osd_matrix_bytes(nc, mc) + 24 * osd_row_words(nc) + (2 * nc + 7) / 8 * 8 + kOsdSideBytes + 15) / 16 * 16;
}
struct OsdArgs
{
    uint32_t nc, mc, words;  // words = ceil(nc / 32); nc < 65536
    uint32_t candidates;     // order-1 candidates tried (the first of K in the order; more than |K| counts as |K|)
    uint32_t threads;        // a multiple of 64, <= kOsdMaxThreads, mc <= kOsdRowsPerThread * threads
    uint32_t lds_bytes;      // osd_lds_bytes(nc, mc)
    int32_t llr_type;        // LlrType: the kernel reads the elements in place
    const uint32_t *row_ptr; // [mc + 1]: the rows of H as the library loaded it, repeated entries included
    const uint32_t *row_col; // columns, < nc
    const void *llr;         // [n][nc] elements of llr_type
    uint32_t *word_out;      // [n][words] or nullptr
    uint32_t *flips;         // [n] or nullptr
    uint64_t *metric;        // [n] or nullptr
    uint32_t *flipped_column; // [n] or nullptr
    uint32_t *status;        // [n] or nullptr
    uint64_t n;              // <= 2^20
};
int launch_osd(const OsdArgs &a, void *stream);

// ---- ordered-statistics decoding toward a given syndrome, with a bounded order-2 sweep (kernels_osd_syndrome.hip;
// include/ldpc_amd.h, ldpc_hip_osd_syndrome_batch): the layout of osd_kernel, and bit 63 of a row's side word is the row's
// right-hand side (s + M z, eliminated along with the row) ----
constexpr uint32_t kOsdReprocessedPair = 3, kOsdInfeasible = 4, kOsdMaxPairDepth = 256;
// beside the order: 8 bytes of metric(x0), per wave (16 of them) its best metric (8 bytes) and that candidate's index and its
// two places in K (4 bytes each), 16 32-bit scalars = 392 bytes, rounded to 512; then the reliabilities of the first
// kOsdMaxPairDepth columns of K (4 bytes each)
constexpr uint32_t kOsdSyndromeSideBytes = 512 + 4 * kOsdMaxPairDepth;
constexpr size_t osd_syndrome_lds_bytes(size_t nc, size_t mc)
{
    return (osd_matrix_bytes(nc, mc) + 24 * osd_row_words(nc) + (2 * nc + 7) / 8 * 8 + kOsdSyndromeSideBytes + 15) / 16 * 16;
}
struct OsdSyndromeArgs
{
    uint32_t nc, mc, words;   // words = ceil(nc / 32); nc < 65536
    uint32_t syn_words;       // ceil(mc / 32)
    uint32_t candidates;      // single flips tried (the first of K in the order; more than |K| counts as |K|)
    uint32_t pair_depth;      // <= kOsdMaxPairDepth: every pair among the first min(pair_depth, |K|) of K is tried
    uint32_t threads;         // a multiple of 64, <= kOsdMaxThreads, mc <= kOsdRowsPerThread * threads
    uint32_t lds_bytes;       // osd_syndrome_lds_bytes(nc, mc)
    int32_t llr_type;         // LlrType: the kernel reads the elements in place
    int32_t syndrome_format;  // BitsFormat of `syndrome`
    const uint32_t *row_ptr;  // [mc + 1]: the rows of H as the library loaded it, repeated entries included
    const uint32_t *row_col;  // columns, < nc
    const void *llr;          // [n][nc] elements of llr_type
    const void *syndrome;     // [n][mc] bytes or [n][syn_words] words, bit r = row r; nullptr = all zero
    uint32_t *word_out;       // [n][words] or nullptr
    uint32_t *flips;          // [n] or nullptr
    uint64_t *metric;         // [n] or nullptr
    uint32_t *flipped_columns; // [n][2] or nullptr
    uint32_t *status;         // [n] or nullptr
    uint64_t n;               // <= 2^20
};
int launch_osd_syndrome(const OsdSyndromeArgs &a, void *stream);

// ---- quantized min-sum decoding toward a given syndrome (kernels_syndrome_decode.hip; include/ldpc_amd.h,
// ldpc_hip_syndrome_decode_batch): one workgroup per frame on the tables of DevQmsPlan, the typed LLRs read in place ----
// LDS of one frame (include/ldpc_amd.h, ldpc_hip_syndrome_decode_lds_bytes), every part rounded up to 16 bytes: the messages
// (a byte each, `slots`), the 32-bit totals, the 128-byte table and 32 bytes of votes and partial sums, the syndrome (a bit
// per check node, in the order the kernel walks them), the quantized inputs (a byte each)
constexpr size_t syndrome_decode_round16(size_t x) { return (x + 15) & ~size_t(15); }
constexpr size_t kSyndromeDecodeSideBytes = 160;
constexpr size_t syndrome_decode_lds_bytes(size_t slots, size_t nc, size_t mc)
{
    return syndrome_decode_round16(slots) + syndrome_decode_round16(4 * nc) + kSyndromeDecodeSideBytes +
           syndrome_decode_round16(4 * ((mc + 31) / 32)) + syndrome_decode_round16(nc);
}
struct SyndromeDecodeArgs
{
    uint32_t nc, mc;
    uint32_t words, syn_words;  // ceil(nc / 32), ceil(mc / 32)
    uint32_t iterations;
    int32_t early_term;
    int32_t llr_type;           // LlrType: the kernel reads the elements in place
    int32_t syndrome_format;    // BitsFormat (not read where syndrome is null)
    int32_t shared_llr;         // llr is one row [nc] for every frame
    int32_t qmax;               // 2^(q_bits - 1) - 1, 1..127
    double step, inv;           // the LLR step and fl(1 / step)
    uint32_t lut[32];           // lut[m], m = 0..qmax, four per word (engine.cpp, correction_lut)
    uint32_t lds_bytes;         // syndrome_decode_lds_bytes(slots, nc, mc)
    const uint32_t *col_rank;   // [nc] column -> VN rank (DevPlan)
    const uint32_t *cn_row;     // [mc] check node in the tables' order -> row of H in file order (Plan::cn_rank_row)
    const void *llr;            // [n][nc] (or [nc]) elements of llr_type, column order
    const void *syndrome;       // [n][mc] bytes or [n][syn_words] words, row order; nullptr = all zero
    uint32_t *hard_bits;        // [n][words] or nullptr
    uint32_t *iters;            // [n] or nullptr
    uint32_t *weight;           // [n] or nullptr
    double *llr_out;            // [n][nc] or nullptr
    uint64_t n;                 // <= 2^20
};
int launch_syndrome_decode(const SyndromeDecodeArgs &a, const DevQmsPlan &Q, void *stream);

// ---- fixed-point layered min-sum decoding toward a given syndrome (kernels_syndrome_decode_layered.hip; include/ldpc_amd.h,
// ldpc_hip_syndrome_decode_layered_batch): one wave per frame on the tables of DevLayerPlan, the typed LLRs read in place.
// LDS of one frame: plan.hpp, layered_fixed_direct_region_bytes — the syndrome bit of a check node is bit 31 of its record ----
constexpr uint32_t kSdlSyndromeBit = 0x80000000u;
struct SyndromeDecodeLayeredArgs
{
    uint32_t nc, mc;
    uint32_t words, syn_words;  // ceil(nc / 32), ceil(mc / 32)
    uint32_t iterations;
    int32_t early_term;
    int32_t llr_type;           // LlrType: the kernel reads the elements in place
    int32_t syndrome_format;    // BitsFormat (not read where syndrome is null)
    int32_t shared_llr;         // llr is one row [nc] for every frame
    uint32_t lds_bytes;         // layered_fixed_direct_region_bytes(record slots, nc)
    LayeredFixedArgs q;         // the quantizer, the two limits, the correction table
    const uint32_t *col_rank;   // [nc] column -> VN rank (DevPlan)
    const uint32_t *step_row;   // [n_steps][64]: the row of H in file order of the step's lane-th check node (lanes >= count: 0)
    const void *llr;            // [n][nc] (or [nc]) elements of llr_type, column order
    const void *syndrome;       // [n][mc] bytes or [n][syn_words] words, row order; nullptr = all zero
    uint32_t *hard_bits;        // [n][words] or nullptr
    uint32_t *iters;            // [n] or nullptr
    uint32_t *weight;           // [n] or nullptr
    double *llr_out;            // [n][nc] or nullptr
    uint64_t n;                 // <= 2^20
};
int launch_syndrome_decode_layered(const SyndromeDecodeLayeredArgs &a, const DevLayerPlan &L, void *stream);

// ---- gradient-descent bit flipping toward a given syndrome (kernels_bit_flip.hip; include/ldpc_amd.h,
// ldpc_hip_bit_flip_batch): one wave per frame, several frames to a workgroup, on the two adjacency tables of H in file
// order (u16 indices), the typed LLRs read in place ----
// LDS of one frame (include/ldpc_amd.h, ldpc_hip_bit_flip_lds_bytes), every part rounded up to 16 bytes: the quantized
// inputs (a byte each: sign = y, magnitude = r), the word x (a bit per column), the unmet checks u (a bit per check node)
// twice: the round's and the next round's
constexpr size_t bit_flip_round16(size_t x) { return (x + 15) & ~size_t(15); }
constexpr size_t bit_flip_lds_bytes(size_t nc, size_t mc)
{
    return bit_flip_round16(nc) + bit_flip_round16(4 * ((nc + 31) / 32)) + 2 * bit_flip_round16(4 * ((mc + 31) / 32));
}
constexpr uint32_t kBitFlipMaxFrames = 4; // frames (waves) of a workgroup at most
// frames of a workgroup: as many as kBitFlipMaxFrames whose LDS stays within a quarter of the CU's, one at least
constexpr uint32_t bit_flip_group_frames(size_t frame_bytes)
{
    const size_t fit = (160 * 1024 / 4) / (frame_bytes ? frame_bytes : 1);
    return fit >= kBitFlipMaxFrames ? kBitFlipMaxFrames : (fit >= 1 ? static_cast<uint32_t>(fit) : 1u);
}
constexpr uint32_t kBitFlipEveryCandidate = 0xFFFFFFFFu; // flip_threshold: no draws
struct BitFlipArgs
{
    uint32_t nc, mc;            // both 1..65535
    uint32_t words, syn_words;  // ceil(nc / 32), ceil(mc / 32)
    uint32_t iterations;        // <= 65535
    int32_t llr_type;           // LlrType: the kernel reads the elements in place
    int32_t syndrome_format;    // BitsFormat (not read where syndrome is null)
    int32_t shared_llr;         // llr is one row [nc] for every frame
    int32_t qmax;               // 2^(q_bits - 1) - 1, 1..127
    double inv;                 // fl(1 / step)
    int32_t check_weight;       // w, 1..255
    int32_t margin;             // 0..65535
    uint32_t flip_threshold;    // kBitFlipEveryCandidate, or a candidate flips iff its draw is below
    uint32_t k0, k1;            // the Philox key: seed & 0xFFFFFFFF, seed >> 32
    uint64_t first_frame;       // frame f draws as frame first_frame + f
    uint32_t draw_blocks;       // ceil(nc / 4): the Philox blocks of one round
    uint32_t frame_bytes;       // bit_flip_lds_bytes(nc, mc)
    uint32_t group_frames;      // bit_flip_group_frames(frame_bytes)
    const uint32_t *row_ptr;    // [mc + 1]: the rows of H in file order, repeated entries included
    const uint16_t *row_col;    // columns, < nc
    const uint32_t *col_ptr;    // [nc + 1]: the columns of H, the entries of each in file order
    const uint16_t *col_row;    // rows, < mc
    const void *llr;            // [n][nc] (or [nc]) elements of llr_type, column order
    const void *syndrome;       // [n][mc] bytes or [n][syn_words] words, row order; nullptr = all zero
    uint32_t *hard_bits;        // [n][words] or nullptr
    uint32_t *iters;            // [n] or nullptr
    uint32_t *weight;           // [n] or nullptr
    uint64_t n;                 // <= 2^20
};
int launch_bit_flip(const BitFlipArgs &a, void *stream);

// ---- min-sum with memory, run as a relay of legs, toward a given syndrome (kernels_relay_decode.hip; include/ldpc_amd.h,
// ldpc_hip_relay_decode_batch): the iteration of kernels_syndrome_decode.hip on the tables of DevQmsPlan with a memory term
// per column and leg, the cheapest word that met the syndrome kept.  One body in two forms: a workgroup of 256 threads per
// frame, or a wave per frame and four frames to a workgroup ----
// LDS of one frame (include/ldpc_amd.h, ldpc_hip_relay_decode_lds_bytes): the frame of syndrome_decode_lds_bytes and the kept
// word, a bit per column.  The cost's reduction takes the four partial sums that frame already holds: no byte more
constexpr size_t relay_decode_lds_bytes(size_t slots, size_t nc, size_t mc)
{
    return syndrome_decode_lds_bytes(slots, nc, mc) + syndrome_decode_round16(4 * ((nc + 31) / 32));
}
constexpr uint32_t kRelayWaveFrames = 4;          // form 2: frames (waves) of a workgroup
constexpr uint32_t kRelayNone = 0xFFFFFFFFu;      // best_leg and cost of a frame without a solution
enum RelayForm : int32_t
{
    kRelayFormGroup = 1, // 256 threads share a frame
    kRelayFormWave = 2   // 64 threads share a frame
};
struct RelayDecodeArgs
{
    uint32_t nc, mc;
    uint32_t words, syn_words;  // ceil(nc / 32), ceil(mc / 32)
    uint32_t legs;              // 1..256
    uint32_t first_iterations, leg_iterations; // 1..65535
    uint32_t stop_after;        // 1..legs
    int32_t form;               // RelayForm
    int32_t llr_type;           // LlrType: the kernel reads the elements in place
    int32_t syndrome_format;    // BitsFormat (not read where syndrome is null)
    int32_t shared_llr;         // llr is one row [nc] for every frame
    int32_t qmax;               // 2^(q_bits - 1) - 1, 1..127
    double inv;                 // fl(1 / step)
    uint32_t lut[32];           // lut[m], m = 0..qmax, four per word (engine.cpp, correction_lut)
    uint32_t frame_bytes;       // relay_decode_lds_bytes(slots, nc, mc)
    const uint32_t *col_rank;   // [nc] column -> VN rank (DevPlan)
    const uint32_t *rank_col;   // [nc] VN rank -> column (DevPlan): gamma is read by rank
    const uint32_t *cn_row;     // [mc] check node in the tables' order -> row of H in file order (Plan::cn_rank_row)
    const void *llr;            // [n][nc] (or [nc]) elements of llr_type, column order
    const void *syndrome;       // [n][mc] bytes or [n][syn_words] words, row order; nullptr = all zero
    const int8_t *gamma;        // [legs][nc], column order, in 64ths; nullptr = all zero
    uint32_t *hard_bits;        // [n][words] or nullptr
    uint32_t *iters;            // [n] or nullptr
    uint32_t *weight;           // [n] or nullptr
    uint32_t *solutions;        // [n] or nullptr
    uint32_t *best_leg;         // [n] or nullptr
    uint32_t *cost;             // [n] or nullptr
    uint64_t n;                 // <= 2^20
};
int launch_relay_decode(const RelayDecodeArgs &a, const DevQmsPlan &Q, void *stream);

// opt-in non-parity ternary min-sum, bit-sliced over 32 frames per workgroup (kernels_ternary.hip; include/ldpc_amd.h,
// ldpc_hip_set_min_sum_ternary) on the general plan.  a.ms_* are not read.  With a.llr_out null the planes of A are left out
// of the group's LDS (plan.hpp, ternary_lds_bytes)
struct TernaryArgs
{
    int32_t weight; // w of A = w r + the sum of the inputs, 1..7
    int32_t planes; // plan.hpp, ternary_planes(max_vn_degree)
};
int launch_decode_ternary(const DecodeArgs &a, const TernaryArgs &t, void *stream);

// ---- mt19937_64 on the device ----
constexpr int kMtN = 312;
constexpr uint32_t kBlockTrials = kMtN / 2; // one twist block of 312 words = 156 polar trials
// Chunk start states live in a RING of ring_rows rows of 312 words: chunk i of a launch starts from row
// (first_row + i) % ring_rows (first_row < ring_rows, n <= ring_rows).
// Raw (tempered) outputs: chunk i writes out[i * chunk_words ..), chunk_words a multiple of 312; the LAST chunk of the
// launch generates last_words <= chunk_words only (a prefix, in the same launch).  pack: chunks per workgroup (1, or 4 to
// keep the generator on a quarter of the compute units beside decode kernels that own a whole CU).
int launch_mt_generate(const uint64_t *ring, uint32_t ring_rows, uint32_t first_row, uint64_t *out, uint32_t n_chunks,
                       uint32_t chunk_words, uint32_t last_words, int pack, void *stream);
// Jump: row (dst_first + t) % ring_rows = row (src_first + t) % ring_rows advanced by the polynomial `poly` (19937
// coefficient bits, kJumpPolyWords words: 312 + zero padding), t < n_tasks.  A task reads its source row before it writes,
// so src_first == dst_first (in place) is allowed; otherwise the two row ranges must not overlap.
// groups: 4 = one task per workgroup, its taps shared by four thread groups (a short chain: where the jump is on the critical
// path or holds a CU a decoder wants); else one group, one task per workgroup — rng_kernels.hip says which where.
int launch_mt_jump(uint64_t *ring, uint32_t ring_rows, uint32_t src_first, uint32_t dst_first, const uint64_t *poly,
                   uint32_t n_tasks, int groups, void *stream);
constexpr uint32_t kJumpPolyWords = 320;

// The AWGN noise generator: chunks of the raw stream -> the normal variates the reference's normal_distribution would
// return (libstdc++ polar method).  Two launches: mt_generate writes the chunks' raw words, polar_slab_kernel
// reads them ONCE — acceptance test of every trial (raw words 2t, 2t+1), and for each accepted trial its two normals
// y*mult, x*mult, compacted in stream order into the chunk's SLAB (the workgroups of a chunk, 2048 trials each, chain
// their counts by decoupled look-back: no separate counting pass, no global prefix sum between the test and the
// compaction).  counts[i] = accepted trials of chunk i.
struct NormalsArgs
{
    const uint64_t *ring;
    uint32_t ring_rows, first_row;
    uint32_t n_chunks;
    uint32_t blocks;      // twist blocks (312 words = 156 trials each) a chunk holds
    uint32_t last_blocks; // ... and how many of them the launch's LAST chunk generates (a prefix; == blocks: all of it)
    int pack;             // generator: chunks per workgroup (launch_mt_generate)
    uint64_t *raw;        // scratch: n_chunks * 312 * blocks words
    uint64_t *lookback;   // scratch: n_chunks * (ceil(156 * blocks / kSlabBlock) + 1) words (zeroed by the launcher)
    uint64_t *slabs;      // chunk i writes slabs[i * slab_words ..): 2 words per accepted pair
    uint64_t slab_words;
    uint32_t *counts;     // [n_chunks]
    int write_normals;    // 0: count only (stream_skip, locate)
    // locate: in chunk locate_chunk (index in this launch; 0xFFFFFFFF = none) the chunk-local trial index of the accepted
    // pair with chunk-local rank locate_rank (0xFFFFFFFF = the chunk's last accepted pair) is written to *locate_out
    uint32_t locate_chunk, locate_rank;
    uint64_t *locate_out;
};
constexpr uint32_t kSlabBlock = 2048; // trials per workgroup of the slab kernel
inline uint64_t normals_lookback_words(uint32_t n_chunks, uint32_t blocks)
{
    return static_cast<uint64_t>(n_chunks) * ((static_cast<uint64_t>(kBlockTrials) * blocks + kSlabBlock - 1) / kSlabBlock + 1);
}
int launch_mt_normals(const NormalsArgs &a, void *stream);

// One small launch after the generator: cum[0..n] = exclusive prefix sums of counts[0..n) (the decode kernels' slab
// table), and where the consumer stands afterwards.
struct NormalsResult
{
    uint64_t total;      // cum[n]
    uint64_t piece;      // cum[n_piece] (sharded stream: accepted pairs of the rank's piece, without the margin chunk)
    uint64_t next_k;     // ... at this chunk-local pair index
    uint32_t next_slab;  // the pair with list index `target` sits in this slab ...
    uint32_t enough;     // total >= need
};
// target: list index (over the concatenated slabs) of the first pair the consumer has NOT used; n_full: leading chunks that
// were generated to full length (n or n - 1).  When target lies beyond everything generated, the position is
// (n, target - total) if the last chunk is complete and (n - 1, target - cum[n-1]) if it is a prefix that can be extended.
int launch_normals_finish(const uint32_t *counts, uint32_t n, uint32_t n_piece, uint32_t n_full, uint64_t need, uint64_t target,
                          uint64_t *cum, NormalsResult *result, void *stream);

// GF(2) encoding on the reference's info-word stream (channel.cpp:44-60, sparse.h:163-172); sim_kernels.hip.
// The reference draws kc bernoulli(0.5) bits per frame from mt19937_64(seed << 1) and ACCUMULATES u*G
// into the codeword it never clears, so the codeword of frame f is cw_prev ^ (u_0 ^ ... ^ u_f) G:
//   encode_info_kernel   info bit i of frame f = canonical(info_raw[f*kc + i]) < 0.5, packed 64 per word
//   encode_prefix_kernel running XOR of the packed info words over the frames of the batch
//   encode_cw_kernel     codeword[f][j] = cw_prev[j] ^ parity of (prefix_f AND column j of G)
struct EncodeArgs
{
    int nc, kc, words;         // words = ceil(kc/64)
    const uint32_t *g_col_ptr; // [g_cols+1] CSC of G (row indices per column)
    const uint32_t *g_col_row; // [g_nnz]
    int g_cols;
    const uint64_t *info_raw;  // [n_frames][kc]
    uint64_t *prefix;          // [n_frames][words] scratch / result
    const uint8_t *cw_prev;    // [nc]
    uint8_t *codeword;         // [n_frames][nc], may be nullptr (skip: only cw_last is wanted)
    uint8_t *cw_last;          // [nc] codeword after the batch
    uint64_t n_frames;
    // sharded encoding: XOR of the info words of the step's frames before this rank's (0 for a whole stream): joins every
    // prefix of the batch (the codeword accumulates linearly over the frames: channel.cpp:44-60, sparse.h:163-172)
    const uint64_t *base;      // [words] device, or nullptr
    // the columns of G as bit masks over the info word, [nc][words] (zero rows beyond g_cols), or nullptr: with them and
    // words <= 4 a codeword bit is a handful of AND / popcount instead of a walk over the column's entries
    const uint64_t *g_mask;
};
int launch_encode(const EncodeArgs &a, void *stream);
// the two halves of launch_encode by themselves (sharded encoding): info words + their running XOR over the batch; the
// codewords of the batch (only_last: just cw_last, from the batch's last prefix)
int launch_encode_prefix(const EncodeArgs &a, void *stream);
int launch_encode_codewords(const EncodeArgs &a, void *stream, bool only_last);

// ---- counter-based noise (device_philox.hpp, counter_kernels.hip) ----
// raw Philox4x32-10 words of blocks [first_block, first_block + n_blocks) of `frame` under `tag`: out[4 i + k] = word k of
// block first_block + i (device pointer)
int launch_philox(uint64_t seed, uint32_t tag, uint64_t frame, uint32_t first_block, uint64_t n_blocks, uint32_t *out, void *stream);
// the info words of frames [frame0, frame0 + n) in counter mode, packed as EncodeArgs::prefix expects them: prefix[f][w] =
// info bits 64 w .. 64 w + 63 of frame frame0 + f (bits from kc on zero)
int launch_encode_info_counter(uint64_t seed, uint64_t frame0, uint64_t n, int kc, int words, uint64_t *prefix, void *stream);

// {frames, frame errors, bit errors, iterations, early stops} of a batch (all device pointers), one launch (sim_kernels.hip)
int launch_batch_counters(const uint32_t *iters, const uint32_t *bit_errors, uint64_t n, uint32_t max_iters, int early_term,
                          long long *counters, void *stream);

// selftest.hip: dm_ratio_div vs the IEEE division on n pseudo-random operand pairs; *mismatches (device, zeroed by the caller)
int launch_division_selftest(uint64_t n, uint64_t seed, unsigned long long *mismatches, void *stream);

// functions of detmath.h / device_cn.hpp evaluated element by element (include/ldpc_amd.h: ldpc_hip_selftest_math)
enum MathFn : int
{
    kMathExp = 0,       // dm_exp(a)
    kMathLog,           // dm_log(a)
    kMathBoxplus,       // dm_boxplus(a, b)
    kMathRatioDiv,      // dm_ratio_div(a, b)
    kMathRatioRho,      // dm_ratio_rho(a, b)
    kMathRatioLambda,   // dm_ratio_lambda(a, b)
    kMathECombine,      // dm_e_combine(a, b)
    kMathExpClamped,    // dm_exp_clamped(a)
    kMathBoxplusExp,    // dm_boxplus_exp(a)
    kMathBoxplusLog,    // dm_boxplus_log(a)
    kMathCnRatio3,      // cn_ratio<3> on rows a[i][3] -> out[i][3]
    kMathCnRatio4,
    kMathCnRatio5,
    kMathCnRatio6,
    kMathCnRatio8,
    kMathCnLlr4,        // cn_core<4, sum-product> (LLR domain, E-form recursion)
    kMathCnLlr6,
    kMathCnRatio3s,     // dm_cn3_shared / dm_cn4_shared: the shared-reciprocal forms
    kMathCnRatio4s,
    kMathCnRatio6s,     // dm_cn6_shared: degree 6, two reciprocals
    // the fused form's check nodes (detmath.h "Fused form"), one row per node: a[i] = {v_0 .. v_{D-1}, flip | leaf << 4, 0},
    // out[i] = {m_0 .. m_{D-1}, leaf_bit, leaf_tot}; leaf_tot NaN without a leaf, the whole row NaN where the upper word the
    // node returns reaches DM_FUSED_P_HI
    kMathCnf2,          // dm_cnf2
    kMathCnf3,          // dm_cnf3, shared = 1 (early termination)
    kMathCnf4,          // dm_cnf4, shared = 1
    kMathCnf3d,         // dm_cnf3, shared = 0 (hand-over form: every output divided on its own)
    kMathCnf4d,         // dm_cnf4, shared = 0
    kMathCnLlr3,        // cn_core<3 / 5 / 16, sum-product>
    kMathCnLlr5,
    kMathCnLlr16,
    kMathPredicates,    // the range predicates of detmath.h on a, as a bit mask (selftest.hip: predicate_mask)
    kMathCount
};
int math_selftest_width(int fn); // values per element in a / out (0 = unknown function)
int launch_math_selftest(int fn, uint64_t n, const double *a, const double *b, double *out, void *stream);

} // namespace ldpc_amd
