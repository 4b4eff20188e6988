// engine.hpp — host runtime around the HIP kernels: device tables, workspaces, the mt19937_64
// stream engine and the batched channel+decode step.  One Engine per (code, GPU).
//
// This is the native replacement for the reference's per-thread `channel` objects
// (src/sim/channel.h:7-252) driven frame by frame from ldpc_sim::start (src/sim/ldpcsim.cpp:158-188):
// instead of five virtual calls per frame, one call decodes a batch of frames of the same stream.
#pragma once

#include <cstdint>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "code.hpp"
#include "comm.hpp"
#include "kernels.hpp"
#include "mt64.hpp"
#include "mtstates.hpp"
#include "plan.hpp"

namespace ldpc_amd
{

enum ChannelType : int
{
    kAwgn = 1, // same numbering as the reference's channel_type enum (ldpcsim.h:15-20)
    kBsc = 2,
    kBec = 3
};

struct DecParams
{
    bool early_term = true;
    uint32_t iterations = 50;
    bool min_sum = false;
};

// Output buffers of a batch; device or host pointers, nullptr = not wanted.
struct BatchOut
{
    uint32_t *iters = nullptr;      // [n]
    uint32_t *bit_errors = nullptr; // [n]
    uint8_t *hard = nullptr;        // [n][nc]
    double *llr_out = nullptr;      // [n][nc] (BEC: symbol values widened to double)
    double *llr_in = nullptr;       // [n][nc]
    uint8_t *codeword = nullptr;    // [n][nc]
    // the same outputs from frame `frame` of the batch on (a sub-batch)
    BatchOut at(uint64_t frame, uint64_t nc) const
    {
        BatchOut o = *this;
        if (o.iters) o.iters += frame;
        if (o.bit_errors) o.bit_errors += frame;
        if (o.hard) o.hard += frame * nc;
        if (o.llr_out) o.llr_out += frame * nc;
        if (o.llr_in) o.llr_in += frame * nc;
        if (o.codeword) o.codeword += frame * nc;
        return o;
    }
};

// Where a frame's decoder state lives: fixed per code when the engine is built (Engine::residency)
enum class Residency : int
{
    kNone,        // no decoder instantiation takes the code (the first decode throws)
    kLds,         // LDS-resident (kernels.hip, kernels_fused.hip)
    kRegTotals,   // register-resident, totals form (kernels_reg2.hip)
    kRegMessages, // register-resident, messages form (kernels_reg.hip)
    kMemory       // messages in device memory (kernels.hip)
};

// The launches of one batch, in order (kernels.hpp, Stage).  Pure host arithmetic, no HIP: run_decode walks
// the sequence, the CPU tests read it through ldpc_hip_decode_stages.
struct StageSeq
{
    int n = 0;
    Stage s[3] = {};
};

// Which kernel family decodes a batch: the resident decoders the library picks by the code (Residency), or one of the opt-in
// NON-PARITY variants the caller switched on — flooding sum-product with binary32 messages (kernels_fast.hip), layered
// sum-product with binary32 / binary16 messages (kernels_layered.hip), layered min-sum (kernels_layered_ms.hip), quantized
// min-sum (kernels_qms.hip), ternary min-sum (kernels_ternary.hip), fixed-point layered min-sum (kernels_layered_fixed.hip).
// One value per batch: Engine::stages names its launches from it, run_decode switches on it, Engine::refusal says whether
// that decoder takes the code.
enum class Decoder : int { kResident, kFast32, kLayered32, kLayered16, kLayeredMinSum, kQuantizedMinSum, kTernary, kLayeredFixedMinSum };
// The variant of "BP_MS" decoding the caller switched on: at most one is in force (Engine::enter_ms_variant is where the
// setters agree on that), kFlooding = none of them, the resident decoder
enum class MsVariant : int { kFlooding, kLayered, kQuantized, kTernary, kLayeredFixed };
// One row per variant, in the enum's order: the decoder it selects, and what the setters' messages call it — its setter, the
// noun when it is what the caller asked for, the noun when it stands in another's way, and how to switch it off first
struct MsVariantInfo
{
    Decoder decoder;
    const char *setter, *subject, *obstacle, *off_first;
};
inline constexpr MsVariantInfo kMsVariants[] = {
    {Decoder::kResident, "", "", "", ""},
    {Decoder::kLayeredMinSum, "ldpc_hip_set_min_sum_schedule", "the layered schedule", "the layered schedule",
     "ldpc_hip_set_min_sum_schedule(ctx, LDPC_HIP_MS_SCHEDULE_FLOODING)"},
    {Decoder::kQuantizedMinSum, "ldpc_hip_set_min_sum_quantization", "quantized min-sum", "quantized min-sum",
     "ldpc_hip_set_min_sum_quantization(ctx, 0, 0)"},
    {Decoder::kTernary, "ldpc_hip_set_min_sum_ternary", "ternary min-sum", "ternary min-sum", "ldpc_hip_set_min_sum_ternary(ctx, 0)"},
    {Decoder::kLayeredFixedMinSum, "ldpc_hip_set_min_sum_layered_fixed", "fixed-point layered min-sum", "fixed-point layered min-sum",
     "ldpc_hip_set_min_sum_layered_fixed(ctx, 0, 0, 0)"},
};
constexpr const MsVariantInfo &ms_info(MsVariant v) { return kMsVariants[static_cast<int>(v)]; }
// min-sum follows its variant and ignores the fast mode; sum-product follows the fast mode alone
constexpr Decoder choose_decoder(bool min_sum, int fast_mode, MsVariant ms_variant)
{
    if (min_sum)
        return ms_info(ms_variant).decoder;
    return fast_mode == 1 ? Decoder::kFast32 : fast_mode == 2 ? Decoder::kLayered32 : fast_mode == 3 ? Decoder::kLayered16 : Decoder::kResident;
}

// shared6: not LDS-resident and a check node of degree 6; ratio_width: no check node wider than kMaxCnDegree (wider ones
// run the LLR-domain form only; the oracle applies the same rule)
struct StageQuery
{
    Residency residency;
    Decoder decoder;
    bool shared6, ratio_width, min_sum, early_term, iterations;
};
inline StageSeq decode_stages(const StageQuery &q)
{
    // every opt-in variant is one launch of its own kernel, whatever the resident decoder would take
    if (q.decoder != Decoder::kResident)
        return {1, {Stage::kWhole}};
    // Sum-product runs in likelihood-ratio form (detmath.h: no exp/log inside the iteration); the few frames whose values
    // leave the box that form can represent come back in a list and go on to the next stage.  Which form finishes a frame
    // depends on that frame's data only, never on the batch it travels in.
    if (q.min_sum || !q.iterations || !q.ratio_width || q.residency == Residency::kNone)
        return {1, {Stage::kWhole}};
    // LDS-resident: ONE more launch over the first one's list (kernels.hip, decode_kernel_list); without early termination
    // every frame still starts in the ratio form and is handed over to the LLR-domain form at an iteration boundary when
    // its totals near the edge of the box (detmath.h "Hand-over")
    if (q.residency == Residency::kLds)
        return q.early_term ? StageSeq{2, {Stage::kRatioFirst, Stage::kListChain}}
                          : StageSeq{2, {Stage::kHandoverFirst, Stage::kHandoverResume}};
    if (!q.early_term)
        return {1, {Stage::kWhole}};
    if (q.residency == Residency::kRegTotals) // the kernel chains all three forms in its workgroup: no frame is handed back
        return {1, {Stage::kRatioFirst}};
    // The first launch of a code with check nodes of degree 6 runs them with shared reciprocals (detmath.h, dm_cn6_shared),
    // whose denominator products leave their range in a few frames per ten thousand at the waterfall: those are decoded
    // again with every output divided separately, and only what leaves the box there goes on to the LLR domain.
    return q.shared6 ? StageSeq{3, {Stage::kRatioFirst, Stage::kRatioSeparate, Stage::kLlrRedo}}
                   : StageSeq{2, {Stage::kRatioFirst, Stage::kLlrRedo}};
}

struct OutStage; // engine.cpp: a batch's outputs, written directly or through staging buffers

class DeviceBuffer
{
  public:
    DeviceBuffer() = default;
    ~DeviceBuffer();
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    void *reserve(size_t bytes); // grow-only
    void *get() const { return ptr_; }
    size_t size() const { return size_; }

  private:
    void *ptr_ = nullptr;
    size_t size_ = 0;
};

// page-locked host memory for small transfers (single-frame decode(): the copies are latency, not bandwidth)
class PinnedBuffer
{
  public:
    PinnedBuffer() = default;
    ~PinnedBuffer();
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    void *reserve(size_t bytes); // grow-only
  private:
    void *ptr_ = nullptr;
    size_t size_ = 0;
};

// The chunk start states of one mt19937_64(seed) stream on the device: executes the operations mtstates.hpp plans
// (uploads, copies, jump launches) and keeps the device copies of the jump polynomials.
class MtDevice
{
  public:
    MtDevice();
    ~MtDevice();
    MtDevice(const MtDevice &) = delete;
    MtDevice &operator=(const MtDevice &) = delete;
    void reset(uint64_t seed); // chunk states depend on the seed only: kept when it does not change
    uint64_t seed() const { return seed_; }
    uint32_t chunk_blocks() const { return chunk_blocks_; }
    // before the first use of the stream only (the engine picks the chunk size by the decoder's residency; LDPC_AMD_CHUNK_BLOCKS
    // overrides either choice)
    void set_default_chunk_blocks(uint32_t blocks)
    {
        if (!chunk_blocks_from_env_)
            chunk_blocks_ = blocks;
    }
    uint64_t chunk_words() const { return static_cast<uint64_t>(kMtWords) * chunk_blocks_; }
    uint64_t chunk_trials() const { return chunk_words() / 2; }
    // consecutive chunks [c_lo, c_hi): their start states in the ring; returns the ring row of c_lo
    uint32_t ensure_ring(uint64_t c_lo, uint64_t c_hi, void *stream);
    // look-ahead: the start states of the chunks up to c_hi computed NOW, on a stream of this object's own, so that the
    // jump-ahead chain of a later request runs beside the generator chain of an earlier one instead of in front of it
    // (ensure_ring waits for exactly the look-ahead launches whose rows it reads)
    void prefetch_ring(uint64_t c_hi);
    uint64_t *ring() const { return static_cast<uint64_t *>(ring_buf_.get()); }
    static constexpr uint32_t ring_rows() { return StateRing::kRows; }
    // sharded stream: rows 0 .. n-1 = chunks [first, first + n), consecutive calls `stride` chunks apart cost one launch
    uint64_t *ensure_strided(uint64_t first, uint32_t n, uint64_t stride, void *stream);
    static constexpr uint32_t strided_rows() { return StridedTable::kMaxRows; }
    // look-ahead: the launches that bring the sharded stream's tables of the next two steps into being, now, on the
    // object's own stream (three tables: the generator of this step reads one while the others are written)
    void prefetch_strided();
    uint64_t jump_tasks() const { return jump_tasks_; } // jump-ahead tasks launched so far (tools/shard_probe.py)
    void set_jump_groups(int groups) { jump_groups_ = groups; }

  private:
    void apply(const std::vector<StateOp> &ops, uint64_t *table, void *stream);
    const uint64_t *device_poly(uint64_t stride, void *stream);
    uint64_t seed_ = 0;
    bool seeded_ = false;
    uint32_t chunk_blocks_;
    bool chunk_blocks_from_env_ = false;
    StateRing ring_;
    StridedTable strided_;
    DeviceBuffer ring_buf_, strided_buf_;
    std::vector<std::pair<uint64_t, void *>> polys_; // (stride in chunks, device copy)
    uint64_t jump_tasks_ = 0;
    int jump_groups_ = 1;
    bool ring_polys_ready_ = false;
    // look-ahead launches in flight on jump_stream_: the ring rows of chunks [hi_before, hi_after) are valid after `event`
    struct Ahead
    {
        uint64_t hi_before, hi_after;
        void *event;
    };
    void drain_ahead(void *stream, uint64_t below); // `stream` waits for the look-ahead launches that wrote rows below `below`
    void *jump_stream_ = nullptr;
    void *ev_main_ = nullptr;   // recorded on the caller's stream after ring operations issued there
    bool main_dirty_ = false;   // ... which the look-ahead stream has not waited for yet
    std::vector<Ahead> ahead_;  // oldest first
    void *ev_strided_[StridedTable::kSlots] = {}; // after the look-ahead launch into a table of the sharded stream
    bool strided_pending_[StridedTable::kSlots] = {};
    std::vector<void *> ev_free_;
};

// Raw words of one mt19937_64(seed) stream (BSC / BEC draws, info words, ldpc_hip_mt64).
class MtStream
{
  public:
    void reset(uint64_t seed) { st.reset(seed), last_end_ = ~0ull; }
    uint64_t seed() const { return st.seed(); }
    // chunks per generator workgroup (1 or 4, kernels.hpp launch_mt_generate)
    void set_pack(int chunks_per_workgroup) { pack_ = chunks_per_workgroup; }
    int pack() const { return pack_; }
    // raw words [first, first + count) on `stream`, into one of the stream object's two output buffers; returns a device
    // pointer to word `first`
    const uint64_t *generate(uint64_t first, uint64_t count, void *stream, int buffer = 0);
    MtDevice st;

  private:
    int pack_ = 1;
    uint64_t last_end_ = ~0ull; // word after the previous request
    DeviceBuffer raw_[2];
};

class Engine
{
  public:
    Engine(const std::string &pc_file, const std::string &gen_file, int device);
    ~Engine();

    const LdpcCode &code() const { return *code_; }
    const Plan &plan() const { return plan_; }
    const RegPlan &reg_plan() const { return reg_plan_; }
    const Reg2Plan &reg2_plan() const { return reg2_plan_; }
    const FusedPlan &fused_plan() const { return fused_plan_; }
    Residency residency() const { return residency_; }
    // the decoder and the launches a batch with these parameters takes (host only)
    Decoder decoder(const DecParams &p) const { return choose_decoder(p.min_sum, fast_mode, ms_variant_); }
    StageSeq stages(const DecParams &p) const
    {
        return decode_stages({.residency = residency_, .decoder = decoder(p), .shared6 = shared6_,
                              .ratio_width = plan_.max_cn_degree <= kMaxCnDegree, .min_sum = p.min_sum, .early_term = p.early_term,
                              .iterations = p.iterations > 0});
    }
    // host only: empty when decoder d takes this code, else the reason.  The one statement of what each variant takes; the
    // min-sum setters ask at set time, run_decode before the launch (set_fast_mode accepts anything: the first decode fails)
    std::string refusal(Decoder d);
    int device() const { return device_; }
    bool bec_deg1_compat = false;
    // opt-in NON-PARITY modes of sum-product, off (0) by default and never chosen by the library: 1 / 2 / 3 = kFast32 /
    // kLayered32 / kLayered16
    int fast_mode = 0;
    // noise of the stream interface (include/ldpc_amd.h, LDPC_HIP_NOISE_*): 0 = the reference's mt19937_64 stream (parity),
    // 1 = counter-based Philox4x32-10 of (seed, frame, bit), NON-PARITY (device_philox.hpp); stream_begin latches it
    int noise_mode = 0;
    // corrected min-sum of BP_MS decoding (include/ldpc_amd.h, ldpc_hip_set_min_sum_correction), NON-PARITY unless (1, 0):
    // check-node output magnitudes max(fl(fl(ms_scale * m) - ms_offset), +0.0) (device_cn.hpp, MsCorr); read at every decode
    double ms_scale = 1.0, ms_offset = 0.0;
    // The variants of BP_MS decoding, NON-PARITY (include/ldpc_amd.h): the schedule (0 flooding, 1 layered;
    // ldpc_hip_set_min_sum_schedule), quantization (bits 0 = off, 2..8, with LLR step; _quantization), ternary min-sum with its
    // channel weight (0 = off, 1..7; _ternary) and fixed-point layered min-sum (msg_bits 0 = off, 2..8 with msg_bits <= app_bits
    // <= 16 and the LLR step; _layered_fixed).  The four exclude each other.  Host only; each setter throws, leaving everything
    // as it is, for invalid values, another of the four in force, or a code refusal() names; "off" is always taken and
    // clears that variant alone.  A variant remembers its other parameters when it goes off: the getters report them
    void set_ms_schedule(int schedule);
    void set_ms_quantization(int bits, double step);
    void set_ms_ternary(int weight);
    void set_ms_layered_fixed(int msg_bits, int app_bits, double step);
    int ms_schedule() const { return ms_variant_ == MsVariant::kLayered; }
    int ms_bits() const { return ms_variant_ == MsVariant::kQuantized ? ms_bits_ : 0; }
    double ms_step() const { return ms_step_; }
    int ms_ternary() const { return ms_variant_ == MsVariant::kTernary ? ms_ternary_ : 0; }
    int ms_lf_msg_bits() const { return ms_variant_ == MsVariant::kLayeredFixed ? ms_lf_msg_bits_ : 0; }
    int ms_lf_app_bits() const { return ms_lf_app_bits_; }
    double ms_lf_step() const { return ms_lf_step_; }
    // host only: LDS bytes of one frame of a min-sum variant's decoder (plan.hpp, layered_ms_region_bytes / qms_region_bytes /
    // layered_fixed_region_bytes; ternary: of one 32-frame group with llr_out wanted, ternary_lds_bytes), -1 where its plan or
    // the kernel's tables do not take the code (a frame beyond the LDS of a CU still gets its byte count: refusal() judges it)
    int64_t lds_bytes(Decoder d);
    int64_t lds_bytes_if_taken(Decoder d) { return refusal(d).empty() ? lds_bytes(d) : -1; } // ... -1 for every code refusal() names
    int64_t layered_fixed_direct_lds_bytes(); // (plan.hpp, layered_fixed_direct_region_bytes: typed LLRs, nothing staged)
    // host only, built at the first call, once per engine
    const LayerPlan &layer_plan();
    const QmsPlan &qms_plan();
    int layer_plan_builds() const { return layer_plan_builds_; } // (tests: build_layer_plan runs at most once)

    // ---- decode given LLRs (C-ABI decode(), shared.cpp:47-65, batched) ----
    void decode_llr(const DecParams &p, uint64_t n, const double *llr_in, const BatchOut &out, void *stream);
    // ... of element type `type` (kernels.hpp, LlrType), and the decisions packed 32 to a word as well (hard_bits [n][ceil(nc /
    // 32)], device or host, nullptr = not wanted; include/ldpc_amd.h, ldpc_hip_decode_batch_typed).  kLlrF64 without
    // hard_bits is decode_llr.  Host only: what the call refuses before anything touches the GPU, empty when it is taken
    std::string typed_refusal(const DecParams &p, int type) const;
    void decode_typed(const DecParams &p, uint64_t n, const void *llr_in, int type, const BatchOut &out, uint32_t *hard_bits, void *stream);

    // ---- frames of bits that stay on the device (include/ldpc_amd.h, ldpc_hip_encode_batch / _syndrome_batch /
    // _bit_errors_batch; kernels_gf2.hip).  Rows are bytes or packed words (kernels.hpp, BitsFormat); every buffer is device or
    // host memory, an output nullptr = not wanted.  None of them reads or changes a setting or the stream interface's state.
    // Host only: what each call refuses before anything touches the GPU, empty when it is taken ----
    std::string encode_refusal(int info_format) const;
    std::string syndrome_refusal(int word_format) const;
    std::string bit_errors_refusal(int a_format, int b_format) const;
    // codeword[f][j] = XOR of info[f][i] over the entries (i, j) of G; column order, no running sum over the frames
    void encode_batch(uint64_t n, const void *info, int info_format, uint8_t *codeword, uint32_t *codeword_bits, void *stream);
    // syndrome[f][r] = XOR of word[f][c] over the entries (r, c) of H; weight[f] = the frame's unsatisfied check nodes
    void syndrome_batch(uint64_t n, const void *word, int word_format, uint8_t *syndrome, uint32_t *syndrome_bits, uint32_t *weight,
                        void *stream);
    // bit_errors[f] = transmitted positions at which rows f of a and b differ
    void bit_errors_batch(uint64_t n, const void *a, int a_format, const void *b, int b_format, uint32_t *bit_errors, void *stream);
    // the channel between them (include/ldpc_amd.h, ldpc_hip_channel_batch; kernels_channel.hip): codeword[n][nc] (nullptr =
    // all zero) -> llr[n][nc] of spec.llr_type and / or received[n][ceil(nct / m)], the noise that of the counter mode under
    // (spec.seed, spec.first_frame + row).  Reads neither the stream interface's channel point nor its noise setting
    struct ChannelSpec
    {
        int channel = 0; // kAwgn or kBsc
        double x = 0.0;  // stream_begin's meaning
        uint64_t seed = 0, first_frame = 0;
        int bits_per_symbol = 1;
        int llr_type = kLlrF64;
        int q_bits = 0;    // kLlrI8 only
        double step = 1.0; // kLlrI8 only
    };
    std::string channel_refusal(const ChannelSpec *spec, uint64_t n, int codeword_format, const void *llr, const double *received) const;
    void channel_batch(const ChannelSpec *spec, uint64_t n, const void *codeword, int codeword_format, void *llr, double *received,
                       void *stream);
    // the erasure channel and the genie-free erasure decoder behind it (include/ldpc_amd.h, ldpc_hip_erasure_channel_batch /
    // ldpc_hip_erasure_decode_batch; kernels_erasure.hip): packed words and erasure masks [n][ceil(nc / 32)] out of the
    // channel, into the decoder and out of it.  Host only: what each call refuses, empty when it is taken; the LDS of one
    // 32-frame group, -1 for a code the decoder refuses
    std::string erasure_channel_refusal(double eps, uint64_t n, int codeword_format, const void *word_bits, const void *erased_bits) const;
    void erasure_channel_batch(double eps, uint64_t seed, uint64_t first_frame, uint64_t n, const void *codeword, int codeword_format,
                               uint32_t *word_bits, uint32_t *erased_bits, void *stream);
    std::string erasure_decode_refusal(int flags, int format);
    int64_t erasure_lds_bytes();
    void erasure_decode_batch(uint32_t iterations, int flags, uint64_t n, const void *word, const void *erased, int format,
                              uint32_t *word_out, uint32_t *erased_out, uint32_t *iters, uint32_t *unresolved, void *stream);
    // maximum-likelihood erasure decoding: what elimination over GF(2) determines (include/ldpc_amd.h,
    // ldpc_hip_erasure_solve_batch; kernels_erasure_solve.hip).  Host only: the refusal, and the LDS of one frame at a cap,
    // -1 for a cap of 0 or a frame beyond a CU
    std::string erasure_solve_refusal(uint32_t max_unknowns, int format) const;
    int64_t erasure_solve_lds_bytes(uint32_t max_unknowns) const;
    void erasure_solve_batch(uint32_t max_unknowns, uint64_t n, const void *word, const void *erased, int format, uint32_t *word_out,
                             uint32_t *erased_out, uint32_t *unresolved, uint32_t *rank, uint32_t *status, void *stream);
    // ordered-statistics decoding of LLR frames: order 0 and the first `candidates` single flips (include/ldpc_amd.h,
    // ldpc_hip_osd_batch; kernels_osd.hip).  Host only: the refusal, and the LDS of one frame, -1 for a code beyond a CU
    std::string osd_refusal(int llr_type) const;
    int64_t osd_lds_bytes() const;
    void osd_batch(uint32_t candidates, uint64_t n, const void *llr, int llr_type, uint32_t *word_out, uint32_t *flips, uint64_t *metric,
                   uint32_t *flipped_column, uint32_t *status, void *stream);
    // ... toward a given syndrome, with every pair among the first `pair_depth` trusted columns as a second stage
    // (include/ldpc_amd.h, ldpc_hip_osd_syndrome_batch; kernels_osd_syndrome.hip).  Host only: the refusal and the LDS
    std::string osd_syndrome_refusal(uint32_t pair_depth, int llr_type, int syndrome_format) const;
    int64_t osd_syndrome_lds_bytes() const;
    void osd_syndrome_batch(uint32_t candidates, uint32_t pair_depth, uint64_t n, const void *llr, int llr_type, const void *syndrome,
                            int syndrome_format, uint32_t *word_out, uint32_t *flips, uint64_t *metric, uint32_t *flipped_columns,
                            uint32_t *status, void *stream);
    // quantized min-sum decoding toward a given syndrome (include/ldpc_amd.h, ldpc_hip_syndrome_decode_batch;
    // kernels_syndrome_decode.hip) on the tables of qms_plan().  Everything the call uses is in the spec: no setting of the
    // engine is read.  Host only: the refusal, and the LDS of one frame, -1 for a code the call does not take
    struct SyndromeDecodeSpec
    {
        uint32_t iterations = 0;
        int early_term = 0, q_bits = 0;
        double step = 0.0, scale = 0.0, offset = 0.0;
        int flags = 0;
    };
    static constexpr int kSyndromeSharedLlr = 1;
    std::string syndrome_decode_refusal(const SyndromeDecodeSpec *spec, int llr_type, int syndrome_format);
    int64_t syndrome_decode_lds_bytes();
    void syndrome_decode_batch(const SyndromeDecodeSpec *spec, uint64_t n, const void *llr, int llr_type, const void *syndrome,
                               int syndrome_format, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight, double *llr_out, void *stream);
    // ... on the layered schedule in fixed point (include/ldpc_amd.h, ldpc_hip_syndrome_decode_layered_batch;
    // kernels_syndrome_decode_layered.hip) on the tables of layer_plan().  As above: everything is in the spec
    struct SyndromeDecodeLayeredSpec
    {
        uint32_t iterations = 0;
        int early_term = 0, msg_bits = 0, app_bits = 0;
        double step = 0.0, scale = 0.0, offset = 0.0;
        int flags = 0;
    };
    std::string syndrome_decode_layered_refusal(const SyndromeDecodeLayeredSpec *spec, int llr_type, int syndrome_format);
    int64_t syndrome_decode_layered_lds_bytes();
    void syndrome_decode_layered_batch(const SyndromeDecodeLayeredSpec *spec, uint64_t n, const void *llr, int llr_type, const void *syndrome,
                                       int syndrome_format, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight, double *llr_out,
                                       void *stream);
    // gradient-descent bit flipping toward a given syndrome (include/ldpc_amd.h, ldpc_hip_bit_flip_batch;
    // kernels_bit_flip.hip) on the two adjacency tables of H in file order.  As above: everything is in the spec
    struct BitFlipSpec
    {
        uint32_t iterations = 0;
        int q_bits = 0;
        double step = 0.0;
        uint32_t check_weight = 0, margin = 0, flip_threshold = 0;
        uint64_t seed = 0, first_frame = 0;
        int flags = 0;
    };
    std::string bit_flip_refusal(const BitFlipSpec *spec, int llr_type, int syndrome_format) const;
    int64_t bit_flip_lds_bytes() const;
    void bit_flip_batch(const BitFlipSpec *spec, uint64_t n, const void *llr, int llr_type, const void *syndrome, int syndrome_format,
                        uint32_t *hard_bits, uint32_t *iters, uint32_t *weight, void *stream);
    // min-sum with memory, run as a relay of legs, toward a given syndrome (include/ldpc_amd.h, ldpc_hip_relay_decode_batch;
    // kernels_relay_decode.hip) on the tables of qms_plan().  As above: everything is in the spec.  `form` 0 = relay_form()
    struct RelayDecodeSpec
    {
        uint32_t legs = 0, first_iterations = 0, leg_iterations = 0, stop_after = 0;
        int q_bits = 0;
        double step = 0.0, scale = 0.0, offset = 0.0;
        int form = 0, flags = 0;
    };
    std::string relay_decode_refusal(const RelayDecodeSpec *spec, int llr_type, int syndrome_format);
    int relay_form(); // the form the library chooses for this code: 2 where it fits and the code is small
    int64_t relay_decode_lds_bytes(int form);
    void relay_decode_batch(const RelayDecodeSpec *spec, uint64_t n, const void *llr, int llr_type, const void *syndrome, int syndrome_format,
                            const int8_t *gamma, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight, uint32_t *solutions,
                            uint32_t *best_leg, uint32_t *cost, void *stream);

    // ---- fused channel + decode on the reference's noise stream ----
    // set_channel_param semantics (channel.cpp:37-42): the stream restarts at frame 0.
    // `fresh` also resets the encoder (info-word stream position and the accumulated codeword), i.e. a
    // newly constructed channel object; the reference keeps both across channel points of one run.
    void stream_begin(int channel, uint64_t seed, double x, bool fresh = true);
    void stream_skip(uint64_t n_frames, void *stream);
    void stream_decode(const DecParams &p, uint64_t n_frames, const BatchOut &out, void *stream);
    // Un-consume the last `frames_back` frames of the most recent stream_decode batch from the ENCODER state
    // (info-word stream position and accumulated codeword), so that the next channel point continues where a
    // frame-by-frame run that stopped inside the batch would (the noise stream restarts per point anyway).
    void stream_rewind_encoder(uint64_t frames_back, void *stream);
    // ---- the same stream decoded by several ranks (one process per GPU), SURVEY §8e ----
    // One global step of about target_frames frames.  AWGN: the step is a fixed range of the RAW stream cut into
    // world equal pieces; rank r generates and scans only its piece (+ a margin of one frame's worth), the ranks
    // all-gather their accepted-pair counts (one u64 each), and a frame belongs to the rank whose piece holds its
    // first pair — so every frame keeps its place in mt19937_64(seed) and nobody scans another rank's noise.
    // BSC / BEC draw once per bit: frames split evenly, no exchange.  Every rank ends the step with the same
    // stream position.  `out` must hold shard_capacity(target_frames, world) frames.
    struct ShardStep
    {
        uint64_t step_first = 0, step_frames = 0; // the global step
        uint64_t first = 0, n = 0;                // this rank's frames [first, first + n)
    };
    ShardStep stream_decode_sharded(Comm &comm, const DecParams &p, uint64_t target_frames, const BatchOut &out, void *stream,
                                    const std::string *failed_before = nullptr);
    // encoder state (info-word stream position + accumulated codeword) saved before a step / put back and advanced by
    // `frames` frames: how every rank lands on the state after the frame at which the simulation stopped
    void encoder_snapshot(void *stream);
    void encoder_restore_and_skip(uint64_t frames, void *stream);
    uint64_t stream_frame() const { return frame_pos_; }
    uint64_t stream_raw_draws(); // (AWGN: locates the last consumed trial with one generator pass over its chunk)
    // frames a sharded step of about target_frames can put on one rank (the output buffers' size)
    uint64_t shard_capacity(uint64_t target_frames, int world) const;
    uint64_t noise_jump_tasks() const { return noise_.st.jump_tasks(); }
    bool counter_noise() const { return counter_; }

    void synchronize(void *stream);
    uint64_t max_sub_batch() const; // frames one launch takes; larger requests are split

    // kernel timing with HIP events on the launch stream (bench.py's roofline figure)
    void set_profiling(bool on);
    // mean ms since the previous call: which = 0 decode launches, 1 noise-stream kernels (HIP events); 2 host time inside the
    // ranks' exchange, 3 host time waiting for the noise stream's result (wall clock)
    float last_ms(int which);

  private:
    void bind_device();
    void ensure_rng_stream();
    // BSC / BEC: the batch's raw words generated on the engine's side stream into one of two buffers, ordered before the
    // caller's stream by an event — so that the generation for batch s+1 runs under the decode of batch s, as the AWGN
    // path's noise stream does; noise_raw_release() after the launch that reads them
    const uint64_t *noise_raw_async(uint64_t first, uint64_t count, void *stream, int &buffer);
    void noise_raw_release(int buffer, void *stream);
    // hipMalloc (kept until the engine goes), synchronous copy; `what` names the table in an error
    const void *upload_table(const void *src, size_t bytes, const char *what);
    void upload_plan();
    // the device halves of layer_plan() and qms_plan(): at the first launch that needs them
    void upload_layer_plan();
    void upload_qms_plan();
    // after a setter has checked its own arguments: throws if another variant is in force or the code is refused, else v is in force
    void enter_ms_variant(MsVariant v);
    void leave_ms_variant(MsVariant v) { ms_variant_ = ms_variant_ == v ? MsVariant::kFlooding : ms_variant_; }
    QmsArgs qms_args() const; // the quantizer and the correction table of the settings in force
    LayeredFixedArgs layered_fixed_args() const; // ... and those of fixed-point layered min-sum
    bool register_resident() const { return residency_ == Residency::kRegTotals || residency_ == Residency::kRegMessages; }
    // what a typed batch call adds to a launch of given LLRs: the typed input on the device (llr null: a.llr_in holds binary64
    // values already) with the step an int8 stands for, and where the packed decisions go (null: not wanted)
    struct TypedIo
    {
        const void *llr = nullptr;
        int type = kLlrF64;
        double step = 1.0;
        uint32_t *hard_bits = nullptr;
    };
    void run_decode(DecodeArgs &a, const DecParams &p, const BatchOut &out, uint64_t n, void *stream, const TypedIo *typed = nullptr);
    // BSC / BEC: the batch reads the noise stream's raw draws from word `raw_first` on
    void run_bsc(DecodeArgs &a, const DecParams &p, const BatchOut &out, uint64_t n, uint64_t raw_first, void *stream);
    // (ctr_frame0: counter-based noise, the stream index of the batch's frame 0; raw_first is then unused)
    void run_bec(const DecParams &p, const BatchOut &out, uint64_t n, const uint8_t *codeword, uint64_t raw_first, void *stream,
                 const uint64_t *ctr_frame0 = nullptr);
    // after a batch's last launch: the noise buffer it read released (-1: none), the codewords and the staged outputs delivered
    void finish_batch(OutStage &st, const BatchOut &out, uint64_t n, const uint8_t *codeword, int noise_buffer, void *stream);
    // normals of frames [frame_pos_, frame_pos_ + n): generate, count, place (write_normals false: count only, stream_skip)
    void awgn_prepare(uint64_t n_frames, DecodeArgs &a, void *stream, bool write_normals = true);
    // one generator pass over chunks [chunk, chunk + full) (+ a prefix of `last_blocks` blocks of the next one) on the side stream
    struct NoisePass
    {
        uint32_t n_slabs = 0;
        uint64_t *slabs = nullptr, *cum = nullptr;
        NormalsResult res{};
    };
    // Small requests in a row (one frame at a time: the reference's own call pattern) — the last single-chunk pass is kept:
    // it was generated a few frames further than asked, and while the following requests fall inside it they take their
    // normals from the slab that is already there instead of regenerating their chunk's prefix from its start
    struct SmallCache
    {
        bool valid = false;
        uint64_t chunk = 0;
        int buf = 0;
        NoisePass np;
    } small_cache_;
    NoisePass noise_pass(uint64_t chunk, uint32_t full, uint32_t last_blocks, uint32_t n_piece, uint64_t need, uint64_t target, int buf,
                         bool write_normals, bool strided, uint64_t stride);
    void fill_slab_args(DecodeArgs &a, const NoisePass &np, uint64_t pair_origin, int buf) const;
    // advance the encoder by n frames; returns the per-frame codewords [n][nc] (nullptr when no G is
    // loaded, or when want_codewords is false)
    const uint8_t *encode_frames(uint64_t n, bool want_codewords, void *stream);
    // the encoder's part of a sharded step of step_frames frames of which this rank decodes [before, before + n): the rank
    // draws the info words of ITS frames only, the ranks exchange the XOR of theirs (one all-gather of ceil(kc / 64) words),
    // and every rank ends with the codeword accumulated over the whole step.  Returns this rank's codewords [n][nc].
    const uint8_t *encode_frames_sharded(Comm &comm, uint64_t before, uint64_t n, uint64_t step_frames, void *stream);
    // both: G checked against the code (and, sharded, against the exchange's size), the running codeword (zeroed when not
    // valid) and its copy for stream_rewind_encoder; returns the running codeword
    uint8_t *encoder_prologue(uint64_t frames_kept, bool sharded, void *stream);
    // counter-based noise: the codewords u_f G of frames [frame0, frame0 + n) from their own info words (tag 2), no running
    // state (nullptr when no G is loaded)
    const uint8_t *encode_frames_counter(uint64_t frame0, uint64_t n, void *stream);
    // counter-based noise: the channel of frames [frame0, frame0 + n) computed inside the decode launch (fast modes refused)
    void run_counter(const DecParams &p, const BatchOut &out, uint64_t frame0, uint64_t n, void *stream);

    std::unique_ptr<LdpcCode> code_;
    Plan plan_;
    RegPlan reg_plan_;
    Reg2Plan reg2_plan_;
    bool shared6_ = false; // not LDS-resident and a check node of degree 6 (decode_stages: dm_cn6_shared, then kRatioSeparate)
    FusedPlan fused_plan_; // fused form of the first ratio launch (kernels_fused.hip); ok = the code qualifies (fused_rule.h)
    Residency residency_ = Residency::kNone;
    int lds_llr_mode_ = 0;     // LDS-resident: the input LLRs in LDS (0) or in registers (2), kernels.hpp launch_decode_lds
    uint32_t mem_occ_lds_ = 0; // memory-resident: the dummy LDS request that bounds the resident frames per CU
    DevFusedPlan dev_fused_{};
    MsVariant ms_variant_ = MsVariant::kFlooding;
    int ms_bits_ = 0, ms_ternary_ = 0; // each variant's parameters as last set (they mean something while it is in force)
    double ms_step_ = 1.0;
    int ms_lf_msg_bits_ = 0, ms_lf_app_bits_ = 8;
    double ms_lf_step_ = 1.0;
    std::optional<LayerPlan> layer_plan_;
    int layer_plan_builds_ = 0;
    DevLayerPlan dev_layer_{}; // (rec_off == nullptr: not uploaded yet)
    std::optional<QmsPlan> qms_plan_;
    DevQmsPlan dev_qms_{}; // (cn_desc == nullptr: not uploaded yet)
    DevPlan dev_{};
    DevRegPlan dev_reg_{};
    DevReg2Plan dev_reg2_{};
    int device_ = 0;
    bool device_checked_ = false;
    std::vector<void *> owned_;

    // stream state
    int chan_ = 0;
    double x_ = 0, sigma2_ = 0, sigma_ = 0, delta_ = 0;
    uint64_t frame_pos_ = 0;
    bool counter_ = false;    // counter-based noise latched by stream_begin (noise_mode == 1)
    uint64_t ctr_seed_ = 0;   // ... and its Philox key (seed & 0xFFFFFFFF, seed >> 32)
    DeviceBuffer cw_zero_;    // counter-mode encoder: an all-zero running codeword
    int stream_mode_ = 0; // 0 fresh, 1 stream_decode / stream_skip, 2 stream_decode_sharded (pair bookkeeping differs)
    uint64_t raw_next_ = 0;  // BSC / BEC: raw draws consumed so far
    // AWGN, one rank reading the stream front to back: the pair with stream index cur_pair_ (= first normal of the next
    // frame >> 1) is the cur_k_-th accepted pair of chunk cur_chunk_
    uint64_t cur_pair_ = 0, cur_chunk_ = 0, cur_k_ = 0;
    // AWGN, sharded: the next step starts at chunk sh_chunk_, sh_pairs_ pairs were accepted before it
    uint64_t sh_chunk_ = 0, sh_pairs_ = 0;
    MtStream noise_, info_;
    uint64_t info_pos_ = 0;     // info-word draws consumed (kc per frame)
    bool cw_run_valid_ = false; // cw_run_ holds the accumulated codeword
    DeviceBuffer cw_run_, cw_next_, cw_frames_, cw_before_, enc_prefix_;
    uint64_t last_enc_n_ = 0;   // frames of the last encode_frames call that produced cw_frames_
    const uint32_t *g_col_ptr_ = nullptr, *g_col_row_ = nullptr;
    const uint64_t *g_mask_ = nullptr; // the columns of G as bit masks, [nc][words] (kernels.hpp, EncodeArgs::g_mask)
    DeviceBuffer slabs_[2], slab_cum_[2], nz_counts_, nz_result_, nz_locate_, nz_cum_skip_, nz_raw_, nz_lookback_;
    // the AWGN noise generator runs on its own stream so that the normals of batch s+1 are produced while
    // the decode kernel of batch s drains; the slabs are double-buffered, events order the two streams
    void *rng_stream_ = nullptr;
    void *ev_pairs_ready_[2] = {nullptr, nullptr}, *ev_pairs_free_[2] = {nullptr, nullptr};
    bool pairs_in_use_[2] = {false, false};
    int pp_ = 0;
    DeviceBuffer enc_base_; // sharded encoding: the other ranks' info-word sums (two rows of `words`)
    DeviceBuffer stage_in_, stage_iters_, stage_be_, stage_hard_, stage_llr_out_, stage_llr_in_, stage_cw_;
    DeviceBuffer stage_typed_, stage_bits_; // typed batch call: host input in its own type, packed decisions for a host buffer
    // the batch calls on frames of bits: the tables (each uploaded by the first call that needs it: a context that never
    // encodes builds no mask table), the packed image of byte information, staging of a second host input and of host outputs
    const uint32_t *gf2_mask_ = nullptr;    // [ceil(kc / 32)][gf2_mask_cols_]: the columns of G as masks, word-major (Gf2EncodeArgs)
    uint64_t gf2_mask_cols_ = 0;
    const uint32_t *gf2_row_ptr_ = nullptr, *gf2_row_col_ = nullptr; // row CSR of H
    void upload_rows_of_h();                                         // (the first call that reads them)
    const uint64_t *gf2_tx_mask_ = nullptr; // the transmitted positions (bit_pos) as a mask over the columns
    DeviceBuffer gf2_info_, stage_in_b_, stage_gf2_[3];
    // the channel call: the columns the channel does not write (column | kChannelShortened) and the ASK constellations of
    // m = 2..4 (16 levels each, binary64), both uploaded by the first call; staging of host outputs
    const uint32_t *chan_other_ = nullptr;
    uint32_t chan_n_other_ = 0;
    const double *chan_levels_ = nullptr;
    DeviceBuffer stage_chan_[2];
    // the erasure calls: the channel's column table ([32][ceil(nc / 32)], kernels.hpp ErasureChannelArgs) and the decoder's
    // chunked graph (kernels.hpp ErasureDecodeArgs), each built on the host at the first call that needs it and uploaded by
    // the first one that launches; the packed images of byte input; staging of host outputs
    struct ErasureTables
    {
        std::vector<uint32_t> desc;
        std::vector<uint16_t> cn_entries, vn_entries, vn_col;
        uint32_t cn_chunks = 0, vn_chunks = 0;
        int64_t lds_bytes = -1; // -1: the decoder does not take the code
    };
    std::optional<ErasureTables> erasure_tables_;
    const ErasureTables &erasure_tables();
    const uint32_t *era_col_tx_ = nullptr, *era_desc_ = nullptr;
    const uint16_t *era_cn_entries_ = nullptr, *era_vn_entries_ = nullptr, *era_vn_col_ = nullptr;
    DeviceBuffer era_packed_[2], stage_era_[5]; // (five outputs: the solver's)
    DeviceBuffer stage_osd_[5];                 // the outputs of osd_batch for host buffers
    DeviceBuffer stage_sd_[4];                  // ... and of syndrome_decode_batch
    const uint32_t *sd_cn_row_ = nullptr;       // Plan::cn_rank_row on the device, at the first syndrome_decode_batch
    const uint32_t *sdl_step_row_ = nullptr;    // (step, lane) -> file row, at the first syndrome_decode_layered_batch
    const uint32_t *bf_row_ptr_ = nullptr, *bf_col_ptr_ = nullptr; // the rows and the columns of H, file order, u16 indices,
    const uint16_t *bf_row_col_ = nullptr, *bf_col_row_ = nullptr; // at the first bit_flip_batch
    DeviceBuffer stage_relay_[3];               // relay_decode_batch: its three further outputs (the first three: stage_sd_)
    DeviceBuffer stage_relay_gamma_;            // ... and a host gamma
    uint64_t gf2_sub_batch() const; // frames per launch: staging buffers stay modest, no grid dimension overflows
    // a host input of a batch call on the device (small ones through page-locked memory); a device pointer comes back as it is
    const void *stage_input(const void *src, size_t bytes, DeviceBuffer &stage, void *stream);
    DeviceBuffer ws_msg_, ws_llr_, ws_hb_, ws_scr_;
    PinnedBuffer pin_in_, pin_out_;
    void *pin_in_ev_ = nullptr; // hipEvent_t: the last host-to-device copy out of pin_in_
    DeviceBuffer enc_snap_;
    uint64_t enc_snap_pos_ = 0;
    bool enc_snap_valid_ = false;
    DeviceBuffer redo_, redo2_; // [0] = count, [1..] = frames handed back by the (first / second) ratio-form launch
    bool profiling_ = false;
    double host_ms_[2] = {0, 0}; // [0] exchange, [1] noise-stream wait
    uint64_t host_n_[2] = {0, 0};
    std::vector<void *> prof_pending_[2], prof_free_; // hipEvent_t: begin/end pairs per launch, spare events
    void prof_mark(int which, void *stream);
};

std::string hip_error_string(int err);

} // namespace ldpc_amd
