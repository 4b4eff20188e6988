// plan.hpp — device execution plan for a parity-check graph.
//
// The reference walks H through per-node neighbour vectors (sparse.h:77-79) one frame at a time.
// The MI355X decoder keeps one frame's messages in LDS and gives every lane one node, so the graph
// is re-laid-out once per code:
//
//   * check nodes are grouped by degree into blocks of <= 64 (one wave, uniform degree, no
//     divergence); block b owns message slots [off, off + degree*count), slot(lane, j) =
//     off + j*count + lane, so a wave's j-th load/store is one contiguous, bank-conflict-free run;
//   * variable nodes are grouped the same way; VN lane `rank` reaches its edges (in the file order
//     the reference sums them in, decoder.cpp:50-56) through a u16 slot table laid out
//     [block][position][lane] so the index loads coalesce;
//   * blocks are dealt to the workgroup's waves by longest-processing-time so that waves finish
//     each half-iteration together.
//
// Message values, their summation order and the per-edge results are those of the reference;
// only where they live changes.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "code.hpp"

namespace ldpc_amd
{

constexpr int kWaveSize = 64;
constexpr int kMaxLdsCnDegree = 8;  // widest check node of the LDS-resident decoder's register CN update
constexpr int kMaxCnDegree = 16;    // widest check node of the memory-resident decoder
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr int kDecodeWaves = 4;     // waves per workgroup of the LDS-resident decoder

struct CnBlock
{
    uint32_t off;    // first message slot
    uint16_t count;  // check nodes in the block (<= 64)
    uint16_t degree;
};

constexpr int kVnPackedRows = 32;
constexpr uint32_t kVnSrcZero = 0xFFFFFFFFu, kVnSrcShortened = 0xFFFFFFFEu;

struct VnBlock
{
    uint32_t idx_off; // into vn_slot: [idx_off + p*count + lane]
    uint32_t first;   // first VN rank
    uint16_t count;
    uint16_t degree;
};

// Host-side plan (uploaded verbatim by the engine)
struct Plan
{
    int nc = 0, mc = 0, nnz = 0, nct = 0;
    int n_bitpos = 0; // entries of bit_pos (> nct when a column is both punctured and shortened)
    int max_cn_degree = 0, max_vn_degree = 0;
    std::vector<CnBlock> cn_blocks;
    std::vector<VnBlock> vn_blocks;
    std::vector<uint32_t> vn_slot;   // slot of the p-th edge (column file order) of each VN
    std::vector<uint32_t> cn_work;   // [kDecodeWaves][cn_work_stride] block ids, 0xFFFF = none
    std::vector<uint32_t> vn_work;   // [kDecodeWaves][vn_work_stride]
    int cn_work_stride = 0, vn_work_stride = 0;
    // the same work lists with the descriptors in place of the block ids (count 0 = none; cn_work_desc rows are
    // padded to an even number of entries plus two): a wave reads the two blocks it handles together with ONE
    // scalar load instead of two dependent ones
    std::vector<CnBlock> cn_work_desc; // [kDecodeWaves][cn_desc_stride]
    int cn_desc_stride = 0;
    std::vector<uint32_t> vn_work_desc; // [kDecodeWaves][vn_work_stride + 1][4]: idx_off, first, count | degree << 16, 0
    // the slot indices a lane of the LDS-resident decoder keeps in registers, as it keeps them (two u16 per word), so that it
    // picks them up with one load per word, none dependent on another: [kDecodeWaves][kVnPackedRows][64] — rows 0..7: block
    // w of the wave's work list if its nodes have one or two edges (first slot | last slot << 16), rows 8..15: the wave's
    // FIRST block if its nodes have 3..16 edges (slots 2i, 2i+1 in word i); zero where there is nothing.  Rows 16..23: where
    // the LLR of the lane's node in block w comes from — the index of its bit among the transmitted ones, or kVnSrcZero
    // (punctured, never written by the channel, no node) / kVnSrcShortened; rows 24..31: the node's column (kVnSrcZero: no
    // node).  Empty when a slot needs more than 16 bits or a wave has more than 8 blocks (such codes do not use the
    // register-held indices).
    std::vector<uint32_t> vn_packed;
    std::vector<uint32_t> col_rank;  // column -> VN rank
    std::vector<uint32_t> rank_col;  // VN rank -> column
    std::vector<uint32_t> tx_rank;   // transmitted index i -> rank of bit_pos[i]
    std::vector<uint8_t> rank_kind;  // 0 transmitted, 1 punctured, 2 shortened, 3 never written by the channel
    std::vector<uint32_t> rank_slot0; // slot of the VN's first edge, kNoSlot for an isolated VN
    std::vector<uint32_t> edge_slot; // file-order edge -> slot (tests / debugging)
    std::vector<uint32_t> cn_rank_row; // slot-space CN order -> original row (tests)
    size_t lds_bytes = 0;            // dynamic LDS the LDS-resident kernel needs per frame
    bool lds_ok = false;             // fits the LDS-resident kernel's limits
    bool hbm_ok = false;             // within the memory-resident kernel's limits
    bool has_isolated_vn = false;    // a column without any edge
};

// ---- register-resident decoder (codes too large for 4 frames of LDS per CU, e.g. n=8192) ----------------
// One workgroup of nt threads = one frame.  Thread (wave, lane) owns the check nodes of the CN blocks
// k*(nt/64) + wave, k < kc, and keeps their messages in registers m[k][j].  The variable-node side is reached through
// an LDS mailbox laid out VN-block-major ([position][lane] inside a block of <= 64 equal-degree VNs); a code
// whose edges do not fit the mailbox at once is exchanged in `rounds` groups of VN blocks.
constexpr uint32_t kRegNoEdge = 0xFFFFFFFFu;

struct RegVnBlock
{
    uint32_t first;   // first VN rank
    uint32_t mb_off;  // mailbox offset (in doubles) of (position 0, lane 0); (p, lane) sits at mb_off + p*count + lane
    uint16_t count;
    uint16_t degree;
};

struct RegPlan
{
    bool ok = false;
    int nt = 0;                     // threads per workgroup (1024: one frame per CU, 512: two)
    int kc = 0, maxd = 0;           // CN blocks per wave, register columns per CN
    int rounds = 0;
    uint32_t mb_doubles = 0;        // mailbox capacity in doubles (LDS = 9 bytes per entry)
    std::vector<uint32_t> cn_edge;  // [(k*maxd + j)*nt + tid] = (round << 28) | mailbox offset, kRegNoEdge = none
    std::vector<uint8_t> cn_deg;    // [k*(nt/64) + wave] degree of that CN block (0 = none)
    std::vector<uint8_t> cn_cnt;    // [k*(nt/64) + wave] check nodes in the block
    std::vector<RegVnBlock> vn_blocks;      // in round order
    std::vector<uint32_t> round_first;      // [rounds+1] first VN block of each round
};

// ---- register-resident decoder, second form: totals come back instead of messages ---------------------------
// One workgroup of nt threads (nt/64 waves) = one frame per CU.  Thread (wave, lane) owns the check nodes of CN blocks
// k*(nt/64) + wave, k < kc, and keeps their messages in registers.  The thread that owns an edge also forms the edge's
// v2c message: the variable node's thread returns only the node's TOTAL (decoder.cpp:50-56: out, or its likelihood
// ratio), one entry per node instead of one per edge, and the hard decision travels in that entry's sign
// (ratio form) or is read off it (LLR domain: out <= 0).  c2v messages reach the variable nodes through an LDS
// mailbox of 8-byte entries in two rounds (the n=8192 code's 24576 messages exceed 160 KB):
//
//   entries [0, e_max)            mailbox: round 0 uses [0, E0), round 1 [0, E1); a VN block's column sits at
//                                 p0_off + lane (position 0) and prest_off + (p-1)*count + lane (positions >= 1)
//   entries [e_max, e_max + n0)   totals of the round-0 variable nodes (round-1 totals are written in place, over
//                                 position 0 of their column, which nothing overwrites before the gather)
//   entry   16384                 trash, at byte 0x20000 exactly: every thread writes all its register columns in
//                                 both rounds, and the address arithmetic sends the columns whose node belongs to
//                                 the other round (or that hold no edge) here (edge_w below)
//   entry   neutral               +1.0: what register columns without an edge gather
//   (when the round-0 totals do not fit below the trash entries they follow them)
//
// Variable-node blocks are dealt to (round, i, wave): wave w handles blocks [(round, i, w)] for i < nv[round].

constexpr uint32_t kReg2TrashEntry = 16384; // byte 0x20000

struct Reg2VnBlock
{
    uint32_t p0_off;    // entry of (position 0, lane 0)
    uint32_t prest_off; // entry of (position 1, lane 0)
    uint32_t tot_off;   // entry the total of lane 0 is written to
    uint16_t count;     // 0 = no block
    uint16_t degree;
};

struct Reg2Plan
{
    bool ok = false;
    int nt = 0, kc = 0, maxd = 0, nv0 = 0, nv1 = 0;
    uint32_t e_max = 0, neutral = 0, lds_entries = 0;
    bool uniform_cn = false; // all kc * (nt/64) check-node blocks exist and have maxd edges: the kernel's UCN instantiation
    bool uniform_vn = false; // all (nv0 + nv1) * (nt/64) variable-node blocks are full, of degree 3, at affine offsets:
    uint32_t vn_affine[2][6] = {}; // per round {p0 base, stride, prest base, stride, tot base, stride} in entries per block
    // [(k*maxd + j)*nt + tid]: bits 3..17 = byte address the edge's VN total is gathered from, bits 18..31 = mailbox
    // entry the edge's c2v message is scattered to, bit 0 = the round of the edge's node, bit 1 = no edge.  Rotated
    // right by 15 and masked with 0x7FFF8 the word is the scatter byte address plus 0x20000 (round 1) or 0x40000 (no
    // edge): round r subtracts r * 0x20000 and takes the unsigned minimum with the trash address 0x20000, which leaves
    // the addresses of its own round alone and sends everything else to trash.
    std::vector<uint32_t> edge_w;
    std::vector<uint8_t> cn_deg;       // [k*(nt/64) + wave] degree of that CN block (0 = none)
    std::vector<uint8_t> cn_cnt;       // [k*(nt/64) + wave] check nodes in the block
    std::vector<Reg2VnBlock> vn_blocks; // [(i*(nt/64) + wave)], i < nv0 + nv1 (i < nv0: round 0)
    std::vector<uint32_t> vn_rank;      // [(i*(nt/64) + wave)*64 + lane] VN rank of the Plan (kNoSlot = none)
};

// ---- layered schedule of the opt-in non-parity modes (kernels_layered.hip) -----------------------------------------
// A sweep over the check nodes is a sequence of STEPS; a step is up to 64 check nodes of equal degree no two of which
// share a variable node (one wave = one frame, one lane = one check node of the step).  Edge j of lane l of a step sits
// at offset off + j * 64 + l of the vn table (VN rank of the Plan) and of the frame's message array.
struct LayerStep
{
    uint32_t off;
    uint16_t count, degree;
};
struct LayerPlan
{
    bool ok = false;
    std::vector<LayerStep> steps;
    std::vector<uint16_t> vn;
    uint32_t slots = 0; // entries of the message array (sum of 64 * degree over the steps)
    std::vector<int> step_of_row; // (tests: the step each check node is processed in)
};
LayerPlan build_layer_plan(const LdpcCode &code, const Plan &plan);
// Layered min-sum (kernels_layered_ms.hip) keeps a 20-byte RECORD per check node instead of its messages: two binary64
// magnitudes and one 32-bit word, [field][lane] within a step over the step's real check nodes rounded up to an even
// number (every step stays 8-byte aligned).  Returns the records' size in bytes; rec_off (if given) receives each step's
// byte offset.
inline size_t layered_ms_records(const LayerPlan &L, std::vector<uint32_t> *rec_off = nullptr)
{
    size_t bytes = 0;
    for (const LayerStep &st : L.steps)
    {
        if (rec_off)
            rec_off->push_back(static_cast<uint32_t>(bytes));
        bytes += 20 * ((static_cast<size_t>(st.count) + 1) & ~size_t(1));
    }
    return bytes;
}
// ... and the LDS of one frame: the binary64 totals and the records
inline size_t layered_ms_region_bytes(const LayerPlan &L, size_t nc) { return (8 * nc + layered_ms_records(L) + 15) & ~size_t(15); }
// Fixed-point layered min-sum (kernels_layered_fixed.hip; include/ldpc_amd.h, ldpc_hip_set_min_sum_layered_fixed) keeps the
// totals as int16 and ONE 32-bit record per check-node slot (`slots` = layered_ms_records / 20: each step's check nodes
// rounded up to an even number).  The channel first writes nc binary64 LLRs; the totals (2 nc bytes) and, from the next
// multiple of 4, the records overlay them; the 128-byte correction table sits behind the larger of the two:
//   bytes = max(8 nc, round4(2 nc) + 4 slots) + 128, rounded up to 16
constexpr size_t layered_fixed_records_off(size_t nc) { return (2 * nc + 3) & ~size_t(3); }
constexpr size_t layered_fixed_lut_off(size_t slots, size_t nc)
{
    return 8 * nc > layered_fixed_records_off(nc) + 4 * slots ? 8 * nc : layered_fixed_records_off(nc) + 4 * slots;
}
constexpr size_t layered_fixed_region_bytes(size_t slots, size_t nc) { return (layered_fixed_lut_off(slots, nc) + 128 + 15) & ~size_t(15); }
// ... and where typed LLRs are quantized straight from memory (kernels_layered_fixed_direct.hip) no binary64 value is staged:
// the totals, the records, the table
//   bytes = round4(2 nc) + 4 slots + 128, rounded up to 16
constexpr size_t layered_fixed_direct_region_bytes(size_t slots, size_t nc)
{
    return (layered_fixed_records_off(nc) + 4 * slots + 128 + 15) & ~size_t(15);
}
constexpr size_t kCuLdsBytes = 160 * 1024; // the LDS of one CU: what a frame of any decoder has to fit
// what build_reg_plan leaves of it to the static LDS of the messages-form register kernels (kernels_reg.hip: 272 bytes in the
// compiler's resource report — 16 of misc[] and 256 the compiler adds; tests/test_generator_codes_host.py holds the report to
// this figure).  It was 256: a code whose mailbox peak reached the last 64-entry step asked for 160 KiB + 16 bytes and every
// launch failed with "invalid argument"
constexpr uint32_t kRegStaticLds = 512;

// ---- quantized (fixed-point) min-sum (kernels_qms.hip; include/ldpc_amd.h, ldpc_hip_set_min_sum_quantization) ----------
// One byte per message.  Check nodes in CSR, in the order of Plan::cn_rank_row (by degree, so neighbouring threads loop
// alike); a check node's message slots are consecutive bytes, padded to a multiple of 4 so that the check-node pass reads
// and writes whole words.  Variable nodes in CSC, in rank order (the order channel_init writes the LLRs in).
struct QmsPlan
{
    bool ok = false;                // nc <= 65535 (a VN rank takes 16 bits)
    uint32_t slots = 0;             // message bytes of a frame, padding included (a multiple of 4)
    std::vector<uint32_t> cn_desc;  // [mc][2]: byte offset of the check node's first slot, its degree
    std::vector<uint16_t> cn_vn;    // [slots]: VN rank of the slot's edge (0 in the padding)
    std::vector<uint32_t> vn_start; // [nc + 1] into vn_slot
    std::vector<uint32_t> vn_slot;  // [nnz]: slots of the variable node's edges
};
QmsPlan build_qms_plan(const LdpcCode &code, const Plan &plan);
// The LDS of one frame.  The channel first writes nc binary64 LLRs; behind them sit the nc quantized channel values (one
// byte each).  Once those are taken, the binary64 area is used again for the messages (`slots` bytes), the nc 32-bit totals
// the 128-byte correction table and 16 bytes for the workgroup's vote, and grows to hold them where 8 nc bytes are too few:
//   bytes = max(8 nc, slots + 4 nc + 144) rounded up to 4, + nc, rounded up to 16
inline size_t qms_work_bytes(size_t slots, size_t nc) { return (std::max(8 * nc, slots + 4 * nc + 144) + 3) & ~size_t(3); }
inline size_t qms_region_bytes(size_t slots, size_t nc) { return (qms_work_bytes(slots, nc) + nc + 15) & ~size_t(15); }

// ---- ternary min-sum, bit-sliced (kernels_ternary.hip; include/ldpc_amd.h, ldpc_hip_set_min_sum_ternary) ----------------
// One workgroup = 32 frames, bit f of every word = frame f, on the general plan's blocks and slot table.
constexpr int kTernaryFrames = 32;
constexpr int kTernaryMaxVnDegree = 56; // |A| <= 56 + 7 = 63: seven planes
constexpr size_t kTernaryHeadWords = 64; // the group's votes and error counts
// planes of A = w r + the sum of a column's inputs in two's complement, for any weight 1..7: |A| <= max_vn_degree + 7
constexpr int ternary_planes(int max_vn_degree)
{
    int bits = 1;
    for (int x = max_vn_degree + 7; x; x >>= 1)
        ++bits;
    return bits;
}
// the message words Z[nnz] S[nnz]; at least 8 nc bytes, which the channel prologue stages one frame's binary64 LLRs in
constexpr size_t ternary_message_words(size_t nnz, size_t nc) { return 2 * std::max(nnz, nc); }
// The LDS of one 32-frame group: the head, the messages, three words per column (r = +1, r = -1, the decision), the
// `planes` words per column of A where llr_out is wanted (`totals`), and two u16 per edge (the variable nodes' slot table
// and the table slot -> variable-node rank the syndrome goes through)
constexpr size_t ternary_lds_bytes(size_t nnz, size_t nc, int planes, bool totals)
{
    const size_t words = kTernaryHeadWords + ternary_message_words(nnz, nc) + 3 * nc + (totals ? static_cast<size_t>(planes) * nc : 0);
    return (4 * words + 4 * nnz + 15) & ~size_t(15);
}

// ---- fused form of the likelihood-ratio iteration (kernels_fused.hip; detmath.h "Fused form", fused_rule.h) ----------
// First launch of sum-product with early termination for codes the rule takes (check nodes of degree 2..4 with at most one
// leaf each).  One workgroup (4 waves) per frame as in the LDS-resident decoder, but only edges that do NOT end in a leaf
// have a message slot, check-node blocks are uniform in CLASS (degree, leaf or not, how many outputs go to degree-2
// neighbours) with their inputs in the rule's order, and a wave's work is a list of CALLS of one or two blocks.
//   slot of (block, lane, k-th message input) = off + k * count + lane; all offsets below are BYTE offsets (< 2^16).
constexpr int kFusedVnSlots = 8;    // variable-node blocks per wave (general instantiation; the small one takes 4)
constexpr int kFusedLeafCalls = 2;  // calls with leaves per wave (general instantiation; the small one takes 1)
constexpr int kFusedLaneRows = 44;  // rows of the lane table
struct FusedCall
{
    uint32_t offs; // block 0 | block 1 << 16
    uint32_t cnts; // nodes in block 0 | nodes in block 1 << 16 (0: a call of one block; both zero: end of list)
    uint32_t cls;  // dm_fused_class(degree, flip, leaf)
    uint32_t pad;
};
struct FusedPlan
{
    bool ok = false;
    int n_slots = 0;     // message slots
    int vnb = 0, cnl = 0; // largest number of variable-node blocks / of leaf calls any wave holds
    bool has_shortened = false;
    bool need_lambda = false; // a transmitted or shortened column of degree >= 3: its node keeps lambda_ch (detmath.h "Fused form")
    // a wave that serves a block through register-held offsets (slot 0, degree 3..15) serves no other, and no block goes
    // through the slot table: what the small instantiation of the kernel is compiled for
    bool wide_exclusive = false;
    // index of the compile-time wave program of this plan's shape (fused_program.hpp), or -1: the kernel interprets the plan
    int program = -1;
    std::vector<FusedCall> leaf_calls; // [kDecodeWaves][kFusedLeafCalls]
    std::vector<FusedCall> calls;      // [kDecodeWaves][calls_stride], each row ends in a zero entry
    int calls_stride = 0;
    // [kDecodeWaves][kFusedVnSlots][4]: nodes | degree << 16, offset into vn_slot, 0, 0 (nodes 0 = none).  Slot 0 holds the
    // wave's widest block; blocks of degree 2 sit in consecutive slots from an even one on (lock-step pairs).
    std::vector<uint32_t> vn_desc;
    // per wave, four bits per slot: what the variable-node pass does there (one scalar word instead of a handful of
    // loop-invariant conditions per slot that the compiler would keep in scalar registers for the whole decode)
    uint32_t vn_prog[kDecodeWaves] = {0, 0, 0, 0};
    std::vector<uint32_t> vn_slot;     // table path (degree >= 3 outside slot 0, or wider than 15): [off + p * count + lane]
    // [kDecodeWaves][kFusedLaneRows][64], what a lane keeps or needs once per frame:
    //   rows  0..7   slot w, degree 2: slot of edge 0 | slot of edge 1 << 16
    //   rows  8..15  slot 0, degree 3..15: slots of edges 2i, 2i+1 in word i
    //   rows 16..23  slot w: stage entry of the node's channel value (index among the transmitted bits; nct = shortened,
    //                nct + 1 = punctured / never written / no node), as a byte offset (x 16)
    //   rows 24..31  slot w: the node's column | kFusedCounted (its bit is one the error count visits); kFusedNone = no node
    //   rows 32..35  leaf call c, block h (row 32 + 2c + h): stage entry of the leaf's channel value
    //   rows 36..39  ... and the leaf's column | flags
    //   rows 40..43  ... and the message slot of the leaf's edge in the GENERAL plan (Plan::edge_slot: the hand-over)
    std::vector<uint32_t> lane_tab;
    std::vector<uint32_t> edge_slot;   // file-order edge -> slot, kNoSlot for an edge that ends in a leaf (tests)
    std::vector<uint32_t> ho_map;      // [n_slots] slot -> the same edge's slot in the general plan (the hand-over hands the
                                       // frame's c2v messages to the LLR-domain kernel in that plan's order)
};
constexpr uint32_t kFusedCounted = 0x80000000u, kFusedNone = 0xFFFFFFFFu;
enum : uint32_t { kFusedVnNone = 0, kFusedVnPair = 1 /* degree 2, 64 nodes */, kFusedVn2 = 2 /* degree 2 */, kFusedVnWide = 3 /* slot 0, degree 3..15 */, kFusedVnTable = 4 };
FusedPlan build_fused_plan(const LdpcCode &code, const Plan &plan);

Plan build_plan(const LdpcCode &code);
// plan for the decode_reg2_kernel<nt, kc, maxd, nv0, nv1> instantiation; ok = false when the code does not fit it
Reg2Plan build_reg2_plan(const LdpcCode &code, const Plan &plan, int nt, int kc, int maxd, int nv0, int nv1);
// `nt` threads, `kc` x `maxd` register tile = the kernel instantiation to plan for; lds_budget = bytes of LDS
// one workgroup may use for its mailbox
RegPlan build_reg_plan(const LdpcCode &code, const Plan &plan, int nt, int kc, int maxd, uint32_t lds_budget);

} // namespace ldpc_amd
