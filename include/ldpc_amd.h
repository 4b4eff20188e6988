/*
 * ldpc_amd.h — C ABI of libldpc.so, the MI355X-native drop-in for heat1q/libldpc's shared library.
 *
 * Part 1 re-exports, symbol for symbol and struct for struct, the six entry points of the
 * reference's src/shared.cpp:9-78 that pyLDPC/ldpc.py binds through ctypes, so an existing
 * `LDPC(pc_file, gen_file, lib="…/libldpc.so")` keeps working unchanged.
 * Part 2 is the batch interface the HIP path sits behind: the reference's per-frame virtual calls
 * (src/sim/channel.h:17-24 invoked at src/sim/ldpcsim.cpp:158-174) become one call per batch of
 * frames.  Plain pointers and sizes only; device pointers are accepted wherever a buffer is named
 * "device or host".
 */
#ifndef LDPC_AMD_H
#define LDPC_AMD_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ------------------------------------------------------------------------------------------ */
/* Part 1 — reference C ABI (src/core/functions.h:107-127, src/sim/ldpcsim.h:23-31)            */
/* ------------------------------------------------------------------------------------------ */
typedef struct
{
    bool earlyTerm;
    uint32_t iterations;
    const char *type; /* "BP_MS" selects min-sum, anything else sum-product (decoder.h:73-80) */
} decoder_param;

typedef struct
{
    uint64_t seed;
    double xRange[3]; /* MIN, MAX (exclusive), STEP */
    const char *type; /* "AWGN" | "BSC" | "BEC" */
} channel_param;

typedef struct
{
    uint32_t threads;  /* accepted for compatibility; the GPU batch replaces OpenMP threads */
    uint64_t maxFrames;
    uint64_t fec;
    const char *resultFile;
} simulation_param;

typedef struct
{
    double *fer;
    double *ber;
    double *avg_iter;
    double *time;
    uint64_t *fec;
    uint64_t *frames;
} sim_results_t;

/* replaces shared.cpp:11-24 — (re)creates the process-global code; file errors print and exit(1) */
void ldpc_setup(const char *pcFile, const char *genFile, int *n, int *m, int *nct, int *mct);
/* replaces shared.cpp:26-30 — blocks until done; writes results->x[i] per channel point; polls *stopFlag */
void simulate(decoder_param decoderParams, channel_param channelParam, simulation_param simParam,
              sim_results_t *results, bool *stopFlag);
/* replaces shared.cpp:32-35 */
int calculate_rank(void);
/* replaces shared.cpp:37-45 — infoWord[kct] -> codeWord[nct] (transmitted positions) */
void encode(uint8_t *infoWord, uint8_t *codeWord);
/* replaces shared.cpp:47-65 — llr[nct] in, llrOut[nct] out, returns the iteration count */
int decode(decoder_param decoderParams, double *llr, double *llrOut);
/* replaces shared.cpp:67-77 — word[nc] -> syndrome[mc] */
void syndrome(uint8_t *word, uint8_t *syndrome);

/* ------------------------------------------------------------------------------------------ */
/* Part 2 — batch interface (HIP shim)                                                         */
/* ------------------------------------------------------------------------------------------ */
typedef struct ldpc_hip_ctx ldpc_hip_ctx;

enum
{
    LDPC_HIP_AWGN = 1, /* ldpcsim.h:15-20 */
    LDPC_HIP_BSC = 2,
    LDPC_HIP_BEC = 3
};

/* outputs of a batch of n frames; each pointer is device or host memory, NULL = not wanted */
typedef struct
{
    uint32_t *iters;      /* [n]      iteration count as returned by ldpc_decoder::decode (decoder.cpp:74-77) */
    uint32_t *bit_errors; /* [n]      ldpcsim.cpp:184-188, transmitted positions only */
    uint8_t *hard;        /* [n][nc]  estimate() */
    double *llr_out;      /* [n][nc]  llr_out() (BEC: symbol values 0,1,'E') */
    double *llr_in;       /* [n][nc]  the decoder input the channel produced */
    uint8_t *codeword;    /* [n][nc]  transmitted codeword */
} ldpc_hip_out;

/* number of visible GPUs (0 when none); never throws */
int ldpc_hip_device_count(void);
/* message of the last failed ldpc_hip_* call on this thread */
const char *ldpc_hip_last_error(void);

/* parse the code (host only; the GPU is touched lazily by the first decode). NULL on error. */
ldpc_hip_ctx *ldpc_hip_create(const char *pcFile, const char *genFile, int device);
void ldpc_hip_destroy(ldpc_hip_ctx *ctx);
/* info[0..9] = nc, mc, nnz, nct, mct, kct, kc, max_degree, residency (0 memory, 1 LDS, 2 registers with a message
   mailbox, 3 registers with variable-node totals returned), lds_bytes_per_frame */
void ldpc_hip_code_info(const ldpc_hip_ctx *ctx, int64_t info[10]);
/* the text block the reference CLI prints for a code (ldpc.cpp:111-130); owned by the context */
const char *ldpc_hip_describe(ldpc_hip_ctx *ctx);
/* BEC: 1 = reproduce the reference's out-of-bounds read for erased degree-1 variable nodes
   (they emit 0); 0 (default) = defined semantics, they emit an erasure */
void ldpc_hip_set_bec_compat(ldpc_hip_ctx *ctx, int compat);
/* NON-PARITY modes for sum-product decoding ("BP"), off (0) by default and never chosen by the library itself; min-sum and
   BEC ignore them.  Error rates differ from the reference's within what profiles/ reports; iteration counts and decisions
   are not the reference's.
     1  flooding schedule, binary32 messages, LLRs clipped to +-27.7, hardware reciprocal / log2 / exp2
        (libldpc_amd/csrc/kernels_fast.hip)
     2  LAYERED (row-serial) schedule, binary32 check-to-variable messages: one wavefront per frame, a sweep is a sequence
        of conflict-free steps of up to 64 check nodes (libldpc_amd/csrc/kernels_layered.hip)
     3  the same with binary16 check-to-variable messages
   The reference has no such modes in src/ (its legacy gpu/ simulator uses single precision and processes H in layers,
   gpu/ldpc/ldpc.h, gpu/ldpc/ldpc.cpp:111-138: ideas only). */
void ldpc_hip_set_fast_mode(ldpc_hip_ctx *ctx, int mode);

/* Noise of the stream interface (ldpc_hip_stream_*, ldpc_hip_simulate*).  LDPC_HIP_NOISE_REFERENCE (the default) is the
   reference's own stream, mt19937_64(seed): every frame can be held bit for bit against the reference.
   LDPC_HIP_NOISE_COUNTER is NON-PARITY and not seed-comparable with the reference: a frame's noise is Philox4x32-10 of
   (seed, frame index since ldpc_hip_stream_begin, bit index), computed inside the decode launch, and the same seed gives the
   same frames on any number of GPUs and in any batch split.  Key (seed & 0xFFFFFFFF, seed >> 32), counter (block, frame low,
   frame high, tag); tag 0 AWGN: transmitted bit i is normal i % 4 of block i / 4, two binary32 Box-Muller pairs per block,
   u = (w0 + 0.5) / 2^32, angle w1 / 2^32 revolutions (so |n| <= sqrt(66 ln 2) = 6.764); tag 1 BSC / BEC: bit i flipped /
   erased when (w[i % 4] of block i / 4 + 0.5) / 2^32 < eps; tag 2 encoder (a generator matrix loaded): info bit j is bit
   j % 32 of word (j / 32) % 4 of block j / 128, and frame f's codeword is u_f G (no running sum over the frames); tag 3 the flip draws of ldpc_hip_bit_flip_batch and tag 4
   the gamma table of ldpc_hip_relay_decode_batch, both stated there (batch interface: no stream state).  Only error
   rates (statistically) compare with the reference; ldpc_hip_stream_skip is O(1), ldpc_hip_stream_raw_draws fails, a
   sharded step exchanges nothing.  Does not combine with ldpc_hip_set_fast_mode (ldpc_hip_stream_decode fails).  Part 1
   (simulate(), decode(), ...) always uses the reference stream. */
enum
{
    LDPC_HIP_NOISE_REFERENCE = 0,
    LDPC_HIP_NOISE_COUNTER = 1
};
/* takes effect at the next ldpc_hip_stream_begin; touches no GPU.  0, or -1 (last_error set) for an unknown mode */
int ldpc_hip_set_noise(ldpc_hip_ctx *ctx, int mode);
/* the counter mode's raw generator words: out[4 i + k] = word k of Philox4x32-10 block first_block + i of `frame` under
   `tag` and seed (n_blocks <= 2^32 - first_block); out is device or host memory.  For tests, as ldpc_hip_mt64 is for the
   reference stream.  0 on success */
int ldpc_hip_philox(ldpc_hip_ctx *ctx, uint64_t seed, uint32_t tag, uint64_t frame, uint32_t first_block, uint64_t n_blocks,
                    uint32_t *out, void *hip_stream);

/* Corrected min-sum of "BP_MS" decoding: normalized (scale alpha < 1) and offset (offset beta > 0) min-sum.  NON-PARITY
   unless (1, 0): the reference has plain min-sum only (decoder.h:17-20).  For check node c and its edge j:
     m_j   = the smallest |v2c| over the node's other edges (what plain min-sum computes, exactly)
     s_j   = XOR of the sign bits of the other edges' v2c (a zero carries its sign bit too)
     t     = fl(alpha * m_j)                 (rounded; no fused multiply-add)
     r     = fl(t - beta), and +0.0 where r is not greater than +0.0
     c2v_j = r with sign bit s_j
   Everything else is BP_MS as it is: v2c initialisation, the variable-node sum in column file order and v2c = out - c2v,
   the hard decision out <= 0, the syndrome early stop, the iteration counts, bit errors over transmitted positions,
   puncturing and shortening.  (1, 0) reproduces plain min-sum bit for bit and runs exactly today's kernels.
   Applies to ldpc_hip_decode_batch, ldpc_hip_stream_decode(_sharded) and ldpc_hip_simulate(_sharded) whenever the call's
   decoder_param.type is "BP_MS"; sum-product and the BEC ignore it; it combines with LDPC_HIP_NOISE_COUNTER.  Part 1
   (simulate(), decode(), ...) is plain min-sum always.
   Valid: 0 < scale <= 1 and 0 <= offset <= 1e6 (NaN and infinities fail).  Takes effect at the next decode call; touches no
   GPU.  0, or -1 (last_error set; the setting unchanged) for invalid values */
int ldpc_hip_set_min_sum_correction(ldpc_hip_ctx *ctx, double scale, double offset);

/* Schedule of "BP_MS" decoding.  LDPC_HIP_MS_SCHEDULE_FLOODING (the default) is the reference's.
   LDPC_HIP_MS_SCHEDULE_LAYERED is the layered (row-serial) schedule: NON-PARITY (the reference's schedule is flooding,
   decoder.cpp:22-76), off by default and never chosen by the library itself.
   Where it applies: whenever a call's decoder_param.type is "BP_MS" in ldpc_hip_decode_batch,
   ldpc_hip_stream_decode(_sharded) and ldpc_hip_simulate(_sharded).  Sum-product, the BEC decoder and Part 1 (simulate(),
   decode(), ...) never see it.  It combines with ldpc_hip_set_min_sum_correction and with both noise modes
   (ldpc_hip_set_noise).  ldpc_hip_decode_stages reports one `whole` launch for "BP_MS" while it is set and unchanged stages
   for "BP".
   Which codes it takes: every check node of degree 2..8, at most 65 535 columns, no isolated variable node, and the frame's
   LDS — 8 nc bytes of totals plus 20 bytes per check node (each step of the schedule rounded up to an even number of check
   nodes), ldpc_hip_layered_min_sum_lds_bytes — within 160 KB.  For any other code, and for an unknown `schedule` value, the
   setter returns -1 with ldpc_hip_last_error set and the setting unchanged.  The check is host-only; the setting takes
   effect at the next decode call and touches no GPU.  LAYERED is also refused while quantization, ternary min-sum or
   ldpc_hip_set_min_sum_layered_fixed (the same schedule in fixed point, a setting of its own) is on.
   Arithmetic: everything is binary64, every operation is rounded once, there is no fused multiply-add.
     1. T[v] := the frame's decoder input (channel LLR; punctured 0, shortened shorten_llr).  Every message m[c][j] := +0.0.
     2. One sweep visits the steps of the layered plan (libldpc_amd/csrc/plan.cpp, build_layer_plan: check nodes in file order
        within each degree, each put into the first step of its degree that has a free lane — 64 per step — and none of its
        variable nodes yet; steps ordered by their first check node) in order.  For each check node c of the step, with
        neighbours v_j:
          t_j = fl(T[v_j] - m[c][j])
          a_j = the smallest |t_k| over k != j
          s_j = XOR of the sign bits of t_k, k != j (a zero carries its sign bit)
          r_j = max(fl(fl(scale * a_j) - offset), +0.0), exactly the rule of ldpc_hip_set_min_sum_correction ((1, 0): a_j)
          m[c][j] := r_j with sign bit s_j
          T[v_j] := fl(t_j + m[c][j])
        The check nodes of a step share no variable node, so the result depends on the step order only.
     3. After every sweep hard = (T <= 0).  With early termination a zero syndrome stops the frame; iters = sweeps completed
        before the sweep whose syndrome passed (the reference's convention).  Otherwise iters = iterations.
     4. llr_out = T.
     5. bit_errors, llr_in and codeword are as everywhere.
     6. iterations == 0: hard and llr_out all zero (as the layered modes of ldpc_hip_set_fast_mode). */
enum
{
    LDPC_HIP_MS_SCHEDULE_FLOODING = 0,
    LDPC_HIP_MS_SCHEDULE_LAYERED = 1
};
int ldpc_hip_set_min_sum_schedule(ldpc_hip_ctx *ctx, int schedule);
/* the schedule in force (LDPC_HIP_MS_SCHEDULE_*); ctx is a live context, as for every entry that takes one */
int ldpc_hip_min_sum_schedule(const ldpc_hip_ctx *ctx);
/* LDS bytes one frame of layered min-sum takes on this context's code (host only; worked out once per context), -1 where the
   layered plan does not take the code, or on an error (last_error set) */
int64_t ldpc_hip_layered_min_sum_lds_bytes(const ldpc_hip_ctx *ctx);

/* Quantized (fixed-point) min-sum: "BP_MS" decoding with messages of `bits` bits on a saturating integer datapath and the
   LLR step `step` — the decoder that is built in hardware.  NON-PARITY (the reference's min-sum is binary64,
   decoder.cpp:22-76), off by default and never chosen by the library itself.
   bits 0 = off (the default; step ignored), 2..8 = on.  The setter is host-only and takes effect at the next decode call.
   It returns -1 with ldpc_hip_last_error set and the setting unchanged for bits outside {0, 2..8}, for a step that is NaN,
   infinite, <= 0 or outside [2^-20, 2^20], for a code it does not take, and while LDPC_HIP_MS_SCHEDULE_LAYERED is in force
   (ldpc_hip_set_min_sum_schedule(LAYERED) in turn returns -1 while quantization is on), and while
   ldpc_hip_set_min_sum_layered_fixed is on.
   Where it applies: whenever a call's decoder_param.type is "BP_MS" in ldpc_hip_decode_batch,
   ldpc_hip_stream_decode(_sharded) and ldpc_hip_simulate(_sharded).  Sum-product, the BEC decoder and Part 1 never see it.
   It combines with both noise modes (ldpc_hip_set_noise) and with ldpc_hip_set_min_sum_correction (through the table of
   item 3).  ldpc_hip_decode_stages reports one `whole` launch for "BP_MS" while it is on and unchanged stages for "BP".
   Which codes it takes: every code the library loads — any check-node degree >= 2, any column degree, isolated columns
   included — with at most 65 535 columns and the frame's LDS (below) within 160 KB.
   Arithmetic, with q = bits, D = step, Qmax = 2^(q-1) - 1 (symmetric: there is no -2^(q-1)) and inv = fl(1 / D), computed
   once on the host in binary64:
     1. Channel.  llr = the frame's decoder input as everywhere (binary64; punctured columns 0, shortened columns
        shorten_llr).  It is quantized once: L[v] = clamp(rint(fl(llr[v] * inv)), -Qmax, +Qmax), rint = round-half-to-even,
        the clamp applied in binary64 before the conversion to an integer (an infinity and 99999.9 saturate; a NaN gives
        0).  The llr_in output stays the unquantized binary64 value.
     2. Start.  v2c[e] = L[col(e)].
     3. Correction table, built on the host from ldpc_hip_set_min_sum_correction(scale, offset): for m = 0..Qmax
        lut[m] = max(0, (int) rint(fl(fl(scale * m) - fl(offset * inv)))), binary64, every operation rounded once, no
        fused multiply-add.  (1, 0) gives the identity.  lut is non-decreasing, so applying it after the minimum equals
        applying it before.  The kernel sees the table only (at most 128 bytes), never scale or offset.
     4. Check node c, edge j: magnitude = lut[min over k != j of |v2c_k|]; negative iff an odd number of the other v2c_k
        are < 0 (an integer zero is not negative); c2v_j = +-magnitude.
     5. Variable node v: A[v] = L[v] + the sum of its c2v (an exact integer sum in 32 bits: the order does not matter);
        v2c_e = clamp(A[v] - c2v_e, -Qmax, +Qmax); hard[v] = (A[v] <= 0), the reference's convention: a tie decides 1.
     6. Schedule and stop: flooding, the syndrome early stop and the iteration count of the reference, exactly as for
        "BP_MS" without quantization: iters = the index of the iteration whose decisions passed the syndrome check,
        otherwise iters = iterations.  iterations == 0: hard and llr_out all zero, as the other min-sum kernels.
     7. llr_out[v] = fl((double) A[v] * D).  bit_errors and codeword are as everywhere. */
int ldpc_hip_set_min_sum_quantization(ldpc_hip_ctx *ctx, int bits, double step);
/* the setting in force: *bits (0 = off) and *step (the last step set; 1.0 before any); either pointer may be null */
int ldpc_hip_min_sum_quantization(const ldpc_hip_ctx *ctx, int *bits, double *step);
/* LDS bytes one frame of quantized min-sum takes on this context's code (host only; worked out once per context), -1 for a
   code it does not take, or on an error (last_error set).  With `slots` = the check-node degrees, each rounded up to a
   multiple of 4, summed (one byte per message, a check node's messages padded to whole words):
     bytes = max(8 nc, slots + 4 nc + 144) rounded up to 4, + nc, rounded up to 16
   — the nc binary64 channel LLRs first, later reused for the messages, the nc 32-bit totals, the 128-byte table and 16
   bytes of the workgroup's vote; behind them the nc quantized channel values. */
int64_t ldpc_hip_quantized_min_sum_lds_bytes(const ldpc_hip_ctx *ctx);

/* Ternary min-sum (Gallager's Algorithm E): "BP_MS" decoding with messages in {-1, 0, +1} and the channel weight w, the
   hard-decision message passing of a BSC or of a hard-decision front end.  NON-PARITY (the reference's min-sum is binary64,
   decoder.cpp:22-76), off by default and never chosen by the library itself.
   weight 0 = off (the default), 1..7 = on with channel weight w.  The setter is host-only and takes effect at the next
   decode call.  It returns -1 with ldpc_hip_last_error naming it and the setting unchanged for a weight outside 0..7, for a
   code it does not take, and while LDPC_HIP_MS_SCHEDULE_LAYERED or quantization is in force; ldpc_hip_set_min_sum_schedule(
   LAYERED) and ldpc_hip_set_min_sum_quantization(bits > 0) in turn return -1 while it is on: of the three, at most one.
   (ldpc_hip_set_min_sum_layered_fixed is the fourth of the kind: each of the four returns -1 while another is in force.)
   Where it applies: whenever a call's decoder_param.type is "BP_MS" in ldpc_hip_decode_batch,
   ldpc_hip_stream_decode(_sharded) and ldpc_hip_simulate(_sharded).  Sum-product, the BEC decoder and Part 1 never see it.
   It combines with both noise modes (ldpc_hip_set_noise).  While it is on ldpc_hip_set_min_sum_correction has no effect (there
   is no magnitude to correct), ldpc_hip_decode_stages reports one `whole` launch for "BP_MS" (unchanged stages for "BP") and
   ldpc_hip_decoder_choice returns 6.
   Which codes it takes: at most 65 535 columns (and edges), any check-node degree >= 2, column degree <= 56 (so |A| <= 63);
   isolated, punctured and shortened columns are fine; the LDS of one 32-frame group (below) within 160 KB.  There is no
   byte-per-message fallback: a code beyond that is refused.  A code whose every check node sees two or more punctured
   columns (tests/golden/h.txt) is taken and decodes nothing: every message stays zero.
   Arithmetic, all integer, so every output bit is determined:
     1. r[v] = +1 where the frame's decoder input llr[v] > 0, -1 where it is < 0, 0 for +-0 and NaN: punctured columns 0,
        shortened columns +1, +-infinity +-1.  The llr_in output stays the binary64 value.
     2. v2c[e] = r[col(e)].
     3. Check node c, edge j: c2v_j = the product of v2c_k over k != j (0 if any other input is 0).
     4. Variable node v: A[v] = w r[v] + the sum of its c2v; v2c_e = sgn(A[v] - c2v_e); hard[v] = 1 iff 2 A[v] + r[v] <= 0:
        a tie A = 0 goes to the received bit (the decoder stays symmetric, all-zero-codeword simulation stays valid), and to 1,
        the library's convention, where there is none.
     5. Schedule and stop: flooding, the syndrome early stop and the iteration count of the reference, exactly as for
        "BP_MS" (decoder.cpp:22-77): iters = the iterations completed before the one whose decisions passed the syndrome
        check, otherwise iters = iterations.  iterations == 0: hard and llr_out all zero.
     6. llr_out[v] = (double) A[v] of the last iteration the frame ran.  bit_errors and codeword are as everywhere.
     7. A frame's results do not depend on which other frames share its group or batch: 32 consecutive frames of a batch are
        decoded by one workgroup, bit f of every word being frame f, and a frame that stops is frozen while its group goes on. */
int ldpc_hip_set_min_sum_ternary(ldpc_hip_ctx *ctx, int weight);
/* the weight in force (0 = off) */
int ldpc_hip_min_sum_ternary(const ldpc_hip_ctx *ctx);
/* LDS bytes one 32-frame group of ternary min-sum takes on this context's code (host only), -1 for a code the setter
   refuses.  In 4-byte words: 64 (the group's votes and error counts) + 2 max(nnz, nc) (the messages' Z and S words, over which
   the channel prologue first stages one frame's nc binary64 LLRs) + 3 nc (r = +1, r = -1, the decisions) + P nc (the planes
   of A in two's complement, P = 1 + the bits of (largest column degree + 7): kept for llr_out, left out of a launch that
   does not want it); then 4 nnz bytes (two u16 per edge: the variable nodes' slot table and slot -> column for the syndrome),
   all rounded up to 16. */
int64_t ldpc_hip_ternary_lds_bytes(const ldpc_hip_ctx *ctx);

/* Fixed-point layered min-sum: "BP_MS" decoding on the layered (row-serial) schedule with messages of `msg_bits` bits, a
   saturating a-posteriori total (APP) of `app_bits` bits per column and the LLR step `step` — the datapath of hardware
   decoders (5G NR, 802.11, DVB-S2).  NON-PARITY (the reference's min-sum is flooding and binary64, decoder.cpp:22-76), off
   by default and never chosen by the library itself.
   msg_bits 0 = off (the default; the other arguments are then ignored), 2..8 = on; on needs msg_bits <= app_bits <= 16 and
   2^-20 <= step <= 2^20 (a NaN fails).  The setter is host-only and takes effect at the next decode call.  It returns -1
   with ldpc_hip_last_error naming ldpc_hip_set_min_sum_layered_fixed and the setting unchanged for invalid values, for a code
   it does not take, and while LDPC_HIP_MS_SCHEDULE_LAYERED, quantization or ternary min-sum is in force;
   ldpc_hip_set_min_sum_schedule(LAYERED), ldpc_hip_set_min_sum_quantization(bits > 0) and ldpc_hip_set_min_sum_ternary(weight
   > 0) in turn return -1 while it is on: of the four, at most one is in force.
   Where it applies: whenever a call's decoder_param.type is "BP_MS" in ldpc_hip_decode_batch,
   ldpc_hip_stream_decode(_sharded) and ldpc_hip_simulate(_sharded).  Sum-product, the BEC decoder and Part 1 never see it.
   It combines with both noise modes (ldpc_hip_set_noise) and with ldpc_hip_set_min_sum_correction (through the table of
   item 3).  While it is on ldpc_hip_decode_stages reports one `whole` launch for "BP_MS" (unchanged stages for "BP") and
   ldpc_hip_decoder_choice returns 7.
   Which codes it takes: those of the layered schedule, on the same plan (libldpc_amd/csrc/plan.cpp, build_layer_plan, built
   once per context): every check node of degree 2..8, at most 65 535 columns, no isolated variable node, and the frame's LDS
   (below) within 160 KB.
   Arithmetic, all integer after the quantizer, so every output bit is determined.  q = msg_bits, p = app_bits, D = step,
   Qmax = 2^(q-1) - 1, Pmax = 2^(p-1) - 1 (both symmetric), inv = fl(1 / D), computed once on the host in binary64:
     1. Channel.  L[v] = clamp(rint(fl(llr[v] * inv)), -Qmax, +Qmax), exactly item 1 of ldpc_hip_set_min_sum_quantization:
        the clamp applied in binary64, a NaN gives 0, punctured columns give 0, shortened columns and infinities saturate at
        +-Qmax.  The llr_in output stays the unquantized binary64 value.
     2. Start.  T[v] := L[v].  Every message m[c][j] := 0.
     3. Correction table.  lut[0..Qmax] is exactly item 3 of ldpc_hip_set_min_sum_quantization, built on the host with the
        same routine from ldpc_hip_set_min_sum_correction(scale, offset).  The kernel sees the table only, never scale or
        offset.  The table is non-decreasing.
     4. One sweep visits the steps of the layered plan in order (ldpc_hip_set_min_sum_schedule, item 2).  For each check node
        c of the step, with neighbours v_j:
          t_j = T[v_j] - m[c][j]                  (an exact integer; |t_j| <= Pmax + Qmax)
          u_j = clamp(t_j, -Qmax, +Qmax)          (the variable-to-check message at message width)
          a_j = the smallest |u_k| over k != j
          m[c][j] := +-lut[a_j], negative iff an odd number of the other u_k are < 0 (an integer zero is not negative)
          T[v_j] := clamp(t_j + m[c][j], -Pmax, +Pmax)
        The check nodes of a step share no variable node, so the result depends on the step order only.
     5. After every sweep hard = (T <= 0).  With early termination a zero syndrome stops the frame; iters = sweeps completed
        before the sweep whose syndrome passed.  Otherwise iters = iterations.  (As layered min-sum does it.)
     6. llr_out[v] = fl((double) T[v] * D).  bit_errors, codeword and llr_in are as everywhere.
     7. iterations == 0: hard and llr_out all zero. */
int ldpc_hip_set_min_sum_layered_fixed(ldpc_hip_ctx *ctx, int msg_bits, int app_bits, double step);
/* the setting in force: *msg_bits (0 = off), *app_bits and *step (the last ones set; 8 and 1.0 before any); any pointer may
   be null */
int ldpc_hip_min_sum_layered_fixed(const ldpc_hip_ctx *ctx, int *msg_bits, int *app_bits, double *step);
/* LDS bytes one frame of fixed-point layered min-sum takes on this context's code (host only; worked out once per
   context), -1 for a code it does not take, or on an error (last_error set).  With R = the check-node slots of the layered
   plan (each step's check nodes rounded up to an even number, summed):
     bytes = max(8 nc, round4(2 nc) + 4 R) + 128, rounded up to 16
   — the nc binary64 channel LLRs first; over them the int16 totals and, from the next multiple of 4, one 32-bit record per
   slot; behind the larger of the two the 128-byte correction table.  tests/golden/h.txt: 9 344 bytes, 17 frames per CU. */
int64_t ldpc_hip_layered_fixed_lds_bytes(const ldpc_hip_ctx *ctx);

/* decode n frames of given LLRs llr_in[n][nc] (column order, device or host). 0 on success.
   Which values a caller may hand in, for "BP" and "BP_MS" (tests/test_gpu_edge_llrs.py, tests/edge_llrs.py):
     - Finite values of any magnitude — signed zeros, subnormals, values on the limits the arithmetic forms switch at
       (detmath.h: 2^-52, 40, ln 2^220, 166, ln 2^240, 600, 700 ...), 1e300 — and infinities, as long as the reference's
       arithmetic makes no NaN of them, are decoded bit for bit as the det-mode oracle decodes them: iters, hard, bit_errors,
       llr_out and llr_in.  A frame that holds an input 0 < |L| < 2^-52 (e^L rounds to exactly 1.0 and the sign of L would be
       lost) or |L| > 166 never takes the likelihood-ratio forms, and a check node that receives such a tiny message is
       evaluated with the reference's expression term by term (detmath.h, dm_ratio_llr_refused, dm_llr_tiny): a tiny positive
       LLR decides 0 and a frame of tiny LLRs converges as in the reference.
     - A frame in which the reference's arithmetic makes a NaN — a NaN input; infinite inputs on all or all but one of the
       neighbours of one check node (two of the three of a degree-3 node: the third receives +-inf and answers inf - inf) —
       has unspecified outputs within iters <= dec.iterations and hard in {0, 1}.  The same call on the same batch gives the
       same bits again.  (Min-sum takes its minima with v_min_f64, which drops a NaN operand where the reference's std::min
       keeps or drops it by position: profiles/README.md, "Class-N frames", lists what each decoder returns.)
     - Such a frame never affects another frame of the batch. */
int ldpc_hip_decode_batch(ldpc_hip_ctx *ctx, decoder_param dec, uint64_t n, const double *llr_in,
                          const ldpc_hip_out *out, void *hip_stream);

/* ldpc_hip_decode_batch for LLRs of another element type, and decisions packed 32 to a word.  llr_in[n][nc] is in column
   order, in device or host memory, its elements of llr_type; host input is staged to the device in its own type (inputs of up
   to 1 MB through page-locked memory, as for ldpc_hip_decode_batch).
   The call decodes the WIDENED array W[n][nc], binary64:
     LDPC_HIP_LLR_F64  W = the value itself;
     LDPC_HIP_LLR_F32, LDPC_HIP_LLR_F16 (IEEE binary16)  W = the value widened to binary64, which is exact: NaN stays NaN,
                       infinities and signed zeros are kept, binary16 subnormals become exact doubles.  W is then under
                       the contract of ldpc_hip_decode_batch for non-finite inputs: a value beyond the type's range is an
                       infinity in W (binary16: beyond 65504, so a shortened column's 99999.9), and a code with two
                       shortened columns on one check node of degree 3 — tests/orc.py shortened_variant — then holds two
                       infinities there: outputs unspecified, though still equal to ldpc_hip_decode_batch on W;
     LDPC_HIP_LLR_I8   an element k stands for W = fl((double) k * D), D = the `step` of the fixed-point mode in force: what a
                       demapper with q-bit outputs delivers.  Accepted only when dec.type is "BP_MS" and
                       ldpc_hip_set_min_sum_quantization or ldpc_hip_set_min_sum_layered_fixed is on; otherwise (sum-product,
                       plain, layered or ternary min-sum) the call returns -1 and ldpc_hip_last_error names
                       ldpc_hip_decode_batch_typed.  Values beyond +-Qmax saturate in the quantizer like any other LLR.
   An unknown llr_type returns -1 in the same way.  These checks run before anything touches the GPU; after them n == 0
   returns 0.
   Every output in *out equals, bit for bit, what ldpc_hip_decode_batch returns for W under the same settings — iters,
   bit_errors, hard, llr_out, llr_in (which is W) and codeword, for every decoder, mode and combination that call takes — and
   the typed call fails wherever that call fails.  LDPC_HIP_LLR_F64 is ldpc_hip_decode_batch itself.
   hard_bits[n][ceil(nc / 32)] (device or host memory, NULL = not wanted; independent of out->hard, which may be NULL): bit
   c & 31 of word c >> 5 of a frame's row is hard[c]; the unused high bits of a row's last word are 0; iterations == 0 gives
   rows of zeros.
   The call changes nothing about later calls: no setting, no state.
   How it runs: fixed-point layered min-sum (ldpc_hip_decoder_choice returns 7) reads F32, F16 and I8 input itself and stages
   no binary64 value in LDS (ldpc_hip_layered_fixed_direct_lds_bytes; I8 is clamp(k, -Qmax, +Qmax), which equals item 1 of
   ldpc_hip_set_min_sum_layered_fixed applied to W for every int8 k and every valid step); every other decoder gets W from
   one conversion launch in front of its own.  hard_bits comes from one small launch behind the decoder's. */
enum
{
    LDPC_HIP_LLR_F64 = 0,
    LDPC_HIP_LLR_F32 = 1,
    LDPC_HIP_LLR_F16 = 2,
    LDPC_HIP_LLR_I8 = 3
};
int ldpc_hip_decode_batch_typed(ldpc_hip_ctx *ctx, decoder_param dec, uint64_t n, const void *llr_in, int llr_type,
                                const ldpc_hip_out *out, uint32_t *hard_bits, void *hip_stream);
/* LDS bytes one frame of fixed-point layered min-sum takes when ldpc_hip_decode_batch_typed feeds it F32, F16 or I8 input
   (host only; worked out once per context), -1 for a code the layered plan refuses, or on an error (last_error set).  With R
   as for ldpc_hip_layered_fixed_lds_bytes:
     bytes = round4(2 nc) + 4 R + 128, rounded up to 16
   — the int16 totals, from the next multiple of 4 one 32-bit record per slot, behind them the 128-byte correction table; no
   binary64 channel LLRs.  tests/golden/h.txt: 6 528 bytes, 25 frames per CU. */
int64_t ldpc_hip_layered_fixed_direct_lds_bytes(const ldpc_hip_ctx *ctx);

/* Frames of bits that stay on the device: the transmit side of ldpc_hip_decode_batch_typed and its check,
     ldpc_hip_encode_batch -> ldpc_hip_channel_batch -> ldpc_hip_decode_batch_typed -> ldpc_hip_syndrome_batch,
     ldpc_hip_bit_errors_batch
   with packed words passing from one call to the next.  The GF(2) calls are pure: every output bit is determined
   (ldpc_hip_channel_batch states its own contract below).
   Common rules.  Every buffer is device or host memory (host buffers are staged; inputs and results of up to 1 MB through
   page-locked memory; device buffers are used in place).  An output pointer may be NULL = not wanted.  A row of L bits is
     LDPC_HIP_BITS_U8        L bytes, a non-zero byte is 1 (as encode() reads its input); outputs are 0 / 1;
     LDPC_HIP_BITS_PACKED32  ceil(L / 32) words, the layout of hard_bits: bit i & 31 of word i >> 5.  On input the bits of a
                             row's last word from L on are ignored, on output they are 0.
   The argument checks (an unknown format value, a missing input, and what each entry names below) run before anything
   touches the GPU: they return -1 and ldpc_hip_last_error names the entry.  After them n == 0 returns 0.  Work is ordered on
   hip_stream; with host outputs the call returns after they are written.  No call reads or changes a setting or any state of
   the stream interface: a running ldpc_hip_stream_* sequence gives the same frames with or without these calls in between. */
enum
{
    LDPC_HIP_BITS_U8 = 0,
    LDPC_HIP_BITS_PACKED32 = 1
};
/* info[n][kc] (kc = info[6] of ldpc_hip_code_info) -> codeword[n][nc] bytes and / or codeword_bits[n][ceil(nc / 32)], both in
   COLUMN order: the layout of ldpc_hip_out.codeword, not the transmitted-positions order of Part 1.
   codeword[f][j] = XOR of info[f][i] over the entries (i, j) of the generator file: an entry listed twice cancels (as in the
   stream encoder's masks and its walk), columns from G.cols up to nc are 0, rows of G the file leaves out contribute nothing,
   and there is no running sum over the frames.  Two identities:
     - for info whose bits from kct on are 0, encode() of Part 1 returns codeword[f][bit_pos[i]] at transmitted position i;
     - with LDPC_HIP_NOISE_COUNTER the stream's frame f has codeword = ldpc_hip_encode_batch(u_f), u_f its information bits of
       Philox tag 2 as specified above.
   Fails (host only) when the context has no generator matrix, when G.rows > kc (the stream encoder's rule), and when the
   column-mask table below would exceed 256 MiB.
   How it runs: the columns of G as bit masks over the information word, nc x ceil(kc / 32) words, are built on the host at
   the context's first encode call (a context that never encodes pays nothing); byte information is packed by one small
   launch in front; the product is one launch per 2^20 frames at most (libldpc_amd/csrc/kernels_gf2.hip). */
int ldpc_hip_encode_batch(ldpc_hip_ctx *ctx, uint64_t n, const void *info, int info_format, uint8_t *codeword,
                          uint32_t *codeword_bits, void *hip_stream);
/* word[n][nc] (column order) -> syndrome[n][mc] bytes 0 / 1, syndrome_bits[n][ceil(mc / 32)] and weight[n], the number of
   unsatisfied check nodes of the frame.  syndrome[f][r] = XOR of word[f][c] over the entries (r, c) of H as the library
   loaded it (an entry listed twice counts twice); for 0 / 1 input that is what syndrome() of Part 1 returns.  Works on every
   code the library loads up to 524 288 columns (a frame's packed word is staged in LDS; beyond, -1) and needs no generator. */
int ldpc_hip_syndrome_batch(ldpc_hip_ctx *ctx, uint64_t n, const void *word, int word_format, uint8_t *syndrome,
                            uint32_t *syndrome_bits, uint32_t *weight, void *hip_stream);
/* bit_errors[f] = the number of transmitted positions (the bit_pos set: punctured and shortened columns left out) at which
   rows f of a[n][nc] and b[n][nc] differ, each operand in its own format: the count of ldpcsim.cpp:184-188.  Fed out->hard
   and out->codeword of a stream decode it returns that call's out->bit_errors. */
int ldpc_hip_bit_errors_batch(ldpc_hip_ctx *ctx, uint64_t n, const void *a, int a_format, const void *b, int b_format,
                              uint32_t *bit_errors, void *hip_stream);

/* The channel between the encoder and the decoder: modulation, noise, demapper and the quantizer in one launch
   (libldpc_amd/csrc/kernels_channel.hip).  codeword[n][nc] in, LLRs in the element type the decoder reads out; the common
   rules above hold (device or host buffers, checks before the GPU, n == 0 returns 0 after them, ordered on hip_stream, no
   setting read or changed, the stream interface's state untouched — the channel point and the noise mode of
   ldpc_hip_stream_begin / ldpc_hip_set_noise included: everything the call uses is in *ch).
   Buffers.  codeword[n][nc], column order, LDPC_HIP_BITS_U8 or LDPC_HIP_BITS_PACKED32 (what ldpc_hip_encode_batch writes);
   NULL = the all-zero codeword.  llr[n][nc], column order, elements of ch->llr_type; may be NULL.  received[n][S], binary64,
   S = ceil(nct / m) symbols per frame; may be NULL.  Every element of a wanted output is written exactly once: the caller
   need not clear it.
   Refused (host only, -1, ldpc_hip_last_error names ldpc_hip_channel_batch): a null ch; an unknown channel, format or type;
   m outside 1..4, or m != 1 with the BSC; a non-finite x for AWGN; x outside (0, 1) for the BSC; with LDPC_HIP_LLR_I8 q_bits
   outside 2..8 or step outside [2^-20, 2^20]; both outputs NULL with n > 0.  (The BEC is not offered: its decoder takes symbols.)
   Arithmetic.  NON-PARITY, the noise of LDPC_HIP_NOISE_COUNTER: every bit of llr is determined given received, and received
   is determined up to the hardware's binary32 log / sqrt / sin / cos, as for that mode.  Binary64 throughout, every operation
   rounded once, no fused multiply-add.
     Setup.  i = 0..nct-1 are the transmitted positions, bit_pos[i] their columns; only those columns of the codeword are read,
       a non-zero byte counts as 1.  Symbol s carries the bits i = m s + k, k = 0..m-1; a bit beyond nct - 1 counts as 0.
       AWGN: sigma2 = pow(10, -x / 10), sigma = sqrt(sigma2); BSC: delta = log((1 - x) / x) — the host expressions of
       ldpc_hip_stream_begin.
     AWGN noise.  Symbol s takes normal s % 4 of Philox block s / 4 of frame first_frame + f under tag 0 (ldpc_hip_set_noise:
       the Box-Muller pairs specified there); noise = (double) normal * sigma + 0.0.
     AWGN, m = 1.  a = 1 - 2 bit, y = noise + a, received = y, llr = (2 * y) / sigma2: the operations of the stream's channel.
     AWGN, m = 2..4 (M = 2^m).  Levels level[j] = (double) (M - 1 - 2 j) * c for j = 0..M-1, c = 1.0 / sqrt((double) (M * M - 1)
       / 3.0), built once on the host: unit mean energy; the kernel sees the table only.  g = the symbol's m bits, the first
       the most significant; the level index j is the inverse Gray code of g: j ^ (j >> 1) == g.  y = noise + level[j],
       received = y.  Max-log demapping: d_j = (y - level[j]) * (y - level[j]) for every j; for bit k D0 = the smallest d_j over
       the levels whose label j ^ (j >> 1) has bit k = 0, D1 the same for bit k = 1; llr = (D1 - D0) / (2 * sigma2).  The LLRs
       of padding bits are written nowhere.  Two such dimensions form a square 2^(2m)-QAM symbol: the error rates at the
       per-dimension x are those of QPSK, 16-, 64- and 256-QAM.  There is no complex interface.
     BSC.  ybit = bit ^ hit, hit = ((word i % 4 of block i / 4 under tag 1) + 0.5) / 2^32 < x; received = (double) (1 - 2 ybit);
       llr = delta * received.
     Other columns.  Punctured and unconnected columns get +0.0; shortened columns 99999.9 (AWGN) or delta (BSC): the stream's
       values.
     For m = 1 the rows of llr (LDPC_HIP_LLR_F64) equal, bit for bit, out->llr_in of ldpc_hip_stream_decode under
       LDPC_HIP_NOISE_COUNTER, the same channel, x and seed, for the stream's frames first_frame + f and their codewords.
     Element type, L the binary64 value above.  LDPC_HIP_LLR_F64: L.  LDPC_HIP_LLR_F32: L rounded to nearest-even.
       LDPC_HIP_LLR_F16: that binary32 value rounded to nearest-even (two roundings); 99999.9 becomes +infinity, which the
       decoders widen back to +infinity (two such columns on one check node: the non-finite contract at ldpc_hip_decode_batch).
       LDPC_HIP_LLR_I8: clamp(rint(fl(L * inv)), -Qmax, +Qmax), inv = fl(1 / step), Qmax =
       2^(q_bits - 1) - 1: item 1 of ldpc_hip_set_min_sum_quantization, the clamp applied in binary64, a NaN gives 0 — feed it to
       ldpc_hip_decode_batch_typed under a fixed-point mode of the same step.
   How it runs: one launch per 2^31 / (lanes per frame) frames at most; a lane owns one Philox block of a frame — four symbols,
   4 m bits — and further lanes fill the columns the channel does not write; no LDS. */
typedef struct
{
    int channel;          /* LDPC_HIP_AWGN or LDPC_HIP_BSC */
    double x;             /* AWGN: Es / sigma^2 in dB; BSC: crossover probability (ldpc_hip_stream_begin's meaning) */
    uint64_t seed;        /* Philox key, as LDPC_HIP_NOISE_COUNTER takes it */
    uint64_t first_frame; /* row f of the call is frame first_frame + f of that noise */
    int bits_per_symbol;  /* m: AWGN 1..4 (2^m-ASK per real dimension), BSC 1 */
    int llr_type;         /* LDPC_HIP_LLR_F64 / F32 / F16 / I8: element type of llr */
    int q_bits;           /* LDPC_HIP_LLR_I8 only: 2..8 */
    double step;          /* LDPC_HIP_LLR_I8 only: 2^-20..2^20 */
} ldpc_hip_channel;
int ldpc_hip_channel_batch(ldpc_hip_ctx *ctx, const ldpc_hip_channel *ch, uint64_t n, const void *codeword,
                           int codeword_format, void *llr, double *received, void *hip_stream);

/* The third channel and its decoder, for a caller who holds received words with holes in them:
     ldpc_hip_encode_batch -> ldpc_hip_erasure_channel_batch -> ldpc_hip_erasure_decode_batch -> ldpc_hip_syndrome_batch,
     ldpc_hip_bit_errors_batch
   (libldpc_amd/csrc/kernels_erasure.hip).  The common rules of this block hold for both calls: device or host buffers,
   checks before the GPU naming the entry in ldpc_hip_last_error, n == 0 returns 0 after them, ordered on hip_stream, no
   setting and no state of the stream interface read or changed.  Every output bit is determined.  W = ceil(nc / 32); a
   packed row is the layout of hard_bits / LDPC_HIP_BITS_PACKED32.

   The erasure channel.  codeword[n][nc], column order, LDPC_HIP_BITS_U8 or LDPC_HIP_BITS_PACKED32; NULL = the all-zero
   codeword.  word_bits[n][W] and erased_bits[n][W]: either may be NULL, not both when n > 0.  Refused (host only, -1): an
   unknown format, eps outside (0, 1) — the endpoints and a NaN included —, both outputs NULL with n > 0.
   Per column c of frame first_frame + f:
     - c = bit_pos[i] for an i < nct, a transmitted position: erased iff (w + 0.5) / 2^32 < eps (binary64, exact), w = word
       i % 4 of Philox block i / 4 of the frame under tag 1 and `seed`: exactly the draw of LDPC_HIP_NOISE_COUNTER for the BEC
       (ldpc_hip_set_noise);
     - a punctured column (one listed as both punctured and shortened counts as shortened): erased;
     - every other column — shortened ones, the surplus positions a column in both lists leaves in bit_pos, unconnected
       ones —: known, carrying the codeword's bit of THAT column.  Deliberately not the stream channel's value for a
       shortened column, which the reference reads from the transmitted-symbol vector at the column's index
       (channel.cpp:222);
     - word = the codeword's bit & ~erased everywhere; the bits of a row's last word from nc on are 0 in both outputs.
   For a code without shortened columns erased_bits and word_bits are, bit for bit, (llr_in == 69) and (llr_in == 1) of
   ldpc_hip_stream_decode on the BEC under LDPC_HIP_NOISE_COUNTER, the same eps and seed, for the stream's frames
   first_frame + f and their codewords.
   How it runs: one launch per 2^31 / W frames at most, no LDS; a lane owns one output word of a frame — 32 columns — and
   writes it once, with the Philox block of the last transmitted index in registers: where bit_pos is consecutive every
   block is computed once. */
int ldpc_hip_erasure_channel_batch(ldpc_hip_ctx *ctx, double eps, uint64_t seed, uint64_t first_frame, uint64_t n,
                                   const void *codeword, int codeword_format, uint32_t *word_bits, uint32_t *erased_bits,
                                   void *hip_stream);
/* The erasure decoder (flooding, peeling): word[n][nc] and erased[n][nc] in, both in `format` (LDPC_HIP_BITS_U8: a non-zero
   byte is 1 / erased; LDPC_HIP_BITS_PACKED32: the bits of a row's last word from nc on are ignored); word_out[n][W],
   erased_out[n][W], iters[n] and unresolved[n] out, each may be NULL.  It needs no generator matrix, no codeword and no
   knowledge of what was sent (the stream's BEC decoder compares every message with the transmitted bit).  Refused (host
   only, -1): an unknown format, a bit of `flags` other than the two below, a missing input with n > 0, and a code whose
   group does not fit (ldpc_hip_erasure_lds_bytes returns -1; there is no other kernel).
   Per frame, E the set of erased columns and V the set of columns of value 1; a value under an erased bit is ignored:
   V := word & ~E on entry.
     1. Pass I = 0 .. iterations - 1, while the frame is active.  For every check node r, over the entries of H as the
        library loaded it (an entry listed twice is two edges):
          c0[r] = some edge's column is in E;  c1[r] = two or more edges' columns are in E;
          xa[r] = XOR over the edges of (column in V).
     2. For every column v in E: res = OR over its edges (r, v) of (c0[r] & ~c1[r]), val = OR over them of (c0[r] & ~c1[r] &
        xa[r]).  If res, v leaves E, and enters V iff val.  All of step 2 reads the c0 / c1 / xa of step 1: a flooding pass.
        (For a codeword with erasures every resolving check node agrees; the OR is the rule for inconsistent input.)
     3. The frame still holds an erasure iff E is non-empty over all nc columns, punctured, unconnected and degree-0 ones
        included.  With LDPC_HIP_ERASURE_EARLY_TERM a frame whose pass left E empty stops; with
        LDPC_HIP_ERASURE_STOP_STALLED a frame also stops after a pass that removed nothing from E (no later pass would).  A
        stopped frame's outputs are frozen while other frames go on.
     4. iters[f]: with LDPC_HIP_ERASURE_EARLY_TERM the number of passes the frame ran after which it still held an erasure —
        the stream decoder's convention (decoder.cpp:169-186): resolved in pass I gives I; without it the number of passes
        the frame ran: `iterations` with neither flag.  A frame stopped as stalled after pass I gives I + 1 either way.
     5. unresolved[f] = |E| at the end, erased_out = E, word_out = V; the bits of a row's last word from nc on are 0.
     6. iterations == 0: word_out = word & ~erased, erased_out = erased, iters = 0, unresolved = |E|.  (Not the stream
        decoder's all-zero rows: here the inputs are the caller's data.)
     7. A frame's results do not depend on which frames share its call.
   Identity: after every pass E and V are those of the message-passing decoder of decoder.cpp:91-192 run without its genie
   (an erased variable node of degree 1 sends an erasure); fed the outputs of ldpc_hip_erasure_channel_batch for the
   stream's codewords, iters, erased_out and word_out equal the stream's iters, (llr_out == 69) and (llr_out == 1) under
   ldpc_hip_set_bec_compat(0) for iterations > 0.
   How it runs: byte input is packed by one small launch per operand in front; one workgroup of 512 threads decodes 32
   consecutive frames bit-sliced, all state in LDS, one launch per 2^20 frames at most. */
enum
{
    LDPC_HIP_ERASURE_EARLY_TERM = 1,
    LDPC_HIP_ERASURE_STOP_STALLED = 2
};
int ldpc_hip_erasure_decode_batch(ldpc_hip_ctx *ctx, uint32_t iterations, int flags, uint64_t n, const void *word,
                                  const void *erased, int format, uint32_t *word_out, uint32_t *erased_out, uint32_t *iters,
                                  uint32_t *unresolved, void *hip_stream);
/* LDS bytes one 32-frame group of ldpc_hip_erasure_decode_batch takes on this context's code (host only; worked out once
   per context), -1 for a code the decoder refuses: a group beyond 160 KB or more than 524 288 columns.
     bytes = 4 (2 (nc + 1) + 2 (mc + 1)) + 8 C + 144, rounded up to 16
   — per column its erased word and its value word, per check node TWO words, not three: the kernel stores c0 & ~c1 and
   c0 & ~c1 & xa, all that step 2 reads; one zero word behind each of the four arrays (what a padded list entry points
   at); 8 bytes for each of the C chunks the graph is cut into, C = ceil(mc / 64) + ceil(n8 / 16) + ceil((nc - n8) / 64)
   with n8 the columns of degree >= 8; 144 bytes of votes and counts.  tests/golden/h.txt: 17 888 bytes; four groups of
   512 threads, the 32 waves a CU holds, take 70 KB of its 160.  (Within 160 KB nc and mc stay below 20 480: every index
   of the graph's lists is 16 bits.) */
int64_t ldpc_hip_erasure_lds_bytes(const ldpc_hip_ctx *ctx);

/* Maximum-likelihood erasure decoding: every erased bit that the parity checks determine
   (libldpc_amd/csrc/kernels_erasure_solve.hip).  Peeling stops at the first stopping set; the erased bits still satisfy a
   linear system over GF(2), and this call solves it.  The common rules of this block hold: device or host buffers, checks
   before the GPU naming the entry in ldpc_hip_last_error, n == 0 returns 0 after them, every output may be NULL, ordered on
   hip_stream, no setting and no state of the stream interface read or changed, a frame's results do not depend on which
   frames share its call, every output bit is determined.
   word[n][nc] and erased[n][nc] in, both in `format`, exactly as ldpc_hip_erasure_decode_batch reads them (LDPC_HIP_BITS_U8:
   a non-zero byte is 1 / erased; LDPC_HIP_BITS_PACKED32: the bits of a row's last word from nc on are ignored; a value
   under an erased bit is ignored); word_out[n][W], erased_out[n][W], unresolved[n], rank[n] and status[n] out.  Refused
   (host only, -1): an unknown format, a missing input with n > 0, max_unknowns == 0, and a code and cap whose frame does not
   fit (ldpc_hip_erasure_solve_lds_bytes returns -1; there is no other kernel).  max_unknowns above nc counts as nc.
   Per frame, with E the erased columns on entry and V = word & ~E:
     1. The matrix.  M[r][c] = (the number of times (r, c) is listed in H as the library loaded it) mod 2: an entry listed
        twice cancels.  This is GF(2) — deliberately NOT the rule of ldpc_hip_erasure_decode_batch, where an entry listed twice
        is two edges.
     2. The solutions.  S = the set of x in GF(2)^nc with M x = 0 and x[c] = V[c] for every column c not in E.  All mc check
        nodes count, those without an erased column included.
     3. status[f] = LDPC_HIP_ERASURE_TOO_LARGE if |E| > max_unknowns; otherwise LDPC_HIP_ERASURE_INCONSISTENT if S is empty;
        otherwise LDPC_HIP_ERASURE_SOLVED if every column of E has the same value in all of S; otherwise
        LDPC_HIP_ERASURE_PARTIAL.
     4. SOLVED and PARTIAL: a column of E on which all of S agrees leaves E and takes that value; the others stay erased.
        INCONSISTENT and TOO_LARGE: the frame is returned as it came, word_out = V, erased_out = E.
     5. rank[f] = the rank over GF(2) of the columns E of M for SOLVED, PARTIAL and INCONSISTENT, 0 for TOO_LARGE.  For
        SOLVED and PARTIAL |S| = 2^(|E| - rank).
     6. unresolved[f] = |E| at the end.  The bits of a row's last word from nc on are 0 in both packed outputs.
     7. A frame without erasures is SOLVED iff its syndrome is zero (rank 0), else INCONSISTENT.
   None of this depends on the order of the pivots: a column of E is determined iff its unit vector lies in the row space of
   M restricted to E, which is a property of that row space alone — the reason why the kernel and the numpy mirror of the
   tests, which choose their pivots differently, agree bit for bit.
   Consequence: a bit that peeling recovers is a determined bit.  Solving what the channel delivered and solving what
   ldpc_hip_erasure_decode_batch left of it give the same word_out, erased_out, unresolved and status wherever both stay
   within max_unknowns; rank differs (fewer columns are left).  The advised use is ldpc_hip_erasure_decode_batch with
   LDPC_HIP_ERASURE_EARLY_TERM | LDPC_HIP_ERASURE_STOP_STALLED first and this call on what is left.
   How it runs: byte input is packed by one small launch per operand in front; one workgroup of up to 1024 threads solves
   one frame, its whole system in LDS, by Gauss-Jordan elimination with one barrier per unknown; a frame without erasures or
   over the cap leaves before the matrix is built; one launch per 2^20 frames at most.  ldpcsim, simulate() and the stream's
   BEC decoder are not touched: they stay peeling decoders, as the reference's is. */
enum
{
    LDPC_HIP_ERASURE_SOLVED = 0,
    LDPC_HIP_ERASURE_PARTIAL = 1,
    LDPC_HIP_ERASURE_INCONSISTENT = 2,
    LDPC_HIP_ERASURE_TOO_LARGE = 3
};
int ldpc_hip_erasure_solve_batch(ldpc_hip_ctx *ctx, uint32_t max_unknowns, uint64_t n, const void *word, const void *erased,
                                 int format, uint32_t *word_out, uint32_t *erased_out, uint32_t *unresolved, uint32_t *rank,
                                 uint32_t *status, void *hip_stream);
/* LDS bytes one frame of ldpc_hip_erasure_solve_batch takes at that cap on this context's code (host only), -1 for
   max_unknowns == 0 and for a frame beyond 160 KB.  With U = min(max_unknowns, nc), W = ceil(nc / 32), d the largest number
   of entries H lists for one column:
     R = min(mc, U d)          the rows: the check nodes that list an erased column — each of at most U erased columns is
                               listed by at most d of them, so a sparse code of many check nodes stays in range at a small cap;
     S = ceil((U + 1) / 64) | 1   64-bit words of a row: a bit per unknown and the right-hand side, made odd so that the rows
                               of adjacent threads start on different banks;
     bytes = 8 R S + 12 ceil(mc / 64) + 4 (3 W + 1) + 4 U + 64, rounded up to 16
   — the matrix; per 64 check nodes the mask of those with a row and the rows in front of them; E, V and the unknowns in
   front of each word of E; the column of every unknown; 64 bytes of votes and counts.  Monotone in max_unknowns.
   tests/golden/h.txt (mc = 1024, d = 15) at max_unknowns = 1024: R = 1024, S = 17, 144 064 bytes: one frame per CU. */
int64_t ldpc_hip_erasure_solve_lds_bytes(const ldpc_hip_ctx *ctx, uint32_t max_unknowns);

/* Ordered-statistics decoding (OSD) of frames of LLRs, order 0 and order-1 reprocessing
   (libldpc_amd/csrc/kernels_osd.hip): the codeword that agrees with the hard decisions on the most reliable independent
   positions, and the best of the first `candidates` single flips among them.  Meant as BP + OSD behind a decoder of the
   noisy channels: fed with the llr_out of a frame that message passing left with a non-zero syndrome, it returns a codeword,
   often the transmitted one on short codes; fed with a codeword's LLRs it returns that codeword.  The common rules of this
   block hold: device or host buffers, checks before the GPU naming the entry in ldpc_hip_last_error, n == 0 returns 0 after
   them, every output may be NULL, ordered on hip_stream, no setting and no state of the stream interface read or changed, a
   frame's results do not depend on which frames share its call, every output bit is determined.
   llr[n][nc] in, column order, elements of llr_type (LDPC_HIP_LLR_F64 / F32 / F16 / I8); word_out[n][W] (packed as
   hard_bits is, W = ceil(nc / 32), the bits of a row's last word from nc on 0), flips[n], metric[n], flipped_column[n] and
   status[n] out.  Refused (host only, -1): an unknown llr_type, a NULL llr with n > 0, and a code whose frame does not fit
   (ldpc_hip_osd_lds_bytes returns -1; there is no other kernel).
   Per frame — everything after step 1 is integer or GF(2) arithmetic, nothing depends on a summation order:
     1. The widened value.  W[c] = the element widened exactly to binary64, as in ldpc_hip_decode_batch_typed; for
        LDPC_HIP_LLR_I8 the integer k itself (no step is read: a positive scale changes nothing that matters).
        The decision z[c] = (W[c] <= 0), the decoders' rule; a NaN gives 0.  The reliability
        q[c] = min(floor(|W[c]| * 4096), 2^31 - 1) as uint32; a NaN gives 0, an infinity 2^31 - 1; for I8 it is |k| * 4096.
     2. The matrix.  M[r][c] = (the number of times (r, c) is listed in H as the library loaded it) mod 2, the rule of
        ldpc_hip_erasure_solve_batch.
     3. The order pi lists the columns by (q ascending, column index ascending): the least reliable first.
     4. The solved set.  Scan pi; a column joins the solved set P iff its column of M is linearly independent of the columns
        already in P.  P does not depend on which row is taken as a pivot; |P| = rank(M).  K = every other column, kept in
        the order of pi: the n - rank(M) columns that are trusted, the most reliable ones among them last.
     5. Order 0.  x0 = the unique x with M x = 0 and x[c] = z[c] on K (it exists: the columns of P span the column space of
        M; it is unique: they are independent).
     6. The metric of a word x = the sum of q[c] over the columns where x[c] != z[c], as uint64.
     7. Order-1 reprocessing.  T = min(candidates, |K|).  For the t-th column j of K in the order of pi, t < T, x_j = the
        unique solution that agrees with z on K except at j.  The winner is x0 unless some x_j has a strictly smaller metric;
        among those the smallest metric wins, among equal metrics the smallest t.
     8. word_out = the winner; flips = the number of columns where it differs from z; metric = its metric;
        flipped_column = j if an x_j won, 0xFFFFFFFF otherwise; status = LDPC_HIP_OSD_CODEWORD if M z = 0 (then the winner
        is z itself with metric 0 and 0 flips: the label is the only thing this case changes), otherwise
        LDPC_HIP_OSD_REPROCESSED if an x_j won, otherwise LDPC_HIP_OSD_ORDER0.
   Identities: M word_out = 0 always, so ldpc_hip_syndrome_batch of word_out has weight 0 on every frame; the metric is
   non-increasing in `candidates` (a larger T only adds words to choose from, and the first T stay the first T).
   None of this depends on the order of the pivots — the reason why the kernel and the numpy mirror of the tests, which
   choose their pivots differently, agree bit for bit.
   How it runs: the elements are read in place in their own type (no widening launch in front); one workgroup of up to 1024
   threads takes one frame, its whole check matrix as mc rows of bits in LDS; the order by counting ranks over the nc keys;
   Gauss-Jordan elimination over the columns in that order with one barrier per column (a dependent column costs a vote
   only); x0 from the reduced rows; the candidates scored a wave each from the reduced rows; a frame whose z is a codeword
   leaves before the matrix is built; one launch per 2^20 frames at most.  ldpcsim, simulate() and the stream interface are
   not touched. */
enum
{
    LDPC_HIP_OSD_CODEWORD = 0,
    LDPC_HIP_OSD_ORDER0 = 1,
    LDPC_HIP_OSD_REPROCESSED = 2
};
int ldpc_hip_osd_batch(ldpc_hip_ctx *ctx, uint32_t candidates, uint64_t n, const void *llr, int llr_type, uint32_t *word_out,
                       uint32_t *flips, uint64_t *metric, uint32_t *flipped_column, uint32_t *status, void *hip_stream);
/* LDS bytes one frame of ldpc_hip_osd_batch takes on this context's code (host only), -1 for a code with 65 536 columns or
   more, with more than 32 768 check nodes, or with a frame beyond 160 KB.  With V = ceil(nc / 64):
     S = (V + 1) | 1           64-bit words of a row: a bit per column and at least one word beside them (what the candidate
                               search reads of the row's pivot column), made odd so that the rows of adjacent threads
                               start on different banks;
     bytes = max(8 mc S, 4 nc rounded up to 8) + 24 V + (2 nc rounded up to 8) + 384, rounded up to 16
   — the matrix, whose region holds the nc sort keys before it is built; z, P and the word as masks; the order, 16 bits a
   column; 384 bytes of votes, sums and one best candidate per wave.
   tests/golden/h.txt (mc = 1024, nc = 1152): V = 18, S = 19, 155 648 + 432 + 2 304 + 384 = 158 768 bytes: one frame per CU. */
int64_t ldpc_hip_osd_lds_bytes(const ldpc_hip_ctx *ctx);

/* Ordered-statistics decoding TOWARD A GIVEN SYNDROME, with a bounded order-2 sweep
   (libldpc_amd/csrc/kernels_osd_syndrome.hip): ldpc_hip_osd_batch asks for M x = 0, this entry for M x = s with the s the
   caller holds, and it adds a second stage of candidates — every pair among the first `pair_depth` trusted columns, the
   "combination sweep" of BP + OSD.  Meant behind ldpc_hip_syndrome_decode_batch: fed with the llr_out and the syndromes of the
   frames that message passing left at a weight > 0, it returns a word with syndrome s wherever one exists.
   ldpc_hip_osd_batch is unchanged.  The common rules of this block hold: device or host buffers, checks before the GPU
   naming the entry in ldpc_hip_last_error, n == 0 returns 0 after them, every output may be NULL, ordered on hip_stream, no
   setting and no state of the stream interface read or changed, a frame's results do not depend on which frames share its
   call, every output bit is determined.
   In:  llr[n][nc] exactly as in ldpc_hip_osd_batch; syndrome[n][mc] and syndrome_format exactly as in
        ldpc_hip_syndrome_decode_batch (LDPC_HIP_BITS_U8 or LDPC_HIP_BITS_PACKED32, what ldpc_hip_syndrome_batch writes, bit r
        = check node r in file row order; NULL = all zero; the bits of a row's last word from mc on are ignored).
   Out: word_out[n][W], flips[n], metric[n], status[n] as in ldpc_hip_osd_batch, and flipped_columns[n][2].  "none" below
        is 0xFFFFFFFF.
   Per frame, with W, z, q, M, pi, P, K and the metric of steps 1..4 and 6 of ldpc_hip_osd_batch:
     a. Met.  If M z = s: status = LDPC_HIP_OSD_CODEWORD (value 0, read here as "z already meets s"), word_out = z, metric
        0, 0 flips, both columns none.
     b. Infeasible.  If s is not in the column space of M (a property of M and s alone, not of the pivots): status =
        LDPC_HIP_OSD_INFEASIBLE, word_out = z, metric 0, 0 flips, both columns none.  Not an error return: on
        tests/golden/h.txt (rank 1021 of 1024 check nodes) 7 of 8 random syndromes are infeasible; s = H x of any word x is
        always feasible.
     c. Order 0.  x0 = the unique x with M x = s and x = z on K.
     d. Singles.  T = min(candidates, |K|); x_t agrees with z on K except at K[t], t < T; its candidate index is e = t.
     e. Pairs.  L = min(pair_depth, |K|); for 0 <= t1 < t2 < L, x_{t1,t2} agrees with z on K except at K[t1] and K[t2]; its
        candidate index is e = T + the lexicographic rank of (t1, t2) among those pairs.
     f. Winner.  x0 unless some candidate has a strictly smaller metric; among the candidates the smallest metric wins,
        among equal metrics the smallest e (every single before every pair).
     g. status = LDPC_HIP_OSD_ORDER0 if x0 wins, LDPC_HIP_OSD_REPROCESSED if a single does, LDPC_HIP_OSD_REPROCESSED_PAIR if a
        pair does; flipped_columns = (K[t], none), (K[t1], K[t2]) or (none, none); word_out, flips and metric are the
        winner's.
   Identities: for every frame that is not infeasible, ldpc_hip_syndrome_batch(word_out) XOR s has weight 0.  The metric is
   non-increasing in `candidates` and in `pair_depth` (either only adds words to choose from).  With syndrome == NULL and
   pair_depth == 0, word, flips, metric, status and flipped_columns[:][0] are those of ldpc_hip_osd_batch.  With s = M u for
   a known word u and LLRs that hold no zero and no NaN, word_out = (the word of ldpc_hip_osd_batch on the LLRs with the sign
   flipped wherever u is 1) XOR u, and flips, metric, column and status are the same: the sign flip changes z by u and leaves
   q, pi, P and K alone.  None of this depends on the order of the pivots.
   Refused (host only, -1): an unknown llr_type or syndrome_format, a NULL llr with n > 0, pair_depth > 256, and a code whose
   frame does not fit (ldpc_hip_osd_syndrome_lds_bytes returns -1; there is no other kernel).  The limit on pair_depth bounds
   a frame's time on a shared device: at most 32 640 pairs, each one pass of a wave over the mc reduced rows.  Measured at the
   cap on an MI355X (profiles/osd_syndrome.jsonl): the pair stage takes 1.59 ms per frame of tests/golden/h.txt (16 waves) and
   2.28 ms per frame of a (3,6)-regular code of 240 columns (2 waves, 7 140 pairs); reasoned from those, a code of at most 64
   check nodes with 256 trusted columns (one wave) takes about 25 ms.
   How it runs: the kernel of ldpc_hip_osd_batch with a right-hand side — every row carries the bit (s + M z) of its check
   node in bit 63 of its side word through the elimination, order 0 reads it off the pivot rows, a row left without a pivot
   whose bit is set is the infeasible case; singles as there; pairs a wave each, scored directly from the reduced rows
   (metric(x0) + q[j1] + q[j2] + the signed reliabilities of the pivots of the rows that hold exactly one of the two
   columns), so no second elimination; one launch per 2^20 frames at most.  ldpcsim, simulate() and the stream interface are
   not touched. */
enum
{
    LDPC_HIP_OSD_REPROCESSED_PAIR = 3,
    LDPC_HIP_OSD_INFEASIBLE = 4
};
int ldpc_hip_osd_syndrome_batch(ldpc_hip_ctx *ctx, uint32_t candidates, uint32_t pair_depth, uint64_t n, const void *llr, int llr_type,
                                const void *syndrome, int syndrome_format, uint32_t *word_out, uint32_t *flips, uint64_t *metric,
                                uint32_t *flipped_columns /* [n][2] */, uint32_t *status, void *hip_stream);
/* LDS bytes one frame of ldpc_hip_osd_syndrome_batch takes on this context's code (host only), -1 under the conditions of
   ldpc_hip_osd_lds_bytes.  With V and S as there:
     bytes = max(8 mc S, 4 nc rounded up to 8) + 24 V + (2 nc rounded up to 8) + 1536, rounded up to 16
   — the parts of ldpc_hip_osd_lds_bytes with 1 536 bytes in place of 384: 512 of votes, sums and per wave its best
   candidate (metric, index, two places in K), and 1 024 of the reliabilities of the first 256 columns of K, which the
   pair stage reads instead of the input.  The right-hand side takes no room: it is a bit of the side word.
   tests/golden/h.txt: 155 648 + 432 + 2 304 + 1 536 = 159 920 bytes: one frame per CU. */
int64_t ldpc_hip_osd_syndrome_lds_bytes(const ldpc_hip_ctx *ctx);

/* Quantized min-sum decoding of frames of LLRs TOWARD A GIVEN SYNDROME (libldpc_amd/csrc/kernels_syndrome_decode.hip): which
   word x with H x = s fits these LLRs, for the s the caller holds — every other decoder of this library asks for H x = 0.
   The decoder of syndrome-based source coding with side information (Slepian-Wolf) and of information reconciliation: one
   side sends s = H x of ANY word x (ldpc_hip_syndrome_batch writes it, packed), the other decodes its noisy copy of x toward
   s; and of every syndrome-measuring application: s the measured syndrome, the LLRs one prior row shared by every shot
   (LDPC_HIP_SYNDROME_SHARED_LLR), the output an error estimate.  NON-PARITY (the reference has no such decoder).
   The common rules of this block hold: device or host buffers, checks before the GPU naming the entry in
   ldpc_hip_last_error, n == 0 returns 0 after them, every output may be NULL (all NULL: nothing is launched), ordered on
   hip_stream, a frame's results do not depend on which frames share its call, every output bit is determined.  NO SETTING AND
   NO STATE OF THE STREAM INTERFACE IS READ OR CHANGED: everything the call uses is in *p; the context's quantization,
   correction, schedule and ternary settings are ignored.
   In:  llr[n][nc], column order, elements of llr_type (LDPC_HIP_LLR_F64 / F32 / F16 / I8), read in place in their own type
        (no widening launch, no binary64 staging in LDS).  All nc columns are the caller's values, as in
        ldpc_hip_decode_batch: punctured and shortened columns get no substitute.  With LDPC_HIP_SYNDROME_SHARED_LLR in
        p->flags llr is ONE row [nc], used for every frame.
        syndrome[n][mc] in syndrome_format (LDPC_HIP_BITS_U8: a byte per check node, non-zero = 1; LDPC_HIP_BITS_PACKED32:
        ceil(mc / 32) words per row), exactly what ldpc_hip_syndrome_batch writes: bit r is check node r in file row order.
        NULL = the all-zero syndrome.  The bits of a row's last word from mc on are ignored.
   Out: hard_bits[n][ceil(nc / 32)] (the layout of hard_bits in ldpc_hip_decode_batch_typed, the bits of a row's last word
        from nc on 0), iters[n], weight[n], llr_out[n][nc] (binary64, column order).
   Arithmetic: items 1..7 of ldpc_hip_set_min_sum_quantization with q = p->q_bits, D = p->step, Qmax = 2^(q-1) - 1,
   inv = fl(1 / D) and lut built from (p->scale, p->offset) by the same host routine (item 3), with two changes and two
   additions.  All integer after the quantizer:
     1. Quantizer.  L[v] = clamp(rint(fl(W[v] * inv)), -Qmax, +Qmax), W the element widened exactly to binary64; a NaN gives
        0, infinities saturate.  For LDPC_HIP_LLR_I8, L = clamp(k, -Qmax, +Qmax) — the equality stated for the direct
        fixed-point layered path (ldpc_hip_decode_batch_typed): it is the quantizer applied to fl(k * D) for every step the
        call takes.
     2. CHANGE, check node sign: in check node c, c2v_j is negative iff (the number of other v2c_k < 0) + s[c] is odd.
        Magnitudes, the table and the variable nodes are items 3..5 unchanged.
     3. CHANGE, stop rule: with early_term the frame stops after the first iteration whose decisions satisfy
        XOR of hard over the row == s[c] for every check node (instead of == 0).
     4. iters = the index of the iteration whose decisions met the test (the reference's convention, as everywhere),
        otherwise `iterations`.
     5. ADDITION, weight[f] = the number of check nodes whose test fails on the frame's final decisions, also without
        early termination: 0 iff the returned word has syndrome s.
     6. ADDITION, iterations == 0 returns the quantized input: A = L, hard = (L <= 0), llr_out = fl(L * D), iters = 0, and the
        weight of that.  Deliberately not the all-zero rows of the stream decoders: the inputs are the caller's data, as
        ldpc_hip_erasure_decode_batch argues.
     7. llr_out[v] = fl((double) A[v] * D) of the last iteration the frame ran.
   Identities: with syndrome == NULL and iterations > 0, iters, the decisions and llr_out are those of
   ldpc_hip_decode_batch_typed under ldpc_hip_set_min_sum_quantization(q, D) and ldpc_hip_set_min_sum_correction(scale,
   offset); with any s, the messages are those of that decoder on the code [H | I] (mc further columns, column nc + r in
   row r alone) fed 99999.9 (1 - 2 s[r]) there — the route this entry replaces —, so without early termination the first nc
   decisions and totals agree after any number of iterations.  With early termination iters agrees too whenever
   lut[Qmax] < Qmax (any scale below 1 that moves Qmax): an extra column decides on +-Qmax + c2v, and with (1, 0) a check node
   whose other inputs all sit at Qmax returns -+Qmax, the total is 0, the tie decides 1 and the augmented route runs on
   after this entry has met s.
   Refused (host only, -1): a null p; q_bits outside 2..8; a step that is NaN, <= 0 or outside [2^-20, 2^20]; a scale
   outside (0, 1], an offset outside [0, 1e6], a NaN in either; early_term other than 0 / 1; an unknown flag bit, llr_type
   or syndrome_format; a NULL llr with n > 0; a code the call does not take.
   Which codes it takes: every code the library loads in which every check node has at least two entries, with at most
   65 535 columns and the frame's LDS (below) within 160 KB; otherwise ldpc_hip_syndrome_decode_lds_bytes returns -1 and
   there is no other kernel.
   How it runs: one workgroup of 256 threads per frame on the tables of quantized min-sum (built once per context, uploaded
   at the first call that needs them); a thread per column quantizes the element it reads and stores the byte at the
   column's place in the kernel's order; a thread per check node fetches its syndrome bit through the map from the kernel's
   check-node order to file rows; a byte per message in LDS; the packed decisions by a ballot per 64 columns; one launch per
   2^20 frames at most.  OSD toward a syndrome is ldpc_hip_osd_syndrome_batch: llr_out and s feed it.  ldpcsim, simulate() and
   the stream interface are not touched. */
enum
{
    LDPC_HIP_SYNDROME_SHARED_LLR = 1
};
typedef struct
{
    uint32_t iterations;
    int early_term; /* 0 / 1 */
    int q_bits;     /* 2..8 */
    double step;    /* 2^-20 .. 2^20 */
    double scale;   /* (0, 1] */
    double offset;  /* [0, 1e6] */
    int flags;      /* LDPC_HIP_SYNDROME_SHARED_LLR or 0 */
} ldpc_hip_syndrome_decode;
int ldpc_hip_syndrome_decode_batch(ldpc_hip_ctx *ctx, const ldpc_hip_syndrome_decode *p, uint64_t n, const void *llr, int llr_type,
                                   const void *syndrome, int syndrome_format, uint32_t *hard_bits, uint32_t *iters,
                                   uint32_t *weight, double *llr_out, void *hip_stream);
/* LDS bytes one frame of ldpc_hip_syndrome_decode_batch takes on this context's code (host only), -1 for a code the call
   does not take.  With `slots` = the check-node degrees, each rounded up to a multiple of 4, summed (one byte per message, a
   check node's messages padded to whole words), and every term rounded up to 16:
     bytes = r16(slots) + r16(4 nc) + 160 + r16(4 ceil(mc / 32)) + r16(nc)
   — the messages; the nc 32-bit totals; the 128-byte table with 32 bytes of votes and partial sums; the frame's syndrome, a
   bit per check node; the nc quantized inputs.  There is no binary64 area.
   tests/golden/h.txt (nc = 1152, mc = 1024): see DESIGN.md section 4 for the figure and the frames per CU. */
int64_t ldpc_hip_syndrome_decode_lds_bytes(const ldpc_hip_ctx *ctx);

/* Fixed-point LAYERED min-sum decoding of frames of LLRs toward a given syndrome
   (libldpc_amd/csrc/kernels_syndrome_decode_layered.hip): ldpc_hip_syndrome_decode_batch on the row-serial schedule, with
   messages of p->msg_bits bits and saturating totals of p->app_bits bits — the schedule and datapath reconciliation and
   hardware decoders use, about half the sweeps of flooding.  NON-PARITY.  ldpc_hip_syndrome_decode_batch and its struct are
   unchanged; this entry stands beside it.
   The common rules are those of ldpc_hip_syndrome_decode_batch, word for word: device or host buffers, checks before the GPU
   naming the entry in ldpc_hip_last_error, n == 0 returns 0 after them, every output may be NULL (all NULL: nothing is
   launched), ordered on hip_stream, a frame's results do not depend on which frames share its call, every output bit is
   determined.  NO SETTING AND NO STATE OF THE STREAM INTERFACE IS READ OR CHANGED: everything the call uses is in *p.
   In and Out: as there.  llr[n][nc] of llr_type (F64 / F32 / F16 / I8) read in place, one row [nc] with
   LDPC_HIP_SYNDROME_SHARED_LLR; syndrome[n][mc] U8 or PACKED32, bit r = check node r in file row order, NULL = all zero, the
   bits of a row's last word from mc on ignored; hard_bits[n][ceil(nc / 32)] with the bits of a row's last word from nc on 0,
   iters[n], weight[n], llr_out[n][nc] binary64 in column order.
   Arithmetic: items 1..7 of ldpc_hip_set_min_sum_layered_fixed with q = p->msg_bits, p = p->app_bits, D = p->step,
   Qmax = 2^(q-1) - 1, Pmax = 2^(p-1) - 1, inv = fl(1 / D), on the layered plan of the context (build_layer_plan) and with lut
   built from (p->scale, p->offset) by the same host routine (item 3), with the two changes and two additions of
   ldpc_hip_syndrome_decode_batch.  All integer after the quantizer:
     1. Quantizer.  Unchanged: L[v] = clamp(rint(fl(W[v] * inv)), -Qmax, +Qmax), W the element widened exactly to binary64; a
        NaN gives 0, infinities saturate.  For LDPC_HIP_LLR_I8, L = clamp(k, -Qmax, +Qmax).  T[v] := L[v], every message 0.
     2. CHANGE, check node sign: in check node c, m[c][j] is negative iff (the number of other u_k < 0) + s[c] is odd.
        t, u, the magnitudes, the table and the saturating update of T are item 4 unchanged.
     3. CHANGE, stop rule: with early_term the frame stops after the first sweep whose decisions satisfy
        XOR of hard over the row == s[c] for every check node (instead of == 0).
     4. iters = the number of sweeps completed before the sweep whose decisions met the test, otherwise `iterations`.
     5. ADDITION, weight[f] = the number of check nodes whose test fails on the frame's final decisions, also without
        early termination: 0 iff the returned word has syndrome s.
     6. ADDITION, iterations == 0 returns the quantized input: T = L, hard = (L <= 0), llr_out = fl(L * D), iters = 0, and the
        weight of that.
     7. llr_out[v] = fl((double) T[v] * D) of the last sweep the frame ran.
   Identities (tests/test_syndrome_decode_layered_host.py on the mirror, tests/test_gpu_syndrome_decode_layered.py on the GPU):
     (a) with syndrome == NULL and iterations > 0, iters, the decisions and llr_out are those of ldpc_hip_decode_batch_typed
         under ldpc_hip_set_min_sum_layered_fixed(q, p, D) and ldpc_hip_set_min_sum_correction(scale, offset);
     (b) with any s, on a code whose check nodes all have degree <= 7 and with app_bits > msg_bits, the first nc totals and
         decisions are those of that decoder on the code [H | I] (mc further columns, column nc + r in row r alone) fed
         99999.9 (1 - 2 s[r]) there, without early termination, after any number of sweeps.  The augmented code's plan has
         the same steps (every degree grows by one — hence degree <= 7 —, and an extra column conflicts with nobody); the
         extra column's total is +-Qmax + m with |m| <= Qmax, never clamped as Pmax >= 2 Qmax + 1 — hence app_bits >
         msg_bits —, so its t is exactly +-Qmax in every sweep: the largest magnitude, which moves no minimum, and a sign that
         is s[r].
   Refused (host only, -1): a null p; msg_bits outside 2..8; app_bits outside msg_bits..16; a step that is NaN, <= 0 or
   outside [2^-20, 2^20]; a scale outside (0, 1], an offset outside [0, 1e6], a NaN in either; early_term other than 0 / 1;
   an unknown flag bit, llr_type or syndrome_format; a NULL llr with n > 0; a code the call does not take.
   Which codes it takes: those of the layered plan — every check node of degree 2..8, at most 65 535 columns, no isolated
   column — whose frame (below) fits 160 KB of LDS; otherwise ldpc_hip_syndrome_decode_layered_lds_bytes returns -1 and there
   is no other kernel.
   How it runs: one wave and one frame per workgroup on the tables of the layered plan, with one further table, (step, lane)
   -> file row of that check node, built from the host plan and uploaded at the first call; the prologue quantizes the elements
   it reads in place to the totals, no binary64 value is staged; the syndrome bit of a check node is bit 31 of its 32-bit
   record (bits 0..24 hold its two magnitudes, argmin and signs), set when the records are initialised and kept by every
   rewrite; the packed decisions by a ballot per 64 columns, the weight by one parity pass, a popcount of ballots; one launch
   per 2^20 frames at most.  OSD toward a syndrome is ldpc_hip_osd_syndrome_batch: llr_out and s feed it. */
typedef struct
{
    uint32_t iterations;
    int early_term; /* 0 / 1 */
    int msg_bits;   /* 2..8 */
    int app_bits;   /* msg_bits..16 */
    double step;    /* 2^-20 .. 2^20 */
    double scale;   /* (0, 1] */
    double offset;  /* [0, 1e6] */
    int flags;      /* LDPC_HIP_SYNDROME_SHARED_LLR or 0 */
} ldpc_hip_syndrome_decode_layered;
int ldpc_hip_syndrome_decode_layered_batch(ldpc_hip_ctx *ctx, const ldpc_hip_syndrome_decode_layered *p, uint64_t n, const void *llr,
                                           int llr_type, const void *syndrome, int syndrome_format, uint32_t *hard_bits,
                                           uint32_t *iters, uint32_t *weight, double *llr_out, void *hip_stream);
/* LDS bytes one frame of ldpc_hip_syndrome_decode_layered_batch takes on this context's code (host only), -1 for a code the
   call does not take.  With R as for ldpc_hip_layered_fixed_lds_bytes (each step's check nodes rounded up to an even number,
   summed):
     bytes = round4(2 nc) + 4 R + 128, rounded up to 16
   — the int16 totals, from the next multiple of 4 one 32-bit record per slot, behind them the 128-byte correction table:
   exactly ldpc_hip_layered_fixed_direct_lds_bytes, the syndrome costs no byte.  tests/golden/h.txt: 6 528 bytes, 25 frames
   per CU. */
int64_t ldpc_hip_syndrome_decode_layered_lds_bytes(const ldpc_hip_ctx *ctx);

/* GRADIENT-DESCENT BIT FLIPPING of frames toward a given syndrome (libldpc_amd/csrc/kernels_bit_flip.hip): the
   hard-decision, low-complexity family beside the message-passing decoders — GDBF (Wadayama, Nakamura, Yagita, Funahashi,
   Usami, Takumi, "Gradient descent bit flipping algorithms for decoding LDPC codes", IEEE Trans. Commun. 2010) with soft
   reliabilities and multi-bit flipping, and its probabilistic variant PGDBF (Rasheed, Ivanis, Vasic, "Fault-tolerant
   probabilistic gradient-descent bit flipping decoder", IEEE Commun. Lett. 2014) on the counter generator of
   ldpc_hip_set_noise.  A frame's whole state is a byte and a bit per column and a bit per check node.  NON-PARITY (the
   reference has no such decoder).
   The common rules are those of ldpc_hip_syndrome_decode_batch, word for word: device or host buffers, checks before the GPU
   naming the entry in ldpc_hip_last_error, n == 0 returns 0 after them, every output may be NULL (all NULL: nothing is
   launched), ordered on hip_stream, one launch per 2^20 frames at most, a frame's results do not depend on which frames
   share its call or its workgroup, every output bit is determined.  NO SETTING AND NO STATE OF THE STREAM INTERFACE IS READ OR
   CHANGED: everything the call uses is in *p (the noise mode of ldpc_hip_set_noise included: the draws below are this
   call's own).
   In:  llr[n][nc] of llr_type (F64 / F32 / F16 / I8), column order, read in place; one row [nc] with
        LDPC_HIP_SYNDROME_SHARED_LLR in p->flags.  A caller with hard decisions only passes I8 values +-1 with q_bits = 2.
        syndrome[n][mc] U8 or PACKED32, bit r = check node r in file row order (what ldpc_hip_syndrome_batch writes), NULL =
        all zero, the bits of a row's last word from mc on ignored.
   Out: hard_bits[n][ceil(nc / 32)] with the bits of a row's last word from nc on 0, iters[n], weight[n].
   Arithmetic, all integer after the quantizer, with Qmax = 2^(q_bits-1) - 1, inv = fl(1 / step), w = check_weight:
     1. Quantizer: item 1 of ldpc_hip_syndrome_decode_batch.  L[v] = clamp(rint(fl(W[v] * inv)), -Qmax, +Qmax), W the element
        widened exactly to binary64; a NaN gives 0, infinities saturate.  For LDPC_HIP_LLR_I8, L = clamp(k, -Qmax, +Qmax).
        y[v] = (L[v] <= 0), r[v] = |L[v]|, x := y.
     2. Round t = 0, 1, ...: u[c] = s[c] XOR the XOR of x over the entries of row c (an entry listed twice counts twice).  If
        every u[c] is 0 the frame is finished with iters = t: a word that meets s is never flipped.  If t == iterations the
        frame is finished with iters = iterations.
     3. The penalty of every one of the nc columns: P[v] = w U[v] + (x[v] != y[v] ? +r[v] : -r[v]), U[v] the sum of u[c] over
        the entries (c, v) of H (an entry listed twice adds twice).  With w = 2 and r = 1 everywhere this orders the columns
        exactly as PGDBF's energy "unsatisfied neighbours + disagreement with the channel" does.
     4. Pmax = the largest P[v] of the frame; the candidates are the v with P[v] >= Pmax - margin.
     5. With flip_threshold == 0xFFFFFFFF every candidate flips (GDBF; nothing is drawn).  Otherwise candidate v flips iff
        its draw < flip_threshold, the draw being word v & 3 of Philox4x32-10 block t ceil(nc / 4) + (v >> 2) of frame
        first_frame + f under TAG 3 and p->seed (key and counter layout: ldpc_hip_set_noise; ldpc_hip_philox returns the same
        words).  A round in which nothing flips still counts.  The same frames come out of any split of a batch into calls,
        once first_frame is set accordingly.
     6. weight[f] = the number of u[c] != 0 on the final word: 0 iff the returned word has syndrome s.  A frame that meets s
        only after its last round has iters = iterations and weight 0.
     7. iterations == 0 returns the quantized input's decisions, iters = 0 and the weight of that.
   Identities (tests/test_bit_flip_host.py on the mirror tests/bit_flip_ref.py, tests/test_gpu_bit_flip.py on the GPU): (a)
   translation — on frames without a quantized zero, decoding L (1 - 2 x0) toward s XOR H x0 returns the word of (L, s) XOR
   x0 with the same iters and weight, in both modes: the draws depend on (frame, round, column) alone; (b) prefix — a run of
   k rounds agrees with a longer one on every frame that finished within k.
   Refused (host only, -1): a null p; iterations above 65535; q_bits outside 2..8; a step that is NaN, <= 0 or outside
   [2^-20, 2^20]; check_weight outside 1..255; margin above 65535; an unknown flag bit, llr_type or syndrome_format; a NULL
   llr with n > 0; a code the call does not take.
   Which codes it takes: every code the library loads with at most 65 535 columns and 65 535 check nodes whose frame
   (below) fits the 160 KB of LDS — any degrees, isolated columns, entries listed twice; otherwise
   ldpc_hip_bit_flip_lds_bytes returns -1 and there is no other kernel.
   How it runs: one wave per frame, up to four frames to a workgroup (as many as keep the group within 40 KB), no workgroup
   barrier; the two adjacency tables of H (row -> columns, column -> rows, u16 indices, file order) built once per context
   and uploaded at the first call.  The prologue quantizes the elements it reads in place to a byte per column, packs x by a
   ballot per 64 columns and forms u once, a lane per check node, with s folded in.  A round walks the columns twice, a lane
   per column: the first walk forms P from the bits of u and reduces the maximum across the wave, the second forms P again
   in the lanes that can hold a candidate and flips: the bit of x, and the bits of the column's check nodes in the NEXT
   round's copy of u (LDS atomics), so u is never recomputed from x.  The stop test is a ballot over the words of u, the
   weight a popcount of them, the packed decisions the words of x. */
typedef struct
{
    uint32_t iterations;     /* 0..65535 flip rounds at most */
    int q_bits;              /* 2..8: width of the reliabilities */
    double step;             /* 2^-20 .. 2^20 */
    uint32_t check_weight;   /* 1..255: w above */
    uint32_t margin;         /* 0..65535: flip every column within `margin` of the frame's largest penalty */
    uint32_t flip_threshold; /* 0xFFFFFFFF: every candidate flips (GDBF, no draws); else a candidate flips iff its draw < this */
    uint64_t seed;           /* of the draws */
    uint64_t first_frame;    /* frame f of the call draws as frame first_frame + f */
    int flags;               /* LDPC_HIP_SYNDROME_SHARED_LLR or 0 */
} ldpc_hip_bit_flip;
int ldpc_hip_bit_flip_batch(ldpc_hip_ctx *ctx, const ldpc_hip_bit_flip *p, uint64_t n, const void *llr, int llr_type,
                            const void *syndrome, int syndrome_format, uint32_t *hard_bits, uint32_t *iters, uint32_t *weight,
                            void *hip_stream);
/* LDS bytes one frame of ldpc_hip_bit_flip_batch takes on this context's code (host only), -1 for a code the call does not
   take.  Every term rounded up to 16:
     bytes = r16(nc) + r16(4 ceil(nc / 32)) + 2 r16(4 ceil(mc / 32))
   — the nc quantized inputs, a byte each (sign = y, magnitude = r); the word x, a bit per column; the unmet checks u, a bit
   per check node, of this round and of the next.  tests/golden/h.txt (nc = 1152, mc = 1024): 1 152 + 144 + 2 * 128 = 1 552
   bytes; a CU's 32 waves are reached before its LDS. */
int64_t ldpc_hip_bit_flip_lds_bytes(const ldpc_hip_ctx *ctx);

/* MIN-SUM WITH MEMORY, RUN AS A RELAY OF LEGS, toward a given syndrome (libldpc_amd/csrc/kernels_relay_decode.hip): the
   message-passing decoder for the degenerate check matrices of quantum LDPC and surface codes (column degree 2, many
   equal-weight solutions, trapping sets everywhere), on which plain min-sum swings between solutions instead of choosing
   one.  DMem-BP (Mueller, Alexander, Beverland, Buehler, Johnson, Maurer, Vandeth, "Improved belief propagation is
   sufficient for real-time decoding of quantum memory", 2025): a column's prior for an iteration is a mix of its input
   and its own previous total, by a strength gamma per column.  Relay-BP (the same authors): several such runs ("legs") are
   chained, each with its own gamma, some of them negative, each starting from the totals the last one left; every word
   that meets the syndrome is priced and the cheapest returned.  No elimination (ldpc_hip_osd_syndrome_batch), a byte per
   message of LDS.  NON-PARITY (the reference has no such decoder).
   The common rules are those of ldpc_hip_syndrome_decode_batch, word for word: device or host buffers, checks before the GPU
   naming the entry in ldpc_hip_last_error, n == 0 returns 0 after them, every output may be NULL (all NULL: nothing is
   launched), ordered on hip_stream, one launch per 2^20 frames at most, a frame's results do not depend on which frames
   share its call or its workgroup, every output bit is determined.  NO SETTING AND NO STATE OF THE STREAM INTERFACE IS READ OR
   CHANGED: everything the call uses is in *p and gamma.
   In:  llr, llr_type, syndrome, syndrome_format: exactly as in ldpc_hip_syndrome_decode_batch — llr[n][nc] of llr_type
        (F64 / F32 / F16 / I8), column order, read in place in their own type, ONE row [nc] with
        LDPC_HIP_SYNDROME_SHARED_LLR in p->flags; syndrome[n][mc] U8 or PACKED32, bit r = check node r in file row order,
        NULL = all zero, the bits of a row's last word from mc on ignored.
        gamma[legs][nc], int8, column order, shared by all frames (device or host): g means a strength of g / 64.  Values
        outside -64..64 are clamped to that range by the kernel.  NULL = all zero.
   Out: hard_bits[n][ceil(nc / 32)] (the bits of a row's last word from nc on 0), iters[n], weight[n], solutions[n],
        best_leg[n], cost[n].
   Arithmetic, with q = p->q_bits, D = p->step, Qmax = 2^(q-1) - 1, inv = fl(1 / D) and lut built from (p->scale, p->offset) by
   the same host routine as everywhere.  All integer after the quantizer:
     1. Quantizer: item 1 of ldpc_hip_syndrome_decode_batch.  L[v] = clamp(rint(fl(W[v] * inv)), -Qmax, +Qmax), W the element
        widened exactly to binary64; a NaN gives 0, infinities saturate.  For LDPC_HIP_LLR_I8, L = clamp(k, -Qmax, +Qmax).
        y[v] = (L[v] <= 0).
     2. The state is the totals A[v], carried from leg to leg, and the messages.  Before leg 0, A := L.
     3. Leg l runs at most T iterations, T = first_iterations for l = 0 and leg_iterations otherwise.  At the start of a leg
        every check-to-variable message is 0.
     4. Iteration, memory term.  For every column, with g = gamma[l][v] clamped to -64..64: p = g (A[v] - L[v]) (fits 32
        bits), d = sign(p) ((|p| + 32) >> 6) (rounds half away from zero: the decoder stays sign-symmetric),
        Lambda[v] = clamp(L[v] + d, -32767, +32767), A[v] being the total the previous iteration or leg left.
     5. Variable nodes: v2c_e = clamp(Lambda[v] + (the sum of the column's c2v) - c2v_e, -Qmax, +Qmax).  In a leg's first
        iteration the c2v are 0, so v2c = clamp(Lambda[v]).
     6. Check nodes: items 3 and 4 of ldpc_hip_set_min_sum_quantization with the sign change of
        ldpc_hip_syndrome_decode_batch: the message is negative iff (the number of other v2c < 0) + s[c] is odd.
     7. Totals: A[v] = Lambda[v] + the sum of the column's c2v of this iteration; hard[v] = (A[v] <= 0).
     8. Test: if XOR of hard over the row == s[c] for every check node, the leg ends at this iteration, of index i counted
        from 0, and hard is a SOLUTION.  Its cost is the sum of |L[v]| over the columns with hard[v] != y[v] (fits 32 bits).
        It replaces the kept word iff no word is kept yet or its cost is STRICTLY smaller (the earliest wins ties).  A leg
        that never meets s ends after T iterations.  In either case the next leg starts from these A.
     9. The frame ends after leg legs - 1, or as soon as stop_after legs have produced a solution.
    10. hard_bits = the kept word; if there is none, the decisions of the last iteration run.  iters = the sum, over the
        legs run, of i for a leg that met s and of T for one that did not (one leg counts exactly as
        ldpc_hip_syndrome_decode_batch).  weight = the check nodes the returned word does not meet: 0 iff a solution was
        found.  solutions = the legs that met s.  best_leg and cost = those of the kept word, both 0xFFFFFFFF when there is
        none.
   Identity: with legs = 1 and gamma NULL or all zero, hard_bits, iters and weight are those of
   ldpc_hip_syndrome_decode_batch with early_term = 1 and iterations = first_iterations, for any s and any setting.
   Prefix: a call with k legs agrees, in every output, with a call with K > k legs on the first k rows of the same gamma, on
   every frame whose solutions reached stop_after within k legs.
   (tests/test_relay_decode_host.py on the mirror tests/relay_decode_ref.py, tests/test_gpu_relay_decode.py on the GPU.)
   Refused (host only, -1): a null p; legs outside 1..256; first_iterations or leg_iterations outside 1..65535; stop_after
   outside 1..legs; q_bits outside 2..8; a step that is NaN, <= 0 or outside [2^-20, 2^20]; a scale outside (0, 1], an offset
   outside [0, 1e6], a NaN in either; form outside 0..2; an unknown flag bit, llr_type or syndrome_format; a NULL llr with
   n > 0; a code the call does not take, or a form the code does not fit.
   Which codes it takes: those of ldpc_hip_syndrome_decode_batch — every check node with at least two entries, at most 65 535
   columns — whose frame (below) fits 160 KB of LDS.  Form 2 additionally needs FOUR frames to fit 160 KB.
   How it runs: one kernel body on the tables of quantized min-sum, the column map and the check-node order of
   ldpc_hip_syndrome_decode_batch, templated on the threads that share a frame.  Form 1: a workgroup of 256 threads per
   frame, workgroup barriers between the passes, the stop test through two vote words.  Form 2: a wave per frame and four
   frames to a workgroup, no workgroup barrier (a wave's LDS operations execute in order), the stop test a ballot: for codes
   of 72 to a few hundred columns with very many shots, where 256 threads would mostly idle.  Form 0 chooses: form 2 where
   it fits and the code has at most 384 columns and 384 check nodes.  All forms return the same
   bits.  The memory term is formed inside the variable-node pass from the total it is about to overwrite (no further pass,
   no further array); the leg's gamma is read from global memory through the rank -> column map; the cost (a reduction)
   and the kept word (a ballot per 64 columns into LDS, column order) are formed only in iterations that met s.
   A gamma table: HipDecoder.relay_gammas (libldpc_amd/binding.py) draws one from ldpc_hip_philox under TAG 4: row 0 is one
   value everywhere, row l >= 1, column v is lo + ((draw * (hi - lo + 1)) >> 32), the draw being word v & 3 of block v >> 2
   of frame l (tags 0..2: ldpc_hip_set_noise; tag 3: ldpc_hip_bit_flip_batch). */
typedef struct
{
    uint32_t legs;             /* 1..256 */
    uint32_t first_iterations; /* 1..65535: iterations leg 0 may take */
    uint32_t leg_iterations;   /* 1..65535: iterations every later leg may take */
    uint32_t stop_after;       /* 1..legs: the call ends for a frame once this many legs have met s */
    int q_bits;                /* 2..8 */
    double step;               /* 2^-20 .. 2^20 */
    double scale;              /* (0, 1] */
    double offset;             /* [0, 1e6] */
    int form;                  /* 0 = the library chooses, 1 = a workgroup per frame, 2 = a wave per frame; same results */
    int flags;                 /* LDPC_HIP_SYNDROME_SHARED_LLR or 0 */
} ldpc_hip_relay_decode;
int ldpc_hip_relay_decode_batch(ldpc_hip_ctx *ctx, const ldpc_hip_relay_decode *p, uint64_t n, const void *llr, int llr_type,
                                const void *syndrome, int syndrome_format, const int8_t *gamma, uint32_t *hard_bits,
                                uint32_t *iters, uint32_t *weight, uint32_t *solutions, uint32_t *best_leg, uint32_t *cost,
                                void *hip_stream);
/* LDS bytes one frame of ldpc_hip_relay_decode_batch takes on this context's code in `form` (host only; 0 = either form),
   -1 for a code the call does not take, a form outside 0..2, or form 2 on a code of which four frames exceed 160 KB.  With
   `slots` as for ldpc_hip_syndrome_decode_lds_bytes and every term rounded up to 16:
     bytes = r16(slots) + r16(4 nc) + 160 + r16(4 ceil(mc / 32)) + r16(nc) + r16(4 ceil(nc / 32))
   — the frame of ldpc_hip_syndrome_decode_lds_bytes and behind it the kept word, a bit per column.  The cost's reduction
   takes the four partial sums that are part of the 160 bytes (form 2 reduces in registers): no byte more.  The same number
   in both forms; a workgroup of form 2 takes four times as much. */
int64_t ldpc_hip_relay_decode_lds_bytes(const ldpc_hip_ctx *ctx, int form);

/* channel point x of stream mt19937_64(seed): set_channel_param semantics, frame position := 0 */
int ldpc_hip_stream_begin(ldpc_hip_ctx *ctx, int channel, uint64_t seed, double x);
/* advance the stream by n frames without decoding them */
int ldpc_hip_stream_skip(ldpc_hip_ctx *ctx, uint64_t n, void *hip_stream);
/* channel + LLR init + decode of the next n frames of the stream, fused in one launch */
int ldpc_hip_stream_decode(ldpc_hip_ctx *ctx, decoder_param dec, uint64_t n, const ldpc_hip_out *out,
                           void *hip_stream);
/* the counters ldpc_sim::start accumulates per frame (ldpcsim.cpp:175-200), summed over a batch on the device:
   counters[0..4] = {frames, frame errors (bit_errors > 0), bit errors, iterations, frames that stopped early
   (iters < max_iters; 0 unless early_term)}.  iters / bit_errors / counters are DEVICE pointers (the outputs of a
   decode call on the same stream); one launch, ordered on hip_stream.  A multi-GPU run all-reduces these five. */
int ldpc_hip_batch_counters(ldpc_hip_ctx *ctx, const uint32_t *iters, const uint32_t *bit_errors, uint64_t n,
                            uint32_t max_iters, int early_term, int64_t *counters, void *hip_stream);
/* frames consumed / raw 64-bit draws consumed since ldpc_hip_stream_begin */
uint64_t ldpc_hip_stream_frame(const ldpc_hip_ctx *ctx);
uint64_t ldpc_hip_stream_raw_draws(const ldpc_hip_ctx *ctx);
int ldpc_hip_synchronize(ldpc_hip_ctx *ctx, void *hip_stream);

/* time kernels with HIP events: which = 0 the decode launches (recorded on the launch stream), 1 the noise-stream
   refills (jump-ahead + generator + slab table, recorded on the library's internal stream); host wall-clock: which = 2 the
   time the calling thread spent inside the ranks' exchange (all-gather) of a sharded step, 3 the time it waited for the
   noise stream's result (both: mean milliseconds per step since the previous call).  Event pairs are queued
   per launch; ldpc_hip_last_ms waits for them and returns the MEAN duration in milliseconds of the launches since
   the previous call (so a caller that reads it once per launch sees that launch, and a caller that reads it after
   a loop does not serialise the overlap of the noise stream with the decode) */
void ldpc_hip_set_profiling(ldpc_hip_ctx *ctx, int on);
float ldpc_hip_last_ms(ldpc_hip_ctx *ctx, int which);

/* first n outputs of std::mt19937_64(seed) starting at output `first`, produced by the device
   generator (jump-ahead + parallel chunks); out is device or host memory */
int ldpc_hip_mt64(ldpc_hip_ctx *ctx, uint64_t seed, uint64_t first, uint64_t n, uint64_t *out, void *hip_stream);

/* self-test of the device arithmetic: n pseudo-random positive operand pairs (a, b) with a, b and a/b inside
   2^-+1000 go through the division sequence the likelihood-ratio kernels use (detmath.h, dm_ratio_div) and through
   the IEEE division; *mismatches receives the number of pairs whose quotients differ in any bit (expected: 0) */
int ldpc_hip_selftest_division(ldpc_hip_ctx *ctx, uint64_t n, uint64_t seed, uint64_t *mismatches);

/* the kernels' arithmetic, element by element, for tests that hold it against libm and extended-precision host values
   rather than against the same header compiled for the host: out[i] = fn(a[i] [, b[i]]) for the scalar functions
   (fn 0..9: dm_exp, dm_log, dm_boxplus, dm_ratio_div, dm_ratio_rho, dm_ratio_lambda, dm_e_combine, dm_exp_clamped,
   dm_boxplus_exp, dm_boxplus_log of libldpc_amd/csrc/detmath.h), out[i][0..D) = check-node update of the row
   a[i][0..D) for fn 10..14 (likelihood-ratio form, D = 3, 4, 5, 6, 8), fn 15, 16 (LLR domain, D = 4, 6), fn 17..19 (shared
   reciprocals, D = 3, 4, 6) and fn 25..27 (LLR domain, D = 3, 5, 16).  fn 20..24 are the fused form's check nodes (dm_cnf2,
   dm_cnf3, dm_cnf4 with shared reciprocals, dm_cnf3 and dm_cnf4 with every output divided on its own), rows of D + 2:
   a[i] = {v_0 .. v_{D-1}, flip | leaf << 4, 0} -> out[i] = {messages, leaf_bit, leaf_tot}, a row of NaN where the node
   reports a product beyond its range.  fn 28: the range predicates of detmath.h on a[i] as a bit mask held in a double.
   a, b, out are HOST buffers of n (x row width) doubles; b may be NULL for one-operand functions. */
int ldpc_hip_selftest_math(ldpc_hip_ctx *ctx, int fn, uint64_t n, const double *a, const double *b, double *out);

/* host-only self-tests of the noise stream's chunk-state bookkeeping (libldpc_amd/csrc/mtstates.hpp; no GPU needed): the
   planned operations are replayed on a symbolic table in which every row records which chunk's state it holds.
   chunk_table: n_requests requests of chunks_per_request consecutive chunks each, `gap` chunks apart (0 = one rank reading
   the stream front to back; > 0 = a rank of a sharded BSC / BEC stream), starting at first_chunk.  Returns the number of
   jump-ahead tasks issued in total, or UINT64_MAX if an operation read a row without a valid state or a request was left
   without its rows.
   shard_table: `steps` sharded AWGN steps of rank `rank` of `world` (piece_chunks chunks + the margin chunk per rank and
   step).  Returns the jump-ahead tasks of the steps AFTER the first (and their launches in *launches): piece_chunks + 1
   per step whatever the world size — or UINT64_MAX as above. */
uint64_t ldpc_hip_selftest_chunk_table(uint64_t first_chunk, uint64_t chunks_per_request, uint64_t n_requests, uint64_t gap);
uint64_t ldpc_hip_selftest_shard_table(int world, int rank, uint32_t piece_chunks, uint64_t steps, uint64_t *launches);
/* jump-ahead tasks (one task = one chunk start state advanced by one polynomial) this context's noise stream has launched */
uint64_t ldpc_hip_jump_tasks(const ldpc_hip_ctx *ctx);

/* the simulation loop of ldpc_sim::start (ldpcsim.cpp:97-263) on one context; totals[4*i..] =
   {frames, fec, bec, iters} per channel point.  Returns the number of channel points, <0 on error. */
int ldpc_hip_simulate(ldpc_hip_ctx *ctx, decoder_param dec, channel_param ch, simulation_param sim,
                      sim_results_t *results, uint64_t *totals, bool *stopFlag, int cli_output);

/* ------------------------------------------------------------------------------------------ */
/* Part 3 — several GPUs, one process per GPU                                     */
/* ------------------------------------------------------------------------------------------ */
/* The reference shares its counters between OpenMP threads (ldpcsim.cpp:175-252); here the ranks of a sharded
   simulation exchange them, and the accepted-pair counts that place each rank in the one noise stream, through a
   communicator: RCCL over xGMI (one rank per GPU), or a host shared-memory segment for rehearsals in which ranks
   share a GPU and for tests without one.  All payloads are a few 64-bit words per rank. */
typedef struct ldpc_hip_comm ldpc_hip_comm;

/* rank 0 obtains an RCCL unique id (ncclGetUniqueId: 128 bytes) and hands the bytes to every rank by whatever means
   the launcher has (torch.distributed in bench.py, pipes in `ldpcsim --devices`) */
int ldpc_hip_comm_unique_id(uint8_t id[128]);
/* RCCL communicator of `world` ranks; this rank uses GPU `device` (ncclCommInitRank: collective, blocks) */
ldpc_hip_comm *ldpc_hip_comm_create(int rank, int world, int device, const uint8_t id[128]);
/* host shared-memory communicator; `name` ("/something") is the same on every rank and unique to the job */
ldpc_hip_comm *ldpc_hip_comm_create_shm(int rank, int world, const char *name);
/* one process standing in for rank `rank` of `world`, no transport: every rank's slot of an all-gather is answered with the
   caller's own payload.  For cost probes of the sharded step on one GPU (tools/shard_probe.py), not for results. */
ldpc_hip_comm *ldpc_hip_comm_create_echo(int rank, int world);
void ldpc_hip_comm_destroy(ldpc_hip_comm *comm);
/* recv[q*bytes ..) = rank q's send[0 .. bytes): host buffers, bytes a multiple of 8 and at most 256.  Never waits without a
   bound: when a rank does not arrive within LDPC_AMD_COMM_TIMEOUT_S seconds (default 60; ncclCommInitRank in
   ldpc_hip_comm_create likewise) the call fails on the ranks that wait for it and the communicator is unusable from then on */
int ldpc_hip_comm_allgather(ldpc_hip_comm *comm, const void *send, void *recv, uint64_t bytes);
/* the plan of the fused form of the first ratio launch (libldpc_amd/csrc/fused_rule.h decides which codes
   take it): info = {the code qualifies, message slots, variable-node blocks per wave, leaf calls per wave, the small
   instantiation applies, check-node calls per wave + 1, the code has shortened bits, entries of the slot table} */
void ldpc_hip_fused_plan_info(const ldpc_hip_ctx *ctx, int64_t info[8]);
/* index of the compile-time wave program whose shape that plan has (libldpc_amd/csrc/fused_program.hpp): the first ratio
   launch then runs the program's kernel instead of interpreting the plan; -1: no program (or no fused plan).  Host only */
int ldpc_hip_fused_program(const ldpc_hip_ctx *ctx);
/* the launches a batch decoded with `dec` takes on this context, in order (host only; honours ldpc_hip_set_fast_mode,
   ldpc_hip_set_min_sum_schedule, ldpc_hip_set_min_sum_quantization, ldpc_hip_set_min_sum_ternary and ldpc_hip_set_min_sum_layered_fixed): stages[i] = 0 whole, 1 ratio-first, 2 ratio-separate, 3 list-chain,
   4 llr-redo, 5 handover-first, 6 handover-resume; returns their number, 1 to 3 */
int ldpc_hip_decode_stages(const ldpc_hip_ctx *ctx, decoder_param dec, int32_t stages[3]);
/* the decoder that runs such a batch (host only; the same switches): 0 resident (the library's own choice by the code),
   1 fast32, 2 layered32, 3 layered16 (ldpc_hip_set_fast_mode 1 / 2 / 3, sum-product only), 4 layered min-sum, 5 quantized
   min-sum, 6 ternary min-sum, 7 fixed-point layered min-sum ("BP_MS" only).  Anything but 0 is one `whole` launch. */
int ldpc_hip_decoder_choice(const ldpc_hip_ctx *ctx, decoder_param dec);
/* Host arithmetic only. The simulation loop's counters over given per-frame results. Frames [0, n) are presented as
   consecutive ranges; ends[k] is the end of range k (ascending, <= n; ranges may be empty); `world` consecutive ranges form
   one step (world == 1: the ranges are the batches of the one-rank loop, world > 1: the ranks' ranges of a sharded step).
   out[0..3] = frames, fec, bec, iters (the `totals` of ldpc_hip_simulate); out[4], out[5] = frames and iterations at the
   last published report (0, 0: none); out[6] = 1 if the stop rule fired; out[7] = frames of the last step that counted
   (what the encoder is advanced by). Returns the number of steps walked, -1 on bad arguments. */
int ldpc_hip_selftest_sim_fold(const uint32_t *iters, const uint32_t *bit_errors, uint64_t n, const uint64_t *ends,
                               uint64_t n_ranges, int world, uint64_t min_fec, uint64_t max_frames, uint64_t out[8]);
/* the steps of the layered schedule of the non-parity modes 2 / 3 (host only): step_of_row[mc] = the step each check node
   is processed in; returns the number of steps, -1 when the schedule does not take the code.  step_of_row == NULL: returns
   how many times the context has built that plan so far instead (at most once, whoever asks for it) */
int ldpc_hip_selftest_layer_plan(ldpc_hip_ctx *ctx, int32_t *step_of_row);
/* the placement step of ldpc_hip_stream_decode_sharded by itself, without a GPU (tests): this rank reports {pairs in its
   piece, pairs including the margin, status}; after the all-gather over `comm` out = {first frame, frames of this rank,
   frames of the step, stream index of the piece's first pair, stream index of the first pair after the step}.  A non-zero
   status on any rank, a piece with more frames than cap, or a frame beyond a margin fails the call on every rank. */
int ldpc_hip_selftest_place(ldpc_hip_comm *comm, uint64_t nct, uint64_t pairs_before, uint64_t frame_pos, uint64_t cap,
                            uint64_t piece_pairs, uint64_t pairs_with_margin, uint64_t status, uint64_t out[5]);
/* host microseconds spent inside the communicator's all-gathers since the last reset: out = {calls, min, median, max} */
void ldpc_hip_comm_stats(ldpc_hip_comm *comm, double out[4], int reset);
/* "rccl 2.22.3", "shm" or "echo" (valid until the communicator is destroyed) */
const char *ldpc_hip_comm_describe(ldpc_hip_comm *comm);

/* frames the output buffers of ldpc_hip_stream_decode_sharded must hold for a step of target_frames frames: a bound (every
   trial of a piece accepted), not a statistical estimate */
uint64_t ldpc_hip_shard_capacity(const ldpc_hip_ctx *ctx, uint64_t target_frames, int world);
/* this rank's share of the next global step of about target_frames frames of the stream (all ranks call it with the same
   arguments).  AWGN: the step is a range of the raw mt19937_64 stream cut into `world` pieces of whole generator chunks;
   each rank generates its own piece only (its chunk start states are the previous step's advanced by one polynomial), one
   all-gather of the accepted-pair counts tells every rank where its piece starts in the pair sequence, and a frame belongs
   to the rank whose piece holds its first pair.  The step holds whatever frames its raw range holds (at least one chunk
   per rank).  BSC / BEC: even split.  A failure on any rank makes every rank return an error from the same call.
   step[0..3] = first frame and frame count of the global step, first frame and frame count of this rank. */
int ldpc_hip_stream_decode_sharded(ldpc_hip_ctx *ctx, ldpc_hip_comm *comm, decoder_param dec, uint64_t target_frames,
                                   const ldpc_hip_out *out, uint64_t step[4], void *hip_stream);
/* ldpc_hip_simulate over the ranks of `comm`: every rank returns the counters of the one-rank run with the same
   arguments (the stop rule of ldpcsim.cpp:255 is applied in stream order across the ranks); rank 0 prints and writes
   the result file */
int ldpc_hip_simulate_sharded(ldpc_hip_ctx *ctx, ldpc_hip_comm *comm, decoder_param dec, channel_param ch,
                              simulation_param sim, sim_results_t *results, uint64_t *totals, bool *stopFlag,
                              int cli_output);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* LDPC_AMD_H */
