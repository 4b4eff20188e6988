// fused_program.hpp — fused plans the library knows at compile time ("wave programs").
//
// The fused decoder (kernels_fused.hip) interprets its plan: every loop pass each wave reads its call descriptors, unpacks
// them and branches to the routine of each call's class.  The plan is a property of the code alone, so for a plan whose
// SHAPE — which calls of which class at which slot offsets each wave makes, and what its variable-node slots hold — equals
// an entry of kFusedPrograms, decode_fused_prog<P> runs the same calls in the same order as straight-line code with the
// offsets as immediates.  plan.cpp (match_fused_program) compares a built plan with every entry field by field; the kernel
// relies on nothing the matcher does not check.  What depends on the code's edges and columns (FusedPlan::lane_tab) stays
// runtime data.
#pragma once

#include <cstdint>

#include "plan.hpp"

namespace ldpc_amd
{

constexpr int kFusedProgCalls = 2; // check-node calls without a leaf a wave of a program makes, at most

// one check-node call (plan.hpp, FusedCall): nodes of degree `degree`, `leaf` of their inputs a leaf, the last `nm` of the
// message inputs handed to neighbours of degree 2; cnt0 = 0: no call; cnt1 != 0: two full blocks
struct FusedProgCall
{
    int degree, leaf, nm;
    uint32_t cnt0, cnt1; // nodes in block 0 / 1
    uint32_t off0, off1; // byte offsets of the blocks' first slots
    constexpr bool two() const { return cnt1 != 0; }
    constexpr uint32_t flip() const { return ((1u << nm) - 1u) << (degree - leaf - nm); }
    constexpr uint32_t cls() const { return static_cast<uint32_t>(degree) | (static_cast<uint32_t>(leaf) << 3) | (flip() << 4); }
    constexpr FusedCall call() const { return cnt0 ? FusedCall{off0 | (off1 << 16), cnt0 | (cnt1 << 16), cls(), 0} : FusedCall{0, 0, 0, 0}; }
    // (a pair call is two FULL blocks: the kernel's two-block routines do not look at the lane)
    constexpr bool valid() const { return cnt0 == 0 || (cnt0 <= kWaveSize && (cnt1 == 0 || (cnt0 == kWaveSize && cnt1 == kWaveSize))); }
};

struct FusedProgWave
{
    FusedProgCall leaf;                   // the wave's call with leaves (programs have at most one: the small instantiation)
    FusedProgCall calls[kFusedProgCalls]; // the others, in the plan's order; the list ends at the first cnt0 = 0
    // variable-node slots 0..3: kFusedVnPair / kFusedVn2 / kFusedVnWide (slot 0 only) / kFusedVnNone, nodes, degree
    uint32_t vn_kind[4], vn_cnt[4], vn_deg[4];
    constexpr uint32_t vn_prog() const { return vn_kind[0] | (vn_kind[1] << 4) | (vn_kind[2] << 8) | (vn_kind[3] << 12); }
    constexpr uint32_t vn_desc(int s) const { return vn_kind[s] == kFusedVnNone ? 0u : (vn_cnt[s] | (vn_deg[s] << 16)); }
};

struct FusedProgram
{
    int n_slots, vnb, cnl; // FusedPlan's; wide_exclusive is implied (a program is a shape of the small instantiation)
    FusedProgWave wave[kDecodeWaves];
};

namespace fused_program_detail
{
constexpr uint32_t kB = kWaveSize * 8u; // bytes of one message input of a full block
constexpr FusedProgCall pair(int d, int leaf, int nm, uint32_t first_slot_byte)
{
    return FusedProgCall{d, leaf, nm, kWaveSize, kWaveSize, first_slot_byte, first_slot_byte + static_cast<uint32_t>(d - leaf) * kB};
}
constexpr FusedProgCall none() { return FusedProgCall{0, 0, 0, 0, 0, 0, 0}; }
constexpr FusedProgWave wide_wave(FusedProgCall leaf, FusedProgCall rest, uint32_t dv)
{
    return FusedProgWave{leaf, {rest, none()}, {kFusedVnWide, kFusedVnNone, kFusedVnNone, kFusedVnNone}, {kWaveSize, 0, 0, 0}, {dv, 0, 0, 0}};
}
constexpr FusedProgWave pairs_wave(FusedProgCall leaf, FusedProgCall rest)
{
    return FusedProgWave{leaf, {rest, none()}, {kFusedVnPair, kFusedVnPair, kFusedVnPair, kFusedVnPair}, {kWaveSize, kWaveSize, kWaveSize, kWaveSize}, {2, 2, 2, 2}};
}
} // namespace fused_program_detail

// Entry 0: what build_fused_plan makes of the reference's n = 1024 test code.  Slots in class-key order: 2 blocks of
// degree-3 check nodes with a leaf (2 message inputs each), 6 of degree 4 with a leaf (3 each), 8 of degree 3 without a
// leaf whose last two outputs go to neighbours of degree 2 (3 each): 2 944 slots.  Each wave makes one pair call with
// leaves and one without; waves 0 and 1 serve a block of degree-15 variable nodes each, waves 2 and 3 four blocks of
// degree 2 in two lock-step pairs.
constexpr FusedProgram kFusedPrograms[] = {
    {2944, 4, 1,
     {fused_program_detail::wide_wave(fused_program_detail::pair(4, 1, 0, 2048), fused_program_detail::pair(3, 0, 2, 14336), 15),
      fused_program_detail::wide_wave(fused_program_detail::pair(4, 1, 0, 5120), fused_program_detail::pair(3, 0, 2, 17408), 15),
      fused_program_detail::pairs_wave(fused_program_detail::pair(4, 1, 0, 8192), fused_program_detail::pair(3, 0, 2, 20480)),
      fused_program_detail::pairs_wave(fused_program_detail::pair(3, 1, 0, 0), fused_program_detail::pair(3, 0, 2, 11264))}},
};
constexpr int kNumFusedPrograms = static_cast<int>(sizeof(kFusedPrograms) / sizeof(kFusedPrograms[0]));

// what decode_fused_prog is written for: checked for every entry when the table is compiled
constexpr bool fused_program_valid(const FusedProgram &p)
{
    if (p.vnb > 4 || p.cnl > 1 || static_cast<uint32_t>(p.n_slots) * 8u > 0x10000u)
        return false;
    for (const FusedProgWave &w : p.wave)
    {
        if (!w.leaf.valid() || (w.leaf.cnt0 != 0 && (w.leaf.leaf != 1 || w.leaf.degree < 3 || w.leaf.degree > 4)))
            return false;
        for (const FusedProgCall &c : w.calls)
            if (!c.valid() || (c.cnt0 != 0 && (c.leaf != 0 || c.degree < 2 || c.degree > 4)))
                return false;
        const bool wide = w.vn_kind[0] == kFusedVnWide;
        for (int s = 0; s < 4; ++s)
        {
            const uint32_t k = w.vn_kind[s];
            if (k == kFusedVnWide ? (s != 0 || w.vn_deg[s] < 3 || w.vn_deg[s] > 15 || w.vn_cnt[s] == 0 || w.vn_cnt[s] > kWaveSize)
                                  : (k == kFusedVnPair ? (w.vn_deg[s] != 2 || w.vn_cnt[s] != kWaveSize || w.vn_kind[s ^ 1] != kFusedVnPair)
                                                       : (k == kFusedVn2 ? (w.vn_deg[s] != 2 || w.vn_cnt[s] == 0 || w.vn_cnt[s] >= kWaveSize) : k != kFusedVnNone)))
                return false;
            if (wide && s > 0 && k != kFusedVnNone) // (wide_exclusive)
                return false;
        }
    }
    return true;
}
constexpr bool fused_programs_valid()
{
    for (const FusedProgram &p : kFusedPrograms)
        if (!fused_program_valid(p))
            return false;
    return true;
}
static_assert(fused_programs_valid(), "a fused program decode_fused_prog cannot run");

// index of the program whose shape `f` has, or -1 (plan.cpp; -DLDPC_AMD_FUSED_PROGRAM=0: always -1)
int match_fused_program(const FusedPlan &f);

} // namespace ldpc_amd
