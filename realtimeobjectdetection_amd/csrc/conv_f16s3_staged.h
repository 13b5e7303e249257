// The LDS-staged main loop of the split-f16 implicit-GEMM kernels that stage both operands through registers: the generic tiles
// (conv_igemm_f16s3.hip), the 16-channel tiles (conv_c16_f16s3.hip) and the K-sliced tiles (conv_ks_f16s3.hip).  A kernel brings
// its `gload` (where the 16-byte pieces of the next K-chunk come from, and how its cursor advances); everything between those
// loads and the accumulators exists ONCE, in this header and its two .inc files: the register stage sets, the counted
// wait with its register ties, the tile constants, the swizzled LDS image, the fragment reads, the three-product MFMA block and the
// schedule (prologue, steady state, drain).
//
// This is the one home of the stage-set rule ("Two GPU memory-access faults of round 2"): gload's loads go
// through inline asm, so a register of a stage set may be touched only after wait_stage has retired its load AND named it as
// in/out, and the pipeline must not end before both sets have been named after a vmcnt(0).
//
// Main loop: BM x BN x 32 per stage = one k32 step of 16x16x32 MFMAs; LDS double-buffered, four 64-byte-row f16 panels per stage
// (two in a plain-f16 instance) with a 16-byte-chunk XOR swizzle (chunk ^= (row>>1)&3: conflict-free ds_read_b128 for 16 rows x 4
// chunks per read, tools/lds_bank_sim.py); two register stage sets keep two K-chunks of global loads in flight; one barrier per
// K-chunk.
//
// Why includes: the LDS write, the fragment reads, the MFMA block (conv_f16s3_staged_defs.inc) and the schedule
// (conv_f16s3_staged_run.inc) are kernel-body text, not member functions.  Written as __forceinline__ members of StagedTile with the schedule in a
// `run(acc, kc0, kc1, gload)`, the same statements in the same order compiled to 2 ... 4 more VGPRs in 33 of the 154 instances of
// the three kernels, and five instances lost a wave per SIMD (64x64 generic with a hosted 1x1: 96 -> 98 VGPRs, occupancy 5 -> 4):
// value numbering then hoists pixel-origin + channel-offset sums of gload out of the steady state into registers of their own.
// Neither inlining attributes nor where the stage sets and fragments are declared changed that; the text form compiles to the
// registers of the three former copies (profiles/experiments/staged_loop_resource_usage.txt).
#pragma once
#include "conv_f16s3_common.h"

namespace rtod {

// The 16-byte pieces one thread loads for one K-chunk: ASL rows of the A panel, BSL rows of the B panel, hi and lo plane each
// (plain-f16 instances leave al / bl untouched).
template <int ASL, int BSL>
struct StageRegs {
    u32x4 ah[ASL], al[ASL], bh[BSL], bl[BSL];
};

// Wait until at most one stage set's loads (the younger set) are outstanding: the older set S has landed.  Every register of S
// is an in/out operand so no use can be scheduled above the wait.
template <bool F16, int A_SLOTS, int B_SLOTS>
__device__ __forceinline__ void wait_stage(StageRegs<A_SLOTS, B_SLOTS>& S) {
    static_assert(A_SLOTS >= 1 && A_SLOTS <= 2 && B_SLOTS >= 1 && B_SLOTS <= 2, "stage shape");
    if constexpr (F16 && A_SLOTS == 2 && B_SLOTS == 2)
        asm volatile("s_waitcnt vmcnt(4)" : "+v"(S.ah[0]), "+v"(S.ah[1]), "+v"(S.bh[0]), "+v"(S.bh[1]) :: "memory");
    else if constexpr (F16 && A_SLOTS == 2 && B_SLOTS == 1)
        asm volatile("s_waitcnt vmcnt(3)" : "+v"(S.ah[0]), "+v"(S.ah[1]), "+v"(S.bh[0]) :: "memory");
    else if constexpr (F16 && A_SLOTS == 1 && B_SLOTS == 2)
        asm volatile("s_waitcnt vmcnt(3)" : "+v"(S.ah[0]), "+v"(S.bh[0]), "+v"(S.bh[1]) :: "memory");
    else if constexpr (F16)
        asm volatile("s_waitcnt vmcnt(2)" : "+v"(S.ah[0]), "+v"(S.bh[0]) :: "memory");
    else if constexpr (A_SLOTS == 2 && B_SLOTS == 2)
        asm volatile("s_waitcnt vmcnt(8)" : "+v"(S.ah[0]), "+v"(S.al[0]), "+v"(S.ah[1]), "+v"(S.al[1]),
                     "+v"(S.bh[0]), "+v"(S.bl[0]), "+v"(S.bh[1]), "+v"(S.bl[1]) :: "memory");
    else if constexpr (A_SLOTS == 2 && B_SLOTS == 1)
        asm volatile("s_waitcnt vmcnt(6)" : "+v"(S.ah[0]), "+v"(S.al[0]), "+v"(S.ah[1]), "+v"(S.al[1]),
                     "+v"(S.bh[0]), "+v"(S.bl[0]) :: "memory");
    else if constexpr (A_SLOTS == 1 && B_SLOTS == 2)
        asm volatile("s_waitcnt vmcnt(6)" : "+v"(S.ah[0]), "+v"(S.al[0]),
                     "+v"(S.bh[0]), "+v"(S.bl[0]), "+v"(S.bh[1]), "+v"(S.bl[1]) :: "memory");
    else
        asm volatile("s_waitcnt vmcnt(4)" : "+v"(S.ah[0]), "+v"(S.al[0]), "+v"(S.bh[0]), "+v"(S.bl[0]) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// BM x BN workgroup tile, NWM x NWN waves of (BM/NWM) x (BN/NWN), both multiples of 16.  F16: plain-f16 instance (hi planes only:
// half the loads and LDS panels, one MFMA per fragment pair).
template <int BM, int BN, int NWM, int NWN, bool F16>
struct StagedTile {
    static constexpr int WM = BM / NWM, WN = BN / NWN;
    static constexpr int NT = NWM * NWN * 64;
    static_assert(WM % 16 == 0 && WN % 16 == 0 && BM % NWM == 0 && BN % NWN == 0, "wave tile");
    static constexpr int TM = WM / 16, TN = WN / 16;
    static constexpr int RPP = NT / 4;                    // rows per pass: 4 x 16-B chunks per 64-B row
    static constexpr int A_SLOTS = (BM + RPP - 1) / RPP, B_SLOTS = (BN + RPP - 1) / RPP;
    static_assert(RPP % 16 == 0, "predication per 16-row wave slice; swizzle period 8");
    // a pass that runs past the panel (BM or BN not a multiple of RPP) is predicated per 16-row wave
    // slice: its loads are issued out of range (the vmcnt count per stage stays constant) and its LDS
    // writes are skipped
    static constexpr int PANEL_A = BM * 64, PANEL_B = BN * 64;        // bytes
    static constexpr int STAGE = (F16 ? 1 : 2) * (PANEL_A + PANEL_B);     // [A hi][A lo][B hi][B lo], f16: [A hi][B hi]
    static constexpr int PANEL_B0 = (F16 ? 1 : 2) * PANEL_A;                  // offset of the B hi panel
    // the epilogue's transpose tile needs at least one WM-row pass of BN fp32 (f16 128x256: 64 KiB against 48 KiB of stages)
    static constexpr int SMEM = 2 * STAGE > WM * BN * 4 ? 2 * STAGE : WM * BN * 4;
    static constexpr int LOADS_PER_STAGE = (F16 ? 1 : 2) * (A_SLOTS + B_SLOTS);
    static_assert(LOADS_PER_STAGE <= 8, "vmcnt literals of wait_stage");
    using Regs = StageRegs<A_SLOTS, B_SLOTS>;

    static __device__ __forceinline__ void zero(f32x4 (&acc)[TM][TN]) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;
    }
};

}  // namespace rtod
