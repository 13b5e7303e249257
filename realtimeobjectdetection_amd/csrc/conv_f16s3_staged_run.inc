// The schedule of the LDS-staged main loop (conv_f16s3_staged.h): acc += the K-chunks [kc0, kc1).  Included as statements, after
// conv_f16s3_staged_defs.inc, where the kernel walks a chunk range.  In scope besides the names of that file:
//   kc0, kc1        the chunk range; the kernel's cursor is seeded at kc0
//   gload           callable (typename Tile::Regs&): issues the Tile::LOADS_PER_STAGE loads of the K-chunk at the kernel's cursor
//                   with buffer_load_b128 and advances the cursor; past kc1 it still issues them, out of range (zeros)
//   RTOD_STAGED_PHASE(i)   optional macro, a statement run at the phase marks 0 ... 5 below (diagnostic stamps); default: nothing
//
// Prologue: chunks kc0 and kc0 + 1 in flight, the first staged, the third issued.  The steady state is branch-free: every
// half-iteration computes one chunk, stages the next and issues the load of the one after (chunks >= kc1 are zero chunks, so
// that the vmcnt bookkeeping stays exact; an odd chunk count costs one zero chunk of MFMAs).  vmcnt bookkeeping: loads complete
// in issue order; at every wait the older stage set has LOADS_PER_STAGE loads outstanding and the younger set
// LOADS_PER_STAGE more behind them.
// A_AHEAD: the A fragments of the K-chunk are read into registers first, then the next chunk's LDS writes and the global
// loads of the chunk after are issued, and only then the MFMA block runs (B fragments read just ahead of their MFMAs): the LDS
// write drain (~80 B/clk/CU through the VGPR path) and the load latency overlap with the matrix pipe instead of sitting
// between the MFMAs and the barrier.
// Ends on a barrier with no load in flight: LDS may be reused at once (the next slice, the epilogue's transpose tile).
#ifndef RTOD_STAGED_PHASE
#define RTOD_STAGED_PHASE(i)
#endif
    gload(S0);
    gload(S1);
    wait_stage<F16>(S0);
    lds_write(S0, 0);
    gload(S0);
    __syncthreads();
    RTOD_STAGED_PHASE(0)                              // 0: prologue
    for (int t = kc0; t < kc1; t += 2) {
        if constexpr (A_AHEAD) read_a(0);             // chunk t
        wait_stage<F16>(S1);
        RTOD_STAGED_PHASE(1)                          // 1: A reads issued + wait for the staged set
        lds_write(S1, 1);                             // chunk t+1
        gload(S1);                                    // chunk t+3
        __builtin_amdgcn_sched_barrier(0);
        RTOD_STAGED_PHASE(2)                          // 2: LDS writes + loads issued
        compute(0);
        RTOD_STAGED_PHASE(3)                          // 3: B reads + MFMA issue
        __syncthreads();
        RTOD_STAGED_PHASE(4)                          // 4: barrier
        if constexpr (A_AHEAD) read_a(1);             // chunk t+1
        wait_stage<F16>(S0);
        RTOD_STAGED_PHASE(1)
        lds_write(S0, 0);                             // chunk t+2
        gload(S0);                                    // chunk t+4
        __builtin_amdgcn_sched_barrier(0);
        RTOD_STAGED_PHASE(2)
        compute(1);
        RTOD_STAGED_PHASE(3)
        __syncthreads();
        RTOD_STAGED_PHASE(4)
    }
    // Drain the trailing zero-chunk loads.  Their destination registers are dead to the compiler from the moment the last gload
    // statement ends, and register-only code after the loop (the epilogue's address arithmetic, hoisted above this asm:
    // "memory" orders memory operations only) may be allocated into them — a load landing afterwards then zeroes a live pointer
    // (observed: 'Memory access fault on address (nil)' once the epilogue's code changed).  wait_stage names every register of
    // a set as in/out, so both sets stay allocated until the loads have landed.
    vmcnt<0>();
    wait_stage<F16>(S0);
    wait_stage<F16>(S1);
    RTOD_STAGED_PHASE(5)                              // 5: drain
