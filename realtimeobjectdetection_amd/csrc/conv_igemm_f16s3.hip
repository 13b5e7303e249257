// Implicit-GEMM convolution on split-precision f16 MFMA (v_mfma_f32_16x16x32_f16), gfx950.
//
// Same contract, GEMM view and epilogues as conv_igemm_f32.hip (reference: conv -> BN(eval) -> leaky,
// src/darknet.py:467-501; shortcut 263-268; head decode src/util.py:193-237), but the contraction
// runs at the f16 matrix rate (16x the exact-fp32 MFMA per product) with fp32-class accuracy:
//
//   x = xh + xl  (xh = f16(x), xl = f16(x - xh): 22 significant bits), same for the weights
//   a*w ~= ah*wh + ah*wl + al*wh      three MFMA products, fp32 accumulate; al*wl ~ 2^-22 dropped
//
// Data format ("split" activations): every activation tensor of a precision-1 plan is NHWC with each
// pixel stored as [ldc halves: hi plane][ldc halves: lo plane] of the value PRE-SCALED by
// SPLIT_SCALE = 8 (power of two, keeps low parts of small activations out of the f16 subnormal
// range; |activation| must stay < 8188).  Same bytes per pixel as fp32.  Producers (this kernel's
// epilogue, the stem conv, upsample) write it, so staging an A tile is a pure 16-byte copy exactly
// like the pre-split weight planes: no conversion VALU in the main loop.
// Weights: [Kpad/32][Npad][32] hi and lo planes (K-chunk major), per-output-channel power-of-two pre-scale undone (exactly)
// in the epilogue through inv_scale[n].
//
// Main loop: BMxBNx32 per stage = one k32 step of 16x16x32 MFMAs (the shape the chip clocks highest on, and
// whose 16-row granularity allows 48-row wave tiles: conv_band_f16s3.hip); LDS double-buffered, four
// 64-byte-row f16 panels per stage with a 16-byte-chunk XOR swizzle (chunk ^= (row>>1)&3: conflict-free
// ds_read_b128 for 16 rows x 4 chunks per read, tools/lds_bank_sim.py); two register stage sets keep two
// K-chunks of global loads in flight; one barrier per K-chunk.
// K order: k = ((c/32)*kh*kw + tap)*32 + c%32 (channel chunk outer, tap inner).
// Addressing: the tap (ky,kx) and channel offset of a K-chunk are wave-uniform (Cin % 32 == 0) and
// advanced in scalar registers; loads are raw buffer loads whose per-lane voffset is
// pixel-origin + tap offset, forced out of range (-> zeros) for padding taps and rows >= M.
#include "conv_f16s3_common.h"
#include <cstdio>
#include <cstdlib>

namespace rtod {

// Diagnostic build only (make stamps, -DRTOD_STAMPS): per-wave s_memtime attribution of the phases, as in conv_band_f16s3.hip.
#ifdef RTOD_STAMPS
constexpr int GSTAMP_SLOTS = 8, GSTAMP_BLOCKS = 128, GSTAMP_WAVES = 16;
__device__ unsigned long long g_igemm_stamps[GSTAMP_BLOCKS * GSTAMP_WAVES * (GSTAMP_SLOTS + 1)];
#define RTOD_GSTAMP(i) { const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); ts_[i] += tn_ - tprev_; tprev_ = tn_; }
#else
#define RTOD_GSTAMP(i)
#endif

template <int ASL, int BSL>
struct StageRegs {
    u32x4 ah[ASL], al[ASL], bh[BSL], bl[BSL];
};

// BM x BN workgroup tile, NWM x NWN waves of (BM/NWM) x (BN/NWN), both multiples of 16.  MINW = waves per SIMD the
// register budget must admit (2nd __launch_bounds__ argument): wave tiles of 32x64 / 48x32 or smaller are built for
// 4 waves/SIMD — tools/ubench_tiles.hip: occupancy buys more MFMA utilisation than a larger wave tile.
// EPI | EPI_F16: plain-f16 instance (hi planes only: half the loads and LDS panels, one MFMA per fragment pair).
// EPI_SPLIT | EPI_RAW: raw-sum instance (the f16s3 main loop as it stands; the epilogue stores the fp32 sums to ConvArgs::raw_out).
template <int BM, int BN, int NWM, int NWN, int MINW, int EPI>
__global__ __launch_bounds__(NWM * NWN * 64, MINW)
void conv_igemm_f16s3_kernel(const ConvArgs a, const int grid_m, const int grid_n) {
    constexpr bool F16 = epi_f16(EPI);
    constexpr int WM = BM / NWM, WN = BN / NWN;
    constexpr int NT = NWM * NWN * 64;
    static_assert(WM % 16 == 0 && WN % 16 == 0 && BM % NWM == 0 && BN % NWN == 0, "wave tile");
    constexpr int TM = WM / 16, TN = WN / 16;
    constexpr int RPP = NT / 4;                    // rows per pass: 4 x 16-B chunks per 64-B row
    constexpr int A_SLOTS = (BM + RPP - 1) / RPP, B_SLOTS = (BN + RPP - 1) / RPP;
    static_assert(RPP % 16 == 0, "predication per 16-row wave slice; swizzle period 8");
    // a pass that runs past the panel (BM or BN not a multiple of RPP) is predicated per 16-row wave
    // slice: its loads are issued out of range (the vmcnt count per stage stays constant) and its LDS
    // writes are skipped
    constexpr int PANEL_A = BM * 64, PANEL_B = BN * 64;        // bytes
    constexpr int STAGE = (F16 ? 1 : 2) * (PANEL_A + PANEL_B);     // [A hi][A lo][B hi][B lo], f16: [A hi][B hi]
    constexpr int PANEL_B0 = (F16 ? 1 : 2) * PANEL_A;                  // offset of the B hi panel
    // the epilogue's transpose tile needs at least one WM-row pass of BN fp32 (f16 128x256: 64 KiB against 48 KiB of stages)
    constexpr int SMEM = 2 * STAGE > WM * BN * 4 ? 2 * STAGE : WM * BN * 4;

    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];

    const int nwg = grid_m * grid_n;
    int bid = blockIdx.x;
    bid = xcd_remap(bid, nwg);                                   // blocks sharing an A row-panel run on one XCD / L2
    const int bm = bid / grid_n, bn = bid - bm * grid_n;

    const int tid = threadIdx.x;
    const int M = a.B * a.Ho * a.Wo;
    const int c16 = tid & 3, row0 = tid >> 2;
    const unsigned PS = (unsigned)a.in_ldc * 4u;                 // bytes per pixel (hi plane + lo plane)
    const unsigned lo_plane = (unsigned)a.in_ldc * 2u;

    // ---- A: per-slot pixel origin (receptive-field corner), byte offset may be "negative" (wraps)
    int iy0[A_SLOTS], ix0[A_SLOTS];
    unsigned pbase[A_SLOTS];
#pragma unroll
    for (int i = 0; i < A_SLOTS; ++i) {
        const int m = bm * BM + row0 + i * RPP;
        if (m < M && row0 + i * RPP < BM) {
            const int hw = a.Ho * a.Wo;
            const int b = m / hw, r = m - b * hw;
            const int oy = r / a.Wo, ox = r - oy * a.Wo;
            iy0[i] = oy * a.stride - a.pad;
            ix0[i] = ox * a.stride - a.pad;
            pbase[i] = (unsigned)((b * a.Hi + iy0[i]) * a.Wi + ix0[i]) * PS + (unsigned)(a.in_coff + c16 * 8) * 2u;
        } else {
            iy0[i] = -(1 << 28); ix0[i] = 0; pbase[i] = 0;
        }
    }
    // ---- B: per-slot row offset in the weight planes
    unsigned wbase[B_SLOTS];
#pragma unroll
    for (int i = 0; i < B_SLOTS; ++i)
        wbase[i] = (row0 + i * RPP < BN) ? (unsigned)((bn * BN + row0 + i * RPP) * 32 + c16 * 8) * 2u : OOB;
    const unsigned wchunk = (unsigned)a.Npad * (HBK * 2);        // bytes of one K-chunk panel of a weight plane

    const __amdgpu_buffer_rsrc_t rs_a = buffer_rsrc(a.in, a.in_bytes);
    const __amdgpu_buffer_rsrc_t rs_wh = buffer_rsrc(a.w_hi, a.w_bytes);
    const __amdgpu_buffer_rsrc_t rs_wl = buffer_rsrc(a.w_lo, a.w_bytes);

    // wave-uniform K-chunk cursor: tap (ky,kx) and first channel c0 of the chunk to be LOADED next
    int ld_kc = 0, ld_c0 = 0, ld_ky = 0, ld_kx = 0;
    const int nk = a.Kpad / HBK;

    StageRegs<A_SLOTS, B_SLOTS> S0, S1;
    auto gload = [&](StageRegs<A_SLOTS, B_SLOTS>& S) {
        // chunks past the end of K (issued unconditionally to keep the loop branch-free, so that the
        // compiler's vmcnt bookkeeping stays exact) read out of range -> zeros
        const bool live = ld_kc < nk;
        const unsigned tap_off = (unsigned)(ld_ky * a.Wi + ld_kx) * PS + (unsigned)ld_c0 * 2u;
#pragma unroll
        for (int i = 0; i < A_SLOTS; ++i) {
            const bool ok = live && (unsigned)(iy0[i] + ld_ky) < (unsigned)a.Hi && (unsigned)(ix0[i] + ld_kx) < (unsigned)a.Wi;
            const unsigned vo = ok ? pbase[i] + tap_off : OOB;
            S.ah[i] = buffer_load_b128(rs_a, vo, 0u);
            if constexpr (!F16) S.al[i] = buffer_load_b128(rs_a, vo, lo_plane);
        }
        const unsigned koff = (unsigned)ld_kc * wchunk;
#pragma unroll
        for (int i = 0; i < B_SLOTS; ++i) {
            const unsigned wo = live ? wbase[i] : OOB;
            S.bh[i] = buffer_load_b128(rs_wh, wo, koff);
            if constexpr (!F16) S.bl[i] = buffer_load_b128(rs_wl, wo, koff);
        }
        // advance the cursor (scalar).  K order = (32-channel chunk outer, tap inner), the same order as the
        // band kernel and the packed weights, so every tile variant / kernel sums each output identically
        ++ld_kc;
        if (++ld_kx == a.kw) { ld_kx = 0; if (++ld_ky == a.kh) { ld_ky = 0; ld_c0 += HBK; } }
    };
    constexpr int LOADS_PER_STAGE = (F16 ? 1 : 2) * (A_SLOTS + B_SLOTS);
    static_assert(LOADS_PER_STAGE <= 8, "vmcnt literals below");
    // wait until at most `LOADS_PER_STAGE` loads (the younger stage set) are outstanding: the older set S
    // has landed.  Every register of S is an in/out operand so no use can be scheduled above the wait.
    auto wait_stage = [&](StageRegs<A_SLOTS, B_SLOTS>& S) {
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
    };
    // LDS image: panel row r, 16-B chunk c at byte r*64 + ((c ^ ((r>>1)&3)) << 4)
    const int wr_swz = (c16 ^ ((row0 >> 1) & 3)) << 4;           // RPP % 8 == 0 -> same swizzle for every slot
    auto lds_write = [&](const StageRegs<A_SLOTS, B_SLOTS>& S, int buf) {
        unsigned char* st = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < A_SLOTS; ++i) {
            const int o = (row0 + i * RPP) * 64 + wr_swz;
            if ((i + 1) * RPP <= BM || row0 + i * RPP < BM) {
                *reinterpret_cast<u32x4*>(st + o) = S.ah[i];
                if constexpr (!F16) *reinterpret_cast<u32x4*>(st + PANEL_A + o) = S.al[i];
            }
        }
#pragma unroll
        for (int i = 0; i < B_SLOTS; ++i) {
            const int o = (row0 + i * RPP) * 64 + wr_swz;
            if ((i + 1) * RPP <= BN || row0 + i * RPP < BN) {
                *reinterpret_cast<u32x4*>(st + PANEL_B0 + o) = S.bh[i];
                if constexpr (!F16) *reinterpret_cast<u32x4*>(st + PANEL_B0 + PANEL_B + o) = S.bl[i];
            }
        }
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave / NWN, wn = wave - wm * NWN;
    const int lr = lane & 15, lh = lane >> 4;
    const int co = (lh ^ ((lr >> 1) & 3)) << 4;                  // WM, WN % 16 == 0: the row's swizzle is the lane's
    const int a_row = (wm * WM + lr) * 64 + co, b_row = PANEL_B0 + (wn * WN + lr) * 64 + co;

    // the A fragments of the K-chunk are read into registers first, then the next chunk's LDS writes and the
    // global loads of the chunk after are issued, and only then the MFMA block runs (B fragments read per
    // 16-column group just ahead of their MFMAs): the LDS write drain (~80 B/clk/CU through the VGPR path) and
    // the load latency overlap with the matrix pipe instead of sitting between the MFMAs and the barrier.
    f16x8 ah[TM], al[TM];
    auto read_a = [&](int buf) {
        const unsigned char* st = smem + buf * STAGE + a_row;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            ah[i] = *reinterpret_cast<const f16x8*>(st + i * 16 * 64);
            if constexpr (!F16) al[i] = *reinterpret_cast<const f16x8*>(st + PANEL_A + i * 16 * 64);
        }
    };
    auto compute = [&](int buf) {
        const unsigned char* st = smem + buf * STAGE + b_row;
        f16x8 bh[TN], bl[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            bh[j] = *reinterpret_cast<const f16x8*>(st + j * 16 * 64);
            if constexpr (!F16) bl[j] = *reinterpret_cast<const f16x8*>(st + PANEL_B + j * 16 * 64);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if constexpr (F16) { acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0); continue; }
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
            }
    };

    // prologue: chunks 0 and 1 in flight, chunk 0 staged, chunk 2 issued.  The steady state is
    // branch-free: every half-iteration computes one chunk, stages the next and issues the load of the
    // one after (chunks >= nk are zero chunks); an odd nk costs one zero chunk of MFMAs.
    // vmcnt bookkeeping: loads complete in issue order; at every wait the older stage set has
    // LOADS_PER_STAGE loads outstanding and the younger set LOADS_PER_STAGE more behind them.
#ifdef RTOD_STAMPS
    unsigned long long ts_[GSTAMP_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev_ = __builtin_amdgcn_s_memtime();
    const unsigned long long tstart_ = tprev_;
#endif
    gload(S0);
    gload(S1);
    wait_stage(S0);
    lds_write(S0, 0);
    gload(S0);
    __syncthreads();
    RTOD_GSTAMP(0)                                    // 0: prologue
    for (int t = 0; t < nk; t += 2) {
        read_a(0);                                    // chunk t
        wait_stage(S1);
        RTOD_GSTAMP(1)                                // 1: A reads issued + wait for the staged set
        lds_write(S1, 1);                             // chunk t+1
        gload(S1);                                    // chunk t+3
        __builtin_amdgcn_sched_barrier(0);
        RTOD_GSTAMP(2)                                // 2: LDS writes + loads issued
        compute(0);
        RTOD_GSTAMP(3)                                // 3: B reads + MFMA issue
        __syncthreads();
        RTOD_GSTAMP(4)                                // 4: barrier
        read_a(1);                                    // chunk t+1
        wait_stage(S0);
        RTOD_GSTAMP(1)
        lds_write(S0, 0);                             // chunk t+2
        gload(S0);                                    // chunk t+4
        __builtin_amdgcn_sched_barrier(0);
        RTOD_GSTAMP(2)
        compute(1);
        RTOD_GSTAMP(3)
        __syncthreads();
        RTOD_GSTAMP(4)
    }
    // Drain the trailing zero-chunk loads.  Their destination registers are dead to the compiler from the moment the
    // last gload statement ends, and register-only epilogue code (address arithmetic, hoisted above this asm: "memory"
    // orders memory operations only) may be allocated into them — a load landing afterwards then zeroes a live pointer
    // (observed: 'Memory access fault on address (nil)' once the epilogue's code changed).  wait_stage names every
    // register of a set as in/out, so both sets stay allocated until the loads have landed.
    vmcnt<0>();
    wait_stage(S0);
    wait_stage(S1);
    RTOD_GSTAMP(5)                                    // 5: drain

#ifdef RTOD_DIAG
    if (a.dbg & 4) return;                            // timing experiment: no epilogue
#endif
    conv_f16s3_epilogue<BM, BN, WM, WN, NT, epi_kind(EPI), SMEM, 1, false, F16, epi_raw(EPI)>(a, acc, smem, bm, bn, tid, wm, wn, lr, lh, M);
#ifdef RTOD_STAMPS
    RTOD_GSTAMP(6)                                    // 6: epilogue
    if ((threadIdx.x & 63) == 0 && blockIdx.x < GSTAMP_BLOCKS) {
        unsigned long long* o = g_igemm_stamps + (blockIdx.x * GSTAMP_WAVES + (threadIdx.x >> 6)) * (GSTAMP_SLOTS + 1);
        for (int i = 0; i < GSTAMP_SLOTS; ++i) o[i] = ts_[i];
        o[GSTAMP_SLOTS] = tprev_ - tstart_;
    }
#endif
}

// One list drives the tile table, the launch switch and the kernel names rocprofv3 prints:
//   X(variant id, BM, BN, waves along M, waves along N, MINW)
#define RTOD_IGEMM_TILES(X) \
    X(HV_128x128, 128, 128, 2, 2, 2) X(HV_128x64, 128, 64, 2, 2, 3) X(HV_64x64, 64, 64, 2, 2, 4) X(HV_64x128, 64, 128, 2, 2, 3) \
    X(HV_256x128, 256, 128, 4, 2, 2) X(HV_128x256, 128, 256, 2, 4, 2) X(HV_128x128_8W, 128, 128, 4, 2, 4) X(HV_128x64_8W, 128, 64, 4, 2, 4) \
    X(HV_256x128_16W, 256, 128, 8, 2, 4) X(HV_192x128_8W, 192, 128, 4, 2, 2) X(HV_96x128_8W, 96, 128, 2, 4, 4) X(HV_192x128_12W, 192, 128, 6, 2, 3)

#define RTOD_X_INFO(id, bm, bn, nwm, nwn, minw) {bm, bn, "conv_igemm_f16s3<" #bm "x" #bn "," #nwm "x" #nwn ">"},
static const ConvVariantInfo kHVariants[HV_COUNT] = { RTOD_IGEMM_TILES(RTOD_X_INFO) };
#undef RTOD_X_INFO

// demangled name of the instantiation (what rocprofv3 --kernel-trace reports), for bench.py / profiles
int conv_f16s3_kernel_name(int variant, int epi, char* buf, size_t len) {
#define RTOD_X_NAME(id, bm, bn, nwm, nwn, minw) \
    if (variant == id) return snprintf(buf, len, "void rtod::conv_igemm_f16s3_kernel<" #bm ", " #bn ", " #nwm ", " #nwn ", " #minw ", %d>(rtod::ConvArgs, int, int)", epi);
    RTOD_IGEMM_TILES(RTOD_X_NAME)
#undef RTOD_X_NAME
    return -1;
}

const ConvVariantInfo& conv_f16s3_variant_info(int v) { return kHVariants[v < 0 || v >= HV_COUNT ? 0 : v]; }

template <int BM, int BN, int NWM, int NWN, int MINW>
static int launch_h(const ConvArgs& a, hipStream_t s) {
    const int M = a.B * a.Ho * a.Wo;
    const int gm = (M + BM - 1) / BM, gn = (a.Cout + BN - 1) / BN;
    constexpr int NT = NWM * NWN * 64;
    auto k_dec = conv_igemm_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_DECODE>;
    auto k_res = conv_igemm_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT_RES>;
    auto k_plain = conv_igemm_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT>;
    auto k_res_pw = conv_igemm_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT_RES_PW>;
    auto k_pw = conv_igemm_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT_PW>;
    if (a.raw_out) {
        if (a.f16 || a.pw_wh || a.dec.enabled || a.res) { set_error("conv_igemm_f16s3: a raw-sum launch carries no shortcut, decode, hosted pointwise conv or plain-f16 store"); return RTOD_E_ARG; }
        auto k_raw = conv_igemm_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT | EPI_RAW>;
        hipLaunchKernelGGL(k_raw, dim3(gm * gn), dim3(NT), 0, s, a, gm, gn);
    }
    else if (a.f16) {
        if (a.pw_wh) { set_error("conv_igemm_f16s3: plain-f16 launch with a fused pointwise conv"); return RTOD_E_ARG; }
        auto f_dec = conv_igemm_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_DECODE | EPI_F16>;
        auto f_res = conv_igemm_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT_RES | EPI_F16>;
        auto f_plain = conv_igemm_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT | EPI_F16>;
        hipLaunchKernelGGL(a.dec.enabled ? f_dec : a.res ? f_res : f_plain, dim3(gm * gn), dim3(NT), 0, s, a, gm, gn);
    }
    else if (a.pw_wh) {
        if (gn != 1 || a.dec.enabled) { set_error("conv_igemm_f16s3: fused pointwise conv needs Cout <= BN (%d > %d) and no decode", a.Cout, BN); return RTOD_E_ARG; }
        if (a.res) hipLaunchKernelGGL(k_res_pw, dim3(gm), dim3(NT), 0, s, a, gm, gn);
        else hipLaunchKernelGGL(k_pw, dim3(gm), dim3(NT), 0, s, a, gm, gn);
    }
    else if (a.dec.enabled) hipLaunchKernelGGL(k_dec, dim3(gm * gn), dim3(NT), 0, s, a, gm, gn);
    else if (a.res) hipLaunchKernelGGL(k_res, dim3(gm * gn), dim3(NT), 0, s, a, gm, gn);
    else hipLaunchKernelGGL(k_plain, dim3(gm * gn), dim3(NT), 0, s, a, gm, gn);
#ifdef RTOD_STAMPS
    {
        static int printed = 0;
        if (printed < 400 && hipDeviceSynchronize() == hipSuccess) {
            static unsigned long long h[GSTAMP_BLOCKS * GSTAMP_WAVES * (GSTAMP_SLOTS + 1)];
            if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_igemm_stamps), sizeof(h)) == hipSuccess) {
                const int nb = gm * gn < GSTAMP_BLOCKS ? gm * gn : GSTAMP_BLOCKS, nw = NWM * NWN;
                double sum[GSTAMP_SLOTS + 1] = {0};
                for (int b = 0; b < nb; ++b) for (int w = 0; w < nw; ++w) for (int i = 0; i <= GSTAMP_SLOTS; ++i)
                    sum[i] += (double)h[(b * GSTAMP_WAVES + w) * (GSTAMP_SLOTS + 1) + i];
                fprintf(stderr, "[stamps] igemm<%d,%d,%dx%d> k=%d s=%d W=%d Cin=%d Cout=%d tiles=%d steps=%d epi=%d | cycles/wave:", BM, BN, NWM, NWN, a.kh, a.stride,
                        a.Wo, a.Cin, a.Cout, gm * gn, a.Kpad / 32, a.pw_wh ? 3 : (a.dec.enabled ? 2 : (a.res ? 1 : 0)));
                for (int i = 0; i <= GSTAMP_SLOTS; ++i) fprintf(stderr, " %s%.0f", i == GSTAMP_SLOTS ? "total=" : "", sum[i] / (nb * nw));
                fprintf(stderr, "\n");
                ++printed;
            }
        }
    }
#endif
    return hip_fail(hipGetLastError(), "conv_igemm_f16s3 launch");
}

int launch_conv_f16s3(const ConvArgs& a_in, int variant, hipStream_t s) {
    ConvArgs a = a_in;
    if (int rc = check_split_conv_args(a, "launch_conv_f16s3", true)) return rc;
    if (a.Cin % HBK || a.in_ldc % 8 || a.in_coff % 8 || a.Kpad % HBK || a.K != a.Kpad || a.K != a.kh * a.kw * a.Cin) {
        set_error("launch_conv_f16s3: needs Cin %% 32 == 0 and 8-channel aligned views (Cin=%d ldc=%ld coff=%d K=%d Kpad=%d)", a.Cin, (long)a.in_ldc, a.in_coff, a.K, a.Kpad);
        return RTOD_E_ARG;
    }
    if (!a.dec.enabled && (a.out_ldc % 1 || a.out_ldc <= 0)) { set_error("launch_conv_f16s3: bad output view"); return RTOD_E_ARG; }
    if (a.B <= 0 || a.Ho <= 0 || a.Wo <= 0 || a.Cout <= 0) { set_error("launch_conv_f16s3: empty shape"); return RTOD_E_ARG; }
    if (a.pw_wh && (!a.pw_wl || !a.pw_inv_scale || !a.pw_bias || !a.pw_out || a.pw_k != a.Cout || a.pw_k % 32 || a.pw_k > PW_MAX_K ||
                    (a.pw_cout != 16 && a.pw_cout != 32 && a.pw_cout != 64) || a.pw_out_ldc % 8 || a.pw_out_coff % 8)) {
        set_error("launch_conv_f16s3: bad fused pointwise conv (k=%d cout=%d, conv Cout=%d)", a.pw_k, a.pw_cout, a.Cout); return RTOD_E_ARG;
    }
#ifdef RTOD_DIAG
    // diagnostic build only: timing experiments (cdna guide 7: zero-record descriptors drop the loads of one operand, results are garbage)
    static const int dbg_zero = getenv("RTOD_DBG_ZERO") ? atoi(getenv("RTOD_DBG_ZERO")) : 0;
    if (dbg_zero & 1) a.in_bytes = 1;
    if (dbg_zero & 2) a.w_bytes = 1;
    a.dbg = dbg_zero;
#endif
    switch (variant) {
#define RTOD_X_CASE(id, bm, bn, nwm, nwn, minw) case id: return launch_h<bm, bn, nwm, nwn, minw>(a, s);
        RTOD_IGEMM_TILES(RTOD_X_CASE)
#undef RTOD_X_CASE
    }
    set_error("launch_conv_f16s3: unknown variant %d", variant);
    return RTOD_E_ARG;
}

}  // namespace rtod
