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
// whose 16-row granularity allows 48-row wave tiles: conv_band_f16s3.hip), staged through LDS by the pipeline of
// conv_f16s3_staged.h (shared with conv_c16_f16s3.hip and conv_ks_f16s3.hip); this file holds where a K-chunk is loaded from.
// K order: k = ((c/32)*kh*kw + tap)*32 + c%32 (channel chunk outer, tap inner).
// Addressing: the tap (ky,kx) and channel offset of a K-chunk are wave-uniform (Cin % 32 == 0) and
// advanced in scalar registers; loads are raw buffer loads whose per-lane voffset is
// pixel-origin + tap offset, forced out of range (-> zeros) for padding taps and rows >= M.
#include "conv_f16s3_staged.h"
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

// BM x BN workgroup tile, NWM x NWN waves of (BM/NWM) x (BN/NWN), both multiples of 16.  MINW = waves per SIMD the
// register budget must admit (2nd __launch_bounds__ argument): wave tiles of 32x64 / 48x32 or smaller are built for
// 4 waves/SIMD — tools/ubench_tiles.hip: occupancy buys more MFMA utilisation than a larger wave tile.
// EPI | EPI_F16: plain-f16 instance (hi planes only: half the loads and LDS panels, one MFMA per fragment pair).
// EPI_SPLIT | EPI_RAW: raw-sum instance (the f16s3 main loop as it stands; the epilogue stores the fp32 sums to ConvArgs::raw_out).
template <int BM, int BN, int NWM, int NWN, int MINW, int EPI>
__global__ __launch_bounds__(NWM * NWN * 64, MINW)
void conv_igemm_f16s3_kernel(const ConvArgs a, const int grid_m, const int grid_n) {
    constexpr bool F16 = epi_f16(EPI);
    using Tile = StagedTile<BM, BN, NWM, NWN, F16>;
    constexpr int WM = Tile::WM, WN = Tile::WN, NT = Tile::NT, RPP = Tile::RPP, A_SLOTS = Tile::A_SLOTS, B_SLOTS = Tile::B_SLOTS, SMEM = Tile::SMEM;

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

    auto gload = [&](typename Tile::Regs& S) {
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

    f32x4 acc[Tile::TM][Tile::TN];
    Tile::zero(acc);
#ifdef RTOD_STAMPS
    unsigned long long ts_[GSTAMP_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long tprev_ = __builtin_amdgcn_s_memtime();
    const unsigned long long tstart_ = tprev_;
#endif
    // the shared pipeline over the whole K sum, A fragments read ahead of the wait; its phases are stamped in a diagnostic build
    constexpr bool A_AHEAD = true;
#define RTOD_STAGED_PHASE(i) RTOD_GSTAMP(i)
#include "conv_f16s3_staged_defs.inc"
    {
        const int kc0 = 0, kc1 = nk;
#include "conv_f16s3_staged_run.inc"
    }

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
