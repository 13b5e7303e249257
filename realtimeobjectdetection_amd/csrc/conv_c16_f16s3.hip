// Implicit-GEMM convolution for layers that read 16 input channels (option "narrow_cin": YOLOv3-tiny's layer 2, any cfg that
// opens with a 16-filter stem), split-precision f16 MFMA (v_mfma_f32_16x16x32_f16), gfx950.
//
// Same data formats and epilogues as conv_igemm_f16s3.hip, and the same main loop (conv_f16s3_staged.h); what differs is the K order and with it
// the A-tile addressing.  A 32-wide K-chunk cannot be one tap of 32 channels here, so it is TWO taps of 16:
//
//   k = tap * 16 + c,  tap = ky * kw + kx          K-chunk j = taps 2j and 2j + 1;  K = 16 kh kw, Kpad = 160 (3x3) / 32 (1x1)
//
// (the packed weights of a narrow layer are laid out in this order: plan_weights.cpp, pack_conv).  A 64-byte panel row is four
// 16-byte chunks; the thread that stages chunk c16 of a row loads channels 8 (c16 & 1) ... + 7 of tap 2j + (c16 >> 1).  The tap
// and the padding predicate are therefore per LANE, not per wave: a row's two taps may straddle an image border (one in range,
// one padding), and the second tap of the last chunk of an odd kh kw does not exist.  Both are sent out of range (the buffer load
// returns zeros) rather than read and multiplied by the zero weight: what lies at that address is a neighbouring pixel, or its lo
// plane, and 0 * inf would be NaN.
// These layers have K <= 160 and few output channels: they are bandwidth- and launch-bound, so the tiles are few and simple
// (no LDS-DMA, no hosted pointwise conv).  Every tile sums in the same order: results are bit-identical across tiles.
#include "conv_f16s3_staged.h"
#include <cstdio>

namespace rtod {

// BM x BN workgroup tile, NWM x NWN waves of (BM/NWM) x (BN/NWN); EPI | EPI_F16: plain-f16 instance (hi planes only).
// EPI_SPLIT | EPI_RAW: raw-sum instance (plan option bn_split_narrow): the f16s3 main loop as it stands, the shared epilogue's RAW
// branch stores the fp32 sums to ConvArgs::raw_out in rows of ConvArgs::raw_ld floats.
template <int BM, int BN, int NWM, int NWN, int MINW, int EPI>
__global__ __launch_bounds__(NWM * NWN * 64, MINW)
void conv_c16_f16s3_kernel(const ConvArgs a, const int grid_m, const int grid_n) {
    constexpr bool F16 = epi_f16(EPI);
    using Tile = StagedTile<BM, BN, NWM, NWN, F16>;
    constexpr int WM = Tile::WM, WN = Tile::WN, NT = Tile::NT, RPP = Tile::RPP, A_SLOTS = Tile::A_SLOTS, SMEM = Tile::SMEM;
    static_assert(Tile::B_SLOTS == 1, "gload below loads one B row per thread");

    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];

    const int nwg = grid_m * grid_n;
    int bid = blockIdx.x;
    bid = xcd_remap(bid, nwg);
    const int bm = bid / grid_n, bn = bid - bm * grid_n;

    const int tid = threadIdx.x;
    const int M = a.B * a.Ho * a.Wo;
    const int c16 = tid & 3, row0 = tid >> 2;
    const unsigned PS = (unsigned)a.in_ldc * 4u;                 // bytes per pixel (hi plane + lo plane)
    const unsigned lo_plane = (unsigned)a.in_ldc * 2u;

    // ---- A: per-slot pixel origin (receptive-field corner) of this lane's row; the lane's 8 channels are fixed
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
            pbase[i] = (unsigned)((b * a.Hi + iy0[i]) * a.Wi + ix0[i]) * PS + (unsigned)(a.in_coff + (c16 & 1) * 8) * 2u;
        } else {
            iy0[i] = -(1 << 28); ix0[i] = 0; pbase[i] = 0;
        }
    }
    // ---- B: row offset in the weight planes
    const unsigned wbase = (row0 < BN) ? (unsigned)((bn * BN + row0) * 32 + c16 * 8) * 2u : OOB;
    const unsigned wchunk = (unsigned)a.Npad * (HBK * 2);        // bytes of one K-chunk panel of a weight plane

    const __amdgpu_buffer_rsrc_t rs_a = buffer_rsrc(a.in, a.in_bytes);
    const __amdgpu_buffer_rsrc_t rs_wh = buffer_rsrc(a.w_hi, a.w_bytes);
    const __amdgpu_buffer_rsrc_t rs_wl = buffer_rsrc(a.w_lo, a.w_bytes);

    // K-chunk cursor of the chunk to be LOADED next: the chunk index is wave-uniform, the tap (ky, kx) is the lane's own
    // (tap 2 kc + (c16 >> 1)) and advances by two taps per chunk
    int ld_kc = 0;
    int ld_kx = c16 >> 1, ld_ky = 0;
    if (ld_kx >= a.kw) { ld_kx -= a.kw; ++ld_ky; }               // kw == 1
    const int nk = a.Kpad / HBK;

    auto gload = [&](typename Tile::Regs& S) {
        // chunks past the end of K (issued unconditionally: the loop stays branch-free and the vmcnt bookkeeping exact) and
        // taps past the last one (ld_ky >= kh) read out of range -> zeros
        const bool live = ld_kc < nk;
        const bool tap_ok = live && ld_ky < a.kh;
        const unsigned tap_off = (unsigned)(ld_ky * a.Wi + ld_kx) * PS;
#pragma unroll
        for (int i = 0; i < A_SLOTS; ++i) {
            const bool ok = tap_ok && (unsigned)(iy0[i] + ld_ky) < (unsigned)a.Hi && (unsigned)(ix0[i] + ld_kx) < (unsigned)a.Wi;
            const unsigned vo = ok ? pbase[i] + tap_off : OOB;
            S.ah[i] = buffer_load_b128(rs_a, vo, 0u);
            if constexpr (!F16) S.al[i] = buffer_load_b128(rs_a, vo, lo_plane);
        }
        const unsigned koff = (unsigned)ld_kc * wchunk;
        const unsigned wo = live ? wbase : OOB;
        S.bh[0] = buffer_load_b128(rs_wh, wo, koff);
        if constexpr (!F16) S.bl[0] = buffer_load_b128(rs_wl, wo, koff);
        ++ld_kc;
        ld_kx += 2;                                               // two taps on; kw >= 1, so at most two row wraps
        if (ld_kx >= a.kw) { ld_kx -= a.kw; ++ld_ky; }
        if (ld_kx >= a.kw) { ld_kx -= a.kw; ++ld_ky; }
    };

    f32x4 acc[Tile::TM][Tile::TN];
    Tile::zero(acc);
    // the shared pipeline over the whole K sum; in this family the A fragments are read with the B fragments, after the staging
    constexpr bool A_AHEAD = false;
#include "conv_f16s3_staged_defs.inc"
    {
        const int kc0 = 0, kc1 = nk;
#include "conv_f16s3_staged_run.inc"
    }

    conv_f16s3_epilogue<BM, BN, WM, WN, NT, epi_kind(EPI), SMEM, 1, false, F16, epi_raw(EPI)>(a, acc, smem, bm, bn, tid, wm, wn, lr, lh, M);
}

// One list drives the tile table, the launch switch and the kernel names rocprofv3 prints:
//   X(mode, BM, BN, waves along M, waves along N, MINW)
#define RTOD_C16_TILES(X) \
    X(0, 128, 32, 4, 1, 2) X(1, 64, 32, 2, 1, 2) X(2, 128, 64, 4, 1, 2) X(3, 64, 64, 2, 2, 2)

#define RTOD_X_INFO(id, bm, bn, nwm, nwn, minw) {bm, bn, "conv_c16_f16s3<" #bm "x" #bn "," #nwm "x" #nwn ">"},
static const ConvVariantInfo kC16Modes[] = { RTOD_C16_TILES(RTOD_X_INFO) };
#undef RTOD_X_INFO
static_assert(sizeof(kC16Modes) / sizeof(kC16Modes[0]) == C16_MODES, "C16_MODES (rtod_internal.h) counts this table");

const ConvVariantInfo& conv_c16_mode_info(int mode) { return kC16Modes[mode < 0 || mode >= C16_MODES ? 0 : mode]; }

// Closed form: the narrowest N tile that holds the layer's channels (these layers have 16 ... 64 of them), and the 128-row tile
// once that still gives two workgroups to each of the 256 CUs.
int conv_c16_default_mode(int cout, int64_t m) {
    const bool n32 = cout <= 32;
    const int64_t gn = n32 ? 1 : (cout + 63) / 64;
    const bool m128 = ((m + 127) / 128) * gn >= 512;
    return n32 ? (m128 ? 0 : 1) : (m128 ? 2 : 3);
}

// demangled name of the instantiation (what rocprofv3 --kernel-trace reports)
int conv_c16_kernel_name(int mode, int epi, char* buf, size_t len) {
#define RTOD_X_NAME(id, bm, bn, nwm, nwn, minw) \
    if (mode == id) return snprintf(buf, len, "void rtod::conv_c16_f16s3_kernel<" #bm ", " #bn ", " #nwm ", " #nwn ", " #minw ", %d>(rtod::ConvArgs, int, int)", epi);
    RTOD_C16_TILES(RTOD_X_NAME)
#undef RTOD_X_NAME
    return -1;
}

template <int BM, int BN, int NWM, int NWN, int MINW>
static int launch_c16(const ConvArgs& a, hipStream_t s) {
    const int M = a.B * a.Ho * a.Wo;
    const int gm = (M + BM - 1) / BM, gn = (a.Cout + BN - 1) / BN;
    constexpr int NT = NWM * NWN * 64;
    auto k_dec = conv_c16_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_DECODE>;
    auto k_res = conv_c16_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT_RES>;
    auto k_plain = conv_c16_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT>;
    auto f_dec = conv_c16_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_DECODE | EPI_F16>;
    auto f_res = conv_c16_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT_RES | EPI_F16>;
    auto f_plain = conv_c16_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT | EPI_F16>;
    auto k_raw = conv_c16_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT | EPI_RAW>;
    if (a.raw_out) hipLaunchKernelGGL(k_raw, dim3(gm * gn), dim3(NT), 0, s, a, gm, gn);
    else if (a.f16) hipLaunchKernelGGL(a.dec.enabled ? f_dec : a.res ? f_res : f_plain, dim3(gm * gn), dim3(NT), 0, s, a, gm, gn);
    else hipLaunchKernelGGL(a.dec.enabled ? k_dec : a.res ? k_res : k_plain, dim3(gm * gn), dim3(NT), 0, s, a, gm, gn);
    return hip_fail(hipGetLastError(), "conv_c16_f16s3 launch");
}

int launch_conv_c16_f16s3(const ConvArgs& a, int mode, hipStream_t s) {
    if (int rc = check_split_conv_args(a, "launch_conv_c16_f16s3", true)) return rc;
    if (!conv_c16_supported(a.Cin) || a.in_ldc % 8 || a.in_coff % 8 || a.in_coff < 0 || a.in_coff + a.Cin > a.in_ldc || a.kh < 1 || a.kw < 1 ||
        a.K != a.kh * a.kw * a.Cin || a.Kpad != (a.K + HBK - 1) / HBK * HBK || a.Npad % 128 || a.Cout > a.Npad ||
        (uint64_t)a.Npad * a.Kpad * 2ull > (uint64_t)a.w_bytes) {
        set_error("launch_conv_c16_f16s3: needs Cin == 16, 8-channel aligned views and tap-major packed weights (Cin=%d ldc=%ld coff=%d K=%d Kpad=%d Npad=%d)",
                  a.Cin, (long)a.in_ldc, a.in_coff, a.K, a.Kpad, a.Npad);
        return RTOD_E_ARG;
    }
    if (a.stride < 1 || a.pad < 0) { set_error("launch_conv_c16_f16s3: bad geometry"); return RTOD_E_ARG; }
    if (!a.dec.enabled && a.out_ldc <= 0) { set_error("launch_conv_c16_f16s3: bad output view"); return RTOD_E_ARG; }
    if (a.B <= 0 || a.Ho <= 0 || a.Wo <= 0 || a.Cout <= 0) { set_error("launch_conv_c16_f16s3: empty shape"); return RTOD_E_ARG; }
    if (a.pw_wh) { set_error("launch_conv_c16_f16s3: no hosted pointwise conv in this family"); return RTOD_E_ARG; }
    if (a.raw_out && (a.f16 || a.res || a.dec.enabled)) { set_error("launch_conv_c16_f16s3: a raw-sum launch carries no shortcut, decode or plain-f16 store"); return RTOD_E_ARG; }
    switch (mode) {
#define RTOD_X_CASE(id, bm, bn, nwm, nwn, minw) case id: return launch_c16<bm, bn, nwm, nwn, minw>(a, s);
        RTOD_C16_TILES(RTOD_X_CASE)
#undef RTOD_X_CASE
    }
    set_error("launch_conv_c16_f16s3: unknown mode %d", mode);
    return RTOD_E_ARG;
}

}  // namespace rtod
