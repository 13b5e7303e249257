// K-sliced implicit-GEMM convolution on split-precision f16 MFMA, gfx950 (plan option "k_slices_split"): the generic tile of
// conv_igemm_f16s3.hip with the K sum formed slice by slice, for single-frame latency.
//
// At one or two frames the deep layers (13x13 ... 52x52 grids, K = 256 ... 9216) have a few dozen output tiles for 256 CUs and
// each tile walks the whole K sum.  Here the K-chunks of 32 are cut into slices of `a.slice_chunks` chunks (a property of the
// layer: plan_build.cpp, split_slice_chunks; the last slice may be shorter).  Every slice starts from zero accumulators and runs the
// very same pipelined loop, and the slice sums are added in ascending slice order in fp32, starting from zero.  That order is
// fixed by the layer alone, so two schedules give the same bits:
//   schedule A (SCHED_B = false): the grid is the tiles; a workgroup walks slice after slice, total = total + slice at every
//                                 slice end, then the common epilogue (plain or fused shortcut) runs on the total;
//   schedule B (SCHED_B = true):  the grid is tiles x slices; a workgroup writes the raw fp32 accumulators of its slice to
//                                 a.partial [slice][M][Npad]; conv_ks_reduce_kernel then adds the panels in ascending order and
//                                 applies the arithmetic of conv_f16s3_epilogue (the epi_* pieces of conv_f16s3_common.h).
// A sliced layer always runs this family, at every batch size (a frame's result must not depend on the batch it rides in);
// autotune picks tile and schedule.  The LDS staging, swizzle, MFMA sequence and schedule are the one copy of conv_f16s3_staged.h; same buffer-load addressing and F16 flag as the
// generic tile; K order k = ((c/32)*kh*kw + tap)*32 + c%32, so the weights are the generic packing.
// No fused head decode and no hosted pointwise conv in this family (the planner never slices such layers).
#include "conv_f16s3_staged.h"
#include <cstdio>

namespace rtod {

// BM x BN workgroup tile, NWM x NWN waves; MINW = waves per SIMD the register budget must admit.  Schedule A keeps two
// accumulator sets (slice + total): 64x64 keeps the generic tile's 4 waves per SIMD (112 VGPRs) and 64x128 its 3 (162 VGPRs); the
// 128x64 tile states 2 for it (178 VGPRs; the generic tile of that shape states 3).  No instance spills.
template <int BM, int BN, int NWM, int NWN, int MINW, int EPI, bool SCHED_B>
__global__ __launch_bounds__(NWM * NWN * 64, MINW)
void conv_ks_f16s3_kernel(const ConvArgs a, const int grid_m, const int grid_n) {
    constexpr bool F16 = epi_f16(EPI);
    using Tile = StagedTile<BM, BN, NWM, NWN, F16>;
    constexpr int WM = Tile::WM, WN = Tile::WN, NT = Tile::NT, TM = Tile::TM, TN = Tile::TN, RPP = Tile::RPP;
    constexpr int A_SLOTS = Tile::A_SLOTS, B_SLOTS = Tile::B_SLOTS, SMEM = Tile::SMEM;

    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];

    const int nwg = grid_m * grid_n;
    int bid = blockIdx.x;
    int slice = 0;
    if constexpr (SCHED_B) { slice = bid / nwg; bid -= slice * nwg; }
    bid = xcd_remap(bid, nwg);
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

    // wave-uniform K-chunk cursor: tap (ky,kx) and first channel c0 of the chunk to be LOADED next; ld_end = end of the slice
    int ld_kc = 0, ld_c0 = 0, ld_ky = 0, ld_kx = 0, ld_end = 0;
    const int nk = a.Kpad / HBK;

    auto gload = [&](typename Tile::Regs& S) {
        // chunks past the end of the slice (issued unconditionally: the loop stays branch-free and the vmcnt bookkeeping exact)
        // read out of range -> zeros
        const bool live = ld_kc < ld_end;
        const unsigned tap_off = (unsigned)(ld_ky * a.Wi + ld_kx) * PS + (unsigned)ld_c0 * 2u;
#pragma unroll
        for (int i = 0; i < A_SLOTS; ++i) {
            const bool ok = live && (unsigned)(iy0[i] + ld_ky) < (unsigned)a.Hi && (unsigned)(ix0[i] + ld_kx) < (unsigned)a.Wi;
            const unsigned vo = ok ? pbase[i] + tap_off : OOB;
            S.ah[i] = buffer_load_b128(rs_a, vo, 0u);
            if constexpr (!F16) S.al[i] = buffer_load_b128(rs_a, vo, lo_plane);
        }
        const unsigned koff = live ? (unsigned)ld_kc * wchunk : 0u;
#pragma unroll
        for (int i = 0; i < B_SLOTS; ++i) {
            const unsigned wo = live ? wbase[i] : OOB;
            S.bh[i] = buffer_load_b128(rs_wh, wo, koff);
            if constexpr (!F16) S.bl[i] = buffer_load_b128(rs_wl, wo, koff);
        }
        ++ld_kc;
        if (++ld_kx == a.kw) { ld_kx = 0; if (++ld_ky == a.kh) { ld_ky = 0; ld_c0 += HBK; } }
    };

    f32x4 acc[TM][TN];                                           // the current slice
    f32x4 total[SCHED_B ? 1 : TM][SCHED_B ? 1 : TN];             // schedule A: sum of the finished slices
    (void)total;
    if constexpr (!SCHED_B) Tile::zero(total);

    constexpr bool A_AHEAD = true;                               // the generic tile's read order
#include "conv_f16s3_staged_defs.inc"

    // One slice [kc0, kc1): zero accumulators, the cursor seeded at kc0, then the shared pipeline (chunks >= kc1 are zero chunks, so
    // an odd slice length costs one zero chunk of MFMAs, which leaves every accumulator bit as it is in both schedules alike).  It
    // ends on a barrier with no load in flight, so the next slice may restage LDS at once.
    auto run_slice = [&](int kc0, int kc1) {
        Tile::zero(acc);
        const int taps = a.kh * a.kw;
        const int cchunk = kc0 / taps, tap = kc0 - cchunk * taps;
        ld_kc = kc0; ld_end = kc1; ld_c0 = cchunk * HBK; ld_ky = tap / a.kw; ld_kx = tap - ld_ky * a.kw;
#include "conv_f16s3_staged_run.inc"
    };

    if constexpr (SCHED_B) {
        const int kc0 = slice * a.slice_chunks;
        const int kc1 = kc0 + a.slice_chunks < nk ? kc0 + a.slice_chunks : nk;
        run_slice(kc0, kc1);
        // raw slice sums -> a.partial [slice][M][Npad]: lane = column lr of the 16x16 tile, rows e + 4 lh; the 16 lanes of a row
        // write 64 consecutive bytes
        float* part = a.partial + (int64_t)slice * M * a.Npad;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = bm * BM + wm * WM + i * 16 + 4 * lh + e;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = bn * BN + wn * WN + j * 16 + lr;
                    if (m < M && n < a.Npad) part[(int64_t)m * a.Npad + n] = acc[i][j][e];
                }
            }
    } else {
#pragma unroll 1
        for (int kc0 = 0; kc0 < nk; kc0 += a.slice_chunks) {
            run_slice(kc0, kc0 + a.slice_chunks < nk ? kc0 + a.slice_chunks : nk);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) total[i][j][e] = total[i][j][e] + acc[i][j][e];
        }
        conv_f16s3_epilogue<BM, BN, WM, WN, NT, epi_kind(EPI), SMEM, 1, false, F16>(a, total, smem, bm, bn, tid, wm, wn, lr, lh, M);
    }
}

// Schedule B's second half: one thread per (pixel, group of 8 channels), channels fastest.  Adds the slice panels in ascending
// order from zero (as schedule A's `total`), then the arithmetic of conv_f16s3_epilogue in its order: (8 inv_scale) s + 8 bias,
// activation, fused shortcut (hi + lo of the split residual, hi alone of a plain-f16 one), split_f16 / f16_sat with the overflow
// sentinel, 16-byte stores into the output view (out_ldc / out_coff: a concat slice).
template <bool RES, bool F16>
__global__ __launch_bounds__(256)
void conv_ks_reduce_kernel(const ConvArgs a, const int n_slices, const int M) {
    const int gpr = a.Cout / 8;                                  // Cout % 8 == 0 (checked by the launcher)
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float amax = 0.f;
    if (g < (int64_t)M * gpr) {
        const int m = (int)(g / gpr), c8 = (int)(g - (int64_t)m * gpr) * 8;
        const float* p = a.partial + (int64_t)m * a.Npad + c8;
        const int64_t panel = (int64_t)M * a.Npad;
        f16x8 qh = {0, 0, 0, 0, 0, 0, 0, 0}, ql = {0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (RES) {
            const _Float16* q = reinterpret_cast<const _Float16*>(a.res) + a.res_coff + (int64_t)m * 2 * a.res_ldc + c8;
            qh = *reinterpret_cast<const f16x8*>(q);
            if constexpr (!F16) ql = *reinterpret_cast<const f16x8*>(q + a.res_ldc);
        }
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < n_slices; ++k) {
            const f32x4 p0 = *reinterpret_cast<const f32x4*>(p + k * panel), p1 = *reinterpret_cast<const f32x4*>(p + k * panel + 4);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] = s[e] + (e < 4 ? p0[e] : p1[e - 4]);
        }
        const f32x4 iv0 = *reinterpret_cast<const f32x4*>(a.inv_scale + c8), iv1 = *reinterpret_cast<const f32x4*>(a.inv_scale + c8 + 4);
        const f32x4 bs0 = *reinterpret_cast<const f32x4*>(a.bias + c8), bs1 = *reinterpret_cast<const f32x4*>(a.bias + c8 + 4);
        float v[8];
        epi_by_activation(a.leaky, [&](auto act) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                v[e] = epi_scale_act1<decltype(act)::value>(s[e], (e < 4 ? iv0[e] : iv1[e - 4]) * SPLIT_SCALE, (e < 4 ? bs0[e] : bs1[e - 4]) * SPLIT_SCALE, 1.0f / SPLIT_SCALE);
        });
        if constexpr (RES) epi_add_shortcut8<F16>(v, qh, ql);
        f16x8 ph, pl;
        epi_split8<F16>(v, ph, pl, amax);
        epi_store8<F16>(reinterpret_cast<_Float16*>(a.out) + a.out_coff + (int64_t)m * 2 * a.out_ldc + c8, a.out_ldc, ph, pl, false);
    }
    split_overflow_report(a.ovf, amax);
}

// One list drives the tile table, the launch switch and the kernel names rocprofv3 prints:
//   X(tile, BM, BN, waves along M, waves along N, MINW)          family mode = 2 * tile + schedule (0: A, 1: B)
#define RTOD_KS_TILES(X) \
    X(0, 64, 64, 2, 2, 4) X(1, 64, 128, 2, 2, 3) X(2, 128, 64, 2, 2, 2)

#define RTOD_X_INFO(id, bm, bn, nwm, nwn, minw) \
    {bm, bn, "conv_ks_f16s3<" #bm "x" #bn "," #nwm "x" #nwn ",k-slices>"}, {bm, bn, "conv_ks_f16s3<" #bm "x" #bn "," #nwm "x" #nwn ",wg per k-slice>"},
static const ConvVariantInfo kKsModes[] = { RTOD_KS_TILES(RTOD_X_INFO) };
#undef RTOD_X_INFO
static_assert(sizeof(kKsModes) / sizeof(kKsModes[0]) == KS_MODES, "KS_MODES (rtod_internal.h) counts this table");

const ConvVariantInfo& conv_ks_mode_info(int mode) { return kKsModes[mode < 0 || mode >= KS_MODES ? 0 : mode]; }

int conv_ks_slices(const ConvArgs& a) { return a.slice_chunks > 0 ? (a.Kpad / HBK + a.slice_chunks - 1) / a.slice_chunks : 1; }

// demangled name of the instantiation (what rocprofv3 --kernel-trace reports); schedule B: its first kernel, which has no epilogue
// of its own (EPI carries the plain-f16 flag alone) and is followed by conv_ks_reduce_kernel
int conv_ks_kernel_name(int mode, int epi, char* buf, size_t len) {
    const int sched = mode & 1;
    if (sched) epi &= EPI_F16;
#define RTOD_X_NAME(id, bm, bn, nwm, nwn, minw) \
    if (mode >> 1 == id) return snprintf(buf, len, "void rtod::conv_ks_f16s3_kernel<" #bm ", " #bn ", " #nwm ", " #nwn ", " #minw ", %d, %s>(rtod::ConvArgs, int, int)", epi, sched ? "true" : "false");
    RTOD_KS_TILES(RTOD_X_NAME)
#undef RTOD_X_NAME
    return -1;
}

template <int BM, int BN, int NWM, int NWN, int MINW>
static int launch_ks(const ConvArgs& a, int sched, hipStream_t s) {
    const int M = a.B * a.Ho * a.Wo;
    const int gm = (M + BM - 1) / BM, gn = (a.Cout + BN - 1) / BN;
    constexpr int NT = NWM * NWN * 64;
    if (!sched) {
        auto k_res = conv_ks_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT_RES, false>;
        auto k_plain = conv_ks_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT, false>;
        auto f_res = conv_ks_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT_RES | EPI_F16, false>;
        auto f_plain = conv_ks_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT | EPI_F16, false>;
        hipLaunchKernelGGL(a.f16 ? (a.res ? f_res : f_plain) : (a.res ? k_res : k_plain), dim3(gm * gn), dim3(NT), 0, s, a, gm, gn);
        return hip_fail(hipGetLastError(), "conv_ks_f16s3 launch");
    }
    const int S = conv_ks_slices(a);
    auto k_b = conv_ks_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT, true>;
    auto f_b = conv_ks_f16s3_kernel<BM, BN, NWM, NWN, MINW, EPI_SPLIT | EPI_F16, true>;
    hipLaunchKernelGGL(a.f16 ? f_b : k_b, dim3(gm * gn * S), dim3(NT), 0, s, a, gm, gn);
    if (int rc = hip_fail(hipGetLastError(), "conv_ks_f16s3 slice launch")) return rc;
    const int64_t n = (int64_t)M * (a.Cout / 8);
    auto r = a.f16 ? (a.res ? conv_ks_reduce_kernel<true, true> : conv_ks_reduce_kernel<false, true>)
                   : (a.res ? conv_ks_reduce_kernel<true, false> : conv_ks_reduce_kernel<false, false>);
    hipLaunchKernelGGL(r, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, S, M);
    return hip_fail(hipGetLastError(), "conv_ks_f16s3 reduce launch");
}

int launch_conv_ks_f16s3(const ConvArgs& a, int mode, hipStream_t s) {
    if (int rc = check_split_conv_args(a, "launch_conv_ks_f16s3", true)) return rc;
    if (a.Cin % HBK || a.in_ldc % 8 || a.in_coff % 8 || a.in_coff < 0 || a.in_coff + a.Cin > a.in_ldc || a.Kpad % HBK || a.K != a.Kpad ||
        a.kh < 1 || a.kw < 1 || a.K != a.kh * a.kw * a.Cin) {
        set_error("launch_conv_ks_f16s3: needs Cin %% 32 == 0 and 8-channel aligned views (Cin=%d ldc=%ld coff=%d K=%d Kpad=%d)", a.Cin, (long)a.in_ldc, a.in_coff, a.K, a.Kpad);
        return RTOD_E_ARG;
    }
    if (a.B <= 0 || a.Ho <= 0 || a.Wo <= 0 || a.Cout <= 0 || a.stride < 1 || a.pad < 0) { set_error("launch_conv_ks_f16s3: empty shape or bad geometry"); return RTOD_E_ARG; }
    if ((int64_t)a.B * a.Ho * a.Wo >= (1ll << 31) / 256) { set_error("launch_conv_ks_f16s3: too many output pixels"); return RTOD_E_ARG; }
    if (a.dec.enabled || a.pw_wh) { set_error("launch_conv_ks_f16s3: no fused head decode and no hosted pointwise conv in this family"); return RTOD_E_ARG; }
    if (a.Cout % 8 || a.out_ldc % 8 || a.out_coff % 8 || a.out_coff < 0 || a.out_coff + a.Cout > a.out_ldc) { set_error("launch_conv_ks_f16s3: bad output view"); return RTOD_E_ARG; }
    if (a.res && (a.res_ldc % 8 || a.res_coff % 8 || a.res_coff < 0 || a.res_coff + a.Cout > a.res_ldc)) { set_error("launch_conv_ks_f16s3: bad residual view"); return RTOD_E_ARG; }
    if (a.slice_chunks <= 0 || a.Npad < a.Cout || a.Npad % 32 || (uint64_t)a.Npad * a.Kpad * 2ull > (uint64_t)a.w_bytes) {
        set_error("launch_conv_ks_f16s3: bad K-slice arguments (slice_chunks=%d Npad=%d Cout=%d)", a.slice_chunks, a.Npad, a.Cout); return RTOD_E_ARG;
    }
    if (mode < 0 || mode >= KS_MODES) { set_error("launch_conv_ks_f16s3: unknown mode %d", mode); return RTOD_E_ARG; }
    const int sched = mode & 1;
    if (sched && (!a.partial || (int64_t)conv_ks_slices(a) * a.B * a.Ho * a.Wo * a.Npad > a.partial_floats)) {
        set_error("launch_conv_ks_f16s3: slice scratch missing or too small"); return RTOD_E_ARG;
    }
    switch (mode >> 1) {
#define RTOD_X_CASE(id, bm, bn, nwm, nwn, minw) case id: return launch_ks<bm, bn, nwm, nwn, minw>(a, sched, s);
        RTOD_KS_TILES(RTOD_X_CASE)
#undef RTOD_X_CASE
    }
    set_error("launch_conv_ks_f16s3: unknown mode %d", mode);
    return RTOD_E_ARG;
}

}  // namespace rtod
