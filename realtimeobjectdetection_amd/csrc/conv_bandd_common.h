// Pieces shared by the kernels that load their weight fragments straight from global memory (conv_bandd_f16s3.hip: 3x3 band;
// conv_pwd_f16s3.hip: 1x1): the wait behind a wave-uniform number of band pieces, and the epilogue in row passes.
#pragma once
#include "conv_f16s3_common.h"

namespace rtod {

#ifdef RTOD_TIMELINE
// diagnostic build: shader cycles of the epilogue's phases per workgroup (thread 0): [0] loads issued + first barrier, [1] transpose writes,
// [2] barrier, [3] tile reads + shortcut + split + stores, [4] trailing barrier
constexpr int BD_EPI_BLOCKS = 2048;
static __device__ unsigned long long g_bandd_epi[BD_EPI_BLOCKS * 5];
#define BD_ESTAMP(slot) { const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); et_[slot] += tn_ - eprev_; eprev_ = tn_; }
#else
#define BD_ESTAMP(slot)
#endif

// wait for all but the NBASE + PER n youngest operations, n (0 ... 5) wave-uniform: the band pieces issued after the awaited B set
// (PER: loads per band piece, 2 = hi + lo, 1 = hi only in plain-f16 instances)
template <int NBASE, int PER = 2> __device__ __forceinline__ void bandd_wait_vmcnt_plus(int n) {
    static_assert(((NBASE == 4 || NBASE == 8) && PER == 2) || ((NBASE == 2 || NBASE == 4) && PER == 1), "two B sets of 1, 2 or 4 loads");
    asm volatile("" : "+s"(n));                                 // opaque: left visible, the loop-invariant n unswitches the whole chunk loop six ways
    if (n == 0) vmcnt<NBASE>();
    else if (n == 1) vmcnt<NBASE + PER>();
    else if (n == 2) vmcnt<NBASE + 2 * PER>();
    else if (n == 3) vmcnt<NBASE + 3 * PER>();
    else if (n == 4) vmcnt<NBASE + 4 * PER>();
    else vmcnt<NBASE + 5 * PER>();
}

// ---- epilogue: scale / bias / activation, LDS transpose in passes of RG rows, split-format store (+ residual).
// The arithmetic is conv_f16s3_epilogue's: the same bits (epi_col_params and the text of conv_f16s3_epi_transpose.inc are the one copy
// both use; the finish-and-store statements are restated below).  Unlike that
// function a pass may cover a PART of a wave's rows (a wave owns all BM rows of its strip; the whole tile would need 64 KB).
// F16: plain-f16 output (hi plane of the shortcut operand read, hi plane stored).
// RAW: raw-sum instance (epi_raw, conv_f16s3_common.h): acc * inv_scale[n] as fp32 rows of ConvArgs::raw_out; no bias load, no
// shortcut operand (RES is false: its loads are not compiled), no split store.
template <int BM, int BN, int WM, int WN, int NT, int RG, bool RES, int KG, bool F16 = false, bool RAW = false>
__device__ __forceinline__ void bandd_epilogue(const ConvArgs& a, f32x4 (&acc)[WM / 16][WN / 16], unsigned char* smem, int bm, int bn, int tid,
                                               int wm, int wn, int lr, int lh, int M, int kg) {
    constexpr int TM = WM / 16, TN = WN / 16, MT = 16, TS = BN;
    static_assert(BM % RG == 0 && RG % 16 == 0, "epilogue pass");
    static_assert(!RAW || (!RES && !F16), "raw-sum instances: no shortcut, no plain-f16 store");
#ifdef RTOD_TIMELINE
    unsigned long long et_[5] = {0, 0, 0, 0, 0};
    unsigned long long eprev_ = __builtin_amdgcn_s_memtime();
#endif
    float* T = reinterpret_cast<float*>(smem);
    float amax = 0.f;
    const float escale = RAW ? 1.0f : SPLIT_SCALE;
    constexpr int GPR = BN / 8;
    constexpr int NG = (RG * GPR + NT - 1) / NT;
    // every global load of the epilogue up front, for ALL passes: bias / scale of the wave's column tiles, then the residual
    // operands (vmcnt retires in order: the transpose only has to wait for the first).  Loaded per pass, every pass paid the
    // memory latency again, between two barriers.
    constexpr int NP = BM / RG;
    float bias_j[TN], inv_j[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) epi_col_params<!RAW>(a, bn * BN + wn * WN + j * MT + lr, bias_j[j], inv_j[j]);
    f16x8 rq_h[RES ? NP : 1][RES ? NG : 1], rq_l[RES ? NP : 1][RES ? NG : 1];
    // Item (pass p, i) of a thread is row p RG + tid / GPR + i (NT / GPR), 8 channels at (tid % GPR) 8 when NT is a multiple of GPR
    // (every tile of this family): row and channel split ONCE, addresses advance by a constant — the per-item 64-bit multiplies of
    // `m * 2 * ldc` (quarter-rate v_mul_lo_u32) were ~5 % of the epilogue's vector time.
    static_assert(NT % GPR == 0, "epilogue items: constant row step");
    constexpr int RSTEP = NT / GPR;
    const int er = tid / GPR, ec8 = (tid - er * GPR) * 8;
    const bool ecol = bn * BN + ec8 < a.Cout;
    if constexpr (RES) {
        const _Float16* rh0 = reinterpret_cast<const _Float16*>(a.res) + a.res_coff + bn * BN;
        const int64_t rstep = (int64_t)RSTEP * 2 * a.res_ldc;
        const _Float16* const q0 = rh0 + (int64_t)(bm * BM + er) * 2 * a.res_ldc + ec8;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const _Float16* q = q0 + (int64_t)(p * RG) * 2 * a.res_ldc;
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const int m = bm * BM + p * RG + er + i * RSTEP;
                // rows past M / channels past Cout are never stored: their operand only has to come from a valid address
                const _Float16* qq = (er + i * RSTEP < RG && m < M && ecol) ? q : rh0;      // (a pass's last item may be partial: RG GPR items over NT threads)
                rq_h[p][i] = *reinterpret_cast<const f16x8*>(qq);
                if constexpr (!F16) rq_l[p][i] = *reinterpret_cast<const f16x8*>(qq + a.res_ldc);
                q += rstep;
            }
        }
    }
    __syncthreads();                                            // every wave has read its last fragments: the band becomes the transpose tile
    BD_ESTAMP(0)
#pragma unroll
    for (int rg = 0; rg < BM; rg += RG) {
        // a pass takes whole 16-row tiles, a part of the wave's: compile-time for one wave along M
#define EPI_WAVE_IN_PASS true
#define EPI_TILE_IN_PASS(i) (wm * WM + (i) * MT >= rg && wm * WM + (i) * MT < rg + RG)
#define EPI_TILE_ROW(i) (wm * WM + (i) * MT - rg)
#include "conv_f16s3_epi_transpose.inc"
#undef EPI_WAVE_IN_PASS
#undef EPI_TILE_IN_PASS
#undef EPI_TILE_ROW
        BD_ESTAMP(1)
        __syncthreads();
        BD_ESTAMP(2)
        _Float16* oq = reinterpret_cast<_Float16*>(a.out) + a.out_coff + bn * BN + (int64_t)(bm * BM + rg + er) * 2 * a.out_ldc + ec8;
        const int64_t ostep = (int64_t)RSTEP * 2 * a.out_ldc;
#pragma unroll
        for (int gi = 0; gi < NG; ++gi, oq += ostep) {
            const int r = er + gi * RSTEP;
            const int m = bm * BM + rg + r;
            if (r >= RG || m >= M || !ecol) continue;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(T + r * TS + ec8);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(T + r * TS + ec8 + 4);
            if constexpr (RAW) {                                         // 8 channels of row m of the dense [M][Npad] scratch
                float* rp = a.raw_out + (int64_t)m * a.Npad + bn * BN + ec8;
                *reinterpret_cast<f32x4*>(rp) = v0;
                *reinterpret_cast<f32x4*>(rp + 4) = v1;
                continue;
            }
            // shortcut add, split and store: the statements of epi_add_shortcut8 / epi_split8 / epi_store8 (conv_f16s3_common.h), NOT
            // shared with them: called here, two shortcut instances (128- and 96-row bandd tiles) changed their VGPR count
            float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            if constexpr (RES && F16) {
                const f16x8 qh = rq_h[rg / RG][gi];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += (float)qh[e];
            } else if constexpr (RES) {
                const f16x8 qh = rq_h[rg / RG][gi], ql = rq_l[rg / RG][gi];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += (float)qh[e] + (float)ql[e];
            }
            if constexpr (F16) {
                f16x8 ph;
#pragma unroll
                for (int e = 0; e < 8; ++e) ph[e] = f16_sat(v[e], amax);
                store_act16(oq, ph, false);
            } else {
                f16x8 ph, pl;
#pragma unroll
                for (int e = 0; e < 8; ++e) { _Float16 h, l; split_f16(v[e], h, l, amax); ph[e] = h; pl[e] = l; }
                store_act16(oq, ph, false);
                store_act16(oq + a.out_ldc, pl, false);
            }
        }
        BD_ESTAMP(3)
        if (rg + RG < BM) __syncthreads();
        BD_ESTAMP(4)
    }
#ifdef RTOD_TIMELINE
    if (threadIdx.x == 0 && blockIdx.x < BD_EPI_BLOCKS) for (int i = 0; i < 5; ++i) g_bandd_epi[blockIdx.x * 5 + i] = et_[i];
#endif
    if constexpr (!RAW) split_overflow_report(a.ovf, amax);
}

}  // namespace rtod
