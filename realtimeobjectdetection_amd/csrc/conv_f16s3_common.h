// Shared pieces of the split-precision f16 convolution kernels (conv_igemm_f16s3, conv_c16_f16s3, conv_ks_f16s3 through
// conv_f16s3_staged.h; conv_band_f16s3, conv_ring_f16s3, conv_patch_f16s3, conv_stem2_f16s3; conv_bandd_f16s3, conv_pwd_f16s3 through
// conv_bandd_common.h): the inline-asm memory primitives, the launchers' common argument checks, the epilogue arithmetic (epi_*),
// the register epilogue and the LDS-transposed epilogue.
#pragma once
#include "rtod_internal.h"
#include <type_traits>

namespace rtod {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int HBK = 32;                  // K elements per LDS stage (64 bytes per panel row)
constexpr unsigned OOB = 0x80000000u;    // voffset beyond any buffer (< 2 GiB enforced on the host)

// ---- Memory primitives of the main loops.  Their loads are issued through inline asm, so hipcc's s_waitcnt insertion does not
// see them: the loops keep loads in flight across barriers and retire them with hand-counted waits (cdna guide 5.7).  Why they
// are written exactly this way: DESIGN.md section 4, "Two GPU memory-access faults of round 2".

// Wait until at most N of this wave's vector-memory operations are outstanding (loads, stores and LDS-DMA count together and
// retire in issue order).
template <int N> __device__ __forceinline__ void vmcnt() {
    static_assert(0 <= N && N <= 63, "vmcnt range");
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

// 16-byte raw buffer load, OFF = instruction offset in bytes.  Its destination may be used only after the counted wait that
// retires it and a tie (below) that names it.
template <int OFF = 0> __device__ __forceinline__ u32x4 buffer_load_b128(const __amdgpu_buffer_rsrc_t rsrc, unsigned voffset, unsigned soffset) {
    u32x4 v;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(v) : "v"(voffset), "s"(rsrc), "s"(soffset), "n"(OFF) : "memory");
    return v;
}

// Register ties.  To the compiler an asm load writes its destination when the statement ends: once the last read is
// scheduled, the register is dead and may be reused (or register-only code hoisted above a wait: "memory" orders memory
// operations only) while the load is still in flight — a late load then overwrites a live value (fault 1).
// Rule: after the wait that retires a load, one empty statement names every register that load may still write as in/out.
// The registers then stay allocated until the data has landed, and no use is scheduled above the wait.
template <typename T> __device__ __forceinline__ void tie(T& a) { asm volatile("" : "+v"(a) :: "memory"); }
template <typename T> __device__ __forceinline__ void tie(T& a, T& b) { asm volatile("" : "+v"(a), "+v"(b) :: "memory"); }
template <typename T> __device__ __forceinline__ void tie(T& a, T& b, T& c) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c) :: "memory"); }
template <typename T> __device__ __forceinline__ void tie(T& a, T& b, T& c, T& d) {
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) :: "memory");
}
template <typename T> __device__ __forceinline__ void tie(T& a, T& b, T& c, T& d, T& e) {
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) :: "memory");
}
// every element of a register array, in one statement
template <typename T, int N> __device__ __forceinline__ void tie(T (&r)[N]) {
    static_assert(N >= 1 && N <= 5, "tie: 1 to 5 registers");
    if constexpr (N == 1) tie(r[0]);
    else if constexpr (N == 2) tie(r[0], r[1]);
    else if constexpr (N == 3) tie(r[0], r[1], r[2]);
    else if constexpr (N == 4) tie(r[0], r[1], r[2], r[3]);
    else tie(r[0], r[1], r[2], r[3], r[4]);
}
// a B set of the strip kernels (conv_bandd_common.h): [strip tile][hi, lo]; plain-f16 instances load the hi registers only
template <bool F16, int TN> __device__ __forceinline__ void tie_bset(u32x4 (&q)[TN][2]) {
    static_assert(TN >= 1 && TN <= 2, "strip width");
    if constexpr (F16 && TN == 1) tie(q[0][0]);
    else if constexpr (F16) tie(q[0][0], q[1][0]);
    else if constexpr (TN == 1) tie(q[0][0], q[0][1]);
    else tie(q[0][0], q[0][1], q[1][0], q[1][1]);
}

// LDS-DMA: `buffer_load_dwordx4 ... offen lds` writes lane l's 16 bytes at LDS byte address M0 + 16 l (a voffset past the
// descriptor's extent writes zeros).  The compiler neither tracks nor preserves M0 around asm, so M0 is saved, written in the
// statement that uses it, and restored; s_nop 0 separates the SALU write of M0 from the DMA that reads it.
// Two pieces with their own descriptors and LDS addresses (the hi and lo plane of the same rows).
__device__ __forceinline__ void lds_dma_pair(const __amdgpu_buffer_rsrc_t rsrc_hi, const __amdgpu_buffer_rsrc_t rsrc_lo, unsigned voffset,
                                             unsigned soff_hi, unsigned soff_lo, unsigned lds_hi, unsigned lds_lo) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %6\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %1, %2, %4 offen lds\n\t"
        "s_mov_b32 m0, %7\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %1, %3, %5 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voffset), "s"(rsrc_hi), "s"(rsrc_lo), "s"(soff_hi), "s"(soff_lo), "s"(lds_hi), "s"(lds_lo)
        : "memory");
}
// Two pieces from one descriptor, the lo piece LO_STEP bytes behind the hi piece in LDS.
template <int LO_STEP>
__device__ __forceinline__ void lds_dma_pair(const __amdgpu_buffer_rsrc_t rsrc, unsigned voffset, unsigned soff_hi, unsigned soff_lo, unsigned lds_hi) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %5\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %1, %2, %3 offen lds\n\t"
        "s_add_u32 m0, %5, %6\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %1, %2, %4 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voffset), "s"(rsrc), "s"(soff_hi), "s"(soff_lo), "s"(lds_hi), "n"(LO_STEP)
        : "memory", "scc");
}
// One piece (the hi plane alone: plain-f16 instances).
__device__ __forceinline__ void lds_dma(const __amdgpu_buffer_rsrc_t rsrc, unsigned voffset, unsigned soff, unsigned lds) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %4\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %1, %2, %3 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voffset), "s"(rsrc), "s"(soff), "s"(lds)
        : "memory", "scc");
}

// ---- Host: the argument checks every split launcher shares; `who` (the launcher's name) starts every error text.  The operands are
// present (a plain-f16 launch may omit the lo weight plane where `f16_ok`: the families with f16 instances), both buffers are
// non-empty and below OOB (so that a voffset of OOB is out of range), and the input view lies inside its buffer.
inline int check_split_conv_args(const ConvArgs& a, const char* who, bool f16_ok) {
    if (!a.in || !a.w_hi || (!a.w_lo && !(f16_ok && a.f16)) || !a.bias || !a.inv_scale || !a.out) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    if (a.in_bytes == 0 || a.in_bytes >= OOB || a.w_bytes == 0 || a.w_bytes >= OOB) {
        set_error("%s: buffer of %u / %u bytes outside (0, 2 GiB)", who, a.in_bytes, a.w_bytes); return RTOD_E_ARG;
    }
    if ((uint64_t)a.B * a.Hi * a.Wi * a.in_ldc * 4ull > (uint64_t)a.in_bytes) { set_error("%s: input view exceeds its buffer", who); return RTOD_E_ARG; }
    if (a.raw_out && (a.raw_ld % 4 || a.raw_ld < (a.Cout + 7) / 8 * 8)) { set_error("%s: raw-sum rows of %d floats for %d channels", who, a.raw_ld, a.Cout); return RTOD_E_ARG; }
    return RTOD_OK;
}

enum { EPI_SPLIT = 0, EPI_SPLIT_RES = 1, EPI_DECODE = 2, EPI_SPLIT_PW = 3, EPI_SPLIT_RES_PW = 4 };
// Plain-f16 instances (precision mode 2, "f16"): EPI | EPI_F16 as the kernels' EPI template argument.  The main loop drops the lo
// loads / LDS panels and two of the three MFMAs (one ah*bh product per fragment pair); the epilogue reads the hi plane of a
// shortcut operand only and stores the hi plane only (the lo halves of an f16 plan's arena are never written or read).
// Kept inside EPI so that the f16s3 instances keep their names (rocprofv3, bench.py).  EPI_F16 itself: rtod_internal.h.
__host__ __device__ constexpr bool epi_f16(int epi) { return (epi & EPI_F16) != 0; }
// Raw-sum instances (plan option bn_batch_split): EPI_SPLIT | EPI_RAW.  Same main loop; the epilogue stores acc * inv_scale[n] — the
// convolution sum itself: the pre-scales are powers of two — as fp32 rows [M][ConvArgs::raw_ld] to ConvArgs::raw_out, after the same LDS
// transpose: no SPLIT_SCALE, bias, activation or shortcut, no split store, no overflow sentinel.  The normalisation that follows
// (aux_kernels.hip: bn_apply_split_kernel) writes the split format.
__host__ __device__ constexpr bool epi_raw(int epi) { return (epi & EPI_RAW) != 0; }
__host__ __device__ constexpr int epi_kind(int epi) { return epi & ~(EPI_F16 | EPI_RAW); }
constexpr int PW_MAX_COUT = 64, PW_MAX_K = 64;    // measured: hosts with 128 output channels gain nothing over the stand-alone 1x1 kernel

__device__ __forceinline__ float h_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

__device__ __forceinline__ float h_decode(const DecodeArgs& d, float v, int n, int gx, int gy) {
    const int a = n / d.attrs;
    const int c = n - a * d.attrs;
    if (c >= 4) return h_sigmoid(v);
    if (c < 2) {
        float s = h_sigmoid(v);
        if (d.train) return s;
        return (s + (float)(c == 0 ? gx : gy)) * d.stride;
    }
    if (d.train) return v;
    const float anc = (c == 2) ? d.aw[a] : d.ah[a];
    return (expf(v) * anc) * d.stride;
}

// 16-byte activation store, sc1 (write-through): a layer's output is read by the NEXT kernel, on all XCDs, so it has
// to reach memory anyway; written back line by line while the kernel runs it leaves the kernel-end release little
// dirty L2 to drain (measured +1.2 % frames/s over plain write-back stores; non-temporal stores: -2.7 %).
// `plain` (diagnostic build, RTOD_DBG_ZERO bit 8) keeps the write-back store for that comparison.
__device__ __forceinline__ void store_act16(_Float16* p, const f16x8& v, bool plain) {
#ifdef RTOD_DIAG
    if (plain) { *reinterpret_cast<f16x8*>(p) = v; return; }
#endif
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(v) : "memory");
}

// SiLU on a value in the split format's domain (8 x): 8 * silu(x) = v / (1 + exp(-v / 8)); hardware exp2 / rcp (~1e-6 relative).
// The epilogues select it with a uniform branch AROUND their loops (a per-value select made the compiler evaluate both
// activations for every element: 2.5 % on the YOLOv3 forward, measured).
__device__ __forceinline__ float silu_scaled(float v, float inv_domain) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v * inv_domain)); }

// ---- The epilogue arithmetic.  Every tile of a layer gives the same bits; these pieces and conv_f16s3_epi_transpose.inc (the
// deposit / scale / activate text of the two LDS-transposed epilogues) are the copies the epilogues share.  The form follows the
// code objects (profiles/experiments/epilogue_share_resource_usage.txt): where a call changed an instance's registers, the call
// site keeps its own statements and says so (conv_f16s3_epilogue_regs, the store half of bandd_epilogue, the hosted 1x1's activation).

// (a) bias[n] / inv_scale[n] of output channel n: loads from a clamped index, selected afterwards (the conditional form
// `n < Cout ? bias[n] : 0` cost a branch and a full memory wait per value).  BIAS = false (raw-sum instances): no bias load.
template <bool BIAS = true> __device__ __forceinline__ void epi_col_params(const ConvArgs& a, int n, float& bias, float& inv) {
    const int nc = n < a.Cout ? n : 0;
    const float b = BIAS ? a.bias[nc] : 0.f, iv = a.inv_scale[nc];
    bias = n < a.Cout ? b : 0.f; inv = n < a.Cout ? iv : 0.f;
}

// (b) one value: s inv + bias in ONE rounding (inv and bias carry the format's scale, exact products by a power of two; spelled as
// an fma so that no call site is free to fuse the bias product into the add instead), then ACT: 0 linear, 1 leaky, 2 SiLU.
template <int ACT> __device__ __forceinline__ float epi_scale_act1(float s, float inv, float bias, float inv_domain) {
    const float v = __builtin_fmaf(s, inv, bias);
    if constexpr (ACT == 2) return silu_scaled(v, inv_domain);
    else if constexpr (ACT == 1) return __builtin_fmaxf(v, v * 0.1f);           // == v > 0 ? v : 0.1 v, bit for bit (signed zeros, infinities, NaN)
    else return v;
}
// f(integral_constant<int, ACT>) behind a uniform three-way branch on ConvArgs::leaky, AROUND the caller's loops (silu_scaled above)
template <typename F> __device__ __forceinline__ void epi_by_activation(int leaky, F f) {
    if (leaky == 2) f(std::integral_constant<int, 2>{});
    else if (leaky) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}

// (d) eight finished values -> the stored format.  The shortcut operand: hi + lo of a split tensor, hi alone of a plain-f16 one.
template <bool F16> __device__ __forceinline__ void epi_add_shortcut8(float (&v)[8], const f16x8& qh, const f16x8& ql) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if constexpr (F16) v[e] += (float)qh[e];
        else v[e] += (float)qh[e] + (float)ql[e];
    }
}
// split_f16 (F16: f16_sat, pl untouched) of eight values with the overflow sentinel
template <bool F16> __device__ __forceinline__ void epi_split8(const float (&v)[8], f16x8& ph, f16x8& pl, float& amax) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if constexpr (F16) ph[e] = f16_sat(v[e], amax);
        else { _Float16 h, l; split_f16(v[e], h, l, amax); ph[e] = h; pl[e] = l; }
    }
}
// the hi plane at q, the lo plane ldc halves behind it (F16: the hi plane alone)
template <bool F16> __device__ __forceinline__ void epi_store8(_Float16* q, int ldc, const f16x8& ph, const f16x8& pl, bool plain) {
    store_act16(q, ph, plain);
    if constexpr (!F16) store_act16(q + ldc, pl, plain);
}

// ---- transposed product (out^T = W * act^T): the MFMA's first operand is the weight fragment, the second the activation
// fragment, so a lane's accumulator holds 4 consecutive output CHANNELS (rows 4*lh + e) of ONE pixel (column lr).  With the
// weight rows of a 32-channel group interleaved over two 16-row tiles (tr_chan_of_row) the two tiles of a pair give the lane
// 8 consecutive channels: one 16-byte store per plane straight from the accumulators — no LDS transpose, no barrier.
// Panel row rho of an N tile (tile t = rho/16, row r = rho%16) <-> channel 32*(t/2) + 8*(r/4) + 4*(t%2) + r%4 of the tile.
__host__ __device__ __forceinline__ int tr_chan_of_row(int rho) {
    const int t = rho >> 4, r = rho & 15;
    return 32 * (t >> 1) + 8 * (r >> 2) + 4 * (t & 1) + (r & 3);
}

// Register epilogue of the transposed product.  acc[i][j]: pixel tile i (16 pixels), channel tile j of the wave.
// mrow[i] = linear output pixel (b*Ho + y)*Wo + x of this lane's column in pixel tile i, or -1 if it lies outside the tensor;
// cbase = first output channel of the wave's channel tiles.
// KG == 2 (in-workgroup split-K): group 1 parks its accumulators in LDS (`smem`, 16 bytes per lane and tile: the MFMA layout
// as it stands), one barrier, group 0 adds them to its own and stores.
template <int WM, int WN, bool RES, int KG = 1>
__device__ __forceinline__ void conv_f16s3_epilogue_regs(const ConvArgs& a, f32x4 (&acc)[WM / 16][WN / 16], unsigned char* smem,
                                                         const int (&mrow)[WM / 16], int cbase, int tidg, int lh, int kg = 0) {
    constexpr int TM = WM / 16, TN = WN / 16, NP = TN / 2;
    static_assert(TN % 2 == 0, "channel tiles come in pairs");
    if constexpr (KG == 2) {
        f32x4* T = reinterpret_cast<f32x4*>(smem);
        const int base = ((tidg >> 6) * TM * TN) * 64 + (tidg & 63);          // [wave of the group][i][j][lane]
        if (kg == 1) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) T[base + (i * TN + j) * 64] = acc[i][j];
        }
        __syncthreads();
        if (kg == 1) return;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const f32x4 o = T[base + (i * TN + j) * 64];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] += o[e];
            }
    }
    float amax = 0.f;
    _Float16* const oh = reinterpret_cast<_Float16*>(a.out) + a.out_coff;
    const _Float16* const rh = reinterpret_cast<const _Float16*>(a.res) + a.res_coff;
#pragma unroll
    for (int P = 0; P < NP; ++P) {
        const int c0 = cbase + 32 * P + 8 * lh;
        const bool cok = c0 < a.Cout;                                        // Cout % 8 == 0 for every split-format tensor
        const int cc = cok ? c0 : 0;
        // residual operands of this channel group first: their latency runs under the scale / bias loads and the conversions
        f16x8 rq_h[RES ? TM : 1], rq_l[RES ? TM : 1];
        if constexpr (RES) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = mrow[i];
                const bool ok = m >= 0 && cok;
                const _Float16* q = rh + (int64_t)(ok ? m : 0) * 2 * a.res_ldc + cc;
                rq_h[i] = ok ? *reinterpret_cast<const f16x8*>(q) : f16x8{0, 0, 0, 0, 0, 0, 0, 0};     // (unconditional loads + select, as in the
                rq_l[i] = ok ? *reinterpret_cast<const f16x8*>(q + a.res_ldc) : f16x8{0, 0, 0, 0, 0, 0, 0, 0};   //  LDS epilogue below: +6 % on the patch kernel, measured)
            }
        }
        f32x4 iv0 = *reinterpret_cast<const f32x4*>(a.inv_scale + cc), iv1 = *reinterpret_cast<const f32x4*>(a.inv_scale + cc + 4);
        f32x4 bs0 = *reinterpret_cast<const f32x4*>(a.bias + cc), bs1 = *reinterpret_cast<const f32x4*>(a.bias + cc + 4);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = mrow[i];
            // (not shared with epi_split8 / epi_store8: built on them, 30 ring / patch instances changed their VGPR count, up to +13)
            f16x8 ph, pl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float s = e < 4 ? acc[i][2 * P][e] : acc[i][2 * P + 1][e - 4];
                // (acc*inv + bias)*8 == acc*(8 inv) + 8 bias exactly (power of two)
                float v = s * ((e < 4 ? iv0[e] : iv1[e - 4]) * SPLIT_SCALE) + (e < 4 ? bs0[e] : bs1[e - 4]) * SPLIT_SCALE;
                if (a.leaky) v = v > 0.f ? v : v * 0.1f;              // linear / leaky only: SiLU layers run on the LDS-transposed epilogue (plan_tiles.cpp)
                if constexpr (RES) v += (float)rq_h[i][e] + (float)rq_l[i][e];
                _Float16 h, l;
                split_f16(v, h, l, amax);
                ph[e] = h; pl[e] = l;
            }
            if (m >= 0 && cok) {
                _Float16* q = oh + (int64_t)m * 2 * a.out_ldc + c0;
                store_act16(q, ph, false);
                store_act16(q + a.out_ldc, pl, false);
            }
        }
    }
    split_overflow_report(a.ovf, amax);
}

constexpr int epi_row_group(int bm, int wm, int rg_max) {
    int best = wm;
    for (int r = wm; r <= bm && r <= rg_max; r += wm) if (bm % r == 0) best = r;
    return best;
}


// ---- common epilogue: scale / bias / leaky, LDS transpose, then split-format store (+ residual) or head decode.
// `smem` is the kernel's whole LDS allocation (dead after the main loop, which must end on a barrier).
// Accumulators are v_mfma_f32_16x16x32_f16 tiles: lane holds column lr = lane%16, rows e + 4*lh, lh = lane/16.
// KG = 2 (in-workgroup split-K, conv_band_f16s3.hip): NT counts both wave groups, `tid` is the workgroup-wide thread
// index, wm / wn are positions inside the group `kg`; group 1 deposits its raw accumulators in the tile first and
// group 0 adds its own before scale / bias / activation.
// PRE: the caller hands over bias[n] / inv_scale[n] of its WN / 16 column groups in registers (conv_ring_f16s3.hip loads them at
// the start of a tile: a compiler-visible global load inside the epilogue would be waited for with vmcnt(0), which also
// drains the LDS-DMA ring that is prefetching the next tile).
// F16: plain-f16 output (precision mode 2): hi plane of the shortcut operand, hi plane stored (no hosted pointwise conv).
// RAW: raw-sum instance (epi_raw above): EPI_SPLIT only, never with F16.
template <int BM, int BN, int WM, int WN, int NT, int EPI, int SMEM_BYTES, int KG = 1, bool PRE = false, bool F16 = false, bool RAW = false>
__device__ __forceinline__ void conv_f16s3_epilogue(const ConvArgs& a, f32x4 (&acc)[WM / 16][WN / 16], unsigned char* smem,
                                                    int bm, int bn, int tid, int wm, int wn, int lr, int lh, int M, int kg = 0,
                                                    const float* pre_bias = nullptr, const float* pre_inv = nullptr) {
    constexpr int MT = 16, TM = WM / MT, TN = WN / MT;
    constexpr bool PW = EPI == EPI_SPLIT_PW || EPI == EPI_SPLIT_RES_PW;
    constexpr bool RES = EPI == EPI_SPLIT_RES || EPI == EPI_SPLIT_RES_PW;
    static_assert(!(F16 && PW), "plain-f16 plans host no pointwise conv");
    static_assert(!RAW || (EPI == EPI_SPLIT && !F16), "raw-sum instances: no shortcut, decode, hosted pointwise conv or plain-f16 store");
    // fused pointwise conv: the transpose tile doubles as the A operand of the second GEMM (row stride + 4 floats: the
    // 16 rows x 16 bytes of a fragment read then cover all 64 banks), and a second tile T2 takes its result
    constexpr int TS = PW ? BN + 4 : BN;
    constexpr int T2S = PW_MAX_COUT + 4;
    // ---- epilogue.  The accumulators (MFMA layout: channel on the lane, 16 pixel rows per register set)
    // are scaled / biased / activated and transposed through LDS (the stage buffers are dead: the main
    // loop ended on a barrier) as an fp32 [rows][BN] tile, so that the residual loads and the output
    // stores are row-contiguous 16-byte accesses (split format) or 256-byte row segments (decode).
    constexpr int RG_MAX = SMEM_BYTES / ((TS + (PW ? T2S : 0)) * 4);
    constexpr int RG = epi_row_group(BM, WM, RG_MAX);                     // rows per pass: multiple of WM dividing BM
    static_assert(RG >= WM && BM % RG == 0, "epilogue row group");
    static_assert(RG * (TS + (PW ? T2S : 0)) * 4 <= SMEM_BYTES, "epilogue tile exceeds the kernel's LDS");
    float* T = reinterpret_cast<float*>(smem);
    const int hw = a.Ho * a.Wo;
#ifdef RTOD_DIAG
    const bool st_plain = (a.dbg & 8) != 0;
#else
    constexpr bool st_plain = false;
#endif
    float amax = 0.f;                                                    // overflow sentinel of the split-format stores
    // fused pointwise conv: a wave owns one 16-column group of the second GEMM; its B fragments (the whole K of the
    // 1x1 conv, <= 4 k32 steps) are fetched once here, their latency hidden behind the transpose and the first store pass
    constexpr int PWK = PW_MAX_K / 32;
    f16x8 b2h[PW ? PWK : 1], b2l[PW ? PWK : 1];
    float bias2 = 0.f, inv2 = 0.f;
    int pw_n2t = 1, pw_j = 0;
    if constexpr (PW) {
        pw_n2t = a.pw_cout / 16;                                  // 1, 2 or 4: divides the wave count
        pw_j = (tid >> 6) % pw_n2t;
        const int n2 = pw_j * 16 + (tid & 15);
        const _Float16* w2h = a.pw_wh + (int64_t)n2 * 32 + ((tid & 63) >> 4) * 8;      // [chunk][pw_npad][32]
        const _Float16* w2l = a.pw_wl + (int64_t)n2 * 32 + ((tid & 63) >> 4) * 8;
#pragma unroll
        for (int ks = 0; ks < PWK; ++ks) {
            const bool ok = ks * 32 < a.pw_k;
            b2h[ks] = ok ? *reinterpret_cast<const f16x8*>(w2h + (int64_t)ks * a.pw_npad * 32) : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
            b2l[ks] = ok ? *reinterpret_cast<const f16x8*>(w2l + (int64_t)ks * a.pw_npad * 32) : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        bias2 = a.pw_bias[n2] * SPLIT_SCALE; inv2 = a.pw_inv_scale[n2] * SPLIT_SCALE;
    }
    const float escale = (EPI == EPI_DECODE || RAW) ? 1.0f : SPLIT_SCALE;   // (acc*inv + bias)*8 == acc*(8 inv) + 8 bias exactly
    constexpr int GPR_ = BN / 8;                                          // 8-channel (16-byte) groups per row
    constexpr int NG = (RG * GPR_ + NT - 1) / NT;                         // groups per thread and pass
    // bias / scale of the wave's TN column groups: all loads first and ahead of the residual loads (vmcnt retires in order: the
    // transpose must not wait for those), from a clamped index and selected afterwards — the conditional form
    // `n < Cout ? bias[n] : 0` cost a branch and a full memory wait per value, 2 TN of them in a row
    // (loaded at the top of every pass: held across the passes of a multi-pass epilogue they cost the generic tiles 10-60 registers)
#pragma unroll 1
    for (int rg = 0; rg < BM; rg += RG) {
        float bias_j[TN], inv_j[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if constexpr (PRE) { bias_j[j] = pre_bias[j]; inv_j[j] = pre_inv[j]; }
            else epi_col_params(a, bn * BN + wn * WN + j * MT + lr, bias_j[j], inv_j[j]);
        }
        // residual operands of this pass: issued ahead of the transpose so that their latency (HBM / L2, ~2 us when
        // waited for inside the store loop: in-kernel stamps showed the epilogue at 15 % of a 76x76 tile) overlaps the
        // accumulator -> LDS phase and the barrier
        f16x8 rq_h[RES ? NG : 1], rq_l[RES ? NG : 1];
        if constexpr (RES) {
            const _Float16* rh0 = reinterpret_cast<const _Float16*>(a.res) + a.res_coff + bn * BN;
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const int g = tid + i * NT;
                const int r = g / GPR_, c8 = (g - r * GPR_) * 8;
                const int m = bm * BM + rg + r;
                const bool ok = g < RG * GPR_ && m < M && bn * BN + c8 < a.Cout;
                // unconditional loads from a clamped address, selected afterwards: written as `ok ? *q : 0` each load became a
                // branch with its own s_waitcnt vmcnt(0) — NG pairs of memory latencies in a row at the head of every epilogue
                const _Float16* q = rh0 + (int64_t)(ok ? m : 0) * 2 * a.res_ldc + (ok ? c8 : 0);
                const f16x8 th = *reinterpret_cast<const f16x8*>(q);
                rq_h[i] = ok ? th : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
                if constexpr (!F16) {
                    const f16x8 tl = *reinterpret_cast<const f16x8*>(q + a.res_ldc);
                    rq_l[i] = ok ? tl : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
                }
            }
        }
        // a wave's WM rows lie in one pass (RG is a multiple of WM); single pass: no branch
#define EPI_WAVE_IN_PASS (RG == BM || (wm * WM >= rg && wm * WM < rg + RG))
#define EPI_TILE_IN_PASS(i) true
#define EPI_TILE_ROW(i) (wm * WM - rg + (i) * MT)
#include "conv_f16s3_epi_transpose.inc"
#undef EPI_WAVE_IN_PASS
#undef EPI_TILE_IN_PASS
#undef EPI_TILE_ROW
        __syncthreads();
        if constexpr (EPI == EPI_DECODE) {
            // thread <-> fixed channel n: anchor / attribute kind are per-thread constants; rows advance by NT/BN
            constexpr int RSTEP = NT / BN > 0 ? NT / BN : 1;
            static_assert(NT % BN == 0 || BN % NT == 0, "decode mapping");
            for (int nl = tid % BN; nl < BN; nl += NT) {
                const int n = bn * BN + nl;
                if (n >= a.Cout) continue;
                const int an = n / a.dec.attrs, c = n - an * a.dec.attrs;
                const bool is_wh = (c == 2 || c == 3) && !a.dec.train;
                const bool is_raw = (c == 2 || c == 3) && a.dec.train;
                const float anc = (c == 2 ? a.dec.aw[an] : a.dec.ah[an]);
                const int r0 = (NT >= BN) ? tid / BN : 0;
                int m = bm * BM + rg + r0;
                const int b = m / hw;
                int cell = m - b * hw;
                int gy = cell / a.dec.GW, gx = cell - gy * a.dec.GW;
                // The loop is VALU-bound (1 600 instructions per thread per 128-row tile with libm expf, an IEEE divide and
                // 64-bit index arithmetic per element: the decode epilogue was 58 % of the 76x76 head kernel): hardware
                // exp2 / rcp (1 ulp; the result has to meet 1e-4) and a running output pointer.
                float* op = a.out + (int64_t)b * a.dec.img_stride + a.dec.head_off + (int64_t)cell * a.Cout + n;
                const int64_t row_step = (int64_t)RSTEP * a.Cout;
                const int64_t img_fix = a.dec.img_stride - (int64_t)hw * a.Cout;      // first cell of the next image
                if (a.dec.v5) {                                          // YOLOv5-style head (cfg extension); uniform
                    for (int r = r0; r < RG && m < M; r += RSTEP, m += RSTEP) {
                        const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-T[r * TS + nl]));
                        float o = sg;
                        if (c < 2) o = ((sg * 2.0f - 0.5f) + (float)(c == 0 ? gx : gy)) * a.dec.stride;
                        else if (c < 4) { const float t2 = sg * 2.0f; o = (t2 * t2) * anc; }
                        *op = o;
                        op += row_step; cell += RSTEP; gx += RSTEP;
                        while (gx >= a.dec.GW) { gx -= a.dec.GW; ++gy; }
                        while (cell >= hw) { cell -= hw; gy -= a.dec.GH; op += img_fix; }
                    }
                } else
                for (int r = r0; r < RG && m < M; r += RSTEP, m += RSTEP) {
                    const float v = T[r * TS + nl];
                    float o;
                    if (is_raw) o = v;
                    else {
                        const float ex = __expf(is_wh ? v : -v);          // one exp serves both kinds
                        if (is_wh) o = (ex * anc) * a.dec.stride;
                        else {
                            o = __builtin_amdgcn_rcpf(1.0f + ex);
                            if (c < 2 && !a.dec.train) o = (o + (float)(c == 0 ? gx : gy)) * a.dec.stride;
                        }
                    }
                    *op = o;
                    op += row_step; cell += RSTEP; gx += RSTEP;
                    while (gx >= a.dec.GW) { gx -= a.dec.GW; ++gy; }
                    while (cell >= hw) { cell -= hw; gy -= a.dec.GH; op += img_fix; }   // GH*GW < RSTEP: a step may cross several images
                }
            }
        } else {
            constexpr int GPR = GPR_;
            _Float16* oh = reinterpret_cast<_Float16*>(a.out) + a.out_coff + bn * BN;
#pragma unroll
            for (int gi = 0; gi < NG; ++gi) {
                const int g = tid + gi * NT;
                if (g >= RG * GPR) continue;
                const int r = g / GPR, c8 = (g - r * GPR) * 8;
                const int m = bm * BM + rg + r;
                if (m >= M || bn * BN + c8 >= a.Cout) continue;
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(T + r * TS + c8);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(T + r * TS + c8 + 4);
                if constexpr (RAW) {                                      // 8 channels of row m of the [M][raw_ld] scratch (Cout rounded up to 8 <= raw_ld)
                    float* rp = a.raw_out + (int64_t)m * a.raw_ld + bn * BN + c8;
                    *reinterpret_cast<f32x4*>(rp) = v0;
                    *reinterpret_cast<f32x4*>(rp + 4) = v1;
                    continue;
                }
                float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                if constexpr (RES) {
                    epi_add_shortcut8<F16>(v, rq_h[gi], rq_l[gi]);
                    if constexpr (PW) {                                   // the second GEMM reads the sum
                        *reinterpret_cast<f32x4*>(T + r * TS + c8) = f32x4{v[0], v[1], v[2], v[3]};
                        *reinterpret_cast<f32x4*>(T + r * TS + c8 + 4) = f32x4{v[4], v[5], v[6], v[7]};
                    }
                }
                f16x8 ph, pl;
                epi_split8<F16>(v, ph, pl, amax);
                epi_store8<F16>(oh + (int64_t)m * 2 * a.out_ldc + c8, a.out_ldc, ph, pl, st_plain);
            }
            if constexpr (PW) {
                // ---- fused 1x1 conv: out2[RG x pw_cout] = act[RG x pw_k] * W2^T, same three-product split arithmetic.
                // T holds this conv's activations x SPLIT_SCALE (the stored format), so hi / lo come from it directly.
                // Work item = one 16x16 output tile; A from T (ds_read_b128 pairs), B straight from the 1x1 conv's packed
                // planes (a few KiB, L1/L2 resident).
                __syncthreads();
                float* T2 = T + RG * TS;
                const int lane = tid & 63, wave = tid >> 6;
                const int lr16 = lane & 15, lh16 = lane >> 4;
                const int k2s = a.pw_k / 32;
                const int n2 = pw_j * 16 + lr16;
                for (int sl = wave / pw_n2t; sl < RG / 16; sl += (NT / 64) / pw_n2t) {
                    f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
                    const float* trow = T + (sl * 16 + lr16) * TS + lh16 * 8;
#pragma unroll
                    for (int ks = 0; ks < PWK; ++ks) {
                        if (ks < k2s) {                                   // uniform
                            const f32x4 x0 = *reinterpret_cast<const f32x4*>(trow + ks * 32);
                            const f32x4 x1 = *reinterpret_cast<const f32x4*>(trow + ks * 32 + 4);
                            f16x8 ah, al;
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const float x = e < 4 ? x0[e] : x1[e - 4];
                                const _Float16 h = (_Float16)x;
                                ah[e] = h; al[e] = (_Float16)(x - (float)h);
                            }
                            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, b2h[ks], acc2, 0, 0, 0);
                            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, b2l[ks], acc2, 0, 0, 0);
                            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, b2h[ks], acc2, 0, 0, 0);
                        }
                    }
                    if (a.pw_leaky == 2) {                                   // uniform
#pragma unroll
                        for (int e = 0; e < 4; ++e) T2[(sl * 16 + 4 * lh16 + e) * T2S + n2] = silu_scaled(acc2[e] * inv2 + bias2, 1.0f / SPLIT_SCALE);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float v = acc2[e] * inv2 + bias2;
                            if (a.pw_leaky) v = v > 0.f ? v : v * 0.1f;
                            T2[(sl * 16 + 4 * lh16 + e) * T2S + n2] = v;
                        }
                    }
                }
                __syncthreads();
                const int gpr2 = a.pw_cout / 8;
                _Float16* oh2 = reinterpret_cast<_Float16*>(a.pw_out) + a.pw_out_coff;
                for (int g = tid; g < RG * gpr2; g += NT) {
                    const int r = g / gpr2, c8 = (g - r * gpr2) * 8;
                    const int m = bm * BM + rg + r;
                    if (m >= M) continue;
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(T2 + r * T2S + c8);
                    const f32x4 v1 = *reinterpret_cast<const f32x4*>(T2 + r * T2S + c8 + 4);
                    const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    f16x8 ph, pl;
                    epi_split8<false>(v, ph, pl, amax);
                    epi_store8<false>(oh2 + (int64_t)m * 2 * a.pw_out_ldc + c8, a.pw_out_ldc, ph, pl, st_plain);
                }
            }
        }
        if (rg + RG < BM) __syncthreads();
    }
    if constexpr (EPI != EPI_DECODE && !RAW) split_overflow_report(a.ovf, amax);
}

}  // namespace rtod
