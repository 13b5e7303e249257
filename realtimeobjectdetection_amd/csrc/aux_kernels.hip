// Bandwidth-bound helper kernels of the Darknet forward (gfx950): input NCHW->NHWC pack, bilinear and nearest x2 upsample, stand-alone
// shortcut add, channel copy, max-pool, batch-statistics BatchNorm, NHWC->NCHW read-back, stand-alone head decode, confidence mask.
// All are HBM-bound elementwise work: 16 bytes per lane along the channel axis wherever the layout allows, grid capped at
// ~2048 blocks + grid stride.  Each op has ONE kernel body over the activation format (Act<F> below).
#include "conv_f16s3_common.h"
#include "bn_constants.h"
#include <algorithm>

namespace rtod {

static inline int grid_for(int64_t work, int block) {
    int64_t g = (work + block - 1) / block;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

// ---------------------------------------------------------------------------------------------
// input pack: x [B,C,H,W] (NCHW, C=3) -> [B,H,W,Cp] with channels C..Cp-1 zero.  The stem conv then
// runs through the generic implicit-GEMM with Cin = Cp = 4 (16-B pixel = one float4 gather).
__global__ void pack_input_kernel(const float* __restrict__ x, int B, int C, int H, int W,
                                  float* __restrict__ out, int Cp) {
    const int64_t npix = (int64_t)B * H * W;
    const int64_t hw = (int64_t)H * W;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = p / hw, r = p - b * hw;
        const float* src = x + b * C * hw + r;
        for (int c0 = 0; c0 < Cp; c0 += 4) {
            f32x4 v;
            v[0] = c0 + 0 < C ? src[(c0 + 0) * hw] : 0.f;
            v[1] = c0 + 1 < C ? src[(c0 + 1) * hw] : 0.f;
            v[2] = c0 + 2 < C ? src[(c0 + 2) * hw] : 0.f;
            v[3] = c0 + 3 < C ? src[(c0 + 3) * hw] : 0.f;
            *reinterpret_cast<f32x4*>(out + p * Cp + c0) = v;
        }
    }
}

int launch_pack_input(const float* x, int B, int C, int H, int W, float* out, int Cp, hipStream_t s) {
    if (!x || !out || Cp % 4 || Cp < C) { set_error("pack_input: bad args"); return RTOD_E_ARG; }
    const int64_t npix = (int64_t)B * H * W;
    hipLaunchKernelGGL(pack_input_kernel, dim3(grid_for(npix, 256)), dim3(256), 0, s, x, B, C, H, W, out, Cp);
    return hip_fail(hipGetLastError(), "pack_input launch");
}

// ---------------------------------------------------------------------------------------------
// One accessor per activation format, F = View::split: exact fp32, split f16 (a hi and a lo plane per pixel, values 8 x), plain f16
// (the same layout, the lo plane never read or written).  A thread owns 16 bytes of a pixel along the channel axis: PER = 4 fp32
// channels, or 8 halves of each plane.  Stored is what memory holds of them; values() what they mean as floats, in the format's own
// domain (SPLIT_SCALE carries through every op below).  plain() and saturating() are the two ways back: a bare conversion (split:
// hi = RNE(x), lo = RNE(x - hi); no range check), and the producers' split_f16 / f16_sat with the overflow sentinel.
enum { FMT_F32 = 0, FMT_SPLIT = 1, FMT_F16 = 2 };

__host__ __device__ __forceinline__ int64_t pixel_of(const View& v, int b, int y, int x) { return ((int64_t)b * v.H + y) * v.W + x; }
__device__ __forceinline__ float* f32_at(const View& v, int64_t pix, int c) { return v.base + v.coff + c + pix * v.ldc; }
// the hi plane of a split / plain-f16 pixel at channel c; the lo plane lies v.ldc halves behind it
__device__ __forceinline__ _Float16* split_plane(const View& v, int64_t pix, int c) {
    return reinterpret_cast<_Float16*>(v.base) + pix * 2 * v.ldc + v.coff + c;
}
// N = 4 or 8 consecutive floats, 16 bytes at a time
template <int N> __device__ __forceinline__ void load_f32(const float* p, float (&x)[N]) {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + i);
        x[i] = v[0]; x[i + 1] = v[1]; x[i + 2] = v[2]; x[i + 3] = v[3];
    }
}

template <int F> struct Act {                                   // FMT_SPLIT and FMT_F16
    static_assert(F == FMT_SPLIT || F == FMT_F16, "activation format");
    static constexpr int PER = 8;
    static constexpr bool F16 = F == FMT_F16;
    struct Stored { f16x8 h, l; };                              // (plain f16: l is a placeholder no store reads)
    static __device__ __forceinline__ Stored load(const View& v, int64_t pix, int c) {
        const _Float16* q = split_plane(v, pix, c);
        Stored s;
        s.h = *reinterpret_cast<const f16x8*>(q);
        if constexpr (F16) s.l = s.h; else s.l = *reinterpret_cast<const f16x8*>(q + v.ldc);
        return s;
    }
    static __device__ __forceinline__ void values(const Stored& s, float (&x)[PER]) {
#pragma unroll
        for (int e = 0; e < PER; ++e) x[e] = F16 ? (float)s.h[e] : (float)s.h[e] + (float)s.l[e];      // exact in fp32: 22 significant bits
    }
    static __device__ __forceinline__ Stored none() { return {f16x8{0, 0, 0, 0, 0, 0, 0, 0}, f16x8{0, 0, 0, 0, 0, 0, 0, 0}}; }
    static __device__ __forceinline__ void copy_element(Stored& to, const Stored& from, int e) { to.h[e] = from.h[e]; if constexpr (!F16) to.l[e] = from.l[e]; }
    static __device__ __forceinline__ Stored plain(const float (&x)[PER]) {
        Stored s = none();
#pragma unroll
        for (int e = 0; e < PER; ++e) { const _Float16 h = (_Float16)x[e]; s.h[e] = h; s.l[e] = (_Float16)(x[e] - (float)h); }
        return s;
    }
    static __device__ __forceinline__ Stored saturating(const float (&x)[PER], float& amax) {
        Stored s = none();
        epi_split8<F16>(x, s.h, s.l, amax);
        return s;
    }
    // SC1: the write-through store of the conv epilogues (store_act16)
    template <bool SC1 = false> static __device__ __forceinline__ void store(const View& v, int64_t pix, int c, const Stored& s) {
        _Float16* q = split_plane(v, pix, c);
        if constexpr (SC1) epi_store8<F16>(q, (int)v.ldc, s.h, s.l, false);
        else {
            *reinterpret_cast<f16x8*>(q) = s.h;
            if constexpr (!F16) *reinterpret_cast<f16x8*>(q + v.ldc) = s.l;
        }
    }
};

template <> struct Act<FMT_F32> {
    static constexpr int PER = 4;
    struct Stored { f32x4 v; };
    static __device__ __forceinline__ Stored load(const View& v, int64_t pix, int c) { return {*reinterpret_cast<const f32x4*>(f32_at(v, pix, c))}; }
    static __device__ __forceinline__ void values(const Stored& s, float (&x)[PER]) {
#pragma unroll
        for (int e = 0; e < PER; ++e) x[e] = s.v[e];
    }
    static __device__ __forceinline__ Stored none() { return {f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY}}; }
    static __device__ __forceinline__ void copy_element(Stored& to, const Stored& from, int e) { to.v[e] = from.v[e]; }
    static __device__ __forceinline__ Stored plain(const float (&x)[PER]) { return {f32x4{x[0], x[1], x[2], x[3]}}; }
    static __device__ __forceinline__ Stored saturating(const float (&x)[PER], float&) { return plain(x); }
    template <bool SC1 = false> static __device__ __forceinline__ void store(const View& v, int64_t pix, int c, const Stored& s) {
        *reinterpret_cast<f32x4*>(f32_at(v, pix, c)) = s.v;
    }
};

// thread index t -> the pixel (b, y, x) of an H x W map (pix = (b * H + y) * W + x) and the first of its `per` channels
struct Pos { int64_t pix; int b, y, x, c; };
__device__ __forceinline__ Pos position(int64_t t, int CV, int per, int H, int W) {
    Pos o;
    o.c = (int)(t % CV) * per;
    o.pix = t / CV;
    int64_t p = o.pix;
    o.x = (int)(p % W); p /= W;
    o.y = (int)(p % H);
    o.b = (int)(p / H);
    return o;
}

// Host side: the one view check (16-byte pieces of format `format`, or of `per` channels), the threads of a launch over the pixels of
// `v`, and the one dispatch on View::split: f(integral_constant<int, F>).
static int per_thread(int format) { return format ? 8 : 4; }
static bool view_ok(const View& v, int format, int per = 0) {
    if (!per) per = per_thread(format);
    return v.base && format >= FMT_F32 && format <= FMT_F16 && v.split == format && v.C % per == 0 && v.ldc % per == 0 && v.coff % per == 0;
}
static bool same_map(const View& a, const View& b) { return a.C == b.C && a.H == b.H && a.W == b.W; }
static int64_t threads_over(const View& v, int B) { return (int64_t)B * v.H * v.W * (v.C / per_thread(v.split)); }
template <typename Fn> static void by_format(int format, Fn f) {
    if (format == FMT_F16) f(std::integral_constant<int, FMT_F16>{});
    else if (format == FMT_SPLIT) f(std::integral_constant<int, FMT_SPLIT>{});
    else f(std::integral_constant<int, FMT_F32>{});
}
#define RTOD_LAUNCH_BY_FORMAT(format, kernel, total, stream, ...) \
    by_format(format, [&](auto f_) { hipLaunchKernelGGL((kernel<decltype(f_)::value>), dim3(grid_for(total, 256)), dim3(256), 0, stream, __VA_ARGS__); })

// ---------------------------------------------------------------------------------------------
// bilinear x2, align_corners=False (reference: nn.Upsample(scale_factor=2, mode="bilinear"),
// src/darknet.py:587-593).  src = (dst+0.5)/2-0.5 clamped at 0; weights are
// exactly {1,0} on the borders and {0.25,0.75} inside.  Evaluated as wy0*(wx0*a+wx1*b)+wy1*(wx0*c+wx1*d),
// ATen's separable order.  Interpolation is linear, so the split format runs directly on hi + lo and re-splits the result with the
// plain conversion (no saturation, no report: the result lies between its inputs); plain f16 rounds once (RNE).
__device__ __forceinline__ void up_coord(int o, int n, int& i0, int& i1, float& w1) {
    float src = ((float)o + 0.5f) * 0.5f - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    i1 = i0 + (i0 < n - 1 ? 1 : 0);
    w1 = src - (float)i0;
}

template <int F>
__global__ void upsample2x_kernel(View in, View out, int B) {
    using A = Act<F>;
    const int CV = in.C / A::PER;
    const int64_t total = (int64_t)B * out.H * out.W * CV;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const Pos o = position(t, CV, A::PER, out.H, out.W);
        int y0, y1, x0, x1; float wy1, wx1;
        up_coord(o.y, in.H, y0, y1, wy1);
        up_coord(o.x, in.W, x0, x1, wx1);
        const float wy0 = 1.f - wy1, wx0 = 1.f - wx1;
        float v00[A::PER], v01[A::PER], v10[A::PER], v11[A::PER], r[A::PER];
        A::values(A::load(in, pixel_of(in, o.b, y0, x0), o.c), v00);
        A::values(A::load(in, pixel_of(in, o.b, y0, x1), o.c), v01);
        A::values(A::load(in, pixel_of(in, o.b, y1, x0), o.c), v10);
        A::values(A::load(in, pixel_of(in, o.b, y1, x1), o.c), v11);
#pragma unroll
        for (int e = 0; e < A::PER; ++e)
            r[e] = wy0 * (wx0 * v00[e] + wx1 * v01[e]) + wy1 * (wx0 * v10[e] + wx1 * v11[e]);
        A::store(out, o.pix, o.c, A::plain(r));
    }
}

int launch_upsample2x(const View& in, const View& out, int B, hipStream_t s) {
    if (!view_ok(in, in.split) || !view_ok(out, in.split) || out.H != 2 * in.H || out.W != 2 * in.W || out.C != in.C) {
        set_error("upsample2x: bad views"); return RTOD_E_ARG;
    }
    RTOD_LAUNCH_BY_FORMAT(in.split, upsample2x_kernel, threads_over(out, B), s, in, out, B);
    return hip_fail(hipGetLastError(), "upsample2x launch");
}

// nearest x2 (cfg extension `[upsample] mode=nearest`; nn.Upsample(scale_factor=2, mode="nearest")): out(y, x) = in(y/2, x/2).
// A pure copy of the stored representation in every format.
template <int F>
__global__ void upsample_nearest2x_kernel(View in, View out, int B) {
    using A = Act<F>;
    const int CV = in.C / A::PER;
    const int64_t total = (int64_t)B * out.H * out.W * CV;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const Pos o = position(t, CV, A::PER, out.H, out.W);
        A::store(out, o.pix, o.c, A::load(in, pixel_of(in, o.b, o.y >> 1, o.x >> 1), o.c));
    }
}

int launch_upsample_nearest2x(const View& in, const View& out, int B, hipStream_t s) {
    if (!view_ok(in, in.split) || !view_ok(out, in.split) || in.C != out.C || out.H != 2 * in.H || out.W != 2 * in.W) { set_error("upsample_nearest: bad views"); return RTOD_E_ARG; }
    RTOD_LAUNCH_BY_FORMAT(in.split, upsample_nearest2x_kernel, threads_over(out, B), s, in, out, B);
    return hip_fail(hipGetLastError(), "upsample_nearest launch");
}

// ---------------------------------------------------------------------------------------------
// stand-alone shortcut (src/darknet.py:263-268) for cfgs where the add cannot ride a conv epilogue, and for plans with option
// keep_backbone_activations, which hold the shortcut out of the conv's epilogue.  One fp32 add of the operands' values.  Split
// format: (ah + al) + (bh + bl) in the format's own domain, split again by split_f16 — the sum rounds once, at its store, and
// saturates and reports like every other split producer.  Plain f16: ah + bh through f16_sat, no lo plane.
template <int F>
__global__ void add_kernel(View a, View b, View out, int B, int32_t* ovf) {
    using A = Act<F>;
    const int CV = a.C / A::PER;
    float amax = 0.f;
    const int64_t total = (int64_t)B * a.H * a.W * CV;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const Pos o = position(t, CV, A::PER, a.H, a.W);
        float x[A::PER], y[A::PER], r[A::PER];
        A::values(A::load(a, o.pix, o.c), x);
        A::values(A::load(b, o.pix, o.c), y);
#pragma unroll
        for (int e = 0; e < A::PER; ++e) r[e] = x[e] + y[e];
        A::store(out, o.pix, o.c, A::saturating(r, amax));
    }
    if constexpr (F != FMT_F32) split_overflow_report(ovf, amax);
}

int launch_add(const View& a, const View& b, const View& out, int B, hipStream_t s, int32_t* ovf) {
    if (!view_ok(a, a.split) || !view_ok(b, a.split) || !view_ok(out, a.split) || !same_map(a, b) || !same_map(a, out)) { set_error("add: bad views"); return RTOD_E_ARG; }
    RTOD_LAUNCH_BY_FORMAT(a.split, add_kernel, threads_over(a, B), s, a, b, out, B, ovf);
    return hip_fail(hipGetLastError(), "add launch");
}

// channel-slice copy (fallback when a route concat cannot be zero-copy): exact-fp32 plans only
__global__ void copy_kernel(View a, View out, int B) {
    using A = Act<FMT_F32>;
    const int CV = a.C / A::PER;
    const int64_t total = (int64_t)B * a.H * a.W * CV;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const Pos o = position(t, CV, A::PER, a.H, a.W);
        A::store(out, o.pix, o.c, A::load(a, o.pix, o.c));
    }
}

int launch_copy(const View& a, const View& out, int B, hipStream_t s) {
    if (a.split || out.split) { set_error("copy: split-format views unsupported (route concat must be zero-copy)"); return RTOD_E_ARG; }
    if (!view_ok(a, FMT_F32) || !view_ok(out, FMT_F32) || !same_map(a, out)) { set_error("copy: bad views"); return RTOD_E_ARG; }
    hipLaunchKernelGGL(copy_kernel, dim3(grid_for(threads_over(a, B), 256)), dim3(256), 0, s, a, out, B);
    return hip_fail(hipGetLastError(), "copy launch");
}

// ---------------------------------------------------------------------------------------------
// max-pool: size/stride floor mode (nn.MaxPool2d, src/darknet.py:547-555); stride 1 = MaxPoolStride1
// (src/darknet.py:17-46): replicate-pad right/bottom by size-1 then size/1 pool == clamp the window.
// pad > 0 (cfg extension `symmetric=1`, SPPF-style pools): the window starts pad pixels up / left and out-of-image taps
// count as -inf (nn.MaxPool2d(size, stride, pad)).
//
// The winner rule, stated once (the stand-alone pool and the pool inside the BatchNorm normalise kernel): the values are compared
// in fp32 (split: hi + lo; plain f16: hi), a candidate replaces the held element only when strictly greater, and the winner's
// STORED representation is kept as it stands — the (hi, lo) pair of a split tensor is not split again, nothing rounds.
template <int F> struct PoolMax {
    using A = Act<F>;
    float m[A::PER];
    typename A::Stored held = A::none();
    __device__ __forceinline__ PoolMax() {
#pragma unroll
        for (int e = 0; e < A::PER; ++e) m[e] = -INFINITY;
    }
    __device__ __forceinline__ void take(const typename A::Stored& s) {
        float x[A::PER];
        A::values(s, x);
#pragma unroll
        for (int e = 0; e < A::PER; ++e)
            if (x[e] > m[e]) { m[e] = x[e]; A::copy_element(held, s, e); }
    }
};

template <int F>
__global__ void maxpool_kernel(View in, View out, int B, int size, int stride, int pad) {
    using A = Act<F>;
    const int CV = in.C / A::PER;
    const int64_t total = (int64_t)B * out.H * out.W * CV;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const Pos o = position(t, CV, A::PER, out.H, out.W);
        PoolMax<F> best;
        for (int dy = 0; dy < size; ++dy) {
            int iy = o.y * stride + dy - pad;
            if (pad) { if ((unsigned)iy >= (unsigned)in.H) continue; } else if (iy > in.H - 1) iy = in.H - 1;
            for (int dx = 0; dx < size; ++dx) {
                int ix = o.x * stride + dx - pad;
                if (pad) { if ((unsigned)ix >= (unsigned)in.W) continue; } else if (ix > in.W - 1) ix = in.W - 1;
                best.take(A::load(in, pixel_of(in, o.b, iy, ix), o.c));
            }
        }
        A::store(out, o.pix, o.c, best.held);
    }
}

int launch_maxpool(const View& in, const View& out, int B, int size, int stride, int pad, hipStream_t s) {
    if (in.split != out.split) { set_error("maxpool: mixed activation formats"); return RTOD_E_ARG; }
    if (in.C != out.C || size < 1 || stride < 1 || pad < 0 || pad >= size) { set_error("maxpool: bad geometry"); return RTOD_E_ARG; }
    const int eh = pad ? (in.H + 2 * pad - size) / stride + 1 : (stride != 1 ? (in.H - size) / stride + 1 : in.H);
    const int ew = pad ? (in.W + 2 * pad - size) / stride + 1 : (stride != 1 ? (in.W - size) / stride + 1 : in.W);
    if (out.H != eh || out.W != ew) { set_error("maxpool: output %dx%d, expected %dx%d", out.H, out.W, eh, ew); return RTOD_E_ARG; }
    if (!view_ok(in, in.split) || !view_ok(out, in.split)) { set_error("maxpool: bad views"); return RTOD_E_ARG; }
    RTOD_LAUNCH_BY_FORMAT(in.split, maxpool_kernel, threads_over(out, B), s, in, out, B, size, stride, pad);
    return hip_fail(hipGetLastError(), "maxpool launch");
}

// ---------------------------------------------------------------------------------------------
// Batch-statistics BatchNorm ("as run" by the reference: detect.py never calls .eval(), so nn.BatchNorm2d normalises
// with the statistics of the batch, src/darknet.py:493-495).  Parity mode of the exact-fp32 plans (plan option
// bn_batch_stats) and of the split-f16 plans (bn_batch_split): the conv writes its raw sums as fp32 rows, the statistics kernels
// reduce per-channel mean and biased variance over (B, H, W) in double precision (PyTorch's CPU kernels accumulate float
// statistics in double) and leave the normalisation's per-channel constants, then bn_apply_kernel normalises, applies the
// activation and the shortcut.
// stats layout: [sstride] mean, [sstride] biased variance (doubles).  bn: [gstride] beta, [gstride] gamma (the order of the .weights
// stream, src/darknet.py:356-376).  Constants: [sstride] w, [sstride] b (floats).

// y = (x - mean) / sqrt(var + eps) * gamma + beta = x w + b: the ONE statement of w = gamma / sqrt(var + eps), b = beta - mean w'
// (double precision, rounded to float once each), evaluated once per channel by whichever kernel finishes the statistics.
// beta and gamma come by reference on purpose: the loads stay where the expressions use them, which keeps bn_stats_final_kernel's
// two divisions by npix interleaved (by value they ran one after the other: +0.5 us per BatchNorm layer, measured).
struct BnConstants { float w, b; };
__device__ __forceinline__ BnConstants bn_channel_constants(double mean, double var, const float& beta, const float& gamma) {
    const double invstd = bn_inv_std(var);                            // (bn_constants.h: the backward reads the same r)
    return {(float)(invstd * (double)gamma), (float)((double)beta - mean * invstd * (double)gamma)};
}
// ... and of the normalise step of one value
__device__ __forceinline__ float bn_normalise(float raw, float w, float b, int act) {
    const float u = raw * w + b;
    return apply_act(u, act);
}
// what a statistics kernel's finishing thread writes for channel c from the sums over npix pixels
__device__ __forceinline__ void bn_finish_channel(int c, double sum, double sumsq, double npix, double* __restrict__ stats, int sstride,
                                                  const float* __restrict__ bn, int gstride, float* __restrict__ wb) {
    const double mean = sum / npix;
    double var = sumsq / npix - mean * mean;
    if (var < 0) var = 0;
    stats[c] = mean;
    stats[sstride + c] = var;
    const BnConstants k = bn_channel_constants(mean, var, bn[c], bn[gstride + c]);
    wb[c] = k.w;
    wb[sstride + c] = k.b;
}

// One stage: one workgroup per group of 4 channels; threads stride over the pixels (deterministic: fixed partition, ordered tree)
__global__ __launch_bounds__(256)
void bn_stats_kernel(View x, int B, double* __restrict__ stats, int sstride, const float* __restrict__ bn, int gstride, float* __restrict__ wb) {
    const int c = blockIdx.x * 4;
    const int64_t npix = (int64_t)B * x.H * x.W;
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    for (int64_t p = threadIdx.x; p < npix; p += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(f32_at(x, p, c));
#pragma unroll
        for (int e = 0; e < 4; ++e) { s[e] += (double)v[e]; q[e] += (double)v[e] * (double)v[e]; }
    }
    __shared__ double red[2][4][256];
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[0][e][threadIdx.x] = s[e]; red[1][e][threadIdx.x] = q[e]; }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { red[0][e][threadIdx.x] += red[0][e][threadIdx.x + w]; red[1][e][threadIdx.x] += red[1][e][threadIdx.x + w]; }
        }
        __syncthreads();
    }
    if (threadIdx.x < 4 && c + (int)threadIdx.x < x.C) {
        const int e = threadIdx.x;
        bn_finish_channel(c + e, red[0][e][0], red[1][e][0], (double)npix, stats, sstride, bn, gstride, wb);
    }
}

// Two stages (round 4): bn_stats_kernel above reads 16 bytes per pixel row from C/4 workgroups (8 for the first layer) —
// every line of the tensor fetched for one of its eight 16-byte pieces at a time.  Here the pixels are cut into `nparts` ranges, a
// workgroup reads its range with consecutive threads on consecutive channels (whole lines), reduces its 256 / (C/4) pixel lanes
// through LDS in a fixed tree and writes per-channel partial sums; bn_stats_final_kernel adds the parts in ascending order.
// Fixed partition, fixed order: deterministic.  Needs 256 % (C/4) == 0 or (C/4) % 256 == 0; other channel counts keep the one stage
// (the two orders of summation differ, so neither replaces the other).
constexpr int BN_PARTS_MAX = 1024;
__global__ __launch_bounds__(256)
void bn_stats_partial_kernel(View x, int B, double* __restrict__ partial, int pstride, int nparts) {
    const int C4 = x.C / 4;
    const int64_t npix = (int64_t)B * x.H * x.W;
    const int64_t per = (npix + nparts - 1) / nparts;
    const int64_t p0 = blockIdx.x * per, p1 = p0 + per < npix ? p0 + per : npix;
    __shared__ double red[2][4][256];
    for (int cb = 0; cb < C4; cb += 256) {
        const int W = C4 - cb < 256 ? C4 - cb : 256;            // channel quads handled in this pass (divides 256)
        const int PL = 256 / W;                                 // pixel lanes
        const int cq = cb + (int)threadIdx.x % W, pl = (int)threadIdx.x / W;
        double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
        for (int64_t p = p0 + pl; p < p1; p += PL) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(f32_at(x, p, cq * 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) { s[e] += (double)v[e]; q[e] += (double)v[e] * (double)v[e]; }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) { red[0][e][threadIdx.x] = s[e]; red[1][e][threadIdx.x] = q[e]; }
        __syncthreads();
        for (int w = PL / 2; w > 0; w >>= 1) {                  // lanes pl and pl + w of the same channel quad
            if (pl < w) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { red[0][e][threadIdx.x] += red[0][e][threadIdx.x + w * W]; red[1][e][threadIdx.x] += red[1][e][threadIdx.x + w * W]; }
            }
            __syncthreads();
        }
        if (pl == 0) {
            double* o = partial + (int64_t)blockIdx.x * 2 * pstride;
#pragma unroll
            for (int e = 0; e < 4; ++e) { o[cq * 4 + e] = red[0][e][threadIdx.x]; o[pstride + cq * 4 + e] = red[1][e][threadIdx.x]; }
        }
    }
}

// 16 channels per workgroup, 16 lanes per channel: lane k adds parts k, k + 16, ... in ascending order, then a fixed tree over the lanes
// (one thread per channel walking all parts was a chain of `nparts` dependent L2 round trips: 29 us per layer)
__global__ __launch_bounds__(256)
void bn_stats_final_kernel(const double* __restrict__ partial, int pstride, int nparts, int C, double npix, double* __restrict__ stats, int sstride,
                           const float* __restrict__ bn, int gstride, float* __restrict__ wb) {
    const int cl = threadIdx.x & 15, k0 = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    double s = 0, q = 0;
    if (c < C)
        for (int k = k0; k < nparts; k += 16) { s += partial[(int64_t)k * 2 * pstride + c]; q += partial[(int64_t)k * 2 * pstride + pstride + c]; }
    __shared__ double red[2][256];
    red[0][threadIdx.x] = s; red[1][threadIdx.x] = q;
    __syncthreads();
    for (int w = 8; w > 0; w >>= 1) {
        if (k0 < w) { red[0][threadIdx.x] += red[0][threadIdx.x + w * 16]; red[1][threadIdx.x] += red[1][threadIdx.x + w * 16]; }
        __syncthreads();
    }
    if (k0 != 0 || c >= C) return;
    bn_finish_channel(c, red[0][threadIdx.x], red[1][threadIdx.x], npix, stats, sstride, bn, gstride, wb);
}

size_t bn_partial_doubles(int max_channels) { return (size_t)BN_PARTS_MAX * 2 * (size_t)max_channels + (size_t)max_channels; }   // partial sums + [2][C] float constants

// The one statistics path of both launchers: mean / variance of the raw fp32 view `x` into `stats` and the constants into the
// `partial` scratch, whose device pointer comes back in `wb`.  Two stages where the channel count allows (and the scratch holds the
// parts), else one; the constants lie behind the partial sums, or at the start of a scratch no partial sums use.
static int bn_statistics(const View& x, int B, double* stats, int sstride, const float* bn, int gstride, double* partial, int64_t partial_doubles,
                         hipStream_t s, const float*& wb) {
    if (!partial || partial_doubles < sstride) { set_error("bn statistics: no scratch for the per-channel constants"); return RTOD_E_ARG; }
    const int C4 = x.C / 4;
    const int64_t npix = (int64_t)B * x.H * x.W;
    const int nparts = (int)std::min<int64_t>(BN_PARTS_MAX, std::max<int64_t>(1, npix / 128));
    if ((256 % C4 == 0 || C4 % 256 == 0) && (int64_t)nparts * 2 * sstride + sstride <= partial_doubles) {
        float* w = reinterpret_cast<float*>(partial + (int64_t)nparts * 2 * sstride);
        hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(nparts), dim3(256), 0, s, x, B, partial, sstride, nparts);
        if (hipGetLastError() != hipSuccess) return hip_fail(hipGetLastError(), "bn_stats_partial launch");
        hipLaunchKernelGGL(bn_stats_final_kernel, dim3((x.C + 15) / 16), dim3(256), 0, s, partial, sstride, nparts, x.C, (double)npix, stats, sstride, bn, gstride, w);
        wb = w;
        return hip_fail(hipGetLastError(), "bn_stats_final launch");
    }
    float* w = reinterpret_cast<float*>(partial);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(C4), dim3(256), 0, s, x, B, stats, sstride, bn, gstride, w);
    wb = w;
    return hip_fail(hipGetLastError(), "bn_stats launch");
}

// y = act(x w + b) + shortcut from the raw fp32 view x and the constants, into format F (x and y may be the same fp32 view).  One
// thread per Act<F>::PER channels of a pixel.  fp32: the shortcut operand is added as it is.  Split (the conv's raw-sum instance,
// EPI_RAW, wrote x as dense rows): y = act(x w + b) + (hi + lo) / 8, and 8 y goes through split_f16 with the write-through stores
// of the conv epilogues.
template <int F>
__global__ void bn_apply_kernel(View x, View y, View res, int has_res, int B, const float* __restrict__ wb, int sstride, int act, int32_t* ovf) {
    using A = Act<F>;
    const int CV = x.C / A::PER;
    float amax = 0.f;
    const int64_t total = (int64_t)B * x.H * x.W * CV;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const Pos o = position(t, CV, A::PER, x.H, x.W);
        float u[A::PER], w[A::PER], b[A::PER], r[A::PER];
        load_f32(f32_at(x, o.pix, o.c), u);
        load_f32(wb + o.c, w);
        load_f32(wb + sstride + o.c, b);
#pragma unroll
        for (int e = 0; e < A::PER; ++e) r[e] = 0.f;
        if (has_res) A::values(A::load(res, o.pix, o.c), r);
#pragma unroll
        for (int e = 0; e < A::PER; ++e) {
            u[e] = bn_normalise(u[e], w[e], b[e], act);
            if constexpr (F == FMT_F32) u[e] = has_res ? u[e] + r[e] : u[e];
            else {
                if (has_res) u[e] += r[e] * (1.0f / SPLIT_SCALE);
                u[e] = u[e] * SPLIT_SCALE;
            }
        }
        A::template store<true>(y, o.pix, o.c, A::saturating(u, amax));
    }
    if constexpr (F != FMT_F32) split_overflow_report(ovf, amax);
}

// The same followed by the 2x2 / stride-2 max-pool that alone reads the conv (plan options bn_split_narrow + fuse_bn_pool): the
// conv's full-resolution split map is never stored.  One thread per 8 channels of a POOLED pixel of `y` (the pool's view).  Every
// window position, in (dy, dx) order, is normalised, activated and split as bn_apply_kernel does it (amax over all four: the range
// flag equals the stand-alone path's) and offered to the max-pool's own winner rule (PoolMax): bit-identical to bn_apply_kernel
// followed by maxpool_kernel.  x.H and x.W are even (y.H = x.H / 2, y.W = x.W / 2).
__global__ void bn_apply_split_pool_kernel(View x, View y, int B, const float* __restrict__ wb, int sstride, int act, int32_t* ovf) {
    using A = Act<FMT_SPLIT>;
    const int CV = x.C / A::PER;
    float amax = 0.f;
    const int64_t total = (int64_t)B * y.H * y.W * CV;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const Pos o = position(t, CV, A::PER, y.H, y.W);
        float w[A::PER], b[A::PER], v[4][A::PER];
        load_f32(wb + o.c, w);
        load_f32(wb + sstride + o.c, b);
        // the four window rows first: eight 16-byte loads in flight
#pragma unroll
        for (int pos = 0; pos < 4; ++pos) load_f32(f32_at(x, pixel_of(x, o.b, 2 * o.y + (pos >> 1), 2 * o.x + (pos & 1)), o.c), v[pos]);
        PoolMax<FMT_SPLIT> best;
#pragma unroll
        for (int pos = 0; pos < 4; ++pos) {
            float u[A::PER];
#pragma unroll
            for (int e = 0; e < A::PER; ++e) u[e] = bn_normalise(v[pos][e], w[e], b[e], act) * SPLIT_SCALE;
            best.take(A::saturating(u, amax));
        }
        A::store<true>(y, o.pix, o.c, best.held);
    }
    split_overflow_report(ovf, amax);
}

int launch_bn_batch(const View& x, const View& y, const View* res, int B, double* stats, int sstride, const float* bn, int gstride, int act,
                    double* partial, int64_t partial_doubles, hipStream_t s) {
    if (x.split || y.split || (res && res->split)) { set_error("bn_batch: exact-fp32 plans only"); return RTOD_E_ARG; }
    if (!view_ok(x, FMT_F32) || !view_ok(y, FMT_F32) || !same_map(x, y) || !stats || !bn || gstride < x.C || sstride < x.C) { set_error("bn_batch: bad views"); return RTOD_E_ARG; }
    if (res && (!view_ok(*res, FMT_F32) || !same_map(*res, x))) { set_error("bn_batch: bad shortcut view"); return RTOD_E_ARG; }
    const float* wb = nullptr;
    if (int rc = bn_statistics(x, B, stats, sstride, bn, gstride, partial, partial_doubles, s, wb)) return rc;
    hipLaunchKernelGGL(bn_apply_kernel<FMT_F32>, dim3(grid_for(threads_over(x, B), 256)), dim3(256), 0, s, x, y, res ? *res : x, res ? 1 : 0, B, wb, sstride, act, (int32_t*)nullptr);
    return hip_fail(hipGetLastError(), "bn_apply launch");
}

int launch_bn_batch_split(const View& raw, const View& y, const View* res, int B, double* stats, int sstride, const float* bn, int gstride, int act,
                          double* partial, int64_t partial_doubles, int32_t* ovf, hipStream_t s, int pool) {
    if (!view_ok(raw, FMT_F32, 8)) { set_error("bn_batch_split: bad raw-sum view"); return RTOD_E_ARG; }
    if (pool && (res || raw.H % 2 || raw.W % 2)) { set_error("bn_batch_split: the fused 2x2 max-pool needs an even map and no shortcut"); return RTOD_E_ARG; }
    const int yh = pool ? raw.H / 2 : raw.H, yw = pool ? raw.W / 2 : raw.W;
    if (!view_ok(y, FMT_SPLIT) || raw.C != y.C || yh != y.H || yw != y.W || !stats || !bn || gstride < raw.C || sstride < raw.C || B < 1) { set_error("bn_batch_split: bad views"); return RTOD_E_ARG; }
    if (res && (!view_ok(*res, FMT_SPLIT) || !same_map(*res, raw))) { set_error("bn_batch_split: bad shortcut view"); return RTOD_E_ARG; }
    const float* wb = nullptr;
    if (int rc = bn_statistics(raw, B, stats, sstride, bn, gstride, partial, partial_doubles, s, wb)) return rc;
    const dim3 grid(grid_for(threads_over(y, B), 256));           // 8 channels of a written pixel per thread
    if (pool) hipLaunchKernelGGL(bn_apply_split_pool_kernel, grid, dim3(256), 0, s, raw, y, B, wb, sstride, act, ovf);
    else hipLaunchKernelGGL(bn_apply_kernel<FMT_SPLIT>, grid, dim3(256), 0, s, raw, y, res ? *res : y, res ? 1 : 0, B, wb, sstride, act, ovf);
    return hip_fail(hipGetLastError(), "bn_apply_split launch");
}

// Training-mode side effect of nn.BatchNorm2d on its buffers, for ALL BatchNorm layers of a plan in one launch (the host class
// used to fetch every layer's statistics with a synchronising call and update the module buffers with two small copies each:
// 72 round trips + 144 copies per forward at YOLOv3).  running = (1 - momentum) * running + momentum * batch statistic in float32,
// the variance UNBIASED (n / (n - 1)), as torch does (momentum 0.1 by default; src/darknet.py:493-495 builds plain BatchNorm2d).
// One workgroup per (layer, 256 channels).
__global__ __launch_bounds__(256)
void bn_update_running_kernel(BnUpdateTable t, const double* __restrict__ stats, float momentum, double momentum_d) {
    const BnUpdateEntry e = t.e[blockIdx.y];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= e.channels) return;
    const double mean = stats[e.stats_off + c];
    const double var = stats[e.stats_off + e.sstride + c] * e.unbias;
    // mul_(1 - momentum) then add_(float32(momentum * statistic)): two rounded float32 operations, no contraction
    e.running_mean[c] = __fadd_rn(__fmul_rn(e.running_mean[c], 1.0f - momentum), (float)(momentum_d * mean));
    e.running_var[c] = __fadd_rn(__fmul_rn(e.running_var[c], 1.0f - momentum), (float)(momentum_d * var));
}

int launch_bn_update_running(const BnUpdateEntry* entries, int n, const double* stats, double momentum, hipStream_t s) {
    if (!entries || n < 1 || !stats) { set_error("bn_update_running: bad args"); return RTOD_E_ARG; }
    for (int i0 = 0; i0 < n; i0 += BN_UPDATE_MAX) {
        BnUpdateTable t;
        const int m = n - i0 < BN_UPDATE_MAX ? n - i0 : BN_UPDATE_MAX;
        int cmax = 0;
        for (int i = 0; i < m; ++i) { t.e[i] = entries[i0 + i]; if (t.e[i].channels > cmax) cmax = t.e[i].channels; }
        hipLaunchKernelGGL(bn_update_running_kernel, dim3((cmax + 255) / 256, m), dim3(256), 0, s, t, stats, (float)momentum, momentum);
        if (hipGetLastError() != hipSuccess) return hip_fail(hipGetLastError(), "bn_update_running launch");
    }
    return RTOD_OK;
}

// ---------------------------------------------------------------------------------------------
// NHWC view -> dense NCHW (test/debug read-back of a layer output)
__global__ void view_to_nchw_kernel(View in, int B, float* __restrict__ out) {
    const int64_t total = (int64_t)B * in.C * in.H * in.W;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t p = t;
        const int x = (int)(p % in.W); p /= in.W;
        const int y = (int)(p % in.H); p /= in.H;
        const int c = (int)(p % in.C);
        const int b = (int)(p / in.C);
        const int64_t pix = pixel_of(in, b, y, x);
        if (in.split) {
            const _Float16* q = split_plane(in, pix, c);
            out[t] = (in.split == 2 ? (float)q[0] : (float)q[0] + (float)q[in.ldc]) * (1.0f / SPLIT_SCALE);     // 2: plain f16, hi plane only
        } else {
            out[t] = in.base[pix * in.ldc + in.coff + c];
        }
    }
}

int launch_view_to_nchw(const View& in, int B, float* out, hipStream_t s) {
    if (!in.base || !out) { set_error("view_to_nchw: null"); return RTOD_E_ARG; }
    const int64_t total = (int64_t)B * in.C * in.H * in.W;
    hipLaunchKernelGGL(view_to_nchw_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, in, B, out);
    return hip_fail(hipGetLastError(), "view_to_nchw launch");
}

// ---------------------------------------------------------------------------------------------
// stand-alone head decode = predict_transform (src/util.py:175-239) over a strided raw tensor.
// out row r = (gy*GW + gx)*A + a, attribute c  <->  raw channel a*attrs + c at cell (gy, gx).
__device__ __forceinline__ float sigm(float v) { return 1.0f / (1.0f + expf(-v)); }

__global__ void decode_kernel(const float* __restrict__ raw, int64_t sb, int64_t sc, int64_t sy, int64_t sx,
                              int B, DecodeArgs d, float* __restrict__ out) {
    const int AC = d.n_anchors * d.attrs;
    const int64_t per_img = (int64_t)d.GH * d.GW * AC;
    const int64_t total = (int64_t)B * per_img;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / per_img;
        const int64_t r = t - b * per_img;
        const int cell = (int)(r / AC);
        const int n = (int)(r - (int64_t)cell * AC);
        const int gy = cell / d.GW, gx = cell - gy * d.GW;
        const int a = n / d.attrs, c = n - a * d.attrs;
        float v = raw[b * sb + (int64_t)n * sc + (int64_t)gy * sy + (int64_t)gx * sx];
        if (c >= 4) v = sigm(v);
        else if (d.v5) {                                 // YOLOv5-style head (cfg extension)
            const float sg = sigm(v);
            if (c < 2) v = ((sg * 2.0f - 0.5f) + (float)(c == 0 ? gx : gy)) * d.stride;
            else { const float t2 = sg * 2.0f; v = (t2 * t2) * (c == 2 ? d.aw[a] : d.ah[a]); }
        }
        else if (c < 2) { v = sigm(v); if (!d.train) v = (v + (float)(c == 0 ? gx : gy)) * d.stride; }
        else if (!d.train) v = (expf(v) * (c == 2 ? d.aw[a] : d.ah[a])) * d.stride;
        out[b * d.img_stride + d.head_off + r] = v;
    }
}

int launch_decode(const float* raw, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int B,
                  const DecodeArgs& d, float* out, hipStream_t s) {
    if (!raw || !out || d.GH <= 0 || d.GW <= 0 || d.attrs < 5 || d.n_anchors < 1 || d.n_anchors > 4) { set_error("decode: bad args"); return RTOD_E_ARG; }
    const int64_t total = (int64_t)B * d.GH * d.GW * d.n_anchors * d.attrs;
    hipLaunchKernelGGL(decode_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, raw, sb, sc, sy, sx, B, d, out);
    return hip_fail(hipGetLastError(), "decode launch");
}

// ---------------------------------------------------------------------------------------------
// TRAIN=True decode -> eval decode, in place, columns 0-3 of one head: what the decode above (and the conv epilogues) add when
// train == 0, from the values they store when train != 0 — the sigmoid for x / y, the raw sum for w / h — in their operation
// order.  hw_exp: the head was decoded by the split-f16 epilogue (conv_f16s3_common.h: __expf), else by libm expf.
__global__ void finish_decode_kernel(float* __restrict__ out, int B, DecodeArgs d, int hw_exp) {
    const int64_t rows = (int64_t)d.GH * d.GW * d.n_anchors;
    const int64_t total = (int64_t)B * rows * 4;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / (rows * 4);
        const int64_t q = t - b * rows * 4;
        const int64_t r = q >> 2;
        const int c = (int)(q & 3);
        const int cell = (int)(r / d.n_anchors), a = (int)(r - (int64_t)cell * d.n_anchors);
        const int gy = cell / d.GW, gx = cell - gy * d.GW;
        float* p = out + b * d.img_stride + d.head_off + r * d.attrs + c;
        float v = *p;
        if (c < 2) v = (v + (float)(c == 0 ? gx : gy)) * d.stride;
        else {
            const float ex = hw_exp ? __expf(v) : expf(v);
            v = (ex * (c == 2 ? d.aw[a] : d.ah[a])) * d.stride;
        }
        *p = v;
    }
}

int launch_finish_decode(float* out, int B, const DecodeArgs& d, int hw_exp, hipStream_t s) {
    if (!out || d.GH <= 0 || d.GW <= 0 || d.attrs < 5 || d.n_anchors < 1 || d.n_anchors > 4 || d.v5) { set_error("finish_decode: bad args"); return RTOD_E_ARG; }
    const int64_t total = (int64_t)B * d.GH * d.GW * d.n_anchors * 4;
    hipLaunchKernelGGL(finish_decode_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, out, B, d, hw_exp);
    return hip_fail(hipGetLastError(), "finish_decode launch");
}

// ---------------------------------------------------------------------------------------------
// confidence_mask (src/util.py:106-117): out = pred * float(pred[...,4] > conf)
__global__ void confidence_mask_kernel(const float* __restrict__ pred, int64_t rows, int attrs, float conf, float* __restrict__ out) {
    const int64_t total = rows * attrs;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / attrs;
        const float m = pred[r * attrs + 4] > conf ? 1.0f : 0.0f;
        out[t] = pred[t] * m;
    }
}

int launch_confidence_mask(const float* pred, int64_t rows, int attrs, float conf, float* out, hipStream_t s) {
    if (!pred || !out || attrs < 5) { set_error("confidence_mask: bad args"); return RTOD_E_ARG; }
    hipLaunchKernelGGL(confidence_mask_kernel, dim3(grid_for(rows * attrs, 256)), dim3(256), 0, s, pred, rows, attrs, conf, out);
    return hip_fail(hipGetLastError(), "confidence_mask launch");
}

}  // namespace rtod
