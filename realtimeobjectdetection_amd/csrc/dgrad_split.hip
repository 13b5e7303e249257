// Data gradient of a size x size (1 or 3), stride 1, same-padding convolution on the forward's split-f16 MFMA tiles (opt-in:
// rtod_conv_dgrad_split; the exact entry is rtod_conv_dgrad, dgrad.hip), gfx950.
//   dx[b][c][y][x] = m(y_in[b][c][y][x]) * sum_{ky,kx,o} v[o][c][ky][kx] * dz[b][o][y + pad - ky][x + pad - kx]
// is itself a stride-1 same-padding conv: it reads dz, its "cin" is the forward's cout rounded up to 32 (Kc), its "cout" the forward's
// cin, and its weights are the forward's with O and I swapped and the taps flipped.  So the conv is an EXISTING launcher, called
// with a bare ConvArgs that sets raw_out / raw_ld (the raw-sum instances: fp32 sums out, no bias, activation or split store), and
// which tile runs is decided by Plan::tile_legal / default_tile / launch_split_variant over a private one-conv plan description
// (dgs_describe below fills the shape facts and lets Plan::layout_weights decide band / narrow / sliced as for any conv).
// New here are the four bandwidth kernels around it, all on the caller's stream, no atomics, nothing synchronises:
//   (a) dgs_amax_kernel + dgs_exponent_kernel: per image b, a_b = max |dz[b]| (a maximum: independent of the order) -> e_b with
//       a_b 2^e_b in [2^12, 2^13) (a_b == 0: e_b = 0; e_b held to -126 .. 126 so that 2^e_b and 2^-e_b are normal floats).  Per
//       image, so that an image's dx does not depend on the batch it rides in.
//   (b) dgs_split_dz_kernel: NCHW fp32 dz -> v = dz 2^e_b as f16 hi = RNE(v), lo = RNE(v - hi) in the NHWC split layout the conv
//       kernels read ([pixel][hi plane Kc][lo plane Kc], no SPLIT_SCALE), channels cout .. Kc written as zeros; 32 channels x 64
//       pixels through LDS, 16-byte pieces on both sides where the map has a multiple of 4 pixels (else 4-byte loads).
//   (c) dgs_rowmax_kernel + dgs_pack_w_kernel: v = (float)((double)w * row_scale[o]); gradient-conv output row c (the forward's
//       input channel) gets the pre-scale of channel_prescale (plan_weights.cpp): max over o and taps of |(double)w * scale| placed
//       in [2^12, 2^13), e in -24 .. 40, an all-zero row e = 0; hi / lo planes [chunk][Npad][32] with K index
//       ((o / 32) * taps + tap') * 32 + o % 32, tap' = taps - 1 - tap (the flip).  Packed from the float32 masters at every call:
//       they step in place.  Rows cin .. Npad and channels cout .. Kc are zeros; inv_scale[c] = 2^-e_c rides to the conv's epilogue.
//   (d) dgs_finish_kernel: raw rows [M][Npad] (= sum * 2^-e_c, exact) -> NCHW dx = m(y) * (raw * 2^-e_b): the scale is exact, the
//       mask is the one rounding multiplication.
// Every byte of the workspace that a kernel reads is written earlier in the same call (padding included).
#include "plan.h"
#include "conv_f16s3_common.h"

#include <cmath>

namespace rtod {

constexpr int DGS_THREADS = 256;
constexpr int DGS_MAX_PARTS = 64;        // partial maxima per image: one wave of dgs_exponent_kernel reads them
constexpr int DGS_MAX_WPARTS = 16;       // slices of cout in the row maximum
constexpr int DGS_CT = 32, DGS_PT = 64;  // channels x pixels of a transpose tile

// ---- (a) per-image max |dz|: `parts` workgroups per image, each over an interleaved share
template <bool VEC>
__global__ __launch_bounds__(DGS_THREADS)
void dgs_amax_kernel(const float* __restrict__ dz, int64_t per_image, int parts, float* __restrict__ partial) {
    __shared__ float red[DGS_THREADS / 64];
    const int b = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const float* p = dz + (int64_t)b * per_image;
    float m = 0.f;
    const int64_t step = (int64_t)parts * DGS_THREADS;
    if constexpr (VEC) {
        const f32x4* q = reinterpret_cast<const f32x4*>(p);
        for (int64_t i = (int64_t)part * DGS_THREADS + tid; i < per_image / 4; i += step) {
            const f32x4 v = q[i];
            m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
        }
    } else {
        for (int64_t i = (int64_t)part * DGS_THREADS + tid; i < per_image; i += step) m = fmaxf(m, fabsf(p[i]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) partial[b * parts + part] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ... to the image's scales: scale[b] = 2^e_b, scale[batch + b] = 2^-e_b
__global__ __launch_bounds__(64)
void dgs_exponent_kernel(const float* __restrict__ partial, int parts, int batch, float* __restrict__ scale) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float m = lane < parts ? partial[b * parts + lane] : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) {
        int e = 0;
        if (m > 0.f && m < __builtin_huge_valf()) { int ex; (void)frexpf(m, &ex); e = 13 - ex; }     // m * 2^e in [2^12, 2^13)
        e = e < -126 ? -126 : e > 126 ? 126 : e;
        scale[b] = ldexpf(1.0f, e);
        scale[batch + b] = ldexpf(1.0f, -e);
    }
}

// ---- (b) dz [B][cout][HW] fp32 -> split planes [B * HW][2][Kc] halves.  grid (pixel tiles, Kc / 32, B)
template <bool VEC>
__global__ __launch_bounds__(DGS_THREADS)
void dgs_split_dz_kernel(const float* __restrict__ dz, const float* __restrict__ scale, int cout, int Kc, int HW, _Float16* __restrict__ out) {
    __shared__ float T[DGS_CT][DGS_PT + 1];
    const int p0 = blockIdx.x * DGS_PT, c0 = blockIdx.y * DGS_CT, b = blockIdx.z, tid = threadIdx.x;
    const float up = scale[b];
    const float* src = dz + ((int64_t)b * cout + c0) * HW + p0;
    if constexpr (VEC) {                                          // HW % 4 == 0: a quad never straddles the end of a channel's map
        for (int i = tid; i < DGS_CT * (DGS_PT / 4); i += DGS_THREADS) {
            const int c = i / (DGS_PT / 4), p = (i - c * (DGS_PT / 4)) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (c0 + c < cout && p0 + p < HW) v = *reinterpret_cast<const f32x4*>(src + (int64_t)c * HW + p);
#pragma unroll
            for (int j = 0; j < 4; ++j) T[c][p + j] = v[j];
        }
    } else {
        for (int i = tid; i < DGS_CT * DGS_PT; i += DGS_THREADS) {
            const int c = i / DGS_PT, p = i - c * DGS_PT;
            T[c][p] = (c0 + c < cout && p0 + p < HW) ? src[(int64_t)c * HW + p] : 0.f;
        }
    }
    __syncthreads();
    const int p = tid >> 2, q = tid & 3;                          // 64 pixels x 4 pieces of 8 channels
    if (p0 + p >= HW) return;
    f16x8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = T[q * 8 + e][p] * up;                     // exact: |v| < 2^13
        const _Float16 hh = (_Float16)v;
        h[e] = hh; l[e] = (_Float16)(v - (float)hh);
    }
    _Float16* o = out + ((int64_t)b * HW + p0 + p) * 2 * Kc + c0 + q * 8;
    *reinterpret_cast<f16x8*>(o) = h;
    *reinterpret_cast<f16x8*>(o + Kc) = l;
}

// ---- (c) row maxima: partial[part][c] = max over the part's o and all taps of |(double)w[o][c][tap] * scale[o]|.  grid (cin tiles of 64, parts)
template <int TAPS, bool SCALED>
__global__ __launch_bounds__(DGS_THREADS)
void dgs_rowmax_kernel(const float* __restrict__ w, const double* __restrict__ scale, int cout, int cin, int olen, double* __restrict__ partial) {
    __shared__ double red[DGS_THREADS / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, o0 = blockIdx.y * olen, o1 = min(cout, o0 + olen);
    double m = 0.0;
    if (c < cin)
        for (int o = o0 + wave; o < o1; o += DGS_THREADS / 64) {
            const float* p = w + ((int64_t)o * cin + c) * TAPS;
            const double s = SCALED ? scale[o] : 1.0;
#pragma unroll
            for (int t = 0; t < TAPS; ++t) m = fmax(m, fabs((double)p[t] * s));
        }
    red[wave][lane] = m;
    __syncthreads();
    if (wave == 0 && c < cin) partial[(int64_t)blockIdx.y * cin + c] = fmax(fmax(red[0][lane], red[1][lane]), fmax(red[2][lane], red[3][lane]));
}

// ... and the pack: 32 rows c x 32 filters o x TAPS per workgroup through LDS.  grid (Npad / 32, Kc / 32)
template <int TAPS, bool SCALED>
__global__ __launch_bounds__(DGS_THREADS)
void dgs_pack_w_kernel(const float* __restrict__ w, const double* __restrict__ scale, const double* __restrict__ rowmax, int wparts, int cout, int cin,
                       int Npad, _Float16* __restrict__ hi, _Float16* __restrict__ lo, float* __restrict__ inv, float* __restrict__ bias) {
    constexpr int RUN = 32 * TAPS, LD = RUN + 1;
    __shared__ float T[32 * LD];
    __shared__ double ps[32];
    const int c0 = blockIdx.x * 32, oc = blockIdx.y, o0 = oc * 32, tid = threadIdx.x;
    const bool rows = c0 < cin;                                   // cin % 32 == 0: a whole tile of rows, or padding rows alone
    if (tid < 32) {
        const int c = c0 + tid;
        double mx = 0.0;
        if (c < cin) for (int k = 0; k < wparts; ++k) mx = fmax(mx, rowmax[(int64_t)k * cin + c]);
        int e = 0;
        if (mx > 0.0) { int ex; (void)frexp(mx, &ex); e = 13 - ex; }      // channel_prescale: mx * 2^e in [2^12, 2^13)
        e = e < -24 ? -24 : e > 40 ? 40 : e;
        ps[tid] = ldexp(1.0, e);
        if (oc == 0) { inv[c] = (float)ldexp(1.0, -e); bias[c] = 0.f; }
    }
    if (rows)
        for (int i = tid; i < 32 * RUN; i += DGS_THREADS) {
            const int j = i / RUN, r = i - j * RUN, o = o0 + j;
            float v = 0.f;
            if (o < cout) {
                v = w[((int64_t)o * cin + c0) * TAPS + r];
                if constexpr (SCALED) v = (float)((double)v * scale[o]);
            }
            T[j * LD + r] = v;
        }
    __syncthreads();
    for (int i = tid; i < TAPS * 32 * 4; i += DGS_THREADS) {
        const int q = i & 3, c = (i >> 2) & 31, tap = i >> 7;     // tap: the gradient conv's; the forward's is TAPS - 1 - tap
        f16x8 h = {0, 0, 0, 0, 0, 0, 0, 0}, l = {0, 0, 0, 0, 0, 0, 0, 0};
        if (rows) {
            const double s = ps[c];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float vs = (float)((double)T[(q * 8 + e) * LD + c * TAPS + (TAPS - 1 - tap)] * s);      // exact (power of two)
                const _Float16 hh = (_Float16)vs;
                h[e] = hh; l[e] = (_Float16)(vs - (float)hh);
            }
        }
        const int64_t d = ((int64_t)(oc * TAPS + tap) * Npad + c0 + c) * 32 + q * 8;
        *reinterpret_cast<f16x8*>(hi + d) = h;
        *reinterpret_cast<f16x8*>(lo + d) = l;
    }
}

// ---- (d) raw [B * HW][Npad] -> dx [B][cin][HW].  grid (pixel tiles, cin / 32, B)
template <bool VEC>
__global__ __launch_bounds__(DGS_THREADS)
void dgs_finish_kernel(const float* __restrict__ raw, int Npad, const float* __restrict__ scale, int batch, const float* __restrict__ y, float slope,
                       int cin, int HW, float* __restrict__ dx) {
    __shared__ float T[DGS_PT][DGS_CT + 1];
    const int p0 = blockIdx.x * DGS_PT, c0 = blockIdx.y * DGS_CT, b = blockIdx.z, tid = threadIdx.x;
    const float down = scale[batch + b];
    for (int i = tid; i < DGS_PT * (DGS_CT / 4); i += DGS_THREADS) {
        const int p = i / (DGS_CT / 4), q = (i - p * (DGS_CT / 4)) * 4;
        if (p0 + p >= HW) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(raw + ((int64_t)b * HW + p0 + p) * Npad + c0 + q);
#pragma unroll
        for (int j = 0; j < 4; ++j) T[p][q + j] = v[j];
    }
    __syncthreads();
    const bool masked = y != nullptr && slope != 1.0f;
    if constexpr (VEC) {
        for (int i = tid; i < DGS_CT * (DGS_PT / 4); i += DGS_THREADS) {
            const int c = i / (DGS_PT / 4), p = (i - c * (DGS_PT / 4)) * 4;
            if (p0 + p >= HW) continue;
            const int64_t idx = ((int64_t)b * cin + c0 + c) * HW + p0 + p;
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = T[p + j][c] * down;
            if (masked) {
                const f32x4 yy = *reinterpret_cast<const f32x4*>(y + idx);
#pragma unroll
                for (int j = 0; j < 4; ++j) if (!(yy[j] > 0.f)) o[j] = o[j] * slope;
            }
            *reinterpret_cast<f32x4*>(dx + idx) = o;
        }
    } else {
        for (int i = tid; i < DGS_CT * DGS_PT; i += DGS_THREADS) {
            const int c = i / DGS_PT, p = i - c * DGS_PT;
            if (p0 + p >= HW) continue;
            const int64_t idx = ((int64_t)b * cin + c0 + c) * HW + p0 + p;
            float v = T[p][c] * down;
            if (masked && !(y[idx] > 0.f)) v = v * slope;
            dx[idx] = v;
        }
    }
}

// ---- host.  The gradient conv described as a plan of its own: layer 0 stands for the producer of dz, layer 1 is the conv (a
// BatchNorm conv of a batch-statistics split plan, which is what makes its launch a raw-sum launch: Plan::raw_launch); layout_weights
// lays out its packed image and decides band / narrow / sliced by the plan's rules.  Nothing here touches a device.
struct DgsDesc {
    Plan plan;
    int taps = 1, Kc = 0, HW = 0, parts = 1, wparts = 1, olen = 1;
    int64_t M = 0;
    size_t off_amax = 0, off_scale = 0, off_rowmax = 0, off_image = 0, off_dz = 0, off_raw = 0, bytes = 0;
    const Launch& launch() const { return plan.launches[0]; }
    const PackedConv& conv() const { return plan.convs[0]; }
};

static int dgs_describe(const char* who, int batch, int cout, int cin, int h, int w, int size, DgsDesc& d) {
    if (batch < 1 || batch > 65535 || cout < 1 || cin < 32 || cin % 32 || h < 1 || w < 1 || (size != 1 && size != 3)) {
        set_error("%s: unsupported arguments (batch=%d cout=%d cin=%d height=%d width=%d size=%d; batch 1 .. 65535, cin a multiple of 32, size 1 or 3)", who, batch, cout, cin, h, w, size);
        return RTOD_E_ARG;
    }
    d.taps = size * size;
    const int64_t Kc = ((int64_t)cout + 31) / 32 * 32, Npad = ((int64_t)cin + 127) / 128 * 128, HW = (int64_t)h * w, M = batch * HW;
    if (HW > INT32_MAX || M > INT32_MAX - 256 || Kc * d.taps > INT32_MAX) { set_error("%s: batch * pixels or cout * size * size exceeds int32", who); return RTOD_E_ARG; }
    // the conv kernels address both operands through 32-bit buffer offsets: an offset of 2 GiB is their out-of-range mark
    if (M * Kc * 4 >= (int64_t)OOB) { set_error("%s: the split dz buffer would hold %lld bytes, 2 GiB or more", who, (long long)(M * Kc * 4)); return RTOD_E_ARG; }
    if (Kc * d.taps * Npad * 2 >= (int64_t)OOB) { set_error("%s: a split weight plane would hold %lld bytes, 2 GiB or more", who, (long long)(Kc * d.taps * Npad * 2)); return RTOD_E_ARG; }
    d.Kc = (int)Kc; d.HW = (int)HW; d.M = M;
    Plan& P = d.plan;
    P.precision = 1; P.opt_bn_batch_stats = P.opt_bn_batch_split = true;
    P.height = h; P.width = w; P.max_batch = batch;
    Layer src; src.index = 0; src.cout = (int)Kc; src.hout = h; src.wout = w;
    Layer L; L.index = 1; L.type = LT_CONV; L.cin = (int)Kc; L.cout = cin; L.hin = L.hout = h; L.win = L.wout = w;
    L.size = size; L.stride = 1; L.pad = size / 2; L.bn = true; L.act = 0;
    P.layers = {src, L};
    Launch l; l.kind = LK_CONV; l.layer = 1; l.in_layer = 0; l.out_layer = 1; l.conv_slot = 0;
    P.launches = {l};
    PackedConv pc; pc.layer = 1; pc.cin_p = (int)Kc; pc.K = pc.Kpad = d.taps * (int)Kc; pc.Npad = (int)Npad;
    P.convs = {pc};
    P.layout_weights();
    const int64_t per_image = (int64_t)cout * HW;
    d.parts = (int)std::max<int64_t>(1, std::min<int64_t>(DGS_MAX_PARTS, (per_image + 4095) / 4096));
    d.wparts = std::max(1, std::min(DGS_MAX_WPARTS, (cout + 31) / 32));
    d.olen = (cout + d.wparts - 1) / d.wparts;
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off += (n + 255) / 256 * 256; return at; };
    d.off_amax = take(sizeof(float) * (size_t)batch * d.parts);
    d.off_scale = take(sizeof(float) * 2 * (size_t)batch);
    d.off_rowmax = take(sizeof(double) * (size_t)d.wparts * cin);
    d.off_image = take(sizeof(float) * (size_t)P.packed_floats);
    d.off_dz = take((size_t)(M * Kc * 4));
    d.off_raw = take(sizeof(float) * (size_t)(M * Npad));
    d.bytes = off;
    return RTOD_OK;
}

// the legal tiles of the shape, the default first, the others in ascending id order
static std::vector<int> dgs_tiles(const DgsDesc& d, int batch) {
    const Plan& P = d.plan;
    std::vector<int> ids = {P.default_tile(d.launch(), batch)};
    for (int f = 0; f < TF_COUNT; ++f) {
        const TileFamily& F = tile_family(f);
        for (int m = 0; m < F.modes; ++m)
            if (F.base + m != ids[0] && P.tile_legal(d.launch(), F.base + m)) ids.push_back(F.base + m);
    }
    return ids;
}

int conv_dgrad_split_tiles(int batch, int cout, int cin, int h, int w, int size, int* ids, int capacity) {
    if (capacity < 0 || (capacity > 0 && !ids)) { set_error("conv_dgrad_split_tiles: null pointer"); return RTOD_E_ARG; }
    DgsDesc d;
    if (int rc = dgs_describe("conv_dgrad_split_tiles", batch, cout, cin, h, w, size, d)) return rc;
    const std::vector<int> t = dgs_tiles(d, batch);
    for (int i = 0; i < (int)t.size() && i < capacity; ++i) ids[i] = t[i];
    return (int)t.size();
}

int conv_dgrad_split_workspace(int batch, int cout, int cin, int h, int w, int size, size_t* bytes) {
    if (!bytes) { set_error("conv_dgrad_split_workspace: null pointer"); return RTOD_E_ARG; }
    DgsDesc d;
    if (int rc = dgs_describe("conv_dgrad_split_workspace", batch, cout, cin, h, w, size, d)) return rc;
    *bytes = d.bytes;
    return RTOD_OK;
}

int launch_conv_dgrad_split(const float* w, const double* row_scale, const float* dz, const float* y, float slope, int batch, int cout, int cin,
                            int h, int w_, int size, int tile, float* dx, void* workspace, size_t workspace_bytes, hipStream_t s, int phases) {
    const char* who = "conv_dgrad_split";
    if (phases < 1 || phases > DGS_ALL) { set_error("%s: phases %d outside 1 .. %d", who, phases, DGS_ALL); return RTOD_E_ARG; }
    if (!w || !dz || !dx || !workspace) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    if (!(slope == slope)) { set_error("%s: slope is NaN", who); return RTOD_E_ARG; }
    DgsDesc d;
    if (int rc = dgs_describe(who, batch, cout, cin, h, w_, size, d)) return rc;
    if (workspace_bytes < d.bytes) { set_error("%s: the workspace has %zu bytes, %zu are needed", who, workspace_bytes, d.bytes); return RTOD_E_ARG; }
    if (((uintptr_t)workspace & 15) || ((uintptr_t)w & 3) || ((uintptr_t)dz & 3) || ((uintptr_t)dx & 3) || ((uintptr_t)y & 3) || ((uintptr_t)row_scale & 7)) {
        set_error("%s: the workspace must be 16-byte aligned, the tensors 4-byte and the row scale 8-byte aligned", who);
        return RTOD_E_ARG;
    }
    const Plan& P = d.plan;
    const PackedConv& pc = d.conv();
    int v = P.default_tile(d.launch(), batch);
    if (tile != -1) {
        if (!P.tile_legal(d.launch(), tile)) { set_error("%s: tile %d is not a legal tile of this shape (rtod_conv_dgrad_split_tiles lists them)", who, tile); return RTOD_E_ARG; }
        v = tile;
    }
    char* ws = static_cast<char*>(workspace);
    float* amax = reinterpret_cast<float*>(ws + d.off_amax);
    float* scale = reinterpret_cast<float*>(ws + d.off_scale);
    double* rowmax = reinterpret_cast<double*>(ws + d.off_rowmax);
    float* image = reinterpret_cast<float*>(ws + d.off_image) - pc.w_off;      // the conv's block of a packed image, at the plan's offsets
    _Float16* dzs = reinterpret_cast<_Float16*>(ws + d.off_dz);
    float* raw = reinterpret_cast<float*>(ws + d.off_raw);
    _Float16* w_hi = reinterpret_cast<_Float16*>(image + pc.w_off);
    _Float16* w_lo = reinterpret_cast<_Float16*>(image + pc.wl_off);
    float* inv = image + pc.s_off;
    float* bias = image + pc.b_off;
    const int Kc = d.Kc, HW = d.HW, Npad = pc.Npad;
    const int64_t per_image = (int64_t)cout * HW;
    const dim3 block(DGS_THREADS);

    // (a) the images' exponents
    if (phases & DGS_AMAX) {
    if (per_image % 4 == 0 && ((uintptr_t)dz & 15) == 0) hipLaunchKernelGGL(dgs_amax_kernel<true>, dim3(d.parts, batch), block, 0, s, dz, per_image, d.parts, amax);
    else hipLaunchKernelGGL(dgs_amax_kernel<false>, dim3(d.parts, batch), block, 0, s, dz, per_image, d.parts, amax);
    if (int rc = hip_fail(hipGetLastError(), "conv_dgrad_split: amax launch")) return rc;
    hipLaunchKernelGGL(dgs_exponent_kernel, dim3(batch), dim3(64), 0, s, (const float*)amax, d.parts, batch, scale);
    if (int rc = hip_fail(hipGetLastError(), "conv_dgrad_split: exponent launch")) return rc;
    }
    // (b) dz -> split planes
    const dim3 tgrid((HW + DGS_PT - 1) / DGS_PT, Kc / DGS_CT, batch);
    if (!(phases & DGS_SPLIT)) {}
    else if (HW % 4 == 0 && ((uintptr_t)dz & 15) == 0) hipLaunchKernelGGL(dgs_split_dz_kernel<true>, tgrid, block, 0, s, dz, (const float*)scale, cout, Kc, HW, dzs);
    else hipLaunchKernelGGL(dgs_split_dz_kernel<false>, tgrid, block, 0, s, dz, (const float*)scale, cout, Kc, HW, dzs);
    if (int rc = hip_fail(hipGetLastError(), "conv_dgrad_split: split launch")) return rc;
    // (c) the weights
    const dim3 rgrid((cin + 63) / 64, d.wparts), pgrid(Npad / 32, Kc / 32);
#define RTOD_DGS_W(TAPS, SCALED)                                                                                                            \
    do {                                                                                                                                    \
        hipLaunchKernelGGL((dgs_rowmax_kernel<TAPS, SCALED>), rgrid, block, 0, s, w, row_scale, cout, cin, d.olen, rowmax);                 \
        if (int rc = hip_fail(hipGetLastError(), "conv_dgrad_split: row maximum launch")) return rc;                                        \
        hipLaunchKernelGGL((dgs_pack_w_kernel<TAPS, SCALED>), pgrid, block, 0, s, w, row_scale, (const double*)rowmax, d.wparts, cout, cin, \
                           Npad, w_hi, w_lo, inv, bias);                                                                                    \
    } while (0)
    if (!(phases & DGS_PACK)) {}
    else if (size == 3 && row_scale) RTOD_DGS_W(9, true);
    else if (size == 3) RTOD_DGS_W(9, false);
    else if (row_scale) RTOD_DGS_W(1, true);
    else RTOD_DGS_W(1, false);
#undef RTOD_DGS_W
    if (int rc = hip_fail(hipGetLastError(), "conv_dgrad_split: pack launch")) return rc;
    // the conv: a raw-sum launch of an existing tile
    ConvArgs a;
    a.in = reinterpret_cast<const float*>(dzs); a.in_ldc = Kc; a.in_coff = 0;
    a.B = batch; a.Hi = a.Ho = h; a.Wi = a.Wo = w_; a.Cin = Kc;
    a.bias = bias; a.K = pc.K; a.Kpad = pc.Kpad; a.Npad = Npad;
    a.kh = a.kw = size; a.stride = 1; a.pad = size / 2; a.Cout = cin; a.leaky = 0;
    a.out = raw; a.out_ldc = Npad;                                // required non-null by the launchers' common check; a raw-sum instance never writes it
    a.w_hi = w_hi; a.w_lo = w_lo; a.inv_scale = inv;
    a.in_bytes = (unsigned)(d.M * Kc * 4); a.w_bytes = (unsigned)((int64_t)Npad * pc.Kpad * 2);
    a.raw_out = raw; a.raw_ld = Npad;
    if (phases & DGS_CONV) if (int rc = P.launch_split_variant(a, pc, v, s)) return rc;
    if (!(phases & DGS_FINISH)) return RTOD_OK;
    // (d) the finish
    const dim3 fgrid((HW + DGS_PT - 1) / DGS_PT, cin / DGS_CT, batch);
    const bool vec = HW % 4 == 0 && ((uintptr_t)dx & 15) == 0 && ((uintptr_t)y & 15) == 0;
    if (vec) hipLaunchKernelGGL(dgs_finish_kernel<true>, fgrid, block, 0, s, (const float*)raw, Npad, (const float*)scale, batch, y, slope, cin, HW, dx);
    else hipLaunchKernelGGL(dgs_finish_kernel<false>, fgrid, block, 0, s, (const float*)raw, Npad, (const float*)scale, batch, y, slope, cin, HW, dx);
    return hip_fail(hipGetLastError(), "conv_dgrad_split: finish launch");
}

}  // namespace rtod
