// Weight gradient of a size x size (1 or 3), stride 1, same-padding BatchNorm convolution as three f16 MFMA products (opt-in:
// rtod_conv_wgrad_split; the exact entry is rtod_conv_wgrad, wgrad.hip), gfx950.
//   dW[o][c][ky][kx] = row_scale[o] * sum_{b,y,x} dz[b,o,y,x] * x[b,c,y+ky-p,x+kx-p]          x an exact zero outside the map
// The arithmetic (rtod.h states it; tests/wgrad_split_cases.py is its float64 model), free of any summation order:
//   exponents  ONE per tensor (dW sums over the batch): a = max |t|, e = 13 - frexp(a).exp so that a 2^e lies in [2^12, 2^13); a == 0
//              or not finite: e = 0; e held to -126 .. 126 (the rule of dgs_exponent_kernel, dgrad_split.hip).
//   split      v = t 2^e (exact), hi = RNE_f16(v), lo = RNE_f16(v - hi), subnormal halves kept.
//   sum        zh*xh + zh*xl + zl*xh over all (b, y, x) in fp32 on v_mfma_f32_32x32x16_f16; zl*xl is absent by definition.
//   finish     dW = (float)((double)sum * 2^-(e_z + e_x) * row_scale[o]): the power of two is exact, one rounding in double.
//
// Four kernel groups on the caller's stream, no atomics, nothing synchronises:
//   (a) wgs_amax_kernel + wgs_exponent_kernel: the two maxima (order-independent) -> 2^e_z, 2^e_x as floats and -(e_z + e_x) as an int.
//   (b) wgs_split_kernel: NCHW fp32 -> channel-major, k-contiguous f16 hi and lo planes (rows of `pitch` halves, stored in blocks of 32
//       rows with their 16-byte pieces interleaved: see the kernel), ONE launch for dz and x, which share
//       a COMMON PADDED k GRID so that eight consecutive k are eight consecutive halves of both operands for every tap:
//         size 3: the grid is [B][H + 2][Wp], Wp = 8 * ceil((W + 2) / 8); pixel (y, x) sits at (y + 1, x + 1); halo rows and columns are
//                 written as zeros, in dz too (a zero dz half times the x half beside it is what makes the halo k contribute nothing), and
//                 tap (ky, kx) of x is the same plane read at k + (ky - 1) * Wp + (kx - 1): no bounds test, the row shifts 16-byte aligned.
//         size 1: the flat k = b * HW + p.
//       Kg (the grid) is rounded up to Kpad, a multiple of the k step 16, with zeros; every plane carries a zero guard of G = Wp + 8 halves
//       in front and behind (size 1: none).  The kernel writes EVERY half of every plane: guards, halo and tail included.
//   (c) wgs_gemm_kernel: a workgroup of 4 waves (2 x 2) owns TM filters x TN channels x ALL taps of dW over one K slice; a wave holds
//       MI x NI x taps 32 x 32 accumulators (3x3: 64 x 64 x 9, nine accumulators per wave in AGPRs; 1x1: 128 x 128, four per wave).  Per k step
//       of 16 a lane loads its MFMA fragments straight from the planes in operand order (lane l: row l & 31, halves k + 8 * (l >> 5) ..
//       + 7, one 16-byte load, 512 contiguous bytes per lane half thanks to the interleaved rows: with plain row-major planes every lane
//       of a load sat in another cache line, a step touched more lines than the L1 holds, and the GEMM ran at half this rate; rocm's A/B
//       map of the 32x32x16 shape): dz hi / lo once, and the three row windows of x once for all nine
//       taps.  The kx = 0 / 2 operands are formed in registers from the aligned 16 bytes and the dword in front / behind (shifts by 16
//       bits: v_alignbit; the inner dword comes from the other lane half by one exchange), so x is not stored three times.  No LDS:
//       each x fragment is used by 9 and each dz fragment by 27 MFMAs of its own wave (3x3: 14 loads per 27 MFMAs), and the two
//       waves that share it hit the same L1 lines; the next step's loads are in flight under the current step's MFMAs.  Rows past
//       cout / cin read the last valid row (their results are not stored).  K slices: wgrad_schedule's idea over Kpad in units of 16,
//       at most WGS_MAX_SLICES = 64 (a tile holds all nine taps, so the tile grid is nine times smaller than the exact kernel's and a
//       64 x 32 layer at 208 x 208 is ONE tile), fewer once the tile grid alone reaches a thousand workgroups, none shorter than
//       WGS_MIN_SLICE unless K is; a pure function of the shape.
//   (d) wgs_reduce_kernel: the slice sums added in ascending order, then the one multiplication in double.
// Every byte of the workspace that a kernel reads is written earlier in the same call.
#include "conv_f16s3_common.h"

#include <cmath>

namespace rtod {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WGS_THREADS = 256;
constexpr int WGS_MAX_PARTS = 256;       // partial maxima per tensor: one workgroup of wgs_exponent_kernel reads them
constexpr int WGS_STEP = 16;             // k per MFMA
constexpr int WGS_MIN_SLICE = 64;        // a small K is not cut into slivers
constexpr int WGS_MAX_SLICES = 64;       // the exact kernel's cap is 16, but its tile grid is nine times larger on a 3x3 layer: a tile here holds all nine taps

// ---- (a) max |t| of both tensors: blockIdx.y = 0 dz, 1 x; `parts` workgroups each over an interleaved share
__global__ __launch_bounds__(WGS_THREADS)
void wgs_amax_kernel(const float* __restrict__ dz, int64_t n_dz, int parts_dz, const float* __restrict__ x, int64_t n_x, int parts_x,
                     float* __restrict__ partial) {
    __shared__ float red[WGS_THREADS / 64];
    const int t = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const int parts = t ? parts_x : parts_dz;
    if (part >= parts) return;
    const float* p = t ? x : dz;
    const int64_t n = t ? n_x : n_dz;
    float m = 0.f;
    for (int64_t i = (int64_t)part * WGS_THREADS + tid; i < n; i += (int64_t)parts * WGS_THREADS) m = fmaxf(m, fabsf(p[i]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) partial[t * WGS_MAX_PARTS + part] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// ... to scale[0] = 2^e_z, scale[1] = 2^e_x and, behind them, the int -(e_z + e_x).  One workgroup
__global__ __launch_bounds__(WGS_THREADS)
void wgs_exponent_kernel(const float* __restrict__ partial, int parts_dz, int parts_x, float* __restrict__ scale) {
    __shared__ float red[2][WGS_THREADS / 64];
    const int tid = threadIdx.x;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        float m = tid < (t ? parts_x : parts_dz) ? partial[t * WGS_MAX_PARTS + tid] : 0.f;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        if ((tid & 63) == 0) red[t][tid >> 6] = m;
    }
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float m = fmaxf(fmaxf(red[t][0], red[t][1]), fmaxf(red[t][2], red[t][3]));
            int e = 0;
            if (m > 0.f && m < __builtin_huge_valf()) { int ex; (void)frexpf(m, &ex); e = 13 - ex; }     // m * 2^e in [2^12, 2^13)
            e = e < -126 ? -126 : e > 126 ? 126 : e;
            scale[t] = ldexpf(1.0f, e);
            sum += e;
        }
        reinterpret_cast<int*>(scale)[2] = -sum;
    }
}

// ---- (b) both tensors -> split planes.  A plane is stored in blocks of 32 rows, the 16-byte pieces of a block's rows interleaved:
// halves k .. k + 7 (k % 8 == 0, counted from the start of the padded row) of row 32 q + r live at ((q * pitch / 8 + k / 8) * 32 + r) * 8,
// so the 32 lanes of an MFMA operand load read 512 contiguous bytes.  hi planes of all blocks first, then the lo planes (`lo` halves on).
// grid (ceil(pitch / 8 / 8), row blocks of dz + row blocks of x): a workgroup writes 8 pieces of 32 rows; a thread reads 8
// consecutive floats of one channel and writes one piece of hi and lo.  Piece g covers grid positions j = 8 g - G .. + 7
template <int SIZE>
__global__ __launch_bounds__(WGS_THREADS)
void wgs_split_kernel(const float* __restrict__ dz, const float* __restrict__ x, const float* __restrict__ scale, int batch, int cout, int cin,
                      int H, int W, int Wp, int G, int Kg, int pitch, _Float16* __restrict__ zs, int64_t lo_z, _Float16* __restrict__ xs, int64_t lo_x) {
    const int g = blockIdx.x * 8 + (threadIdx.x >> 5), r = threadIdx.x & 31;
    const int zblocks = (cout + 31) / 32;
    const bool isx = (int)blockIdx.y >= zblocks;
    const int q = isx ? blockIdx.y - zblocks : blockIdx.y, C_ = isx ? cin : cout, ch = q * 32 + r;
    if (g >= pitch / 8 || ch >= C_) return;                           // rows past cout are never read: the GEMM reads row cout - 1 in their place
    const float* t = isx ? x : dz;
    const float up = scale[isx ? 1 : 0];
    const int j = g * 8 - G;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (j >= 0 && j < Kg) {
        if constexpr (SIZE == 3) {                                    // Wp % 8 == 0: the eight positions lie in one grid row
            const int row = j / Wp, xx0 = j - row * Wp;
            const int b = row / (H + 2), yy = row - b * (H + 2);
            if (yy >= 1 && yy <= H) {
                const float* src = t + (((int64_t)b * C_ + ch) * H + (yy - 1)) * W;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int xx = xx0 + e;
                    if (xx >= 1 && xx <= W) v[e] = src[xx - 1];
                }
            }
        } else {
            const int HW = H * W;
            int b = j / HW, p = j - b * HW;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (j + e < Kg) v[e] = t[((int64_t)b * C_ + ch) * HW + p];
                if (++p == HW) { p = 0; ++b; }
            }
        }
    }
    f16x8 h, l;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float s = v[e] * up;                                    // exact: |s| < 2^13
        const _Float16 hh = (_Float16)s;
        h[e] = hh; l[e] = (_Float16)(s - (float)hh);
    }
    _Float16* o = (isx ? xs : zs) + (((int64_t)q * (pitch / 8) + g) * 32 + r) * 8;
    *reinterpret_cast<f16x8*>(o) = h;
    *reinterpret_cast<f16x8*>(o + (isx ? lo_x : lo_z)) = l;
}

// ---- (c) the GEMM.  part: [S][cout][cin][TAPS] slice sums (OIHW).  grid: slices * grid_m * grid_n workgroups
template <int TAPS, int MI, int NI>
__global__ __launch_bounds__(WGS_THREADS)
void wgs_gemm_kernel(const _Float16* __restrict__ zs, int64_t lo_z, const _Float16* __restrict__ xs, int64_t lo_x, int cout, int cin, int pitch, int G,
                     int Wp, int Kpad, int slice_len, int grid_m, int grid_n, float* __restrict__ part) {
    constexpr int R = TAPS == 9 ? 3 : 1;                              // row windows of x per step
    constexpr int TM = 64 * MI, TN = 64 * NI;
    const int tiles = grid_m * grid_n;
    const int slice = blockIdx.x / tiles;
    const int tile = blockIdx.x - slice * tiles;
    const int bm = tile / grid_n, bn = tile - bm * grid_n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int k0 = slice * slice_len, k1 = min(k0 + slice_len, Kpad);

    const _Float16* pz[MI];
    const _Float16* px[NI];
    // a lane's piece of step k: row `row` (block row / 32, place row % 32), piece (G + k) / 8 + lh; a step moves on by 2 pieces = 512 halves
    auto piece = [&](const _Float16* plane, int row) { return plane + (((int64_t)(row >> 5) * (pitch / 8) + G / 8 + lh) * 32 + (row & 31)) * 8; };
#pragma unroll
    for (int i = 0; i < MI; ++i) pz[i] = piece(zs, min(bm * TM + (wm * MI + i) * 32 + lr, cout - 1));
#pragma unroll
    for (int j = 0; j < NI; ++j) px[j] = piece(xs, min(bn * TN + (wn * NI + j) * 32 + lr, cin - 1));
    const int row_shift = Wp * 32;                                    // one grid row: Wp / 8 pieces of 256 halves

    f32x16 acc[MI][NI][TAPS];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int t = 0; t < TAPS; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][t][e] = 0.f;

    struct Frag {
        f16x8 zh[MI], zl[MI];
        u32x4 xh[NI][R], xl[NI][R];
        unsigned hs[NI][R], ls[NI][R];                                // TAPS == 9: the dword in front of (lane half 0) / behind (half 1) the wave's 32 halves
    };
    auto load = [&](Frag& f, int k) {
        const int64_t at = (int64_t)k * 32;                           // k / 8 pieces of 256 halves
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            f.zh[i] = *reinterpret_cast<const f16x8*>(pz[i] + at);
            f.zl[i] = *reinterpret_cast<const f16x8*>(pz[i] + lo_z + at);
        }
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const _Float16* p = px[j] + at + (R == 3 ? (r - 1) * row_shift : 0);
                f.xh[j][r] = *reinterpret_cast<const u32x4*>(p);
                f.xl[j][r] = *reinterpret_cast<const u32x4*>(p + lo_x);
                if constexpr (TAPS == 9) {                            // the first dword of the next piece of the row, or the last of the one before
                    f.hs[j][r] = *reinterpret_cast<const unsigned*>(p + (lh ? 256 : -256 + 6));
                    f.ls[j][r] = *reinterpret_cast<const unsigned*>(p + lo_x + (lh ? 256 : -256 + 6));
                }
            }
    };
    // The dword in front of and behind a lane's 16 bytes.  The two lane halves hold neighbouring 16 bytes of one row, so half 0 takes
    // the dword behind from its partner's first dword and half 1 the dword in front from its partner's last: one exchange across the
    // wave halves, and only the outer dword of each half is loaded (side)
    auto beside = [&](const u32x4& d, unsigned side, unsigned& m, unsigned& p) {
        const unsigned got = __shfl_xor(lh ? d[0] : d[3], 32);
        m = lh ? got : side;
        p = lh ? side : got;
    };
    // the window shifted by kx - 1 halves: little-endian, half 2 i is the low half of dword i
    auto window = [](unsigned m, const u32x4& d, unsigned p, int kx) -> f16x8 {
        u32x4 w = d;
        if (kx == 0) { w[0] = (m >> 16) | (d[0] << 16); w[1] = (d[0] >> 16) | (d[1] << 16); w[2] = (d[1] >> 16) | (d[2] << 16); w[3] = (d[2] >> 16) | (d[3] << 16); }
        if (kx == 2) { w[0] = (d[0] >> 16) | (d[1] << 16); w[1] = (d[1] >> 16) | (d[2] << 16); w[2] = (d[2] >> 16) | (d[3] << 16); w[3] = (d[3] >> 16) | (p << 16); }
        return __builtin_bit_cast(f16x8, w);
    };
    auto compute = [&](const Frag& f) {
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                unsigned hm = 0u, hp = 0u, lm = 0u, lp = 0u;
                if constexpr (TAPS == 9) { beside(f.xh[j][r], f.hs[j][r], hm, hp); beside(f.xl[j][r], f.ls[j][r], lm, lp); }
#pragma unroll
                for (int kx = 0; kx < R; ++kx) {
                    const f16x8 bh = window(hm, f.xh[j][r], hp, R == 3 ? kx : 1);
                    const f16x8 bl = window(lm, f.xl[j][r], lp, R == 3 ? kx : 1);
#pragma unroll
                    for (int i = 0; i < MI; ++i) {
                        f32x16& a = acc[i][j][r * R + kx];
                        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.zh[i], bh, a, 0, 0, 0);
                        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.zh[i], bl, a, 0, 0, 0);
                        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.zl[i], bh, a, 0, 0, 0);
                    }
                }
            }
    };

    Frag cur, nxt;
    if (k0 < k1) load(cur, k0);
    for (int k = k0; k < k1; k += WGS_STEP) {
        const bool more = k + WGS_STEP < k1;
        if (more) load(nxt, k + WGS_STEP);                            // in flight while the MFMAs below run
        compute(cur);
        if (more) cur = nxt;
    }

    // D: column = lane & 31 (c), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (o)
    float* out = part + (int64_t)slice * cout * cin * TAPS;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int c = bn * TN + (wn * NI + j) * 32 + lr;
            if (c >= cin) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int o = bm * TM + (wm * MI + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (o >= cout) continue;
                float* q = out + ((int64_t)o * cin + c) * TAPS;
#pragma unroll
                for (int t = 0; t < TAPS; ++t) q[t] = acc[i][j][t][e];
            }
        }
}

// ---- (d) the slice sums in ascending order, then (double)sum * (2^neg * row_scale[o]): the factor is exact, the product rounds once
__global__ __launch_bounds__(WGS_THREADS)
void wgs_reduce_kernel(const float* __restrict__ part, int64_t n_dw, int slices, int ncol, const float* __restrict__ scale,
                       const double* __restrict__ row_scale, float* __restrict__ dw) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_dw) return;
    float v = part[i];
    for (int s = 1; s < slices; ++s) v = v + part[(int64_t)s * n_dw + i];
    const double f = ldexp(1.0, reinterpret_cast<const int*>(scale)[2]);
    dw[i] = (float)((double)v * (row_scale ? f * row_scale[i / ncol] : f));
}

// ---- host.  The one description the workspace entry, the schedule entry, the bounds entry and the launcher read; nothing here touches a device
struct WgsDesc {
    int taps = 1, Wp = 0, G = 0;           // size 3: the padded row and the guard (halves); size 1: 0
    int Kg = 0, Kpad = 0, pitch = 0;       // the k grid, rounded up to the step, and a plane with its guards (halves)
    int tm = 64, tn = 64, gm = 1, gn = 1;  // the tile of dW and the tile grid
    int slices = 1, slice_len = WGS_STEP;
    int parts_dz = 1, parts_x = 1;
    int64_t n_dz = 0, n_x = 0, n_dw = 0, lo_z = 0, lo_x = 0;           // lo_*: halves from a hi plane to its lo plane
    size_t off_amax = 0, off_scale = 0, off_z = 0, off_x = 0, off_part = 0, bytes = 0;
};

static int wgs_describe(const char* who, int batch, int cout, int cin, int h, int w, int size, WgsDesc& d) {
    if (batch < 1 || cout < 1 || cin < 32 || cin % 32 || h < 1 || w < 1 || (size != 1 && size != 3)) {
        set_error("%s: unsupported shape (batch=%d cout=%d cin=%d height=%d width=%d size=%d; cin a positive multiple of 32, size 1 or 3)", who, batch, cout, cin, h, w, size);
        return RTOD_E_ARG;
    }
    d.taps = size * size;
    const int64_t Wp = size == 3 ? ((int64_t)w + 2 + 7) / 8 * 8 : 0, G = size == 3 ? Wp + 8 : 0;
    const int64_t Kg = size == 3 ? (int64_t)batch * (h + 2) * Wp : (int64_t)batch * h * w;
    const int64_t n_dw = (int64_t)cout * cin * d.taps;
    if (Kg > INT32_MAX - 64 || n_dw > INT32_MAX) { set_error("%s: the padded batch * height * width or cout * cin * size * size exceeds int32", who); return RTOD_E_ARG; }
    const int64_t Kpad = (Kg + WGS_STEP - 1) / WGS_STEP * WGS_STEP, pitch = G + Kpad + G;
    if (pitch * 2 >= (int64_t)OOB) { set_error("%s: a split plane would hold %lld bytes, 2 GiB or more", who, (long long)(pitch * 2)); return RTOD_E_ARG; }
    d.Wp = (int)Wp; d.G = (int)G; d.Kg = (int)Kg; d.Kpad = (int)Kpad; d.pitch = (int)pitch; d.n_dw = n_dw;
    d.tm = d.tn = size == 3 ? 64 : 128;                               // wgs_gemm_kernel<9, 1, 1> and <1, 2, 2>
    d.gm = (cout + d.tm - 1) / d.tm; d.gn = (cin + d.tn - 1) / d.tn;
    const int64_t tiles = (int64_t)d.gm * d.gn;
    // at most `want` slices, none shorter than WGS_MIN_SLICE: `want` grows with K and shrinks as the tile grid grows; the workspace holds
    // `want` slice sums (the count that runs, ceil(Kpad / L), can be a few below it)
    const int64_t cap = std::min<int64_t>(WGS_MAX_SLICES, (1024 + tiles - 1) / tiles), units = Kpad / WGS_STEP;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(cap, units / (WGS_MIN_SLICE / WGS_STEP)));
    const int64_t L = WGS_STEP * ((units + want - 1) / want);
    d.slice_len = (int)L;
    d.slices = (int)((Kpad + L - 1) / L);
    if (tiles * d.slices > INT32_MAX || (int64_t)cout + cin > 65535) { set_error("%s: grid too large", who); return RTOD_E_ARG; }
    d.n_dz = (int64_t)batch * cout * h * w; d.n_x = (int64_t)batch * cin * h * w;
    d.parts_dz = (int)std::max<int64_t>(1, std::min<int64_t>(WGS_MAX_PARTS, (d.n_dz + 16383) / 16384));
    d.parts_x = (int)std::max<int64_t>(1, std::min<int64_t>(WGS_MAX_PARTS, (d.n_x + 16383) / 16384));
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off += (n + 255) / 256 * 256; return at; };
    d.off_amax = take(sizeof(float) * 2 * WGS_MAX_PARTS);
    d.off_scale = take(sizeof(float) * 3);
    d.lo_z = ((int64_t)cout + 31) / 32 * 32 * pitch; d.lo_x = (int64_t)cin * pitch;      // the hi planes of all row blocks, then the lo planes
    d.off_z = take((size_t)d.lo_z * 2 * 2);
    d.off_x = take((size_t)d.lo_x * 2 * 2);
    d.off_part = take(sizeof(float) * (size_t)want * n_dw);
    d.bytes = off;
    return RTOD_OK;
}

// The lowest and the highest half index (from the start of a plane, guard included) that wgs_gemm_kernel forms for the description:
// lane half 0 of the first step of slice 0 at tap (0, 0), and lane half 1 of the last step of the last slice at tap (2, 2), each with
// the dword beside it.  Both must lie in [0, pitch): the halves wgs_split_kernel writes
static void wgs_half_range(const WgsDesc& d, int64_t* lowest, int64_t* highest) {
    const int64_t reach_lo = d.taps == 9 ? (int64_t)d.Wp + 2 : 0;                 // row above, and the dword in front
    const int64_t reach_hi = d.taps == 9 ? (int64_t)d.Wp + 8 + 1 : 7;             // row below, and the dword behind
    int64_t last_step = 0;
    for (int s = 0; s < d.slices; ++s) {
        const int64_t k0 = (int64_t)s * d.slice_len, k1 = std::min<int64_t>(k0 + d.slice_len, d.Kpad);
        if (k0 < k1) last_step = std::max(last_step, k0 + (k1 - k0 - 1) / WGS_STEP * WGS_STEP);
    }
    *lowest = d.G - reach_lo;
    *highest = d.G + last_step + 8 + reach_hi;
}

int conv_wgrad_split_schedule(int batch, int cout, int cin, int h, int w, int size, int* tiles, int* slices, int* slice_len, int64_t* k_padded) {
    const char* who = "conv_wgrad_split_schedule";
    if (!tiles || !slices || !slice_len || !k_padded) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    WgsDesc d;
    if (int rc = wgs_describe(who, batch, cout, cin, h, w, size, d)) return rc;
    *tiles = d.gm * d.gn; *slices = d.slices; *slice_len = d.slice_len; *k_padded = d.Kpad;
    return RTOD_OK;
}

int conv_wgrad_split_bounds(int batch, int cout, int cin, int h, int w, int size, int64_t* lowest, int64_t* highest, int64_t* plane_halves) {
    const char* who = "conv_wgrad_split_bounds";
    if (!lowest || !highest || !plane_halves) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    WgsDesc d;
    if (int rc = wgs_describe(who, batch, cout, cin, h, w, size, d)) return rc;
    wgs_half_range(d, lowest, highest);
    *plane_halves = d.pitch;
    return RTOD_OK;
}

int conv_wgrad_split_workspace(int batch, int cout, int cin, int h, int w, int size, size_t* bytes) {
    const char* who = "conv_wgrad_split_workspace";
    if (!bytes) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    WgsDesc d;
    if (int rc = wgs_describe(who, batch, cout, cin, h, w, size, d)) return rc;
    *bytes = d.bytes;
    return RTOD_OK;
}

int launch_conv_wgrad_split(const float* dz, const float* x, int batch, int cout, int cin, int h, int w, int size, const double* row_scale,
                            float* dw, void* workspace, size_t workspace_bytes, hipStream_t s, int phases) {
    const char* who = "conv_wgrad_split";
    if (phases < 1 || phases > WGS_ALL) { set_error("%s: phases %d outside 1 .. %d", who, phases, WGS_ALL); return RTOD_E_ARG; }
    if (!dz || !x || !dw || !workspace) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    WgsDesc d;
    if (int rc = wgs_describe(who, batch, cout, cin, h, w, size, d)) return rc;
    if (workspace_bytes < d.bytes) { set_error("%s: the workspace has %zu bytes, %zu are needed", who, workspace_bytes, d.bytes); return RTOD_E_ARG; }
    if (((uintptr_t)workspace & 15) || ((uintptr_t)dz & 3) || ((uintptr_t)x & 3) || ((uintptr_t)dw & 3) || ((uintptr_t)row_scale & 7)) {
        set_error("%s: the workspace must be 16-byte aligned, the tensors 4-byte and the row scale 8-byte aligned", who);
        return RTOD_E_ARG;
    }
    int64_t lo, hi;
    wgs_half_range(d, &lo, &hi);
    if (lo < 0 || hi >= d.pitch) { set_error("%s: internal: the GEMM would read halves %lld .. %lld of a plane of %d", who, (long long)lo, (long long)hi, d.pitch); return RTOD_E_ARG; }
    char* ws = static_cast<char*>(workspace);
    float* amax = reinterpret_cast<float*>(ws + d.off_amax);
    float* scale = reinterpret_cast<float*>(ws + d.off_scale);
    _Float16* zs = reinterpret_cast<_Float16*>(ws + d.off_z);
    _Float16* xs = reinterpret_cast<_Float16*>(ws + d.off_x);
    float* part = reinterpret_cast<float*>(ws + d.off_part);
    const dim3 block(WGS_THREADS);

    if (phases & WGS_EXPONENTS) {
        hipLaunchKernelGGL(wgs_amax_kernel, dim3(std::max(d.parts_dz, d.parts_x), 2), block, 0, s, dz, d.n_dz, d.parts_dz, x, d.n_x, d.parts_x, amax);
        if (int rc = hip_fail(hipGetLastError(), "conv_wgrad_split: amax launch")) return rc;
        hipLaunchKernelGGL(wgs_exponent_kernel, dim3(1), block, 0, s, (const float*)amax, d.parts_dz, d.parts_x, scale);
        if (int rc = hip_fail(hipGetLastError(), "conv_wgrad_split: exponent launch")) return rc;
    }
    if (phases & WGS_SPLIT) {
        const dim3 grid((d.pitch / 8 + 7) / 8, (cout + 31) / 32 + cin / 32);
        if (size == 3) hipLaunchKernelGGL(wgs_split_kernel<3>, grid, block, 0, s, dz, x, (const float*)scale, batch, cout, cin, h, w, d.Wp, d.G, d.Kg, d.pitch, zs, d.lo_z, xs, d.lo_x);
        else hipLaunchKernelGGL(wgs_split_kernel<1>, grid, block, 0, s, dz, x, (const float*)scale, batch, cout, cin, h, w, d.Wp, d.G, d.Kg, d.pitch, zs, d.lo_z, xs, d.lo_x);
        if (int rc = hip_fail(hipGetLastError(), "conv_wgrad_split: split launch")) return rc;
    }
    if (phases & WGS_GEMM) {
        const dim3 grid((unsigned)((int64_t)d.gm * d.gn * d.slices));
        if (size == 3) hipLaunchKernelGGL((wgs_gemm_kernel<9, 1, 1>), grid, block, 0, s, (const _Float16*)zs, d.lo_z, (const _Float16*)xs, d.lo_x, cout, cin, d.pitch, d.G, d.Wp, d.Kpad, d.slice_len, d.gm, d.gn, part);
        else hipLaunchKernelGGL((wgs_gemm_kernel<1, 2, 2>), grid, block, 0, s, (const _Float16*)zs, d.lo_z, (const _Float16*)xs, d.lo_x, cout, cin, d.pitch, d.G, d.Wp, d.Kpad, d.slice_len, d.gm, d.gn, part);
        if (int rc = hip_fail(hipGetLastError(), "conv_wgrad_split: GEMM launch")) return rc;
    }
    if (phases & WGS_REDUCE) {
        hipLaunchKernelGGL(wgs_reduce_kernel, dim3((unsigned)((d.n_dw + WGS_THREADS - 1) / WGS_THREADS)), block, 0, s, (const float*)part, d.n_dw, d.slices, cin * d.taps,
                           (const float*)scale, row_scale, dw);
        if (int rc = hip_fail(hipGetLastError(), "conv_wgrad_split: reduce launch")) return rc;
    }
    return RTOD_OK;
}

}  // namespace rtod
