// Data gradient of a size x size (1 or 3), stride 1, pad size / 2 convolution z = V * y with the derivative of the activation that
// produced y fused, on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), gfx950:
//   dx[b][c][y][x] = m(y_in[b][c][y][x]) * sum_{ky,kx,o} v[o][c][ky][kx] * dz[b][o][y + pad - ky][x + pad - kx]
//   m(y) = 1 for y > 0, else slope   (torch's leaky_relu backward)        v = (float)((double)w * s[o]), or w without a row scale
// w [cout, cin, size, size] (OIHW: the float32 masters of a detection-head conv, or the raw masters of a BatchNorm conv with its
// frozen scale s, which gives the folded weight pack_conv computes), dz [batch, cout, h, w], y_in [batch, cin, h, w] the STORED
// output of the layer the conv reads (rtod_plan_read_layer): the sign of a leaky-ReLU's output is the sign of its input, so no
// pre-activation buffer is kept.  y == NULL or slope == 1: linear, no mask.  dz positions outside the map are exact zeros.
//
// GEMM view:  D[m][n] = sum_k A[m][k] * B[k][n],  m = c (MFMA rows), n = b * pixels + p (MFMA columns, on the lane: coalesced dx
// stores), k = tap * cout32 + o with tap = ky * size + kx and cout32 = cout rounded up to 32.  A is contiguous along c up to the
// tap stride, B along p: column n reads dz at the pixel shifted by the tap, so a thread stages one row index for eight k and LDS
// holds a K-chunk k-major, [32][64 + 32] floats per operand: a wave's ds_read_b32 of one k takes 32 consecutive floats per lane
// half and the halves (k, k + 1) sit 96 floats = 32 banks apart.  A chunk never straddles two taps, so the shift and the bounds
// test of a staged pixel are taken once per chunk; tiles cross row and image boundaries freely (every column has its own (b, y, x)).
// Workgroup: 4 waves, a 64 x 64 tile of dx, one 32 x 32 accumulator per wave; the next chunk's global loads are in flight during
// the MFMAs.  cout is ragged (255): rows past cout are staged as zeros, which leave an fmaf chain unchanged.  Size 1: every dx
// element is ONE fmaf chain over o in ascending pairs (o, o + 1).  Size 3: one such chain PER TAP, and the nine tap sums are added
// in ascending tap order with one fp32 add each (total = total + chain, in registers: no workspace, no second kernel).  One chain
// over all 9 * cout terms was measured first: at K = 4608 / 9216 its rounding error, about u sqrt(K) of the result, put dW of the
// convs behind it at 4.2 - 4.4 x the error of torch's blocked float32 sums, past the project's 4 x gate; chains of cout terms stay
// inside it.  Then one multiplication by the mask.  Plain vector stores, no atomics: bit-identical from call to call.  The size 1
// instance without a row scale is the kernel of rtod_conv1x1_dgrad as it was.
#include "rtod_internal.h"

namespace rtod {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int DG_BK = 32;               // k per LDS stage
constexpr int DG_T = 64;                // tile edge
constexpr int DG_LD = DG_T + 32;        // floats per k row

// what the instances other than <1, false> take behind the arguments of the 1x1 kernel: that instance keeps the old argument list, and
// with it the old code, register for register
struct DgradExtra { const double* scale; int height, width; };

template <int SIZE, bool SCALED, class... Extra>
__global__ __launch_bounds__(256)
void dgrad_kernel(const float* __restrict__ w, const float* __restrict__ dz, const float* __restrict__ y, float slope,
                  int cout, int cin, int pixels, int N, int grid_n, float* __restrict__ dx, Extra... extra) {
    [[maybe_unused]] const double* scale = nullptr;
    [[maybe_unused]] int height = 1, width = pixels;
    if constexpr (sizeof...(Extra) > 0) { const DgradExtra x = (extra, ...); scale = x.scale; height = x.height; width = x.width; }
    constexpr int TAPS = SIZE * SIZE;
    __shared__ float sA[DG_BK * DG_LD];
    __shared__ float sB[DG_BK * DG_LD];
    const int bm = blockIdx.x / grid_n, bn = blockIdx.x - bm * grid_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = tid & 63, ks = tid >> 6;                        // this thread stages row r at k = ks, ks + 4, ...
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, lh = lane >> 5;

    // the staged rows: channel c of w, position n = (b, p) of dz
    const int sc = bm * DG_T + r;
    const int sn = bn * DG_T + r;
    const bool c_ok = sc < cin, n_ok = sn < N;
    const int sb = n_ok ? sn / pixels : 0;
    const int sp = n_ok ? sn - sb * pixels : 0;
    const int sy = SIZE == 1 ? 0 : sp / width, sx = SIZE == 1 ? 0 : sp - sy * width;
    const float* wcol = w + (int64_t)sc * TAPS;
    const float* dzrow = dz + (int64_t)sb * cout * pixels + sp;

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float ra[DG_BK / 4], rb[DG_BK / 4];
    auto gload = [&](int tap, int kc) {
        bool t_ok = n_ok;                                         // the pixel this column reads under the tap lies inside the map
        int shift = 0;
        if constexpr (SIZE > 1) {
            const int ty = SIZE / 2 - tap / SIZE, tx = SIZE / 2 - tap % SIZE;
            t_ok = n_ok && (unsigned)(sy + ty) < (unsigned)height && (unsigned)(sx + tx) < (unsigned)width;
            shift = ty * width + tx;
        }
#pragma unroll
        for (int i = 0; i < DG_BK / 4; ++i) {
            const int o = kc + ks + 4 * i;
            ra[i] = (c_ok && o < cout) ? wcol[(int64_t)o * cin * TAPS + tap] : 0.f;
            if constexpr (SCALED) ra[i] = (float)((double)ra[i] * (o < cout ? scale[o] : 0.0));
            rb[i] = (t_ok && o < cout) ? dzrow[(int64_t)o * pixels + shift] : 0.f;
        }
    };
    gload(0, 0);
    const float* pa = sA + lh * DG_LD + wm * 32 + lr;
    const float* pb = sB + lh * DG_LD + wn * 32 + lr;
    [[maybe_unused]] f32x16 total;                                    // 3x3: the sum of the finished taps (the 1x1 instances have none)
    if constexpr (SIZE > 1) total = acc;
#pragma unroll 1
    for (int tap = 0; tap < TAPS; ++tap)
        for (int kc = 0; kc < cout; kc += DG_BK) {
            __syncthreads();                                          // the previous chunk's LDS reads are done
#pragma unroll
            for (int i = 0; i < DG_BK / 4; ++i) {
                sA[(ks + 4 * i) * DG_LD + r] = ra[i];
                sB[(ks + 4 * i) * DG_LD + r] = rb[i];
            }
            __syncthreads();
            if (kc + DG_BK < cout) gload(tap, kc + DG_BK);            // in flight while the MFMAs below run
            else if (SIZE > 1 && tap + 1 < TAPS) gload(tap + 1, 0);
#pragma unroll
            for (int t = 0; t < DG_BK / 2; ++t)                       // lane half lh supplies k = 2 t + lh
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * t * DG_LD], pb[2 * t * DG_LD], acc, 0, 0, 0);
            if constexpr (SIZE > 1)
                if (kc + DG_BK >= cout) {                             // the tap's chain joins the total: one fp32 add per tap, ascending
#pragma unroll
                    for (int e = 0; e < 16; ++e) { total[e] = total[e] + acc[e]; acc[e] = 0.f; }
                }
        }
    if constexpr (SIZE > 1) acc = total;
    // D: column = lane & 31 (n), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (c)
    const int n = bn * DG_T + wn * 32 + lr;
    if (n >= N) return;
    const int b = n / pixels, p = n - b * pixels;
    const bool masked = y != nullptr && slope != 1.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = bm * DG_T + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (c >= cin) continue;
        const int64_t idx = ((int64_t)b * cin + c) * pixels + p;
        float v = acc[e];
        if (masked && !(y[idx] > 0.f)) v = v * slope;
        dx[idx] = v;
    }
}

int launch_conv_dgrad(const char* who, const float* w, const double* row_scale, const float* dz, const float* y, float slope, int batch, int cout,
                      int cin, int h, int w_, int size, float* dx, hipStream_t s) {
    if (!w || !dz || !dx) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    if (batch < 1 || cout < 1 || cin < 32 || cin % 32 || h < 1 || w_ < 1 || (size != 1 && size != 3) || !(slope == slope)) {
        set_error("%s: unsupported arguments (batch=%d cout=%d cin=%d height=%d width=%d size=%d slope=%g; cin must be a multiple of 32, size 1 or 3)",
                  who, batch, cout, cin, h, w_, size, (double)slope);
        return RTOD_E_ARG;
    }
    const int64_t N = (int64_t)batch * h * w_;
    if ((int64_t)h * w_ > INT32_MAX || N > INT32_MAX - 64 || (int64_t)cout * cin * size * size > INT32_MAX) {
        set_error("%s: batch * pixels or cout * cin * size * size exceeds int32", who);
        return RTOD_E_ARG;
    }
    const int64_t gm = (cin + DG_T - 1) / DG_T, gn = (N + DG_T - 1) / DG_T;
    if (gm * gn > INT32_MAX) { set_error("%s: grid too large", who); return RTOD_E_ARG; }
    const dim3 grid((unsigned)(gm * gn)), block(256);
    const int pixels = h * w_;
    const DgradExtra x{row_scale, h, w_};
#define RTOD_DGRAD(SIZE, SCALED) hipLaunchKernelGGL((dgrad_kernel<SIZE, SCALED, DgradExtra>), grid, block, 0, s, w, dz, y, slope, cout, cin, pixels, (int)N, (int)gn, dx, x)
    if (size == 1 && !row_scale) hipLaunchKernelGGL((dgrad_kernel<1, false>), grid, block, 0, s, w, dz, y, slope, cout, cin, pixels, (int)N, (int)gn, dx);
    else if (size == 1) RTOD_DGRAD(1, true);
    else if (row_scale) RTOD_DGRAD(3, true);
    else RTOD_DGRAD(3, false);
#undef RTOD_DGRAD
    return hip_fail(hipGetLastError(), who);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Stride 2 (rtod_conv_dgrad_s2): the data gradient of a 3x3 / stride 2 / pad 1 conv, h x w its INPUT map, ho = (h - 1) / 2 + 1.
//   dx[b][c][iy][ix] = m(y[b][c][iy][ix]) * sum over taps (ky, kx) with iy + 1 - ky and ix + 1 - kx even of
//                      chain_o v[o][c][ky][kx] * dz[b][o][(iy + 1 - ky) / 2][(ix + 1 - kx) / 2]
// The parities of (iy, ix) pick the taps: an even row takes ky = 1 alone, an odd row ky = 0 and 2, columns likewise: 1, 2, 2 or 4
// taps, nine per four pixels.  The stride-1 kernel with a stride argument would stage zeros for the other 27 of 36.  So the GEMM
// columns are ordered by (class q = 2 * (iy & 1) + (ix & 1), b, iy / 2, ix / 2), every class is rounded up to whole 64-column tiles
// by itself, and a workgroup serves ONE class and loops over that class's taps alone, in ascending tap order.  The rest is the
// recipe above: 64 x 64 tiles, k-major LDS stages of 32, one fmaf chain per tap over o in ascending pairs, total = total + chain
// with one fp32 add per tap, one multiplication by the mask.  Only ky = 0 / kx = 0 can look past the map (iy = h - 1 odd reads row
// ho of dz): such a tap stages zeros and adds an exact +0.  A class may be empty (h == 1 has no odd row): it gets no tile.
// Memory: the dz loads of a stage are contiguous along ox (consecutive columns of a class are consecutive ox).  The dx stores and the
// y loads of a class are 8 bytes apart along x: a wave's store of one channel row covers 32 columns = 256 bytes of which it writes
// every other dword, and the class of the other column parity, in another workgroup, writes the rest.  That is at worst twice the
// write sectors of a dense store on a tensor the kernel touches once (Cin * h * w floats against 2 * 9 / 4 * Cout flops per
// element); pairing the two column classes in one workgroup would make the stores dense but give one wave 1 and 2 (or 2 and 4)
// taps to loop over, and the fixed tap order per element is what the entry promises.  Not avoided here.
struct DgradS2 { const double* scale; int batch, h, w, ho, wo; int tile_end[4]; };   // tile_end[q]: tiles of classes 0..q

template <bool SCALED>
__global__ __launch_bounds__(256)
void dgrad_s2_kernel(const float* __restrict__ w, const float* __restrict__ dz, const float* __restrict__ y, float slope,
                     int cout, int cin, int grid_n, float* __restrict__ dx, DgradS2 g) {
    __shared__ float sA[DG_BK * DG_LD];
    __shared__ float sB[DG_BK * DG_LD];
    const int bm = blockIdx.x / grid_n, bt = blockIdx.x - bm * grid_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = tid & 63, ks = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, lh = lane >> 5;

    // the class of this workgroup (uniform): the number of classes whose tiles end at or before bt; an empty class is skipped
    const int q = (bt >= g.tile_end[0]) + (bt >= g.tile_end[1]) + (bt >= g.tile_end[2]);
    const int t0 = q == 0 ? 0 : q == 1 ? g.tile_end[0] : q == 2 ? g.tile_end[1] : g.tile_end[2];
    const int py = q >> 1, px = q & 1;
    const int hq = (g.h + 1 - py) >> 1, wq = (g.w + 1 - px) >> 1;     // rows / columns of the map with that parity
    const int pq = hq * wq, nq = g.batch * pq;
    const int nkx = 1 + px, ntaps = (1 + py) * nkx;
    const int dzpix = g.ho * g.wo;

    const int sc = bm * DG_T + r;
    const int sn = (bt - t0) * DG_T + r;
    const bool c_ok = sc < cin, n_ok = sn < nq;
    const int sb = n_ok ? sn / pq : 0;
    const int sp = n_ok ? sn - sb * pq : 0;
    const int sjy = sp / wq, sjx = sp - sjy * wq;                     // the staged pixel is (2 sjy + py, 2 sjx + px)
    const float* wcol = w + (int64_t)sc * 9;
    const float* dzimg = dz + (int64_t)sb * cout * dzpix;

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float ra[DG_BK / 4], rb[DG_BK / 4];
    auto gload = [&](int t, int kc) {
        const int a = t / nkx, b = t - a * nkx;
        const int ky = py ? 2 * a : 1, kx = px ? 2 * b : 1;
        const int oy = sjy + (ky == 0), ox = sjx + (kx == 0);         // (iy + 1 - ky) / 2, (ix + 1 - kx) / 2
        const bool t_ok = n_ok && oy < g.ho && ox < g.wo;
        const int tap = ky * 3 + kx, off = oy * g.wo + ox;
#pragma unroll
        for (int i = 0; i < DG_BK / 4; ++i) {
            const int o = kc + ks + 4 * i;
            ra[i] = (c_ok && o < cout) ? wcol[(int64_t)o * cin * 9 + tap] : 0.f;
            if constexpr (SCALED) ra[i] = (float)((double)ra[i] * (o < cout ? g.scale[o] : 0.0));
            rb[i] = (t_ok && o < cout) ? dzimg[(int64_t)o * dzpix + off] : 0.f;
        }
    };
    gload(0, 0);
    const float* pa = sA + lh * DG_LD + wm * 32 + lr;
    const float* pb = sB + lh * DG_LD + wn * 32 + lr;
    f32x16 total = acc;
#pragma unroll 1
    for (int t = 0; t < ntaps; ++t)
        for (int kc = 0; kc < cout; kc += DG_BK) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < DG_BK / 4; ++i) {
                sA[(ks + 4 * i) * DG_LD + r] = ra[i];
                sB[(ks + 4 * i) * DG_LD + r] = rb[i];
            }
            __syncthreads();
            if (kc + DG_BK < cout) gload(t, kc + DG_BK);
            else if (t + 1 < ntaps) gload(t + 1, 0);
#pragma unroll
            for (int u = 0; u < DG_BK / 2; ++u)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * u * DG_LD], pb[2 * u * DG_LD], acc, 0, 0, 0);
            if (kc + DG_BK >= cout) {
#pragma unroll
                for (int e = 0; e < 16; ++e) { total[e] = total[e] + acc[e]; acc[e] = 0.f; }
            }
        }
    const int n = (bt - t0) * DG_T + wn * 32 + lr;
    if (n >= nq) return;
    const int b = n / pq, p = n - b * pq;
    const int jy = p / wq, jx = p - jy * wq;
    const int64_t pix = (int64_t)(2 * jy + py) * g.w + (2 * jx + px);
    const int64_t map = (int64_t)g.h * g.w;
    const bool masked = y != nullptr && slope != 1.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = bm * DG_T + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (c >= cin) continue;
        const int64_t idx = ((int64_t)b * cin + c) * map + pix;
        float v = total[e];
        if (masked && !(y[idx] > 0.f)) v = v * slope;
        dx[idx] = v;
    }
}

int launch_conv_dgrad_s2(const float* w, const double* row_scale, const float* dz, const float* y, float slope, int batch, int cout, int cin,
                         int h, int w_, int size, float* dx, hipStream_t s) {
    const char* who = "conv_dgrad_s2";
    if (!w || !dz || !dx) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    if (batch < 1 || cout < 1 || cin < 32 || cin % 32 || h < 1 || w_ < 1 || size != 3 || !(slope == slope)) {
        set_error("%s: unsupported arguments (batch=%d cout=%d cin=%d height=%d width=%d size=%d slope=%g; cin must be a multiple of 32, size 3)",
                  who, batch, cout, cin, h, w_, size, (double)slope);
        return RTOD_E_ARG;
    }
    const int64_t N = (int64_t)batch * h * w_;
    if ((int64_t)h * w_ > INT32_MAX || N > INT32_MAX - 64 || (int64_t)cout * cin * 9 > INT32_MAX) {
        set_error("%s: batch * pixels or cout * cin * size * size exceeds int32", who);
        return RTOD_E_ARG;
    }
    DgradS2 g{row_scale, batch, h, w_, (h - 1) / 2 + 1, (w_ - 1) / 2 + 1, {0, 0, 0, 0}};
    int64_t tiles = 0;
    for (int q = 0; q < 4; ++q) {
        const int64_t nq = (int64_t)batch * ((h + 1 - (q >> 1)) / 2) * ((w_ + 1 - (q & 1)) / 2);
        tiles += (nq + DG_T - 1) / DG_T;
        g.tile_end[q] = (int)tiles;                                   // <= N / 64 + 4
    }
    const int64_t gm = (cin + DG_T - 1) / DG_T;
    if (gm * tiles > INT32_MAX) { set_error("%s: grid too large", who); return RTOD_E_ARG; }
    const dim3 grid((unsigned)(gm * tiles)), block(256);
    if (row_scale) hipLaunchKernelGGL(dgrad_s2_kernel<true>, grid, block, 0, s, w, dz, y, slope, cout, cin, (int)tiles, dx, g);
    else hipLaunchKernelGGL(dgrad_s2_kernel<false>, grid, block, 0, s, w, dz, y, slope, cout, cin, (int)tiles, dx, g);
    return hip_fail(hipGetLastError(), who);
}

}  // namespace rtod
