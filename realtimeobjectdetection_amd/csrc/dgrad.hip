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
// inside it.  Then one multiplication by the mask.  Plain vector stores, no atomics: bit-identical from call to call.
//
// Stride 2 (rtod_conv_dgrad_s2): the data gradient of a 3x3 / stride 2 / pad 1 conv, h x w its INPUT map, ho = (h - 1) / 2 + 1.
//   dx[b][c][iy][ix] = m(y[b][c][iy][ix]) * sum over taps (ky, kx) with iy + 1 - ky and ix + 1 - kx even of
//                      chain_o v[o][c][ky][kx] * dz[b][o][(iy + 1 - ky) / 2][(ix + 1 - kx) / 2]
// The parities of (iy, ix) pick the taps: an even row takes ky = 1 alone, an odd row ky = 0 and 2, columns likewise: 1, 2, 2 or 4
// taps, nine per four pixels.  Stride 1's columns with a stride argument would stage zeros for the other 27 of 36.  So the GEMM
// columns are ordered by (class q = 2 * (iy & 1) + (ix & 1), b, iy / 2, ix / 2), every class is rounded up to whole 64-column tiles
// by itself, and a workgroup serves ONE class and loops over that class's taps alone, in ascending tap order.  Only ky = 0 / kx = 0
// can look past the map (iy = h - 1 odd reads row ho of dz): such a tap stages zeros and adds an exact +0.  A class may be empty
// (h == 1 has no odd row): it gets no tile.
// Memory: the dz loads of a stage are contiguous along ox (consecutive columns of a class are consecutive ox).  The dx stores and the
// y loads of a class are 8 bytes apart along x: a wave's store of one channel row covers 32 columns = 256 bytes of which it writes
// every other dword, and the class of the other column parity, in another workgroup, writes the rest.  That is at worst twice the
// write sectors of a dense store on a tensor the kernel touches once (Cin * h * w floats against 2 * 9 / 4 * Cout flops per
// element); pairing the two column classes in one workgroup would make the stores dense but give one wave 1 and 2 (or 2 and 4)
// taps to loop over, and the fixed tap order per element is what the entry promises.  Not avoided here.
//
// Thin convs (rtod_conv_dgrad_thin): any cin >= 1 through the same stride-1 instances.  Rows past cin are staged as zeros (c_ok) and
// never stored, so an element's chain, tap order and mask are those of the entries above; a 16-channel conv fills a quarter of the row
// tile's accumulators, which is accepted here (its cost is the dz staging, shared with a full tile).
//
// One body, three geometries.  dgrad_tile below is the whole recipe: staging, prefetch, MFMAs, total = total + chain, masked store.
// Its `if constexpr` arms hold only what differs between 1x1 pixels, 3x3 stride 1 and 3x3 stride 2 (one parity class per workgroup): how
// a GEMM column becomes a pixel, which taps that pixel has, which dz element a tap reads, where dx goes.
#include "rtod_internal.h"

namespace rtod {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int DG_BK = 32;               // k per LDS stage
constexpr int DG_T = 64;                // tile edge
constexpr int DG_LD = DG_T + 32;        // floats per k row

// the maps of a launch.  Stride 1: dz, y and dx live on height x width (size 1: 1 x pixels), N = batch * pixels columns.  Stride 2:
// height x width is the conv's INPUT map (y, dx), dz lives on ho x wo, tile_end[q] counts the column tiles of classes 0..q
struct DgradMaps { int batch, pixels, N, height, width, ho, wo; int tile_end[4]; };

// the 64 x 64 tile of workgroup bx: rows are channels, columns pixels (stride 2: the pixels of one parity class)
template <int SIZE, int STRIDE, bool SCALED>
__device__ __forceinline__ void dgrad_tile(int bx, const float* __restrict__ w, const float* __restrict__ dz, const float* __restrict__ y, float slope,
                                           int cout, int cin, int grid_n, float* __restrict__ dx, const double* scale, const DgradMaps g) {
    constexpr int TAPS = SIZE * SIZE;
    __shared__ float sA[DG_BK * DG_LD];
    __shared__ float sB[DG_BK * DG_LD];
    const int bm = bx / grid_n, bt = bx - bm * grid_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = tid & 63, ks = tid >> 6;                        // this thread stages row r at k = ks, ks + 4, ...
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 31, lh = lane >> 5;

    // the columns of this workgroup: tile bn of N columns, `pixels` per image, in rows of `width`; dz has dzpix pixels per channel
    int bn = bt, N = g.N, pixels = g.pixels, width = g.width, dzpix = g.pixels, ntaps = TAPS;
    [[maybe_unused]] int py = 0, px = 0;
    if constexpr (STRIDE == 2) {
        // the class of this workgroup (uniform): the number of classes whose tiles end at or before bt; an empty class is skipped
        const int q = (bt >= g.tile_end[0]) + (bt >= g.tile_end[1]) + (bt >= g.tile_end[2]);
        bn = bt - (q == 0 ? 0 : q == 1 ? g.tile_end[0] : q == 2 ? g.tile_end[1] : g.tile_end[2]);
        py = q >> 1, px = q & 1;
        width = (g.width + 1 - px) >> 1;                              // rows / columns of the map with that parity
        pixels = ((g.height + 1 - py) >> 1) * width;
        N = g.batch * pixels;
        dzpix = g.ho * g.wo;
        ntaps = (1 + py) * (1 + px);
    }

    // the staged rows: channel c of w, column n = (b, p) of dz
    const int sc = bm * DG_T + r;
    const int sn = bn * DG_T + r;
    const bool c_ok = sc < cin, n_ok = sn < N;
    const int sb = n_ok ? sn / pixels : 0;
    const int sp = n_ok ? sn - sb * pixels : 0;
    const int sy = SIZE == 1 ? 0 : sp / width, sx = SIZE == 1 ? 0 : sp - sy * width;   // stride 2: the staged pixel is (2 sy + py, 2 sx + px)
    const float* wcol = w + (int64_t)sc * TAPS;
    const float* dzrow = dz + (int64_t)sb * cout * dzpix + (STRIDE == 2 ? 0 : sp);

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float ra[DG_BK / 4], rb[DG_BK / 4];
    auto gload = [&](int t, int kc) {
        bool t_ok = n_ok;                                         // the pixel this column reads under tap step t lies inside the map
        int tap = t, shift = 0;                                   // the weight tap and the dz element of the step
        if constexpr (STRIDE == 2) {
            const int a = t / (1 + px), b = t - a * (1 + px);
            const int ky = py ? 2 * a : 1, kx = px ? 2 * b : 1;
            const int oy = sy + (ky == 0), ox = sx + (kx == 0);       // (iy + 1 - ky) / 2, (ix + 1 - kx) / 2
            t_ok = n_ok && oy < g.ho && ox < g.wo;
            tap = ky * 3 + kx;
            shift = oy * g.wo + ox;
        } else if constexpr (SIZE > 1) {
            const int ty = SIZE / 2 - t / SIZE, tx = SIZE / 2 - t % SIZE;
            t_ok = n_ok && (unsigned)(sy + ty) < (unsigned)g.height && (unsigned)(sx + tx) < (unsigned)width;
            shift = ty * width + tx;
        }
#pragma unroll
        for (int i = 0; i < DG_BK / 4; ++i) {
            const int o = kc + ks + 4 * i;
            ra[i] = (c_ok && o < cout) ? wcol[(int64_t)o * cin * TAPS + tap] : 0.f;
            if constexpr (SCALED) ra[i] = (float)((double)ra[i] * (o < cout ? scale[o] : 0.0));
            rb[i] = (t_ok && o < cout) ? dzrow[(int64_t)o * dzpix + shift] : 0.f;
        }
    };
    gload(0, 0);
    const float* pa = sA + lh * DG_LD + wm * 32 + lr;
    const float* pb = sB + lh * DG_LD + wn * 32 + lr;
    [[maybe_unused]] f32x16 total;                                    // 3x3: the sum of the finished taps (the 1x1 instances have none)
    if constexpr (SIZE > 1) total = acc;
#pragma unroll 1
    for (int t = 0; t < ntaps; ++t)
        for (int kc = 0; kc < cout; kc += DG_BK) {
            __syncthreads();                                          // the previous chunk's LDS reads are done
#pragma unroll
            for (int i = 0; i < DG_BK / 4; ++i) {
                sA[(ks + 4 * i) * DG_LD + r] = ra[i];
                sB[(ks + 4 * i) * DG_LD + r] = rb[i];
            }
            __syncthreads();
            if (kc + DG_BK < cout) gload(t, kc + DG_BK);              // in flight while the MFMAs below run
            else if (SIZE > 1 && t + 1 < ntaps) gload(t + 1, 0);
#pragma unroll
            for (int u = 0; u < DG_BK / 2; ++u)                       // lane half lh supplies k = 2 u + lh
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * u * DG_LD], pb[2 * u * DG_LD], acc, 0, 0, 0);
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
    int64_t pix = p, map = pixels;                                    // the dx element of the column inside a channel's map, and that map's size
    if constexpr (STRIDE == 2) {
        const int jy = p / width, jx = p - jy * width;
        pix = (int64_t)(2 * jy + py) * g.width + (2 * jx + px);
        map = (int64_t)g.height * g.width;
    }
    const bool masked = y != nullptr && slope != 1.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int c = bm * DG_T + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (c >= cin) continue;
        const int64_t idx = ((int64_t)b * cin + c) * map + pix;
        float v = acc[e];
        if (masked && !(y[idx] > 0.f)) v = v * slope;
        dx[idx] = v;
    }
}

template <int SIZE, int STRIDE, bool SCALED>
__global__ __launch_bounds__(256)
void dgrad_kernel(const float* __restrict__ w, const float* __restrict__ dz, const float* __restrict__ y, float slope, int cout, int cin, int grid_n,
                  float* __restrict__ dx, const double* scale, DgradMaps g) {
    dgrad_tile<SIZE, STRIDE, SCALED>(blockIdx.x, w, dz, y, slope, cout, cin, grid_n, dx, scale, g);
}

int launch_conv_dgrad(const char* who, const float* w, const double* row_scale, const float* dz, const float* y, float slope, int batch, int cout,
                      int cin, int h, int w_, int size, int stride, float* dx, hipStream_t s, bool any_cin) {
    const bool s2 = stride == 2;
    if (!w || !dz || !dx) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    if (any_cin && s2) { set_error("%s: stride 1 only", who); return RTOD_E_ARG; }
    if (batch < 1 || cout < 1 || cin < 1 || (!any_cin && cin % 32) || h < 1 || w_ < 1 || (size != 3 && (size != 1 || s2)) || (stride != 1 && !s2) || !(slope == slope)) {
        set_error("%s: unsupported arguments (batch=%d cout=%d cin=%d height=%d width=%d size=%d slope=%g; %ssize %s)",
                  who, batch, cout, cin, h, w_, size, (double)slope, any_cin ? "" : "cin must be a multiple of 32, ", s2 ? "3" : "1 or 3");
        return RTOD_E_ARG;
    }
    const int64_t N = (int64_t)batch * h * w_;
    if ((int64_t)h * w_ > INT32_MAX || N > INT32_MAX - 64 || (int64_t)cout * cin * size * size > INT32_MAX) {
        set_error("%s: batch * pixels or cout * cin * size * size exceeds int32", who);
        return RTOD_E_ARG;
    }
    DgradMaps g{batch, h * w_, (int)N, h, w_, (h - 1) / 2 + 1, (w_ - 1) / 2 + 1, {0, 0, 0, 0}};
    int64_t gn = 0;                                                   // column tiles
    if (s2) {
        for (int q = 0; q < 4; ++q) {                                 // the four classes one after the other, each in whole tiles
            const int64_t nq = (int64_t)batch * ((h + 1 - (q >> 1)) / 2) * ((w_ + 1 - (q & 1)) / 2);
            gn += (nq + DG_T - 1) / DG_T;
            g.tile_end[q] = (int)gn;                                  // <= N / 64 + 4
        }
    } else {
        gn = (N + DG_T - 1) / DG_T;
    }
    const int64_t gm = (cin + DG_T - 1) / DG_T;
    if (gm * gn > INT32_MAX) { set_error("%s: grid too large", who); return RTOD_E_ARG; }
    const dim3 grid((unsigned)(gm * gn)), block(256);
#define RTOD_DGRAD(SIZE, STRIDE, SCALED) hipLaunchKernelGGL((dgrad_kernel<SIZE, STRIDE, SCALED>), grid, block, 0, s, w, dz, y, slope, cout, cin, (int)gn, dx, row_scale, g)
    if (s2 && row_scale) RTOD_DGRAD(3, 2, true);
    else if (s2) RTOD_DGRAD(3, 2, false);
    else if (size == 1 && row_scale) RTOD_DGRAD(1, 1, true);
    else if (size == 1) RTOD_DGRAD(1, 1, false);
    else if (row_scale) RTOD_DGRAD(3, 1, true);
    else RTOD_DGRAD(3, 1, false);
#undef RTOD_DGRAD
    return hip_fail(hipGetLastError(), who);
}

}  // namespace rtod
