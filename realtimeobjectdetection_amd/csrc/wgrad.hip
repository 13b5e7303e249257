// Weight and bias gradient of a 1x1 convolution on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), gfx950:
//   dW[o][c] = sum_{b,p} dz[b,o,p] * x[b,c,p]        db[o] = sum_{b,p} dz[b,o,p]
// dz [batch, cout, pixels] and x [batch, cin, pixels] are dense NCHW maps (the gradient of rtod_yolo_loss_grad for one head and
// rtod_plan_read_layer of the head conv's input).  An NT GEMM: both operands are contiguous along the summed index
// k = b * pixels + p inside an image, K = batch * pixels.
//
// GEMM view:  D[m][n] = sum_k A[m][k] * B[n][k],  m = o (MFMA rows), n = c (MFMA columns, on the lane: coalesced dW stores).
// Workgroup: 4 waves, a 64 x 64 tile of dW, one 32 x 32 accumulator per wave.  K-chunks of 32 are staged through LDS as
// [row][32 + 4] floats (conv_igemm_f32.hip's layout: one ds_read_b128 feeds four MFMAs; inside an 8-wide k group the lane halves
// take k = {0..3} and {4..7}), and the next chunk's global loads are in flight during the MFMAs.  Global loads are 4-byte loads
// with k on the lane: a row of an image starts on a 4-byte boundary only (pixels = 169), consecutive lanes read consecutive
// addresses inside an image, and a chunk may cross an image boundary.
// Rows past cout / cin and k past the slice are staged as zeros, which leave an fmaf chain unchanged.
//
// K slices.  The tile grid is small (4 x 16 tiles at most), so K is split into S contiguous slices, one workgroup per (tile,
// slice); slice sums go to the workspace and wgrad_reduce_kernel adds them in ascending slice order.  No floating-point atomics:
// the result is bit-identical from call to call.  The slice rule (wgrad_slice_len, documented in rtod.h) sees K and a cap:
//   units = ceil(K / 8);  slice length = 8 * ceil(units / cap);  S = ceil(K / slice length)  (<= cap; rtod_conv1x1_wgrad: cap = 16)
// Every accumulator is an fmaf chain over its slice in a fixed permutation of k; db is a plain fp32 sum over the slice in
// ascending k, kept by the workgroups of the first column of tiles.
//
// 3x3 convs (rtod_conv_wgrad, TAPS = 9).  The same kernel as an implicit GEMM: the column index is n = c * 9 + tap, OIHW order, so
// the dW stores stay coalesced, and B[n][k] = x[b, c, y + ky - 1, x + kx - 1], an exact zero outside the map.  A thread's eight
// columns (channel and tap offsets) do not depend on k and are resolved once; k -> (b, y, x) costs two divisions per staged chunk.
// Stride 2 (rtod_conv_wgrad_s2) is the same column with the tap positions doubled: k runs over the conv's OUTPUT map, x lives on
// its input map.  The 1x1 instance (TAPS = 1) reads x where it reads dz.  The cap of rtod_conv_wgrad also sees the
// number of tiles (wgrad_tile_cap: a 13 x 13 block has a thousand tiles already and is not sliced), and its reduce kernel
// multiplies the reduced sum of a row by a caller-supplied double once — the frozen BatchNorm scale of the conv.
#include "rtod_internal.h"

namespace rtod {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG_BK = 32;               // k per LDS stage
constexpr int WG_LD = WG_BK + 4;        // padded row (floats)
constexpr int WG_T = 64;                // tile edge (rows of dz and rows of x per workgroup)

// The slice rule (rtod.h): units = ceil(K / 8); slice length = 8 * ceil(units / cap); S = ceil(K / slice length) <= cap.  The two
// entries differ in the cap alone: rtod_conv1x1_wgrad always allows WGRAD_MAX_SLICES, rtod_conv_wgrad wgrad_tile_cap.
int64_t wgrad_slice_len(int64_t K, int cap) {
    const int64_t units = (K + 7) / 8;
    return 8 * ((units + cap - 1) / cap);
}
static int64_t wgrad_slices(int64_t K, int cap) { const int64_t L = wgrad_slice_len(K, cap); return (K + L - 1) / L; }
static int64_t wgrad_tiles(int cout, int cin, int size) {
    return (((int64_t)cout + WG_T - 1) / WG_T) * (((int64_t)cin * size * size + WG_T - 1) / WG_T);    // (the entries call this before their shape checks)
}
// min(16, ceil(1024 / tiles)): a grid that has a thousand tiles already is not sliced.  (No tiles: a shape wgrad_check_shape refuses.)
int wgrad_tile_cap(int cout, int cin, int size) {
    constexpr int64_t WG_TILE_TARGET = 1024;
    const int64_t tiles = wgrad_tiles(cout, cin, size);
    return tiles < 1 ? WGRAD_MAX_SLICES : (int)std::min<int64_t>(WGRAD_MAX_SLICES, (WG_TILE_TARGET + tiles - 1) / tiles);
}

size_t wgrad_workspace_bytes(int batch, int cout, int cin, int h, int w, int size, int cap) {
    const int64_t S = wgrad_slices((int64_t)batch * h * w, cap);
    return sizeof(float) * (size_t)S * ((size_t)cout * cin * size * size + (size_t)cout);
}

// part: [S][cout][ncol] slice sums of dW (ncol = cin * TAPS), then [S][cout] slice sums of db.  pixels and W describe the map of dz, the
// conv's OUTPUT, which k = (b, oy, ox) runs over; B[n][k] = x[b, c, STRIDE * oy + ky - 1, STRIDE * ox + kx - 1] on the xh x xw input
// map (stride 1: the same map), an exact zero outside it.  TAPS == 1: W, xh and xw are not read.
// TM x TN: the tile of dW (rows of dz x rows of x per workgroup), one 32 x 32 accumulator per wave, TM / 32 x TN / 32 = 4 waves: 64 x 64
// (waves 2 x 2) for the entries above, 32 x 128 (waves 1 x 4) for rtod_conv_wgrad_thin.  The arithmetic of an element does not depend on it
template <int TAPS, int STRIDE = 1, int TM = WG_T, int TN = WG_T>
__global__ __launch_bounds__(256)
void wgrad_slice_kernel(const float* __restrict__ dz, const float* __restrict__ x, int cout, int cin, int pixels, int W, int xh, int xw, int K, int slice_len,
                        int grid_m, int grid_n, float* __restrict__ part, float* __restrict__ part_db) {
    const int ncol = cin * TAPS;
    static_assert(TM % 32 == 0 && TN % 32 == 0 && (TM / 32) * (TN / 32) == 4, "four waves, one 32 x 32 accumulator each");
    __shared__ __attribute__((aligned(16))) float smem[(TM + TN) * WG_LD];
    float* sA = smem;
    float* sB = smem + TM * WG_LD;
    const int tiles = grid_m * grid_n;
    const int slice = blockIdx.x / tiles;
    const int tile = blockIdx.x - slice * tiles;
    const int bm = tile / grid_n, bn = tile - bm * grid_n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = tid & 31, row0 = tid >> 5;                     // this thread stages k = kk of rows row0, row0 + 8, ...
    const int k0 = slice * slice_len;
    const int k1 = min(k0 + slice_len, K);

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float db = 0.f;
    const int wm = wave / (TN / 32), wn = wave % (TN / 32);
    const int lr = lane & 31, lh = lane >> 5;
    const float* pa = sA + (wm * 32 + lr) * WG_LD + lh * 4;
    const float* pb = sB + (wn * 32 + lr) * WG_LD + lh * 4;

    // one register stage, as in conv_igemm_f32.hip: chunk kc + 1 is fetched while chunk kc computes
    float ra[TM / 8], rb[TN / 8];
    int col_c[TN / 8], col_dy[TN / 8], col_dx[TN / 8];      // TAPS > 1: channel and tap offsets of this thread's columns
    if (TAPS > 1) {
#pragma unroll
        for (int i = 0; i < TN / 8; ++i) {
            const int n = bn * TN + row0 + i * 8;
            const int tap = n % TAPS;
            col_c[i] = n / TAPS;
            col_dy[i] = tap / 3 - 1;
            col_dx[i] = tap % 3 - 1;
        }
    }
    auto gload = [&](int kc) {
        const int k = kc + kk;
        const bool kok = k < k1;
        const int b = kok ? k / pixels : 0;
        const int p = kok ? k - b * pixels : 0;
        const int py = TAPS > 1 ? p / W : 0;
        const int px = TAPS > 1 ? p - py * W : 0;
#pragma unroll
        for (int i = 0; i < TM / 8; ++i) {
            const int o = bm * TM + row0 + i * 8;
            ra[i] = (kok && o < cout) ? dz[((int64_t)b * cout + o) * pixels + p] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < TN / 8; ++i) {
            const int c = bn * TN + row0 + i * 8;
            if (TAPS == 1) {
                rb[i] = (kok && c < cin) ? x[((int64_t)b * cin + c) * pixels + p] : 0.f;
            } else {
                const int yy = STRIDE * py + col_dy[i], xx = STRIDE * px + col_dx[i];
                const bool in = kok && c < ncol && yy >= 0 && yy < xh && xx >= 0 && xx < xw;
                rb[i] = in ? x[((int64_t)b * cin + col_c[i]) * xh * xw + yy * xw + xx] : 0.f;
            }
        }
    };
    gload(k0);
    for (int kc = k0; kc < k1; kc += WG_BK) {
        __syncthreads();                                          // the previous chunk's LDS reads are done
#pragma unroll
        for (int i = 0; i < TM / 8; ++i) sA[(row0 + i * 8) * WG_LD + kk] = ra[i];
#pragma unroll
        for (int i = 0; i < TN / 8; ++i) sB[(row0 + i * 8) * WG_LD + kk] = rb[i];
        __syncthreads();
        if (kc + WG_BK < k1) gload(kc + WG_BK);                   // in flight while the MFMAs below run
#pragma unroll
        for (int q = 0; q < WG_BK / 8; ++q) {
            const f32x4 fa = *reinterpret_cast<const f32x4*>(pa + q * 8);
            const f32x4 fb = *reinterpret_cast<const f32x4*>(pb + q * 8);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], fb[s], acc, 0, 0, 0);
        }
        if (part_db && bn == 0 && tid < TM) {                     // uniform per wave: wave 0 alone
#pragma clang fp contract(off)
            const float* r = sA + tid * WG_LD;
            for (int j = 0; j < WG_BK; ++j) db = db + r[j];
        }
    }
    // D: column = lane & 31 (c), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (o)
    const int c = bn * TN + wn * 32 + lr;
    float* out = part + (int64_t)slice * cout * ncol;
    if (c < ncol) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int o = bm * TM + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (o < cout) out[(int64_t)o * ncol + c] = acc[e];
        }
    }
    if (part_db && bn == 0 && tid < TM) {
        const int o = bm * TM + tid;
        if (o < cout) part_db[(int64_t)slice * cout + o] = db;
    }
}

// the slice sums added in ascending slice order: one thread per element of dW, then of db.  row_scale (may be NULL): the reduced
// sum of row o of dW (ncol elements) times row_scale[o] in double, rounded once; db is the plain sum
__global__ __launch_bounds__(256)
void wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ part_db, int64_t n_dw, int cout, int slices,
                         const double* __restrict__ row_scale, int ncol, float* __restrict__ dw, float* __restrict__ db) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_dw) {
        float v = part[i];
        for (int s = 1; s < slices; ++s) v = v + part[(int64_t)s * n_dw + i];
        if (row_scale) v = (float)((double)v * row_scale[i / ncol]);
        dw[i] = v;
    } else if (db && i < n_dw + cout) {
        const int64_t o = i - n_dw;
        float v = part_db[o];
        for (int s = 1; s < slices; ++s) v = v + part_db[(int64_t)s * cout + o];
        db[o] = v;
    }
}

// stride 2 (h x w the conv's input map) takes size 3 alone
int wgrad_check_shape(const char* who, int batch, int cout, int cin, int h, int w, int size, int stride) {
    const int64_t K = (int64_t)batch * h * w, taps = (int64_t)size * size;
    if (batch < 1 || cout < 1 || cin < 32 || cin % 32 || h < 1 || w < 1 || (size != 1 && size != 3)) {
        set_error("%s: unsupported shape (batch=%d cout=%d cin=%d h=%d w=%d size=%d; cin must be a multiple of 32, size 1 or 3)", who, batch, cout, cin, h, w, size);
        return RTOD_E_ARG;
    }
    if ((int64_t)h * w > INT32_MAX || K > INT32_MAX - 64 || (int64_t)cout * cin * taps > INT32_MAX) { set_error("%s: batch * h * w or cout * cin * size * size exceeds int32", who); return RTOD_E_ARG; }
    if (stride == 2 && size != 3) { set_error("%s: unsupported shape (size=%d; the stride-2 entry takes 3x3 convs)", who, size); return RTOD_E_ARG; }
    return RTOD_OK;
}

// `who` names the entry in every error text; `cap` is the entry's cap on the slice count (at most WGRAD_MAX_SLICES).  stride 2
// (rtod_conv_wgrad_s2: size 3, pad 1): h x w is the conv's INPUT map, dz lives on the output map and K = batch * ho * wo
int launch_wgrad(const char* who, const float* dz, const float* x, int batch, int cout, int cin, int h, int w, int size, int cap,
                 const double* row_scale, float* dw, float* db, void* ws, size_t ws_bytes, hipStream_t s, int stride) {
    if (!dz || !x || !dw || !ws) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    if (int rc = wgrad_check_shape(who, batch, cout, cin, h, w, size, stride)) return rc;
    const int xh = h, xw = w;
    if (stride == 2) { h = (xh - 1) / 2 + 1; w = (xw - 1) / 2 + 1; }  // from here on the map that k runs over
    if (ws_bytes < wgrad_workspace_bytes(batch, cout, cin, h, w, size, cap)) { set_error("%s: workspace too small", who); return RTOD_E_ARG; }
    if ((uintptr_t)ws & 15) { set_error("%s: workspace must be 16-byte aligned", who); return RTOD_E_ARG; }
    const int pixels = h * w, ncol = cin * size * size;
    const int64_t K = (int64_t)batch * pixels, tiles = wgrad_tiles(cout, cin, size);
    const int S = (int)wgrad_slices(K, cap), L = (int)wgrad_slice_len(K, cap);
    const int gm = (cout + WG_T - 1) / WG_T, gn = (ncol + WG_T - 1) / WG_T;
    if (tiles * S > INT32_MAX) { set_error("%s: grid too large", who); return RTOD_E_ARG; }
    float* part = (float*)ws;
    float* part_db = part + (int64_t)S * cout * ncol;
    float* pdb = db ? part_db : (float*)nullptr;
#define RTOD_WGRAD(...) hipLaunchKernelGGL((wgrad_slice_kernel<__VA_ARGS__>), dim3((unsigned)(tiles * S)), dim3(256), 0, s, dz, x, cout, cin, pixels, w, xh, xw, (int)K, L, gm, gn, part, pdb)
    if (stride == 2) RTOD_WGRAD(9, 2);
    else if (size == 1) RTOD_WGRAD(1);
    else RTOD_WGRAD(9);
#undef RTOD_WGRAD
    const int64_t n = (int64_t)cout * ncol + (db ? cout : 0);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, part_db, (int64_t)cout * ncol, cout, S, row_scale, ncol, dw, db);
    return hip_fail(hipGetLastError(), (std::string(who) + " launch").c_str());
}

// ---------------------------------------------------------------------------------------------
// Thin convs (rtod_conv_wgrad_thin): few channels, a huge K — YOLOv3-tiny's layer 0 at 416 x 416 batch 8 is a 16 x 27 dW over
// K = 1,384,448.  The same slice kernel on a 32 x 128 tile (layer 0: one tile, layer 2's 32 x 144: two) with a slice count cut for K
// instead of capped at 16.  The slice rule (rtod.h, exported as rtod_conv_wgrad_thin_slices), a pure function of the shape:
//   tiles = ceil(cout / 32) * ceil(cin * size * size / 128);  target = ceil(1024 / tiles)
//   L = 8 * ceil(ceil(K / 8) / target), clamped to [WGRAD_THIN_MIN_CHAIN, WGRAD_THIN_MAX_CHAIN];  S = ceil(K / L)
// so a large K gets at least 1024 workgroups and no fmaf chain is longer than WGRAD_THIN_MAX_CHAIN = 1024 terms: the longest chain
// measured inside the 4 x gate (dgrad.hip's per-tap chain of a 1024-filter conv; one chain of 4608 / 9216 terms was measured outside).
// The S slice sums are added as a fixed two-level tree: groups of WGRAD_THIN_GROUP = 32 consecutive slices in ascending order, then the
// group sums in ascending order (S = 1352 at layer 0: the longest run of fp32 adds is 31 + 42, not 1351).
constexpr int WT_M = 32, WT_N = 128;

void wgrad_thin_slices(int64_t K, int cout, int cin, int size, int64_t* slices, int64_t* slice_len) {
    const int64_t tiles = (((int64_t)cout + WT_M - 1) / WT_M) * (((int64_t)cin * size * size + WT_N - 1) / WT_N);
    const int64_t target = tiles < 1 ? 1 : std::max<int64_t>(1, (1024 + tiles - 1) / tiles);
    int64_t L = 8 * (((K + 7) / 8 + target - 1) / target);
    L = std::min<int64_t>(WGRAD_THIN_MAX_CHAIN, std::max<int64_t>(WGRAD_THIN_MIN_CHAIN, L));
    *slice_len = L;
    *slices = (K + L - 1) / L;
}

int wgrad_thin_check_shape(const char* who, int batch, int cout, int cin, int h, int w, int size) {
    if (batch < 1 || cout < 1 || cin < 1 || h < 1 || w < 1 || (size != 1 && size != 3)) {
        set_error("%s: unsupported shape (batch=%d cout=%d cin=%d h=%d w=%d size=%d; size 1 or 3)", who, batch, cout, cin, h, w, size);
        return RTOD_E_ARG;
    }
    if ((int64_t)h * w > INT32_MAX || (int64_t)batch * h * w > INT32_MAX - WGRAD_THIN_MAX_CHAIN || (int64_t)cout * cin * size * size > INT32_MAX) {
        set_error("%s: batch * h * w or cout * cin * size * size exceeds int32", who);
        return RTOD_E_ARG;
    }
    return RTOD_OK;
}

size_t wgrad_thin_workspace_bytes(int batch, int cout, int cin, int h, int w, int size) {
    int64_t S = 0, L = 0;
    wgrad_thin_slices((int64_t)batch * h * w, cout, cin, size, &S, &L);
    return sizeof(float) * (size_t)S * (size_t)cout * cin * size * size;
}

// the two-level tree over the slice sums, one thread per element of dW; then row_scale as wgrad_reduce_kernel applies it
__global__ __launch_bounds__(64)
void wgrad_thin_reduce_kernel(const float* __restrict__ part, int64_t n_dw, int slices, const double* __restrict__ row_scale, int ncol,
                              float* __restrict__ dw) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n_dw) return;
    float total = 0.f;
    for (int g0 = 0; g0 < slices; g0 += WGRAD_THIN_GROUP) {
        const int g1 = min(g0 + WGRAD_THIN_GROUP, slices);
        float v = part[(int64_t)g0 * n_dw + i];
#pragma unroll 8
        for (int s = g0 + 1; s < g1; ++s) v = v + part[(int64_t)s * n_dw + i];
        total = g0 == 0 ? v : total + v;
    }
    if (row_scale) total = (float)((double)total * row_scale[i / ncol]);
    dw[i] = total;
}

int launch_wgrad_thin(const float* dz, const float* x, int batch, int cout, int cin, int h, int w, int size, const double* row_scale, float* dw,
                      void* ws, size_t ws_bytes, hipStream_t s) {
    const char* who = "conv_wgrad_thin";
    if (!dz || !x || !dw || !ws) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    if (int rc = wgrad_thin_check_shape(who, batch, cout, cin, h, w, size)) return rc;
    if (ws_bytes < wgrad_thin_workspace_bytes(batch, cout, cin, h, w, size)) { set_error("%s: workspace too small", who); return RTOD_E_ARG; }
    if ((uintptr_t)ws & 15) { set_error("%s: workspace must be 16-byte aligned", who); return RTOD_E_ARG; }
    const int pixels = h * w, ncol = cin * size * size;
    const int64_t K = (int64_t)batch * pixels;
    int64_t S = 0, L = 0;
    wgrad_thin_slices(K, cout, cin, size, &S, &L);
    const int gm = (cout + WT_M - 1) / WT_M, gn = (ncol + WT_N - 1) / WT_N;
    if ((int64_t)gm * gn * S > INT32_MAX) { set_error("%s: grid too large", who); return RTOD_E_ARG; }
    float* part = (float*)ws;
    const dim3 grid((unsigned)((int64_t)gm * gn * S));
    if (size == 1) hipLaunchKernelGGL((wgrad_slice_kernel<1, 1, WT_M, WT_N>), grid, dim3(256), 0, s, dz, x, cout, cin, pixels, w, h, w, (int)K, (int)L, gm, gn, part, (float*)nullptr);
    else hipLaunchKernelGGL((wgrad_slice_kernel<9, 1, WT_M, WT_N>), grid, dim3(256), 0, s, dz, x, cout, cin, pixels, w, h, w, (int)K, (int)L, gm, gn, part, (float*)nullptr);
    const int64_t n = (int64_t)cout * ncol;
    hipLaunchKernelGGL(wgrad_thin_reduce_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, part, n, (int)S, row_scale, ncol, dw);
    return hip_fail(hipGetLastError(), "conv_wgrad_thin launch");
}

}  // namespace rtod
