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
// slice); slice sums go to the workspace and wgrad_reduce_kernel adds them in a fixed order.  No floating-point atomics: the
// result is bit-identical from call to call.  Every accumulator is an fmaf chain over its slice in a fixed permutation of k; db
// is a plain fp32 sum over the slice in ascending k, kept by the workgroups of the first column of tiles.
//
// One launcher, three slice rules.  Every entry goes through launch_wgrad: one shape check, one schedule (wgrad_schedule: tile,
// K, S, slice length L, reduction group), one workspace size, one slice kernel, one reduce kernel.  The entries differ in the
// rule alone (documented in rtod.h), a pure function of the shape:
//   head  (rtod_conv1x1_wgrad)            cap = 16
//   tiled (rtod_conv_wgrad, _s2)          cap = min(16, ceil(1024 / tiles)): a 13 x 13 block has a thousand tiles already and is not sliced
//       both: 64 x 64 tiles;  L = 8 * ceil(ceil(K / 8) / cap);  S = ceil(K / L) <= cap;  the S sums added in ascending order
//   thin  (rtod_conv_wgrad_thin: any cin, stride 1, no db)   few channels, a huge K — YOLOv3-tiny's layer 0 at 416 x 416 batch 8
//       is a 16 x 27 dW over K = 1,384,448.  32 x 128 tiles (layer 0: one tile, layer 2's 32 x 144: two);  target = ceil(1024 / tiles);
//       L = 8 * ceil(ceil(K / 8) / target) clamped to [WGRAD_THIN_MIN_CHAIN, WGRAD_THIN_MAX_CHAIN];  S = ceil(K / L)
//       (rtod_conv_wgrad_thin_slices), so a large K gets at least 1024 workgroups and no fmaf chain is longer than 1024 terms: the
//       longest chain measured inside the 4 x gate (dgrad.hip's per-tap chain of a 1024-filter conv; one chain of 4608 / 9216
//       terms was measured outside).  The S sums are added as a fixed two-level tree: groups of WGRAD_THIN_GROUP = 32 consecutive
//       slices in ascending order, then the group sums in ascending order (S = 1352 at layer 0: the longest run of fp32 adds is
//       31 + 42, not 1351).
// The ascending sum of the first two rules is the same tree with one group that holds every slice.
//
// 3x3 convs (rtod_conv_wgrad, TAPS = 9).  The same kernel as an implicit GEMM: the column index is n = c * 9 + tap, OIHW order, so
// the dW stores stay coalesced, and B[n][k] = x[b, c, y + ky - 1, x + kx - 1], an exact zero outside the map.  A thread's eight
// columns (channel and tap offsets) do not depend on k and are resolved once; k -> (b, y, x) costs two divisions per staged chunk.
// Stride 2 (rtod_conv_wgrad_s2) is the same column with the tap positions doubled: k runs over the conv's OUTPUT map, x lives on
// its input map.  The 1x1 instance (TAPS = 1) reads x where it reads dz.  The reduce kernel multiplies the reduced sum of a
// row by a caller-supplied double once — the frozen BatchNorm scale of the conv.
#include "rtod_internal.h"

namespace rtod {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG_BK = 32;               // k per LDS stage
constexpr int WG_LD = WG_BK + 4;        // padded row (floats)
constexpr int WG_T = 64;                // tile edge (rows of dz and rows of x per workgroup)

constexpr int WT_M = 32, WT_N = 128;    // the thin tile

// The three slice rules (header; rtod.h), of a shape wgrad_check_shape accepted.  h x w: the map of x; stride 2: k runs over the conv's output map
WgradSchedule wgrad_schedule(WgradRule rule, int batch, int cout, int cin, int h, int w, int size, int stride) {
    const bool thin = rule == WGRAD_THIN;
    WgradSchedule sc;
    sc.tm = thin ? WT_M : WG_T;
    sc.tn = thin ? WT_N : WG_T;
    sc.h = stride == 2 ? (h - 1) / 2 + 1 : h;
    sc.w = stride == 2 ? (w - 1) / 2 + 1 : w;
    sc.K = (int64_t)batch * sc.h * sc.w;
    const int64_t tiles = std::max<int64_t>(1, (((int64_t)cout + sc.tm - 1) / sc.tm) * (((int64_t)cin * size * size + sc.tn - 1) / sc.tn));
    const int64_t target = (1024 + tiles - 1) / tiles;              // slices that bring the grid to a thousand workgroups
    const int64_t units = (sc.K + 7) / 8;
    const int64_t cap = thin ? target : rule == WGRAD_HEAD ? WGRAD_MAX_SLICES : std::min<int64_t>(WGRAD_MAX_SLICES, target);
    int64_t L = 8 * ((units + cap - 1) / cap);
    if (thin) L = std::min<int64_t>(WGRAD_THIN_MAX_CHAIN, std::max<int64_t>(WGRAD_THIN_MIN_CHAIN, L));
    sc.slice_len = (int)L;
    sc.slices = (int)((sc.K + L - 1) / L);
    sc.group = thin ? WGRAD_THIN_GROUP : sc.slices;
    sc.reduce_block = thin ? 64 : 256;                               // few elements, long sums: more workgroups
    sc.db = !thin;
    return sc;
}

// S slice sums of dW and, where the entry has a db, of db
size_t wgrad_workspace_bytes(const WgradSchedule& sc, int cout, int cin, int size) {
    return sizeof(float) * (size_t)sc.slices * ((size_t)cout * cin * size * size + (sc.db ? (size_t)cout : 0));
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

// the slice sums added as a fixed two-level tree, one thread per element of dW, then of db: groups of `group` consecutive slices in
// ascending order, then the group sums in ascending order.  One group (group >= slices) is v = part[0]; v = v + part[s] ascending
// and no further add.  row_scale (may be NULL): the reduced sum of row o of dW (ncol elements) times row_scale[o] in double,
// rounded once; db (may be NULL) is the plain sum
__global__ __launch_bounds__(256)
void wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ part_db, int64_t n_dw, int cout, int slices, int group,
                         const double* __restrict__ row_scale, int ncol, float* __restrict__ dw, float* __restrict__ db) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool bias = i >= n_dw;
    if (bias && !(db && i < n_dw + cout)) return;
    const float* p = bias ? part_db + (i - n_dw) : part + i;
    const int64_t step = bias ? cout : n_dw;                         // floats between consecutive slices
    float total = 0.f;
    for (int g0 = 0; g0 < slices; g0 += group) {
        const int g1 = min(g0 + group, slices);
        float v = p[(int64_t)g0 * step];
#pragma unroll 8
        for (int s = g0 + 1; s < g1; ++s) v = v + p[(int64_t)s * step];
        total = g0 == 0 ? v : total + v;
    }
    if (bias) db[i - n_dw] = total;
    else dw[i] = row_scale ? (float)((double)total * row_scale[i / ncol]) : total;
}

// stride 2 (h x w the conv's input map) takes size 3 alone; the thin rule takes any cin >= 1
int wgrad_check_shape(const char* who, WgradRule rule, int batch, int cout, int cin, int h, int w, int size, int stride) {
    const bool thin = rule == WGRAD_THIN;
    const int64_t K = (int64_t)batch * h * w, taps = (int64_t)size * size;
    if (batch < 1 || cout < 1 || cin < 1 || (!thin && cin % 32) || h < 1 || w < 1 || (size != 1 && size != 3)) {
        set_error("%s: unsupported shape (batch=%d cout=%d cin=%d h=%d w=%d size=%d; %ssize 1 or 3)", who, batch, cout, cin, h, w, size,
                  thin ? "" : "cin must be a multiple of 32, ");
        return RTOD_E_ARG;
    }
    if ((int64_t)h * w > INT32_MAX || K > INT32_MAX - (thin ? WGRAD_THIN_MAX_CHAIN : 64) || (int64_t)cout * cin * taps > INT32_MAX) {
        set_error("%s: batch * h * w or cout * cin * size * size exceeds int32", who);
        return RTOD_E_ARG;
    }
    if (stride == 2 && size != 3) { set_error("%s: unsupported shape (size=%d; the stride-2 entry takes 3x3 convs)", who, size); return RTOD_E_ARG; }
    return RTOD_OK;
}

// `who` names the entry in every error text, `rule` is its slice rule.  stride 2 (rtod_conv_wgrad_s2: size 3, pad 1): h x w is the
// conv's INPUT map, dz lives on the output map and K = batch * ho * wo.  db may be NULL (the thin entry has none)
int launch_wgrad(const char* who, WgradRule rule, const float* dz, const float* x, int batch, int cout, int cin, int h, int w, int size, int stride,
                 const double* row_scale, float* dw, float* db, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!dz || !x || !dw || !ws) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    if (int rc = wgrad_check_shape(who, rule, batch, cout, cin, h, w, size, stride)) return rc;
    const WgradSchedule sc = wgrad_schedule(rule, batch, cout, cin, h, w, size, stride);
    if (!sc.db) db = nullptr;                                         // no db part in the workspace
    if (ws_bytes < wgrad_workspace_bytes(sc, cout, cin, size)) { set_error("%s: workspace too small", who); return RTOD_E_ARG; }
    if ((uintptr_t)ws & 15) { set_error("%s: workspace must be 16-byte aligned", who); return RTOD_E_ARG; }
    const int pixels = sc.h * sc.w, ncol = cin * size * size, S = sc.slices;
    const int gm = (cout + sc.tm - 1) / sc.tm, gn = (ncol + sc.tn - 1) / sc.tn;
    if ((int64_t)gm * gn * S > INT32_MAX) { set_error("%s: grid too large", who); return RTOD_E_ARG; }
    const int64_t n_dw = (int64_t)cout * ncol;
    float* part = (float*)ws;
    float* part_db = db ? part + S * n_dw : (float*)nullptr;
#define RTOD_WGRAD(...) hipLaunchKernelGGL((wgrad_slice_kernel<__VA_ARGS__>), dim3((unsigned)((int64_t)gm * gn * S)), dim3(256), 0, s, dz, x, cout, cin, pixels, sc.w, h, w, (int)sc.K, sc.slice_len, gm, gn, part, part_db)
    if (sc.tm == WT_M && size == 1) RTOD_WGRAD(1, 1, WT_M, WT_N);
    else if (sc.tm == WT_M) RTOD_WGRAD(9, 1, WT_M, WT_N);
    else if (stride == 2) RTOD_WGRAD(9, 2);
    else if (size == 1) RTOD_WGRAD(1);
    else RTOD_WGRAD(9);
#undef RTOD_WGRAD
    const int64_t n = n_dw + (db ? cout : 0);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((n + sc.reduce_block - 1) / sc.reduce_block)), dim3(sc.reduce_block), 0, s, part, part_db, n_dw, cout, S,
                       sc.group, row_scale, ncol, dw, db);
    return hip_fail(hipGetLastError(), (std::string(who) + " launch").c_str());
}

}  // namespace rtod
