// Data gradient of a 1x1 convolution z = W y with the derivative of the activation that produced y fused, on the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32), gfx950:
//   dx[b][c][p] = m(y[b][c][p]) * sum_o w[o][c] * dz[b][o][p]        m(y) = 1 for y > 0, else slope   (torch's leaky_relu backward)
// w [cout, cin] (the float32 masters of a detection-head conv), dz [batch, cout, pixels] (rtod_yolo_loss_grad's map of that head),
// y [batch, cin, pixels] the STORED output of the conv in front of it (rtod_plan_read_layer): the sign of a leaky-ReLU's output is
// the sign of its input, so no pre-activation buffer is kept.  y == NULL or slope == 1: linear, no mask.
//
// GEMM view:  D[m][n] = sum_k A[m][k] * B[k][n],  m = c (MFMA rows), n = b * pixels + p (MFMA columns, on the lane: coalesced dx
// stores), k = o.  Both operands are contiguous along their free index (w along c, dz along p), so a thread stages one row index
// for eight k and LDS holds a K-chunk k-major, [32][64 + 32] floats per operand: a wave's ds_read_b32 of one k takes 32
// consecutive floats per lane half and the halves (k, k + 1) sit 96 floats = 32 banks apart.
// Workgroup: 4 waves, a 64 x 64 tile of dx, one 32 x 32 accumulator per wave; the next chunk's global loads are in flight during
// the MFMAs.  K = cout is short and ragged (255): rows past cout are staged as zeros, which leave an fmaf chain unchanged, and
// there are no K slices — every dx element is ONE fmaf chain over o in ascending pairs (o, o + 1), then one multiplication by
// the mask.  Plain vector stores, no atomics: bit-identical from call to call.
#include "rtod_internal.h"

namespace rtod {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int DG_BK = 32;               // k per LDS stage
constexpr int DG_T = 64;                // tile edge
constexpr int DG_LD = DG_T + 32;        // floats per k row

__global__ __launch_bounds__(256)
void dgrad_kernel(const float* __restrict__ w, const float* __restrict__ dz, const float* __restrict__ y, float slope,
                  int cout, int cin, int pixels, int N, int grid_n, float* __restrict__ dx) {
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
    const float* wcol = w + sc;
    const float* dzrow = dz + (int64_t)sb * cout * pixels + sp;

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float ra[DG_BK / 4], rb[DG_BK / 4];
    auto gload = [&](int kc) {
#pragma unroll
        for (int i = 0; i < DG_BK / 4; ++i) {
            const int o = kc + ks + 4 * i;
            ra[i] = (c_ok && o < cout) ? wcol[(int64_t)o * cin] : 0.f;
            rb[i] = (n_ok && o < cout) ? dzrow[(int64_t)o * pixels] : 0.f;
        }
    };
    gload(0);
    const float* pa = sA + lh * DG_LD + wm * 32 + lr;
    const float* pb = sB + lh * DG_LD + wn * 32 + lr;
    for (int kc = 0; kc < cout; kc += DG_BK) {
        __syncthreads();                                          // the previous chunk's LDS reads are done
#pragma unroll
        for (int i = 0; i < DG_BK / 4; ++i) {
            sA[(ks + 4 * i) * DG_LD + r] = ra[i];
            sB[(ks + 4 * i) * DG_LD + r] = rb[i];
        }
        __syncthreads();
        if (kc + DG_BK < cout) gload(kc + DG_BK);                 // in flight while the MFMAs below run
#pragma unroll
        for (int t = 0; t < DG_BK / 2; ++t)                       // lane half lh supplies k = 2 t + lh
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * t * DG_LD], pb[2 * t * DG_LD], acc, 0, 0, 0);
    }
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

int launch_conv1x1_dgrad(const float* w, const float* dz, const float* y, float slope, int batch, int cout, int cin, int pixels,
                         float* dx, hipStream_t s) {
    if (!w || !dz || !dx) { set_error("conv1x1_dgrad: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || cout < 1 || cin < 32 || cin % 32 || pixels < 1 || !(slope == slope)) {
        set_error("conv1x1_dgrad: unsupported arguments (batch=%d cout=%d cin=%d pixels=%d slope=%g; cin must be a multiple of 32)", batch, cout, cin, pixels, (double)slope);
        return RTOD_E_ARG;
    }
    const int64_t N = (int64_t)batch * pixels;
    if (N > INT32_MAX - 64 || (int64_t)cout * cin > INT32_MAX) { set_error("conv1x1_dgrad: batch * pixels or cout * cin exceeds int32"); return RTOD_E_ARG; }
    const int64_t gm = (cin + DG_T - 1) / DG_T, gn = (N + DG_T - 1) / DG_T;
    if (gm * gn > INT32_MAX) { set_error("conv1x1_dgrad: grid too large"); return RTOD_E_ARG; }
    hipLaunchKernelGGL(dgrad_kernel, dim3((unsigned)(gm * gn)), dim3(256), 0, s, w, dz, y, slope, cout, cin, pixels, (int)N, (int)gn, dx);
    return hip_fail(hipGetLastError(), "conv1x1_dgrad launch");
}

}  // namespace rtod
