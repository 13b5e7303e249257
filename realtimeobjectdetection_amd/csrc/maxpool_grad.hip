// Backward of the size-2 max-pool over dense NCHW maps, gfx950, in gather form: one thread per INPUT element visits the windows that
// cover it, recomputes each window's winner from x with the forward's rule (aux_kernels.hip maxpool_kernel, torch's rule: scan dy then
// dx, replace only on strictly greater, so the FIRST maximum wins) and adds dz of the windows it won, in ascending (oy, ox) order with
// fp32 adds; then one multiplication by the mask of the conv that produced x (as dgrad.hip: m = 1 where x > 0, else slope; slope == 1:
// none).  The same tensor x serves the winners and the mask.  No atomics, plain stores: bit-identical from call to call.
//   stride 2, floor mode (nn.MaxPool2d(2, 2)): output (oy, ox) reads rows 2 oy, 2 oy + 1 and columns 2 ox, 2 ox + 1; Ho = H / 2,
//     Wo = W / 2.  An input element lies in at most one window; an odd last row or column lies in none and gets an exact +0.
//   stride 1, clamped window (MaxPoolStride1: replicate pad right / bottom, then MaxPool2d(2, 1)): output (oy, ox) reads rows
//     min(oy + dy, H - 1) and columns min(ox + dx, W - 1); Ho = H, Wo = W.  An input element lies in at most four windows, oy in
//     {iy - 1, iy}, ox in {ix - 1, ix}.  At the last row / column the duplicated taps are the same pixel: the winner is decided in
//     window-scan order over the four taps and then mapped to its clamped pixel, as autograd through the padded copy adds it.
// NaN inputs are out of contract (the forward's `v > m` never picks a NaN; torch's pool propagates it).
#include "rtod_internal.h"

namespace rtod {

template <int STRIDE>
__global__ __launch_bounds__(256)
void maxpool2_grad_kernel(const float* __restrict__ dz, const float* __restrict__ x, float slope, int64_t total, int height, int width,
                          float* __restrict__ dx) {
    const bool masked = slope != 1.0f;
    const int ho = STRIDE == 2 ? height / 2 : height, wo = STRIDE == 2 ? width / 2 : width;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int ix = (int)(idx % width);
        const int64_t q = idx / width;
        const int iy = (int)(q % height);
        const int64_t map = q / height;                               // (b, c)
        const float* xm = x + map * height * width;
        const float* g = dz + map * ho * wo;
        // the winner of window (oy, ox) as a clamped pixel index; taps inside the map by construction
        auto winner = [&](int oy, int ox) {
            float m = -INFINITY;
            int at = -1;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const int yy = min(oy * STRIDE + dy, height - 1);
#pragma unroll
                for (int dxx = 0; dxx < 2; ++dxx) {
                    const int xx = min(ox * STRIDE + dxx, width - 1);
                    const float v = xm[(int64_t)yy * width + xx];
                    if (v > m) { m = v; at = yy * width + xx; }
                }
            }
            return at;
        };
        const int self = iy * width + ix;
        float acc = 0.f;
        if (STRIDE == 2) {
            const int oy = iy >> 1, ox = ix >> 1;
            if (oy < ho && ox < wo && winner(oy, ox) == self) acc = acc + g[(int64_t)oy * wo + ox];
        } else {
            for (int oy = max(iy - 1, 0); oy <= iy; ++oy)
                for (int ox = max(ix - 1, 0); ox <= ix; ++ox)
                    if (winner(oy, ox) == self) acc = acc + g[(int64_t)oy * wo + ox];
        }
        if (masked && !(xm[self] > 0.f)) acc = acc * slope;
        dx[idx] = acc;
    }
}

int launch_maxpool_grad(const float* dz, const float* x, float slope, int batch, int channels, int h, int w, int size, int stride, float* dx,
                        hipStream_t s) {
    // (a stride-2 pool of a one-pixel-wide or -high map has an empty output: dz is then not read and may be NULL)
    const bool empty = stride == 2 && h >= 1 && w >= 1 && (h < 2 || w < 2);
    if ((!dz && !empty) || !x || !dx) { set_error("maxpool_grad: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || channels < 1 || h < 1 || w < 1 || size != 2 || (stride != 1 && stride != 2) || !(slope == slope)) {
        set_error("maxpool_grad: unsupported arguments (batch=%d channels=%d height=%d width=%d size=%d stride=%d slope=%g; size 2, stride 1 or 2, no symmetric padding)",
                  batch, channels, h, w, size, stride, (double)slope);
        return RTOD_E_ARG;
    }
    if ((int64_t)h * w > INT32_MAX) { set_error("maxpool_grad: the map exceeds int32"); return RTOD_E_ARG; }
    const int64_t total = (int64_t)batch * channels * h * w;
    int64_t grid = (total + 255) / 256;
    if (grid > 8192) grid = 8192;                                     // grid stride beyond
    if (stride == 2) hipLaunchKernelGGL(maxpool2_grad_kernel<2>, dim3((unsigned)grid), dim3(256), 0, s, dz, x, slope, total, h, w, dx);
    else hipLaunchKernelGGL(maxpool2_grad_kernel<1>, dim3((unsigned)grid), dim3(256), 0, s, dz, x, slope, total, h, w, dx);
    return hip_fail(hipGetLastError(), "maxpool_grad launch");
}

}  // namespace rtod
