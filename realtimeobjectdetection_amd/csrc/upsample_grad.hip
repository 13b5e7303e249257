// Backward of the 2x upsample over dense NCHW maps, gfx950, in gather form: one thread per INPUT pixel adds the contributions of the
// output pixels that read it, in a fixed order (output rows ascending, then columns), then multiplies once by the mask of the conv
// that produced the input (as dgrad.hip: m = 1 where y > 0, else slope; y == NULL or slope == 1: none).  No atomics — torch's own
// backward scatters with them — so the result is bit-identical from call to call.
//   mode 0, bilinear, align_corners=False (the forward of aux_kernels.hip, the reference's nn.Upsample): output row 2 i reads input
//     rows i - 1 and i with weights 0.25 / 0.75, output row 2 i + 1 reads i and i + 1 with 0.75 / 0.25; at the borders the clamp puts
//     both weights on the edge row.  So input row i is read by output rows 2 i - 1 .. 2 i + 2 with
//     wy = {0.25 (i > 0), 0.75 (1 for i == 0), 0.75 (1 for i == H - 1), 0.25 (i < H - 1)}, columns alike: at most 4 x 4 outputs,
//     the weight of one output the product wy * wx (exact: 1, 0.75, 0.5625, 0.25, 0.1875, 0.0625).
//   mode 1, nearest: the sum of the 2 x 2 outputs.
// Arithmetic per term, fp32, no contraction: t = (wy * wx) * dz, acc = acc + t.
#include "rtod_internal.h"

namespace rtod {

template <int MODE>
__global__ __launch_bounds__(256)
void upsample2x_grad_kernel(const float* __restrict__ dz, const float* __restrict__ y, float slope, int64_t total, int height, int width,
                            float* __restrict__ dx) {
    const bool masked = y != nullptr && slope != 1.0f;
    const int W2 = 2 * width;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(idx % width);
        const int64_t q = idx / width;
        const int i = (int)(q % height);
        const float* g = dz + (q / height) * 4 * height * width;      // the [2H, 2W] map of this (b, c)
        float acc = 0.f;
        if (MODE == 0) {
            const float wy[4] = {i > 0 ? 0.25f : 0.f, i > 0 ? 0.75f : 1.f, i < height - 1 ? 0.75f : 1.f, i < height - 1 ? 0.25f : 0.f};
            const float wx[4] = {j > 0 ? 0.25f : 0.f, j > 0 ? 0.75f : 1.f, j < width - 1 ? 0.75f : 1.f, j < width - 1 ? 0.25f : 0.f};
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (wy[a] == 0.f) continue;                           // the row 2 i - 1 or 2 i + 2 does not exist
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if (wx[b] == 0.f) continue;
                    acc = acc + (wy[a] * wx[b]) * g[(int64_t)(2 * i - 1 + a) * W2 + (2 * j - 1 + b)];
                }
            }
        } else {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) acc = acc + g[(int64_t)(2 * i + a) * W2 + (2 * j + b)];
        }
        if (masked && !(y[idx] > 0.f)) acc = acc * slope;
        dx[idx] = acc;
    }
}

int launch_upsample2x_grad(const float* dz, const float* y, float slope, int mode, int batch, int channels, int h, int w, float* dx, hipStream_t s) {
    if (!dz || !dx) { set_error("upsample2x_grad: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || channels < 1 || h < 1 || w < 1 || (mode != 0 && mode != 1) || !(slope == slope)) {
        set_error("upsample2x_grad: unsupported arguments (batch=%d channels=%d height=%d width=%d mode=%d slope=%g; mode 0 bilinear, 1 nearest)",
                  batch, channels, h, w, mode, (double)slope);
        return RTOD_E_ARG;
    }
    if (h > INT32_MAX / 2 || w > INT32_MAX / 2 || 4 * (int64_t)h * w > INT32_MAX) { set_error("upsample2x_grad: the output map exceeds int32"); return RTOD_E_ARG; }
    const int64_t total = (int64_t)batch * channels * h * w;
    int64_t grid = (total + 255) / 256;
    if (grid > 4096) grid = 4096;                                     // grid stride beyond
    if (mode == 0) hipLaunchKernelGGL(upsample2x_grad_kernel<0>, dim3((unsigned)grid), dim3(256), 0, s, dz, y, slope, total, h, w, dx);
    else hipLaunchKernelGGL(upsample2x_grad_kernel<1>, dim3((unsigned)grid), dim3(256), 0, s, dz, y, slope, total, h, w, dx);
    return hip_fail(hipGetLastError(), "upsample2x_grad launch");
}

}  // namespace rtod
