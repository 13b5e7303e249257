// The fan-out point of the gradient walk in one launch (rtod_grad_join), gfx950:
//   out[i] = m(y[i]) * (((c0[i] + c1[i]) + c2[i]) + c3[i])        m(y) = 1 for y > 0, else slope
// 1 to 4 contributions added left to right with one fp32 add each (no contraction: this file is built with -ffp-contract=off), then one
// multiplication by slope where !(y > 0) — what the walk did in four torch passes (a + b, full_like, masked_fill_, *), bit for bit:
// a multiplication by 1 changes nothing, so it is skipped.  y == NULL or slope == 1: no mask.  With one contribution it is the mask
// alone.  Pure streaming: 16-byte loads and stores where every pointer is 16-byte aligned, four elements per thread, and a scalar
// tail (or the scalar form throughout) otherwise.  Plain stores: bit-identical from call to call.
#include "rtod_internal.h"

namespace rtod {

struct GradJoin { const float* c[4]; };

template <int COUNT>
__global__ __launch_bounds__(256)
void grad_join_kernel(GradJoin g, const float* __restrict__ y, float slope, int64_t n, int64_t n_vec, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool masked = y != nullptr && slope != 1.0f;
    if (t < n_vec) {                                                  // elements 4 t .. 4 t + 3
        f32x4 v = reinterpret_cast<const f32x4*>(g.c[0])[t];
#pragma unroll
        for (int j = 1; j < COUNT; ++j) v = v + reinterpret_cast<const f32x4*>(g.c[j])[t];
        if (masked) {
            const f32x4 yy = reinterpret_cast<const f32x4*>(y)[t];
#pragma unroll
            for (int e = 0; e < 4; ++e) if (!(yy[e] > 0.f)) v[e] = v[e] * slope;
        }
        reinterpret_cast<f32x4*>(out)[t] = v;
        return;
    }
    const int64_t i = 4 * n_vec + (t - n_vec);                        // the tail, one element per thread
    if (i >= n) return;
    float v = g.c[0][i];
#pragma unroll
    for (int j = 1; j < COUNT; ++j) v = v + g.c[j][i];
    if (masked && !(y[i] > 0.f)) v = v * slope;
    out[i] = v;
}

int launch_grad_join(const float* const* contributions, int count, const float* y, float slope, int64_t n, float* out, hipStream_t s) {
    if (!contributions || !out) { set_error("grad_join: null pointer"); return RTOD_E_ARG; }
    if (count < 1 || count > 4 || n < 1 || !(slope == slope)) { set_error("grad_join: unsupported arguments (count=%d n=%lld slope=%g; 1 to 4 contributions)", count, (long long)n, (double)slope); return RTOD_E_ARG; }
    GradJoin g{{nullptr, nullptr, nullptr, nullptr}};
    uintptr_t align = (uintptr_t)out | (uintptr_t)y;
    for (int j = 0; j < count; ++j) {
        if (!contributions[j]) { set_error("grad_join: contribution %d is null", j); return RTOD_E_ARG; }
        g.c[j] = contributions[j];
        align |= (uintptr_t)contributions[j];
    }
    const int64_t n_vec = (align & 15) ? 0 : n / 4;
    const int64_t threads = n_vec + (n - 4 * n_vec);
    const int64_t blocks = (threads + 255) / 256;
    if (blocks > INT32_MAX) { set_error("grad_join: grid too large"); return RTOD_E_ARG; }
    const dim3 grid((unsigned)blocks), block(256);
    switch (count) {
        case 1: hipLaunchKernelGGL(grad_join_kernel<1>, grid, block, 0, s, g, y, slope, n, n_vec, out); break;
        case 2: hipLaunchKernelGGL(grad_join_kernel<2>, grid, block, 0, s, g, y, slope, n, n_vec, out); break;
        case 3: hipLaunchKernelGGL(grad_join_kernel<3>, grid, block, 0, s, g, y, slope, n, n_vec, out); break;
        default: hipLaunchKernelGGL(grad_join_kernel<4>, grid, block, 0, s, g, y, slope, n, n_vec, out); break;
    }
    return hip_fail(hipGetLastError(), "grad_join");
}

}  // namespace rtod
