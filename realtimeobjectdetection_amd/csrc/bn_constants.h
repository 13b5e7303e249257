// The ONE statement of the inverse standard deviation of batch-statistics BatchNorm: r = 1 / sqrt(var + eps) in double, eps = 1e-5
// (nn.BatchNorm2d's default, the reference's).  The forward's per-channel constants (aux_kernels.hip bn_channel_constants) and the
// backward (bn_grad.hip) both come here, so the gradient is that of the very function the forward evaluated.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace rtod {

__host__ __device__ __forceinline__ double bn_inv_std(double var) { return 1.0 / sqrt(var + 1e-5); }

}  // namespace rtod
