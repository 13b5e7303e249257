// Backward of batch-statistics BatchNorm over dense NCHW float32 maps (rtod_bn_grad), gfx950.  Per channel, N = batch * pixels,
// mean / var the plan's doubles (the very values the forward normalised with), r = bn_inv_std(var) (bn_constants.h):
//
//   S1 = sum (double)du                      S2 = sum (double)du * ((double)z - mean)
//   dbeta  = (float)S1                       dgamma = (float)(S2 * r)
//   dz_i   = (float)( gamma * r * ( (double)du_i - S1 / N - ((double)z_i - mean) * r * r * S2 / N ) )
//
// du: the gradient with respect to the BatchNorm output (the leaky mask already applied), z: the raw conv output the forward read.
// Every operation is a double operation with one rounding (this file is built with -ffp-contract=off), evaluated as written below
// (bn_grad_apply_kernel); one rounding to float per output.
//
// Two launches, no third, no atomics.  A channel's N values (n = b * pixels + p) are cut into `parts` ranges of `part_len`:
//   target = min(256, ceil(2048 / channels));   part_len = 1024 * ceil(ceil(N / target) / 1024);   parts = ceil(N / part_len)
// — the shape alone, never the device: about 2048 workgroups of 256 threads where the tensor is large (YOLOv3-tiny's layer 0 at
// 416 x 416, batch 8: 16 channels x 123 parts of 11264), and never less than 1024 values per workgroup where it is not (a 13 x 13 map
// at batch 8 with 1024 channels: 1024 x 2 workgroups of four waves, not 1024 x 8 of one).
//   bn_grad_reduce_kernel   one workgroup per (channel, part): each thread adds its values in ascending order in double, the 256
//                           thread sums go through a fixed LDS tree, one pair (S1, S2) of partial sums per (channel, part).
//   bn_grad_apply_kernel    the same grid: every thread adds the channel's parts in ascending order in its prologue — the same
//                           sum in the same order in every workgroup of the channel —, then dz over its part; the workgroup of
//                           part 0 writes dgamma and dbeta.
// A channel's plane starts at an arbitrary 4-byte alignment (pixels = 169 at 13 x 13), so both kernels walk a part as its runs —
// the pieces of the planes (b, c) it covers — and a run as the 16-byte-aligned quads of MEMORY it touches (bn_grad_walk): a quad
// wholly inside the run is one 16-byte access per tensor, the head and the tail of a run go element by element.  The three tensors
// share one layout, so one alignment rule serves du, z and dz; their base pointers must be 16-byte aligned.  The assignment of
// values to threads depends on the shape alone: results are bit-identical from call to call and from device to device.
#include "rtod_internal.h"
#include "bn_constants.h"

namespace rtod {

constexpr int BN_GRAD_THREADS = 256;
constexpr int BN_GRAD_GRANULE = 1024;                                 // values: four per thread
constexpr int BN_GRAD_WORKGROUPS = 2048;                              // the grid the partition aims at
constexpr int BN_GRAD_PARTS_MAX = 256;                                // ... and the longest prologue sum of the second launch

struct BnGradShape { int N, parts, part_len, slots; };                // slots: quad slots per run of the walk

// The partition rule (above) and the refusals all three entries share
static int bn_grad_shape(const char* who, int batch, int channels, int pixels, BnGradShape& g) {
    if (batch < 1 || channels < 1 || pixels < 1) { set_error("%s: unsupported arguments (batch=%d channels=%d pixels=%d)", who, batch, channels, pixels); return RTOD_E_ARG; }
    if ((int64_t)batch * pixels >= (1ll << 29)) { set_error("%s: batch * pixels = %lld is not below 2^29", who, (long long)batch * pixels); return RTOD_E_ARG; }
    g.N = batch * pixels;
    const int target = std::min(BN_GRAD_PARTS_MAX, (BN_GRAD_WORKGROUPS + channels - 1) / channels);
    const int per = (g.N + target - 1) / target;
    g.part_len = BN_GRAD_GRANULE * ((per + BN_GRAD_GRANULE - 1) / BN_GRAD_GRANULE);
    g.parts = (g.N + g.part_len - 1) / g.part_len;
    if ((int64_t)channels * g.parts > INT32_MAX) { set_error("%s: %d channels x %d parts exceed the grid", who, channels, g.parts); return RTOD_E_ARG; }
    g.slots = std::min(pixels, g.part_len) / 4 + 2;                   // a run of len values touches at most len / 4 + 2 aligned quads
    return RTOD_OK;
}

// The walk of part `part` of channel c that both kernels make: values n in [part * part_len, min(N, (part + 1) * part_len)), as runs
// (one per plane (b, c) the range meets) of `slots` quad slots each; slot k of a run is the aligned quad of memory k past the one
// that holds the run's first element.  Thread t takes slots t, t + 256, ... in ascending order: f.quad(e) for a quad wholly inside
// the run (e: element offset, a multiple of 4), f.one(e) for each element of a quad the run covers in part; a slot past the run's
// end is skipped.  Every offset lies inside the plane of (b, c), b < batch.
template <class F>
__device__ __forceinline__ void bn_grad_walk(int c, int channels, int pixels, int N, int part_len, int slots, int part, F& f) {
    const int n0 = part * part_len, n1 = min(N, n0 + part_len);
    const int b0 = n0 / pixels, b1 = (n1 - 1) / pixels;
    const int total = (b1 - b0 + 1) * slots;                          // < 2^31: bn_grad_shape's bound on N
    for (int i = threadIdx.x; i < total; i += BN_GRAD_THREADS) {
        const int r = i / slots, k = i - r * slots;
        const int first = (b0 + r) * pixels;                          // the plane's first n
        const int64_t base = ((int64_t)(b0 + r) * channels + c) * pixels;
        const int64_t a0 = base + (max(n0, first) - first), a1 = base + (min(n1, first + pixels) - first);
        const int64_t e0 = (a0 / 4 + k) * 4;
        if (e0 >= a1) continue;
        if (e0 >= a0 && e0 + 4 <= a1) f.quad(e0);
        else
            for (int64_t e = max(e0, a0); e < min(e0 + 4, a1); ++e) f.one(e);
    }
}

struct BnGradReduce {
    const float* __restrict__ du; const float* __restrict__ z; double mean, s1, s2;
    __device__ __forceinline__ void add(float g, float v) { s1 = s1 + (double)g; s2 = s2 + (double)g * ((double)v - mean); }
    __device__ __forceinline__ void quad(int64_t e) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(du + e), v = *reinterpret_cast<const f32x4*>(z + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) add(g[j], v[j]);
    }
    __device__ __forceinline__ void one(int64_t e) { add(du[e], z[e]); }
};

__global__ __launch_bounds__(BN_GRAD_THREADS)
void bn_grad_reduce_kernel(const float* __restrict__ du, const float* __restrict__ z, const double* __restrict__ mean, int channels, int pixels,
                           BnGradShape g, double* __restrict__ partial) {
    const int c = blockIdx.x / g.parts, part = blockIdx.x - c * g.parts;
    BnGradReduce f{du, z, mean[c], 0.0, 0.0};
    bn_grad_walk(c, channels, pixels, g.N, g.part_len, g.slots, part, f);
    __shared__ double red[2][BN_GRAD_THREADS];
    red[0][threadIdx.x] = f.s1; red[1][threadIdx.x] = f.s2;
    __syncthreads();
    for (int w = BN_GRAD_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { red[0][threadIdx.x] = red[0][threadIdx.x] + red[0][threadIdx.x + w]; red[1][threadIdx.x] = red[1][threadIdx.x] + red[1][threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * (int64_t)blockIdx.x] = red[0][0]; partial[2 * (int64_t)blockIdx.x + 1] = red[1][0]; }
}

struct BnGradApply {
    const float* __restrict__ du; const float* __restrict__ z; float* __restrict__ dz; double mean, scale, shift, slope;
    // dz = gamma r ((du - S1 / N) - (z - mean) (r r S2 / N)): scale = gamma r, shift = S1 / N, slope = r r S2 / N
    __device__ __forceinline__ float value(float g, float v) const { return (float)(scale * (((double)g - shift) - ((double)v - mean) * slope)); }
    __device__ __forceinline__ void quad(int64_t e) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(du + e), v = *reinterpret_cast<const f32x4*>(z + e);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = value(g[j], v[j]);
        *reinterpret_cast<f32x4*>(dz + e) = o;
    }
    __device__ __forceinline__ void one(int64_t e) { dz[e] = value(du[e], z[e]); }
};

__global__ __launch_bounds__(BN_GRAD_THREADS)
void bn_grad_apply_kernel(const float* __restrict__ du, const float* __restrict__ z, const double* __restrict__ mean, const double* __restrict__ var,
                          const float* __restrict__ gamma, int channels, int pixels, BnGradShape g, const double* __restrict__ partial,
                          float* __restrict__ dz, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x / g.parts, part = blockIdx.x - c * g.parts;
    double s1 = 0.0, s2 = 0.0;
    const double* p = partial + 2 * (int64_t)c * g.parts;
    for (int k = 0; k < g.parts; ++k) { s1 = s1 + p[2 * k]; s2 = s2 + p[2 * k + 1]; }     // every thread of every part: the same order
    const double r = bn_inv_std(var[c]);
    if (part == 0 && threadIdx.x == 0) { dbeta[c] = (float)s1; dgamma[c] = (float)(s2 * r); }
    BnGradApply f{du, z, dz, mean[c], (double)gamma[c] * r, s1 / (double)g.N, r * r * s2 / (double)g.N};
    bn_grad_walk(c, channels, pixels, g.N, g.part_len, g.slots, part, f);
}

int bn_grad_parts(int batch, int channels, int pixels, int* parts, int* part_len) {
    if (!parts || !part_len) { set_error("bn_grad_parts: null pointer"); return RTOD_E_ARG; }
    BnGradShape g;
    if (int rc = bn_grad_shape("bn_grad_parts", batch, channels, pixels, g)) return rc;
    *parts = g.parts; *part_len = g.part_len;
    return RTOD_OK;
}

int bn_grad_workspace(int batch, int channels, int pixels, size_t* bytes) {
    if (!bytes) { set_error("bn_grad_workspace: null pointer"); return RTOD_E_ARG; }
    BnGradShape g;
    if (int rc = bn_grad_shape("bn_grad_workspace", batch, channels, pixels, g)) return rc;
    *bytes = sizeof(double) * 2 * (size_t)channels * (size_t)g.parts;
    return RTOD_OK;
}

int launch_bn_grad(const float* du, const float* z, const double* mean, const double* var, const float* gamma, int batch, int channels, int pixels,
                   float* dz, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, hipStream_t s) {
    if (!du || !z || !mean || !var || !gamma || !dz || !dgamma || !dbeta || !workspace) { set_error("bn_grad: null pointer"); return RTOD_E_ARG; }
    BnGradShape g;
    if (int rc = bn_grad_shape("bn_grad", batch, channels, pixels, g)) return rc;
    if ((((uintptr_t)du | (uintptr_t)z | (uintptr_t)dz | (uintptr_t)workspace) & 15) || (((uintptr_t)mean | (uintptr_t)var) & 7)) {
        set_error("bn_grad: du, z, dz and the workspace must be 16-byte aligned, mean and var 8-byte aligned");
        return RTOD_E_ARG;
    }
    const size_t need = sizeof(double) * 2 * (size_t)channels * (size_t)g.parts;
    if (workspace_bytes < need) { set_error("bn_grad: the workspace has %zu bytes, %zu are needed", workspace_bytes, need); return RTOD_E_ARG; }
    const dim3 grid((unsigned)(channels * g.parts)), block(BN_GRAD_THREADS);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(bn_grad_reduce_kernel, grid, block, 0, s, du, z, mean, channels, pixels, g, partial);
    if (int rc = hip_fail(hipGetLastError(), "bn_grad_reduce launch")) return rc;
    hipLaunchKernelGGL(bn_grad_apply_kernel, grid, block, 0, s, du, z, mean, var, gamma, channels, pixels, g, (const double*)partial, dz, dgamma, dbeta);
    return hip_fail(hipGetLastError(), "bn_grad_apply launch");
}

}  // namespace rtod
