// Optimiser step of one 1x1 convolution without BatchNorm (a detection head) fused with the re-pack of its block of the weight
// image, gfx950.  One launch per conv, one workgroup per output channel o (plus one for the bias vector):
//   pass 1  every thread walks c = tid, tid + 256, ...: reads the float32 master w[o][c], the gradient and (Adam) the moments,
//           applies the step (opt_update: the fp32 sequence documented at rtod_plan_step_conv in include/rtod.h), writes master
//           and moments back and keeps the largest |w'| it saw (as integer bits: order-preserving for finite floats, exact);
//   reduce  the workgroup's maximum through LDS (a max is order-independent, so this is exact);
//   pass 2  the same thread re-reads the masters it wrote and places them where Plan::pack_conv (plan_weights.cpp) would:
//           fp32 plans   panel[o * Kpad + c] = w'
//           split plans  e = 13 - exponent(max|w'|) held to -24 .. 40 (0 for an all-zero channel), inv[o] = 2^-e / ACT_SCALE_F16S3,
//                        vs = w' * 2^e (exact), hi = f16_rn(vs), lo = f16_rn(vs - hi) at half ((c / 32) * Npad + o) * 32 + c % 32
//                        of the hi and lo planes.
// The same kernel steps a detection BLOCK conv (rtod_plan_step_conv_folded: 1x1 or 3x3, BatchNorm frozen) and folds while it
// re-packs, as pack_conv does for a BatchNorm conv: the master row is OIHW, q = c * taps + tap; with s = the frozen
// gamma / sqrt(var + 1e-5) of channel o (a double), the folded weight is v = (float)((double)w' * s), the channel's exponent comes
// from max |(double)w' * s| (kept as the double's integer bits), and v lands at panel[o * Kpad + tap * cin_p + c] or at half
// (((c / 32) * taps + tap) * Npad + o) * 32 + c % 32.  There is no bias workgroup: the bias slot (beta - mean * s) keeps its bits.
// A head conv is the case taps = 1, s = 1: (double)w' * 1.0 is w' itself, and the exponent of a double equals that of the float.
// A conv whose BatchNorm runs on batch statistics (rtod_plan_step_conv_bn) is the case s = 1 with any taps — pack_conv leaves such a
// conv unfolded — and the extra workgroup steps beta and gamma where a head conv's steps the bias: one mode of this kernel, not a
// second launch for 2 Cout floats.  On a split plan (option bn_batch_split) that case takes the split arm below: the hi / lo planes, the
// pre-scale and inv[o] of the unfolded weight, which is what the raw-sum conv instances read.  Every split tile family (generic, bandd,
// 1x1 slabs) reads this one image layout, so there is one placement rule here as there is one in pack_conv.
// f32 -> f16 and back are the host's integer routines (f16_round.h: round to nearest even, subnormal halves kept, values at or
// below 2^-25 to (signed) zero) — independent of the denormal mode the library is built with.  Nothing outside channel rows
// [0, Cout) and columns [0, Cin) of this conv's block is written: padding channels, padding K and other convs keep their bits.
// Plain vector stores only; no atomics; bit-identical from call to call.  Built with -ffp-contract=off and correctly rounded
// fp32 divide / sqrt (Makefile: PARITY_FLAGS), so every operator below is one IEEE operation with one rounding and the only
// fused multiply-adds are the ones written as fmaf.
#include "rtod_internal.h"
#include "f16_round.h"

namespace rtod {

// one element: (w, g, m, v) -> w'; m, v updated in place (Adam)
__device__ __forceinline__ float opt_update(const HeadStepLaunch& a, float w, float g, float& m, float& v) {
#pragma clang fp contract(off)
    if (a.kind == 0) { const float d = a.lr * g; return w - d; }
    const float gm = g - m;
    m = __builtin_fmaf(gm, a.omb1, m);
    const float gg = g * g, bv = a.beta2 * v;
    v = __builtin_fmaf(gg, a.omb2, bv);
    const float root = __builtin_sqrtf(v) / a.bc2_sqrt;
    const float denom = root + a.eps;
    const float ratio = m / denom;
    return __builtin_fmaf(-a.lr, ratio, w);
}

__global__ __launch_bounds__(256)
void head_step_kernel(HeadStepLaunch a) {
    __shared__ unsigned long long smax[256];
    const int tid = threadIdx.x;
    const int o = blockIdx.x;
    if (o == a.cout) {                                              // the per-channel vectors: masters, moments and the image's copy
        // the bias of a conv without BatchNorm; or (rtod_plan_step_conv_bn) beta and gamma of a batch-statistics BatchNorm conv,
        // which take the same step and land in the image's [Npad] beta, [Npad] gamma block as pack_conv places them
        auto step_vector = [&](float* master, const float* grad, float* mom1, float* mom2, float* image) {
            for (int q = tid; q < a.cout; q += 256) {
                float m = 0.f, v = 0.f;
                if (a.kind == 1) { m = mom1[q]; v = mom2[q]; }
                const float nb = opt_update(a, master[q], grad[q], m, v);
                if (a.kind == 1) { mom1[q] = m; mom2[q] = v; }
                master[q] = nb;
                image[q] = nb;
            }
        };
        if (a.gamma) { step_vector(a.beta, a.dbeta, a.m_be, a.v_be, a.bn); step_vector(a.gamma, a.dgamma, a.m_g, a.v_g, a.bn + a.Npad); }
        else step_vector(a.b, a.db, a.m_b, a.v_b, a.bias);
        return;
    }
    const int n = a.cin * a.taps;                                   // the row of the OIHW master: q = c * taps + tap
    const int64_t row = (int64_t)o * n;
    const double sc = a.scale ? a.scale[o] : 1.0;                   // (double)w' * 1.0 is w' itself
    unsigned long long mx = 0;
    for (int q = tid; q < n; q += 256) {
        float m = 0.f, v = 0.f;
        if (a.kind == 1) { m = a.m_w[row + q]; v = a.v_w[row + q]; }
        const float nw = opt_update(a, a.w[row + q], a.dw[row + q], m, v);
        if (a.kind == 1) { a.m_w[row + q] = m; a.v_w[row + q] = v; }
        a.w[row + q] = nw;
        // |(double)w' * s| as integer bits: order-preserving for non-negative doubles, exact
        const unsigned long long ab = (unsigned long long)__double_as_longlong((double)nw * sc) & 0x7FFFFFFFFFFFFFFFull;
        if (ab <= 0x7FF0000000000000ull && ab > mx) mx = ab;        // a NaN takes no part (std::max on the host keeps the other operand)
    }
    if (!a.split) {
        for (int q = tid; q < n; q += 256) {
            const int c = q / a.taps, tap = q - c * a.taps;
            a.panel[(int64_t)o * a.Kpad + tap * a.cin_p + c] = (float)((double)a.w[row + q] * sc);
        }
        return;
    }
    smax[tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) smax[tid] = max(smax[tid], smax[tid + s]);
        __syncthreads();
    }
    mx = smax[0];
    // frexp(mx) = (f, ex), f in [0.5, 1): ex = floor(log2 mx) + 1; e = 13 - ex.  A subnormal maximum gives e > 40 either way
    int e = 0;
    if (mx != 0) e = 12 - ((int)(mx >> 52) - 1023);
    e = max(-24, min(40, e));
    const float ps = __uint_as_float((uint32_t)(127 + e) << 23);            // 2^e
    if (tid == 0) a.inv[o] = __uint_as_float((uint32_t)(127 - e - 3) << 23); // 2^-e / 8 (ACT_SCALE_F16S3 = 8)
    for (int q = tid; q < n; q += 256) {
        const int c = q / a.taps, tap = q - c * a.taps;
        const float fv = (float)((double)a.w[row + q] * sc);        // the fp32 folded weight
        const float vs = fv * ps;                                   // one rounding, as (float)((double)fv * 2^e): exact but for subnormal results
        const uint16_t h = f32_to_f16_rn(vs);
        const float rest = vs - f16_to_f32(h);
        const int64_t idx = ((int64_t)((c >> 5) * a.taps + tap) * a.Npad + o) * 32 + (c & 31);
        a.hi[idx] = h;
        a.lo[idx] = f32_to_f16_rn(rest);
    }
}

static_assert(ACT_SCALE_F16S3 == 8.0f, "head_step_kernel builds 2^-e / ACT_SCALE_F16S3 from the exponent");

int launch_head_step(const HeadStepLaunch& h, hipStream_t s) {
    hipLaunchKernelGGL(head_step_kernel, dim3((unsigned)(h.cout + (h.b || h.gamma ? 1 : 0))), dim3(256), 0, s, h);   // no extra workgroup for a frozen-BatchNorm conv
    return hip_fail(hipGetLastError(), "head_step launch");
}

}  // namespace rtod
