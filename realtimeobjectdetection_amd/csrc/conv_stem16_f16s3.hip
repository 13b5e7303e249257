// 16-filter stem (first layer: 3x3, stride 1, pad 1, Cin = 3, Cout = 16; YOLOv3-tiny) in the split-f16 arithmetic of
// conv_stem_split_kernel (conv_stem.hip), optionally with the 2x2 / stride-2 max-pool that follows it fused into the
// epilogue (plan option "stem_pool").  Reads the network input in NCHW directly; x*8 = xh + xl, w*2^e = wh + wl with the
// [Cout][32] hi / lo / inv_scale packing of the 32- and 64-filter split stem; one K = 32 step of three
// v_mfma_f32_16x16x32_f16 per 16-row tile (acc = xl*wh + xh*wl + xh*wh).
//
// One wave iteration = 64 convolution rows = four 16x16 tiles against the one 16-channel B fragment pair held in registers.
//   POOL = false: row r of the iteration is output pixel 64 t + r.
//   POOL = true:  row r of tile i is pooled pixel 16 t + 4 i + r / 4 at window position r % 4, (dy, dx) = (pos >> 1, pos & 1).
//                 The D fragment gives lane l channel l % 16 and rows 4 (l / 16) + e: the four values of one pooling window
//                 are the four accumulator elements of one lane, so the pool is in-register, no LDS or cross-lane traffic.
// Pool rule = stem + maxpool_split_kernel (aux_kernels.hip), bit for bit: every window value is split (saturation and range
// flag included), the window is scanned in (dy, dx) order on hi + lo (plain-f16 plans: on hi) and a pair replaces the held
// one only when strictly greater.
// The (hi, lo) pairs go through LDS as one dword per (pixel, channel), and every lane stores 16-byte row-contiguous pieces:
// [hi c0-7][hi c8-15][lo c0-7][lo c8-15] per pixel, 1 KiB contiguous per store instruction of the wave when ldc == 16.
// Plain-f16 plans never read a lo plane, so its pieces are not stored there.  Nothing depends on the batch size.
#include "conv_f16s3_common.h"

namespace rtod {

struct Stem16Args {
    const float* x; const _Float16* wh; const _Float16* wl; const float* inv_scale; const float* bias;
    _Float16* out; int64_t out_ldc; int out_coff;
    int B, H, W, Ho, Wo;              // Ho x Wo: the written map (pooled when POOL)
    int act, f16;
    unsigned x_bytes;
    int32_t* ovf;
};

constexpr int STEM16_NT = 4;          // 16-row tiles per wave iteration
constexpr int STEM16_TS = 20;         // dwords per pixel row of the LDS transpose (16 channels + 4: 16-byte aligned, conflict-free b128 reads)

template <bool POOL>
__global__ __launch_bounds__(256)
void conv_stem16_kernel(const Stem16Args a) {
    constexpr int NT = STEM16_NT, TS = STEM16_TS;
    constexpr int NP = POOL ? NT * 4 : NT * 16;                        // pixels written per wave iteration
    __shared__ __attribute__((aligned(16))) unsigned T[4][NP * TS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 15, lh = lane >> 4;
    const int hw = a.Ho * a.Wo;
    const int M = a.B * hw;
    const int64_t plane = (int64_t)a.H * a.W;
    unsigned* Tw = T[wave];
    const __amdgpu_buffer_rsrc_t rs_x = buffer_rsrc(a.x, a.x_bytes);
    // tap geometry of the lane's 8 k values, folded once (see conv_stem_split_kernel)
    int koff[8], need[8];
    float amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = lh * 8 + e;                                  // 0..31, k = (ky*3+kx)*3 + c
        const int tap = k / 3, c = k - tap * 3;
        const int ky = tap / 3, kx = tap - ky * 3;
        koff[e] = (c * (int)plane + ky * a.W + kx) * 4;
        need[e] = (ky == 0 ? 1 : 0) | (ky == 2 ? 2 : 0) | (kx == 0 ? 4 : 0) | (kx == 2 ? 8 : 0) | (k >= 27 ? 16 : 0) | 32;
    }
    const f16x8 bh = *reinterpret_cast<const f16x8*>(a.wh + lr * 32 + lh * 8);
    const f16x8 bl = *reinterpret_cast<const f16x8*>(a.wl + lr * 32 + lh * 8);
    const float inv = a.inv_scale[lr], bias = a.bias[lr];

    auto gather = [&](int tile, float (&av)[NT][8]) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int m = POOL ? tile * NP + i * 4 + (lr >> 2) : tile * NP + i * 16 + lr;
            const bool mok = m < M;
            const int mm = mok ? m : 0;
            const int b = mm / hw, r = mm - b * hw;
            int oy = r / a.Wo, ox = r - oy * a.Wo;
            if (POOL) { oy = 2 * oy + ((lr >> 1) & 1); ox = 2 * ox + (lr & 1); }
            const int iy0 = oy - 1, ix0 = ox - 1;
            const int edge = (iy0 < 0 ? 1 : 0) | (iy0 + 2 >= a.H ? 2 : 0) | (ix0 < 0 ? 4 : 0) | (ix0 + 2 >= a.W ? 8 : 0) | 16 | (mok ? 0 : 32);
            const int base = (b * 3 * (int)plane + iy0 * a.W + ix0) * 4;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned vo = (need[e] & edge) ? 0x80000000u : (unsigned)(base + koff[e]);
                av[i][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_x, vo, 0, 0));
            }
        }
    };
    auto pack = [](_Float16 h, _Float16 l) {
        return (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
    };

    const int tstep = gridDim.x * 4;
    int tile = blockIdx.x * 4 + wave;
    float av[NT][8], an[NT][8];
    if ((int64_t)tile * NP < M) gather(tile, av);
    for (; (int64_t)tile * NP < M; tile += tstep) {
        if ((int64_t)(tile + tstep) * NP < M) gather(tile + tstep, an);        // wave-uniform
        f32x4 acc[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            f16x8 ah, al;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = av[i][e] * SPLIT_SCALE;
                const _Float16 h = (_Float16)v;
                ah[e] = h; al[e] = (_Float16)(v - (float)h);
            }
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
            acc[i] = c;
        }
        // D: col = lane%16 (channel), row = 4*(lane/16) + e
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            float best = -INFINITY;
            _Float16 mh = (_Float16)0.f, ml = (_Float16)0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = apply_act(__builtin_fmaf(acc[i][e], inv, bias), a.act);
                _Float16 h, l;
                split_f16(v * SPLIT_SCALE, h, l, amax);
                if (POOL) {
                    const float s = a.f16 ? (float)h : (float)h + (float)l;
                    if (s > best) { best = s; mh = h; ml = l; }
                } else
                    Tw[(i * 16 + 4 * lh + e) * TS + lr] = pack(h, l);
            }
            if (POOL) Tw[(i * 4 + lh) * TS + lr] = pack(mh, ml);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the wave's own LDS writes, then reads (in order)
        __builtin_amdgcn_wave_barrier();
        // NP pixels x 4 pieces of 16 bytes (hi c0-7, hi c8-15, lo c0-7, lo c8-15)
#pragma unroll
        for (int q = 0; q < NP * 4 / 64; ++q) {
            const int g = lane + q * 64;
            const int p = g >> 2, chunk = g & 1, lo = (g >> 1) & 1;
            const int mo = tile * NP + p;
            const u32x4 d0 = *reinterpret_cast<const u32x4*>(Tw + p * TS + chunk * 8);
            const u32x4 d1 = *reinterpret_cast<const u32x4*>(Tw + p * TS + chunk * 8 + 4);
            u32x4 pk;
            if (lo) pk = u32x4{(d0[0] >> 16) | (d0[1] & 0xFFFF0000u), (d0[2] >> 16) | (d0[3] & 0xFFFF0000u),
                               (d1[0] >> 16) | (d1[1] & 0xFFFF0000u), (d1[2] >> 16) | (d1[3] & 0xFFFF0000u)};
            else pk = u32x4{(d0[0] & 0xFFFFu) | (d0[1] << 16), (d0[2] & 0xFFFFu) | (d0[3] << 16),
                            (d1[0] & 0xFFFFu) | (d1[1] << 16), (d1[2] & 0xFFFFu) | (d1[3] << 16)};
            if (mo < M && !(lo && a.f16)) {
                _Float16* o = a.out + (int64_t)mo * 2 * a.out_ldc + a.out_coff + chunk * 8 + (lo ? a.out_ldc : 0);
                store_act16(o, __builtin_bit_cast(f16x8, pk), false);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) av[i][e] = an[i][e];
    }
    split_overflow_report(a.ovf, amax);
}

bool conv_stem16_supported(int ksize, int stride, int pad, int cin, int cout, int act) {
    return ksize == 3 && stride == 1 && pad == 1 && cin == 3 && cout == 16 && act >= 0 && act <= 2;
}

// out: layer 0's view (pool == 0: H x W) or the view of the 2x2 / stride-2 max-pool that follows it (pool == 1: H/2 x W/2, H and W even)
int launch_conv_stem16_f16s3(const float* x, const _Float16* wh, const _Float16* wl, const float* inv_scale, const float* bias,
                             const View& out, int B, int H, int W, int act, int pool, int32_t* ovf, hipStream_t s) {
    if (!x || !wh || !wl || !inv_scale || !bias || !out.base) { set_error("conv_stem16: null pointer"); return RTOD_E_ARG; }
    if (B < 1 || H < 1 || W < 1 || act < 0 || act > 2) { set_error("conv_stem16: bad geometry / activation"); return RTOD_E_ARG; }
    if (pool && (H % 2 || W % 2)) { set_error("conv_stem16: fused 2x2 max-pool needs an even input, got %dx%d", H, W); return RTOD_E_ARG; }
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    if (out.C != 16 || out.H != Ho || out.W != Wo || out.ldc < out.coff + 16 || out.ldc % 8 || out.coff % 8 || out.coff < 0 || (out.split != 1 && out.split != 2)) {
        set_error("conv_stem16: bad output view"); return RTOD_E_ARG;
    }
    if ((int64_t)B * H * W >= (1ll << 31) || (int64_t)B * 3 * H * W * 4 >= (1ll << 31)) { set_error("conv_stem16: input exceeds 2 GiB / int32 pixels"); return RTOD_E_ARG; }
    Stem16Args a;
    a.x = x; a.wh = wh; a.wl = wl; a.inv_scale = inv_scale; a.bias = bias;
    a.out = reinterpret_cast<_Float16*>(out.base); a.out_ldc = out.ldc; a.out_coff = out.coff;
    a.B = B; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.act = act; a.f16 = out.split == 2 ? 1 : 0;
    a.x_bytes = (unsigned)((int64_t)B * 3 * H * W * 4);
    a.ovf = ovf;
    const int np = pool ? STEM16_NT * 4 : STEM16_NT * 16;
    const int64_t tiles = ((int64_t)B * Ho * Wo + np - 1) / np;
    int grid = (int)((tiles + 3) / 4);
    if (grid > 2048) grid = 2048;                                      // larger maps: several tiles per wave, the next one's input in flight
    if (pool) hipLaunchKernelGGL(conv_stem16_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(conv_stem16_kernel<false>, dim3(grid), dim3(256), 0, s, a);
    return hip_fail(hipGetLastError(), "conv_stem16 launch");
}

// ---------------------------------------------------------------------------------------------
// Raw-sum instance of the non-pooling kernel (plan options bn_batch_split + bn_split_narrow + stem_pool): batch-statistics BatchNorm
// on layer 0.  The weights are packed unfolded, so acc * inv_scale IS the convolution sum; it is stored as fp32 rows of `ld` floats —
// no bias, no activation, no split store, no overflow sentinel: the normalise kernel that follows (aux_kernels.hip) writes the split
// format.  A kernel of its own, so that conv_stem16_kernel's instances stay as they are compiled today; same gather, same three
// products, same LDS transpose (one dword per (pixel, channel)), four 16-byte pieces of 4 channels per pixel.
struct Stem16RawArgs {
    const float* x; const _Float16* wh; const _Float16* wl; const float* inv_scale;
    float* raw; int64_t ld;            // rows of `ld` floats (>= 16, multiple of 4), one per pixel
    int B, H, W;
    unsigned x_bytes;
};

__global__ __launch_bounds__(256)
void conv_stem16_raw_kernel(const Stem16RawArgs a) {
    constexpr int NT = STEM16_NT, TS = STEM16_TS;
    constexpr int NP = NT * 16;                                        // pixels written per wave iteration
    __shared__ __attribute__((aligned(16))) float T[4][NP * TS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 15, lh = lane >> 4;
    const int hw = a.H * a.W;
    const int M = a.B * hw;
    float* Tw = T[wave];
    const __amdgpu_buffer_rsrc_t rs_x = buffer_rsrc(a.x, a.x_bytes);
    int koff[8], need[8];                                              // tap geometry of the lane's 8 k values (conv_stem16_kernel)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = lh * 8 + e;                                  // 0..31, k = (ky*3+kx)*3 + c
        const int tap = k / 3, c = k - tap * 3;
        const int ky = tap / 3, kx = tap - ky * 3;
        koff[e] = (c * hw + ky * a.W + kx) * 4;
        need[e] = (ky == 0 ? 1 : 0) | (ky == 2 ? 2 : 0) | (kx == 0 ? 4 : 0) | (kx == 2 ? 8 : 0) | (k >= 27 ? 16 : 0) | 32;
    }
    const f16x8 bh = *reinterpret_cast<const f16x8*>(a.wh + lr * 32 + lh * 8);
    const f16x8 bl = *reinterpret_cast<const f16x8*>(a.wl + lr * 32 + lh * 8);
    const float inv = a.inv_scale[lr];

    auto gather = [&](int tile, float (&av)[NT][8]) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int m = tile * NP + i * 16 + lr;
            const bool mok = m < M;
            const int mm = mok ? m : 0;
            const int b = mm / hw, r = mm - b * hw;
            const int oy = r / a.W, ox = r - oy * a.W;
            const int iy0 = oy - 1, ix0 = ox - 1;
            const int edge = (iy0 < 0 ? 1 : 0) | (iy0 + 2 >= a.H ? 2 : 0) | (ix0 < 0 ? 4 : 0) | (ix0 + 2 >= a.W ? 8 : 0) | 16 | (mok ? 0 : 32);
            const int base = (b * 3 * hw + iy0 * a.W + ix0) * 4;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned vo = (need[e] & edge) ? 0x80000000u : (unsigned)(base + koff[e]);
                av[i][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_x, vo, 0, 0));
            }
        }
    };

    const int tstep = gridDim.x * 4;
    int tile = blockIdx.x * 4 + wave;
    float av[NT][8], an[NT][8];
    if ((int64_t)tile * NP < M) gather(tile, av);
    for (; (int64_t)tile * NP < M; tile += tstep) {
        if ((int64_t)(tile + tstep) * NP < M) gather(tile + tstep, an);        // wave-uniform
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            f16x8 ah, al;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = av[i][e] * SPLIT_SCALE;
                const _Float16 h = (_Float16)v;
                ah[e] = h; al[e] = (_Float16)(v - (float)h);
            }
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, c, 0, 0, 0);
            // D: col = lane%16 (channel), row = 4*(lane/16) + e
#pragma unroll
            for (int e = 0; e < 4; ++e) Tw[(i * 16 + 4 * lh + e) * TS + lr] = c[e] * inv;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the wave's own LDS writes, then reads (in order)
        __builtin_amdgcn_wave_barrier();
        // NP pixels x 4 pieces of 16 bytes (channels 0-3, 4-7, 8-11, 12-15)
#pragma unroll
        for (int q = 0; q < NP * 4 / 64; ++q) {
            const int g = lane + q * 64;
            const int p = g >> 2, piece = g & 3;
            const int mo = tile * NP + p;
            const f32x4 d = *reinterpret_cast<const f32x4*>(Tw + p * TS + piece * 4);
            if (mo < M) *reinterpret_cast<f32x4*>(a.raw + (int64_t)mo * a.ld + piece * 4) = d;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) av[i][e] = an[i][e];
    }
}

// raw: fp32 view H x W over the raw-sum scratch, C = 16, coff 0, rows of raw.ldc floats
int launch_conv_stem16_raw(const float* x, const _Float16* wh, const _Float16* wl, const float* inv_scale, const View& raw, int B, int H, int W, hipStream_t s) {
    if (!x || !wh || !wl || !inv_scale || !raw.base) { set_error("conv_stem16(raw): null pointer"); return RTOD_E_ARG; }
    if (B < 1 || H < 1 || W < 1) { set_error("conv_stem16(raw): bad geometry"); return RTOD_E_ARG; }
    if (raw.split || raw.C != 16 || raw.H != H || raw.W != W || raw.ldc < 16 || raw.ldc % 4 || raw.coff != 0) { set_error("conv_stem16(raw): bad raw-sum view"); return RTOD_E_ARG; }
    if ((int64_t)B * H * W >= (1ll << 31) || (int64_t)B * 3 * H * W * 4 >= (1ll << 31)) { set_error("conv_stem16(raw): input exceeds 2 GiB / int32 pixels"); return RTOD_E_ARG; }
    Stem16RawArgs a;
    a.x = x; a.wh = wh; a.wl = wl; a.inv_scale = inv_scale;
    a.raw = raw.base; a.ld = raw.ldc;
    a.B = B; a.H = H; a.W = W;
    a.x_bytes = (unsigned)((int64_t)B * 3 * H * W * 4);
    const int64_t tiles = ((int64_t)B * H * W + STEM16_NT * 16 - 1) / (STEM16_NT * 16);
    int grid = (int)((tiles + 3) / 4);
    if (grid > 2048) grid = 2048;                                      // larger maps: several tiles per wave, the next one's input in flight
    hipLaunchKernelGGL(conv_stem16_raw_kernel, dim3(grid), dim3(256), 0, s, a);
    return hip_fail(hipGetLastError(), "conv_stem16(raw) launch");
}

}  // namespace rtod
