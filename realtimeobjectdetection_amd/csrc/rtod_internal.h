// Internal declarations shared by the kernels, the plan and the C ABI (not installed).
#pragma once
#include <hip/hip_runtime.h>
// Diagnostic builds (never the product library): -DRTOD_STAMPS = in-kernel s_memtime phase attribution (synchronises after
// every launch), -DRTOD_DIAG = the RTOD_DBG_ZERO timing knobs alone (zero-record descriptors, skipped epilogue); stamps imply diag.
#if defined(RTOD_STAMPS) && !defined(RTOD_DIAG)
#define RTOD_DIAG 1
#endif
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/rtod.h"

namespace rtod {

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define RTOD_HIP(expr)                                              \
    do {                                                            \
        hipError_t _e = (expr);                                     \
        if (_e != hipSuccess) return ::rtod::hip_fail(_e, #expr);   \
    } while (0)

// More than 64 KiB of dynamic LDS needs a per-kernel opt-in, made once per device: `done` is the calling instantiation's own
// static word, one bit per device.  Idempotent: two threads may both make the calls.  Error texts start with `who`.
template <typename... Kernel>
int lds_opt_in(std::atomic<unsigned long long>& done, int bytes, const char* who, Kernel... kernels) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hip_fail(hipGetLastError(), (std::string(who) + " hipGetDevice").c_str());
    if ((done.load(std::memory_order_acquire) >> (dev & 63)) & 1ull) return RTOD_OK;
    for (const void* k : {reinterpret_cast<const void*>(kernels)...})
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
            return hip_fail(hipGetLastError(), (std::string(who) + " LDS attribute").c_str());
    done.fetch_or(1ull << (dev & 63), std::memory_order_release);
    return RTOD_OK;
}

// compute units of the current device (persistent grids are sized by it); 0 if the query fails
inline int device_cu_count() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
}

// NHWC view of an activation: element (b,y,x,c) at base[((b*H + y)*W + x)*ldc + coff + c]
struct View {
    int split = 0;     // 0: fp32 NHWC; 1: split f16 hi/lo planes per pixel (conv_igemm_f16s3.hip), same bytes;
                       // 2: the same layout, hi plane only (plain f16, precision mode 2: the lo plane is never written or read)
    float* base = nullptr;
    int64_t ldc = 0;   // floats between consecutive pixels (>= C: concat buffers are wider)
    int coff = 0;      // first channel of this view inside the pixel
    int C = 0, H = 0, W = 0;
};

// Fused YOLO head decode (reference: src/util.py:193-237) applied in a conv epilogue or by the
// stand-alone kernel.
struct DecodeArgs {
    int enabled = 0;
    int GH = 0, GW = 0;      // grid rows / columns (square plans: GH == GW == G); rows r = (gy * GW + gx) * A + a
    int attrs = 0;           // 5 + classes
    int n_anchors = 0;
    int train = 0;           // TRAIN=True: sigmoids only
    int v5 = 0;              // cfg extension `[yolo] decode=v5` (YOLOv5-style heads): xy = (2 s - 0.5 + g) * stride, wh = (2 s)^2 * anchor
                             // (aw / ah then hold the anchors in PIXELS), everything else sigmoid; not reference behaviour
    float stride = 0.f;      // inp_dim // G: one integer stride, the same along both axes (checked at plan build)
    float aw[4] = {0, 0, 0, 0};   // fp32(anchor_w / stride)
    float ah[4] = {0, 0, 0, 0};
    int64_t img_stride = 0;  // total_rows * attrs
    int64_t head_off = 0;    // row_offset * attrs
};

struct ConvArgs {
    const float* in = nullptr;  int64_t in_ldc = 0;  int in_coff = 0;
    int B = 0, Hi = 0, Wi = 0, Cin = 0;        // Cin = stored channels of the input view
    const float* w = nullptr;                   // packed [Npad][Kpad], k = (ky*kw+kx)*Cin + c
    const float* bias = nullptr;                // [Npad]
    int K = 0, Kpad = 0;
    int Npad = 0;                               // split path: rows of one K-chunk panel of the weight planes ([Kpad/32][Npad][32] f16)
    int kh = 1, kw = 1, stride = 1, pad = 0;
    int Ho = 0, Wo = 0, Cout = 0;
    float* out = nullptr;       int64_t out_ldc = 0; int out_coff = 0;
    const float* res = nullptr; int64_t res_ldc = 0; int res_coff = 0;   // fused shortcut
    int leaky = 0;                              // activation code: 0 linear, 1 leaky(0.1), 2 SiLU (apply_act)
    DecodeArgs dec;
    // split-precision path (conv_igemm_f16s3): pre-split, pre-scaled f16 weight planes [Npad][Kpad]
    // Weight planes are K-chunk major: [Kpad/32 chunks][Npad rows][32 halves], chunk kc = (c/32)*kh*kw + tap.  One (chunk, tap)
    // stage of a tile is then BN consecutive 64-byte rows: contiguous, full 128-byte lines (row-major [Npad][Kpad] planes made every
    // stage BN separate 64-byte pieces at a stride of Kpad*2 bytes: half-line requests, twice the address traffic for the same bytes)
    const _Float16* w_hi = nullptr;
    const _Float16* w_lo = nullptr;
    const float* inv_scale = nullptr;           // [Npad]: 1 / (2^e_n * SPLIT_SCALE)
    unsigned in_bytes = 0, w_bytes = 0;         // extents of the input buffer / one weight plane (buffer-load range check)
    int dbg = 0;                                // timing experiments, diagnostic build only (-DRTOD_STAMPS reads RTOD_DBG_ZERO); the product library never sets or reads it
    int32_t* ovf = nullptr;                     // split-format producers: device word that gets 1 OR-ed in when an activation saturates the f16 range
    int xcd_by_n = 0;                           // split kernels: workgroup -> XCD by output-channel tile instead of by pixel tile (see launch_band)
    int out_split = 0;                          // exact-fp32 kernel only: write the output in the split format
    int f16 = 0;                                // split kernels: 1 = plain-f16 instance (precision mode 2: hi planes only, one MFMA per fragment pair)
    float* raw_out = nullptr;                   // split kernels, raw-sum instances (EPI_RAW; plan option bn_batch_split): acc * inv_scale[n] as fp32 rows [M][raw_ld];
                                                // no bias, activation, shortcut or split store (`out` is not written)
    int raw_ld = 0;                             // ... floats between consecutive rows of raw_out, read by the shared epilogue of the generic and narrow tiles: Npad, or (narrow
                                                // tiles, plan option bn_split_narrow) Cout rounded up to 8.  The bandd and 1x1 slab instances write rows of Npad and refuse another value
    // exact-fp32 kernel and the K-sliced split family (conv_ks_f16s3.hip): K slices (conv_igemm_f32.hip).  slice_chunks > 0: the K sum is formed slice by slice (a property of
    // the layer); partial != nullptr: one workgroup per slice, raw sums to this scratch ([slices][M][Npad] floats), then a reduction
    int slice_chunks = 0;
    float* partial = nullptr;
    int64_t partial_floats = 0;
    // split path, fused trailing 1x1 conv ("pointwise", conv_f16s3_common.h): the workgroup holds every channel of its
    // output pixels (Cout <= BN), so the next layer's 1x1 convolution runs as a second small GEMM in the epilogue
    const _Float16* pw_wh = nullptr;            // [pw_cout..][pw_k] hi / lo planes of the 1x1 conv (its own packed weights)
    const _Float16* pw_wl = nullptr;
    const float* pw_inv_scale = nullptr;
    const float* pw_bias = nullptr;
    float* pw_out = nullptr;    int64_t pw_out_ldc = 0; int pw_out_coff = 0;
    int pw_npad = 0;                            // Npad of the hosted 1x1 conv's weight planes
    int pw_cout = 0, pw_k = 0, pw_leaky = 0;    // pw_k = Cout of this conv = Kpad of the 1x1 (32 or 64); pw_cout 16, 32 or 64
};

// Split activation format: value * SPLIT_SCALE stored as f16 hi + f16 lo planes per pixel.
constexpr float SPLIT_SCALE = 8.0f;
constexpr float ACT_SCALE_F16S3 = SPLIT_SCALE;
constexpr float F16_MAX = 65504.0f;

#ifdef __HIPCC__
// the 16-byte vectors every kernel moves: 4 floats of an fp32 pixel, 8 halves of one plane of a split-f16 pixel
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// v (already x SPLIT_SCALE) -> hi + lo.  Saturates at the f16 range instead of producing inf (inf + -inf = NaN in the
// next layer); `amax` tracks max|v| for the overflow sentinel (split_overflow_report).
__device__ __forceinline__ void split_f16(float v, _Float16& h, _Float16& l, float& amax) {
    amax = fmaxf(amax, fabsf(v));
    const float vc = __builtin_amdgcn_fmed3f(v, -F16_MAX, F16_MAX);
    h = (_Float16)vc;
    l = (_Float16)(vc - (float)h);
}
// Plain-f16 store (precision mode 2): the hi half of split_f16, alone — RNE_f16 of the saturated value, same overflow sentinel.
__device__ __forceinline__ _Float16 f16_sat(float v, float& amax) {
    amax = fmaxf(amax, fabsf(v));
    return (_Float16)__builtin_amdgcn_fmed3f(v, -F16_MAX, F16_MAX);
}
// Activation of a conv epilogue: 0 linear, 1 leaky(0.1) (src/darknet.py:497-501), 2 SiLU x * sigmoid(x) (cfg extension).
// Exact-fp32 kernels and the stems; the split-f16 epilogues have their own form (conv_f16s3_common.h: silu_scaled behind a
// uniform branch around the loops of the LDS-transposed epilogue).
__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == 1) return v > 0.f ? v : v * 0.1f;
    if (act == 2) return v / (1.0f + expf(-v));
    return v;
}
__device__ __forceinline__ void split_overflow_report(int32_t* flag, float amax) {
    if (flag && !(amax <= F16_MAX)) atomicOr(flag, 1);        // also true for NaN
}
// Raw buffer descriptor of `bytes` bytes at p: stride 0, descriptor word 3 = 0x00020000 (32-bit data format).  A buffer load
// at voffset >= bytes returns zeros and an LDS-DMA piece writes zeros: the kernels send padding and tail lanes out of range.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
// XCD-aware bijective remap of a workgroup or tile index id in [0, n): the dispatcher deals consecutive indices round-robin
// over the 8 XCDs, and XCD x = id % 8 takes the x-th contiguous range of the result, so neighbouring tiles (which share an
// operand panel) share one L2.
__device__ __forceinline__ int xcd_remap(int id, int n) {
    const int q = n >> 3, r = n & 7, xcd = id & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
}
#endif

// epilogue-code flag of the plain-f16 kernel instances (precision mode 2): EPI | EPI_F16 (conv_f16s3_common.h)
constexpr int EPI_F16 = 8;
// epilogue-code flag of the raw-sum instances (batch-statistics BatchNorm on the split kernels, plan option bn_batch_split):
// EPI_SPLIT | EPI_RAW.  Generic, bandd, 1x1 slab and narrow tiles (the raw column of the family table)
constexpr int EPI_RAW = 16;

enum ConvVariant { CV_128x128 = 0, CV_128x64 = 1, CV_64x64 = 2, CV_128x32 = 3, CV_COUNT };
struct ConvVariantInfo { int bm, bn; const char* name; };
const ConvVariantInfo& conv_variant_info(int v);
int conv_f32_kernel_name(int variant, char* buf, size_t len);
int launch_conv(const ConvArgs& a, int variant, hipStream_t s);
int conv_f32_slices(const ConvArgs& a);                                       // K slices of an exact-fp32 launch (1: unsliced)
enum ConvF16Variant { HV_128x128 = 0, HV_128x64 = 1, HV_64x64 = 2, HV_64x128 = 3, HV_256x128 = 4, HV_128x256 = 5, HV_128x128_8W = 6, HV_128x64_8W = 7, HV_256x128_16W = 8,
                      HV_192x128_8W = 9, HV_96x128_8W = 10, HV_192x128_12W = 11, HV_COUNT };
const ConvVariantInfo& conv_f16s3_variant_info(int v);
int conv_f16s3_kernel_name(int variant, int epi, char* buf, size_t len);      // demangled instantiation name (rocprofv3)
int launch_conv_f16s3(const ConvArgs& a, int variant, hipStream_t s);
// The split-f16 tile families.  A tile id is family base + mode; the constants below give each family's range and mode-level
// facts.  split_tiles.cpp holds the one table of the ranges (TileFamily, family_of) and is, with this header, the only place
// that compares an id against a base or a mode count.  Which tile a launch may run, runs by default and times in autotune is
// decided in plan_tiles.cpp alone: Plan::tile_legal, Plan::default_tile, Plan::tile_candidates (variant_for / set_tiles /
// tune_launch / launch_split_variant all go through them and family_of).  A new family: its constants here, one row there,
// its rules in those three functions.
// 3x3 stride-1 pad-1 convs with an LDS-resident input band (conv_band_f16s3.hip); weights in band K order
bool conv_band_supported(int ksize, int stride, int pad, int cin, int w_in);
// A layer the band kernel supports ALWAYS runs on it (its split-K layers sum in a different order than the generic kernel, and
// a frame's output must not depend on the batch it rides in); autotune only picks the tile.
constexpr int BANDD_MODES = 9;             // conv_bandd_f16s3.hip (round 4): weight fragments straight from global memory, band by LDS-DMA
constexpr int BAND_LDS_MODES = 11;         // conv_band_f16s3.hip: 128x128/4x2 waves, 128x64/4x2, 192x128/4x2, 192x128/6x2, 96x128/2x4, 128x128/2x2, 64x128/2x4,
                                           // and with in-workgroup split-K (two wave groups): 96x128/2x4, 128x128/4x2, 64x128/2x4, 128x64/4x2 (13x13 grids)
constexpr int BAND_MODES = BAND_LDS_MODES + BANDD_MODES;
                                           // modes >= BAND_LDS_MODES: conv_bandd tile (mode - BAND_LDS_MODES)
constexpr int BAND_K2_MODE0 = 7;
const ConvVariantInfo& conv_bandd_mode_info(int idx);
int conv_bandd_mode_kg(int idx);
// the last bandd tile (one band buffer of up to 29 blocks, two workgroups per CU) also runs 3x3 stride-1 layers with 94 < W <= 160: same K
// order and MFMA sequence as the generic tiles, so it is one more autotune candidate of those (non-band) layers
constexpr int BANDD_WIDE_MODE = BAND_LDS_MODES + 7;       // band-family mode index -> variant BAND_VARIANT_BASE + BANDD_WIDE_MODE
bool conv_bandd_wide_supported(int ksize, int stride, int pad, int cin, int w_in);
int conv_bandd_kernel_name(int idx, int epi, char* buf, size_t len);
int launch_conv_bandd_f16s3(const ConvArgs& a, int idx, hipStream_t s);
int conv_band_layer_kg(int cin, int h, int w);
bool conv_band_mode_valid(int mode, int cin, int h, int w);
int conv_band_default_mode(int cin, int h, int w);
const ConvVariantInfo& conv_band_mode_info(int mode);
int conv_band_kernel_name(int mode, int epi, char* buf, size_t len);
int launch_conv_band_f16s3(const ConvArgs& a, int mode, hipStream_t s);
constexpr int BAND_VARIANT_BASE = 50;      // variant ids in [50, 70) select the band kernel: BAND_VARIANT_BASE + mode
// Persistent LDS-DMA ring kernel (conv_ring_f16s3.hip): same K order and MFMA sequence as the generic implicit GEMM, so
// its tiles are further autotune candidates for every layer the generic kernel runs (bit-identical results).
constexpr int RING_MODES = 8;
constexpr int RING_VARIANT_BASE = 70;      // variant ids >= this: RING_VARIANT_BASE + mode
const ConvVariantInfo& conv_ring_mode_info(int mode);
int conv_ring_kernel_name(int mode, int epi, char* buf, size_t len);
int launch_conv_ring_f16s3(const ConvArgs& a, int mode, hipStream_t s);
// 1x1 convolutions with the A operand staged in 64-channel slabs (full-line LDS-DMA) and weight fragments straight from global
// memory (conv_pwd_f16s3.hip, round 4): same K order and MFMA sequence as the generic / ring tiles -> further autotune candidates
// of the plain 1x1 layers (no fused decode, no hosted pointwise conv), bit-identical results.
constexpr int PWD_MODES = 11;
constexpr int PWD_VARIANT_BASE = 90;       // variant ids in [90, 110): PWD_VARIANT_BASE + mode
bool conv_pwd_supported(int ksize, int stride, int pad, int cin);
const ConvVariantInfo& conv_pwd_mode_info(int mode);
int conv_pwd_kernel_name(int mode, int epi, char* buf, size_t len);
int launch_conv_pwd_f16s3(const ConvArgs& a, int mode, hipStream_t s);
// Stem + first stride-2 convolution (+ hosted 1x1) in one persistent kernel (conv_stem2_f16s3.hip): the stem's output never
// leaves the CU.  Bit-identical to the stand-alone kernels.
constexpr int STEM2_VARIANT = 130;         // variant id reported for the fused launch
bool conv_stem2_supported(int k0, int s0, int p0, int cin0, int cout0, int k1, int s1, int p1, int cout1, int pw_cout);
int conv_stem2_kernel_name(int pw, char* buf, size_t len);
int launch_conv_stem2_f16s3(const float* x, int B, int H, int W, const _Float16* w0h, const _Float16* w0l, const float* inv0, const float* bias0,
                            int leaky0, const ConvArgs& c1, hipStream_t s);
// 2-D tiled 3x3 stride-1 kernel with an LDS-resident input patch (conv_patch_f16s3.hip): for images too wide for the band
// kernel; bit-identical to the generic / ring tiles, so its modes are further autotune candidates of those layers.
constexpr int PATCH_MODES = 5;
constexpr int PATCH_WRES_MODE = 4;         // weights resident in LDS (Cin = 32, Cout = 64 only)
bool conv_patch_mode_valid(int mode, int cin, int cout);
constexpr int PATCH_VARIANT_BASE = 110;    // variant ids >= this: PATCH_VARIANT_BASE + mode
bool conv_patch_supported(int ksize, int stride, int pad, int cin, int cout);
const ConvVariantInfo& conv_patch_mode_info(int mode);
int conv_patch_kernel_name(int mode, int epi, char* buf, size_t len);
int launch_conv_patch_f16s3(const ConvArgs& a, int mode, hipStream_t s);

// Convolutions that read 16 input channels (conv_c16_f16s3.hip; plan option "narrow_cin"): K order tap-major over 16 channels
// (k = tap * 16 + c, a 32-wide K-chunk holds two taps), its own packed weights, so a narrow layer ALWAYS runs on this family and
// no other layer does.  All tiles are bit-identical; f16s3 and plain-f16 instances, epilogues 0 / 1 / 2; raw-sum instances (epilogue 16).
constexpr int C16_MODES = 4;
constexpr int C16_VARIANT_BASE = 140;      // variant ids in [140, 140 + C16_MODES): C16_VARIANT_BASE + mode
constexpr bool conv_c16_supported(int cin) { return cin == 16; }
const ConvVariantInfo& conv_c16_mode_info(int mode);
int conv_c16_default_mode(int cout, int64_t m);                               // m = batch * Ho * Wo
int conv_c16_kernel_name(int mode, int epi, char* buf, size_t len);
int launch_conv_c16_f16s3(const ConvArgs& a, int mode, hipStream_t s);

// K-sliced generic tiles (conv_ks_f16s3.hip; plan option "k_slices_split"): the K sum of a deep small-grid layer formed in slices
// of ConvArgs::slice_chunks K-chunks, added in ascending order.  That summation order differs from every other family's, so a
// sliced layer ALWAYS runs on this family and no other layer does.  Mode = 2 * tile + schedule: schedule 0 walks the slices inside
// the workgroup, schedule 1 gives every (tile, slice) its own workgroup (raw sums to ConvArgs::partial, then a reduction kernel,
// both under one launch entry).  All modes are bit-identical; f16s3 and plain-f16 instances, epilogues 0 / 1.
constexpr int KS_TILES = 3;
constexpr int KS_MODES = 2 * KS_TILES;
constexpr int KS_VARIANT_BASE = 150;       // variant ids in [150, 150 + KS_MODES): KS_VARIANT_BASE + mode
constexpr int64_t KS_SCRATCH_FLOATS = 8ll << 20;   // Plan::d_scratch: 32 MB of slice panels (L2 / Infinity-Cache resident)
const ConvVariantInfo& conv_ks_mode_info(int mode);
int conv_ks_slices(const ConvArgs& a);                                        // K slices of a launch of this family
int conv_ks_kernel_name(int mode, int epi, char* buf, size_t len);
int launch_conv_ks_f16s3(const ConvArgs& a, int mode, hipStream_t s);

// One row per id range (split_tiles.cpp), in ascending base order.  STEM2_VARIANT is a reported id only and has no row.
enum TileFamilyId { TF_GENERIC = 0, TF_BAND, TF_RING, TF_PWD, TF_PATCH, TF_C16, TF_KS, TF_COUNT };
struct TileFamily {
    int id, base, modes;
    int f16_from;                                                   // modes >= this have a plain-f16 instance (== modes: none has)
    int raw_from;                                                   // modes >= this have a raw-sum instance (EPI_RAW; == modes: none has)
    const ConvVariantInfo& (*info)(int mode);
    int (*kernel_name)(int mode, int epi, char* buf, size_t len);
    int (*launch)(const ConvArgs& a, int mode, hipStream_t s);
};
struct TileRef {                                                    // a tile id resolved: its family's row and the mode (fam == nullptr: no such tile)
    const TileFamily* fam; int mode;
    explicit operator bool() const { return fam != nullptr; }
    bool is(int family) const { return fam && fam->id == family; }
    bool f16() const { return fam && mode >= fam->f16_from; }
    bool raw() const { return fam && mode >= fam->raw_from; }
    bool ks_sched_b() const { return is(TF_KS) && (mode & 1); }    // one workgroup per (tile, slice); id - 1 is schedule A of the same tile
    bool bandd_wide() const { return is(TF_BAND) && mode == BANDD_WIDE_MODE; }
};
TileRef family_of(int v);
const TileFamily& tile_family(int family);
inline int tile_id(int family, int mode) { return tile_family(family).base + mode; }

int launch_conv_stem(const float* x_nchw, const float* w, const float* bias, const View& out, int B, int H, int W,
                     int Ho, int Wo, int stride, int Cout, int leaky, hipStream_t s);
int launch_conv_stem_split(const float* x_nchw, const _Float16* wh, const _Float16* wl, const float* inv_scale, const float* bias,
                           const View& out, int B, int H, int W, int Ho, int Wo, int stride, int Cout, int leaky, int32_t* ovf, hipStream_t s);
// 16-filter stem in the split-f16 arithmetic, stand-alone or with the following 2x2 / stride-2 max-pool fused (conv_stem16_f16s3.hip;
// plan option "stem_pool").  pool == 1: `out` is the pool's view (H/2 x W/2); bit-identical to pool == 0 followed by launch_maxpool.
bool conv_stem16_supported(int ksize, int stride, int pad, int cin, int cout, int act);
int launch_conv_stem16_f16s3(const float* x_nchw, const _Float16* wh, const _Float16* wl, const float* inv_scale, const float* bias,
                             const View& out, int B, int H, int W, int act, int pool, int32_t* ovf, hipStream_t s);
// ... its raw-sum instance (plan options bn_batch_split + bn_split_narrow + stem_pool): acc * inv_scale as fp32 rows of raw.ldc floats
int launch_conv_stem16_raw(const float* x_nchw, const _Float16* wh, const _Float16* wl, const float* inv_scale, const View& raw, int B, int H, int W, hipStream_t s);
int launch_prep_image(const unsigned char* img, int h, int w, int bgr, int inp_dim, float* out, hipStream_t s);
int launch_prep_frames(const unsigned char* frames, int batch, int h, int w, int bgr, int out_h, int out_w, float* out, hipStream_t s);
int launch_pack_input(const float* x_nchw, int B, int C, int H, int W, float* out_nhwc, int Cp, hipStream_t s);
// The elementwise helpers (aux_kernels.hip): one kernel template per op over the activation format.  All views of a call share one
// View::split (0 fp32, 1 split f16, 2 plain f16; launch_copy: fp32 only) and pass the file's one view check: base set, C / ldc / coff
// multiples of the 16-byte piece (4 fp32 channels, 8 halves of a plane).
int launch_upsample2x(const View& in, const View& out, int B, hipStream_t s);                              // bilinear; split: re-split without a range check
int launch_add(const View& a, const View& b, const View& out, int B, hipStream_t s, int32_t* ovf = nullptr);   // ovf: split / plain-f16 views' overflow word (the sum saturates and reports)
int launch_maxpool(const View& in, const View& out, int B, int size, int stride, int pad, hipStream_t s);   // pad > 0: symmetric -inf padding; the winner's stored bits move unchanged
int launch_upsample_nearest2x(const View& in, const View& out, int B, hipStream_t s);
// batch-statistics BatchNorm (+ activation + shortcut) over a conv's raw output, in place (aux_kernels.hip); stats: 2*C doubles of scratch.
// Both launchers run the one statistics path (two stages where 256 % (C/4) == 0 or (C/4) % 256 == 0, else one), which also writes the
// per-channel constants w = gamma / sqrt(var + eps), b = beta - mean w as [2][sstride] floats into `partial`, and then one normalise
// kernel that reads those constants.  partial: the plan's scratch of bn_partial_doubles(max channels) doubles (partial sums + constants);
// REQUIRED — null, or fewer than sstride doubles, is an argument error.
int launch_bn_batch(const View& x, const View& y, const View* res, int B, double* stats, int sstride, const float* bn, int gstride, int act,
                    double* partial, int64_t partial_doubles, hipStream_t s);
size_t bn_partial_doubles(int max_channels);
// the same on a split-f16 plan (plan option bn_batch_split): `raw` is the fp32 view of the conv's raw sums (dense scratch rows, C / ldc /
// coff multiples of 8); bn_apply_kernel's split instance normalises, applies the activation, adds the shortcut operand of its split
// view and stores the split format into `y` (ldc / coff honoured: concat slices)
int launch_bn_batch_split(const View& raw, const View& y, const View* res, int B, double* stats, int sstride, const float* bn, int gstride, int act,
                          double* partial, int64_t partial_doubles, int32_t* ovf, hipStream_t s, int pool = 0);
// pool == 1 (plan options bn_split_narrow + fuse_bn_pool): `y` is the view of the 2x2 / stride-2 max-pool that alone reads the conv
// (raw.H / 2 x raw.W / 2, both even, no shortcut); bn_apply_split_pool_kernel normalises and pools with the max-pool's own winner rule,
// bit-identical to pool == 0 + launch_maxpool
// running_mean / running_var update of every BatchNorm layer of a batch-statistics plan in one launch (aux_kernels.hip)
struct BnUpdateEntry { float* running_mean; float* running_var; int64_t stats_off; double unbias; int sstride; int channels; };
constexpr int BN_UPDATE_MAX = 32;                 // entries per launch (by-value kernel argument: 32 x 40 bytes)
struct BnUpdateTable { BnUpdateEntry e[BN_UPDATE_MAX]; };
int launch_bn_update_running(const BnUpdateEntry* entries, int n, const double* stats, double momentum, hipStream_t s);
int launch_copy(const View& in, const View& out, int B, hipStream_t s);                                     // fp32 views only
int launch_view_to_nchw(const View& in, int B, float* out_nchw, hipStream_t s);
// strided decode: raw element (b, ch, y, x) at raw[b*sb + ch*sc + y*sy + x*sx]
int launch_finish_decode(float* out, int B, const DecodeArgs& d, int hw_exp, hipStream_t s);
int launch_decode(const float* raw, int64_t sb, int64_t sc, int64_t sy, int64_t sx, int B,
                  const DecodeArgs& d, float* out, hipStream_t s);
int launch_confidence_mask(const float* pred, int64_t rows, int attrs, float conf, float* out, hipStream_t s);
int launch_bbox_iou(const float* box1, const float* boxes, int k, int row_stride, float* iou, hipStream_t s);

size_t nms_workspace_bytes(int batch, int n);
int launch_write_results(const float* pred, int batch, int n, int num_class, float conf, float nms,
                         float* out, int cap, int32_t* counts, void* ws, size_t ws_bytes, hipStream_t s);
int launch_nms_class_offset(const float* pred, int batch, int n, int num_class, float conf, float iou_thr, float max_wh, int max_det,
                            float* out, int cap, int32_t* counts, void* ws, size_t ws_bytes, hipStream_t s);

// validator: detections of write_results scored against ground truth (match.hip)
void score_limits(int* max_pred, int* max_tgt);
size_t score_workspace_bytes(int batch, int cap, int max_targets);
int launch_score_detections(const float* det, const int32_t* counts, int cap, int batch, const float* tgt, const int32_t* tgt_off,
                            int num_class, const uint32_t* class_mask, float min_box_size, double iou_threshold, int max_targets, int target_corners,
                            int32_t* scores, int32_t* totals, int32_t* match, float* match_iou, int32_t* status,
                            void* ws, size_t ws_bytes, hipStream_t s);

// training loss, forward value: targets from boxes + the five-term sum of squares (loss.hip)
size_t yolo_loss_workspace_bytes(int batch, int n_rows);
int launch_yolo_loss(const float* pred, int batch, int n_rows, int num_class, const rtod_yolo_head* heads, int n_heads,
                     const float* boxes, const int32_t* box_off, float min_box_size, double* loss, double* per_image,
                     float* target, uint8_t* mask, int32_t* n_obj, int32_t* status, void* ws, size_t ws_bytes, hipStream_t s);
int launch_darknet_loss_dense(const float* pred, const float* target, const uint8_t* mask, int64_t rows, int attrs, double* loss,
                              void* ws, size_t ws_bytes, hipStream_t s);
// ... its gradient with respect to the raw head maps (loss_grad.hip; same workspace)
int launch_yolo_loss_grad(const float* pred, int batch, int n_rows, int num_class, const rtod_yolo_head* heads, int n_heads,
                          const float* boxes, const int32_t* box_off, float min_box_size, float* grad_raw, float* grad_pred, double* loss,
                          int32_t* n_obj, int32_t* status, void* ws, size_t ws_bytes, hipStream_t s);
// weight / bias gradient of a 1x1 or 3x3 convolution on the exact-fp32 MFMA, K slices added in order, an optional double scale
// per row of dW (wgrad.hip).  One path under every entry, which names its slice rule: rtod_conv1x1_wgrad is WGRAD_HEAD with size = 1,
// h = 1, w = pixels, no row scale; rtod_conv_wgrad and rtod_conv_wgrad_s2 (stride 2, size 3 alone: h x w is the conv's INPUT map,
// which x lives on; the same kernel with the tap positions doubled) are WGRAD_TILED; rtod_conv_wgrad_thin (any cin >= 1, stride 1, no
// db) is WGRAD_THIN.  `who` names the entry in the error texts.
enum WgradRule { WGRAD_HEAD, WGRAD_TILED, WGRAD_THIN };            // cap 16 | cap min(16, ceil(1024 / tiles)) | slice count cut for K
constexpr int WGRAD_MAX_SLICES = 16;
constexpr int WGRAD_THIN_MAX_CHAIN = 1024;                         // the longest chain measured inside the 4 x gate
constexpr int WGRAD_THIN_MIN_CHAIN = 256;                          // a small K is not cut into slivers
constexpr int WGRAD_THIN_GROUP = 32;                               // slices per first-level group of the reduction tree
struct WgradSchedule {
    int tm, tn;                 // tile of dW per workgroup: 64 x 64, thin 32 x 128
    int h, w;                   // the map k runs over (stride 2: the conv's output map)
    int64_t K;                  // batch * h * w
    int slices, slice_len;      // S = ceil(K / L) workgroups per tile, fmaf chains of at most L terms
    int group;                  // slice sums per first-level group of the reduction tree (head, tiled: S, one group: the ascending sum)
    int reduce_block;           // threads per workgroup of the reduce kernel
    bool db;                    // the entry has a db and the workspace its slice sums
};
WgradSchedule wgrad_schedule(WgradRule rule, int batch, int cout, int cin, int h, int w, int size, int stride);
size_t wgrad_workspace_bytes(const WgradSchedule& sc, int cout, int cin, int size);
int wgrad_check_shape(const char* who, WgradRule rule, int batch, int cout, int cin, int h, int w, int size, int stride);
int launch_wgrad(const char* who, WgradRule rule, const float* dz, const float* x, int batch, int cout, int cin, int h, int w, int size, int stride,
                 const double* row_scale, float* dw, float* db, void* ws, size_t ws_bytes, hipStream_t s);
// data gradient of a 1x1 or 3x3 / same-padding convolution with the leaky-ReLU derivative of the stored activation in its epilogue
// and an optional double scale per filter folded into the weights (dgrad.hip): one tile body under three geometries.  One path under
// the three entries: rtod_conv1x1_dgrad is size = 1, h = 1, w = pixels, no row scale; rtod_conv_dgrad_s2 is stride = 2 (size 3
// alone), h x w the conv's INPUT map, the same chains over parity-class tiles.  `who` names the entry in the error texts.
int launch_conv_dgrad(const char* who, const float* w, const double* row_scale, const float* dz, const float* y, float slope, int batch, int cout,
                      int cin, int h, int w_, int size, int stride, float* dx, hipStream_t s, bool any_cin = false);   // any_cin (rtod_conv_dgrad_thin): cin % 32 is not refused, stride 2 is
// the same gradient (size 1 or 3, stride 1, cin % 32 == 0) on the forward's split-f16 tiles (dgrad_split.hip): per-image scaled split
// dz, weights packed transposed and flipped at every call, a raw-sum launch of an existing tile, a finishing transpose with the mask
int conv_dgrad_split_tiles(int batch, int cout, int cin, int h, int w, int size, int* ids, int capacity);
int conv_dgrad_split_workspace(int batch, int cout, int cin, int h, int w, int size, size_t* bytes);
int launch_conv_dgrad_split(const float* w, const double* row_scale, const float* dz, const float* y, float slope, int batch, int cout, int cin,
                            int h, int w_, int size, int tile, float* dx, void* workspace, size_t workspace_bytes, hipStream_t s, int phases = 31);
// ... `phases` (rtod_conv_dgrad_split_phases: measurement): which kernel groups of the call are enqueued, on a workspace a full call has filled
enum { DGS_AMAX = 1, DGS_SPLIT = 2, DGS_PACK = 4, DGS_CONV = 8, DGS_FINISH = 16, DGS_ALL = 31 };
// weight gradient of a stride-1 1x1 / 3x3 BatchNorm conv (cin % 32 == 0, no db) as three f16 MFMA products (wgrad_split.hip): one exponent per
// tensor, dz and x split into f16 hi / lo planes on a common padded k grid, a tile of dW x all taps per workgroup, K slices added in order
int conv_wgrad_split_schedule(int batch, int cout, int cin, int h, int w, int size, int* tiles, int* slices, int* slice_len, int64_t* k_padded);
int conv_wgrad_split_bounds(int batch, int cout, int cin, int h, int w, int size, int64_t* lowest, int64_t* highest, int64_t* plane_halves);
int conv_wgrad_split_workspace(int batch, int cout, int cin, int h, int w, int size, size_t* bytes);
int launch_conv_wgrad_split(const float* dz, const float* x, int batch, int cout, int cin, int h, int w, int size, const double* row_scale,
                            float* dw, void* workspace, size_t workspace_bytes, hipStream_t s, int phases = 15);
// ... `phases` (rtod_conv_wgrad_split_phases: measurement): which kernel groups of the call are enqueued, on a workspace a full call has filled
enum { WGS_EXPONENTS = 1, WGS_SPLIT = 2, WGS_GEMM = 4, WGS_REDUCE = 8, WGS_ALL = 15 };
// out = m(y) * (((c0 + c1) + c2) + c3): the fan-out sum of the gradient walk, 1 to 4 contributions, in one launch (grad_join.hip)
int launch_grad_join(const float* const* contributions, int count, const float* y, float slope, int64_t n, float* out, hipStream_t s);
// backward of the 2x upsample (bilinear align_corners=False, or nearest) in gather form, the producing conv's mask fused (upsample_grad.hip)
int launch_upsample2x_grad(const float* dz, const float* y, float slope, int mode, int batch, int channels, int h, int w, float* dx, hipStream_t s);
// backward of the size-2 max-pool (stride 2 floor mode, or stride 1 clamped) in gather form, the producing conv's mask fused (maxpool_grad.hip)
int launch_maxpool_grad(const float* dz, const float* x, float slope, int batch, int channels, int h, int w, int size, int stride, float* dx, hipStream_t s);
// backward of batch-statistics BatchNorm over dense NCHW maps: dz, dgamma, dbeta from du, the raw conv output z and the forward's
// double statistics, two launches over one partition that the shape alone fixes (bn_grad.hip)
int bn_grad_parts(int batch, int channels, int pixels, int* parts, int* part_len);
int bn_grad_workspace(int batch, int channels, int pixels, size_t* bytes);
int launch_bn_grad(const float* du, const float* z, const double* mean, const double* var, const float* gamma, int batch, int channels, int pixels,
                   float* dz, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, hipStream_t s);
// optimiser step of one conv fused with the re-pack of its block of the weight image (head_step.hip): a 1x1 conv without BatchNorm
// with its bias (Plan::step_conv), or a conv whose frozen BatchNorm scale is folded while it re-packs (b == NULL, scale given:
// Plan::step_conv_folded).  The kernel's own argument: the scalars are what the host derived in double (Plan::opt_scalars), the
// image pointers are the conv's ranges of the device image (Plan::step_packed)
struct HeadStepLaunch {
    int kind = 0;                                   // 0 SGD, 1 Adam
    float lr = 0.f;                                 // SGD: (float)lr.  Adam: (float)(lr / (1 - beta1^t))
    float beta2 = 0.f, omb1 = 0.f, omb2 = 0.f;      // (float)beta2, (float)(1 - beta1), (float)(1 - beta2)
    float bc2_sqrt = 1.f, eps = 0.f;                // (float)sqrt(1 - beta2^t), (float)eps
    int cout = 0, cin = 0, taps = 1, cin_p = 0;     // taps = size * size; cin_p: channels per tap of the fp32 panel's K order
    int split = 0;                                  // 0: fp32 panel, 1: f16 hi / lo planes
    int Kpad = 0, Npad = 0;
    float *w = nullptr, *b = nullptr;               // masters (b == NULL: a BatchNorm conv, whose bias slot is not written)
    const float *dw = nullptr, *db = nullptr;
    float *m_w = nullptr, *v_w = nullptr, *m_b = nullptr, *v_b = nullptr;
    const double* scale = nullptr;                  // BatchNorm convs: the frozen gamma / sqrt(var + 1e-5) per output channel (NULL: 1)
    float* panel = nullptr;                         // fp32 plans: [Npad][Kpad]
    uint16_t *hi = nullptr, *lo = nullptr;          // split plans: [Kpad / 32][Npad][32] halves each
    float* inv = nullptr;                           // split plans: [Npad]
    float* bias = nullptr;                          // [Npad]
    // a conv whose BatchNorm runs on batch statistics (Plan::step_conv_bn; b == NULL, scale == NULL: the conv is packed unfolded): the
    // extra workgroup steps beta and gamma instead of a bias and writes them to the image's [Npad] beta, [Npad] gamma block
    float *gamma = nullptr, *beta = nullptr;
    const float *dgamma = nullptr, *dbeta = nullptr;
    float *m_g = nullptr, *v_g = nullptr, *m_be = nullptr, *v_be = nullptr;
    float* bn = nullptr;
};
int launch_head_step(const HeadStepLaunch& h, hipStream_t s);

}  // namespace rtod
