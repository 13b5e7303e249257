/*
 * rtod.h — C ABI of librtod.so: the MI355X (gfx950) YOLOv3 inference hot path.
 *
 * The reference (uguryagmur/RealTimeObjectDetection) is pure Python and has no FFI layer; its
 * boundary for this path is the Python API of src/darknet.py and src/util.py.  The host layer
 * in realtimeobjectdetection_amd/{darknet,util}.py keeps that API and binds the entry points
 * below through ctypes (INTEGRATION.md shows the stub).  Each entry point names the reference
 * interface it replaces (file:line into /root/reference).
 *
 * Conventions
 *  - every function returns 0 on success or a negative rtod_status; it never throws and never
 *    synchronises the device unless its comment says so;  rtod_last_error() returns the message
 *    of the calling thread's last failure;
 *  - the library reads no environment variable: every behaviour switch is explicit per-plan state
 *    (rtod_plan_set_precision, rtod_plan_set_option);
 *  - "dev" pointers are device (HBM) addresses owned by the caller (torch.Tensor.data_ptr());
 *    kernels are enqueued on the caller-supplied hipStream_t (void*; 0 = default stream);
 *  - a plan is not thread-safe; distinct plans are independent;
 *  - all tensors are float32.  Activations inside a plan are NHWC; the API edges keep the
 *    reference's layouts (input NCHW [B,3,H,W], predictions [B,N,5+C], detections [D,8]).
 */
#ifndef RTOD_H
#define RTOD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum rtod_status {
    RTOD_OK = 0,
    RTOD_E_ARG = -1,     /* bad argument / shape */
    RTOD_E_HIP = -2,     /* HIP runtime error (message has hipGetErrorString) */
    RTOD_E_CFG = -3,     /* cfg grammar / unknown block (reference: src/darknet.py:524-526 asserts) */
    RTOD_E_STATE = -4,   /* call order (e.g. forward before load_weights) */
    RTOD_E_SIZE = -5     /* weight stream too short (reference: view_as raises, src/darknet.py:348) */
} rtod_status;

typedef struct rtod_plan rtod_plan;

typedef struct rtod_plan_info {
    int32_t n_layers;          /* cfg blocks after [net] (107 for yolov3, 24 for tiny) */
    int32_t n_launches;        /* kernels enqueued by one rtod_forward */
    int32_t height, width, max_batch;
    int32_t total_rows;        /* N of the [B,N,5+C] output (22743 @608) */
    int32_t attrs;             /* 5 + classes */
    int64_t n_weight_floats;   /* floats a .weights payload must hold */
    int64_t conv_flops_per_frame;   /* 2*MACs of the direct convolutions (SURVEY.md §8 d) */
    int64_t arena_bytes;       /* activation arena the plan allocates for max_batch */
    int64_t packed_weight_bytes;
} rtod_plan_info;

typedef struct rtod_launch_info {
    int32_t layer;             /* cfg layer index this launch implements (fused layers: the conv) */
    int32_t kind;              /* 0 conv-igemm, 1 input-pack, 2 upsample, 3 add, 4 maxpool, 5 decode, 6 copy, 7 stem conv */
    int32_t variant;           /* conv tile variant id (see rtod_conv_variant_name) */
    int32_t ksize, stride, cin, cout, hout, wout;
    int32_t fused_residual, fused_decode;
    int32_t fused_pointwise;   /* 1: the next layer's 1x1 conv runs in this conv's epilogue (its own launch entry is then empty) */
    int64_t flops_per_frame;   /* algorithmic 2*MACs (0 for non-conv launches) */
    int64_t bytes_per_frame;   /* algorithmic bytes: input once + output once (+ residual) */
    int64_t weight_bytes;      /* read once per launch */
} rtod_launch_info;

int rtod_version(void);
/* Copies the calling thread's last error message (NUL-terminated, truncated to len). */
int rtod_last_error(char* buf, size_t len);
/* Number of HIP devices visible; does not initialise a device context. */
int rtod_device_count(int* out);

/* ---- plan = Darknet(cfg) ------------------------------------------------------------------
 * replaces Darknet.__init__ -> parse_cfg + create_modules   src/darknet.py:176-189, 412-603
 * Parses the cfg text (same grammar), resolves shapes for [*,3,height,width], plans NHWC buffers
 * (zero-copy route concat, fused shortcut / head decode) and the launch list.  Host-only: no
 * device memory is touched until rtod_plan_load_weights. */
int rtod_plan_create(const char* cfg_text, size_t len, int height, int width, int max_batch,
                     int device, rtod_plan** out);
/* (new; opt-in) Same for a rectangular input [*,3,height,width] (height != width allowed; the reference only defines the square
 * network, whose strides all derive from net_info['height']).  Every [yolo] head's grid GH x GW must have one integer stride
 * on both axes, height / GH == width / GW (and height // (height // GH) == GH, likewise for width), else RTOD_E_CFG naming the
 * layer.  Head rows keep the reference's order with G*G split into GH*GW: row r = (gy * GW + gx) * A + a, GH*GW*A rows per head.
 * With height == width the plan (describe JSON, launches, tiles, output) is identical to rtod_plan_create's.  Option
 * "bn_batch_stats" is refused (RTOD_E_ARG) on a plan with height != width. */
int rtod_plan_create_rect(const char* cfg_text, size_t len, int height, int width, int max_batch,
                          int device, rtod_plan** out);
int rtod_plan_destroy(rtod_plan* plan);
int rtod_plan_get_info(const rtod_plan* plan, rtod_plan_info* out);
int rtod_plan_get_launch(const rtod_plan* plan, int index, rtod_launch_info* out);
/* JSON description of the resolved layer IR (tests compare it with the Python IR / reference). */
int rtod_plan_describe(const rtod_plan* plan, char* buf, size_t len, size_t* needed);
/* (new) The packed weight image rtod_plan_load_weights would upload for the plan's current options and precision, computed on
 * the host: no device is touched, so it works without one and before or after rtod_plan_load_weights.  Same two-call shape as
 * rtod_plan_describe: *needed_floats (if given) receives the image's size; with out == NULL nothing else happens; otherwise
 * capacity_floats must cover it (RTOD_E_SIZE) and `w` / n_floats are the .weights payload as for rtod_plan_load_weights. */
int rtod_plan_pack_weights(const rtod_plan* plan, const float* w, size_t n_floats, float* out, size_t capacity_floats,
                           size_t* needed_floats);
const char* rtod_conv_variant_name(int variant);
/* Demangled name of the kernel instantiation a launch runs (what rocprofv3 --kernel-trace prints): variant from
 * rtod_launch_info, epilogue 0 plain, 1 fused shortcut, 2 fused head decode, 3 / 4 = 0 / 1 with a fused pointwise conv;
 * + 8: the plain-f16 instance (precision 2) of epilogues 0-2. */
int rtod_conv_kernel_name(int variant, int epilogue, char* buf, size_t len);
/* Same for launch `index` of a plan (all context taken from the plan; "" for launches that are not convolution kernels). */
int rtod_plan_launch_kernel_name(const rtod_plan* plan, int index, char* buf, size_t len);
/* Arithmetic of the convolutions (call before rtod_plan_load_weights):
 *   0  exact fp32 MFMA (v_mfma_f32_32x32x2_f32): bit-level fmaf chains, the parity anchor;
 *   1  split-precision f16 MFMA: a*w ~= ah*wh + ah*wl + al*wh with fp32 accumulation (22-bit
 *      operands, error ~2x fp32 per layer), 16x the MFMA rate per product.  Activations live in
 *      HBM as f16 hi/lo planes (x8 pre-scaled): needs |activation| < 8188, every conv after the
 *      stem with Cin % 32 == 0 (or, with option "narrow_cin", Cin == 16: conv_c16_f16s3.hip), no stand-alone
 *      shortcut / copy / decode launch; otherwise RTOD_E_CFG.
 *   2  plain f16 (opt-in speed mode, not the parity path): every activation stored once as RNE_f16(8x) in the hi plane
 *      of mode 1's layout (the lo plane is never written or read), weights = mode 1's pre-scaled hi plane, ONE
 *      v_mfma_f32_16x16x32_f16 per fragment pair with fp32 accumulation; epilogue (scale, bias, activation, fused
 *      shortcut, saturating store + range flag) as mode 1.  Error ~1e-3 relative end to end (profiles/f16_floor.json),
 *      same range |activation| < 8188, same cfg requirements (RTOD_E_CFG otherwise; also with bn_batch_stats).  Kernels:
 *      the split stem, then the generic tiles, the bandd band / wide tiles, the 1x1 slab tiles and the narrow (Cin == 16)
 *      tiles in their f16 instances (no conv_band / ring / patch tile, no fused stem + layer 1, no hosted pointwise conv).
 * Other modes: RTOD_E_ARG.
 * cfg grammar: the reference's (src/darknet.py:412-603) plus three extension keys for YOLOv5-style blocks (detect.py:255-285
 * fetches that model from the network; only its building blocks exist here): [convolutional] activation=silu,
 * [maxpool] symmetric=1 (-inf padding of (size-1)/2 per side), [upsample] mode=nearest, [yolo] decode=v5, [route] with up to
 * four sources. */
int rtod_plan_set_precision(rtod_plan* plan, int mode);
/* Plan options (call before rtod_plan_load_weights; re-plans buffers and launches).  All default to 1 / -1:
 *   "fuse_pointwise"    1x1 conv in the previous conv's epilogue where one workgroup holds all its input channels
 *   "fuse_shortcut"     shortcut (src/darknet.py:263-268) in the producing conv's epilogue; 0: stand-alone add kernel
 *   "fuse_decode"       predict_transform (src/util.py:175-239) in the head conv's epilogue; 0: stand-alone decode kernel
 *   "zero_copy_concat"  route producers (src/darknet.py:270-290) write into the concat buffer; 0: copy kernels
 *   "stem_kernel"       dedicated NCHW-reading kernel for layer 0; 0: input pack + generic conv
 *   "band_kernel"       LDS-band kernel for 3x3 stride-1 layers; 0: generic implicit GEMM
 *   "ring_kernel"       persistent LDS-DMA ring tiles among the autotune candidates (bit-identical to the generic tiles)
 *   "patch_kernel"      2-D patch tiles among the autotune candidates of the wide 3x3 stride-1 layers (bit-identical)
 *   "stem2_kernel"      layers 0-2 of Darknet-53 in one kernel (conv_stem2_f16s3.hip, bit-identical); 0: stand-alone kernels
 *   "bn_batch_stats"    (default 0) exact-fp32 plans: BatchNorm on batch statistics instead of the folded running statistics
 *   "bn_batch_split"    (default 0) with "bn_batch_stats": lets precision 1 (split f16) run that mode; without it the option is inert
 *                       (same plan, same bits, in every precision).  Every BatchNorm conv after layer 0 runs a RAW-SUM instance of a
 *                       generic, bandd or 1x1 slab tile (epilogue code 16 in rtod_conv_kernel_name: the fp32 convolution sums go to a
 *                       dense scratch, "bn_raw_bytes" in rtod_plan_describe, allocated with the weights), then the statistics kernels
 *                       of "bn_batch_stats", then a normalise kernel that applies the activation, adds the shortcut and writes the
 *                       split format.  Layer 0 stays on the exact-fp32 kernel.  Convs without BatchNorm run as in an eval plan; no
 *                       hosted pointwise conv, no fused stem.  Tiles: those with a raw-sum instance that the layer's family rules
 *                       admit (rtod_plan_set_tiles refuses the others).  RTOD_E_CFG from rtod_plan_set_precision (or from the option
 *                       call that completes the combination): precision 2; a BatchNorm conv with Cin == 16 (with or without
 *                       "narrow_cin"); "k_slices_split" or "stem_pool" together with the mode (see "bn_split_narrow").  Accepted before or after
 *                       rtod_plan_set_precision.  rtod_plan_bn_batch_stats / rtod_plan_bn_update_running work as in fp32 plans
 *   "bn_split_narrow"   (default 0) read only when "bn_batch_stats", "bn_batch_split" and precision 1 are all in force (otherwise inert: same
 *                       plan, same bits): that mode also for YOLOv3-tiny's kind of graph.  A BatchNorm conv with Cin == 16 is accepted
 *                       (needs "narrow_cin") and runs a raw-sum instance of a narrow tile (ids 140 ..., epilogue code 16;
 *                       rtod_plan_set_tiles accepts the narrow ids on it and refuses the others).  "stem_pool" is accepted together
 *                       with the mode: a matching layer 0 with BatchNorm runs the raw-sum instance of the 16-filter split stem (NCHW
 *                       input read directly, no pack launch, no exact-fp32 conv); a layer 0 that does not match stays on the
 *                       exact-fp32 kernel.  Rows of the raw-sum scratch are Cout rounded up to 8 floats for those two kernels, Npad
 *                       floats for the others; "bn_raw_bytes" is the maximum over the BatchNorm convs of max_batch * hout * wout *
 *                       row * 4.  Still RTOD_E_CFG, the plan left as it was, in either call order: precision 2, "k_slices_split", a
 *                       BatchNorm conv with a fused head decode
 *   "fuse_bn_pool"      (default 1, read only when "bn_split_narrow" is in force) where a BatchNorm conv (raw-sum launch of any family,
 *                       layer 0 on the exact-fp32 kernel too) without a fused shortcut is followed by a [maxpool] size 2 / stride 2
 *                       (not symmetric) that alone reads it, its hout and wout are even and keep_all_layers is off, the normalise
 *                       kernel also does the pool: the conv's full-resolution map is never stored (describe: "fused_into": <pool
 *                       index>; rtod_plan_read_layer on the conv: RTOD_E_STATE), the pool's launch entry stays in the list and
 *                       enqueues nothing.  Bit-identical to the stand-alone normalise + max-pool kernels, batch statistics and
 *                       range flag included; 0: always stand-alone
 *   "k_slices"          exact-fp32 plans: deep small-grid layers summed in K slices (conv_igemm_f32.hip); 0: one chain
 *   "k_slice_workgroups" ... one workgroup per slice when the grid is small; 0: always inside the workgroup (same bits).
 *                       Governs the K-sliced split-f16 tiles of "k_slices_split" in the same way
 *   "k_slices_split"    (default 0) precisions 1 / 2, for single-frame latency: a conv is SLICED when its shape alone says so — after
 *                       layer 0, Cin % 32 == 0 (not a "narrow_cin" layer), no fused head decode, neither host nor guest of a
 *                       fused-pointwise candidate pair nor layer 1 of the fused stem pattern, hout * wout <= 2704 and at least 8
 *                       K-chunks of 32.  Its K sum is formed in slices of 9 / 4 / 2 chunks (32+ / 16+ / 8+ chunks; the last slice
 *                       may be shorter) in the generic K order, slice sums added in ascending order in fp32.  A sliced layer always
 *                       runs the tile family of conv_ks_f16s3.hip (variant ids 150 + 2 * tile + schedule; schedule 0 walks the
 *                       slices inside the workgroup, schedule 1 gives every (tile, slice) its own workgroup and reduces the panels:
 *                       same bits), at every batch size, and is no band layer; rtod_plan_describe reports "k_slices": S on it.
 *                       The summation order differs from the default plan's, so results differ from it in the last bits.
 *                       At large batches the sliced 3x3 layers lose the band kernels: keep a second plan for throughput.
 *                       Exact-fp32 plans accept the option and ignore it; plans without it are unchanged.  Either order with precision
 *   "narrow_cin"        (default 0) precisions 1 / 2 accept convs after layer 0 that read exactly 16 channels (YOLOv3-tiny's
 *                       layer 2, any cfg with a 16-filter stem): they run on their own tile family (conv_c16_f16s3.hip, variant
 *                       ids 140 ..., K order tap-major over the 16 channels).  Other Cin % 32 != 0 (48, 80, ...) stay refused.
 *                       Plans without such a layer, and exact-fp32 plans, are unchanged by it
 *   "stem_pool"         (default 0) precisions 1 / 2: a layer 0 that is 3x3 / stride 1 / pad 1 with Cin 3 and 16 filters (YOLOv3-tiny's;
 *                       BatchNorm folded or absent, any activation) runs on the split-f16 stem of conv_stem16_f16s3.hip, which
 *                       reads the NCHW input directly (no pack launch, no exact-fp32 conv).  Exact-fp32 plans and plans whose
 *                       layer 0 does not match are unchanged by it.  Precision and option may be set in either order
 *   "fuse_stem_pool"    (default 1) with "stem_pool": where layer 1 is a [maxpool] size 2 / stride 2 (not symmetric) that alone
 *                       reads layer 0, layer 0's H and W are even and keep_all_layers is off, the pool runs in the stem's kernel:
 *                       layer 0 is never stored (describe: "fused_into": 1), the pool's launch entry stays in the list and
 *                       enqueues nothing.  Bit-identical to the stand-alone stem + max-pool kernel; 0: always stand-alone
 *   "keep_head_inputs"  (default 0) the buffer read by every conv in front of a [yolo] layer (the detection-head convs, decode fused or not)
 *                       keeps its lifetime to the end of the forward, so rtod_plan_read_layer of that input layer is valid after a
 *                       forward in every precision: the activations rtod_conv1x1_wgrad needs.  Liveness only: launches, tiles and
 *                       output bits are those of the plan without the option; arena_bytes may grow
 *   "keep_block_inputs" (default 0) likewise the buffer read by every detection BLOCK conv (rtod_plan_head_blocks), a concat buffer
 *                       where that input is a route: the activations rtod_conv_wgrad needs.  Liveness only as well; in addition
 *                       rtod_plan_load_weights then keeps the blocks' frozen BatchNorm scales on the device (rtod_plan_conv_scale)
 *   "keep_neck_activations" (default 0) likewise every buffer that a NECK conv (rtod_plan_neck_layers) or a detection-head conv reads or
 *                       writes, routes as their concat buffers: the activations of the walk behind the backbone (rtod_conv_dgrad,
 *                       rtod_upsample2x_grad, rtod_conv_wgrad).  Requires no other option.  Liveness only as well; rtod_plan_load_weights
 *                       then keeps the frozen BatchNorm scales of ALL neck convs on the device, and rtod_plan_conv_scale,
 *                       rtod_plan_update_conv_weight and rtod_plan_step_conv_folded accept any neck conv (without it: blocks alone)
 *   "keep_backbone_activations" (default 0) a superset of "keep_neck_activations" over the TRAINABLE convs (rtod_plan_trainable_layers):
 *                       every buffer one of them or a detection-head conv reads or writes stays live to the end of the forward, the
 *                       frozen scales of all of them go to the device, and the three folded-conv entries accept every one of them, the
 *                       stride-2 convs included.  Not liveness only: while it is set the plan forms no fusion that would leave a
 *                       trainable conv's own output unstored or its packed layout out of reach — no shortcut in a conv's epilogue,
 *                       no fused pointwise pair, no fused stem + layer 1 kernel — so the forward is, bit for bit and tile for tile,
 *                       that of a plan with "fuse_shortcut" = 0, "fuse_pointwise" = 0, "stem2_kernel" = 0.  Default plans do not change
 *   "keep_full_activations" (default 0) a superset of "keep_backbone_activations" over the FULL graph (rtod_plan_full_layers): thin
 *                       convs (any Cin, layer 0 on a generic layout) and size-2 max-pools too.  Holds the same fusions
 *   "keep_bn_inputs"    (default 0) training under batch statistics: on a "bn_batch_stats" plan (inert without it) every BatchNorm conv
 *                       the plan trains — a detection block, and every BatchNorm conv of the graph the keep option above names — writes
 *                       its raw sums z into an arena buffer of its own (never reused during the forward; rows of Cout floats on an
 *                       exact-fp32 plan, of the raw-sum scratch's stride — Cout rounded up to 128 — on an f16s3 plan); the
 *                       normalise step reads it and writes the layer's view, so the forward's values are those of the in-place path bit
 *                       for bit.  rtod_plan_head_blocks, _neck_layers, _trainable_layers and _full_layers then list what the eval plan
 *                       with the same keep option lists (without it a batch-statistics plan lists nothing), rtod_plan_read_bn_input
 *                       returns z, and rtod_plan_step_conv_bn / rtod_plan_update_conv_bn train conv weight, gamma and beta; the
 *                       folded-conv entries keep refusing the plan.  A conv with a shortcut added in its normalise step is no member
 *                       (its stored output is not act(u)); SiLU, split-f16 ("bn_batch_split") and rectangular plans are out of scope.
 *                       Exact-fp32 plans only: RTOD_E_CFG on precision 1 or 2, in either order of the two calls
 *   "force_f16s3_variant" / "force_f32_variant"   >= 0: one tile variant for every conv (tests, A/B runs)
 * Options that leave a cfg inexpressible in the split-f16 format return RTOD_E_CFG when precision is 1 or 2 (so does setting
 * "narrow_cin" back to 0 on a plan that needs it); the plan then stays as it was. */
int rtod_plan_set_option(rtod_plan* plan, const char* name, int value);
/* Split-f16 plans store activations as f16 hi/lo planes of 8*x: |activation| must stay below 8188.  Producers
 * saturate at that range (never inf / NaN) and OR 1 into *flag_dev (caller-owned device int32, zero it yourself)
 * whenever a value saturated: read it at any synchronisation point.  NULL disables the report. */
int rtod_plan_set_overflow_flag(rtod_plan* plan, int32_t* flag_dev);

/* replaces Darknet.load_weights                              src/darknet.py:316-410
 * `w` is the float payload of a Darknet .weights file (after the 5xint32 header), host memory:
 * per convolutional block [bn.bias, bn.weight, running_mean, running_var] or [conv.bias], then
 * conv.weight (OIHW).  Folds eval-mode BatchNorm (eps 1e-5) into the conv, packs K-major panels,
 * allocates device memory on first call and uploads.  Synchronises the device. */
int rtod_plan_load_weights(rtod_plan* plan, const float* w, size_t n_floats);
/* (new) The detection heads of a plan in cfg order: conv_layers[i] is the conv directly in front of the i-th [yolo] layer,
 * input_layers[i] the layer whose output it reads (conv_layers[i] - 1; see option "keep_head_inputs").  Returns the number of
 * heads (also when it exceeds capacity: then only capacity entries were written; capacity 0 with NULL arrays asks for the count). */
int rtod_plan_head_layers(const rtod_plan* plan, int* conv_layers, int* input_layers, int capacity);
/* (new) Replaces the weights of ONE conv without BatchNorm on a plan whose weights are loaded: weight_oihw_host [Cout,Cin,k,k] and
 * bias_host [Cout] (host float32).  Only that conv's bias, weight planes and per-channel scales are packed again, by the very
 * function rtod_plan_load_weights packs every conv with, and only those ranges are copied to the device: the plan then holds
 * the bits a full rtod_plan_load_weights of the edited stream gives.  Synchronises the device.  RTOD_E_ARG: a null pointer, a
 * layer that is not a convolution, a conv with BatchNorm, a conv that hosts or is hosted in a fused pointwise pair;
 * RTOD_E_STATE: before rtod_plan_load_weights. */
int rtod_plan_update_conv(rtod_plan* plan, int layer, const float* weight_oihw_host, const float* bias_host);
/* (new) The detection BLOCKS of a plan, one entry per head in cfg order: head_conv_layers[i] as rtod_plan_head_layers,
 * block_conv_layers[i] the layer that head conv reads (head - 1) if it is a block, else -1, block_input_layers[i] the layer the
 * block reads (block - 1, possibly a route; -1 without a block; see option "keep_block_inputs").  A block is a convolution
 *   with BatchNorm, folded (plans with option "bn_batch_stats" have no blocks), of size 1 or 3, stride 1, pad size / 2,
 *   activation leaky or linear, Cin a multiple of 32,
 *   packed in one of the two generic layouts — not a stem, not narrow (Cin == 16), neither host nor guest of a fused pointwise
 *   candidate pair (a conv under "k_slices_split" packs by the generic formula and qualifies) — for every tap and channel
 *       fp32 panel    float  o * Kpad + tap * Cin + c
 *       split planes  half   (((c / 32) * taps + tap) * Npad + o) * 32 + c % 32      of the hi and of the lo plane,
 *   and whose own output is stored (not computed inside another layer's kernel).
 * A head that reads a max-pool, a stride-2 conv, a SiLU conv or a conv without BatchNorm has none.  Returns the number of heads,
 * capacity as rtod_plan_head_layers. */
int rtod_plan_head_blocks(const rtod_plan* plan, int* head_conv_layers, int* block_conv_layers, int* block_input_layers, int capacity);
/* (new) The detection NECK of a plan: the BatchNorm convs, in ascending order, of the largest set G of traversable layers that is
 * closed downstream — a layer is in G only if every reader of its output is in G or is a [yolo] layer — so that nothing outside G
 * lies between a neck conv and the loss and the walk back through G gives exact gradients (BatchNorm frozen).  Traversable:
 *   a conv in front of a [yolo] layer (1x1, no BatchNorm, Cin a multiple of 32, read by [yolo] layers alone);
 *   a conv that is a block by the definition at rtod_plan_head_blocks except for its position (any place in the cfg);
 *   a [route];  a 2x [upsample], bilinear or nearest.
 * conv_layers[i] is a neck conv, input_layers[i] the layer it reads (conv - 1, possibly a route or an upsample; see option
 * "keep_neck_activations").  YOLOv3: 75-80, 84, 87-92, 96, 99-104; YOLOv3-tiny: 12, 13, 14, 18, 21 (layer 8 is read by a max-pool).
 * The listing does not depend on the option.  Returns the number of neck convs, capacity as rtod_plan_head_layers. */
int rtod_plan_neck_layers(const rtod_plan* plan, int* conv_layers, int* input_layers, int capacity);
/* (new) The TRAINABLE convs of a plan: the BatchNorm convs, in ascending order, of the set rtod_plan_neck_layers defines with two more
 * traversable kinds:
 *   a conv that is a block except that it is 3x3 / stride 2 / pad 1 (leaky or linear, Cin a multiple of 32, generic packed layout, its
 *   own output stored);
 *   a two-source [shortcut] with linear activation.
 * Layer 0 (three input channels, stem layouts), max-pools, SiLU convs and plans with "bn_batch_stats" are not traversable.  The plan's
 * fusions decide membership: on a default plan a conv whose shortcut runs in its epilogue, a pointwise pair and the fused stem are not
 * members, and the closure rule then drops what they read; with option "keep_backbone_activations" none of these is formed.  With
 * it: YOLOv3 every BatchNorm conv except layer 0 (71); YOLOv3-tiny the neck (12, 13, 14, 18, 21: its backbone is max-pools).
 * conv_layers / input_layers / capacity and the return value as rtod_plan_neck_layers. */
int rtod_plan_trainable_layers(const rtod_plan* plan, int* conv_layers, int* input_layers, int capacity);
/* (new) The frozen BatchNorm scale of a block conv, s[o] = (double)gamma[o] / sqrt((double)var[o] + 1e-5), exactly the factor
 * rtod_plan_load_weights folded into the conv, taken from the stream last loaded.  scale_host (may be NULL): `channels` doubles
 * are copied out.  scale_dev (may be NULL): receives a device pointer to the same doubles, owned by the plan and valid until
 * it is destroyed; the plan keeps them on the device with option "keep_block_inputs" only (else RTOD_E_STATE).  RTOD_E_ARG: a
 * layer that is not a block (the message says why), channels != Cout; RTOD_E_STATE: before rtod_plan_load_weights. */
int rtod_plan_conv_scale(const rtod_plan* plan, int layer, const double** scale_dev, double* scale_host, int channels);
/* (new) rtod_plan_update_conv for a block conv, BatchNorm frozen: weight_oihw_host [Cout,Cin,k,k] replaces the conv's weights;
 * its block of the image is packed again by the function rtod_plan_load_weights packs with, from the BatchNorm parameters of
 * the stream last loaded and these weights, so the plan holds the bits a full load of the edited stream gives (the bias slot
 * beta - mean * s included, unchanged).  Synchronises the device.  RTOD_E_ARG: a null pointer, a layer that is not a block;
 * RTOD_E_STATE: before rtod_plan_load_weights. */
int rtod_plan_update_conv_weight(rtod_plan* plan, int layer, const float* weight_oihw_host);

/* replaces Darknet.forward                                   src/darknet.py:199-303
 * x_dev: [batch,3,H,W] NCHW float32; out_dev: [batch,N,5+C] (new contiguous tensor in the
 * reference; here caller-allocated).  batch <= max_batch.  Enqueues only: no measurement, no host
 * synchronisation, no allocation -> legal under hipStreamBeginCapture (a captured forward replays as a hipGraph). */
int rtod_forward(rtod_plan* plan, const float* x_dev, int batch, float* out_dev, void* stream);
/* One forward that also measures, per distinct split-f16 conv shape, every tile variant on the layer's real input
 * (HIP events on `stream`) and remembers the fastest for this batch size; later rtod_forward calls of that batch
 * size use the table (untuned batch sizes use closed-form heuristics).  out_dev receives a valid forward result.
 * Synchronises `stream` repeatedly; not capturable.  No-op (plain forward) for exact-fp32 plans.  Tile choice never
 * changes results: every candidate of a layer sums its K products in the same order. */
int rtod_plan_autotune(rtod_plan* plan, const float* x_dev, int batch, float* out_dev, void* stream);
/* The tile table of a batch size: one variant id per launch (-1: heuristic / not a split-f16 conv).  get: copies the table an
 * autotune run left (returns the number of launches, or RTOD_E_STATE if that batch size was never tuned; `variants` may be NULL
 * to ask for the count).  set: installs a table (e.g. one saved by an earlier process) so that later forwards of that batch size
 * launch exactly those kernels without measuring anything — profiled passes (rocprofv3 --pmc) then replay the launches of the
 * timing pass.  Every entry is checked against its layer (band tiles on band layers, valid split-K mode, ...): RTOD_E_ARG. */
int rtod_plan_get_tiles(const rtod_plan* plan, int batch, int* variants, int capacity);
int rtod_plan_set_tiles(rtod_plan* plan, int batch, const int* variants, int count);
/* Same, with a hipEvent pair around every launch (recorded on `stream`); synchronises and
 * writes the per-launch durations in ms to launch_ms[n_launches] (host).  For bench/roofline. */
int rtod_forward_timed(rtod_plan* plan, const float* x_dev, int batch, float* out_dev,
                       void* stream, float* launch_ms);
/* replaces `with model.train_mode():`                       src/darknet.py:305-314
 * train != 0: heads apply only the sigmoids (TRAIN=True in predict_transform, util.py:211). */
int rtod_plan_set_train_decode(rtod_plan* plan, int train);
/* (new) Turns the output of a forward run with train != 0 into the eval decode IN PLACE: columns 0-3 of every head become
 * (sigmoid + cell offset) * stride and exp(raw) * anchor / stride * stride, in the operation order and with the exponential of
 * the kernel that decodes that head in this plan (libm expf in exact-fp32 plans, the hardware exponential of the split-f16 / f16
 * head epilogue) — which is why the call is bound to a plan.  pred_dev [batch, N, 5+C] is then bit-identical to the output of a
 * forward of the same input with train == 0: one forward serves both the loss and the detections.  Enqueues only.
 * RTOD_E_CFG: a head with `decode=v5`. */
int rtod_plan_finish_decode(rtod_plan* plan, float* pred_dev, int batch, void* stream);
/* Debug/test: keep != 0 disables liveness-based arena reuse so that every layer's output is still
 * intact after a forward (for rtod_plan_read_layer).  Call before rtod_plan_load_weights. */
int rtod_plan_set_keep_all_layers(rtod_plan* plan, int keep);
/* Debug/test: copies layer `layer`'s output (NHWC view -> dense NCHW float32) to out_dev
 * [batch,C,H,W] after a forward; enqueues on stream. */
int rtod_plan_layer_shape(const rtod_plan* plan, int layer, int* c, int* h, int* w);
int rtod_plan_read_layer(rtod_plan* plan, int layer, int batch, float* out_dev_nchw, void* stream);
/* Plans with option "bn_batch_stats" = 1 (exact fp32 only) run BatchNorm the way the reference's callers do: never calling
 * .eval(), nn.BatchNorm2d normalises with the statistics of the batch (src/darknet.py:493-495, detect.py:185-194; SURVEY.md
 * F2).  Per-channel mean and BIASED variance of a conv layer's last forward (host doubles; synchronises `stream`): what the
 * host class needs to update running_mean / running_var like torch does (momentum 0.1, unbiased variance). */
int rtod_plan_bn_batch_stats(rtod_plan* plan, int layer, double* mean_host, double* var_host, int channels, void* stream);
/* The side effect itself, for ALL BatchNorm layers of such a plan in ONE launch (no host round trip): after a forward of `batch`
 * frames, running_mean[k] = (1 - momentum) * running_mean[k] + momentum * batch mean, running_var[k] likewise with the unbiased
 * batch variance, in float32 like torch (nn.BatchNorm2d in training mode, src/darknet.py:493-495).  running_mean_dev /
 * running_var_dev: HOST arrays of n_bn device pointers (float32 [cout]), the plan's BatchNorm layers in cfg order.  Enqueues only. */
int rtod_plan_bn_update_running(rtod_plan* plan, int batch, float* const* running_mean_dev, float* const* running_var_dev, int n_bn,
                                double momentum, void* stream);

/* replaces predict_transform                                 src/util.py:175-239
 * raw_dev [batch, A*attrs, G, G] NCHW -> out_dev [batch, G*G*A, attrs]; anchors = A (w,h) pairs
 * in input pixels (host); train != 0 applies only the three sigmoids. */
int rtod_predict_transform(const float* raw_dev, int batch, int attrs, int grid, int n_anchors,
                           const float* anchors_wh, int inp_dim, int train, float* out_dev,
                           void* stream);

/* replaces confidence_mask                                   src/util.py:106-117 */
int rtod_confidence_mask(const float* pred_dev, int64_t rows, int attrs, float confidence,
                         float* out_dev, void* stream);
/* replaces bbox_iou (one box vs k boxes, row stride in floats) src/util.py:120-153 */
int rtod_bbox_iou(const float* box1_dev, const float* boxes_dev, int k, int row_stride,
                  float* iou_dev, void* stream);

/* replaces prep_image + letterbox_image                      src/util.py:349-397
 * img_dev: uint8 [height,width,3] (HWC; bgr != 0: OpenCV channel order, swapped to RGB like prep_image's
 * default mode) -> out_dev float32 [3,inp_dim,inp_dim]: aspect-preserving bicubic resize, grey 128 padding,
 * /255.  cv2 is unavailable offline, so parity with cv2.INTER_CUBIC is unpinned (see preprocess.hip). */
int rtod_prep_image(const uint8_t* img_dev, int height, int width, int bgr, int inp_dim, float* out_dev, void* stream);
/* (new) Batched, rectangular-target prep_image: frames_dev uint8 [batch,height,width,3] (HWC frames of one camera size,
 * contiguous) -> out_dev float32 [batch,3,out_h,out_w] in one launch.  Geometry exactly letterbox_image(img, (out_w, out_h))
 * (util.py:360-370: s = min(out_w / width, out_h / height) in double, new size int(dim * s), offsets (out - new) // 2);
 * interpolation, grey 128 fill, channel swap and /255 as rtod_prep_image (batch 1 with out_h == out_w == inp_dim gives its
 * bits).  Enqueues only. */
int rtod_prep_frames(const uint8_t* frames_dev, int batch, int height, int width, int bgr, int out_h, int out_w,
                     float* out_dev, void* stream);

/* replaces write_results                                     src/util.py:242-346
 * pred_dev [batch,n,5+num_class].  Writes detections rows [img,x1,y1,x2,y2,obj,score,cls] to
 * out_dev[cap][8] in the reference's order (image asc, class asc, objectness desc) and
 * counts_dev[0] = D (may exceed cap: then only cap rows were written), counts_dev[1] = number of
 * candidate rows (obj > conf) over the batch, counts_dev[2..2+batch) = detections per image.
 * Workspace: rtod_write_results_workspace(batch, n) bytes of device memory.  Enqueues only. */
int rtod_write_results_workspace(int batch, int n, size_t* bytes);
int rtod_write_results(const float* pred_dev, int batch, int n, int num_class, float confidence,
                       float nms_conf, float* out_dev, int cap, int32_t* counts_dev,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* (new; YOLOv5-style post-processing — the reference's YOLOv5 path is a torch.hub fetch, detect.py:255-285, so this follows the
 * published class-offset batched NMS, parity unpinned)  pred_dev [batch,n,5+num_class] rows (cx,cy,w,h,obj,cls...): candidates
 * obj > confidence and conf = obj * max class score > confidence; greedy NMS by descending conf on boxes shifted by
 * class * max_wh, suppression at IoU > iou_thr (no +1); rows [img,x1,y1,x2,y2,conf,obj,cls] per image by descending conf, at
 * most max_det per image; counts as rtod_write_results; same workspace size.  Enqueues only. */
int rtod_nms_class_offset(const float* pred_dev, int batch, int n, int num_class, float confidence, float iou_thr, float max_wh,
                          int max_det, float* out_dev, int cap, int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);

/* ---- validator: detections scored against ground truth -------------------------------------
 * replaces DarknetValidator.target_filter / pred_filter / compare_boxes / get_img_scores      test.py:62-151, 182-208
 * (as committed the reference's compare_boxes raises TypeError: its two helpers are @staticmethods declared with a `self`
 * parameter; the arithmetic restated here is what those helpers do when called directly).
 * Largest numbers of KEPT predictions / KEPT targets per image the kernel matches (1024 / 256). */
int rtod_score_detections_limits(int* max_pred_per_image, int* max_targets_per_image);
/* Bytes of device workspace for a call with these arguments (1 <= max_targets_per_image <= the limit). */
int rtod_score_detections_workspace(int batch, int cap, int max_targets_per_image, size_t* bytes);
/* One launch for the whole batch, one workgroup per image.  Enqueues only (no allocation, no host synchronisation: legal under
 * stream capture).  An image's results do not depend on the batch it rides in.  Per image b:
 *   rows      det_dev rows [sum counts[2..2+b), + counts[2+b]) — the output of rtod_write_results / rtod_nms_class_offset;
 *   kept predictions: column 7 is an integer in [0, num_class) whose bit is set in class_mask_host   (pred[i, -1] in permitted_classes)
 *   kept targets: t[2] > min_box_size and t[3] > min_box_size (strict, fp32) and the FIRST arg-max of t[5:5+num_class] permitted;
 *             box (cx - w/2, cy - h/2, cx + w/2, cy + h/2) in fp32                                   (xywh2xyxy, src/util.py:39-43)
 *             (target_corners != 0: columns 0-3 already hold those corners, the output of target_filter; the size test then
 *             reads columns 2 and 3 as they are, so pass min_box_size = -inf);
 *   M[i][j]   bbox_iou(pred[i,1:5], box_j) if (double)iou > iou_threshold (strict) else 0             (iou.item() > threshold)
 *   matching  at most P_f rounds, stop when max(M) == 0: first row holding the maximum, first column holding it in that row;
 *             row and column are zeroed, tp += 1 (torch's first-occurrence max / argmax: ties between equal boxes resolve so)
 *   scores_dev[b] = people_num = T_f, tp, fp = P_f - tp, fn = T_f - tp;  totals_dev[0..4) += the same (integer atomics; the caller
 *             zeroes; may be NULL)
 *   match_dev[r] (may be NULL), per detection row: -2 filtered out, -1 kept and unmatched (a false positive), else the matched
 *             target's index in the image's unfiltered target list;  match_iou_dev[r] (may be NULL): M of the matched pair, else 0
 *   status_dev[0] |= 1: counts[0] > cap (or counts that do not fit cap rows): every image's scores are -1, totals and match untouched;
 *                 |= 2: an image has more kept predictions than the limit or more kept targets than max_targets_per_image:
 *                       its scores are -1, the totals are untouched by it, its matching is not run (match_dev: -2 / -1 only).
 * tgt_dev: [T_total][5+num_class] rows (cx, cy, w, h, obj, one-hot...), the images' targets concatenated; tgt_offsets_dev
 * [batch+1] row offsets into it.  After the call the workspace holds every scored image's M: float
 * [batch][max_targets_per_image][ld], entry (b, j, i) for kept target j and kept prediction i, ld = min(max(cap, 1), 1024)
 * rounded up to 64.  RTOD_E_ARG (decided on the host, no device needed): a null pointer, batch < 1, cap < 0, num_class outside
 * 1..4096, max_targets_per_image outside 1..limit, a workspace that is too small or not 16-byte aligned, iou_threshold NaN. */
int rtod_score_detections(const float* det_dev, const int32_t* counts_dev, int cap, int batch,
                          const float* tgt_dev, const int32_t* tgt_offsets_dev, int num_class,
                          const uint32_t* class_mask_host, float min_box_size, double iou_threshold,
                          int max_targets_per_image, int target_corners, int32_t* scores_dev, int32_t* totals_dev,
                          int32_t* match_dev, float* match_iou_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- training loss, forward value only ---------------------------------------------------------
 * replaces DarknetTrainer.target_creator / target_layer / anchor_fit    train.py:129-209
 *          xywh2YOLO, bbox_iou_wh                                       src/util.py:48-75, 156-172
 *          DarknetTrainer.darknet_loss                                  train.py:211-230
 * One [yolo] head of the prediction tensor: grid_h x grid_w cells (separate: rtod_plan_create_rect), stride = input / grid,
 * n_anchors (<= 8) anchors as (w, h) pairs in input pixels.  Rows of a head: (gy * grid_w + gx) * n_anchors + a; the heads follow
 * one another in cfg order (at most 4). */
typedef struct rtod_yolo_head {
    int grid_h, grid_w, stride, n_anchors;
    int anchors[16];
} rtod_yolo_head;
/* Bytes of device workspace of rtod_yolo_loss(batch, n_rows); the same workspace serves rtod_darknet_loss_dense with
 * rows = batch * n_rows (that call needs 40 bytes per 1024 rows). */
int rtod_yolo_loss_workspace(int batch, int n_rows, size_t* bytes);
/* pred_dev [batch, n_rows, 5+num_class]: the TRAIN=True decode (rtod_plan_set_train_decode).  boxes_dev [sum T][5+num_class] rows
 * (cx, cy, w, h, 1, one-hot...) in input pixels, the images' boxes concatenated; box_offsets_dev [batch+1] row offsets into it.
 * Targets, the reference's behaviour as it is (per image and head):
 *   a box is skipped unless box[5] == 1 (only class 0 passes) and w >= min_box_size and h >= min_box_size (fp32; 24 in the reference);
 *   anchor = FIRST maximum over the head's anchors of the IoU of (w, h) with (anchor_w, anchor_w), in doubles (bbox_iou_wh reads
 *   the anchor's width twice; its height takes no part);
 *   x = cx / stride, gx = int(x), fx = x - gx in doubles, y likewise; row (gy * grid_w + gx) * n_anchors + anchor of the head;
 *   target row = the box's row with columns 0-3 replaced by (float(fy), float(fx), tw, th) — the centre slots are swapped in the
 *   reference — tw = float(log(double(w / float(anchor_w) + 1e-16f))) with the quotient and the sum in fp32, th likewise with the
 *   anchor's height;  of two boxes of an image on one row the LATER one wins; mask = 1 on such rows.
 *   (new) a box whose cell lies outside the grid (x or y negative, >= the grid, or NaN) is skipped for that head and
 *   status_dev[0] |= 1 (the reference wraps into the next grid row or raises IndexError); status_dev[0] |= 2: box_offsets_dev not
 *   ascending from >= 0 for an image, whose boxes are then ignored.  The caller zeroes status_dev.
 * Loss (sums over the batch, p = pred, t = target, accumulated in double, terms added in this order):
 *   loss_dev[1..5] = 5 sum_obj (p0-t0)^2 + (p1-t1)^2,  5 sum_obj (p2-t2)^2 + (p3-t3)^2,  sum_obj (p4-t4)^2,
 *                    0.5 sum_noobj (p4-t4)^2,  sum_obj sum_c (p_{5+c} - t_{5+c})^2;   loss_dev[0] = their sum.
 *   per_image_dev (may be NULL) [batch][6]: the same six numbers per image.  No floating-point atomics: workgroup partials are
 *   combined in a fixed order, the result is bit-identical from call to call.  A row without object reads only p4.
 * Optional outputs (NULL: not written): target_dev [batch, n_rows, 5+num_class] and mask_dev [batch, n_rows] (0 / 1), what
 * target_creator returns; n_obj_dev [batch]: masked rows per image.  Enqueues only (memset nodes + kernels: legal under stream
 * capture).  RTOD_E_ARG (decided on the host): a null pointer, batch / n_rows / num_class < 1, n_heads outside 1..4, a head with
 * n_anchors outside 1..8 or a non-positive grid, stride or anchor, heads whose rows do not add up to n_rows, a workspace that is
 * too small or not 8-byte aligned, min_box_size NaN. */
int rtod_yolo_loss(const float* pred_dev, int batch, int n_rows, int num_class,
                   const rtod_yolo_head* heads, int n_heads,
                   const float* boxes_dev, const int32_t* box_offsets_dev, float min_box_size,
                   double* loss_dev, double* per_image_dev, float* target_dev, uint8_t* mask_dev,
                   int32_t* n_obj_dev, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream);
/* darknet_loss(pred, target, obj_mask) on caller-supplied dense tensors: pred_dev / target_dev [rows, attrs], mask_dev [rows]
 * (non-zero = object), loss_dev [6] as above.  Same kernels and summation scheme as rtod_yolo_loss; workgroups take 1024
 * consecutive rows of the flat tensor, so for a one-image tensor the six doubles equal rtod_yolo_loss's bit for bit, for several
 * images they agree to the accuracy of a double sum.  RTOD_E_ARG: null pointer, rows < 1, attrs < 5, workspace. */
int rtod_darknet_loss_dense(const float* pred_dev, const float* target_dev, const uint8_t* mask_dev,
                            int64_t rows, int attrs, double* loss_dev, void* workspace, size_t workspace_bytes, void* stream);


/* ---- gradients of the detection-head convs --------------------------------------------------------
 * Gradient of the loss above with respect to the RAW head maps z (the outputs of the convs in front of the [yolo] layers), what
 * autograd gives through predict_transform(TRAIN=True) (src/util.py:175-239) and darknet_loss (train.py:211-230).  pred_dev is
 * the TRAIN=True decode of those maps.  With p a prediction row, t its target row, w = (5, 5, 5, 5, 1, 1, ...):
 *   object row     g_c = 2 w_c (p_c - t_c)                                  c = 0 .. 4 + num_class
 *   no-object row  g_4 = p_4 (= 2 * 0.5 * (p_4 - 0)), every other g_c = 0
 *   dz_c = g_c p_c (1 - p_c) for the sigmoid columns c in {0, 1, 4, 5, ...};  dz_c = g_c for c in {2, 3}
 * float32, one rounding per operation, in that order; a value the formula makes exactly 0 is stored as +0.
 * grad_raw_dev: the heads' maps concatenated, head h as [batch, A_h * attrs, GH_h, GW_h] NCHW (channel a * attrs + c at cell
 * (gy, gx) <-> prediction row (gy * GW + gx) * A + a of that head) at float offset batch * sum_{h' < h} A * attrs * GH * GW;
 * batch * n_rows * attrs floats in all, every one written (no need to zero).  grad_pred_dev (may be NULL): g, [batch, n_rows, attrs].
 * loss_dev (may be NULL): the six doubles, bit-identical to rtod_yolo_loss on the same arguments.  n_obj_dev (may be NULL) and
 * status_dev as there.  Targets, filters, the owner map and the status bits are exactly that call's; workspace:
 * rtod_yolo_loss_workspace.  Enqueues only (legal under stream capture).  RTOD_E_ARG as rtod_yolo_loss (and a NULL grad_raw_dev),
 * decided on the host. */
int rtod_yolo_loss_grad(const float* pred_dev, int batch, int n_rows, int num_class,
                        const rtod_yolo_head* heads, int n_heads,
                        const float* boxes_dev, const int32_t* box_offsets_dev, float min_box_size,
                        float* grad_raw_dev, float* grad_pred_dev, double* loss_dev,
                        int32_t* n_obj_dev, int32_t* status_dev,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Weight and bias gradient of a 1x1 convolution z = W x + b over dense NCHW maps:
 *   dw_dev[o][c] = sum_{b,p} dz[b,o,p] * x[b,c,p]   ([cout, cin], overwritten);   db_dev[o] = sum_{b,p} dz[b,o,p]   (may be NULL)
 * dz_dev [batch, cout, pixels], x_dev [batch, cin, pixels].  Exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): every partial sum is an
 * fmaf chain.  K = batch * pixels is summed in S contiguous slices, one workgroup per (64 x 64 tile of dW, slice), whose sums a
 * second kernel adds in ascending slice order; no floating-point atomics, so results are bit-identical from call to call.
 * Slice rule (K alone):  units = ceil(K / 8);  slice length L = 8 * ceil(units / 16);  S = ceil(K / L) <= 16.
 * Workspace: 4 * S * (cout * cin + cout) bytes, 16-byte aligned.  Shapes: cout >= 1 (any), cin a multiple of 32, pixels >= 1 (rows
 * of an image may start on any 4-byte boundary), batch * pixels < 2^31 - 64.  Enqueues only.  RTOD_E_ARG: a null pointer, a shape
 * outside those, a workspace that is too small or misaligned. */
int rtod_conv1x1_wgrad_workspace(int batch, int cout, int cin, int pixels, size_t* bytes);
int rtod_conv1x1_wgrad(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int pixels,
                       float* dw_dev, float* db_dev, void* workspace, size_t workspace_bytes, void* stream);
/* ---- gradients of the detection BLOCK convs (the BatchNorm conv a head conv reads), BatchNorm frozen ------------------
 * What torch's autograd leaves on conv.weight of the block under .eval() (running statistics, gamma / beta not trained).
 * Data gradient through a 1x1 convolution z = W y with the derivative of the activation that produced y:
 *   dx[b,c,p] = m(y[b,c,p]) * sum_o w[o,c] * dz[b,o,p],     m(y) = 1 for y > 0, else slope   (torch's leaky_relu backward; y == 0
 *   takes the slope).  y_dev is the STORED output of the block conv (rtod_plan_read_layer): a leaky-ReLU keeps the sign of its
 *   input, so no pre-activation is kept.  y_dev == NULL or slope == 1: linear, dx is the plain sum.
 * w_dev [cout, cin] (the head conv's float32 weights), dz_dev [batch, cout, pixels], y_dev / dx_dev [batch, cin, pixels].
 * Exact-fp32 MFMA: every dx element is ONE fmaf chain over o = 0 .. cout-1 (no K slices; ragged cout is padded with zeros, which
 * leave the chain unchanged), then one fp32 multiplication by the slope where the mask says so.  Plain stores, no atomics:
 * bit-identical from call to call.  Enqueues only.  RTOD_E_ARG: a null w / dz / dx, batch, cout or pixels < 1, cin not a
 * positive multiple of 32, slope NaN, batch * pixels >= 2^31 - 64. */
int rtod_conv1x1_dgrad(const float* w_dev, const float* dz_dev, const float* y_dev, float slope, int batch, int cout, int cin, int pixels,
                       float* dx_dev, void* stream);
/* (new) Data gradient through a size x size (1 or 3), stride 1, pad size / 2 convolution over dense NCHW maps, the generalisation of
 * rtod_conv1x1_dgrad over the taps:
 *   dx[b,c,y,x] = m(y_in[b,c,y,x]) * sum_{ky,kx,o} v[o,c,ky,kx] * dz[b,o,y+pad-ky,x+pad-kx]      (dz outside the map: an exact 0)
 *   v = (float)((double)w * s[o]): the folded fp32 weight rtod_plan_load_weights computes from the raw master w_oihw_dev
 *   [cout,cin,size,size] and the frozen scale row_scale_dev (rtod_plan_conv_scale); v = w when row_scale_dev is NULL.
 * m, y_dev and slope as rtod_conv1x1_dgrad: y_dev [batch,cin,height,width] is the STORED output of the layer the conv reads.
 * Exact-fp32 MFMA, 64 x 64 tiles of the [cin, batch * height * width] matrix.  The order of every sum is fixed by the shape alone:
 * tap-major (tap = ky * size + kx ascending), o ascending within a tap (as pairs (o, o + 1), like rtod_conv1x1_dgrad), cout padded
 * to a multiple of 32 with zeros.  Size 1: every dx element is ONE fmaf chain over o.  Size 3: one fmaf chain PER TAP over o, and the
 * nine tap sums are added in ascending tap order, total = total + chain, one fp32 add each, in the kernel's registers (a single chain
 * over 9 * cout terms errs by about 2^-24 sqrt(K) of the result, which at K = 4608 / 9216 was measured outside the project's 4 x the
 * float32 floor).  Then one fp32 multiplication by the slope where the mask says so.  No workspace, no second kernel, plain stores,
 * no atomics: bit-identical from call to call.  The size 1 call without a row scale is rtod_conv1x1_dgrad, bit for bit.  Enqueues only.  RTOD_E_ARG: as rtod_conv1x1_dgrad with height * width
 * for pixels, and size not 1 or 3, cout * cin * size * size >= 2^31. */
int rtod_conv_dgrad(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                    int batch, int cout, int cin, int height, int width, int size, float* dx_dev, void* stream);
/* (new) Data gradient through a 3x3, stride 2, pad 1 convolution over dense NCHW maps.  height x width is the conv's INPUT map;
 * ho = (height - 1) / 2 + 1, wo likewise; dz_dev [batch,cout,ho,wo], dx_dev and y_dev [batch,cin,height,width]:
 *   dx[b,c,iy,ix] = m(y[b,c,iy,ix]) * sum over taps (ky,kx) with (iy+1-ky) and (ix+1-kx) even, oy = (iy+1-ky)/2 in [0,ho),
 *                   ox = (ix+1-kx)/2 in [0,wo), of  chain_o v[o,c,ky,kx] * dz[b,o,oy,ox]
 * v, m, y_dev, slope and row_scale_dev exactly as rtod_conv_dgrad.  An even row takes ky = 1, an odd row ky = 0 and 2, columns
 * likewise: 1, 2, 2 or 4 taps by the pixel's parity class.  One fmaf chain per tap over o in ascending pairs, cout padded to 32 with
 * zeros; the class's taps are added in ascending tap order, total = total + chain, one fp32 add each; a tap of the class whose dz
 * pixel lies outside the map adds an exact 0; then one multiplication by the mask.  The GEMM columns are ordered by (class, b, iy / 2,
 * ix / 2) and each class is rounded up to whole 64-column tiles, so a workgroup runs its class's taps alone.  No workspace, plain
 * stores, no atomics: bit-identical from call to call.  Enqueues only.  Any height, width >= 1.  RTOD_E_ARG: as rtod_conv_dgrad, and
 * size not 3. */
int rtod_conv_dgrad_s2(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                       int batch, int cout, int cin, int height, int width, int size, float* dx_dev, void* stream);
/* (new) The fan-out point of the gradient walk in one launch: out[i] = m(y[i]) * (((c0[i] + c1[i]) + c2[i]) + c3[i]) over n floats,
 * `count` (1 to 4) contributions in contributions_dev_ptrs (a HOST array of device pointers), added left to right with one fp32 add
 * each, then one multiplication by slope where !(y > 0) (y_dev NULL or slope == 1: no mask; count 1 is the mask alone).  16-byte
 * loads where every pointer is 16-byte aligned, a scalar tail.  Bit-identical from call to call.  Enqueues only.  RTOD_E_ARG: a null
 * pointer, count outside 1..4, n < 1, slope NaN. */
int rtod_grad_join(const float* const* contributions_dev_ptrs, int count, const float* y_dev, float slope, long long n, float* out_dev, void* stream);
/* (new) Backward of the 2x [upsample]: dz_dev [batch,channels,2*height,2*width] -> dx_dev [batch,channels,height,width].
 * mode 0: bilinear, align_corners=False (the plan's forward, the reference's nn.Upsample): input row i is read by output rows
 * 2i-1 .. 2i+2 with weights 0.25, 0.75, 0.75, 0.25, the edge clamp of the forward putting both weights of a border row on the edge
 * (0.75 -> 1, the row outside dropped), columns alike; mode 1: nearest, the 2 x 2 outputs.  Gather form, one thread per input
 * pixel: acc = acc + (wy * wx) * dz over the (at most 4 x 4) outputs, rows ascending, then columns, fp32 without contraction, then
 * one multiplication by the mask m(y_dev) of the producing conv as in rtod_conv_dgrad (y_dev [batch,channels,height,width], NULL or
 * slope == 1: none).  No atomics: bit-identical from call to call.  Enqueues only.  RTOD_E_ARG: a null dz / dx, batch, channels,
 * height or width < 1, mode outside {0, 1}, slope NaN, 4 * height * width >= 2^31. */
int rtod_upsample2x_grad(const float* dz_dev, const float* y_dev, float slope, int mode, int batch, int channels, int height, int width,
                         float* dx_dev, void* stream);
/* Weight gradient of a size x size (1 or 3), stride 1, pad size / 2 convolution over dense NCHW maps:
 *   dw_dev[o][c][ky][kx] = sum_{b,y,x} dz[b,o,y,x] * x[b,c,y+ky-pad,x+kx-pad]     (OIHW, overwritten; a tap outside the map adds an exact 0)
 *   db_dev[o] = sum_{b,y,x} dz[b,o,y,x]                                           (may be NULL)
 * row_scale_dev (double [cout], may be NULL): the reduced sum of every element of row o of dW is multiplied by it once,
 * (float)((double)sum * row_scale[o]), one more rounding — the frozen BatchNorm scale of rtod_plan_conv_scale, which turns the
 * gradient of the folded conv into that of conv.weight.  db is never scaled.
 * The kernel of rtod_conv1x1_wgrad as an implicit GEMM with columns n = c * size * size + tap: exact-fp32 MFMA, one workgroup per
 * (64 x 64 tile of the [cout, cin * size * size] matrix, K slice), K = batch * height * width summed in S contiguous slices that
 * a second kernel adds in ascending order; no floating-point atomics; bit-identical from call to call and device to device.
 * Slice rule (K and the number of tiles alone):
 *   tiles = ceil(cout / 64) * ceil(cin * size * size / 64);   cap = min(16, ceil(1024 / tiles));
 *   units = ceil(K / 8);   slice length L = 8 * ceil(units / cap);   S = ceil(K / L) <= cap.
 * A grid of a thousand tiles fills the device unsliced (YOLOv3's 13 x 13 block: 1152 tiles, S = 1); the 26 x 26 block (288 tiles)
 * gets at most 4 slices, the 52 x 52 block (72 tiles) at most 15.
 * Workspace: 4 * S * (cout * cin * size * size + cout) bytes, 16-byte aligned (at most 19 MB for the YOLOv3 / YOLOv3-tiny blocks at
 * 416 x 416, batch 8).  Enqueues only.  RTOD_E_ARG: a null pointer, batch / cout / height / width < 1, cin not a positive
 * multiple of 32, size not 1 or 3, batch * height * width >= 2^31 - 64, cout * cin * size * size >= 2^31, a workspace that is
 * too small or misaligned. */
int rtod_conv_wgrad_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes);
int rtod_conv_wgrad(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                    const double* row_scale_dev, float* dw_dev, float* db_dev, void* workspace, size_t workspace_bytes, void* stream);
/* (new) Weight gradient of a 3x3, stride 2, pad 1 convolution.  height x width is the conv's INPUT map (x_dev [batch,cin,height,width]);
 * dz_dev [batch,cout,ho,wo] with ho = (height - 1) / 2 + 1, wo likewise:
 *   dw_dev[o][c][ky][kx] = sum_{b,oy,ox} dz[b,o,oy,ox] * x[b,c,2*oy+ky-1,2*ox+kx-1]      (a tap outside the map adds an exact 0)
 * db_dev, row_scale_dev, the two kernels, the slice rule and the workspace formula are those of rtod_conv_wgrad with K = batch * ho *
 * wo (the slice kernel is the same template with the stride as a parameter).  RTOD_E_ARG: as rtod_conv_wgrad, and size not 3. */
int rtod_conv_wgrad_s2_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes);
int rtod_conv_wgrad_s2(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                       const double* row_scale_dev, float* dw_dev, float* db_dev, void* workspace, size_t workspace_bytes, void* stream);
/* (new) Backward of a size-2 [maxpool] over dense NCHW maps.  x_dev [batch,channels,height,width] is the pool's stored INPUT (a dense
 * rtod_plan_read_layer copy), dz_dev lives on the pool's output map, dx_dev [batch,channels,height,width] is overwritten.
 *   stride 2: floor mode, output [height / 2, width / 2]; an odd last row or column is covered by no window and gets an exact +0
 *             (a one-pixel-wide or -high map has an empty output: dz_dev is then not read and may be NULL);
 *   stride 1: the clamped window of the forward (the reference's MaxPoolStride1: replicate pad right / bottom, MaxPool2d(2, 1)),
 *             output [height, width].
 * Gather form, one thread per input element: it visits the one window (stride 2) or the at most four windows (stride 1) that cover
 * it, recomputes each window's winner from x with the forward's rule — scan dy then dx, replace on strictly greater, so the FIRST
 * maximum wins (torch's rule); in a clamped window the duplicated edge taps are the same pixel, and the winner decided in scan order
 * is mapped to that pixel — and adds dz of the windows it won in ascending (oy, ox) order with fp32 adds; then one multiplication by
 * m(x) = x > 0 ? 1 : slope, the leaky mask of the conv that produced x, as rtod_upsample2x_grad (slope == 1: none).  On a split-f16
 * plan the dense copy is (hi + lo) / 8, exact, so the winner is the forward's.  No atomics, plain stores: bit-identical from call to
 * call.  Enqueues only.  NaN inputs are out of contract (the forward's comparison never picks a NaN, torch's propagates it).
 * RTOD_E_ARG: a null pointer, batch / channels / height / width < 1, size != 2, stride outside {1, 2}, slope NaN,
 * height * width >= 2^31.  A symmetric (padded) pool has no entry. */
int rtod_maxpool_grad(const float* dz_dev, const float* x_dev, float slope, int batch, int channels, int height, int width, int size,
                      int stride, float* dx_dev, void* stream);
/* (new) rtod_conv_wgrad for THIN convs: any cin >= 1, 1x1 or 3x3, stride 1, pad size / 2, no db.  The operands, the formula of dW,
 * row_scale_dev and the slice kernel are those of rtod_conv_wgrad; the tile is 32 x 128 of the [cout, cin * size * size] matrix (YOLOv3-
 * tiny's layer 0, 16 x 27, is one tile), and the slice count is cut for K = batch * height * width instead of capped at 16:
 *   tiles = ceil(cout / 32) * ceil(cin * size * size / 128);   target = ceil(1024 / tiles);
 *   L = 8 * ceil(ceil(K / 8) / target) clamped to [256, 1024];   S = ceil(K / L)            (rtod_conv_wgrad_thin_slices returns S and L)
 * so a large K launches at least 1024 workgroups (layer 0 at 416 x 416, batch 8: K = 1,384,448, L = 1024, S = 1352) and no fmaf chain
 * has more than 1024 terms — the longest chain measured inside the project's 4 x the-float32-floor gate (the per-tap chain of a
 * 1024-filter conv in rtod_conv_dgrad; single chains of 4608 and 9216 terms were measured outside it).  The S slice sums of an element
 * are added as a fixed two-level tree: groups of 32 consecutive slices in ascending order, then the group sums in ascending order;
 * then row_scale once, in double, as rtod_conv_wgrad.  Plain stores, no atomics: bit-identical from call to call.
 * Workspace: 4 * S * cout * cin * size * size bytes, 16-byte aligned.  Enqueues only.  RTOD_E_ARG: a null pointer, batch / cout / cin /
 * height / width < 1, size not 1 or 3, batch * height * width >= 2^31 - 1024, cout * cin * size * size >= 2^31, a workspace that is
 * too small or misaligned. */
int rtod_conv_wgrad_thin_slices(int batch, int cout, int cin, int height, int width, int size, int* slices, int* slice_len);
int rtod_conv_wgrad_thin_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes);
int rtod_conv_wgrad_thin(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                         const double* row_scale_dev, float* dw_dev, void* workspace, size_t workspace_bytes, void* stream);
/* (new) rtod_conv_dgrad for THIN convs: any cin >= 1, 1x1 or 3x3, stride 1.  The recipe of rtod_conv_dgrad element for element: one
 * fmaf chain per tap over o in ascending pairs, the tap sums added in ascending tap order, one multiplication by the mask.  Rows past
 * cin are staged as zeros and never stored.  RTOD_E_ARG: as rtod_conv_dgrad without the multiple-of-32 rule. */
int rtod_conv_dgrad_thin(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                         int batch, int cout, int cin, int height, int width, int size, float* dx_dev, void* stream);
/* (new) The FULL graph of a plan: the BatchNorm convs, in ascending order, of the set rtod_plan_trainable_layers defines with two more
 * traversable kinds:
 *   a folded-BatchNorm conv, 1x1 or 3x3 / stride 1 / same padding, leaky or linear, of ANY Cin, layer 0 included, packed in a generic
 *   layout (layer 0's fp32 panel pads its 3 channels per tap to 4; a stem-layout layer 0 and a narrow-layout conv stay out);
 *   a [maxpool] of size 2, stride 1 or 2, without symmetric padding (rtod_maxpool_grad).
 * Option "keep_full_activations" (default 0) is to this graph what "keep_backbone_activations" is to the trainable graph, and a
 * superset of it: the same fusions are held, every buffer a full-graph conv or pool reads or writes stays live, the frozen scales of
 * all its convs go to the device and the three folded-conv entries accept them.  With it, fp32: YOLOv3-tiny all 11 BatchNorm convs
 * (0, 2, 4, 6, 8, 10, 12, 13, 14, 18, 21); YOLOv3 the trainable list (its layer 0 runs the stem kernel; with "stem_kernel" = 0 all 72).
 * conv_layers / input_layers (-1 for layer 0: the network input) / capacity and the return value as rtod_plan_neck_layers. */
int rtod_plan_full_layers(const rtod_plan* plan, int* conv_layers, int* input_layers, int capacity);
/* (new) Backward of batch-statistics BatchNorm (nn.BatchNorm2d in .train(), what the reference's trainer runs: train.py:57, 77) over
 * dense NCHW float32 maps.  du_dev [batch,channels,pixels]: the gradient with respect to the BatchNorm OUTPUT (the leaky mask already
 * applied); z_dev, same shape: the raw conv output the forward normalised; mean_dev / var_dev (double [channels]): the statistics
 * the forward normalised with (biased variance; rtod_plan_bn_batch_stats reads the same values); gamma_dev (float [channels]).  Per
 * channel, N = batch * pixels, r = 1 / sqrt(var + 1e-5) in double (the forward's expression, one header for both):
 *   S1 = sum (double)du                      S2 = sum (double)du * ((double)z - mean)
 *   dbeta_dev[c]  = (float)S1                dgamma_dev[c] = (float)(S2 * r)
 *   dz_dev[i] = (float)( gamma * r * ( ((double)du[i] - S1 / N) - ((double)z[i] - mean) * (r * r * S2 / N) ) )
 * double operations with one rounding each, no contraction; dz_dev, dgamma_dev, dbeta_dev are overwritten.
 * Two launches, no atomics.  A channel's N values, n = b * pixels + p, are cut into `parts` contiguous ranges of `part_len`:
 *   target = min(256, ceil(2048 / channels));   part_len = 1024 * ceil(ceil(N / target) / 1024);   parts = ceil(N / part_len)
 * (rtod_bn_grad_parts returns both) — the shape alone, never the device.  The first launch, one workgroup of 256 threads per (channel,
 * part), adds each thread's values in ascending order and the 256 thread sums in a fixed LDS tree, all in double, and writes one (S1,
 * S2) pair per (channel, part); the second, on the same grid, adds a channel's pairs in ascending order in every workgroup's
 * prologue and writes dz over its part.  Planes start at any 4-byte alignment (pixels = 169): a part is walked as the 16-byte
 * aligned quads of memory it touches, whole quads by 16-byte accesses, a run's head and tail element by element.  Bit-identical from
 * call to call and from device to device.  Workspace: 16 * channels * parts bytes.  Enqueues only (legal under stream capture).
 * RTOD_E_ARG: a null pointer; batch, channels or pixels < 1; batch * pixels >= 2^29; channels * parts >= 2^31; du_dev, z_dev, dz_dev
 * or the workspace not 16-byte aligned, mean_dev or var_dev not 8-byte aligned; a workspace that is too small. */
int rtod_bn_grad_parts(int batch, int channels, int pixels, int* parts, int* part_len);
int rtod_bn_grad_workspace(int batch, int channels, int pixels, size_t* bytes);
int rtod_bn_grad(const float* du_dev, const float* z_dev, const double* mean_dev, const double* var_dev, const float* gamma_dev,
                 int batch, int channels, int pixels, float* dz_dev, float* dgamma_dev, float* dbeta_dev,
                 void* workspace_dev, size_t workspace_bytes, void* stream);
/* (new) rtod_conv_dgrad on the forward's split-f16 MFMA tiles (opt-in; dgrad_split.hip).  Operands and result are those of
 * rtod_conv_dgrad: dx = m(y) * conv_T(dz, v), v = (float)((double)w * row_scale[o]) or w, dense fp32 NCHW, size 1 or 3, stride 1,
 * cin a positive multiple of 32, any cout >= 1 (K is padded with zero channels to a multiple of 32).  The arithmetic:
 *   dz       per image b, a_b = max |dz[b]|, e_b puts a_b 2^e_b in [2^12, 2^13) (a_b == 0: e_b = 0; e_b held to -126 .. 126);
 *            dz 2^e_b stored as f16 hi = RNE(v), lo = RNE(v - hi), NHWC split layout (no 8 x).  Per image: an image's dx does not
 *            depend on the batch it rides in.
 *   weights  row c of the gradient conv (the forward's input channel) is pre-scaled like an output channel of the forward's packed
 *            weights: max over o and taps of |(double)w * row_scale| placed in [2^12, 2^13), e_c in -24 .. 40, an all-zero row e_c = 0;
 *            hi / lo planes [chunk][Npad][32], K index ((o / 32) * taps + tap') * 32 + o % 32, tap' = taps - 1 - tap.  Packed on the
 *            device from the masters at every call.
 *   sum      hi*hi + hi*lo + lo*hi in the MFMA's fp32 accumulators, by the raw-sum instance of an existing forward tile.
 *   finish   dx[b][c] = m(y) * (sum * 2^-e_c * 2^-e_b): exact scales, one rounding multiplication (the mask).
 * rtod_conv_dgrad_split_tiles (no device): the number of legal tile ids of the shape, the default first, by the rules that pick the
 * forward's tiles (band layers W <= 94: the bandd modes of their K-group count; 94 < W <= 160 with Npad % 128 == 0: the wide tile too;
 * 1x1 with K a multiple of 64: the slab tiles too; the generic tiles for the rest); at most `capacity` ids are written.  tile = -1
 * runs the default; an id outside the list: RTOD_E_ARG.  Workspace: rtod_conv_dgrad_split_workspace bytes, 16-byte aligned; every
 * byte a kernel reads is written earlier in the same call.  Seven launches on `stream`, nothing synchronises, no host read of device
 * memory, no atomics: bit-identical from call to call and from tile to tile; legal under stream capture.  RTOD_E_ARG, each text
 * starting with the entry's name: a null w / dz / dx / workspace, batch, cout, height or width < 1, batch > 65535, cin not a
 * positive multiple of 32, size not 1 or 3, slope NaN, batch * pixels >= 2^31 - 256, a split dz buffer (4 * batch * pixels * K bytes)
 * or a weight plane (2 * K * taps * Npad bytes) of 2 GiB or more, a workspace that is too small or misaligned. */
int rtod_conv_dgrad_split_tiles(int batch, int cout, int cin, int height, int width, int size, int* ids, int capacity);
int rtod_conv_dgrad_split_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes);
int rtod_conv_dgrad_split(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                          int batch, int cout, int cin, int height, int width, int size, int tile,
                          float* dx_dev, void* workspace, size_t workspace_bytes, void* stream);
/* ... for measurement (tools/exp_grad_split.py): the same call enqueues only the kernel groups named in `phases`, a sum of 1 (the
 * images' maxima and exponents), 2 (dz to split planes), 4 (row maxima and weight pack), 8 (the conv) and 16 (the finish), on a
 * workspace that a full call of the same shape has filled.  31 is rtod_conv_dgrad_split; outside 1 .. 31: RTOD_E_ARG. */
int rtod_conv_dgrad_split_phases(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                                 int batch, int cout, int cin, int height, int width, int size, int tile,
                                 float* dx_dev, void* workspace, size_t workspace_bytes, void* stream, int phases);
/* (new) rtod_conv_wgrad as three f16 MFMA products (opt-in; wgrad_split.hip): a size x size (1 or 3), stride 1, pad size / 2 BatchNorm
 * conv, cin a positive multiple of 32, any cout >= 1, dense fp32 NCHW dz [batch, cout, height, width] and x [batch, cin, height, width]:
 *   dW[o][c][ky][kx] = row_scale[o] * sum_{b,y,x} dz[b,o,y,x] * x[b,c,y+ky-p,x+kx-p]          (x an exact zero outside the map; no db)
 * The arithmetic, defined free of any summation order:
 *   exponents  ONE per tensor (dW is a sum over the batch): a = max |t|, e = 13 - frexp(a).exp, so that a 2^e lies in [2^12, 2^13);
 *              a == 0 or not finite: e = 0; e held to -126 .. 126.  e_z for dz, e_x for x.
 *   split      v = t 2^e (exact), hi = RNE_f16(v), lo = RNE_f16(v - hi); subnormal halves are kept.
 *   sum        zh*xh + zh*xl + zl*xh over all (b, y, x), products of halves summed in fp32 by v_mfma_f32_32x32x16_f16; zl*xl is absent
 *              by definition.
 *   finish     dW = (float)((double)sum * 2^-(e_z + e_x) * row_scale[o]) (row_scale_dev NULL: the factor 1): one rounding, in double;
 *              2^-(e_z + e_x) need not be a normal float.
 * dz and x are re-laid as channel-major f16 planes on a common padded k grid (size 3: [batch][height + 2][Wp], Wp = 8 * ceil((width +
 * 2) / 8), halo written as zeros in both; size 1: the flat batch * height * width), rounded up with zeros to k_padded, a multiple of
 * 16; a workgroup owns a tile of dW (3x3: 64 filters x 64 channels x all nine taps; 1x1: 128 x 128) over one K slice.
 * rtod_conv_wgrad_split_schedule (no device): tiles, slices, slice_len and k_padded of the shape; with u = k_padded / 16 and
 * want = max(1, min(64, ceil(1024 / tiles), u / 4)): slice_len = 16 * ceil(u / want), slices = ceil(k_padded / slice_len) <= want (the
 * workspace holds `want` slice sums): a pure function of the shape.  The slice sums are
 * added in ascending order; no atomics: bit-identical from call to call.  rtod_conv_wgrad_split_bounds (no device): the lowest and
 * the highest half index, from the start of a plane of plane_halves halves (guards included), that the GEMM forms for the shape; the
 * split kernel writes every half of every plane, so 0 <= lowest and highest < plane_halves is the bounds proof of the call.
 * Workspace: rtod_conv_wgrad_split_workspace bytes, 16-byte aligned; every byte a kernel reads is written earlier in the same call.
 * Five launches on `stream`, nothing synchronises, no host read of device memory; legal under stream capture.  RTOD_E_ARG, each text
 * starting with the entry's name: a null dz / x / dw / workspace, batch, cout, height or width < 1, cin not a positive multiple of 32,
 * size not 1 or 3, the padded k grid or cout * cin * size * size beyond int32, a plane of 2 GiB or more, cout + cin > 65535, a workspace
 * that is too small or misaligned. */
int rtod_conv_wgrad_split_schedule(int batch, int cout, int cin, int height, int width, int size,
                                   int* tiles, int* slices, int* slice_len, int64_t* k_padded);
int rtod_conv_wgrad_split_bounds(int batch, int cout, int cin, int height, int width, int size,
                                 int64_t* lowest, int64_t* highest, int64_t* plane_halves);
int rtod_conv_wgrad_split_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes);
int rtod_conv_wgrad_split(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                          const double* row_scale_dev, float* dw_dev, void* workspace, size_t workspace_bytes, void* stream);
/* ... for measurement (tools/exp_wgrad_split.py): the same call enqueues only the kernel groups named in `phases`, a sum of 1 (maxima and
 * exponents), 2 (the split), 4 (the GEMM) and 8 (the reduce), on a workspace that a full call of the same shape has filled.  15 is
 * rtod_conv_wgrad_split; outside 1 .. 15: RTOD_E_ARG. */
int rtod_conv_wgrad_split_phases(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                                 const double* row_scale_dev, float* dw_dev, void* workspace, size_t workspace_bytes, void* stream,
                                 int phases);

/* ---- optimiser step of a detection-head conv, on the stream ------------------------------------------
 * replaces optim.Adam(self.darknet.parameters(), lr=1e-2) + optimizer.step()     train.py:57, 412-425
 * for the convs rtod_plan_update_conv accepts that are 1x1 (the convs in front of the [yolo] layers).  One kernel per call
 * (head_step.hip) applies the step to the caller's float32 masters and moments IN PLACE and writes the conv's ranges of the plan's
 * packed weight image — fp32 panel, or split-f16 hi / lo planes with the per-channel power-of-two pre-scale and its inverse, and
 * the bias — with the bits rtod_plan_load_weights / rtod_plan_update_conv would give for those masters.  The image keeps its
 * addresses: the next forward on that stream, and a captured graph of the forward, read the new weights.  Padding channels,
 * padding K and every other conv's block are not written.
 *   kind 0, SGD    w' = fl(w - fl(lr32 * g)), lr32 = (float)lr: two roundings, no fused multiply-add (torch's w.sub_(g * lr));
 *                  beta1, beta2, eps, step and the moment pointers are ignored (pass NULL).
 *   kind 1, Adam   torch.optim.Adam without weight decay and amsgrad; `step` is the 1-based count t of this step.  The host forms
 *                  in double and rounds to float:  a = lr / (1 - beta1^t),  r = sqrt(1 - beta2^t),  c1 = 1 - beta1,  c2 = 1 - beta2,
 *                  where lr, beta1 and beta2 are read as the SHORTEST DECIMAL that rounds to the float given (0.999f means 0.999,
 *                  as it prints; 1 - (double)0.999f would miss 0.001 by 2^-25 / 0.001, hundreds of ulps of every v');
 *                  beta2 and eps reach the kernel as the floats given.  Per element, fp32, one rounding per line (fmaf = one):
 *                      d   = g - m
 *                      m'  = fmaf(d, c1, m)
 *                      q   = g * g
 *                      p   = beta2 * v
 *                      v'  = fmaf(q, c2, p)
 *                      s   = sqrt(v')             (correctly rounded)
 *                      s   = s / r                (correctly rounded)
 *                      den = s + eps
 *                      u   = m' / den             (correctly rounded)
 *                      w'  = fmaf(-a, u, w)
 *                  m_w_dev / v_w_dev ([Cout, Cin], torch's exp_avg / exp_avg_sq) and m_b_dev / v_b_dev ([Cout]) are read and written.
 * weight_dev [Cout, Cin] (OIHW of a 1x1 conv) and bias_dev [Cout] are read and written; dw_dev / db_dev are what rtod_conv1x1_wgrad
 * wrote.  The bias takes the same step.  No floating-point atomics: results are bit-identical from call to call.
 * Enqueues only — no allocation, no host copy, no synchronisation: legal under stream capture, the promise of rtod_forward.  It is
 * ordered against forwards by stream order alone; a forward of this plan in flight on ANOTHER stream may read a half-written
 * block, which is the caller's business.
 * RTOD_E_ARG, all decided before anything touches the device: a null plan, opt or required pointer; a layer that is not a
 * convolution, has BatchNorm or is part of a fused pointwise pair (as rtod_plan_update_conv); a stem or narrow (Cin == 16) layout
 * or a kernel size other than 1; kind outside {0, 1}; a non-finite lr; Adam with step < 1, a beta outside [0, 1), a negative eps
 * or a null moment pointer.  RTOD_E_STATE before rtod_plan_load_weights. */
typedef struct rtod_opt_step { int kind; float lr, beta1, beta2, eps; int step; } rtod_opt_step;
int rtod_plan_step_conv(rtod_plan* plan, int layer, const rtod_opt_step* opt,
                        float* weight_dev, float* bias_dev, const float* dw_dev, const float* db_dev,
                        float* m_w_dev, float* v_w_dev, float* m_b_dev, float* v_b_dev, void* stream);
/* (new) The same step for a detection BLOCK conv (rtod_plan_head_blocks), BatchNorm frozen: the device twin of
 * rtod_plan_update_conv_weight.  One kernel, one workgroup per output channel: the step above (same fp32 sequence, same host-derived
 * scalars) on the RAW float32 master weight_dev [Cout, Cin, k, k] and the moments m_w_dev / v_w_dev of that shape, from dw_dev (what
 * rtod_conv_wgrad wrote with the plan's scale), then the row is packed again as rtod_plan_load_weights packs a BatchNorm conv, with
 * s = rtod_plan_conv_scale:   folded v = (float)((double)w' * s[o]);   split plans: channel exponent e from max |(double)w' * s[o]|
 * (e = 13 - frexp exponent, held to -24 .. 40, 0 for an all-zero row), vs = v * 2^e, hi = f16_rn(vs), lo = f16_rn(vs - hi),
 * inv[o] = 2^-e / 8;   fp32 plans: the panel element v.  The bias slot (beta - mean * s) and everything outside rows [0, Cout) x
 * columns [0, Cin * k * k) of the conv's block keep their bits.  Enqueues only (legal under stream capture), ordered by the stream.
 * RTOD_E_ARG, all decided before anything is enqueued: a null plan, opt, weight_dev or dw_dev; a layer that is not a block (no
 * BatchNorm, a stem, a narrow conv, a pair member, any other conv: the message says which); the opt refusals of
 * rtod_plan_step_conv (Adam needs both moment pointers).  RTOD_E_STATE: before rtod_plan_load_weights; a plan without option
 * "keep_block_inputs" (its scales are not on the device). */
int rtod_plan_step_conv_folded(rtod_plan* plan, int layer, const rtod_opt_step* opt, float* weight_dev, const float* dw_dev,
                               float* m_w_dev, float* v_w_dev, void* stream);
/* ---- training under batch statistics (plan options "bn_batch_stats" + "keep_bn_inputs": exact fp32, or f16s3 with "bn_batch_split") ----
 * On an f16s3 plan the option is accepted exactly when "bn_batch_stats" and "bn_batch_split" are both set (every other plan of
 * precision 1 or 2 refuses it, RTOD_E_CFG), and not together with "bn_split_narrow", "stem_pool" or "k_slices_split".  The raw-sum
 * instance of every trained conv then writes its own buffer instead of the shared scratch — the forward's bits do not change —,
 * rtod_plan_read_bn_input returns those fp32 rows, and rtod_plan_step_conv_bn re-packs what that instance reads: the unfolded hi / lo
 * planes, the per-channel pre-scale (inv_scale) and the [beta, gamma] block.  rtod_plan_describe marks the plan "bn_batch_trained":"split".
 * replaces .train() + optim.Adam(self.darknet.parameters()) + loss.backward() through nn.BatchNorm2d     train.py:57, 77, 412-425
 * (new) rtod_plan_read_bn_input: beside rtod_plan_read_layer, a dense NCHW copy [batch, Cout, H, W] of the raw conv output z that the
 * last forward's normalise step read for `layer` — the z of rtod_bn_grad.  RTOD_E_ARG: a null pointer, a batch outside 1..max_batch, a
 * layer that is no BatchNorm conv the plan trains (the message says why: an eval plan, no "keep_bn_inputs", outside the kept scope, a
 * shortcut in its normalise step).  RTOD_E_STATE before rtod_plan_load_weights. */
int rtod_plan_read_bn_input(rtod_plan* plan, int layer, int batch, float* out_dev_nchw, void* stream);
/* (new) Device addresses of the mean and the biased variance (double [Cout] each) the last forward normalised `layer` with, in the style
 * of rtod_plan_conv_scale: the mean_dev / var_dev of rtod_bn_grad, the values rtod_plan_bn_batch_stats copies to the host.  The
 * addresses stay valid for the plan's life; every forward overwrites the values.  Any BatchNorm conv of a "bn_batch_stats" plan. */
int rtod_plan_bn_stats_dev(const rtod_plan* plan, int layer, const double** mean_dev, const double** var_dev);
/* (new) rtod_plan_step_conv_folded for a conv whose BatchNorm runs on batch statistics: one optimiser step (the fp32 sequence of
 * rtod_plan_step_conv, same host-derived scalars) on the float32 masters weight_dev [Cout, Cin, k, k], gamma_dev [Cout] and beta_dev
 * [Cout] from dw_dev, dgamma_dev and dbeta_dev (rtod_conv_wgrad of the dz rtod_bn_grad wrote, and that entry's dgamma / dbeta), Adam
 * moments m_* / v_* of the same shapes (all six or, for SGD, NULL), and the re-pack in place: the unfolded fp32 panel where
 * rtod_plan_load_weights puts it (scale 1; the bias slot keeps its zeros) and the [beta, gamma] block of the image — bit-identical
 * to a load of the stepped stream.  head_step.hip's kernel in one more mode: its extra workgroup steps the two vectors.  One launch;
 * enqueues only (legal under stream capture); every refusal is decided before anything is enqueued.  RTOD_E_ARG: a null plan, opt
 * or required pointer, the opt refusals of rtod_plan_step_conv, a layer rtod_plan_read_bn_input refuses (an eval plan: use
 * rtod_plan_step_conv_folded).  RTOD_E_STATE before rtod_plan_load_weights.  Weight decay is not offered. */
int rtod_plan_step_conv_bn(rtod_plan* plan, int layer, const rtod_opt_step* opt, float* weight_dev, const float* dw_dev, float* gamma_dev, float* beta_dev,
                           const float* dgamma_dev, const float* dbeta_dev, float* m_w_dev, float* v_w_dev, float* m_gamma_dev, float* v_gamma_dev,
                           float* m_beta_dev, float* v_beta_dev, void* stream);
/* (new) Its host twin, in the style of rtod_plan_update_conv_weight: the conv's block re-packed from the three host arrays through the
 * packing of rtod_plan_load_weights and uploaded alone.  Synchronises. */
int rtod_plan_update_conv_bn(rtod_plan* plan, int layer, const float* weight_oihw_host, const float* gamma_host, const float* beta_host);
/* (tests, debugging) The packed weight image as it is on the device now, copied to the host; SYNCHRONISES the device.  Size query
 * as rtod_plan_pack_weights: *needed (if given) receives the image's floats, with out_host == NULL nothing else happens, else
 * capacity_floats must cover it (RTOD_E_SIZE).  RTOD_E_STATE before rtod_plan_load_weights. */
int rtod_plan_read_packed_weights(rtod_plan* plan, float* out_host, size_t capacity_floats, size_t* needed);

#ifdef __cplusplus
}
#endif
#endif /* RTOD_H */
