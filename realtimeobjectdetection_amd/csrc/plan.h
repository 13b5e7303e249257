// Static execution plan of a Darknet cfg on one GPU: layer IR, NHWC buffer arena with liveness
// reuse, zero-copy route concat, fused shortcut / head-decode epilogues, packed weights, launch list.
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "rtod_internal.h"

namespace rtod {

enum LayerType { LT_CONV = 0, LT_SHORTCUT, LT_ROUTE, LT_UPSAMPLE, LT_MAXPOOL, LT_YOLO };
const char* layer_type_name(int t);

struct Layer {
    int index = 0;
    int type = LT_CONV;
    int cin = 0, cout = 0, hin = 0, win = 0, hout = 0, wout = 0;
    int size = 0, stride = 1, pad = 0;
    bool bn = false;
    int act = 0;                  // 0 linear, 1 leaky(0.1), 2 SiLU (cfg extension)
    bool nearest = false;         // upsample: mode=nearest (cfg extension; the reference builds bilinear)
    bool decode_v5 = false;       // yolo: decode=v5 (cfg extension: YOLOv5-style head arithmetic)
    int pool_pad = 0;             // maxpool: symmetric=1 -> (size-1)/2 of -inf padding per side (cfg extension)
    std::vector<int> srcs;                       // absolute layer indices (route / shortcut)
    std::vector<std::pair<int, int>> anchors;    // yolo: masked (w,h) pairs
    int classes = 0, row_offset = 0, rows = 0;
    int64_t w_off = 0;                           // float offset of this conv's block in the .weights payload
    // planning results
    int fused_into = -1;      // conv: index of the shortcut/yolo layer whose output it writes
    bool fused_away = false;  // shortcut / yolo executed inside the preceding conv's epilogue
    int buf = -1, coff = 0;   // materialised output: arena buffer id + channel offset (-1: none/alias)
    int alias_of = -1;        // single-source route / yolo: same view as that layer
    int z_buf = -1;           // BatchNorm conv of a batch-statistics plan with option keep_bn_inputs that the plan trains (Plan::trains_bn): the arena buffer of its
                              // raw sums z, rows of Plan::z_stride floats, live from the conv to the end of the forward (-1: normalised in place, or from the shared scratch)
    int bn_pool = -1;         // BatchNorm conv of a batch-statistics split plan (options bn_split_narrow + fuse_bn_pool): index of the 2x2 / stride-2
                              // max-pool that alone reads it and that its normalise kernel can run (candidate; Plan::form decides at run time)
};

struct Buffer {
    int C = 0, H = 0, W = 0;      // C = ldc (full pixel width)
    int first = 0, last = 0;      // launch-time interval (layer indices) in which it is live
    int64_t floats_per_frame = 0;
    int64_t offset = 0;           // floats from arena base, for max_batch frames
    bool bn_input = false;        // the kept raw sums of a BatchNorm conv (Layer::z_buf): placed behind the arena of the other buffers, never reused
};

enum LaunchKind { LK_CONV = 0, LK_PACK = 1, LK_UPSAMPLE = 2, LK_ADD = 3, LK_MAXPOOL = 4, LK_DECODE = 5, LK_COPY = 6, LK_STEM = 7 };

struct Launch {
    int kind = LK_CONV;
    int layer = 0;
    int in_layer = -1;        // layer whose output view is read (-1: network input buffer)
    int in2_layer = -1;       // residual / second operand
    int out_layer = -1;       // layer whose view is written (-2: final [B,N,attrs] output)
    int out_buf = -1, out_coff = 0;   // for LK_COPY into a concat slice
    int conv_slot = -1;       // index into Plan::convs
    DecodeArgs dec;
    // split-f16 plans: a 1x1 conv that directly follows a conv whose workgroups hold all output channels runs in that
    // conv's epilogue (conv_f16s3_common.h).  pw_guest: launch index of the 1x1 conv hosted by this launch; pw_host:
    // launch index of the host (this launch is then skipped).  Candidates are found at plan build (liveness covers
    // both schedules); Plan::form decides at run time.
    int pw_guest = -1, pw_host = -1;
};

// The form in which a launch runs: the plan's candidates (Launch::pw_guest / pw_host, Layer::bn_pool, Plan::stem2_pattern,
// stem_pool_pattern) under the precision, the options and keep_all_layers.  Plan::form is the one place that decides it.
struct LaunchForm {
    int inside = -1;       // >= 0: this launch enqueues nothing, that launch's kernel does its work (stem in layer 1's kernel, max-pool in the
                           // stem's or in a conv's normalise kernel, 1x1 guest in its host's epilogue)
    // conv and stem launches that run
    bool stem2 = false;    // conv: the fused stem kernel (conv_stem2_f16s3.hip); launch 0's stem rides here
    int guest = -1;        // conv: launch index of the 1x1 conv it hosts in its epilogue
    bool raw = false;      // raw-sum step of a batch-statistics split plan: raw sums, statistics, normalise
    int pool = -1;         // layer index of the 2x2 max-pool that its kernel (16-filter stem) or its normalise kernel also runs
    int epi = 0;           // conv: epilogue code of the kernel instance (EPI_* of conv_f16s3_common.h, | EPI_F16, or EPI_RAW)
};
// ... and what that leaves of a layer: the fused_into it reports, and whether its own output is stored and can be read back
struct LayerForm { int fused_into; bool readable; };

struct PackedConv {
    int layer = 0;
    int cin_p = 0, K = 0, Kpad = 0, Npad = 0;
    int64_t w_off = 0, b_off = 0;     // float offsets into the device weight arena
    bool stem16 = false;              // stem on conv_stem16_f16s3.hip (option stem_pool: 16 filters, split packing of `stem`)
    bool stem = false;                // conv_stem.hip: weights [28][Cout] fp32, or (split) [Cout][32] f16 hi / lo planes + inv_scale
    bool split = false;               // f16 hi/lo planes (conv_igemm_f16s3) instead of an fp32 panel
    bool band = false;                // eligible for conv_band_f16s3 (3x3 s1 p1, band fits LDS)
    bool narrow = false;              // split, Cin == 16 (option narrow_cin): tap-major K order, runs on conv_c16_f16s3 only
    int64_t wl_off = 0, s_off = 0;    // split: w_off = hi plane, wl_off = lo plane (float units), s_off = inv_scale
    int64_t stats_off = -1;           // batch-statistics BatchNorm plans: this layer's [Npad] mean, [Npad] variance in Plan::d_bn_stats (doubles)
    int64_t bn_off = 0;               // batch-statistics BatchNorm plans: [Npad] beta, [Npad] gamma (the conv itself is packed unfolded)
    int slice_chunks = 0;             // exact-fp32 panels: K summed in slices of this many 32-wide chunks (0: one chain), conv_igemm_f32.hip
    int ks_chunks = 0;                // split, option k_slices_split: sliced layer (slices of this many K-chunks), runs on conv_ks_f16s3 only; 0: not sliced
};

// What a plan can train with BatchNorm frozen, narrowest first: the conv in front of each head conv, the neck, everything but layer 0.
// Options keep_block_inputs / keep_neck_activations / keep_backbone_activations keep the activations of one each (Plan::kept_scope)
// keep_full_activations: the full graph (thin convs, layer 0 on a generic layout and size-2 max-pools too: YOLOv3-tiny's backbone)
enum Scope { SCOPE_NONE = 0, SCOPE_BLOCKS, SCOPE_NECK, SCOPE_BACKBONE, SCOPE_FULL };

// One struct, defined over five files by concern (the run-time fused form of every launch is decided in one place, Plan::form in plan_forward.cpp): plan_cfg.cpp (parse, resolve_shapes: no HIP call), plan_build.cpp (options, buffer
// planning, weight layout, describe), plan_weights.cpp (pack_conv, pack_weights, load_weights; repack_conv under update_conv / update_conv_weight, step_packed under step_conv / step_conv_folded), plan_tiles.cpp (which kernel variant a conv
// launch runs, autotune), plan_forward.cpp (the launch list on a stream, launch records).
struct Plan {
    int height = 0, width = 0, max_batch = 0, device = 0;
    std::map<std::string, std::string> net_info;
    std::vector<Layer> layers;
    std::vector<Buffer> bufs;
    int input_buf = -1;
    std::vector<Launch> launches;
    std::vector<PackedConv> convs;
    int total_rows = 0, attrs = 0;
    int64_t n_weight_floats = 0, conv_flops = 0;
    int64_t arena_floats = 0, packed_floats = 0;
    float* d_arena = nullptr;
    float* d_weights = nullptr;
    double* d_bn_stats = nullptr;     // batch-statistics BatchNorm: per-channel mean / biased variance of every BN layer's last forward
    int64_t bn_stats_doubles = 0;
    double* d_bn_partial = nullptr;   // per-range partial sums of the two-stage statistics kernel
    int64_t bn_partial_count = 0;
    float* d_bn_raw = nullptr;        // option bn_batch_split: the raw sums of the BatchNorm conv that is running, fp32 rows [M][raw_stride] (never in place:
                                      // an fp32 slice of a zero-copy concat pixel would overlap the other producers' hi / lo planes)
    int64_t bn_raw_floats = 0;        // max over BatchNorm convs of max_batch * hout * wout * raw_stride (layout_weights); 0 unless bn_split_active()
    float* d_scratch = nullptr;       // slice panels of the one-workgroup-per-K-slice schedules (exact-fp32 plans; split plans with a sliced layer)
    int64_t scratch_floats = 0;
    bool weights_loaded = false;
    int train_decode = 0;
    int precision = 0;         // 0 = exact fp32 MFMA, 1 = f16 hi/lo split (3 products), 2 = plain f16 (hi plane only, 1 product)
    bool keep_all = false;     // debug: no arena reuse, every layer output stays readable after forward
    // plan options (rtod_plan_set_option, before rtod_plan_load_weights).  Explicit per-plan state: the library reads no
    // environment variable.
    bool opt_fuse_pointwise = true;   // run a 1x1 conv in the previous conv's epilogue where the plan allows it
    bool opt_stem_kernel = true;      // dedicated NCHW-reading kernel for layer 0 (else pack + generic conv)
    bool opt_band_kernel = true;      // LDS-band kernel for the 3x3 stride-1 layers it supports
    bool opt_bn_batch_stats = false;  // exact-fp32 plans: BatchNorm on the statistics of the batch (what the reference runs: no .eval()), not folded
    bool opt_bn_batch_split = false;  // ... on the split-f16 kernels (precision 1 only; inert without bn_batch_stats): raw-sum conv instances, statistics,
                                      // a normalise kernel that writes the split format
    bool opt_bn_split_narrow = false; // ... (read only when that mode is in force) also on the narrow tiles and the 16-filter stem: YOLOv3-tiny's 16-channel layers
    bool opt_fuse_bn_pool = true;     // ... with bn_split_narrow: the 2x2 / stride-2 max-pool that alone reads a BatchNorm conv runs in its normalise kernel
    bool opt_k_slices = true;         // exact-fp32 kernels: deep small-grid layers summed in K slices (own workgroups when the grid is small)
    bool opt_k_slice_workgroups = true;   // ... (off: always the in-workgroup schedule — same bits; A/B and tests).  Governs conv_ks_f16s3 too
    bool opt_k_slices_split = false;  // precisions 1 / 2: deep small-grid convs summed in K slices on conv_ks_f16s3.hip (single-frame latency; opt-in)
    bool opt_stem2_kernel = true;     // stem + layer 1 (+ hosted 1x1) in one kernel when the cfg starts like Darknet-53 (split-f16 plans)
    bool opt_patch_kernel = true;     // 2-D patch tiles among the autotune candidates of the wide 3x3 stride-1 layers
    bool opt_ring_kernel = true;      // persistent LDS-DMA ring tiles among the autotune candidates of the other layers
    bool opt_pwd_kernel = true;       // slab tiles (conv_pwd_f16s3.hip) among the autotune candidates of the plain 1x1 layers
    bool opt_fuse_shortcut = true;    // shortcut in the producing conv's epilogue (else stand-alone add kernel)
    bool opt_fuse_decode = true;      // head decode in the head conv's epilogue (else stand-alone decode kernel)
    bool opt_zero_copy_concat = true; // route producers write straight into the concat buffer (else copy kernels)
    bool opt_narrow_cin = false;      // precisions 1 / 2 accept convs after layer 0 that read exactly 16 channels (conv_c16_f16s3.hip)
    bool opt_stem_pool = false;       // precisions 1 / 2: a 3x3 / stride 1 / 16-filter layer 0 runs the split-f16 stem of conv_stem16_f16s3.hip (no pack launch)
    bool opt_keep_head_inputs = false; // the buffer every conv in front of a [yolo] layer reads stays live to the end of the forward (rtod_plan_read_layer after it:
                                      // the activations of rtod_conv1x1_wgrad); liveness only: launches, tiles and output bits are unchanged
    bool opt_keep_block_inputs = false; // ... and the buffer every BLOCK conv reads (block_shape_ok: the BatchNorm conv a head conv reads): the activations of
                                      // rtod_conv_wgrad.  Liveness only as well; the frozen BatchNorm scales then also live on the device (d_block_scale)
    bool opt_keep_neck_activations = false; // ... and every buffer a NECK conv (scope_graph) or a head conv reads or writes: the activations of the walk behind the
                                      // backbone (rtod_conv_dgrad, rtod_upsample2x_grad, rtod_conv_wgrad).  Liveness only; the scales of all neck convs on the device
    bool opt_keep_backbone_activations = false; // a superset of keep_neck_activations over the TRAINABLE convs (scope_graph: stride-2 convs and shortcuts too).  Not
                                      // liveness only: the plan then forms no fusion that hides a trainable conv (fusions_held, next to form)
    bool opt_keep_full_activations = false; // a superset of keep_backbone_activations over the FULL graph (scope_graph(SCOPE_FULL): convs of any Cin, layer 0 on a generic
                                      // layout, size-2 max-pools).  Holds the same fusions
    bool opt_keep_bn_inputs = false;  // batch-statistics plans, exact fp32 or f16s3 with bn_batch_split (inert without bn_batch_stats on fp32, refused on any other plan): the raw output z of every BatchNorm
                                      // conv the plan trains survives the forward in a buffer of its own (Layer::z_buf) — the operand of rtod_bn_grad —, and the
                                      // *_shape_ok predicates stop excluding the plan: the listings are those of the eval plan with the same keep option
    bool opt_fuse_stem_pool = true;   // ... with the 2x2 / stride-2 max-pool that follows it in the same kernel where the plan allows it (off: A/B and tests)
    int opt_force_f16s3_variant = -1; // >= 0: tile variant for every split-f16 conv (>= BAND_VARIANT_BASE: band layers)
    int opt_force_f32_variant = -1;   // >= 0: tile variant for every exact-fp32 conv
    int32_t* overflow_flag = nullptr; // caller-owned device word: split-f16 producers OR 1 into it when a value saturates
    std::vector<hipEvent_t> events;

    ~Plan();
    int parse(const std::string& cfg_text);
    int resolve_shapes();
    int plan_buffers();
    DecodeArgs decode_args(const Layer& yolo) const;
    int replan_or(const std::function<void()>& restore);   // re-plan after an option / precision change; refused: restore, re-plan, keep the message
    void assign_arena();
    void layout_weights();
    bool uses_split(const Layer& L) const;
    int check_split_supported(int mode) const;   // mode 1 (f16s3) or 2 (f16): same layout requirements
    int pack_weights(const float* w, size_t n, std::vector<float>& packed) const;   // the packed image, on the host (no HIP call)
    void pack_conv(const PackedConv& pc, const float* p, float* blk) const;         // one conv: its block of the stream -> its block of the image (blk = image + pc.w_off)
    int64_t conv_block_floats(size_t slot) const;                                   // floats of that block: every range of the conv, padding to the next conv included
    int load_weights(const float* w, size_t n);
    // one conv trained alone.  Two kinds of conv are accepted, each by its own refusals (replaceable_conv: no BatchNorm; block_conv:
    // a detection block); underneath there is one host re-pack (repack_conv) and one device step (step_packed)
    struct ConvSite { int slot = -1; bool pair = false; };                          // slot in `convs` (-1: none); host or guest of a fused-pointwise candidate pair
    int conv_site(const char* who, int layer, ConvSite& cs) const;                  // refuses a layer that is no convolution
    int repack_conv(size_t slot, const std::vector<float>& stream);                 // pack_conv of the conv's block of the stream, uploaded alone (synchronises)
    int step_packed(const char* who, size_t slot, const rtod_opt_step* opt, bool moments, bool folded, HeadStepLaunch& h, hipStream_t s);   // scalars, state, one launch
    int update_conv(int layer, const float* weight_oihw, const float* bias);        // re-pack and upload one conv without BatchNorm (rtod_plan_update_conv)
    int replaceable_conv(const char* who, int layer, size_t& slot) const;            // the conv's slot, or why it cannot be replaced alone
    int step_conv(int layer, const rtod_opt_step* opt, float* weight, float* bias, const float* dw, const float* db,
                  float* m_w, float* v_w, float* m_b, float* v_b, hipStream_t s);   // optimiser step + re-pack on the stream (rtod_plan_step_conv)
    int read_packed_weights(float* out, size_t capacity, size_t* needed) const;     // the device image back on the host (synchronises)
    // detection blocks (rtod_plan_head_blocks): the BatchNorm conv that a head conv reads, trained with BatchNorm frozen
    bool block_shape_ok(int layer) const;                                           // the cfg's part of the definition (what keep_block_inputs keeps alive)
    bool block_plan_ok(int layer) const;                                            // the plan's part: generic packed layout, no pair member, output stored
    int block_of_head(int head_conv_layer) const;                                   // the block conv of that head conv, or -1
    // the detection neck (rtod_plan_neck_layers): the largest set of traversable layers (head convs, block-shaped BatchNorm convs that pass
    // block_plan_ok, routes, 2x upsamples) closed downstream: every reader of a member is a member or a [yolo] layer
    std::vector<std::vector<int>> consumers() const;                                // the readers of every layer's output, ascending
    std::vector<char> scope_graph(Scope scope) const;                               // membership per layer of the neck (SCOPE_NECK) or of the trainable graph
                                                                                    // (SCOPE_BACKBONE: the two more kinds); no member below SCOPE_NECK
    // the trainable graph (rtod_plan_trainable_layers): the neck's closure rule with two more traversable kinds, a block-shaped conv
    // that is 3x3 / stride 2 / pad 1 instead of stride 1, and a two-source linear [shortcut]
    bool train_shape_ok(int layer) const;                                           // block_shape_ok, or block_shape_ok but for that stride
    // the full graph (rtod_plan_full_layers): two more kinds again, a block-shaped conv of ANY Cin (layer 0 included) and a size-2 max-pool
    bool stem_kernel_shape() const;                                                 // layer 0 has the shape the dedicated stem kernel takes, and option stem_kernel is on
    bool full_shape_ok(int layer) const;                                           // train_shape_ok, or block_shape_ok but for Cin and the layer-0 rule
    Scope kept_scope() const {                                                      // the widest scope whose activations the options keep: decided here alone
        return opt_keep_full_activations ? SCOPE_FULL : opt_keep_backbone_activations ? SCOPE_BACKBONE : opt_keep_neck_activations ? SCOPE_NECK : opt_keep_block_inputs ? SCOPE_BLOCKS : SCOPE_NONE;
    }
    bool trained_member(int layer, const std::vector<char>& kept) const;            // a block conv on every plan, and every BatchNorm conv of the kept graph
    bool batch_trained() const { return opt_bn_batch_stats && opt_keep_bn_inputs; } // batch-statistics BatchNorm whose convs, gamma and beta train
    bool trains_bn(int layer, const std::vector<char>& kept) const { return batch_trained() && trained_member(layer, kept); }
    bool trains_bn(int layer) const { return batch_trained() && trained_member(layer, scope_graph(kept_scope())); }
    int bn_conv(const char* who, int layer, size_t& slot) const;                    // the slot of a conv that trains_bn, or why `layer` is none
    View bn_input_view(int layer) const;                                            // the kept raw sums z of that conv (base null: none)
    int z_stride(const Layer& L) const;                                             // floats per row of that buffer: Cout (fp32 plan) or raw_stride (split plan)
    int read_bn_input(int layer, int batch, float* out_nchw, hipStream_t s) const;  // rtod_plan_read_bn_input
    int bn_stats_dev(int layer, const double** mean_dev, const double** var_dev) const;   // rtod_plan_bn_stats_dev
    int step_conv_bn(int layer, const rtod_opt_step* opt, float* weight, const float* dw, float* gamma, float* beta, const float* dgamma, const float* dbeta,
                     float* m_w, float* v_w, float* m_g, float* v_g, float* m_b, float* v_b, hipStream_t s);   // rtod_plan_step_conv_bn
    int update_conv_bn(int layer, const float* weight_oihw, const float* gamma, const float* beta);   // its host twin (rtod_plan_update_conv_bn)
    bool trains_folded(int layer, const std::vector<char>& kept) const;             // what block_conv accepts: a block conv on every plan, and every BatchNorm conv of
    bool trains_folded(int layer) const;                                            // kept = scope_graph(kept_scope()) (load_weights asks that graph once for all layers)
    int block_conv(const char* who, int layer, size_t& slot) const;                 // the slot of a block conv, or why `layer` is none
    int update_conv_weight(int layer, const float* weight_oihw);                    // re-pack and upload one block conv, BatchNorm as loaded (rtod_plan_update_conv_weight)
    int step_conv_folded(int layer, const rtod_opt_step* opt, float* weight, const float* dw, float* m_w, float* v_w, hipStream_t s);   // rtod_plan_step_conv_folded
    int conv_scale(int layer, const double** scale_dev, double* scale_host, int channels) const;   // rtod_plan_conv_scale
    int opt_scalars(const char* who, const rtod_opt_step* opt, bool moments, HeadStepLaunch& h) const;   // the checked step scalars of step_conv / step_conv_folded
    std::map<int, std::vector<float>> block_bn;     // block conv layer -> its [beta, gamma, mean, var] of the stream last loaded
    std::map<int, std::vector<double>> block_scale; // ... -> gamma / sqrt(var + 1e-5), the frozen scale pack_conv folds
    std::map<int, int64_t> block_scale_off;         // ... -> offset in d_block_scale (doubles)
    double* d_block_scale = nullptr;                // options keep_block_inputs / keep_neck_activations / keep_backbone_activations: the scales on the device, allocated at the first load
    int64_t block_scale_doubles = 0;                // ... and how many doubles that allocation holds
    bool feeds_yolo(int layer) const { return layers[layer].type == LT_CONV && layer + 1 < (int)layers.size() && layers[layer + 1].type == LT_YOLO; }
    int forward(const float* x, int batch, float* out, hipStream_t s, float* launch_ms, bool tune = false);
    // the launches of one LK_CONV / LK_STEM step of forward, in order
    int run_conv(size_t li, const LaunchForm& f, const float* x, int batch, float* out, hipStream_t s, bool tune_now);
    int run_conv_f32(const Launch& l, const LaunchForm& f, ConvArgs& a, int batch, hipStream_t s) const;
    int run_conv_split(size_t li, const LaunchForm& f, ConvArgs& a, int batch, hipStream_t s, bool tune_now);
    int run_stem(const Launch& l, const LaunchForm& f, const float* x, int batch, hipStream_t s) const;
    int raw_bn_begin(const Launch& l, int batch, bool site_ok, View& raw) const;        // raw view of a batch-statistics BatchNorm step, checked once
    int run_raw_bn(const Launch& l, const View& raw, int pool, int batch, hipStream_t s) const;   // ... its statistics + normalise (+ max-pool layer `pool`); the only caller of launch_bn_batch_split
    int finish_decode(float* out, int batch, hipStream_t s) const;   // TRAIN=True output -> eval decode in place (rtod_plan_finish_decode)
    int set_option(const char* name, int value);
    int set_precision(int mode);              // re-plans: the launch list depends on the precision (option stem_pool)
    int set_tiles(int batch, const int* variants, int count);   // install a tile table (validated per launch)
    void reset_planning();
    View view_of(int layer) const;            // resolves aliases; base == nullptr if not materialised
    int choose_variant(const Layer& L, int batch) const;
    int build_conv_args(const Launch& l, const LaunchForm& f, int batch, float* out, ConvArgs& a) const;
    int tune_launch(size_t li, ConvArgs& a, int batch, hipStream_t s);
    std::vector<int> tuning;                    // scratch of the tuning forward
    std::map<std::vector<int>, int> tune_cache;
    // split-f16 tiles (ids: split_tiles.cpp): the rules live in these four, and launch_split_variant refuses by the same family facts
    bool tile_legal(const Launch& l, int v) const;            // may this launch run tile v and give the layer's defined bits?
    int default_tile(const Launch& l, int batch) const;                  // closed-form choice per kind of layer
    int variant_for(const Launch& l, int batch) const;                   // forced or tuned id if legal, else the default
    std::vector<int> tile_candidates(const Launch& l, int batch) const;  // what autotune times, in screening order
    int launch_split_variant(ConvArgs& a, const PackedConv& pc, int v, hipStream_t s) const;
    int f32_slice_mode(const Launch& l, int batch, int variant) const;   // 0 plain, 1 slices inside the workgroup, 2 one workgroup per slice
    bool ks_sched_b_fits(const Launch& l, int batch) const;              // sliced split layer: the slice panels of this batch fit the scratch
    bool bn_split_active() const { return opt_bn_batch_stats && opt_bn_batch_split && precision == 1; }   // batch-statistics BatchNorm on the split kernels
    bool raw_launch(const Launch& l) const { return bn_split_active() && l.kind == LK_CONV && layers[l.layer].bn; }   // a BatchNorm conv of such a plan: raw sums, then normalise
    bool bn_narrow_active() const { return bn_split_active() && opt_bn_split_narrow; }   // ... narrow tiles, 16-filter stem and fused pools included
    int raw_stride(const PackedConv& pc) const;           // floats per row of the raw-sum scratch: Npad; narrow tiles and the 16-filter stem: Cout rounded up to 8
    View bn_raw_view(const Launch& l, int batch) const;   // fp32 view of this launch's raw sums: the conv's kept buffer (Layer::z_buf) if it has one, else over d_bn_raw
    bool stem2_pattern = false;                 // launches 0 / 1 are a stem and the stride-2 conv conv_stem2_f16s3 fuses (candidate, set by plan_buffers)
    bool stem_pool_pattern = false;             // launch 0 is the 16-filter stem and launch 1 the 2x2 / stride-2 max-pool that alone reads it (candidate, set by plan_buffers)
    bool fusions_held() const;                  // option keep_backbone_activations: plan_buffers forms no shortcut fusion, no pointwise pair, no stem2 pattern
    LaunchForm form(size_t li) const;           // how launch li runs; computed on demand (keep_all_layers changes it without planning again)
    LayerForm layer_form(int layer) const;      // ... and what describe and the layer readers report of a layer
    std::map<int, std::vector<int>> tuned;     // batch -> per-launch split-f16 tile variant (-1: heuristic)
    std::string describe() const;
    void fill_launch_info(int idx, rtod_launch_info* o, int batch) const;

private:                                        // the run-time predicates over the candidates: read by form / layer_form alone
    bool pw_active() const;                     // fused pointwise convs in use (precision 1, option fuse_pointwise)
    bool stem2_active() const;                  // stem2_pattern, and the plan runs it fused (split-f16 precision, option stem2_kernel, not under keep_all_layers)
    int fused_pool(int layer) const;            // the max-pool layer that conv `layer`'s kernel (stem_pool_pattern) or normalise kernel (Layer::bn_pool) runs, or -1
};

}  // namespace rtod
