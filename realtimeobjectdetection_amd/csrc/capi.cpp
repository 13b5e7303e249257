// extern "C" surface of librtod.so (declared in include/rtod.h).  Nothing throws across it.
#include <cstring>
#include <new>

#include "plan.h"

namespace rtod { const std::string& last_error_string(); }
using namespace rtod;

struct rtod_plan { Plan p; };

#define RTOD_GUARD_BEGIN try {
#define RTOD_GUARD_END                                                                   \
    } catch (const std::bad_alloc&) { set_error("out of host memory"); return RTOD_E_ARG; } \
      catch (const std::exception& e) { set_error("internal error: %s", e.what()); return RTOD_E_ARG; } \
      catch (...) { set_error("internal error"); return RTOD_E_ARG; }

extern "C" {

int rtod_version(void) { return 100; }

int rtod_last_error(char* buf, size_t len) {
    if (!buf || !len) return RTOD_E_ARG;
    const std::string& e = last_error_string();
    const size_t n = e.size() < len - 1 ? e.size() : len - 1;
    memcpy(buf, e.data(), n);
    buf[n] = 0;
    return RTOD_OK;
}

int rtod_device_count(int* out) {
    if (!out) return RTOD_E_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *out = 0; (void)hipGetLastError(); return RTOD_OK; }
    *out = n;
    return RTOD_OK;
}

// rtod_plan_create (`who` = "plan_create": square inputs only) and rtod_plan_create_rect
static int plan_create(const char* who, bool square, const char* cfg_text, size_t len, int height, int width, int max_batch, int device, rtod_plan** out) {
    if (!cfg_text || !out) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    *out = nullptr;
    if (height < 1 || width < 1 || max_batch < 1 || device < 0) { set_error("%s: bad geometry %dx%d batch %d device %d", who, height, width, max_batch, device); return RTOD_E_ARG; }
    if (square && height != width) { set_error("%s: only square inputs are supported (the reference derives every stride from net_info['height']); use rtod_plan_create_rect", who); return RTOD_E_ARG; }
    rtod_plan* h = new rtod_plan();
    h->p.height = height; h->p.width = width; h->p.max_batch = max_batch; h->p.device = device;
    int rc = h->p.parse(std::string(cfg_text, len));
    if (!rc) rc = h->p.resolve_shapes();
    if (!rc) rc = h->p.plan_buffers();
    if (rc) { delete h; return rc; }
    *out = h;
    return RTOD_OK;
}

int rtod_plan_create(const char* cfg_text, size_t len, int height, int width, int max_batch, int device, rtod_plan** out) {
    RTOD_GUARD_BEGIN
    return plan_create("plan_create", true, cfg_text, len, height, width, max_batch, device, out);
    RTOD_GUARD_END
}

int rtod_plan_create_rect(const char* cfg_text, size_t len, int height, int width, int max_batch, int device, rtod_plan** out) {
    RTOD_GUARD_BEGIN
    return plan_create("plan_create_rect", false, cfg_text, len, height, width, max_batch, device, out);
    RTOD_GUARD_END
}

int rtod_plan_destroy(rtod_plan* plan) {
    delete plan;
    return RTOD_OK;
}

int rtod_plan_get_info(const rtod_plan* plan, rtod_plan_info* o) {
    if (!plan || !o) { set_error("plan_get_info: null pointer"); return RTOD_E_ARG; }
    const Plan& p = plan->p;
    memset(o, 0, sizeof(*o));
    o->n_layers = (int32_t)p.layers.size(); o->n_launches = (int32_t)p.launches.size();
    o->height = p.height; o->width = p.width; o->max_batch = p.max_batch;
    o->total_rows = p.total_rows; o->attrs = p.attrs;
    o->n_weight_floats = p.n_weight_floats; o->conv_flops_per_frame = p.conv_flops;
    o->arena_bytes = p.arena_floats * 4; o->packed_weight_bytes = p.packed_floats * 4;
    return RTOD_OK;
}

int rtod_plan_get_launch(const rtod_plan* plan, int index, rtod_launch_info* out) {
    if (!plan || !out || index < 0 || index >= (int)plan->p.launches.size()) { set_error("plan_get_launch: bad index"); return RTOD_E_ARG; }
    plan->p.fill_launch_info(index, out, plan->p.tuned.empty() ? plan->p.max_batch : plan->p.tuned.rbegin()->first);
    return RTOD_OK;
}

int rtod_plan_describe(const rtod_plan* plan, char* buf, size_t len, size_t* needed) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("plan_describe: null plan"); return RTOD_E_ARG; }
    const std::string s = plan->p.describe();
    if (needed) *needed = s.size() + 1;
    if (buf && len) {
        const size_t n = s.size() < len - 1 ? s.size() : len - 1;
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return RTOD_OK;
    RTOD_GUARD_END
}

int rtod_plan_pack_weights(const rtod_plan* plan, const float* w, size_t n_floats, float* out, size_t capacity_floats, size_t* needed_floats) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("pack_weights: null plan"); return RTOD_E_ARG; }
    if (needed_floats) *needed_floats = (size_t)plan->p.packed_floats;
    if (!out) return RTOD_OK;
    if (capacity_floats < (size_t)plan->p.packed_floats) { set_error("pack_weights: capacity %zu < %lld floats", capacity_floats, (long long)plan->p.packed_floats); return RTOD_E_SIZE; }
    std::vector<float> packed;
    if (int rc = plan->p.pack_weights(w, n_floats, packed)) return rc;
    if (!packed.empty()) memcpy(out, packed.data(), sizeof(float) * packed.size());
    return RTOD_OK;
    RTOD_GUARD_END
}

const char* rtod_conv_variant_name(int variant) {
    if (variant == 100 + STEM2_VARIANT) return "conv_stem2_f16s3<2 x 4x16, stem + 3x3 s2 + 1x1>";
    if (variant >= 100) { const TileRef t = family_of(variant - 100); return t ? t.fam->info(t.mode).name : ""; }   // split-f16 tiles: 100 + id
    if (variant < 0 || variant % 10 >= CV_COUNT || variant / 10 > 2) return "";
    static const char* const kSliced[2][CV_COUNT] = {
        {"conv_igemm_f32<128x128,w64x64,k-slices>", "conv_igemm_f32<128x64,w64x32,k-slices>", "conv_igemm_f32<64x64,w32x32,k-slices>", "conv_igemm_f32<128x32,w32x32,k-slices>"},
        {"conv_igemm_f32<128x128,w64x64,wg per k-slice>", "conv_igemm_f32<128x64,w64x32,wg per k-slice>", "conv_igemm_f32<64x64,w32x32,wg per k-slice>", "conv_igemm_f32<128x32,w32x32,wg per k-slice>"}};
    if (variant >= 10) return kSliced[variant / 10 - 1][variant % 10];
    return conv_variant_info(variant).name;
}

int rtod_conv_kernel_name(int variant, int epilogue, char* buf, size_t len) {
    if (!buf || len == 0) { set_error("conv_kernel_name: null buffer"); return RTOD_E_ARG; }
    int n = -1;
    if (variant >= 100) { const TileRef t = family_of(variant - 100); if (t) n = t.fam->kernel_name(t.mode, epilogue, buf, len); }
    else n = conv_f32_kernel_name(variant, buf, len);
    if (n < 0 || (size_t)n >= len) { set_error("conv_kernel_name: unknown variant %d or buffer too small", variant); return RTOD_E_ARG; }
    return RTOD_OK;
}

int rtod_plan_launch_kernel_name(const rtod_plan* plan, int index, char* buf, size_t len) {
    RTOD_GUARD_BEGIN
    if (!plan || !buf || len == 0 || index < 0 || index >= (int)plan->p.launches.size()) { set_error("launch_kernel_name: bad args"); return RTOD_E_ARG; }
    const LaunchForm f = plan->p.form(index);
    buf[0] = 0;
    if (plan->p.launches[index].kind != LK_CONV || f.inside >= 0) return RTOD_OK;      // non-conv launch / conv hosted by the previous launch: empty name
    if (f.stem2) {
        const int n = conv_stem2_kernel_name(f.guest >= 0, buf, len);
        if (n < 0 || (size_t)n >= len) { set_error("launch_kernel_name: buffer too small"); return RTOD_E_ARG; }
        return RTOD_OK;
    }
    rtod_launch_info li;                                                               // (the tile the plan reports for this launch)
    plan->p.fill_launch_info(index, &li, plan->p.tuned.empty() ? plan->p.max_batch : plan->p.tuned.rbegin()->first);
    return rtod_conv_kernel_name(li.variant, f.epi, buf, len);
    RTOD_GUARD_END
}

int rtod_plan_set_precision(rtod_plan* plan, int mode) {
    if (!plan || mode < 0 || mode > 2) { set_error("set_precision: mode must be 0 (fp32), 1 (f16 split) or 2 (plain f16)"); return RTOD_E_ARG; }
    if (plan->p.d_weights) { set_error("set_precision: must be called before rtod_plan_load_weights"); return RTOD_E_STATE; }
    RTOD_GUARD_BEGIN
    return plan->p.set_precision(mode);
    RTOD_GUARD_END
}

int rtod_plan_set_option(rtod_plan* plan, const char* name, int value) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("set_option: null plan"); return RTOD_E_ARG; }
    return plan->p.set_option(name, value);
    RTOD_GUARD_END
}

int rtod_plan_set_overflow_flag(rtod_plan* plan, int32_t* flag_dev) {
    if (!plan) { set_error("set_overflow_flag: null plan"); return RTOD_E_ARG; }
    plan->p.overflow_flag = flag_dev;
    return RTOD_OK;
}

int rtod_plan_load_weights(rtod_plan* plan, const float* w, size_t n_floats) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("load_weights: null plan"); return RTOD_E_ARG; }
    return plan->p.load_weights(w, n_floats);
    RTOD_GUARD_END
}

int rtod_forward(rtod_plan* plan, const float* x_dev, int batch, float* out_dev, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("forward: null plan"); return RTOD_E_ARG; }
    return plan->p.forward(x_dev, batch, out_dev, (hipStream_t)stream, nullptr);
    RTOD_GUARD_END
}

int rtod_plan_autotune(rtod_plan* plan, const float* x_dev, int batch, float* out_dev, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("autotune: null plan"); return RTOD_E_ARG; }
    return plan->p.forward(x_dev, batch, out_dev, (hipStream_t)stream, nullptr, true);
    RTOD_GUARD_END
}

int rtod_plan_get_tiles(const rtod_plan* plan, int batch, int* variants, int capacity) {
    if (!plan) { set_error("get_tiles: null plan"); return RTOD_E_ARG; }
    auto it = plan->p.tuned.find(batch);
    if (it == plan->p.tuned.end()) { set_error("get_tiles: batch %d has no tile table (run rtod_plan_autotune first)", batch); return RTOD_E_STATE; }
    const int n = (int)it->second.size();
    if (variants) {
        if (capacity < n) { set_error("get_tiles: capacity %d < %d launches", capacity, n); return RTOD_E_ARG; }
        for (int i = 0; i < n; ++i) variants[i] = it->second[i];
    }
    return n;
}

int rtod_plan_set_tiles(rtod_plan* plan, int batch, const int* variants, int count) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("set_tiles: null plan"); return RTOD_E_ARG; }
    return plan->p.set_tiles(batch, variants, count);
    RTOD_GUARD_END
}

int rtod_forward_timed(rtod_plan* plan, const float* x_dev, int batch, float* out_dev, void* stream, float* launch_ms) {
    RTOD_GUARD_BEGIN
    if (!plan || !launch_ms) { set_error("forward_timed: null pointer"); return RTOD_E_ARG; }
    return plan->p.forward(x_dev, batch, out_dev, (hipStream_t)stream, launch_ms);
    RTOD_GUARD_END
}

int rtod_plan_set_train_decode(rtod_plan* plan, int train) {
    if (!plan) { set_error("set_train_decode: null plan"); return RTOD_E_ARG; }
    plan->p.train_decode = train ? 1 : 0;
    return RTOD_OK;
}

int rtod_plan_finish_decode(rtod_plan* plan, float* pred_dev, int batch, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("finish_decode: null plan"); return RTOD_E_ARG; }
    return plan->p.finish_decode(pred_dev, batch, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_plan_set_keep_all_layers(rtod_plan* plan, int keep) {
    if (!plan) { set_error("set_keep_all_layers: null plan"); return RTOD_E_ARG; }
    if (plan->p.d_arena) { set_error("set_keep_all_layers: must be called before rtod_plan_load_weights"); return RTOD_E_STATE; }
    plan->p.keep_all = keep != 0;
    plan->p.assign_arena();
    return RTOD_OK;
}

int rtod_plan_layer_shape(const rtod_plan* plan, int layer, int* c, int* h, int* w) {
    if (!plan || layer < 0 || layer >= (int)plan->p.layers.size() || !c || !h || !w) { set_error("layer_shape: bad args"); return RTOD_E_ARG; }
    const View v = plan->p.view_of(layer);
    if (v.C == 0 || !plan->p.layer_form(layer).readable) { set_error("layer %d is fused into its consumer and has no materialised output", layer); return RTOD_E_STATE; }
    *c = v.C; *h = v.H; *w = v.W;
    return RTOD_OK;
}

int rtod_plan_read_layer(rtod_plan* plan, int layer, int batch, float* out_dev_nchw, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan || layer < 0 || layer >= (int)plan->p.layers.size()) { set_error("read_layer: bad args"); return RTOD_E_ARG; }
    if (batch < 1 || batch > plan->p.max_batch) { set_error("read_layer: bad batch"); return RTOD_E_ARG; }
    const View v = plan->p.view_of(layer);
    if (!v.base || !plan->p.layer_form(layer).readable) { set_error("layer %d has no materialised output (fused) or weights not loaded", layer); return RTOD_E_STATE; }
    return launch_view_to_nchw(v, batch, out_dev_nchw, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_plan_bn_batch_stats(rtod_plan* plan, int layer, double* mean_host, double* var_host, int channels, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan || !mean_host || !var_host || layer < 0 || layer >= (int)plan->p.layers.size()) { set_error("bn_batch_stats: bad args"); return RTOD_E_ARG; }
    if (!plan->p.opt_bn_batch_stats || !plan->p.d_bn_stats) { set_error("bn_batch_stats: the plan does not run batch-statistics BatchNorm (option bn_batch_stats, weights loaded)"); return RTOD_E_STATE; }
    for (const auto& pc : plan->p.convs) {
        if (pc.layer != layer) continue;
        if (pc.stats_off < 0 || channels != plan->p.layers[layer].cout) { set_error("bn_batch_stats: layer %d has no BatchNorm / %d channels", layer, plan->p.layers[layer].cout); return RTOD_E_ARG; }
        RTOD_HIP(hipSetDevice(plan->p.device));
        RTOD_HIP(hipStreamSynchronize((hipStream_t)stream));
        RTOD_HIP(hipMemcpy(mean_host, plan->p.d_bn_stats + pc.stats_off, sizeof(double) * channels, hipMemcpyDeviceToHost));
        RTOD_HIP(hipMemcpy(var_host, plan->p.d_bn_stats + pc.stats_off + pc.Npad, sizeof(double) * channels, hipMemcpyDeviceToHost));
        return RTOD_OK;
    }
    set_error("bn_batch_stats: layer %d is not a convolution", layer);
    return RTOD_E_ARG;
    RTOD_GUARD_END
}

int rtod_plan_bn_update_running(rtod_plan* plan, int batch, float* const* running_mean_dev, float* const* running_var_dev, int n_bn,
                                double momentum, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan || !running_mean_dev || !running_var_dev || batch < 1 || batch > plan->p.max_batch) { set_error("bn_update_running: bad args"); return RTOD_E_ARG; }
    if (!plan->p.opt_bn_batch_stats || !plan->p.d_bn_stats) { set_error("bn_update_running: the plan does not run batch-statistics BatchNorm (option bn_batch_stats, weights loaded)"); return RTOD_E_STATE; }
    std::vector<BnUpdateEntry> ent;
    for (const auto& pc : plan->p.convs) {                       // cfg order
        if (pc.stats_off < 0) continue;
        const int k = (int)ent.size();
        if (k >= n_bn) { set_error("bn_update_running: %d pointers for more BatchNorm layers", n_bn); return RTOD_E_ARG; }
        if (!running_mean_dev[k] || !running_var_dev[k]) { set_error("bn_update_running: null buffer %d", k); return RTOD_E_ARG; }
        const auto& L = plan->p.layers[pc.layer];
        const int64_t n = (int64_t)batch * L.hout * L.wout;
        ent.push_back(BnUpdateEntry{running_mean_dev[k], running_var_dev[k], pc.stats_off, (double)n / (double)(n > 1 ? n - 1 : 1), pc.Npad, L.cout});
    }
    if ((int)ent.size() != n_bn) { set_error("bn_update_running: the plan has %d BatchNorm layers, %d pointers given", (int)ent.size(), n_bn); return RTOD_E_ARG; }
    if (ent.empty()) return RTOD_OK;
    RTOD_HIP(hipSetDevice(plan->p.device));
    return launch_bn_update_running(ent.data(), (int)ent.size(), plan->p.d_bn_stats, momentum, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_predict_transform(const float* raw_dev, int batch, int attrs, int grid, int n_anchors, const float* anchors_wh,
                           int inp_dim, int train, float* out_dev, void* stream) {
    RTOD_GUARD_BEGIN
    if (!raw_dev || !out_dev || !anchors_wh) { set_error("predict_transform: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || attrs < 5 || grid < 1 || n_anchors < 1 || n_anchors > 4 || inp_dim < grid) { set_error("predict_transform: bad shape"); return RTOD_E_ARG; }
    const int stride = inp_dim / grid;                 // util.py:194
    if (inp_dim / stride != grid) { set_error("predict_transform: grid %d inconsistent with inp_dim %d (util.py:195 would mis-shape)", grid, inp_dim); return RTOD_E_ARG; }
    DecodeArgs d; d.enabled = 1; d.GH = grid; d.GW = grid; d.attrs = attrs; d.n_anchors = n_anchors; d.train = train ? 1 : 0; d.stride = (float)stride;
    for (int a = 0; a < n_anchors; ++a) {
        d.aw[a] = (float)((double)anchors_wh[2 * a] / (double)stride);
        d.ah[a] = (float)((double)anchors_wh[2 * a + 1] / (double)stride);
    }
    d.img_stride = (int64_t)grid * grid * n_anchors * attrs; d.head_off = 0;
    // NCHW raw tensor: (b, ch, y, x) strides
    return launch_decode(raw_dev, (int64_t)n_anchors * attrs * grid * grid, (int64_t)grid * grid, grid, 1, batch, d, out_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_confidence_mask(const float* pred_dev, int64_t rows, int attrs, float confidence, float* out_dev, void* stream) {
    return launch_confidence_mask(pred_dev, rows, attrs, confidence, out_dev, (hipStream_t)stream);
}

int rtod_bbox_iou(const float* box1_dev, const float* boxes_dev, int k, int row_stride, float* iou_dev, void* stream) {
    return launch_bbox_iou(box1_dev, boxes_dev, k, row_stride, iou_dev, (hipStream_t)stream);
}

int rtod_prep_image(const uint8_t* img_dev, int height, int width, int bgr, int inp_dim, float* out_dev, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_prep_image(img_dev, height, width, bgr, inp_dim, out_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_prep_frames(const uint8_t* frames_dev, int batch, int height, int width, int bgr, int out_h, int out_w, float* out_dev, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_prep_frames(frames_dev, batch, height, width, bgr, out_h, out_w, out_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_score_detections_limits(int* max_pred_per_image, int* max_targets_per_image) {
    if (!max_pred_per_image || !max_targets_per_image) { set_error("score_detections_limits: null pointer"); return RTOD_E_ARG; }
    score_limits(max_pred_per_image, max_targets_per_image);
    return RTOD_OK;
}

int rtod_score_detections_workspace(int batch, int cap, int max_targets_per_image, size_t* bytes) {
    int max_pred = 0, max_tgt = 0;
    score_limits(&max_pred, &max_tgt);
    if (!bytes || batch < 1 || cap < 0 || max_targets_per_image < 1 || max_targets_per_image > max_tgt) {
        set_error("score_detections_workspace: bad args (batch=%d cap=%d max_targets_per_image=%d, limit %d)", batch, cap, max_targets_per_image, max_tgt);
        return RTOD_E_ARG;
    }
    *bytes = score_workspace_bytes(batch, cap, max_targets_per_image);
    return RTOD_OK;
}

int rtod_score_detections(const float* det_dev, const int32_t* counts_dev, int cap, int batch, const float* tgt_dev, const int32_t* tgt_offsets_dev,
                          int num_class, const uint32_t* class_mask_host, float min_box_size, double iou_threshold, int max_targets_per_image, int target_corners,
                          int32_t* scores_dev, int32_t* totals_dev, int32_t* match_dev, float* match_iou_dev, int32_t* status_dev,
                          void* workspace_dev, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_score_detections(det_dev, counts_dev, cap, batch, tgt_dev, tgt_offsets_dev, num_class, class_mask_host, min_box_size,
                                   iou_threshold, max_targets_per_image, target_corners, scores_dev, totals_dev, match_dev, match_iou_dev, status_dev,
                                   workspace_dev, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_yolo_loss_workspace(int batch, int n_rows, size_t* bytes) {
    if (!bytes || batch < 1 || n_rows < 1 || (int64_t)batch * n_rows > INT32_MAX) { set_error("yolo_loss_workspace: bad args (batch=%d n_rows=%d)", batch, n_rows); return RTOD_E_ARG; }
    *bytes = yolo_loss_workspace_bytes(batch, n_rows);
    return RTOD_OK;
}

int rtod_yolo_loss(const float* pred_dev, int batch, int n_rows, int num_class, const rtod_yolo_head* heads, int n_heads,
                   const float* boxes_dev, const int32_t* box_offsets_dev, float min_box_size, double* loss_dev, double* per_image_dev,
                   float* target_dev, uint8_t* mask_dev, int32_t* n_obj_dev, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_yolo_loss(pred_dev, batch, n_rows, num_class, heads, n_heads, boxes_dev, box_offsets_dev, min_box_size, loss_dev, per_image_dev,
                            target_dev, mask_dev, n_obj_dev, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_darknet_loss_dense(const float* pred_dev, const float* target_dev, const uint8_t* mask_dev, int64_t rows, int attrs, double* loss_dev,
                            void* workspace, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_darknet_loss_dense(pred_dev, target_dev, mask_dev, rows, attrs, loss_dev, workspace, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_yolo_loss_grad(const float* pred_dev, int batch, int n_rows, int num_class, const rtod_yolo_head* heads, int n_heads,
                        const float* boxes_dev, const int32_t* box_offsets_dev, float min_box_size, float* grad_raw_dev, float* grad_pred_dev,
                        double* loss_dev, int32_t* n_obj_dev, int32_t* status_dev, void* workspace, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_yolo_loss_grad(pred_dev, batch, n_rows, num_class, heads, n_heads, boxes_dev, box_offsets_dev, min_box_size, grad_raw_dev,
                                 grad_pred_dev, loss_dev, n_obj_dev, status_dev, workspace, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

// The body of every rtod_*wgrad*_workspace entry: the launch's own shape check, schedule and byte count
static int wgrad_workspace(const char* who, WgradRule rule, int batch, int cout, int cin, int h, int w, int size, int stride, size_t* bytes) {
    if (!bytes) { set_error("%s: null pointer", who); return RTOD_E_ARG; }
    if (int rc = wgrad_check_shape(who, rule, batch, cout, cin, h, w, size, stride)) return rc;
    *bytes = wgrad_workspace_bytes(wgrad_schedule(rule, batch, cout, cin, h, w, size, stride), cout, cin, size);
    return RTOD_OK;
}

int rtod_conv1x1_wgrad_workspace(int batch, int cout, int cin, int pixels, size_t* bytes) {
    return wgrad_workspace("conv1x1_wgrad_workspace", WGRAD_HEAD, batch, cout, cin, 1, pixels, 1, 1, bytes);
}

int rtod_conv1x1_wgrad(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int pixels, float* dw_dev, float* db_dev,
                       void* workspace, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_wgrad("conv1x1_wgrad", WGRAD_HEAD, dz_dev, x_dev, batch, cout, cin, 1, pixels, 1, 1, nullptr, dw_dev, db_dev, workspace, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_plan_head_layers(const rtod_plan* plan, int* conv_layers, int* input_layers, int capacity) {
    if (!plan || capacity < 0 || (capacity > 0 && (!conv_layers || !input_layers))) { set_error("plan_head_layers: bad args"); return RTOD_E_ARG; }
    int n = 0;
    for (const auto& L : plan->p.layers) {
        if (!plan->p.feeds_yolo(L.index)) continue;
        if (n < capacity) { conv_layers[n] = L.index; input_layers[n] = L.index - 1; }
        ++n;
    }
    return n;
}

int rtod_conv_wgrad_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes) {
    return wgrad_workspace("conv_wgrad_workspace", WGRAD_TILED, batch, cout, cin, height, width, size, 1, bytes);
}

int rtod_conv_wgrad(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                    const double* row_scale_dev, float* dw_dev, float* db_dev, void* workspace, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_wgrad("conv_wgrad", WGRAD_TILED, dz_dev, x_dev, batch, cout, cin, height, width, size, 1, row_scale_dev, dw_dev, db_dev, workspace, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_conv1x1_dgrad(const float* w_dev, const float* dz_dev, const float* y_dev, float slope, int batch, int cout, int cin, int pixels,
                       float* dx_dev, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_conv_dgrad("conv1x1_dgrad", w_dev, nullptr, dz_dev, y_dev, slope, batch, cout, cin, 1, pixels, 1, 1, dx_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_conv_dgrad(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                    int batch, int cout, int cin, int height, int width, int size, float* dx_dev, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_conv_dgrad("conv_dgrad", w_oihw_dev, row_scale_dev, dz_dev, y_dev, slope, batch, cout, cin, height, width, size, 1, dx_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_conv_dgrad_s2(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                       int batch, int cout, int cin, int height, int width, int size, float* dx_dev, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_conv_dgrad("conv_dgrad_s2", w_oihw_dev, row_scale_dev, dz_dev, y_dev, slope, batch, cout, cin, height, width, size, 2, dx_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_conv_wgrad_s2_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes) {
    return wgrad_workspace("conv_wgrad_s2_workspace", WGRAD_TILED, batch, cout, cin, height, width, size, 2, bytes);
}

int rtod_conv_wgrad_s2(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                       const double* row_scale_dev, float* dw_dev, float* db_dev, void* workspace, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_wgrad("conv_wgrad_s2", WGRAD_TILED, dz_dev, x_dev, batch, cout, cin, height, width, size, 2, row_scale_dev, dw_dev, db_dev, workspace, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_grad_join(const float* const* contributions_dev_ptrs, int count, const float* y_dev, float slope, long long n, float* out_dev, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_grad_join(contributions_dev_ptrs, count, y_dev, slope, (int64_t)n, out_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_upsample2x_grad(const float* dz_dev, const float* y_dev, float slope, int mode, int batch, int channels, int height, int width,
                         float* dx_dev, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_upsample2x_grad(dz_dev, y_dev, slope, mode, batch, channels, height, width, dx_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

// The BatchNorm convs of one graph of the plan and the layer each reads, ascending
static int list_scope_convs(const char* who, const rtod_plan* plan, Scope scope, int* conv_layers, int* input_layers, int capacity) {
    if (!plan || capacity < 0 || (capacity > 0 && (!conv_layers || !input_layers))) { set_error("%s: bad args", who); return RTOD_E_ARG; }
    const std::vector<char> graph = plan->p.scope_graph(scope);
    int n = 0;
    for (const auto& L : plan->p.layers) {
        if (L.type != LT_CONV || !L.bn || !graph[L.index]) continue;
        if (n < capacity) { conv_layers[n] = L.index; input_layers[n] = L.index - 1; }
        ++n;
    }
    return n;
}

int rtod_plan_neck_layers(const rtod_plan* plan, int* conv_layers, int* input_layers, int capacity) {
    return list_scope_convs("plan_neck_layers", plan, SCOPE_NECK, conv_layers, input_layers, capacity);
}

int rtod_plan_trainable_layers(const rtod_plan* plan, int* conv_layers, int* input_layers, int capacity) {
    return list_scope_convs("plan_trainable_layers", plan, SCOPE_BACKBONE, conv_layers, input_layers, capacity);
}

int rtod_plan_full_layers(const rtod_plan* plan, int* conv_layers, int* input_layers, int capacity) {
    return list_scope_convs("plan_full_layers", plan, SCOPE_FULL, conv_layers, input_layers, capacity);
}

int rtod_maxpool_grad(const float* dz_dev, const float* x_dev, float slope, int batch, int channels, int height, int width, int size,
                      int stride, float* dx_dev, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_maxpool_grad(dz_dev, x_dev, slope, batch, channels, height, width, size, stride, dx_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_conv_wgrad_thin_slices(int batch, int cout, int cin, int height, int width, int size, int* slices, int* slice_len) {
    if (!slices || !slice_len) { set_error("conv_wgrad_thin_slices: null pointer"); return RTOD_E_ARG; }
    if (int rc = wgrad_check_shape("conv_wgrad_thin_slices", WGRAD_THIN, batch, cout, cin, height, width, size, 1)) return rc;
    const WgradSchedule sc = wgrad_schedule(WGRAD_THIN, batch, cout, cin, height, width, size, 1);
    *slices = sc.slices; *slice_len = sc.slice_len;
    return RTOD_OK;
}

int rtod_conv_wgrad_thin_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes) {
    return wgrad_workspace("conv_wgrad_thin_workspace", WGRAD_THIN, batch, cout, cin, height, width, size, 1, bytes);
}

int rtod_conv_wgrad_thin(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                         const double* row_scale_dev, float* dw_dev, void* workspace, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_wgrad("conv_wgrad_thin", WGRAD_THIN, dz_dev, x_dev, batch, cout, cin, height, width, size, 1, row_scale_dev, dw_dev, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_conv_dgrad_thin(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                         int batch, int cout, int cin, int height, int width, int size, float* dx_dev, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_conv_dgrad("conv_dgrad_thin", w_oihw_dev, row_scale_dev, dz_dev, y_dev, slope, batch, cout, cin, height, width, size, 1, dx_dev, (hipStream_t)stream, true);
    RTOD_GUARD_END
}

int rtod_conv_dgrad_split_tiles(int batch, int cout, int cin, int height, int width, int size, int* ids, int capacity) {
    RTOD_GUARD_BEGIN
    return conv_dgrad_split_tiles(batch, cout, cin, height, width, size, ids, capacity);
    RTOD_GUARD_END
}

int rtod_conv_dgrad_split_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes) {
    RTOD_GUARD_BEGIN
    return conv_dgrad_split_workspace(batch, cout, cin, height, width, size, bytes);
    RTOD_GUARD_END
}

int rtod_conv_dgrad_split(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                          int batch, int cout, int cin, int height, int width, int size, int tile,
                          float* dx_dev, void* workspace, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_conv_dgrad_split(w_oihw_dev, row_scale_dev, dz_dev, y_dev, slope, batch, cout, cin, height, width, size, tile, dx_dev, workspace,
                                   workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_conv_dgrad_split_phases(const float* w_oihw_dev, const double* row_scale_dev, const float* dz_dev, const float* y_dev, float slope,
                                 int batch, int cout, int cin, int height, int width, int size, int tile,
                                 float* dx_dev, void* workspace, size_t workspace_bytes, void* stream, int phases) {
    RTOD_GUARD_BEGIN
    return launch_conv_dgrad_split(w_oihw_dev, row_scale_dev, dz_dev, y_dev, slope, batch, cout, cin, height, width, size, tile, dx_dev, workspace,
                                   workspace_bytes, (hipStream_t)stream, phases);
    RTOD_GUARD_END
}

int rtod_conv_wgrad_split_schedule(int batch, int cout, int cin, int height, int width, int size, int* tiles, int* slices, int* slice_len, int64_t* k_padded) {
    RTOD_GUARD_BEGIN
    return conv_wgrad_split_schedule(batch, cout, cin, height, width, size, tiles, slices, slice_len, k_padded);
    RTOD_GUARD_END
}

int rtod_conv_wgrad_split_bounds(int batch, int cout, int cin, int height, int width, int size, int64_t* lowest, int64_t* highest, int64_t* plane_halves) {
    RTOD_GUARD_BEGIN
    return conv_wgrad_split_bounds(batch, cout, cin, height, width, size, lowest, highest, plane_halves);
    RTOD_GUARD_END
}

int rtod_conv_wgrad_split_workspace(int batch, int cout, int cin, int height, int width, int size, size_t* bytes) {
    RTOD_GUARD_BEGIN
    return conv_wgrad_split_workspace(batch, cout, cin, height, width, size, bytes);
    RTOD_GUARD_END
}

int rtod_conv_wgrad_split(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                          const double* row_scale_dev, float* dw_dev, void* workspace, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_conv_wgrad_split(dz_dev, x_dev, batch, cout, cin, height, width, size, row_scale_dev, dw_dev, workspace, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_conv_wgrad_split_phases(const float* dz_dev, const float* x_dev, int batch, int cout, int cin, int height, int width, int size,
                                 const double* row_scale_dev, float* dw_dev, void* workspace, size_t workspace_bytes, void* stream, int phases) {
    RTOD_GUARD_BEGIN
    return launch_conv_wgrad_split(dz_dev, x_dev, batch, cout, cin, height, width, size, row_scale_dev, dw_dev, workspace, workspace_bytes, (hipStream_t)stream, phases);
    RTOD_GUARD_END
}

int rtod_bn_grad_parts(int batch, int channels, int pixels, int* parts, int* part_len) { return bn_grad_parts(batch, channels, pixels, parts, part_len); }

int rtod_bn_grad_workspace(int batch, int channels, int pixels, size_t* bytes) { return bn_grad_workspace(batch, channels, pixels, bytes); }

int rtod_bn_grad(const float* du_dev, const float* z_dev, const double* mean_dev, const double* var_dev, const float* gamma_dev,
                 int batch, int channels, int pixels, float* dz_dev, float* dgamma_dev, float* dbeta_dev,
                 void* workspace_dev, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_bn_grad(du_dev, z_dev, mean_dev, var_dev, gamma_dev, batch, channels, pixels, dz_dev, dgamma_dev, dbeta_dev, workspace_dev, workspace_bytes,
                          (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_plan_head_blocks(const rtod_plan* plan, int* head_conv_layers, int* block_conv_layers, int* block_input_layers, int capacity) {
    if (!plan || capacity < 0 || (capacity > 0 && (!head_conv_layers || !block_conv_layers || !block_input_layers))) { set_error("plan_head_blocks: bad args"); return RTOD_E_ARG; }
    int n = 0;
    for (const auto& L : plan->p.layers) {
        if (!plan->p.feeds_yolo(L.index)) continue;
        if (n < capacity) {
            const int blk = plan->p.block_of_head(L.index);
            head_conv_layers[n] = L.index; block_conv_layers[n] = blk; block_input_layers[n] = blk < 0 ? -1 : blk - 1;
        }
        ++n;
    }
    return n;
}

int rtod_plan_conv_scale(const rtod_plan* plan, int layer, const double** scale_dev, double* scale_host, int channels) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("conv_scale: null plan"); return RTOD_E_ARG; }
    return plan->p.conv_scale(layer, scale_dev, scale_host, channels);
    RTOD_GUARD_END
}

int rtod_plan_update_conv_weight(rtod_plan* plan, int layer, const float* weight_oihw_host) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("update_conv_weight: null plan"); return RTOD_E_ARG; }
    return plan->p.update_conv_weight(layer, weight_oihw_host);
    RTOD_GUARD_END
}

int rtod_plan_step_conv_folded(rtod_plan* plan, int layer, const rtod_opt_step* opt, float* weight_dev, const float* dw_dev,
                               float* m_w_dev, float* v_w_dev, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("step_conv_folded: null plan"); return RTOD_E_ARG; }
    return plan->p.step_conv_folded(layer, opt, weight_dev, dw_dev, m_w_dev, v_w_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_plan_read_bn_input(rtod_plan* plan, int layer, int batch, float* out_dev_nchw, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("read_bn_input: null plan"); return RTOD_E_ARG; }
    return plan->p.read_bn_input(layer, batch, out_dev_nchw, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_plan_bn_stats_dev(const rtod_plan* plan, int layer, const double** mean_dev, const double** var_dev) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("bn_stats_dev: null plan"); return RTOD_E_ARG; }
    return plan->p.bn_stats_dev(layer, mean_dev, var_dev);
    RTOD_GUARD_END
}

int rtod_plan_step_conv_bn(rtod_plan* plan, int layer, const rtod_opt_step* opt, float* weight_dev, const float* dw_dev, float* gamma_dev, float* beta_dev,
                           const float* dgamma_dev, const float* dbeta_dev, float* m_w_dev, float* v_w_dev, float* m_gamma_dev, float* v_gamma_dev,
                           float* m_beta_dev, float* v_beta_dev, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("step_conv_bn: null plan"); return RTOD_E_ARG; }
    return plan->p.step_conv_bn(layer, opt, weight_dev, dw_dev, gamma_dev, beta_dev, dgamma_dev, dbeta_dev, m_w_dev, v_w_dev, m_gamma_dev, v_gamma_dev,
                                m_beta_dev, v_beta_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_plan_update_conv_bn(rtod_plan* plan, int layer, const float* weight_oihw_host, const float* gamma_host, const float* beta_host) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("update_conv_bn: null plan"); return RTOD_E_ARG; }
    return plan->p.update_conv_bn(layer, weight_oihw_host, gamma_host, beta_host);
    RTOD_GUARD_END
}

int rtod_plan_update_conv(rtod_plan* plan, int layer, const float* weight_oihw_host, const float* bias_host) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("update_conv: null plan"); return RTOD_E_ARG; }
    return plan->p.update_conv(layer, weight_oihw_host, bias_host);
    RTOD_GUARD_END
}

int rtod_plan_step_conv(rtod_plan* plan, int layer, const rtod_opt_step* opt, float* weight_dev, float* bias_dev, const float* dw_dev, const float* db_dev,
                        float* m_w_dev, float* v_w_dev, float* m_b_dev, float* v_b_dev, void* stream) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("step_conv: null plan"); return RTOD_E_ARG; }
    return plan->p.step_conv(layer, opt, weight_dev, bias_dev, dw_dev, db_dev, m_w_dev, v_w_dev, m_b_dev, v_b_dev, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_plan_read_packed_weights(rtod_plan* plan, float* out_host, size_t capacity_floats, size_t* needed) {
    RTOD_GUARD_BEGIN
    if (!plan) { set_error("read_packed_weights: null plan"); return RTOD_E_ARG; }
    return plan->p.read_packed_weights(out_host, capacity_floats, needed);
    RTOD_GUARD_END
}

int rtod_write_results_workspace(int batch, int n, size_t* bytes) {
    if (!bytes || batch < 1 || n < 1) { set_error("write_results_workspace: bad args"); return RTOD_E_ARG; }
    *bytes = nms_workspace_bytes(batch, n);
    return RTOD_OK;
}

int rtod_write_results(const float* pred_dev, int batch, int n, int num_class, float confidence, float nms_conf,
                       float* out_dev, int cap, int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_write_results(pred_dev, batch, n, num_class, confidence, nms_conf, out_dev, cap, counts_dev,
                                workspace_dev, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

int rtod_nms_class_offset(const float* pred_dev, int batch, int n, int num_class, float confidence, float iou_thr, float max_wh, int max_det,
                          float* out_dev, int cap, int32_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    RTOD_GUARD_BEGIN
    return launch_nms_class_offset(pred_dev, batch, n, num_class, confidence, iou_thr, max_wh, max_det, out_dev, cap, counts_dev,
                                   workspace_dev, workspace_bytes, (hipStream_t)stream);
    RTOD_GUARD_END
}

}  // extern "C"
