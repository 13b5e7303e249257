// Packed weights: the .weights payload -> the image the kernels read (host), and its upload.  Weight stream order in the
// reference: src/darknet.py:316-410.
#include "plan.h"
#include "f16_round.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace rtod {

// The frozen (eval) BatchNorm scale of one channel.  pack_conv folds it into the weights and the bias, load_weights keeps it for
// the gradient and the step of the detection blocks: head_step_kernel re-packs bit for bit only while both read this one line.
static double bn_frozen_scale(float gamma, float var) { return (double)gamma / std::sqrt((double)var + 1e-5); }

// Split layouts, per output channel: a power-of-two pre-scale 2^e puts max|w| in [2^12, 2^13), so that low parts of weights down to
// 2^-16 of the channel maximum stay normal f16; e is held to -24 .. 40 and an all-zero channel keeps e = 0.  ps = 2^e multiplies
// the folded weights, inv = 2^-e / ACT_SCALE_F16S3 is what the kernels' epilogues multiply the sums by.
struct PreScale { double ps = 1.0; float inv = 0.f; };
static PreScale channel_prescale(const float* w, int64_t n, double scale) {
    double mx = 0.0;
    for (int64_t q = 0; q < n; ++q) mx = std::max(mx, std::fabs((double)w[q] * scale));
    int e = 0;
    if (mx > 0.0) { int ex; std::frexp(mx, &ex); e = 13 - ex; }      // mx * 2^e in [2^12, 2^13)
    e = std::max(-24, std::min(40, e));
    PreScale s;
    s.ps = std::ldexp(1.0, e);
    s.inv = (float)(std::ldexp(1.0, -e) / (double)ACT_SCALE_F16S3);
    return s;
}
static void split_hi_lo(float v, uint16_t& hi, uint16_t& lo) {
    hi = f32_to_f16_rn(v);
    lo = f32_to_f16_rn(v - f16_to_f32(hi));
}

// One conv's block of the .weights payload (p: [bn.bias, bn.weight, running_mean, running_var] or [conv.bias], then conv.weight
// OIHW) -> its block of the packed image (blk = image + pc.w_off, conv_block_floats floats, zero on entry: padding rows, padding
// channels and the unused halves of narrow chunks stay zero).  The one place that folds, pre-scales and places a conv's weights:
// pack_weights walks every conv through it, update_conv one.
void Plan::pack_conv(const PackedConv& pc, const float* p, float* blk) const {
    const Layer& L = layers[pc.layer];
    const int C = L.cout, cin = L.cin, k = L.size;
    std::vector<double> scale(C, 1.0);
    float* bias = blk + (pc.b_off - pc.w_off);
    if (L.bn && opt_bn_batch_stats) {
        // batch-statistics mode: the conv stays unfolded (no bias), beta / gamma go to the normalisation kernel; the
        // stream's running mean / variance are not used (the reference only updates them as a side effect)
        float* bnp = blk + (pc.bn_off - pc.w_off);
        for (int o = 0; o < C; ++o) { bias[o] = 0.f; bnp[o] = p[o]; bnp[pc.Npad + o] = p[C + o]; }
        p += 4 * C;
    } else if (L.bn) {
        const float *beta = p, *gamma = p + C, *mean = p + 2 * C, *var = p + 3 * C;
        for (int o = 0; o < C; ++o) {
            // eval BatchNorm (x - mean) / sqrt(var + 1e-5) * gamma + beta folded into the conv
            const double s = scale[o] = bn_frozen_scale(gamma[o], var[o]);
            bias[o] = (float)((double)beta[o] - (double)mean[o] * s);
        }
        p += 4 * C;
    } else {
        for (int o = 0; o < C; ++o) bias[o] = p[o];
        p += C;
    }
    // One walk over the OIHW block.  Every weight is folded to fp32 first ((double) w * scale, rounded once); the four layouts
    // differ in where it lands alone (element index: floats of the fp32 layouts, halves of the split planes):
    //   fp32 stem    [28][Cout], k = (ky*3+kx)*3 + c (conv_stem.hip)
    //   fp32 panel   [Cout][Kpad], k = tap * cin_p + c
    //   split stem   [Cout][32] f16 hi / lo planes, k = (ky*3+kx)*3 + c, k >= 27 zero
    //   split planes K-chunk major, [chunk][Npad][32]: the rows of one stage are contiguous.  K order of the split kernels:
    //                k = ((c/32)*k*k + tap)*32 + c%32 (channel chunk outer, tap inner);
    //                narrow layers (conv_c16_f16s3.hip): tap-major over the 16 channels, k = tap * 16 + c, so chunk j holds
    //                taps 2j and 2j + 1 (the unused half of the last chunk of an odd tap count stays zero in both planes)
    const int taps = k * k;
    auto dst = [&](int o, int c, int tap) -> int64_t {
        if (pc.stem) return pc.split ? o * 32 + tap * 3 + c : (int64_t)(tap * 3 + c) * C + o;
        if (!pc.split) return (int64_t)o * pc.Kpad + tap * pc.cin_p + c;
        return pc.narrow ? ((int64_t)(tap / 2) * pc.Npad + o) * 32 + (tap % 2) * 16 + c
                         : ((int64_t)((c / 32) * taps + tap) * pc.Npad + o) * 32 + (c % 32);
    };
    float* wp = blk;
    uint16_t* wh = reinterpret_cast<uint16_t*>(blk);
    uint16_t* wl = reinterpret_cast<uint16_t*>(blk + (pc.wl_off - pc.w_off));
    float* inv = blk + (pc.s_off - pc.w_off);
    if (pc.split && !pc.stem) for (int o = 0; o < pc.Npad; ++o) inv[o] = 1.0f / ACT_SCALE_F16S3;      // padding channels
    const int64_t per_o = (int64_t)cin * taps;
    for (int o = 0; o < C; ++o) {
        const float* po = p + o * per_o;
        PreScale s;
        if (pc.split) { s = channel_prescale(po, per_o, scale[o]); inv[o] = s.inv; }
        for (int c = 0; c < cin; ++c)
            for (int tap = 0; tap < taps; ++tap) {
                const float v = (float)((double)po[(int64_t)c * taps + tap] * scale[o]);      // the fp32 folded weight
                const int64_t idx = dst(o, c, tap);
                if (!pc.split) { wp[idx] = v; continue; }
                const float vs = (float)((double)v * s.ps);                                   // exact (power of two)
                split_hi_lo(vs, wh[idx], wl[idx]);
            }
    }
}

// layout_weights gives every conv one contiguous run of the image that starts at its w_off
int64_t Plan::conv_block_floats(size_t slot) const {
    return (slot + 1 < convs.size() ? convs[slot + 1].w_off : packed_floats) - convs[slot].w_off;
}

// The image rtod_plan_load_weights uploads, for the plan's current options and precision.  Host only: no HIP call, no device state.
int Plan::pack_weights(const float* w, size_t n, std::vector<float>& packed) const {
    if (!w) { set_error("load_weights: null pointer"); return RTOD_E_ARG; }
    if ((int64_t)n < n_weight_floats) {
        set_error("load_weights: stream has %zu floats, network needs %lld", n, (long long)n_weight_floats);
        return RTOD_E_SIZE;
    }
    packed.assign((size_t)packed_floats, 0.0f);
    for (const auto& pc : convs) pack_conv(pc, w + layers[pc.layer].w_off, packed.data() + pc.w_off);
    return RTOD_OK;
}

// The slot in `convs` of a conv whose weights may be replaced alone (update_conv, step_conv): no BatchNorm, no fused pointwise pair.
int Plan::replaceable_conv(const char* who, int layer, size_t& slot) const {
    ConvSite cs;
    if (int rc = conv_site(who, layer, cs)) return rc;
    if (layers[layer].bn) { set_error("%s: layer %d has BatchNorm (only convs without it can be replaced)", who, layer); return RTOD_E_ARG; }
    if (cs.pair) { set_error("%s: layer %d is part of a fused pointwise pair", who, layer); return RTOD_E_ARG; }
    if (cs.slot < 0) { set_error("%s: layer %d has no packed weights", who, layer); return RTOD_E_ARG; }
    slot = (size_t)cs.slot;
    return RTOD_OK;
}

// What replaceable_conv and block_conv both ask first: `layer` is a convolution (else refused), the slot of its packed weights (-1:
// none) and whether it is host or guest of a fused-pointwise pair (candidates, not forms: a pair that may fuse counts whether or
// not it runs fused now)
int Plan::conv_site(const char* who, int layer, ConvSite& cs) const {
    if (layer < 0 || layer >= (int)layers.size() || layers[layer].type != LT_CONV) { set_error("%s: layer %d is not a convolution", who, layer); return RTOD_E_ARG; }
    for (const auto& l : launches) {
        if ((l.kind != LK_CONV && l.kind != LK_STEM) || l.layer != layer || l.conv_slot < 0) continue;
        cs.slot = l.conv_slot;
        cs.pair = cs.pair || l.pw_guest >= 0 || l.pw_host >= 0;
    }
    return RTOD_OK;
}

// One conv re-packed from its block of the stream (`stream`: [bias] or [beta, gamma, mean, var], then the OIHW weights) and that
// block alone copied to the device: the bits a full load_weights of the edited stream gives, since both go through pack_conv.
// Synchronises the device (a forward in flight may still read the old block).
int Plan::repack_conv(size_t slot, const std::vector<float>& stream) {
    const PackedConv& pc = convs[slot];
    std::vector<float> blk((size_t)conv_block_floats(slot), 0.0f);
    pack_conv(pc, stream.data(), blk.data());
    RTOD_HIP(hipSetDevice(device));
    RTOD_HIP(hipDeviceSynchronize());
    RTOD_HIP(hipMemcpy(d_weights + pc.w_off, blk.data(), sizeof(float) * blk.size(), hipMemcpyHostToDevice));
    RTOD_HIP(hipDeviceSynchronize());
    return RTOD_OK;
}

// A conv without BatchNorm from (weight OIHW, bias)
int Plan::update_conv(int layer, const float* weight_oihw, const float* bias) {
    if (!weight_oihw || !bias) { set_error("update_conv: null pointer"); return RTOD_E_ARG; }
    size_t slot = 0;
    if (int rc = replaceable_conv("update_conv", layer, slot)) return rc;
    if (!weights_loaded || !d_weights) { set_error("update_conv: call rtod_plan_load_weights first"); return RTOD_E_STATE; }
    const Layer& L = layers[layer];
    std::vector<float> stream(bias, bias + L.cout);
    stream.insert(stream.end(), weight_oihw, weight_oihw + (int64_t)L.cout * L.cin * L.size * L.size);
    return repack_conv(slot, stream);
}

// A float field of rtod_opt_step read as the shortest decimal that rounds to it (0.999f means 0.999, as it prints): 1 - beta2 taken
// from the float's own value would be off by 2^-25 / 0.001, hundreds of fp32 ulps of every v'.
static double shortest_decimal(float f) {
    if (!std::isfinite(f)) return (double)f;
    char buf[40];
    for (int prec = 1; prec <= 9; ++prec) {
        snprintf(buf, sizeof buf, "%.*g", prec, (double)f);
        const double d = strtod(buf, nullptr);
        if ((float)d == f) return d;
    }
    return (double)f;
}

// The device twin of update_conv for a 1x1 conv: one kernel (head_step.hip) applies the optimiser step to the caller's float32
// masters and writes the conv's ranges of the image where pack_conv would, bit for bit.  Enqueues only: every refusal is decided
// before anything touches the device, and the scalars of the step are derived here in double and passed as floats.
int Plan::step_conv(int layer, const rtod_opt_step* opt, float* weight, float* bias, const float* dw, const float* db,
                    float* m_w, float* v_w, float* m_b, float* v_b, hipStream_t s) {
    if (!opt || !weight || !bias || !dw || !db) { set_error("step_conv: null pointer"); return RTOD_E_ARG; }
    size_t slot = 0;
    if (int rc = replaceable_conv("step_conv", layer, slot)) return rc;
    const Layer& L = layers[layer];
    const PackedConv& pc = convs[slot];
    if (L.size != 1 || pc.stem || pc.stem16 || pc.narrow) { set_error("step_conv: layer %d is not a 1x1 conv of the generic layouts (size %d%s)", layer, L.size, pc.narrow ? ", narrow" : pc.stem ? ", stem" : ""); return RTOD_E_ARG; }
    if (pc.Kpad < L.cin || L.cout > pc.Npad || (pc.split && L.cin % 32 != 0)) { set_error("step_conv: layer %d has an unexpected packed layout", layer); return RTOD_E_ARG; }
    HeadStepLaunch h;
    h.w = weight; h.b = bias; h.dw = dw; h.db = db; h.m_w = m_w; h.v_w = v_w; h.m_b = m_b; h.v_b = v_b;
    return step_packed("step_conv", slot, opt, m_w && v_w && m_b && v_b, false, h, s);
}

// The body of both steps, after the entry's own refusals: the scalars, the state the step needs (folded: the frozen scales of the
// block convs on the device), then the launch description — h holds the caller's pointers — filled once
int Plan::step_packed(const char* who, size_t slot, const rtod_opt_step* opt, bool moments, bool folded, HeadStepLaunch& h, hipStream_t s) {
    if (int rc = opt_scalars(who, opt, moments, h)) return rc;
    if (!weights_loaded || !d_weights) { set_error("%s: call rtod_plan_load_weights first", who); return RTOD_E_STATE; }
    if (folded && (kept_scope() == SCOPE_NONE || !d_block_scale)) { set_error("%s: the plan needs option keep_block_inputs, keep_neck_activations, keep_backbone_activations or keep_full_activations (they put the frozen scales on the device)", who); return RTOD_E_STATE; }
    const PackedConv& pc = convs[slot];
    const Layer& L = layers[pc.layer];
    h.cout = L.cout; h.cin = L.cin; h.taps = L.size * L.size; h.cin_p = pc.cin_p; h.split = pc.split ? 1 : 0; h.Kpad = pc.Kpad; h.Npad = pc.Npad;
    if (folded) h.scale = d_block_scale + block_scale_off.at(pc.layer);
    h.panel = d_weights + pc.w_off;
    h.hi = reinterpret_cast<uint16_t*>(d_weights + pc.w_off);
    h.lo = reinterpret_cast<uint16_t*>(d_weights + pc.wl_off);
    h.inv = d_weights + pc.s_off;
    h.bias = d_weights + pc.b_off;
    if (h.gamma) h.bn = d_weights + pc.bn_off;                       // step_conv_bn: the [Npad] beta, [Npad] gamma block of a batch-statistics image
    return launch_head_step(h, s);
}

// The scalars of one step, checked and derived in double (step_conv, step_conv_folded); `moments`: every moment buffer Adam needs is there
int Plan::opt_scalars(const char* who, const rtod_opt_step* opt, bool moments, HeadStepLaunch& h) const {
    if (opt->kind != 0 && opt->kind != 1) { set_error("%s: kind %d (0 = SGD, 1 = Adam)", who, opt->kind); return RTOD_E_ARG; }
    if (!std::isfinite(opt->lr)) { set_error("%s: lr is not finite", who); return RTOD_E_ARG; }
    h.kind = opt->kind;
    h.lr = opt->lr;
    if (opt->kind == 1) {
        if (opt->step < 1) { set_error("%s: Adam needs the 1-based step count, got %d", who, opt->step); return RTOD_E_ARG; }
        if (!(opt->beta1 >= 0.f && opt->beta1 < 1.f) || !(opt->beta2 >= 0.f && opt->beta2 < 1.f)) { set_error("%s: Adam betas must lie in [0, 1)", who); return RTOD_E_ARG; }
        if (!(opt->eps >= 0.f)) { set_error("%s: Adam eps must be >= 0", who); return RTOD_E_ARG; }
        if (!moments) { set_error("%s: Adam needs the moment buffers", who); return RTOD_E_ARG; }
        const double b1 = shortest_decimal(opt->beta1), b2 = shortest_decimal(opt->beta2);
        h.lr = (float)(shortest_decimal(opt->lr) / (1.0 - std::pow(b1, (double)opt->step)));
        h.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)opt->step));
        h.beta2 = opt->beta2;
        h.omb1 = (float)(1.0 - b1);
        h.omb2 = (float)(1.0 - b2);
        h.eps = opt->eps;
    }
    return RTOD_OK;
}

// The slot of a detection block conv (rtod_plan_head_blocks) — on a plan with option keep_neck_activations of any neck conv
// (rtod_plan_neck_layers), with keep_backbone_activations of any trainable conv (rtod_plan_trainable_layers) — or why `layer` is
// none: what conv_scale, update_conv_weight and step_conv_folded accept
int Plan::block_conv(const char* who, int layer, size_t& slot) const {
    ConvSite cs;
    if (int rc = conv_site(who, layer, cs)) return rc;
    if (!layers[layer].bn) { set_error("%s: layer %d has no BatchNorm (rtod_plan_update_conv / rtod_plan_step_conv take such convs)", who, layer); return RTOD_E_ARG; }
    if (!trains_folded(layer)) {
        // per kept scope: what the plan trains, the shape such a conv has, and what else keeps a conv of that shape out
        static const struct { const char* what; const char* shape; const char* closure; } kText[] = {
            {"detection block", "not the 1x1 / 3x3 stride-1 leaky or linear BatchNorm conv that a detection-head conv reads", nullptr},
            {"detection block", "not the 1x1 / 3x3 stride-1 leaky or linear BatchNorm conv that a detection-head conv reads", nullptr},
            {"neck conv", "not a 1x1 / 3x3 stride-1 same-padding leaky or linear BatchNorm conv that reads a multiple of 32 channels",
             "a layer outside the neck reads its output, or the plan computes it inside another layer's kernel"},
            {"trainable conv", "not a 1x1 / 3x3 stride-1 or 3x3 stride-2 same-padding leaky or linear BatchNorm conv that reads a multiple of 32 channels",
             "a layer outside the trainable graph reads its output, or the plan computes it inside another layer's kernel"},
            {"full-graph conv", "not a 1x1 / 3x3 stride-1 or 3x3 stride-2 same-padding leaky or linear BatchNorm conv",
             "a layer outside the full graph reads its output, or the plan computes it inside another layer's kernel"}};
        const Scope kept = kept_scope();
        const bool shape_ok = kept == SCOPE_FULL ? full_shape_ok(layer) : kept == SCOPE_BACKBONE ? train_shape_ok(layer) : kept == SCOPE_NECK && block_shape_ok(layer);
        const PackedConv* pc = cs.slot >= 0 ? &convs[cs.slot] : nullptr;
        const char* why = opt_bn_batch_stats ? "the plan runs batch-statistics BatchNorm: the conv is not folded; rtod_plan_step_conv_bn / rtod_plan_update_conv_bn train it with option keep_bn_inputs"
                        : pc && (pc->stem || pc->stem16) ? "a stem layout" : pc && pc->narrow ? "a narrow (Cin == 16) layout"
                        : cs.pair ? "part of a fused pointwise pair"
                        : shape_ok ? kText[kept].closure : kText[kept].shape;
        set_error("%s: layer %d is not a %s (%s)", who, layer, kText[kept].what, why);
        return RTOD_E_ARG;
    }
    slot = (size_t)cs.slot;                                          // block_of_head found it: a block has packed weights
    return RTOD_OK;
}

// The frozen BatchNorm scale of a block conv, as pack_conv folds it: on the host (copied out) and, with option keep_block_inputs, on the device
int Plan::conv_scale(int layer, const double** scale_dev, double* scale_host, int channels) const {
    size_t slot = 0;
    if (int rc = block_conv("conv_scale", layer, slot)) return rc;
    if (channels != layers[layer].cout) { set_error("conv_scale: layer %d has %d output channels, %d given", layer, layers[layer].cout, channels); return RTOD_E_ARG; }
    const auto it = block_scale.find(layer);
    if (!weights_loaded || it == block_scale.end()) { set_error("conv_scale: call rtod_plan_load_weights first"); return RTOD_E_STATE; }
    if (scale_dev) {
        if (!d_block_scale) { set_error("conv_scale: the scales live on the device with option keep_block_inputs only"); return RTOD_E_STATE; }
        *scale_dev = d_block_scale + block_scale_off.at(layer);
    }
    if (scale_host) memcpy(scale_host, it->second.data(), sizeof(double) * (size_t)channels);
    return RTOD_OK;
}

// The host twin of step_conv_folded, update_conv for a block conv: the stream of the conv is assembled from the BatchNorm parameters
// kept at load time and the new OIHW weights and goes through pack_conv, so the block holds the bits a full load of the edited
// stream gives.  Synchronises the device.
int Plan::update_conv_weight(int layer, const float* weight_oihw) {
    if (!weight_oihw) { set_error("update_conv_weight: null pointer"); return RTOD_E_ARG; }
    size_t slot = 0;
    if (int rc = block_conv("update_conv_weight", layer, slot)) return rc;
    const auto it = block_bn.find(layer);
    if (!weights_loaded || !d_weights || it == block_bn.end()) { set_error("update_conv_weight: call rtod_plan_load_weights first"); return RTOD_E_STATE; }
    const Layer& L = layers[layer];
    std::vector<float> stream(it->second);
    stream.insert(stream.end(), weight_oihw, weight_oihw + (int64_t)L.cout * L.cin * L.size * L.size);
    return repack_conv(slot, stream);
}

// The device twin: head_step.hip's kernel on the raw float32 master [Cout, Cin, k, k], folding the frozen scale while it re-packs.
// No bias: beta - mean * s does not depend on the weights.  Enqueues only; every refusal is decided before anything is enqueued.
int Plan::step_conv_folded(int layer, const rtod_opt_step* opt, float* weight, const float* dw, float* m_w, float* v_w, hipStream_t s) {
    if (!opt || !weight || !dw) { set_error("step_conv_folded: null pointer"); return RTOD_E_ARG; }
    size_t slot = 0;
    if (int rc = block_conv("step_conv_folded", layer, slot)) return rc;
    HeadStepLaunch h;
    h.w = weight; h.dw = dw; h.m_w = m_w; h.v_w = v_w;
    return step_packed("step_conv_folded", slot, opt, m_w && v_w, true, h, s);
}

// The slot of a conv whose BatchNorm runs on batch statistics and trains with it (trains_bn: a batch-statistics plan with option
// keep_bn_inputs, a block conv or a BatchNorm conv of the kept graph), or why `layer` is none: what read_bn_input, step_conv_bn and
// update_conv_bn accept
int Plan::bn_conv(const char* who, int layer, size_t& slot) const {
    ConvSite cs;
    if (int rc = conv_site(who, layer, cs)) return rc;
    const Layer& L = layers[layer];
    if (!L.bn) { set_error("%s: layer %d has no BatchNorm (rtod_plan_update_conv / rtod_plan_step_conv take such convs)", who, layer); return RTOD_E_ARG; }
    if (!opt_bn_batch_stats) { set_error("%s: the plan folds BatchNorm (an eval plan): rtod_plan_step_conv_folded / rtod_plan_update_conv_weight train layer %d; this entry needs option bn_batch_stats", who, layer); return RTOD_E_ARG; }
    if (!opt_keep_bn_inputs) { set_error("%s: the plan needs option keep_bn_inputs (it keeps the raw output of the BatchNorm convs the plan trains)", who); return RTOD_E_ARG; }
    if (!trains_bn(layer) || cs.slot < 0 || L.z_buf < 0) {
        const bool shortcut = L.fused_into >= 0 && layers[L.fused_into].type == LT_SHORTCUT;
        set_error("%s: layer %d is not a conv this plan trains (%s)", who, layer,
                  shortcut ? "a shortcut is added in its normalise step: its stored output is not act(u), so it carries no leaky mask; options keep_backbone_activations / keep_full_activations hold that fusion"
                           : L.act > 1 ? "SiLU has no backward here"
                           : "outside the kept scope graph, or no 1x1 / 3x3 leaky or linear BatchNorm conv of a generic layout");
        return RTOD_E_ARG;
    }
    slot = (size_t)cs.slot;
    return RTOD_OK;
}

// Dense NCHW copy of the raw sums z the last forward left for that conv
int Plan::read_bn_input(int layer, int batch, float* out_nchw, hipStream_t s) const {
    if (!out_nchw) { set_error("read_bn_input: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || batch > max_batch) { set_error("read_bn_input: batch %d outside 1..%d", batch, max_batch); return RTOD_E_ARG; }
    size_t slot = 0;
    if (int rc = bn_conv("read_bn_input", layer, slot)) return rc;
    const View z = bn_input_view(layer);
    if (!weights_loaded || !z.base) { set_error("read_bn_input: call rtod_plan_load_weights first"); return RTOD_E_STATE; }
    return launch_view_to_nchw(z, batch, out_nchw, s);
}

// Device addresses of the doubles the last forward normalised that layer with (any BatchNorm conv of a batch-statistics plan)
int Plan::bn_stats_dev(int layer, const double** mean_dev, const double** var_dev) const {
    if (!mean_dev || !var_dev) { set_error("bn_stats_dev: null pointer"); return RTOD_E_ARG; }
    ConvSite cs;
    if (int rc = conv_site("bn_stats_dev", layer, cs)) return rc;
    if (!opt_bn_batch_stats || cs.slot < 0 || convs[cs.slot].stats_off < 0) { set_error("bn_stats_dev: layer %d has no batch-statistics BatchNorm (option bn_batch_stats, a BatchNorm conv)", layer); return RTOD_E_ARG; }
    if (!weights_loaded || !d_bn_stats) { set_error("bn_stats_dev: call rtod_plan_load_weights first"); return RTOD_E_STATE; }
    const PackedConv& pc = convs[cs.slot];
    *mean_dev = d_bn_stats + pc.stats_off;
    *var_dev = d_bn_stats + pc.stats_off + pc.Npad;
    return RTOD_OK;
}

// step_conv_folded for a conv whose BatchNorm runs on batch statistics: the same kernel steps the raw master and re-packs it unfolded
// (scale 1; the bias slot keeps its zeros), and its extra workgroup steps gamma and beta and writes the [beta, gamma] block at bn_off.
// Enqueues only; every refusal is decided before anything is enqueued.
int Plan::step_conv_bn(int layer, const rtod_opt_step* opt, float* weight, const float* dw, float* gamma, float* beta, const float* dgamma, const float* dbeta,
                       float* m_w, float* v_w, float* m_g, float* v_g, float* m_b, float* v_b, hipStream_t s) {
    if (!opt || !weight || !dw || !gamma || !beta || !dgamma || !dbeta) { set_error("step_conv_bn: null pointer"); return RTOD_E_ARG; }
    size_t slot = 0;
    if (int rc = bn_conv("step_conv_bn", layer, slot)) return rc;
    HeadStepLaunch h;
    h.w = weight; h.dw = dw; h.m_w = m_w; h.v_w = v_w;
    h.gamma = gamma; h.beta = beta; h.dgamma = dgamma; h.dbeta = dbeta; h.m_g = m_g; h.v_g = v_g; h.m_be = m_b; h.v_be = v_b;
    return step_packed("step_conv_bn", slot, opt, m_w && v_w && m_g && v_g && m_b && v_b, false, h, s);
}

// ... and its host twin, update_conv_weight for such a conv: the conv's block of the stream from the three arrays (the running
// statistics are not part of a batch-statistics image), through pack_conv.  Synchronises the device.
int Plan::update_conv_bn(int layer, const float* weight_oihw, const float* gamma, const float* beta) {
    if (!weight_oihw || !gamma || !beta) { set_error("update_conv_bn: null pointer"); return RTOD_E_ARG; }
    size_t slot = 0;
    if (int rc = bn_conv("update_conv_bn", layer, slot)) return rc;
    if (!weights_loaded || !d_weights) { set_error("update_conv_bn: call rtod_plan_load_weights first"); return RTOD_E_STATE; }
    const Layer& L = layers[layer];
    std::vector<float> stream(beta, beta + L.cout);
    stream.insert(stream.end(), gamma, gamma + L.cout);
    stream.insert(stream.end(), 2 * (size_t)L.cout, 0.0f);            // running mean / variance: not read by pack_conv in this mode
    stream.insert(stream.end(), weight_oihw, weight_oihw + (int64_t)L.cout * L.cin * L.size * L.size);
    return repack_conv(slot, stream);
}

// The device image as it is now (tests, debugging): synchronises.
int Plan::read_packed_weights(float* out, size_t capacity, size_t* needed) const {
    if (needed) *needed = (size_t)packed_floats;
    if (!out) return RTOD_OK;
    if (capacity < (size_t)packed_floats) { set_error("read_packed_weights: capacity %zu < %lld floats", capacity, (long long)packed_floats); return RTOD_E_SIZE; }
    if (!weights_loaded || !d_weights) { set_error("read_packed_weights: call rtod_plan_load_weights first"); return RTOD_E_STATE; }
    RTOD_HIP(hipSetDevice(device));
    RTOD_HIP(hipDeviceSynchronize());
    RTOD_HIP(hipMemcpy(out, d_weights, sizeof(float) * (size_t)packed_floats, hipMemcpyDeviceToHost));
    return RTOD_OK;
}

int Plan::load_weights(const float* w, size_t n) {
    std::vector<float> packed;
    if (int rc = pack_weights(w, n, packed)) return rc;
    RTOD_HIP(hipSetDevice(device));
    if (!d_weights) RTOD_HIP(hipMalloc((void**)&d_weights, sizeof(float) * (size_t)packed_floats));
    if (!d_arena) {
        RTOD_HIP(hipMalloc((void**)&d_arena, sizeof(float) * (size_t)arena_floats));
        // plain-f16 plans: every half of the arena starts as an f16 NaN, so a kernel that wrongly reads a lo plane (never
        // written in that mode) turns the results NaN, deterministically, instead of picking up stale but plausible values
        if (precision == 2) RTOD_HIP(hipMemsetD16((hipDeviceptr_t)d_arena, 0x7E00, 2 * (size_t)arena_floats));
        else RTOD_HIP(hipMemset(d_arena, 0, sizeof(float) * (size_t)arena_floats));
    }
    if (opt_bn_batch_stats && !d_bn_stats && bn_stats_doubles > 0) {
        RTOD_HIP(hipMalloc((void**)&d_bn_stats, sizeof(double) * (size_t)bn_stats_doubles));
        RTOD_HIP(hipMemset(d_bn_stats, 0, sizeof(double) * (size_t)bn_stats_doubles));
        int maxn = 0;
        for (const auto& pc : convs) if (pc.stats_off >= 0) maxn = std::max(maxn, pc.Npad);
        bn_partial_count = (int64_t)bn_partial_doubles(maxn);
        RTOD_HIP(hipMalloc((void**)&d_bn_partial, sizeof(double) * (size_t)bn_partial_count));
    }
    if (bn_raw_floats > 0 && !d_bn_raw) RTOD_HIP(hipMalloc((void**)&d_bn_raw, sizeof(float) * (size_t)bn_raw_floats));
    if (!d_scratch) {
        bool any = false;
        for (const auto& pc : convs) any = any || (!pc.split && !pc.stem && pc.slice_chunks > 0) || (pc.split && pc.ks_chunks > 0);
        if (any) {
            scratch_floats = KS_SCRATCH_FLOATS;                                   // 32 MB: L2 / Infinity-Cache resident; larger panels run the in-workgroup schedule
            RTOD_HIP(hipMalloc((void**)&d_scratch, sizeof(float) * (size_t)scratch_floats));
        }
    }
    // detection blocks: the BatchNorm parameters of the stream (update_conv_weight assembles its stream from them) and the frozen
    // scale pack_conv folded, on the host; with option keep_block_inputs on the device too, so that a later step allocates nothing
    block_bn.clear(); block_scale.clear(); block_scale_off.clear();
    std::vector<double> scales;
    const std::vector<char> kept = scope_graph(kept_scope());         // (of every conv of the kept graph, the blocks among them)
    for (const auto& L : layers) {
        if (L.type != LT_CONV || !trains_folded(L.index, kept)) continue;
        const int blk = L.index;
        const int C = layers[blk].cout;
        const float* p = w + layers[blk].w_off;
        block_bn[blk].assign(p, p + 4 * C);
        std::vector<double>& sc = block_scale[blk];
        sc.resize(C);
        for (int o = 0; o < C; ++o) sc[o] = bn_frozen_scale(p[C + o], p[3 * C + o]);
        block_scale_off[blk] = (int64_t)scales.size();
        scales.insert(scales.end(), sc.begin(), sc.end());
    }
    if (kept_scope() != SCOPE_NONE && !scales.empty()) {
        if ((int64_t)scales.size() > block_scale_doubles) {           // first load (a later one never has more blocks today; if it had, the buffer grows)
            if (d_block_scale) { RTOD_HIP(hipDeviceSynchronize()); RTOD_HIP(hipFree(d_block_scale)); d_block_scale = nullptr; block_scale_doubles = 0; }
            RTOD_HIP(hipMalloc((void**)&d_block_scale, sizeof(double) * scales.size()));
            block_scale_doubles = (int64_t)scales.size();
        }
        RTOD_HIP(hipMemcpy(d_block_scale, scales.data(), sizeof(double) * scales.size(), hipMemcpyHostToDevice));
    }
    RTOD_HIP(hipMemcpy(d_weights, packed.data(), sizeof(float) * (size_t)packed_floats, hipMemcpyHostToDevice));
    RTOD_HIP(hipDeviceSynchronize());
    weights_loaded = true;
    return RTOD_OK;
}

}  // namespace rtod
