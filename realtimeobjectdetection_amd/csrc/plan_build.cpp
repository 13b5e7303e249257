// Plan construction: errors, options, buffer planning (fusions, zero-copy concat, arena), the layout of the packed weights, the
// JSON description.
#include "plan.h"

#include <algorithm>
#include <cstdarg>
#include <sstream>

namespace rtod {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}
const std::string& last_error_string() { return g_err; }

int hip_fail(hipError_t e, const char* what) {
    if (e == hipSuccess) return RTOD_OK;
    set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
    return RTOD_E_HIP;
}

const char* layer_type_name(int t) {
    static const char* n[] = {"convolutional", "shortcut", "route", "upsample", "maxpool", "yolo"};
    return (t >= 0 && t < 6) ? n[t] : "?";
}

Plan::~Plan() {
    for (auto e : events) (void)hipEventDestroy(e);
    if (d_arena) (void)hipFree(d_arena);
    if (d_scratch) (void)hipFree(d_scratch);
    if (d_bn_stats) (void)hipFree(d_bn_stats);
    if (d_bn_partial) (void)hipFree(d_bn_partial);
    if (d_bn_raw) (void)hipFree(d_bn_raw);
    if (d_block_scale) (void)hipFree(d_block_scale);
    if (d_weights) (void)hipFree(d_weights);
}

static int resolve_alias(const std::vector<Layer>& layers, int i) {
    while (layers[i].alias_of >= 0) i = layers[i].alias_of;
    return i;
}

void Plan::reset_planning() {
    for (auto& L : layers) { L.fused_into = -1; L.fused_away = false; L.buf = -1; L.coff = 0; L.alias_of = -1; L.bn_pool = -1; L.z_buf = -1; }
    bufs.clear(); launches.clear(); convs.clear(); input_buf = -1;
    tuned.clear(); tune_cache.clear(); tuning.clear();
}

int Plan::set_option(const char* name, int value) {
    if (!name) { set_error("set_option: null name"); return RTOD_E_ARG; }
    if (d_weights) { set_error("set_option: must be called before rtod_plan_load_weights"); return RTOD_E_STATE; }
    static const struct { const char* name; bool Plan::*flag; } kFlags[] = {
        {"fuse_pointwise", &Plan::opt_fuse_pointwise}, {"ring_kernel", &Plan::opt_ring_kernel}, {"pwd_kernel", &Plan::opt_pwd_kernel},
        {"stem2_kernel", &Plan::opt_stem2_kernel}, {"k_slices", &Plan::opt_k_slices}, {"bn_batch_stats", &Plan::opt_bn_batch_stats},
        {"bn_batch_split", &Plan::opt_bn_batch_split}, {"bn_split_narrow", &Plan::opt_bn_split_narrow}, {"fuse_bn_pool", &Plan::opt_fuse_bn_pool},
        {"k_slice_workgroups", &Plan::opt_k_slice_workgroups}, {"k_slices_split", &Plan::opt_k_slices_split}, {"patch_kernel", &Plan::opt_patch_kernel},
        {"stem_kernel", &Plan::opt_stem_kernel}, {"band_kernel", &Plan::opt_band_kernel}, {"fuse_shortcut", &Plan::opt_fuse_shortcut},
        {"fuse_decode", &Plan::opt_fuse_decode}, {"zero_copy_concat", &Plan::opt_zero_copy_concat}, {"narrow_cin", &Plan::opt_narrow_cin},
        {"stem_pool", &Plan::opt_stem_pool}, {"fuse_stem_pool", &Plan::opt_fuse_stem_pool}, {"keep_head_inputs", &Plan::opt_keep_head_inputs},
        {"keep_block_inputs", &Plan::opt_keep_block_inputs}, {"keep_neck_activations", &Plan::opt_keep_neck_activations},
        {"keep_backbone_activations", &Plan::opt_keep_backbone_activations}, {"keep_full_activations", &Plan::opt_keep_full_activations},
        {"keep_bn_inputs", &Plan::opt_keep_bn_inputs},
    };
    const std::string k(name);
    bool* flag = nullptr; int* num = nullptr;
    for (const auto& f : kFlags) if (k == f.name) flag = &(this->*f.flag);
    if (k == "force_f16s3_variant") num = &opt_force_f16s3_variant;
    else if (k == "force_f32_variant") num = &opt_force_f32_variant;
    else if (!flag) { set_error("set_option: unknown option '%s'", name); return RTOD_E_ARG; }
    // batch-statistics BatchNorm is the reference's own (square) training-mode path: not offered on a rectangular plan
    if (flag == &opt_bn_batch_stats && value && height != width) { set_error("set_option: bn_batch_stats is not supported on a rectangular plan (%dx%d)", height, width); return RTOD_E_ARG; }
    const bool old_flag = flag ? *flag : false; const int old_num = num ? *num : 0;
    if (flag) *flag = value != 0; else *num = value;
    return replan_or([&] { if (flag) *flag = old_flag; else *num = old_num; });
}

// Plans again after a change of an option or the precision.  Refused: `restore` undoes the change, the plan is rebuilt as it
// was and the error message is kept.
int Plan::replan_or(const std::function<void()>& restore) {
    reset_planning();
    int rc = plan_buffers();
    if (!rc && precision >= 1) rc = check_split_supported(precision);
    if (rc) {
        const std::string msg = last_error_string();
        restore();
        reset_planning();
        (void)plan_buffers();
        set_error("%s", msg.c_str());
    }
    return rc;
}

// The launch list depends on the precision (option stem_pool), so a precision change plans again: option-then-precision and
// precision-then-option give the same plan.  Refused: the plan stays as it was.
int Plan::set_precision(int mode) {
    const int old = precision;
    precision = mode;
    return replan_or([&] { precision = old; });
}

// Decode arguments of yolo layer Y: for the head conv it is fused into, or for the stand-alone decode launch
DecodeArgs Plan::decode_args(const Layer& Y) const {
    DecodeArgs d; d.enabled = 1; d.GH = Y.hout; d.GW = Y.wout; d.attrs = 5 + Y.classes; d.n_anchors = (int)Y.anchors.size();
    const int stride = height / Y.hout;                 // == width / Y.wout (resolve_shapes)
    d.stride = (float)stride;
    for (size_t a = 0; a < Y.anchors.size(); ++a) {
        d.aw[a] = (float)((double)Y.anchors[a].first / (double)stride);     // Python float divide -> FloatTensor (util.py:213-216)
        d.ah[a] = (float)((double)Y.anchors[a].second / (double)stride);
        if (Y.decode_v5) { d.aw[a] = (float)Y.anchors[a].first; d.ah[a] = (float)Y.anchors[a].second; }   // pixels
    }
    d.v5 = Y.decode_v5 ? 1 : 0;
    d.img_stride = (int64_t)total_rows * attrs; d.head_off = (int64_t)Y.row_offset * attrs;
    return d;
}

// consumers of every layer's output
std::vector<std::vector<int>> Plan::consumers() const {
    std::vector<std::vector<int>> cons(layers.size());
    for (const auto& L : layers) {
        const int i = L.index;
        switch (L.type) {
            case LT_CONV: case LT_UPSAMPLE: case LT_MAXPOOL: case LT_YOLO: if (i > 0) cons[i - 1].push_back(i); break;
            case LT_SHORTCUT: case LT_ROUTE: for (int s : L.srcs) cons[s].push_back(i); break;
        }
    }
    return cons;
}

// Layer 0 is what the dedicated stem kernel (reads NCHW directly) takes: a plain 3x3 / pad 1 conv of 3 channels with 32 or 64 filters
bool Plan::stem_kernel_shape() const {
    return layers[0].size == 3 && layers[0].pad == 1 && layers[0].cin == 3 && layers[0].cout % 32 == 0 && layers[0].cout <= 64 && layers[0].fused_into < 0 && opt_stem_kernel;
}

int Plan::plan_buffers() {
    const int n = (int)layers.size();
    const std::vector<std::vector<int>> cons = consumers();
    // aliases
    for (auto& L : layers) {
        if (L.type == LT_ROUTE && L.srcs.size() == 1) L.alias_of = L.srcs[0];
        if (L.type == LT_YOLO) L.alias_of = L.index - 1;
    }
    // fusions: conv -> shortcut, conv -> yolo
    for (auto& L : layers) {
        const int i = L.index;
        if (i == 0) continue;
        Layer& P = layers[i - 1];
        if (P.type != LT_CONV || P.fused_into >= 0 || cons[i - 1].size() != 1) continue;
        if (L.type == LT_SHORTCUT && L.srcs[1] != i - 1 && opt_fuse_shortcut && !fusions_held()) { P.fused_into = i; L.fused_away = true; }
        else if (L.type == LT_YOLO && cons[i].empty() && opt_fuse_decode) { P.fused_into = i; L.fused_away = true; }
    }
    // materialised producers: every non-alias layer except convs fused into the next layer and
    // fused yolo layers (their "output" is the final tensor)
    auto materialised = [&](const Layer& L) {
        if (L.alias_of >= 0) return false;
        if (L.type == LT_CONV && L.fused_into >= 0) return false;
        return true;      // (routes with two or more sources: their concat buffer)
    };
    // zero-copy concat placement
    bufs.clear();
    std::vector<int> placed_buf(n, -1), placed_off(n, 0);
    std::vector<std::vector<std::pair<int, int>>> route_copy(n);   // (src layer, coff) needing a copy
    for (auto& L : layers) {
        if (L.type != LT_ROUTE || L.srcs.size() < 2) continue;
        Buffer b; b.C = L.cout; b.H = L.hout; b.W = L.wout;
        const int bid = (int)bufs.size();
        bufs.push_back(b);
        L.buf = bid; L.coff = 0;
        int off = 0;
        for (int s : L.srcs) {
            const int p = resolve_alias(layers, s);
            const Layer& PL = layers[p];
            const bool can = opt_zero_copy_concat && materialised(PL) && PL.type != LT_ROUTE && placed_buf[p] < 0 && off % 4 == 0 && PL.cout % 4 == 0 &&
                             std::count(L.srcs.begin(), L.srcs.end(), s) == 1;
            if (can) { placed_buf[p] = bid; placed_off[p] = off; }
            else route_copy[L.index].push_back({s, off});
            off += layers[s].cout;
        }
    }
    // remaining materialised layers get their own buffer
    for (auto& L : layers) {
        if (!materialised(L) || L.buf >= 0) continue;
        if (L.type == LT_YOLO) continue;
        if (placed_buf[L.index] >= 0) { L.buf = placed_buf[L.index]; L.coff = placed_off[L.index]; continue; }
        Buffer b; b.C = L.cout; b.H = L.hout; b.W = L.wout;
        if (b.C % 4) { set_error("layer %d: %d channels not a multiple of 4 (unsupported for an intermediate tensor)", L.index, b.C); return RTOD_E_CFG; }
        L.buf = (int)bufs.size(); L.coff = 0;
        bufs.push_back(b);
    }
    // network input, packed NHWC with 4 channels
    {
        Buffer b; b.C = 4; b.H = height; b.W = width;
        input_buf = (int)bufs.size();
        bufs.push_back(b);
    }
    // launch list
    launches.clear();
    convs.clear();
    if (layers[0].type != LT_CONV) { set_error("cfg: first layer must be convolutional"); return RTOD_E_CFG; }
    // dedicated stem kernel (reads NCHW directly) when layer 0 is a plain 3x3 / pad 1 conv with 32 or 64 filters
    const bool use_stem = stem_kernel_shape() && !(opt_bn_batch_stats && layers[0].bn);
    // option stem_pool (split-f16 / f16 plans): a 16-filter layer 0 on the split stem of conv_stem16_f16s3.hip, BatchNorm folded or absent
    const bool use_stem16 = opt_stem_pool && precision >= 1 && layers[0].fused_into < 0 &&
                            conv_stem16_supported(layers[0].size, layers[0].stride, layers[0].pad, layers[0].cin, layers[0].cout, layers[0].act);
    if (!use_stem && !use_stem16) { Launch l; l.kind = LK_PACK; l.layer = 0; launches.push_back(l); }
    for (auto& L : layers) {
        const int i = L.index;
        Launch l; l.layer = i;
        switch (L.type) {
            case LT_CONV: {
                l.kind = LK_CONV; l.in_layer = i - 1; l.out_layer = i;
                if (L.fused_into >= 0) {
                    const Layer& F = layers[L.fused_into];
                    if (F.type == LT_SHORTCUT) { l.out_layer = F.index; l.in2_layer = F.srcs[1]; }
                    else { l.out_layer = -2; l.dec = decode_args(F); }
                }
                PackedConv pc; pc.layer = i; pc.cin_p = (i == 0) ? 4 : L.cin;
                if (i == 0 && (use_stem || use_stem16)) { pc.stem = true; pc.stem16 = use_stem16; l.kind = LK_STEM; }
                if (pc.cin_p % 4) { set_error("layer %d: %d input channels not a multiple of 4", i, pc.cin_p); return RTOD_E_CFG; }
                pc.K = L.size * L.size * pc.cin_p; pc.Kpad = (pc.K + 31) / 32 * 32; pc.Npad = (L.cout + 127) / 128 * 128;
                l.conv_slot = (int)convs.size();
                convs.push_back(pc);
                launches.push_back(l);
                break;
            }
            case LT_UPSAMPLE: l.kind = LK_UPSAMPLE; l.in_layer = i - 1; l.out_layer = i; launches.push_back(l); break;
            case LT_MAXPOOL: l.kind = LK_MAXPOOL; l.in_layer = i - 1; l.out_layer = i; launches.push_back(l); break;
            case LT_SHORTCUT:
                if (!L.fused_away) { l.kind = LK_ADD; l.in_layer = L.srcs[0]; l.in2_layer = L.srcs[1]; l.out_layer = i; launches.push_back(l); }
                break;
            case LT_ROUTE:
                for (auto& sc : route_copy[i]) { Launch c; c.kind = LK_COPY; c.layer = i; c.in_layer = sc.first; c.out_buf = L.buf; c.out_coff = sc.second; c.out_layer = i; launches.push_back(c); }
                break;
            case LT_YOLO:
                if (!L.fused_away) {
                    l.kind = LK_DECODE; l.in_layer = i - 1; l.out_layer = -2; l.dec = decode_args(L);
                    launches.push_back(l);
                }
                break;
        }
    }
    // fused-pointwise candidates: conv launch i immediately followed by a 1x1 / stride 1 conv launch that reads exactly
    // i's output, with Cout_i <= 64 (one N tile; wider hosts measured no gain), Cout_j in {16, 32, 64}, no residual / decode on j (conv_f16s3_common.h)
    for (size_t i = 0; i + 1 < launches.size() && !fusions_held(); ++i) {
        Launch& h = launches[i]; Launch& g = launches[i + 1];
        if (h.kind != LK_CONV || g.kind != LK_CONV || h.out_layer < 0 || g.out_layer < 0 || g.in2_layer >= 0 || h.pw_host >= 0) continue;
        const Layer& H = layers[h.layer]; const Layer& G = layers[g.layer];
        if (g.in_layer != h.out_layer || G.size != 1 || G.stride != 1 || G.pad != 0 || G.cin != H.cout) continue;
        if (H.cout % 32 || H.cout > 64 || (G.cout != 16 && G.cout != 32 && G.cout != 64) || G.fused_into >= 0) continue;   // PW_MAX_K
        if (conv_band_supported(H.size, H.stride, H.pad, H.cin, H.win) && H.hout == H.hin) continue;   // band kernel: no pointwise epilogue
        if (opt_narrow_cin && h.layer > 0 && conv_c16_supported(H.cin)) continue;                     // narrow family (conv_c16_f16s3.hip): no pointwise epilogue
        h.pw_guest = (int)i + 1; g.pw_host = (int)i;
    }
    // stem + layer 1 fusion candidate: launch 0 is the stem kernel, launch 1 the conv of layer 1 reading only it, nothing else reads layer 0
    stem2_pattern = false;
    if (!fusions_held() && launches.size() >= 2 && launches[0].kind == LK_STEM && launches[1].kind == LK_CONV && launches[1].layer == 1 && launches[1].in_layer == 0 &&
        launches[1].in2_layer < 0 && launches[1].out_layer == 1 && cons[0].size() == 1 && n > 1) {
        const Layer& L0 = layers[0]; const Layer& L1 = layers[1];
        int pwc = 0;
        if (launches[1].pw_guest >= 0) pwc = layers[launches[launches[1].pw_guest].layer].cout;
        stem2_pattern = L0.bn && L1.bn && L0.act <= 1 && L1.act <= 1 && (launches[1].pw_guest < 0 || layers[launches[launches[1].pw_guest].layer].act <= 1) && conv_stem2_supported(L0.size, L0.stride, L0.pad, L0.cin, L0.cout, L1.size, L1.stride, L1.pad, L1.cout, pwc) &&
                        (pwc == 0 || pwc == 32);
    }
    // 16-filter stem + max-pool fusion candidate: layer 1 is a plain 2x2 / stride-2 pool over an even map and the only reader of layer 0
    // (a BatchNorm layer 0 of a batch-statistics split plan writes raw sums: its pool, if any, rides the normalise kernel — below)
    stem_pool_pattern = use_stem16 && !(bn_split_active() && layers[0].bn) && opt_fuse_stem_pool && n > 1 && layers[1].type == LT_MAXPOOL && layers[1].size == 2 && layers[1].stride == 2 &&
                        layers[1].pool_pad == 0 && cons[0].size() == 1 && layers[0].hout % 2 == 0 && layers[0].wout % 2 == 0 &&
                        launches.size() >= 2 && launches[0].kind == LK_STEM && launches[1].kind == LK_MAXPOOL && launches[1].layer == 1;
    // normalise + max-pool candidates (options bn_split_narrow + fuse_bn_pool): a BatchNorm conv without a fused shortcut / decode whose
    // even map is read by a plain 2x2 / stride-2 pool alone.  Every BatchNorm conv of such a plan has a raw-sum launch.
    // The conv keeps its own full-resolution buffer in the arena (as layer 0 does under stem_pool_pattern): keep_all_layers, which
    // is set after planning and only re-assigns the arena, turns the pair back into the stand-alone form, which writes that buffer
    if (bn_narrow_active() && opt_fuse_bn_pool)
        for (int i = 0; i + 1 < n; ++i) {
            Layer& L = layers[i]; const Layer& P = layers[i + 1];
            if (L.type == LT_CONV && L.bn && L.fused_into < 0 && P.type == LT_MAXPOOL && P.size == 2 && P.stride == 2 && P.pool_pad == 0 &&
                cons[i].size() == 1 && cons[i][0] == i + 1 && L.hout % 2 == 0 && L.wout % 2 == 0)
                L.bn_pool = i + 1;
        }
    // option keep_bn_inputs on a batch-statistics plan: every BatchNorm conv the plan trains writes its raw sums into a buffer of its own
    // (rows of z_stride floats), which nothing reuses before the end of the forward; the normalise step reads it and writes the layer's view
    if (batch_trained()) {
        const std::vector<char> kept = scope_graph(kept_scope());
        for (auto& L : layers) {
            if (L.type != LT_CONV || !trained_member(L.index, kept)) continue;
            Buffer b; b.C = z_stride(L); b.H = L.hout; b.W = L.wout; b.bn_input = true;
            L.z_buf = (int)bufs.size();
            bufs.push_back(b);
        }
    }
    // liveness per buffer over launch time (= layer index of the launch).  Candidates, not forms: the arena covers the fused and the stand-alone schedule
    const int NB = (int)bufs.size();
    for (auto& b : bufs) { b.first = 1 << 30; b.last = -1; }
    auto touch = [&](int buf, int t) { if (buf < 0) return; bufs[buf].first = std::min(bufs[buf].first, t); bufs[buf].last = std::max(bufs[buf].last, t); };
    auto buf_of_layer = [&](int layer) { if (layer < 0) return input_buf; return layers[resolve_alias(layers, layer)].buf; };
    for (const auto& l : launches) {
        const int t = l.layer;
        if (l.kind == LK_PACK) { touch(input_buf, 0); continue; }
        if (l.kind == LK_STEM) {
            touch(buf_of_layer(l.out_layer), t);
            if (stem_pool_pattern) touch(buf_of_layer(1), t);                            // written by the stem's kernel when fused
            if (layers[l.layer].bn_pool >= 0) touch(buf_of_layer(layers[l.layer].bn_pool), t);   // ... by its normalise kernel
            continue;
        }
        if (l.kind == LK_CONV && layers[l.layer].bn_pool >= 0) touch(buf_of_layer(layers[l.layer].bn_pool), t);   // written by the conv's normalise kernel when fused
        if (l.kind == LK_CONV && layers[l.layer].z_buf >= 0) { touch(layers[l.layer].z_buf, t); touch(layers[l.layer].z_buf, n); }
        touch(buf_of_layer(l.in_layer), t);
        if (l.in2_layer >= 0) touch(buf_of_layer(l.in2_layer), t);
        if (l.kind == LK_COPY) touch(l.out_buf, t);
        else if (l.out_layer >= 0) touch(buf_of_layer(l.out_layer), t);
        if (l.pw_guest >= 0) touch(buf_of_layer(launches[l.pw_guest].out_layer), t);     // written by the host's epilogue when fused
    }
    // option keep_head_inputs: what a head conv (the conv in front of a [yolo] layer, decode fused or not) reads stays intact to the
    // end of the forward; nothing else about the plan depends on the option
    if (opt_keep_head_inputs)
        for (const auto& l : launches)
            if (l.kind == LK_CONV && feeds_yolo(l.layer)) touch(buf_of_layer(l.in_layer), n);
    // option keep_block_inputs: likewise what the conv in front of a head conv reads, where the cfg makes that conv a detection
    // block (block_shape_ok; a route is kept as its concat buffer)
    if (opt_keep_block_inputs)
        for (const auto& l : launches)
            if (l.kind == LK_CONV && l.layer + 1 < n && feeds_yolo(l.layer + 1) && block_shape_ok(l.layer)) touch(buf_of_layer(l.in_layer), n);
    // option keep_neck_activations: what every neck conv and every head conv reads and writes (the walk reads outputs for the
    // activation masks, inputs for the weight gradients; routes are kept as their concat buffers)
    // option keep_backbone_activations: the same over the trainable graph, which contains the neck
    // option keep_full_activations: ... over the full graph, which contains that one; its max-pools keep their input and output too
    if (kept_scope() >= SCOPE_NECK) {
        const std::vector<char> neck = scope_graph(kept_scope());
        for (const auto& l : launches)
            if ((l.kind == LK_CONV && (neck[l.layer] || feeds_yolo(l.layer))) || (l.kind == LK_MAXPOOL && neck[l.layer])) {
                touch(buf_of_layer(l.in_layer), n);
                if (l.out_layer >= 0) touch(buf_of_layer(l.out_layer), n);
            }
    }
    // a concat buffer is live from its first producer to its last consumer: touches above cover both
    for (int b = 0; b < NB; ++b) {
        if (bufs[b].last < 0) { bufs[b].first = bufs[b].last = 0; }      // never used (dead layer): still give it space
        bufs[b].floats_per_frame = (int64_t)bufs[b].C * bufs[b].H * bufs[b].W;
    }
    assign_arena();
    layout_weights();
    return RTOD_OK;
}

// Detection blocks.  The cfg's part of the definition: a BatchNorm conv, 1x1 or 3x3 / stride 1 / same padding, leaky or linear,
// reading a multiple of 32 channels, whose BatchNorm is folded — or, on a batch-statistics plan, whose raw output is kept (option
// keep_bn_inputs: the operand of the BatchNorm backward); a batch-statistics plan without it has none.  The mask of a leaky member
// comes from the sign of its stored output, which is act(u) only while no shortcut is added in its normalise step: fused_into < 0
// below keeps such a conv out in every scope.  Layer 0 reads three channels and is none.
bool Plan::block_shape_ok(int layer) const {
    if (layer < 1 || layer >= (int)layers.size() || (opt_bn_batch_stats && !opt_keep_bn_inputs)) return false;
    const Layer& L = layers[layer];
    return L.type == LT_CONV && L.bn && (L.size == 1 || L.size == 3) && L.stride == 1 && L.pad == L.size / 2 && L.act <= 1 &&
           L.cin % 32 == 0 && L.fused_into < 0;
}

// ... and the plan's part: packed in one of the two generic layouts (no stem, not narrow), neither host nor guest of a
// fused-pointwise candidate pair (candidates, not forms, as replaceable_conv), its output stored where rtod_plan_read_layer finds it
bool Plan::block_plan_ok(int layer) const {
    for (const auto& l : launches) {
        if (l.kind != LK_CONV || l.layer != layer || l.conv_slot < 0) continue;
        const PackedConv& pc = convs[l.conv_slot];
        if (pc.stem || pc.stem16 || pc.narrow || l.pw_guest >= 0 || l.pw_host >= 0 || l.out_layer != layer) return false;
        // (layer 0's generic fp32 panel pads its 3 channels per tap to 4: the one layout with cin_p != cin, which head_step_kernel's
        // panel arm writes as it stands; only full_shape_ok lets layer 0 come this far)
        const bool rgb_panel = layer == 0 && !pc.split && layers[layer].cin == 3 && pc.cin_p == 4;
        if (pc.Kpad < pc.K || layers[layer].cout > pc.Npad || (pc.cin_p != layers[layer].cin && !rgb_panel)) return false;
        return layer_form(layer).readable && layers[layer].buf >= 0;
    }
    return false;
}

int Plan::block_of_head(int head) const {
    if (head < 1 || head >= (int)layers.size() || !feeds_yolo(head) || !block_shape_ok(head - 1)) return -1;
    return block_plan_ok(head - 1) ? head - 1 : -1;
}

// The detection neck.  Traversable: a 1x1 head conv (no BatchNorm, Cin a multiple of 32) that [yolo] layers alone read, a BatchNorm
// conv that is a block by both parts of the definition above, a route, a 2x upsample.  A layer is in the graph if it is traversable
// and every reader of its output is in the graph or a [yolo] layer; readers have higher indices, so one descending pass decides it.
// Closure is what makes the gradients exact: nothing outside the graph lies between a member and the loss.
//
// The trainable graph (SCOPE_BACKBONE): the same closure with the two operations Darknet-53's backbone consists of, the 3x3 / stride-2
// conv and the residual [shortcut] (two sources, linear: it adds and carries no mask of its own).  A superset of the neck on every plan
bool Plan::train_shape_ok(int layer) const {
    if (block_shape_ok(layer)) return true;
    if (layer < 1 || layer >= (int)layers.size() || (opt_bn_batch_stats && !opt_keep_bn_inputs)) return false;
    const Layer& L = layers[layer];
    return L.type == LT_CONV && L.bn && L.size == 3 && L.stride == 2 && L.pad == 1 && L.act <= 1 && L.cin % 32 == 0 && L.fused_into < 0;
}

// The full graph (SCOPE_FULL): the same closure with the two operations YOLOv3-tiny's backbone consists of, the conv that reads any
// number of channels (layer 0 reads 3, layer 2 reads 16: rtod_conv_wgrad_thin / rtod_conv_dgrad_thin) and the size-2 max-pool
// (rtod_maxpool_grad).  The plan's part stays block_plan_ok: a stem-layout layer 0 and a narrow-layout conv are no members
bool Plan::full_shape_ok(int layer) const {
    if (train_shape_ok(layer)) return true;
    if (layer < 0 || layer >= (int)layers.size() || (opt_bn_batch_stats && !opt_keep_bn_inputs)) return false;
    // (a batch-statistics plan runs every BatchNorm layer 0 on the generic layout; one that the eval plan gives to the stem kernel stays
    // out all the same, so that a scope names the same convs in both modes)
    if (layer == 0 && opt_bn_batch_stats && stem_kernel_shape()) return false;
    const Layer& L = layers[layer];
    return L.type == LT_CONV && L.bn && (L.size == 1 || L.size == 3) && L.stride == 1 && L.pad == L.size / 2 && L.act <= 1 && L.cin >= 1 && L.fused_into < 0;
}

std::vector<char> Plan::scope_graph(Scope scope) const {
    const int n = (int)layers.size();
    std::vector<char> in(n, 0);
    if (scope < SCOPE_NECK) return in;
    const bool full = scope == SCOPE_FULL, backbone = scope >= SCOPE_BACKBONE;
    const std::vector<std::vector<int>> cons = consumers();
    for (int i = n - 1; i >= 0; --i) {
        const Layer& L = layers[i];
        bool ok = !cons[i].empty();
        if (L.type == LT_CONV && feeds_yolo(i)) {
            ok = ok && !L.bn && L.size == 1 && L.stride == 1 && L.cin % 32 == 0;
            for (int r : cons[i]) ok = ok && layers[r].type == LT_YOLO;
        } else if (L.type == LT_CONV) ok = ok && (full ? full_shape_ok(i) : backbone ? train_shape_ok(i) : block_shape_ok(i)) && block_plan_ok(i);
        else if (L.type == LT_UPSAMPLE) ok = ok && L.stride == 2;
        else if (L.type == LT_SHORTCUT) ok = ok && backbone && L.srcs.size() == 2 && L.act == 0 && !L.fused_away;
        else if (L.type == LT_MAXPOOL) ok = ok && full && L.size == 2 && (L.stride == 1 || L.stride == 2) && L.pool_pad == 0 && !L.fused_away;
        else ok = ok && L.type == LT_ROUTE;
        for (int r : cons[i]) ok = ok && (layers[r].type == LT_YOLO || in[r]);
        in[i] = ok ? 1 : 0;
    }
    return in;
}

// A block stays a block on every plan; the kept graph adds its BatchNorm convs
bool Plan::trained_member(int layer, const std::vector<char>& kept) const {
    return block_of_head(layer + 1) == layer || (layer >= 0 && layer < (int)layers.size() && layers[layer].type == LT_CONV && layers[layer].bn && kept[layer]);
}

// ... trained folded on a plan that folds BatchNorm (a batch-statistics plan trains them through trains_bn / rtod_plan_step_conv_bn)
bool Plan::trains_folded(int layer, const std::vector<char>& kept) const { return !opt_bn_batch_stats && trained_member(layer, kept); }

bool Plan::trains_folded(int layer) const { return trains_folded(layer, scope_graph(kept_scope())); }

bool Plan::uses_split(const Layer& L) const {
    return precision >= 1 && L.index > 0;      // layer 0 stays on an exact-fp32 kernel and writes the split format
}

int Plan::check_split_supported(int mode) const {
    const char* pn = mode == 2 ? "f16" : "f16s3";
    // the BatchNorm backward reads fp32 raw sums: the exact-fp32 kernels write them, and so do the raw-sum instances of the split kernels
    // (bn_split_active); no other plan of these precisions has any
    const bool split_bn = mode == 1 && opt_bn_batch_stats && opt_bn_batch_split;
    if (opt_keep_bn_inputs && !split_bn) {
        set_error("precision %s unsupported with keep_bn_inputs (the BatchNorm backward reads fp32 raw sums: exact-fp32 plans, or f16s3 with bn_batch_stats + bn_batch_split)", pn);
        return RTOD_E_CFG;
    }
    // ... and of those instances the generic, bandd and 1x1 slab tiles alone feed a conv that head_step_kernel can re-pack: the narrow
    // tiles and the 16-filter stem have packers of their own
    if (opt_keep_bn_inputs && (opt_bn_split_narrow || opt_stem_pool)) {
        set_error("precision %s with keep_bn_inputs: option %s is not supported in that mode (narrow tiles and the 16-filter stem are not trained under batch statistics)",
                  pn, opt_bn_split_narrow ? "bn_split_narrow" : "stem_pool");
        return RTOD_E_CFG;
    }
    if (opt_bn_batch_stats && !(opt_bn_batch_split && mode == 1)) {
        set_error("precision %s unsupported with bn_batch_stats (batch-statistics BatchNorm runs on the exact-fp32 kernels%s)", pn,
                  mode == 1 ? "; option bn_batch_split runs it on the split-f16 kernels" : "");
        return RTOD_E_CFG;
    }
    if (opt_bn_batch_stats) {
        // batch-statistics BatchNorm on the split kernels (option bn_batch_split): every BatchNorm conv after layer 0 needs a raw-sum
        // instance — the generic, bandd and 1x1 slab tiles have one; the K-sliced kernels do not; the narrow tiles and the 16-filter stem
        // run theirs with option bn_split_narrow only
        if (opt_k_slices_split || (opt_stem_pool && !opt_bn_split_narrow)) {
            set_error("precision %s with bn_batch_stats + bn_batch_split: option %s is not supported in that mode (layer %d would run a kernel without a raw-sum instance)",
                      pn, opt_k_slices_split ? "k_slices_split" : "stem_pool", opt_stem_pool ? 0 : 1);
            return RTOD_E_CFG;
        }
        for (const auto& l : launches) {
            if (l.kind != LK_CONV || l.layer == 0 || !layers[l.layer].bn) continue;
            const Layer& L = layers[l.layer];
            if (conv_c16_supported(L.cin) && !opt_bn_split_narrow) {
                set_error("precision %s with bn_batch_stats + bn_batch_split: layer %d is a narrow BatchNorm conv (Cin=%d: no raw-sum instance); use fp32", pn, l.layer, L.cin);
                return RTOD_E_CFG;
            }
            if (l.out_layer == -2) { set_error("precision %s with bn_batch_stats + bn_batch_split: layer %d is a BatchNorm conv with a fused head decode; use fp32", pn, l.layer); return RTOD_E_CFG; }
        }
    }
    // precisions 1 and 2 keep every activation in the split f16 layout: every conv but the stem must read
    // 32-channel K-chunks (or, with option narrow_cin, exactly 16 channels), every shortcut / head must ride a conv epilogue, concats must be zero-copy
    for (const auto& l : launches) {
        if (l.kind == LK_ADD && fusions_held()) continue;                         // option keep_backbone_activations: the held shortcuts run the split-format add
        if (l.kind == LK_ADD || l.kind == LK_COPY || l.kind == LK_DECODE) {       // (max-pool and both upsamples have split-format kernels)
            set_error("precision %s unsupported for this cfg (layer %d needs a stand-alone %s kernel); use fp32", pn, l.layer,
                      l.kind == LK_ADD ? "add" : l.kind == LK_COPY ? "copy" : "decode");
            return RTOD_E_CFG;
        }
        if (l.kind == LK_CONV && l.layer > 0) {
            const Layer& L = layers[l.layer];
            const bool cin_ok = L.cin % 32 == 0 || (opt_narrow_cin && conv_c16_supported(L.cin));      // narrow family: conv_c16_f16s3.hip
            if (!cin_ok || L.cout % 8 * (l.out_layer != -2)) {
                set_error("precision %s unsupported for this cfg (layer %d: Cin=%d Cout=%d); use fp32", pn, l.layer, L.cin, L.cout);
                return RTOD_E_CFG;
            }
        }
    }
    for (const auto& b : bufs) if (b.C % 8 && &b != &bufs[input_buf]) { set_error("precision %s: a buffer has %d channels (not a multiple of 8)", pn, b.C); return RTOD_E_CFG; }
    return RTOD_OK;
}

// Slice length, in K-chunks of 32, of a conv whose K sum is formed in slices (0: not sliced): the exact-fp32 panels (option
// k_slices) and the split convs of option k_slices_split; the callers apply their option.  The one place that holds the
// thresholds and lengths; it sees the layer's shape alone (never the batch), so a frame's bits do not depend on the batch it
// rides in.  Deep small-grid layers (13x13 ... 52x52 stages, K >= 256): slices of 9 chunks (one 3x3 tap row of 32 channels; the
// value only has to be fixed per layer), so that a small batch can give every slice its own workgroup; shorter sums (K = 256 ...
// 992: the head and route 1x1 convs of those stages) use slices of 4 / 2.
static int split_slice_chunks(const Layer& L, int kpad) {
    const int nkc = kpad / 32;
    if (L.hout * L.wout > 2704 || nkc < 8) return 0;
    return nkc >= 32 ? 9 : nkc >= 16 ? 4 : 2;
}

void Plan::layout_weights() {
    packed_floats = 0;
    // sliced layers (option k_slices_split): split convs that are neither the stem nor narrow, carry no fused head decode, are
    // neither host nor guest of a fused-pointwise candidate pair nor layer 1 of the fused stem pattern, and that the rule names
    std::vector<const Launch*> launch_of(convs.size(), nullptr);
    for (const auto& l : launches) if ((l.kind == LK_CONV || l.kind == LK_STEM) && l.conv_slot >= 0) launch_of[l.conv_slot] = &l;
    bn_stats_doubles = 0;
    for (auto& pc : convs) {
        pc.stats_off = -1;
        if (opt_bn_batch_stats && layers[pc.layer].bn) { pc.stats_off = bn_stats_doubles; bn_stats_doubles += 2 * (int64_t)pc.Npad; }
    }
    for (auto& pc : convs) {
        const Layer& L = layers[pc.layer];
        pc.split = uses_split(L);
        pc.narrow = false;
        const int64_t panel = (int64_t)pc.Npad * pc.Kpad;
        if (pc.stem && precision >= 1) {                              // split stem: [Cout][32] f16 hi, lo, inv_scale (its hi output is plain f16's format too)
            pc.split = true;
            pc.w_off = packed_floats; packed_floats += 16 * (int64_t)L.cout;
            pc.wl_off = packed_floats; packed_floats += 16 * (int64_t)L.cout;
            pc.s_off = packed_floats; packed_floats += L.cout;
        } else if (pc.stem) {
            pc.w_off = packed_floats; packed_floats += 28 * (int64_t)L.cout;
        } else if (pc.split) {
            pc.w_off = packed_floats; packed_floats += panel / 2;       // f16 hi plane
            pc.wl_off = packed_floats; packed_floats += panel / 2;      // f16 lo plane
            pc.s_off = packed_floats; packed_floats += pc.Npad;
            pc.narrow = opt_narrow_cin && conv_c16_supported(L.cin);
            const Launch* ll = launch_of[&pc - &convs[0]];
            pc.ks_chunks = 0;                                         // (candidates, not forms: a sliced conv is never part of a pair that may fuse)
            if (opt_k_slices_split && ll && !pc.narrow && ll->out_layer != -2 && ll->pw_guest < 0 && ll->pw_host < 0 &&
                !(stem2_pattern && pc.layer == 1) && pc.K == pc.Kpad && L.cin % 32 == 0)
                pc.ks_chunks = split_slice_chunks(L, pc.Kpad);
            pc.band = conv_band_supported(L.size, L.stride, L.pad, L.cin, L.win) && L.hout == L.hin &&
                      !(L.fused_into >= 0 && layers[L.fused_into].type == LT_YOLO) && opt_band_kernel && !pc.narrow && pc.ks_chunks == 0;
        } else {
            pc.w_off = packed_floats; packed_floats += panel;
            pc.slice_chunks = opt_k_slices ? split_slice_chunks(L, pc.Kpad) : 0;
        }
        pc.b_off = packed_floats; packed_floats += pc.Npad;
        if (opt_bn_batch_stats && L.bn) { pc.bn_off = packed_floats; packed_floats += 2 * (int64_t)pc.Npad; }
        packed_floats = (packed_floats + 63) / 64 * 64;
    }
    bn_raw_floats = 0;                                                   // every layer with its own row stride
    if (bn_split_active())
        for (const auto& pc : convs) {
            const Layer& L = layers[pc.layer];
            if (L.bn) bn_raw_floats = std::max(bn_raw_floats, (int64_t)max_batch * L.hout * L.wout * raw_stride(pc));
        }
}

// Rows of the raw-sum scratch: Npad floats apart for the tiles that had a raw-sum instance before option bn_split_narrow (and the
// exact-fp32 layer 0), dense — Cout rounded up to 8 — for the narrow tiles and the 16-filter stem: their layers are the largest maps
// with the fewest channels (16 filters at 416x416 would use 64 of every 512 bytes)
int Plan::raw_stride(const PackedConv& pc) const {
    return (pc.split && (pc.narrow || pc.stem16)) ? (layers[pc.layer].cout + 7) / 8 * 8 : pc.Npad;
}

// Floats per row of a kept BatchNorm input (Layer::z_buf), the one rule: dense, Cout, where an exact-fp32 conv writes it as its own
// output; on a batch-statistics split plan the buffer stands in for the raw-sum scratch of that conv, so its rows are the scratch's
// (raw_stride: Npad, which the bandd and slab tiles require of raw_ld and the generic tiles, the exact-fp32 layer 0 and
// launch_bn_batch_split accept).  bn_input_view, and through it read_bn_input, take the stride from the buffer.
int Plan::z_stride(const Layer& L) const {
    if (bn_split_active())
        for (const auto& pc : convs) if (pc.layer == L.index) return raw_stride(pc);
    return L.cout;
}

void Plan::assign_arena() {
    const int NB = (int)bufs.size();
    // greedy arena assignment (first fit by offset among lifetime-overlapping buffers)
    std::vector<int> order(NB);
    for (int i = 0; i < NB; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return bufs[a].first != bufs[b].first ? bufs[a].first < bufs[b].first : a < b; });
    std::vector<int> done;
    arena_floats = 0;
    for (int id : order) {
        Buffer& B = bufs[id];
        const int64_t size = (B.floats_per_frame * max_batch + 63) / 64 * 64;   // 256-B granules
        if (B.bn_input) continue;                                               // (below)
        std::vector<std::pair<int64_t, int64_t>> busy;
        for (int o : done) {
            const Buffer& O = bufs[o];
            if (!keep_all && (O.last < B.first || O.first > B.last)) continue;
            busy.push_back({O.offset, O.offset + (O.floats_per_frame * max_batch + 63) / 64 * 64});
        }
        std::sort(busy.begin(), busy.end());
        int64_t off = 0;
        for (auto& iv : busy) { if (off + size <= iv.first) break; off = std::max(off, iv.second); }
        B.offset = off;
        arena_floats = std::max(arena_floats, off + size);
        done.push_back(id);
    }
    // the kept BatchNorm inputs (option keep_bn_inputs) live to the end of the forward and are never reused: one after the other behind
    // the arena above, which is assigned as if they were not there (that of the eval plan with the same keep option)
    for (auto& B : bufs) {
        if (!B.bn_input) continue;
        B.offset = arena_floats;
        arena_floats += (B.floats_per_frame * max_batch + 63) / 64 * 64;
    }
}

View Plan::bn_input_view(int layer) const {
    View v;
    if (layer < 0 || layer >= (int)layers.size() || layers[layer].z_buf < 0) return v;
    const Layer& L = layers[layer];
    const Buffer& b = bufs[L.z_buf];
    v.base = d_arena ? d_arena + b.offset : nullptr;
    v.ldc = b.C; v.coff = 0; v.C = L.cout; v.H = L.hout; v.W = L.wout;
    return v;
}

View Plan::view_of(int layer) const {
    View v;
    if (layer < 0) {
        const Buffer& b = bufs[input_buf];
        v.base = d_arena ? d_arena + b.offset : nullptr; v.ldc = 4; v.coff = 0; v.C = 4; v.H = height; v.W = width;
        return v;
    }
    const Layer& L = layers[resolve_alias(layers, layer)];
    if (L.buf < 0) return v;
    const Buffer& b = bufs[L.buf];
    v.split = precision;                   // 0 fp32, 1 split hi + lo, 2 the split layout with the hi plane alone
    v.base = d_arena ? d_arena + b.offset : nullptr;
    v.ldc = b.C; v.coff = L.coff; v.C = L.cout; v.H = L.hout; v.W = L.wout;
    return v;
}

std::string Plan::describe() const {
    std::ostringstream os;
    os << "{\"height\":" << height << ",\"width\":" << width << ",\"total_rows\":" << total_rows << ",\"attrs\":" << attrs
       << ",\"n_weight_floats\":" << n_weight_floats << ",\"conv_flops\":" << conv_flops << ",\"arena_floats\":" << arena_floats
       << ",\"n_launches\":" << launches.size() << ",\"layers\":[";
    for (size_t i = 0; i < layers.size(); ++i) {
        const Layer& L = layers[i];
        if (i) os << ",";
        os << "{\"index\":" << L.index << ",\"type\":\"" << layer_type_name(L.type) << "\",\"cin\":" << L.cin << ",\"cout\":" << L.cout
           << ",\"hin\":" << L.hin << ",\"win\":" << L.win << ",\"hout\":" << L.hout << ",\"wout\":" << L.wout << ",\"size\":" << L.size
           << ",\"stride\":" << L.stride << ",\"pad\":" << L.pad << ",\"bn\":" << (L.bn ? "true" : "false") << ",\"leaky\":" << (L.act == 1 ? "true" : "false") << ",\"act\":" << L.act << ",\"decode_v5\":" << (L.decode_v5 ? "true" : "false") << ",\"nearest\":" << (L.nearest ? "true" : "false") << ",\"pool_pad\":" << L.pool_pad
           << ",\"srcs\":[";
        for (size_t s = 0; s < L.srcs.size(); ++s) os << (s ? "," : "") << L.srcs[s];
        os << "],\"anchors\":[";
        for (size_t a = 0; a < L.anchors.size(); ++a) os << (a ? "," : "") << "[" << L.anchors[a].first << "," << L.anchors[a].second << "]";
        os << "],\"classes\":" << L.classes << ",\"row_offset\":" << L.row_offset << ",\"rows\":" << L.rows << ",\"w_off\":" << L.w_off
           << ",\"fused_into\":" << layer_form((int)i).fused_into << ",\"fused_away\":" << (L.fused_away ? "true" : "false") << ",\"alias_of\":" << L.alias_of
           << ",\"buf\":" << L.buf << ",\"coff\":" << L.coff;
        if (L.type == LT_CONV)                                                       // sliced layers only (option k_slices_split)
            for (const auto& pc : convs)
                if (pc.layer == L.index && pc.split && pc.ks_chunks > 0) os << ",\"k_slices\":" << (pc.Kpad / 32 + pc.ks_chunks - 1) / pc.ks_chunks;
        os << "}";
    }
    os << "],\"bufs\":[";
    for (size_t i = 0; i < bufs.size(); ++i) {
        const Buffer& b = bufs[i];
        if (i) os << ",";
        os << "{\"C\":" << b.C << ",\"H\":" << b.H << ",\"W\":" << b.W << ",\"first\":" << b.first << ",\"last\":" << b.last << ",\"offset\":" << b.offset
           << ",\"floats_per_frame\":" << b.floats_per_frame << "}";
    }
    os << "]";
    if (bn_split_active()) os << ",\"bn_batch_split\":true,\"bn_raw_bytes\":" << bn_raw_floats * 4;     // batch-statistics BatchNorm on the split kernels: its raw-sum scratch
    if (bn_split_active() && batch_trained()) {                        // ... trained there (option keep_bn_inputs): the kept raw sums behind the arena
        int64_t kept = 0;
        for (const auto& b : bufs) if (b.bn_input) kept += (b.floats_per_frame * max_batch + 63) / 64 * 64;
        os << ",\"bn_batch_trained\":\"split\",\"bn_input_bytes\":" << kept * 4;
    }
    os << "}";
    return os.str();
}

}  // namespace rtod
