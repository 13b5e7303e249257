// Plan execution: the launch list on a stream.  Forward interpreter of the reference: src/darknet.py:199-303.
#include "plan.h"

#include <algorithm>
#include <cstring>

namespace rtod {

// The run-time predicates over the candidates that planning found; form / layer_form below are their only readers
bool Plan::pw_active() const { return precision == 1 && opt_fuse_pointwise && !bn_split_active(); }
bool Plan::stem2_active() const { return precision == 1 && !bn_split_active() && opt_stem2_kernel && stem2_pattern && !keep_all && convs[launches[0].conv_slot].split; }
// The one decision of option keep_backbone_activations: the three fusions that leave a trainable conv's own output unstored (a
// shortcut in its epilogue, the stem2 kernel's layer 1) or make block_plan_ok refuse it (a pointwise candidate pair) are not formed
// as CANDIDATES (plan_buffers asks), so the predicates above never see them and the forward is that of a plan with fuse_shortcut,
// fuse_pointwise and stem2_kernel off
// (keep_full_activations, its superset, holds the same three)
bool Plan::fusions_held() const { return opt_keep_backbone_activations || opt_keep_full_activations; }
int Plan::fused_pool(int layer) const {
    if (keep_all) return -1;                                     // every layer's own map is stored
    if (layer == 0 && precision >= 1 && stem_pool_pattern && convs[launches[0].conv_slot].stem16) return 1;
    return bn_narrow_active() && opt_fuse_bn_pool ? layers[layer].bn_pool : -1;
}

// How launch li runs (LaunchForm, plan.h): the one place that puts candidates and predicates together.  A few compares per call
LaunchForm Plan::form(size_t li) const {
    LaunchForm f;
    const Launch& l = launches[li];
    switch (l.kind) {
        case LK_MAXPOOL:                                         // a fused pool is the launch after its conv's / stem's
            if (li > 0 && launches[li - 1].conv_slot >= 0 && fused_pool(launches[li - 1].layer) == l.layer) f.inside = (int)li - 1;
            return f;
        case LK_STEM: if (stem2_active()) f.inside = 1; break;
        case LK_CONV:
            if (l.pw_host >= 0 && pw_active()) f.inside = l.pw_host;
            else { f.stem2 = li == 1 && stem2_active(); f.guest = l.pw_guest >= 0 && pw_active() ? l.pw_guest : -1; }
            break;
        default: return f;
    }
    if (f.inside >= 0) return f;
    const bool split = convs[l.conv_slot].split;
    f.raw = bn_split_active() && layers[l.layer].bn;
    f.pool = fused_pool(l.layer);
    f.epi = l.out_layer == -2 ? 2 : (f.guest >= 0 ? 3 : 0) + (l.in2_layer >= 0 ? 1 : 0);
    if (split && precision == 2) f.epi |= EPI_F16;                // plain-f16 instance of the split kernels
    if (split && f.raw) f.epi = EPI_RAW;                          // raw-sum instance (the shortcut rides the normalise kernel)
    return f;
}

// Layer 0 inside the fused stem kernel keeps its arena buffer (liveness covers both schedules) and stays readable, though no kernel writes it
LayerForm Plan::layer_form(int layer) const {
    const int pool = fused_pool(layer);
    if (pool >= 0) return {pool, false};
    return {layer == 0 && stem2_active() ? 1 : layers[layer].fused_into, true};
}

int Plan::build_conv_args(const Launch& l, const LaunchForm& f, int batch, float* out, ConvArgs& a) const {
    const Layer& L = layers[l.layer];
    const PackedConv& pc = convs[l.conv_slot];
    const View in = view_of(l.in_layer);
    a.in = in.base; a.in_ldc = in.ldc; a.in_coff = in.coff;
    a.B = batch; a.Hi = L.hin; a.Wi = L.win; a.Cin = pc.cin_p;
    a.w = d_weights + pc.w_off; a.bias = d_weights + pc.b_off; a.K = pc.K; a.Kpad = pc.Kpad; a.Npad = pc.Npad;
    a.in_bytes = (unsigned)std::min<int64_t>((int64_t)batch * in.H * in.W * in.ldc * 4, 0xFFFFFFFFll);
    a.w_bytes = (unsigned)std::min<int64_t>((int64_t)pc.Npad * pc.Kpad * 2, 0xFFFFFFFFll);
    if (pc.split) {
        a.w_hi = reinterpret_cast<const _Float16*>(d_weights + pc.w_off);
        a.w_lo = reinterpret_cast<const _Float16*>(d_weights + pc.wl_off);
        a.inv_scale = d_weights + pc.s_off;
        a.f16 = precision == 2 ? 1 : 0;
    }
    a.kh = a.kw = L.size; a.stride = L.stride; a.pad = L.pad;
    a.Ho = L.hout; a.Wo = L.wout; a.Cout = L.cout; a.leaky = L.act;
    a.ovf = overflow_flag;
    if (in.C != pc.cin_p || in.H != L.hin || in.W != L.win) { set_error("forward: layer %d input view mismatch", l.layer); return RTOD_E_STATE; }
    if (l.out_layer == -2) { a.out = out; a.dec = l.dec; a.dec.train = train_decode; }
    else {
        const View o = view_of(l.out_layer);
        if (!o.base || o.C != L.cout || o.H != L.hout || o.W != L.wout) { set_error("forward: layer %d output view mismatch", l.layer); return RTOD_E_STATE; }
        a.out = o.base; a.out_ldc = o.ldc; a.out_coff = o.coff; a.out_split = o.split;
    }
    if (l.in2_layer >= 0) {
        const View r = view_of(l.in2_layer);
        if (!r.base || r.C != L.cout || r.H != L.hout || r.W != L.wout) { set_error("forward: layer %d residual view mismatch", l.layer); return RTOD_E_STATE; }
        a.res = r.base; a.res_ldc = r.ldc; a.res_coff = r.coff;
    }
    if (f.guest >= 0) {
        const Launch& g = launches[f.guest];
        const Layer& G = layers[g.layer];
        const PackedConv& gc = convs[g.conv_slot];
        const View o = view_of(g.out_layer);
        if (!gc.split || gc.Kpad != L.cout || !o.base || !o.split || o.C != G.cout || o.H != L.hout || o.W != L.wout) { set_error("forward: layer %d fused pointwise mismatch", g.layer); return RTOD_E_STATE; }
        a.pw_wh = reinterpret_cast<const _Float16*>(d_weights + gc.w_off);
        a.pw_wl = reinterpret_cast<const _Float16*>(d_weights + gc.wl_off);
        a.pw_inv_scale = d_weights + gc.s_off; a.pw_bias = d_weights + gc.b_off;
        a.pw_out = o.base; a.pw_out_ldc = o.ldc; a.pw_out_coff = o.coff;
        a.pw_cout = G.cout; a.pw_k = L.cout; a.pw_leaky = G.act; a.pw_npad = gc.Npad;
    }
    return RTOD_OK;
}

// fp32 view of the raw sums of launch `l`'s conv at this batch, rows of raw_stride floats: the conv's own kept buffer where the plan trains
// it (option keep_bn_inputs: the same rows, which then survive the forward), else the shared scratch (base null: no scratch / too small)
View Plan::bn_raw_view(const Launch& l, int batch) const {
    View v = bn_input_view(l.layer);
    if (v.base) return v;
    const Layer& L = layers[l.layer];
    const PackedConv& pc = convs[l.conv_slot];
    if (!d_bn_raw || (int64_t)batch * L.hout * L.wout * raw_stride(pc) > bn_raw_floats) return v;
    v.base = d_bn_raw; v.ldc = raw_stride(pc); v.coff = 0; v.C = L.cout; v.H = L.hout; v.W = L.wout;
    return v;
}

// Every head of the plan, in the arithmetic of the kernel that decodes it in a forward: fused into a split-f16 / f16 conv the
// epilogue of conv_f16s3_common.h (hardware exp2), otherwise the exact-fp32 conv epilogue or the stand-alone kernel (libm expf).
int Plan::finish_decode(float* out, int batch, hipStream_t s) const {
    if (!out) { set_error("finish_decode: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || batch > max_batch) { set_error("finish_decode: batch %d outside 1..%d", batch, max_batch); return RTOD_E_ARG; }
    for (const auto& l : launches)
        if (l.out_layer == -2 && l.dec.v5) { set_error("finish_decode: layer %d decodes YOLOv5-style, which has no TRAIN=True form", l.layer); return RTOD_E_CFG; }
    RTOD_HIP(hipSetDevice(device));
    for (const auto& l : launches) {
        if (l.out_layer != -2) continue;
        if (int rc = launch_finish_decode(out, batch, l.dec, precision >= 1 && l.kind == LK_CONV ? 1 : 0, s)) return rc;
    }
    return RTOD_OK;
}

// The raw-sum step of a BatchNorm conv of a batch-statistics split plan (bn_split_active): its raw view, or the refusal.  The one
// precondition check of that step, made before anything is launched; `site_ok`: what the calling site requires of its launch besides
int Plan::raw_bn_begin(const Launch& l, int batch, bool site_ok, View& raw) const {
    raw = bn_raw_view(l, batch);
    if (!site_ok || !raw.base || !d_bn_stats || convs[l.conv_slot].stats_off < 0) { set_error("forward: layer %d: batch-statistics BatchNorm on an unsupported launch", l.layer); return RTOD_E_STATE; }
    return RTOD_OK;
}

// ... after the raw conv has been enqueued: statistics, then normalise + activation + shortcut into the split format, with the
// max-pool that follows into the view of that layer (`pool`, LaunchForm::pool) when the form says so
int Plan::run_raw_bn(const Launch& l, const View& raw, int pool, int batch, hipStream_t s) const {
    const Layer& L = layers[l.layer];
    const PackedConv& pc = convs[l.conv_slot];
    View r; if (l.in2_layer >= 0) r = view_of(l.in2_layer);
    return launch_bn_batch_split(raw, view_of(pool >= 0 ? pool : l.out_layer), l.in2_layer >= 0 ? &r : nullptr, batch, d_bn_stats + pc.stats_off, pc.Npad, d_weights + pc.bn_off, pc.Npad,
                                 L.act, d_bn_partial, bn_partial_count, overflow_flag, s, pool >= 0 ? 1 : 0);
}

// A conv on the exact-fp32 kernels: every conv of an fp32 plan, layer 0 of a split plan without a stem kernel
int Plan::run_conv_f32(const Launch& l, const LaunchForm& f, ConvArgs& a, int batch, hipStream_t s) const {
    const Layer& L = layers[l.layer];
    const PackedConv& pc = convs[l.conv_slot];
    const int v = choose_variant(L, batch);
    const int mode = f32_slice_mode(l, batch, v);
    a.slice_chunks = mode ? pc.slice_chunks : 0;
    if (mode == 2) { a.partial = d_scratch; a.partial_floats = scratch_floats; }
    if (!(opt_bn_batch_stats && L.bn)) return launch_conv(a, v, s);
    // raw conv, then statistics + normalise + activation + shortcut, in place unless the raw sums are kept
    if (a.dec.enabled || (a.out_split && !bn_split_active()) || !d_bn_stats || pc.stats_off < 0) { set_error("forward: layer %d: batch-statistics BatchNorm on an unsupported launch", l.layer); return RTOD_E_STATE; }
    a.leaky = 0; a.res = nullptr;
    if (a.out_split) {                           // split plan (option bn_batch_split), layer 0: raw sums to the scratch, normalised into the split format
        const View rv = bn_raw_view(l, batch);
        if (!rv.base) { set_error("forward: layer %d: no raw-sum scratch", l.layer); return RTOD_E_STATE; }
        a.out = rv.base; a.out_ldc = rv.ldc; a.out_coff = 0; a.out_split = 0;
        if (int rc = launch_conv(a, v, s)) return rc;
        return run_raw_bn(l, rv, f.pool, batch, s);
    }
    // (option keep_bn_inputs, a conv the plan trains: the raw sums go to the conv's own buffer and stay there; the same values, read from there)
    const View o = view_of(l.out_layer), z = bn_input_view(l.layer);
    if (z.base) { a.out = z.base; a.out_ldc = z.ldc; a.out_coff = 0; }
    if (int rc = launch_conv(a, v, s)) return rc;
    View r; if (l.in2_layer >= 0) r = view_of(l.in2_layer);
    return launch_bn_batch(z.base ? z : o, o, l.in2_layer >= 0 ? &r : nullptr, batch, d_bn_stats + pc.stats_off, pc.Npad, d_weights + pc.bn_off, pc.Npad, L.act, d_bn_partial, bn_partial_count, s);
}

// A conv on a split-f16 / f16 tile; a BatchNorm conv of a batch-statistics split plan (LaunchForm::raw): raw sums, statistics, normalise
int Plan::run_conv_split(size_t li, const LaunchForm& f, ConvArgs& a, int batch, hipStream_t s, bool tune_now) {
    const Launch& l = launches[li];
    const PackedConv& pc = convs[l.conv_slot];
    View rv;
    if (f.raw) {
        if (int rc = raw_bn_begin(l, batch, !a.dec.enabled && !a.pw_wh, rv)) return rc;
        a.raw_out = rv.base; a.raw_ld = (int)rv.ldc; a.res = nullptr; a.leaky = 0;
    }
    if (tune_now) { if (int rc = tune_launch(li, a, batch, s)) return rc; }      // (never reached for the fused stem launch)
    if (int rc = launch_split_variant(a, pc, tune_now && tuning[li] >= 0 ? tuning[li] : variant_for(l, batch), s)) return rc;
    return f.raw ? run_raw_bn(l, rv, f.pool, batch, s) : RTOD_OK;
}

int Plan::run_conv(size_t li, const LaunchForm& f, const float* x, int batch, float* out, hipStream_t s, bool tune_now) {
    const Launch& l = launches[li];
    ConvArgs a;
    if (int rc = build_conv_args(l, f, batch, out, a)) return rc;
    if (!convs[l.conv_slot].split) return run_conv_f32(l, f, a, batch, s);
    if (!f.stem2) return run_conv_split(li, f, a, batch, s, tune_now);
    // stem + this conv (+ its hosted 1x1) in one kernel
    const PackedConv& p0 = convs[launches[0].conv_slot];
    return launch_conv_stem2_f16s3(x, batch, height, width, reinterpret_cast<const _Float16*>(d_weights + p0.w_off),
                                   reinterpret_cast<const _Float16*>(d_weights + p0.wl_off), d_weights + p0.s_off, d_weights + p0.b_off,
                                   layers[0].act, a, s);
}

// Layer 0 on a kernel that reads the NCHW input itself
int Plan::run_stem(const Launch& l, const LaunchForm& f, const float* x, int batch, hipStream_t s) const {
    const Layer& L = layers[l.layer];
    const PackedConv& pc = convs[l.conv_slot];
    const View o = view_of(l.out_layer);
    const _Float16* wh = reinterpret_cast<const _Float16*>(d_weights + pc.w_off);
    const _Float16* wl = reinterpret_cast<const _Float16*>(d_weights + pc.wl_off);
    if (!pc.stem16) {
        if (pc.split) return launch_conv_stem_split(x, wh, wl, d_weights + pc.s_off, d_weights + pc.b_off, o, batch, height, width, L.hout, L.wout, L.stride, L.cout, L.act, overflow_flag, s);
        return launch_conv_stem(x, d_weights + pc.w_off, d_weights + pc.b_off, o, batch, height, width, L.hout, L.wout, L.stride, L.cout, L.act, s);
    }
    // 16 filters: stand-alone, or with layer 1's max-pool (writes layer 1's view)
    if (!pc.split) { set_error("forward: the 16-filter stem needs a split-f16 / f16 plan"); return RTOD_E_STATE; }
    if (f.raw) {                                                 // raw sums (unfolded weights), statistics, normalise (+ the max-pool that follows)
        View rv;
        if (int rc = raw_bn_begin(l, batch, opt_bn_split_narrow, rv)) return rc;
        if (int rc = launch_conv_stem16_raw(x, wh, wl, d_weights + pc.s_off, rv, batch, height, width, s)) return rc;
        return run_raw_bn(l, rv, f.pool, batch, s);
    }
    return launch_conv_stem16_f16s3(x, wh, wl, d_weights + pc.s_off, d_weights + pc.b_off, f.pool >= 0 ? view_of(f.pool) : o, batch, height, width, L.act, f.pool >= 0 ? 1 : 0, overflow_flag, s);
}

int Plan::forward(const float* x, int batch, float* out, hipStream_t s, float* launch_ms, bool tune) {
    if (!weights_loaded) { set_error("forward: load_weights has not been called"); return RTOD_E_STATE; }
    if (!x || !out) { set_error("forward: null pointer"); return RTOD_E_ARG; }
    if (batch < 1 || batch > max_batch) { set_error("forward: batch %d outside 1..%d", batch, max_batch); return RTOD_E_ARG; }
    RTOD_HIP(hipSetDevice(device));
    // rtod_plan_autotune only: rtod_forward never measures, never synchronises (safe under stream capture)
    const bool tune_now = tune && precision >= 1 && opt_force_f16s3_variant < 0;
    if (tune_now) { tuning.assign(launches.size(), -1); tune_cache.clear(); }
    const size_t nl = launches.size();
    if (launch_ms && events.size() < 2 * nl) {
        while (events.size() < 2 * nl) { hipEvent_t e; RTOD_HIP(hipEventCreate(&e)); events.push_back(e); }
    }
    for (size_t li = 0; li < nl; ++li) {
        const Launch& l = launches[li];
        if (launch_ms) RTOD_HIP(hipEventRecord(events[2 * li], s));
        const LaunchForm f = form(li);
        int rc = RTOD_OK;
        if (f.inside < 0) switch (l.kind) {                             // (inside >= 0: that launch's kernel does the work)
            case LK_PACK: {
                View v = view_of(-1);
                rc = launch_pack_input(x, batch, 3, height, width, v.base, 4, s);
                break;
            }
            case LK_CONV: rc = run_conv(li, f, x, batch, out, s, tune_now); break;
            case LK_STEM: rc = run_stem(l, f, x, batch, s); break;
            case LK_UPSAMPLE:
                rc = layers[l.layer].nearest ? launch_upsample_nearest2x(view_of(l.in_layer), view_of(l.out_layer), batch, s)
                                             : launch_upsample2x(view_of(l.in_layer), view_of(l.out_layer), batch, s);
                break;
            case LK_MAXPOOL:
                rc = launch_maxpool(view_of(l.in_layer), view_of(l.out_layer), batch, layers[l.layer].size, layers[l.layer].stride, layers[l.layer].pool_pad, s); break;
            case LK_ADD: rc = launch_add(view_of(l.in_layer), view_of(l.in2_layer), view_of(l.out_layer), batch, s, overflow_flag); break;
            case LK_COPY: {
                const View in = view_of(l.in_layer);
                View o; const Buffer& b = bufs[l.out_buf];
                o.base = d_arena + b.offset; o.ldc = b.C; o.coff = l.out_coff; o.C = in.C; o.H = in.H; o.W = in.W;
                rc = launch_copy(in, o, batch, s);
                break;
            }
            case LK_DECODE: {
                const View in = view_of(l.in_layer);
                // NHWC strides of the raw head tensor
                DecodeArgs d = l.dec; d.train = train_decode;
                rc = launch_decode(in.base + in.coff, (int64_t)in.H * in.W * in.ldc, 1, (int64_t)in.W * in.ldc, in.ldc, batch, d, out, s);
                break;
            }
        }
        if (rc) return rc;
        if (launch_ms) RTOD_HIP(hipEventRecord(events[2 * li + 1], s));
    }
    if (tune_now) tuned[batch] = tuning;
    if (launch_ms) {
        RTOD_HIP(hipEventSynchronize(events[2 * nl - 1]));
        for (size_t li = 0; li < nl; ++li) RTOD_HIP(hipEventElapsedTime(&launch_ms[li], events[2 * li], events[2 * li + 1]));
    }
    return RTOD_OK;
}

// FLOPs and weight bytes of one conv layer, added to the launch that runs it
static void add_conv_cost(const Layer& L, rtod_launch_info* o) {
    o->flops_per_frame += 2ll * L.hout * L.wout * L.cout * L.cin * L.size * L.size;
    o->weight_bytes += ((int64_t)L.cout * L.cin * L.size * L.size + L.cout) * 4;
}

void Plan::fill_launch_info(int idx, rtod_launch_info* o, int batch) const {
    memset(o, 0, sizeof(*o));
    const Launch& l = launches[idx];
    o->layer = l.layer; o->kind = l.kind; o->variant = -1;
    if (l.kind == LK_PACK) { o->bytes_per_frame = (int64_t)height * width * (3 + 4) * 4; return; }
    const Layer& L = layers[l.layer];
    o->ksize = L.size; o->stride = L.stride; o->cin = L.cin; o->cout = L.cout; o->hout = L.hout; o->wout = L.wout;
    const LaunchForm f = form(idx);
    if (f.inside >= 0) return;                                                       // accounted on the launch that does its work
    const int64_t in_b = (int64_t)L.hin * L.win * L.cin * 4, out_b = (int64_t)L.hout * L.wout * L.cout * 4;
    switch (l.kind) {
        case LK_CONV:
            if (f.stem2) o->variant = 100 + STEM2_VARIANT;
            else if (convs[l.conv_slot].split) o->variant = 100 + variant_for(l, batch);
            else { const int v = choose_variant(L, batch); o->variant = v + 10 * f32_slice_mode(l, batch, v); }   // tile + 10 * K-slice schedule
            o->fused_residual = l.in2_layer >= 0; o->fused_decode = l.out_layer == -2;
            [[fallthrough]];
        case LK_STEM:                                                                // (never a shortcut, a hosted 1x1 or the fused stem kernel)
            add_conv_cost(L, o);
            o->bytes_per_frame = in_b + (f.pool >= 0 ? out_b / 4 : out_b) + (l.in2_layer >= 0 ? out_b : 0);   // (fused 2x2 pool: the pooled map is what is written)
            if (f.stem2) {                                                           // fused stem: its FLOPs ride here, its output is never written
                add_conv_cost(layers[0], o);
                o->bytes_per_frame = (int64_t)layers[0].hin * layers[0].win * layers[0].cin * 4 + out_b;
            }
            if (f.guest >= 0) {
                const Layer& G = layers[launches[f.guest].layer];
                o->fused_pointwise = 1;
                add_conv_cost(G, o);
                o->bytes_per_frame += (int64_t)G.hout * G.wout * G.cout * 4;
            }
            break;
        case LK_ADD: o->bytes_per_frame = 3 * out_b; break;
        default: o->bytes_per_frame = in_b + out_b; break;
    }
}

}  // namespace rtod
