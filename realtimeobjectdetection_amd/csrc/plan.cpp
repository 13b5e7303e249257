// Plan construction + execution.  Behavioural sources in the reference (file:line into
// /root/reference): cfg grammar src/darknet.py:428-447; channel bookkeeping and module semantics
// src/darknet.py:449-603; forward interpreter src/darknet.py:199-303; weight stream order
// src/darknet.py:316-410.
#include "plan.h"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
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
    if (d_weights) (void)hipFree(d_weights);
}

// ------------------------------------------------------------------------------------- cfg
static std::string rstrip(const std::string& s) {
    size_t e = s.size();
    while (e > 0 && isspace((unsigned char)s[e - 1])) --e;
    return s.substr(0, e);
}
static std::string lstrip(const std::string& s) {
    size_t b = 0;
    while (b < s.size() && isspace((unsigned char)s[b])) ++b;
    return s.substr(b);
}

static bool to_int(const std::string& s, int& out) {   // Python int(): optional surrounding blanks
    const std::string t = rstrip(lstrip(s));
    if (t.empty()) return false;
    char* end = nullptr;
    long v = strtol(t.c_str(), &end, 10);
    if (*end) return false;
    out = (int)v;
    return true;
}

static std::vector<std::string> split(const std::string& s, char d) {
    std::vector<std::string> out;
    std::string cur;
    for (char c : s) {
        if (c == d) { out.push_back(cur); cur.clear(); } else cur.push_back(c);
    }
    out.push_back(cur);
    return out;
}

struct Block { std::string type; std::map<std::string, std::string> kv; };

static int parse_blocks(const std::string& text, std::vector<Block>& blocks) {
    Block cur;
    bool have = false;
    for (const std::string& raw : split(text, '\n')) {
        if (raw.empty()) continue;
        if (raw[0] == '#') continue;                 // tested before stripping (darknet.py:432)
        const std::string line = rstrip(lstrip(raw));
        if (line.empty()) continue;
        if (line[0] == '[') {
            if (have) blocks.push_back(cur);
            cur = Block();
            have = true;
            cur.type = rstrip(line.substr(1, line.size() >= 2 ? line.size() - 2 : 0));
        } else {
            const auto parts = split(line, '=');
            if (parts.size() != 2 || !have) { set_error("cfg: malformed line '%s'", line.c_str()); return RTOD_E_CFG; }
            cur.kv[rstrip(parts[0])] = lstrip(parts[1]);
        }
    }
    if (have) blocks.push_back(cur);
    if (blocks.empty() || blocks[0].type != "net") { set_error("cfg: first block must be [net]"); return RTOD_E_CFG; }
    return RTOD_OK;
}

#define CFG_INT(blk, key, var)                                                                  \
    do {                                                                                        \
        auto _it = (blk).kv.find(key);                                                          \
        if (_it == (blk).kv.end() || !to_int(_it->second, var)) {                               \
            set_error("cfg: layer %d [%s]: missing/invalid '%s'", i, (blk).type.c_str(), key);  \
            return RTOD_E_CFG;                                                                  \
        }                                                                                       \
    } while (0)

int Plan::parse(const std::string& text) {
    std::vector<Block> blocks;
    int rc = parse_blocks(text, blocks);
    if (rc) return rc;
    net_info = blocks[0].kv;
    layers.clear();
    for (size_t bi = 1; bi < blocks.size(); ++bi) {
        const Block& b = blocks[bi];
        const int i = (int)bi - 1;
        Layer L;
        L.index = i;
        if (b.type == "convolutional") {
            L.type = LT_CONV;
            int bn = 0;
            auto it = b.kv.find("batch_normalize");
            L.bn = (it != b.kv.end() && to_int(it->second, bn) && bn != 0);
            int padflag = 0;
            CFG_INT(b, "filters", L.cout);
            CFG_INT(b, "size", L.size);
            CFG_INT(b, "stride", L.stride);
            CFG_INT(b, "pad", padflag);
            L.pad = padflag ? (L.size - 1) / 2 : 0;
            auto act = b.kv.find("activation");
            if (act == b.kv.end()) { set_error("cfg: layer %d: missing activation", i); return RTOD_E_CFG; }
            L.leaky = act->second == "leaky";
            L.act = L.leaky ? 1 : (act->second == "silu" || act->second == "swish") ? 2 : 0;    // silu: cfg extension
            if (L.cout < 1 || L.size < 1 || L.stride < 1) { set_error("cfg: layer %d: bad conv geometry", i); return RTOD_E_CFG; }
        } else if (b.type == "upsample") {
            L.type = LT_UPSAMPLE;
            int st = 0;
            CFG_INT(b, "stride", st);   // parsed but ignored: scale_factor=2 is hard-coded (darknet.py:589-592)
            L.stride = 2;
            auto md = b.kv.find("mode");                 // cfg extension: mode=nearest (default: the reference's bilinear)
            L.nearest = md != b.kv.end() && md->second == "nearest";
        } else if (b.type == "maxpool") {
            L.type = LT_MAXPOOL;
            CFG_INT(b, "size", L.size);
            CFG_INT(b, "stride", L.stride);
            int sym = 0;
            auto sy = b.kv.find("symmetric");            // cfg extension: -inf padding of (size-1)/2 on every side
            if (sy != b.kv.end() && to_int(sy->second, sym) && sym) L.pool_pad = (L.size - 1) / 2;
            if (L.size < 1 || L.stride < 1) { set_error("cfg: layer %d: bad pool geometry", i); return RTOD_E_CFG; }
        } else if (b.type == "shortcut") {
            L.type = LT_SHORTCUT;
            int from = 0;
            CFG_INT(b, "from", from);
            L.srcs = {i - 1, i + from};
        } else if (b.type == "route") {
            L.type = LT_ROUTE;
            auto it = b.kv.find("layers");
            if (it == b.kv.end()) { set_error("cfg: layer %d: route without layers", i); return RTOD_E_CFG; }
            for (const std::string& tok : split(it->second, ',')) {
                int v = 0;
                if (!to_int(tok, v)) { set_error("cfg: layer %d: bad route entry '%s'", i, tok.c_str()); return RTOD_E_CFG; }
                L.srcs.push_back(v > 0 ? v : i + v);           // positive = absolute (darknet.py:274-275)
            }
            if (L.srcs.empty() || L.srcs.size() > 4) {         // the reference handles one or two sources; up to four here (SPPF-style concats: cfg extension)
                set_error("cfg: layer %d: route with %zu sources unsupported", i, L.srcs.size()); return RTOD_E_CFG;
            }
        } else if (b.type == "yolo") {
            L.type = LT_YOLO;
            auto m = b.kv.find("mask"), a = b.kv.find("anchors");
            if (m == b.kv.end() || a == b.kv.end()) { set_error("cfg: layer %d: yolo without mask/anchors", i); return RTOD_E_CFG; }
            std::vector<int> av;
            for (const std::string& tok : split(a->second, ',')) { int v; if (!to_int(tok, v)) { set_error("cfg: bad anchor"); return RTOD_E_CFG; } av.push_back(v); }
            for (const std::string& tok : split(m->second, ',')) {
                int v;
                if (!to_int(tok, v) || v < 0 || 2 * v + 1 >= (int)av.size()) { set_error("cfg: layer %d: bad mask", i); return RTOD_E_CFG; }
                L.anchors.push_back({av[2 * v], av[2 * v + 1]});
            }
            CFG_INT(b, "classes", L.classes);
            auto dv = b.kv.find("decode");                // cfg extension: decode=v5
            L.decode_v5 = dv != b.kv.end() && dv->second == "v5";
            if (L.anchors.empty() || L.anchors.size() > 4) { set_error("cfg: layer %d: 1..4 anchors per head supported", i); return RTOD_E_CFG; }
        } else {
            set_error("Unknown block error: A unknown block is provided: [%s]", b.type.c_str());   // darknet.py:524-526
            return RTOD_E_CFG;
        }
        layers.push_back(L);
    }
    if (layers.empty()) { set_error("cfg: no layers"); return RTOD_E_CFG; }
    return RTOD_OK;
}

int Plan::resolve_shapes() {
    int pc = 3, ph = height, pw = width;
    int row_off = 0;
    int64_t woff = 0;
    conv_flops = 0;
    attrs = 0;
    bool prev_is_decoded = false;
    for (auto& L : layers) {
        const int i = L.index;
        auto src_ok = [&](int s) { return s >= 0 && s < i; };
        if ((L.type == LT_CONV || L.type == LT_UPSAMPLE || L.type == LT_MAXPOOL || L.type == LT_YOLO) && prev_is_decoded) {
            set_error("cfg: layer %d consumes a decoded yolo tensor (unsupported)", i); return RTOD_E_CFG;
        }
        L.cin = pc; L.hin = ph; L.win = pw;
        switch (L.type) {
            case LT_CONV:
                L.hout = (ph + 2 * L.pad - L.size) / L.stride + 1;
                L.wout = (pw + 2 * L.pad - L.size) / L.stride + 1;
                if (L.hout < 1 || L.wout < 1) { set_error("cfg: layer %d: empty conv output", i); return RTOD_E_CFG; }
                L.w_off = woff;
                woff += (L.bn ? 4 : 1) * (int64_t)L.cout + (int64_t)L.cout * L.cin * L.size * L.size;
                conv_flops += 2ll * L.hout * L.wout * L.cout * L.cin * L.size * L.size;
                break;
            case LT_UPSAMPLE: L.cout = pc; L.hout = 2 * ph; L.wout = 2 * pw; break;
            case LT_MAXPOOL:
                L.cout = pc;
                if (L.pool_pad) { L.hout = (ph + 2 * L.pool_pad - L.size) / L.stride + 1; L.wout = (pw + 2 * L.pool_pad - L.size) / L.stride + 1; }
                else if (L.stride != 1) { L.hout = (ph - L.size) / L.stride + 1; L.wout = (pw - L.size) / L.stride + 1; }
                else { L.hout = ph; L.wout = pw; }
                if (L.hout < 1 || L.wout < 1) { set_error("cfg: layer %d: empty pool output", i); return RTOD_E_CFG; }
                break;
            case LT_SHORTCUT: {
                if (i < 1 || !src_ok(L.srcs[1])) { set_error("cfg: layer %d: shortcut source out of range", i); return RTOD_E_CFG; }
                const Layer& a = layers[L.srcs[0]]; const Layer& b = layers[L.srcs[1]];
                if (a.cout != b.cout || a.hout != b.hout || a.wout != b.wout) { set_error("cfg: layer %d: shortcut shape mismatch", i); return RTOD_E_CFG; }
                L.cout = a.cout; L.hout = a.hout; L.wout = a.wout;
                break;
            }
            case LT_ROUTE: {
                int c = 0;
                for (int s : L.srcs) {
                    if (!src_ok(s)) { set_error("cfg: layer %d: route source %d out of range", i, s); return RTOD_E_CFG; }
                    if (layers[s].hout != layers[L.srcs[0]].hout || layers[s].wout != layers[L.srcs[0]].wout) { set_error("cfg: layer %d: route spatial mismatch", i); return RTOD_E_CFG; }
                    c += layers[s].cout;
                }
                L.cout = c; L.cin = c; L.hout = layers[L.srcs[0]].hout; L.wout = layers[L.srcs[0]].wout;
                break;
            }
            case LT_YOLO: {
                if (i < 1) { set_error("cfg: yolo as first layer"); return RTOD_E_CFG; }
                const int A = (int)L.anchors.size();
                if (pc != A * (5 + L.classes)) { set_error("cfg: layer %d: head has %d channels, expected %d", i, pc, A * (5 + L.classes)); return RTOD_E_CFG; }
                // stride = inp_dim // G, G' = inp_dim // stride (util.py:194-195) must equal G — per axis, and the decode has one stride:
                // a rectangular input needs height // GH == width // GW (square inputs: the reference's own condition)
                if (ph > height || pw > width || height / (height / ph) != ph || width / (width / pw) != pw) {
                    set_error("cfg: layer %d: grid %dx%d does not divide input %dx%d", i, ph, pw, height, width); return RTOD_E_CFG;
                }
                if (height / ph != width / pw) {
                    set_error("cfg: layer %d: head grid %dx%d has stride %d along y but %d along x for input %dx%d (one integer stride on both axes is required)",
                              i, ph, pw, height / ph, width / pw, height, width);
                    return RTOD_E_CFG;
                }
                if (attrs && attrs != 5 + L.classes) { set_error("cfg: heads with different class counts"); return RTOD_E_CFG; }
                attrs = 5 + L.classes;
                L.cout = pc; L.hout = ph; L.wout = pw;
                L.row_offset = row_off; L.rows = ph * pw * A;
                row_off += L.rows;
                break;
            }
        }
        if (L.type == LT_YOLO) {
            prev_is_decoded = true;       // x = decoded tensor; outputs[i] = outputs[i-1] (darknet.py:247)
            pc = layers[i - 1].cout; ph = layers[i - 1].hout; pw = layers[i - 1].wout;
        } else {
            prev_is_decoded = false;
            pc = L.cout; ph = L.hout; pw = L.wout;
        }
        if (L.type == LT_ROUTE || L.type == LT_SHORTCUT) prev_is_decoded = false;
    }
    total_rows = row_off;
    n_weight_floats = woff;
    if (total_rows == 0) { set_error("cfg: no yolo layer (the reference would return [])"); return RTOD_E_CFG; }
    return RTOD_OK;
}

// ------------------------------------------------------------------------------------- planning
static int resolve_alias(const std::vector<Layer>& layers, int i) {
    while (layers[i].alias_of >= 0) i = layers[i].alias_of;
    return i;
}

void Plan::reset_planning() {
    for (auto& L : layers) { L.fused_into = -1; L.fused_away = false; L.buf = -1; L.coff = 0; L.alias_of = -1; L.bn_pool = -1; }
    bufs.clear(); launches.clear(); convs.clear(); input_buf = -1;
    tuned.clear(); tune_cache.clear(); tuning.clear();
}

int Plan::set_option(const char* name, int value) {
    if (!name) { set_error("set_option: null name"); return RTOD_E_ARG; }
    if (d_weights) { set_error("set_option: must be called before rtod_plan_load_weights"); return RTOD_E_STATE; }
    const std::string k(name);
    bool* flag = nullptr; int* num = nullptr;
    if (k == "fuse_pointwise") flag = &opt_fuse_pointwise;
    else if (k == "ring_kernel") flag = &opt_ring_kernel;
    else if (k == "pwd_kernel") flag = &opt_pwd_kernel;
    else if (k == "stem2_kernel") flag = &opt_stem2_kernel;
    else if (k == "k_slices") flag = &opt_k_slices;
    else if (k == "bn_batch_stats") {
        // batch-statistics BatchNorm is the reference's own (square) training-mode path: not offered on a rectangular plan
        if (value && height != width) { set_error("set_option: bn_batch_stats is not supported on a rectangular plan (%dx%d)", height, width); return RTOD_E_ARG; }
        flag = &opt_bn_batch_stats;
    }
    else if (k == "bn_batch_split") flag = &opt_bn_batch_split;
    else if (k == "bn_split_narrow") flag = &opt_bn_split_narrow;
    else if (k == "fuse_bn_pool") flag = &opt_fuse_bn_pool;
    else if (k == "k_slice_workgroups") flag = &opt_k_slice_workgroups;
    else if (k == "k_slices_split") flag = &opt_k_slices_split;
    else if (k == "patch_kernel") flag = &opt_patch_kernel;
    else if (k == "stem_kernel") flag = &opt_stem_kernel;
    else if (k == "band_kernel") flag = &opt_band_kernel;
    else if (k == "fuse_shortcut") flag = &opt_fuse_shortcut;
    else if (k == "fuse_decode") flag = &opt_fuse_decode;
    else if (k == "zero_copy_concat") flag = &opt_zero_copy_concat;
    else if (k == "narrow_cin") flag = &opt_narrow_cin;
    else if (k == "stem_pool") flag = &opt_stem_pool;
    else if (k == "fuse_stem_pool") flag = &opt_fuse_stem_pool;
    else if (k == "force_f16s3_variant") num = &opt_force_f16s3_variant;
    else if (k == "force_f32_variant") num = &opt_force_f32_variant;
    else { set_error("set_option: unknown option '%s'", name); return RTOD_E_ARG; }
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

int Plan::plan_buffers() {
    const int n = (int)layers.size();
    // consumers of every layer's output
    std::vector<std::vector<int>> cons(n);
    for (const auto& L : layers) {
        const int i = L.index;
        switch (L.type) {
            case LT_CONV: case LT_UPSAMPLE: case LT_MAXPOOL: case LT_YOLO: if (i > 0) cons[i - 1].push_back(i); break;
            case LT_SHORTCUT: case LT_ROUTE: for (int s : L.srcs) cons[s].push_back(i); break;
        }
    }
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
        if (L.type == LT_SHORTCUT && L.srcs[1] != i - 1 && opt_fuse_shortcut) { P.fused_into = i; L.fused_away = true; }
        else if (L.type == LT_YOLO && cons[i].empty() && opt_fuse_decode) { P.fused_into = i; L.fused_away = true; }
    }
    // materialised producers: every non-alias layer except convs fused into the next layer and
    // fused yolo layers (their "output" is the final tensor)
    auto materialised = [&](const Layer& L) {
        if (L.alias_of >= 0) return false;
        if (L.type == LT_CONV && L.fused_into >= 0) return false;
        if (L.type == LT_ROUTE) return true;      // two-source concat buffer
        return true;
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
    const bool use_stem = layers[0].size == 3 && layers[0].pad == 1 && layers[0].cin == 3 && layers[0].cout % 32 == 0 &&
                          layers[0].cout <= 64 && layers[0].fused_into < 0 && opt_stem_kernel && !(opt_bn_batch_stats && layers[0].bn);
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
    for (size_t i = 0; i + 1 < launches.size(); ++i) {
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
    if (launches.size() >= 2 && launches[0].kind == LK_STEM && launches[1].kind == LK_CONV && launches[1].layer == 1 && launches[1].in_layer == 0 &&
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
    // liveness per buffer over launch time (= layer index of the launch)
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
        touch(buf_of_layer(l.in_layer), t);
        if (l.in2_layer >= 0) touch(buf_of_layer(l.in2_layer), t);
        if (l.kind == LK_COPY) touch(l.out_buf, t);
        else if (l.out_layer >= 0) touch(buf_of_layer(l.out_layer), t);
        if (l.pw_guest >= 0) touch(buf_of_layer(launches[l.pw_guest].out_layer), t);     // written by the host's epilogue when fused
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

bool Plan::uses_split(const Layer& L, int cin_p) const {
    return precision >= 1 && L.index > 0;      // layer 0 stays on an exact-fp32 kernel and writes the split format
}

int Plan::check_split_supported(int mode) const {
    const char* pn = mode == 2 ? "f16" : "f16s3";
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
        pc.split = uses_split(L, pc.cin_p);
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
            pc.ks_chunks = 0;
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

// ------------------------------------------------------------------------------------- weights
static uint16_t f32_to_f16_rn(float f) {           // IEEE binary16, round to nearest even, host side
    uint32_t x; memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7FFFFFFFu;
    if (x >= 0x7F800000u) return (uint16_t)(sign | (x > 0x7F800000u ? 0x7E00u : 0x7C00u));
    if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);               // rounds to >= 65520 -> inf
    if (x < 0x33000001u) return (uint16_t)sign;                             // < 2^-25 -> 0
    int e = (int)(x >> 23) - 127;
    uint32_t m = (x & 0x7FFFFFu) | 0x800000u;
    int shift = (e < -14) ? (13 + (-14 - e)) : 13;                          // subnormal halves lose extra bits
    uint32_t half_m = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (half_m & 1))) ++half_m;
    uint32_t out;
    if (e < -14) out = half_m;                                               // subnormal (may carry into normal)
    else out = ((uint32_t)(e + 15) << 10) + (half_m - 0x400u);               // carry propagates into the exponent
    return (uint16_t)(sign | out);
}
static float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const int e = (h >> 10) & 0x1F; const uint32_t m = h & 0x3FFu;
    float v;
    if (e == 0) v = std::ldexp((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = std::ldexp((float)(m | 0x400u), e - 25);
    uint32_t x; memcpy(&x, &v, 4); x |= sign; memcpy(&v, &x, 4);
    return v;
}

int Plan::load_weights(const float* w, size_t n) {
    if (!w) { set_error("load_weights: null pointer"); return RTOD_E_ARG; }
    if ((int64_t)n < n_weight_floats) {
        set_error("load_weights: stream has %zu floats, network needs %lld", n, (long long)n_weight_floats);
        return RTOD_E_SIZE;
    }
    RTOD_HIP(hipSetDevice(device));
    std::vector<float> packed((size_t)packed_floats, 0.0f);
    for (const auto& pc : convs) {
        const Layer& L = layers[pc.layer];
        const float* p = w + L.w_off;
        const int C = L.cout, cin = L.cin, k = L.size;
        std::vector<double> scale(C, 1.0);
        float* bias = packed.data() + pc.b_off;
        if (L.bn && opt_bn_batch_stats) {
            // batch-statistics mode: the conv stays unfolded (no bias), beta / gamma go to the normalisation kernel; the
            // stream's running mean / variance are not used (the reference only updates them as a side effect)
            float* bnp = packed.data() + pc.bn_off;
            for (int o = 0; o < C; ++o) { bias[o] = 0.f; bnp[o] = p[o]; bnp[pc.Npad + o] = p[C + o]; }
            p += 4 * C;
        } else if (L.bn) {
            const float *beta = p, *gamma = p + C, *mean = p + 2 * C, *var = p + 3 * C;
            for (int o = 0; o < C; ++o) {
                // eval BatchNorm (x - mean) / sqrt(var + 1e-5) * gamma + beta folded into the conv
                const double s = (double)gamma[o] / std::sqrt((double)var[o] + 1e-5);
                scale[o] = s;
                bias[o] = (float)((double)beta[o] - (double)mean[o] * s);
            }
            p += 4 * C;
        } else {
            for (int o = 0; o < C; ++o) bias[o] = p[o];
            p += C;
        }
        if (pc.stem && pc.split) {
            // [Cout][32] f16 hi / lo planes, k = (ky*3+kx)*3 + c, k >= 27 zero; per-channel power-of-two pre-scale as below
            uint16_t* wh = reinterpret_cast<uint16_t*>(packed.data() + pc.w_off);
            uint16_t* wl = reinterpret_cast<uint16_t*>(packed.data() + pc.wl_off);
            float* inv = packed.data() + pc.s_off;
            const int64_t per_o = (int64_t)cin * k * k;
            for (int o = 0; o < C; ++o) {
                double mx = 0.0;
                for (int64_t q = 0; q < per_o; ++q) mx = std::max(mx, std::fabs((double)p[o * per_o + q] * scale[o]));
                int e = 0;
                if (mx > 0.0) { int ex; std::frexp(mx, &ex); e = 13 - ex; }
                e = std::max(-24, std::min(40, e));
                const double ps = std::ldexp(1.0, e);
                inv[o] = (float)(std::ldexp(1.0, -e) / (double)ACT_SCALE_F16S3);
                for (int q = 0; q < 32; ++q) { wh[o * 32 + q] = 0; wl[o * 32 + q] = 0; }
                for (int c = 0; c < cin; ++c)
                    for (int ky = 0; ky < k; ++ky)
                        for (int kx = 0; kx < k; ++kx) {
                            const float v = (float)((double)p[(((int64_t)o * cin + c) * k + ky) * k + kx] * scale[o]);
                            const float vs = (float)((double)v * ps);
                            const uint16_t h = f32_to_f16_rn(vs);
                            const int idx = o * 32 + (ky * k + kx) * 3 + c;
                            wh[idx] = h; wl[idx] = f32_to_f16_rn(vs - f16_to_f32(h));
                        }
            }
        } else if (pc.stem) {
            float* wp = packed.data() + pc.w_off;                 // [28][Cout], k = (ky*3+kx)*3 + c
            for (int o = 0; o < C; ++o)
                for (int c = 0; c < cin; ++c)
                    for (int ky = 0; ky < k; ++ky)
                        for (int kx = 0; kx < k; ++kx) {
                            const float v = p[(((int64_t)o * cin + c) * k + ky) * k + kx];
                            wp[(int64_t)((ky * k + kx) * 3 + c) * C + o] = (float)((double)v * scale[o]);
                        }
        } else if (!pc.split) {
            float* wp = packed.data() + pc.w_off;
            for (int o = 0; o < C; ++o)
                for (int c = 0; c < cin; ++c)
                    for (int ky = 0; ky < k; ++ky)
                        for (int kx = 0; kx < k; ++kx) {
                            const float v = p[(((int64_t)o * cin + c) * k + ky) * k + kx];          // OIHW
                            wp[(int64_t)o * pc.Kpad + (ky * k + kx) * pc.cin_p + c] = (float)((double)v * scale[o]);
                        }
        } else {
            // f16 hi/lo planes.  Per output channel a power-of-two pre-scale 2^e puts max|w| in
            // [2^12, 2^13): low parts of weights down to 2^-16 of the channel maximum stay normal f16.
            uint16_t* wh = reinterpret_cast<uint16_t*>(packed.data() + pc.w_off);
            uint16_t* wl = reinterpret_cast<uint16_t*>(packed.data() + pc.wl_off);
            float* inv = packed.data() + pc.s_off;
            for (int o = 0; o < pc.Npad; ++o) inv[o] = 1.0f / ACT_SCALE_F16S3;
            const int64_t per_o = (int64_t)cin * k * k;
            for (int o = 0; o < C; ++o) {
                double mx = 0.0;
                for (int64_t q = 0; q < per_o; ++q) mx = std::max(mx, std::fabs((double)p[o * per_o + q] * scale[o]));
                int e = 0;
                if (mx > 0.0) { int ex; std::frexp(mx, &ex); e = 13 - ex; }      // mx * 2^e in [2^12, 2^13)
                e = std::max(-24, std::min(40, e));
                const double ps = std::ldexp(1.0, e);
                inv[o] = (float)(std::ldexp(1.0, -e) / (double)ACT_SCALE_F16S3);
                for (int c = 0; c < cin; ++c)
                    for (int ky = 0; ky < k; ++ky)
                        for (int kx = 0; kx < k; ++kx) {
                            const float v = (float)((double)p[(((int64_t)o * cin + c) * k + ky) * k + kx] * scale[o]);   // the fp32 folded weight
                            const float vs = (float)((double)v * ps);                                                    // exact (power of two)
                            const uint16_t h = f32_to_f16_rn(vs);
                            const uint16_t l = f32_to_f16_rn(vs - f16_to_f32(h));
                            // K order of the split kernels: k = ((c/32)*k*k + tap)*32 + c%32 (channel chunk outer, tap inner);
                            // planes are K-chunk major, [chunk][Npad][32]: the rows of one stage are contiguous
                            // narrow layers (conv_c16_f16s3.hip): tap-major over the 16 channels, k = tap * 16 + c, so chunk j holds
                            // taps 2j and 2j + 1 (the unused half of the last chunk of an odd tap count stays zero in both planes)
                            const int tap = ky * k + kx;
                            const int64_t idx = pc.narrow ? ((int64_t)(tap / 2) * pc.Npad + o) * 32 + (tap % 2) * 16 + c
                                                          : ((int64_t)((c / 32) * k * k + tap) * pc.Npad + o) * 32 + (c % 32);
                            wh[idx] = h; wl[idx] = l;
                        }
            }
        }
    }
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
    RTOD_HIP(hipMemcpy(d_weights, packed.data(), sizeof(float) * (size_t)packed_floats, hipMemcpyHostToDevice));
    RTOD_HIP(hipDeviceSynchronize());
    weights_loaded = true;
    return RTOD_OK;
}

// ------------------------------------------------------------------------------------- forward
int Plan::choose_variant(const Layer& L, int batch) const {
    if (opt_force_f32_variant >= 0 && opt_force_f32_variant < CV_COUNT) return opt_force_f32_variant;
    if (L.cout <= 32) return CV_128x32;
    if (L.cout <= 64) return CV_128x64;
    const int64_t M = (int64_t)batch * L.hout * L.wout;
    const int64_t big = ((M + 127) / 128) * ((L.cout + 127) / 128);
    return big >= 512 ? CV_128x128 : CV_64x64;     // keep >= 2 workgroups per CU in flight
}

// Schedule of a K-sliced exact-fp32 launch: its own workgroup per slice while the tile grid alone leaves the chip idle
// (fewer than two 256-thread workgroups per CU) and the slice panels fit the scratch; both schedules give the same bits.
int Plan::f32_slice_mode(const Launch& l, int batch, int variant) const {
    const PackedConv& pc = convs[l.conv_slot];
    if (pc.split || pc.stem || pc.slice_chunks <= 0) return 0;
    const Layer& L = layers[l.layer];
    const ConvVariantInfo& vi = conv_variant_info(variant);
    const int64_t M = (int64_t)batch * L.hout * L.wout;
    const int64_t tiles = ((M + vi.bm - 1) / vi.bm) * ((L.cout + vi.bn - 1) / vi.bn);
    const int64_t S = (pc.Kpad / 32 + pc.slice_chunks - 1) / pc.slice_chunks;
    return (opt_k_slice_workgroups && d_scratch && tiles < 512 && S * M * pc.Npad <= scratch_floats) ? 2 : 1;
}

// ------------------------------------------------------------------------------------- split-f16 tiles
// Which tile a split-f16 conv launch runs is decided here and nowhere else: tile_legal (may it?), default_tile (the closed-form
// choice), variant_for (forced / tuned / default), tile_candidates (what autotune times); ids resolve through family_of
// (split_tiles.cpp).
//
// May launch `l` run tile `v` and give this layer's defined bits?  Does not depend on the batch; a one-workgroup-per-slice tile
// whose panels do not fit the scratch is legal here: variant_for runs schedule A of the same tile (same bits), set_tiles refuses it.
// Plain-f16 plans (precision 2) run the tiles that have an f16 instance (the f16 column of the family table): the generic, bandd
// (band layers, and the wide tile of the other 3x3 stride-1 layers), 1x1 slab, narrow and K-sliced tiles; never conv_band / ring /
// patch, and no hosted pointwise epilogue (pw_active).
// A BatchNorm conv of a batch-statistics split plan (raw_launch) runs the tiles with a raw-sum instance (the raw column) that its
// family rules admit; for layers that are neither narrow nor sliced that is the set of a plain-f16 plan.
bool Plan::tile_legal(const Launch& l, int /*batch*/, int v) const {
    const TileRef t = family_of(v);
    if (!t || l.kind != LK_CONV || l.conv_slot < 0 || !convs[l.conv_slot].split) return false;
    const PackedConv& pc = convs[l.conv_slot];
    const Layer& L = layers[l.layer];
    if (precision == 2 && !t.f16()) return false;
    if (raw_launch(l) && !t.raw()) return false;
    // own K order / packed weights / summation order: narrow, sliced and band layers run their family only, and no other layer does
    if (pc.narrow || t.is(TF_C16)) return pc.narrow && t.is(TF_C16);
    if (pc.ks_chunks > 0 || t.is(TF_KS)) return pc.ks_chunks > 0 && t.is(TF_KS);
    if (pc.band) return t.is(TF_BAND) && conv_band_mode_valid(t.mode, L.cin, L.hin, L.win);
    // the other layers: generic K order.  plain = no fused head decode, no hosted pointwise conv
    const bool hosts_pw = l.pw_guest >= 0 && pw_active(), plain = l.out_layer != -2 && !hosts_pw, same_map = L.hout == L.hin && L.wout == L.win;
    switch (t.fam->id) {
        case TF_GENERIC: return !(hosts_pw && t.fam->info(t.mode).bn < L.cout);        // fused pointwise: one N tile must cover every output channel
        // the one-buffer bandd tile: 3x3 stride-1 layers too wide for the band family's LDS budget at three workgroups per CU
        case TF_BAND: return t.bandd_wide() && opt_band_kernel && plain && same_map && pc.Npad % 128 == 0 && pc.K == pc.Kpad &&
                             conv_bandd_wide_supported(L.size, L.stride, L.pad, pc.cin_p, L.win);
        // (SiLU layers: only the kernels with the LDS-transposed epilogue carry that activation: generic, band and slab tiles)
        case TF_RING: return !hosts_pw && L.act <= 1;
        case TF_PWD: return opt_pwd_kernel && plain && same_map && conv_pwd_supported(L.size, L.stride, L.pad, pc.cin_p);   // whole 64-channel slabs
        case TF_PATCH: return plain && L.act <= 1 && L.hout == L.hin && conv_patch_supported(L.size, L.stride, L.pad, L.cin, L.cout) &&
                              conv_patch_mode_valid(t.mode, L.cin, L.cout);
    }
    return false;
}

// The closed-form choice (no forced id, no tuned entry, or an illegal one)
int Plan::default_tile(const Launch& l, int batch) const {
    const PackedConv& pc = convs[l.conv_slot];
    const Layer& L = layers[l.layer];
    const int64_t M = (int64_t)batch * L.hout * L.wout;
    if (pc.narrow) return tile_id(TF_C16, conv_c16_default_mode(L.cout, M));
    // sliced: the 64x64 tile, and like f32_slice_mode one workgroup per (tile, slice) while the tile grid alone leaves the chip idle
    if (pc.ks_chunks > 0) return tile_id(TF_KS, ((M + 63) / 64) * ((L.cout + 63) / 64) < 512 ? 1 : 0);
    if (pc.band) {
        if (precision != 2 && !raw_launch(l)) return tile_id(TF_BAND, conv_band_default_mode(L.cin, L.hin, L.win));
        const TileFamily& B = tile_family(TF_BAND);                                       // plain f16, raw sums: the first legal (bandd) mode
        for (int m = 0; m < B.modes; ++m) if (tile_legal(l, batch, B.base + m)) return B.base + m;
        return B.base + B.f16_from;
    }
    const int64_t gn = (L.cout + 127) / 128;
    const int g = L.cout <= 64 ? HV_128x64 : ((M + 127) / 128) * gn >= 512 ? HV_128x128 : ((M + 63) / 64) * gn >= 512 ? HV_64x128 : HV_64x64;
    return tile_legal(l, batch, g) ? g : HV_128x128_8W;                                   // (host of a fused pointwise conv: one N tile)
}

// Forced id (the tuned table is then ignored), else the tuned entry of this batch; an illegal one silently gives the default.
// Option k_slice_workgroups = 0 and slice panels larger than the scratch (allocated with the weights of every plan that has a
// sliced layer) turn a one-workgroup-per-slice tile into schedule A of the same tile (the same bits).
int Plan::variant_for(const Launch& l, int batch) const {
    int want = opt_force_f16s3_variant;
    if (want < 0) {
        auto it = tuned.find(batch);
        const size_t idx = &l - &launches[0];
        if (it != tuned.end() && idx < it->second.size()) want = it->second[idx];
    }
    int v = want >= 0 && tile_legal(l, batch, want) ? want : default_tile(l, batch);
    if (family_of(v).ks_sched_b() && !(opt_k_slice_workgroups && ks_sched_b_fits(l, batch))) --v;
    return v;
}

// What autotune times for a launch, in screening order: the legal tiles minus those far wider than the layer, the families
// switched off as candidates (options ring_kernel / patch_kernel) and the one-workgroup-per-slice tiles that cannot run as such.
// Narrow, sliced and band layers: their own family in mode order.
std::vector<int> Plan::tile_candidates(const Launch& l, int batch) const {
    static const int kOrder[TF_COUNT] = {TF_GENERIC, TF_PATCH, TF_BAND, TF_PWD, TF_RING, TF_C16, TF_KS};
    const int cout = layers[l.layer].cout;
    const bool ks_b = opt_k_slice_workgroups && ks_sched_b_fits(l, batch);
    std::vector<int> cand;
    for (int f : kOrder) {
        if ((f == TF_RING && !opt_ring_kernel) || (f == TF_PATCH && !opt_patch_kernel)) continue;
        const TileFamily& F = tile_family(f);
        for (int m = 0; m < F.modes; ++m) {
            const int bn = F.info(m).bn;
            const bool too_wide = f == TF_GENERIC || f == TF_RING ? bn > 64 && bn > 2 * ((cout + 63) / 64 * 64)
                                : f == TF_PATCH ? bn > 64 && bn > cout
                                : f == TF_PWD ? bn > 128 && bn > (cout + 127) / 128 * 128 : false;
            if (too_wide || (family_of(F.base + m).ks_sched_b() && !ks_b) || !tile_legal(l, batch, F.base + m)) continue;
            cand.push_back(F.base + m);
        }
    }
    return cand;
}

// Refuses what would compute wrong results (tile_legal's family rules; the caller went through variant_for or tile_candidates)
int Plan::launch_split_variant(ConvArgs& a, const PackedConv& pc, int v, hipStream_t s) const {
    const TileRef t = family_of(v);
    if (!t) { set_error("variant %d is no split-f16 tile", v); return RTOD_E_STATE; }
    if (precision == 2 && !t.f16()) { set_error("variant %d has no plain-f16 instance", v); return RTOD_E_STATE; }
    if (a.raw_out && !t.raw()) { set_error("variant %d has no raw-sum instance", v); return RTOD_E_STATE; }
    if (pc.narrow != t.is(TF_C16)) {
        set_error(pc.narrow ? "variant %d requested for a narrow (Cin = 16) layer" : "narrow variant %d requested for a layer without tap-major weights", v);
        return RTOD_E_STATE;
    }
    if ((pc.ks_chunks > 0) != t.is(TF_KS)) {
        set_error(pc.ks_chunks > 0 ? "variant %d requested for a K-sliced layer" : "K-sliced variant %d requested for a layer that is not sliced", v);
        return RTOD_E_STATE;
    }
    if (pc.band != t.is(TF_BAND) && !(t.bandd_wide() && !pc.band)) {
        set_error(pc.band ? "variant %d requested for a band layer" : "band variant %d requested for a layer without band weights", v);
        return RTOD_E_STATE;
    }
    if (t.is(TF_KS)) {
        a.slice_chunks = pc.ks_chunks;
        a.partial = nullptr; a.partial_floats = 0;
        if (t.ks_sched_b()) { a.partial = d_scratch; a.partial_floats = scratch_floats; }     // one workgroup per (tile, slice)
    }
    return t.fam->launch(a, t.mode, s);
}

int Plan::build_conv_args(const Launch& l, int batch, float* out, ConvArgs& a) const {
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
    if (l.pw_guest >= 0 && pw_active()) {
        const Launch& g = launches[l.pw_guest];
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

// Autotune: at the first forward of a batch size every distinct split-f16 conv shape times each tile variant /
// kernel on the device (1 warm-up, the minimum of 3 timed pairs as a screen, then the three fastest re-timed interleaved; HIP events on `s`)
// and remembers the fastest.
// It runs INSIDE that forward, layer by layer, so each candidate sees the layer's real input (timing on a zeroed
// arena ranks kernels differently: zero operands change the clock the chip holds).  Tile choice interacts with the
// 256-CU round structure (a 722-block grid on 512 resident slots runs two rounds at 70 % efficiency) in ways a
// closed-form heuristic keeps getting wrong; measuring costs ~0.3 s once per batch size.
static std::mutex g_tune_mutex;
static std::map<std::vector<int>, int> g_tune_memo;

int Plan::tune_launch(size_t li, ConvArgs& a, int batch, hipStream_t s) {
    const Launch& l = launches[li];
    const Layer& L = layers[l.layer];
    const bool pw = a.pw_wh != nullptr;
    // shape + everything else the candidate set depends on (a second plan with other kernel-selection options must not inherit tiles)
    // (the precision too: an f16 plan must not inherit an f16s3 plan's tile, or the reverse; and the input geometry hin / win / pad:
    // two layers with the same output shape but another input extent or padding are other problems, e.g. across rectangular plans)
    const std::vector<int> key = {L.cin, L.cout, L.size, L.stride, L.hout, L.wout, l.in2_layer >= 0, l.out_layer == -2, pw ? a.pw_cout : 0,
                                  convs[l.conv_slot].band ? 1 : 0, opt_ring_kernel ? 1 : 0, opt_patch_kernel ? 1 : 0, opt_pwd_kernel ? 1 : 0, L.act,
                                  precision, L.hin, L.win, L.pad, convs[l.conv_slot].ks_chunks, opt_k_slice_workgroups ? 1 : 0,
                                  a.raw_out ? 1 : 0};      // (a raw-sum launch times other kernels over another candidate set: never an eval plan's id)
    auto it = tune_cache.find(key);
    if (it != tune_cache.end()) { tuning[li] = it->second; return RTOD_OK; }
    // process-wide memo (device, batch, shape): a second plan of the same network (bench.py keeps two batches in flight)
    // reuses the first one's measurements instead of re-timing every candidate
    std::vector<int> gkey = key; gkey.push_back(device); gkey.push_back(batch);
    {
        std::lock_guard<std::mutex> lock(g_tune_mutex);
        auto git = g_tune_memo.find(gkey);
        if (git != g_tune_memo.end()) { tuning[li] = git->second; tune_cache[key] = git->second; return RTOD_OK; }
    }
    hipEvent_t e0, e1;
    RTOD_HIP(hipEventCreate(&e0)); RTOD_HIP(hipEventCreate(&e1));
    const std::vector<int> cand = tile_candidates(l, batch);
    int best_v = variant_for(l, batch);
    int rc = RTOD_OK;
    // min over `reps` timed groups of `per` back-to-back launches
    auto time_variant = [&](int v, int reps, int per, float& out_ms) -> int {
        out_ms = 1e30f;
        for (int rep = 0; rep < reps; ++rep) {
            (void)hipEventRecord(e0, s);
            for (int r = 0; r < per; ++r) { const int q = launch_split_variant(a, convs[l.conv_slot], v, s); if (q) return q; }
            (void)hipEventRecord(e1, s);
            if (hipEventSynchronize(e1) != hipSuccess) return hip_fail(hipGetLastError(), "autotune sync");
            float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
            out_ms = std::min(out_ms, ms / per);
        }
        return RTOD_OK;
    };
    std::vector<std::pair<float, int>> ranked;
    for (int v : cand) {
        rc = launch_split_variant(a, convs[l.conv_slot], v, s);                       // warm-up
        if (rc) break;
        float ms; rc = time_variant(v, 3, 2, ms);
        if (rc) break;
        ranked.push_back({ms, v});
    }
    if (!rc && !ranked.empty()) {
        // the screen's spread between neighbours is within its noise: re-time the three fastest, interleaved
        std::sort(ranked.begin(), ranked.end());
        const size_t top = std::min<size_t>(3, ranked.size());
        std::vector<float> fin(top, 1e30f);
        for (int round = 0; round < 5 && !rc; ++round)                                 // (five rounds: the top three usually sit within 1-2 % of one another)
            for (size_t t = 0; t < top && !rc; ++t) {
                float ms; rc = time_variant(ranked[t].second, 2, 4, ms);
                fin[t] = std::min(fin[t], ms);
            }
        if (!rc) best_v = ranked[std::min_element(fin.begin(), fin.end()) - fin.begin()].second;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc) return rc;
    tuning[li] = best_v;
    tune_cache[key] = best_v;
    { std::lock_guard<std::mutex> lock(g_tune_mutex); g_tune_memo[gkey] = best_v; }
    return RTOD_OK;
}

int Plan::set_tiles(int batch, const int* variants, int count) {
    if (!variants || count != (int)launches.size() || batch <= 0 || batch > max_batch) { set_error("set_tiles: %d entries for %d launches, batch %d", count, (int)launches.size(), batch); return RTOD_E_ARG; }
    if (precision < 1) { set_error("set_tiles: split-f16 / f16 plans only"); return RTOD_E_STATE; }
    for (int i = 0; i < count; ++i) {
        const int v = variants[i];
        const Launch& l = launches[i];
        if (v < 0) continue;
        if (l.kind != LK_CONV || l.conv_slot < 0 || !convs[l.conv_slot].split) { set_error("set_tiles: launch %d is not a split-f16 convolution", i); return RTOD_E_ARG; }
        if (!tile_legal(l, batch, v)) { set_error("set_tiles: variant %d is not a valid tile of launch %d (layer %d)", v, i, l.layer); return RTOD_E_ARG; }
        if (family_of(v).ks_sched_b() && !ks_sched_b_fits(l, batch)) {
            set_error("set_tiles: variant %d (one workgroup per K slice) of launch %d (layer %d) needs more slice scratch than the plan has at batch %d", v, i, l.layer, batch);
            return RTOD_E_ARG;
        }
    }
    tuned[batch] = std::vector<int>(variants, variants + count);
    return RTOD_OK;
}

// Sliced split layers (option k_slices_split, conv_ks_f16s3.hip).  The slice panels [S][M][Npad] of schedule B fit the scratch:
bool Plan::ks_sched_b_fits(const Launch& l, int batch) const {
    const PackedConv& pc = convs[l.conv_slot];
    if (pc.ks_chunks <= 0) return false;
    const Layer& L = layers[l.layer];
    const int64_t S = (pc.Kpad / 32 + pc.ks_chunks - 1) / pc.ks_chunks;
    return S * batch * L.hout * L.wout * pc.Npad <= KS_SCRATCH_FLOATS;
}
// fp32 view over the raw-sum scratch for the conv of launch `l` at this batch: rows of raw_stride floats (base null: no scratch / too small)
View Plan::bn_raw_view(const Launch& l, int batch) const {
    View v;
    const Layer& L = layers[l.layer];
    const PackedConv& pc = convs[l.conv_slot];
    if (!d_bn_raw || (int64_t)batch * L.hout * L.wout * raw_stride(pc) > bn_raw_floats) return v;
    v.base = d_bn_raw; v.ldc = raw_stride(pc); v.coff = 0; v.C = L.cout; v.H = L.hout; v.W = L.wout;
    return v;
}
bool Plan::pw_active() const { return precision == 1 && opt_fuse_pointwise && !bn_split_active(); }
bool Plan::stem_pool_fused() const { return precision >= 1 && stem_pool_pattern && !keep_all && convs[launches[0].conv_slot].stem16; }
bool Plan::bn_pool_fused(int layer) const { return bn_narrow_active() && opt_fuse_bn_pool && !keep_all && layers[layer].bn_pool >= 0; }
bool Plan::stem2_active() const { return precision == 1 && !bn_split_active() && opt_stem2_kernel && stem2_pattern && !keep_all && convs[launches[0].conv_slot].split; }

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
        int rc = RTOD_OK;
        switch (l.kind) {
            case LK_PACK: {
                View v = view_of(-1);
                rc = launch_pack_input(x, batch, 3, height, width, v.base, 4, s);
                break;
            }
            case LK_CONV: {
                const Layer& L = layers[l.layer];
                const PackedConv& pc = convs[l.conv_slot];
                if (l.pw_host >= 0 && pw_active()) break;           // runs in the host conv's epilogue
                ConvArgs a;
                rc = build_conv_args(l, batch, out, a);
                if (rc) return rc;
                if (!pc.split) {
                    const int v = choose_variant(L, batch);
                    const int mode = f32_slice_mode(l, batch, v);
                    a.slice_chunks = mode ? pc.slice_chunks : 0;
                    if (mode == 2) { a.partial = d_scratch; a.partial_floats = scratch_floats; }
                    if (opt_bn_batch_stats && L.bn) {            // raw conv, then statistics + normalise + activation + shortcut in place
                        if (a.dec.enabled || (a.out_split && !bn_split_active()) || !d_bn_stats || pc.stats_off < 0) { set_error("forward: layer %d: batch-statistics BatchNorm on an unsupported launch", l.layer); return RTOD_E_STATE; }
                        a.leaky = 0; a.res = nullptr;
                        const View o = view_of(l.out_layer);
                        View r; if (l.in2_layer >= 0) r = view_of(l.in2_layer);
                        if (a.out_split) {                           // split plan (option bn_batch_split), layer 0: raw sums to the scratch, normalised into the split format
                            const View rv = bn_raw_view(l, batch);
                            if (!rv.base) { set_error("forward: layer %d: no raw-sum scratch", l.layer); return RTOD_E_STATE; }
                            a.out = rv.base; a.out_ldc = rv.ldc; a.out_coff = 0; a.out_split = 0;
                            rc = launch_conv(a, v, s);
                            if (rc) return rc;
                            const bool pool = bn_pool_fused(l.layer);      // normalise + the max-pool that follows, into the pool's view
                            rc = launch_bn_batch_split(rv, pool ? view_of(L.bn_pool) : o, l.in2_layer >= 0 ? &r : nullptr, batch, d_bn_stats + pc.stats_off, pc.Npad, d_weights + pc.bn_off, pc.Npad, L.act,
                                                       d_bn_partial, bn_partial_count, overflow_flag, s, pool ? 1 : 0);
                            break;
                        }
                        rc = launch_conv(a, v, s);
                        if (rc) return rc;
                        rc = launch_bn_batch(o, o, l.in2_layer >= 0 ? &r : nullptr, batch, d_bn_stats + pc.stats_off, pc.Npad, d_weights + pc.bn_off, pc.Npad, L.act, d_bn_partial, bn_partial_count, s);
                    } else
                    rc = launch_conv(a, v, s);
                }
                else if (li == 1 && stem2_active()) {                  // stem + this conv (+ its hosted 1x1) in one kernel
                    const PackedConv& p0 = convs[launches[0].conv_slot];
                    if (!(l.pw_guest >= 0 && pw_active())) { a.pw_wh = nullptr; a.pw_wl = nullptr; }
                    rc = launch_conv_stem2_f16s3(x, batch, height, width, reinterpret_cast<const _Float16*>(d_weights + p0.w_off),
                                                 reinterpret_cast<const _Float16*>(d_weights + p0.wl_off), d_weights + p0.s_off, d_weights + p0.b_off,
                                                 layers[0].act, a, s);
                } else {
                    const bool raw = raw_launch(l);            // BatchNorm conv of a batch-statistics split plan: raw sums, statistics, normalise (+ activation + shortcut)
                    View rv;
                    if (raw) {
                        rv = bn_raw_view(l, batch);
                        if (!rv.base || a.dec.enabled || a.pw_wh || !d_bn_stats || pc.stats_off < 0) { set_error("forward: layer %d: batch-statistics BatchNorm on an unsupported launch", l.layer); return RTOD_E_STATE; }
                        a.raw_out = rv.base; a.raw_ld = (int)rv.ldc; a.res = nullptr; a.leaky = 0;
                    }
                    if (tune_now) { rc = tune_launch(li, a, batch, s); if (rc) return rc; }      // (never reached for the fused stem launch)
                    rc = launch_split_variant(a, pc, tune_now && tuning[li] >= 0 ? tuning[li] : variant_for(l, batch), s);
                    if (!rc && raw) {
                        View r; if (l.in2_layer >= 0) r = view_of(l.in2_layer);
                        const bool pool = bn_pool_fused(l.layer);
                        rc = launch_bn_batch_split(rv, view_of(pool ? L.bn_pool : l.out_layer), l.in2_layer >= 0 ? &r : nullptr, batch, d_bn_stats + pc.stats_off, pc.Npad, d_weights + pc.bn_off, pc.Npad,
                                                   L.act, d_bn_partial, bn_partial_count, overflow_flag, s, pool ? 1 : 0);
                    }
                }
                break;
            }
            case LK_STEM: {
                if (stem2_active()) break;                              // computed inside layer 1's kernel
                const Layer& L = layers[l.layer];
                const PackedConv& pc = convs[l.conv_slot];
                const View o = view_of(l.out_layer);
                if (pc.stem16) {                                        // 16 filters: stand-alone, or with layer 1's max-pool (writes layer 1's view)
                    if (!pc.split) { set_error("forward: the 16-filter stem needs a split-f16 / f16 plan"); return RTOD_E_STATE; }
                    if (bn_split_active() && L.bn) {                    // raw sums (unfolded weights), statistics, normalise (+ the max-pool that follows)
                        const View rv = bn_raw_view(l, batch);
                        if (!rv.base || !d_bn_stats || pc.stats_off < 0 || !opt_bn_split_narrow) { set_error("forward: layer %d: batch-statistics BatchNorm on an unsupported launch", l.layer); return RTOD_E_STATE; }
                        rc = launch_conv_stem16_raw(x, reinterpret_cast<const _Float16*>(d_weights + pc.w_off), reinterpret_cast<const _Float16*>(d_weights + pc.wl_off),
                                                    d_weights + pc.s_off, rv, batch, height, width, s);
                        if (rc) return rc;
                        const bool fuse = bn_pool_fused(l.layer);
                        rc = launch_bn_batch_split(rv, fuse ? view_of(L.bn_pool) : o, nullptr, batch, d_bn_stats + pc.stats_off, pc.Npad, d_weights + pc.bn_off, pc.Npad, L.act,
                                                   d_bn_partial, bn_partial_count, overflow_flag, s, fuse ? 1 : 0);
                        break;
                    }
                    const bool pool = stem_pool_fused();
                    rc = launch_conv_stem16_f16s3(x, reinterpret_cast<const _Float16*>(d_weights + pc.w_off), reinterpret_cast<const _Float16*>(d_weights + pc.wl_off),
                                                  d_weights + pc.s_off, d_weights + pc.b_off, pool ? view_of(1) : o, batch, height, width, L.act, pool ? 1 : 0, overflow_flag, s);
                }
                else if (pc.split)
                    rc = launch_conv_stem_split(x, reinterpret_cast<const _Float16*>(d_weights + pc.w_off), reinterpret_cast<const _Float16*>(d_weights + pc.wl_off),
                                                d_weights + pc.s_off, d_weights + pc.b_off, o, batch, height, width, L.hout, L.wout,
                                                L.stride, L.cout, L.act, overflow_flag, s);
                else
                    rc = launch_conv_stem(x, d_weights + pc.w_off, d_weights + pc.b_off, o, batch, height, width, L.hout, L.wout,
                                          L.stride, L.cout, L.act, s);
                break;
            }
            case LK_UPSAMPLE:
                rc = layers[l.layer].nearest ? launch_upsample_nearest2x(view_of(l.in_layer), view_of(l.out_layer), batch, s)
                                             : launch_upsample2x(view_of(l.in_layer), view_of(l.out_layer), batch, s);
                break;
            case LK_MAXPOOL:
                if (li == 1 && stem_pool_fused()) break;                // computed inside the stem's kernel
                if (pool_fused_away(l.layer)) break;                    // ... inside the conv's normalise kernel
                rc = launch_maxpool(view_of(l.in_layer), view_of(l.out_layer), batch, layers[l.layer].size, layers[l.layer].stride, layers[l.layer].pool_pad, s); break;
            case LK_ADD: rc = launch_add(view_of(l.in_layer), view_of(l.in2_layer), view_of(l.out_layer), batch, s); break;
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

void Plan::fill_launch_info(int idx, rtod_launch_info* o, int batch) const {
    memset(o, 0, sizeof(*o));
    const Launch& l = launches[idx];
    o->layer = l.layer; o->kind = l.kind; o->variant = -1;
    if (l.kind == LK_PACK) { o->bytes_per_frame = (int64_t)height * width * (3 + 4) * 4; return; }
    const Layer& L = layers[l.layer];
    o->ksize = L.size; o->stride = L.stride; o->cin = L.cin; o->cout = L.cout; o->hout = L.hout; o->wout = L.wout;
    const int64_t in_b = (int64_t)L.hin * L.win * L.cin * 4, out_b = (int64_t)L.hout * L.wout * L.cout * 4;
    switch (l.kind) {
        case LK_STEM:
            if (stem2_active()) { o->bytes_per_frame = 0; break; }                   // accounted on layer 1's launch
            o->flops_per_frame = 2ll * L.hout * L.wout * L.cout * L.cin * L.size * L.size;
            o->bytes_per_frame = in_b + (stem_pool_fused() || bn_pool_fused(l.layer) ? out_b / 4 : out_b);  // fused 2x2 pool: the pooled map is what is written
            o->weight_bytes = ((int64_t)L.cout * L.cin * L.size * L.size + L.cout) * 4;
            break;
        case LK_MAXPOOL:
            o->bytes_per_frame = (idx == 1 && stem_pool_fused()) || pool_fused_away(l.layer) ? 0 : in_b + out_b;   // fused: accounted on the stem's / conv's launch
            break;
        case LK_CONV:
            if (l.pw_host >= 0 && pw_active()) { o->bytes_per_frame = 0; break; }    // accounted on the host conv's launch
            if (convs[l.conv_slot].split) o->variant = 100 + variant_for(l, batch);
            else { const int v = choose_variant(L, batch); o->variant = v + 10 * f32_slice_mode(l, batch, v); }   // tile + 10 * K-slice schedule
            o->flops_per_frame = 2ll * L.hout * L.wout * L.cout * L.cin * L.size * L.size;
            o->fused_residual = l.in2_layer >= 0; o->fused_decode = l.out_layer == -2;
            o->bytes_per_frame = in_b + (bn_pool_fused(l.layer) ? out_b / 4 : out_b) + (l.in2_layer >= 0 ? out_b : 0);   // (fused 2x2 pool: the pooled map is what is written)
            o->weight_bytes = ((int64_t)L.cout * L.cin * L.size * L.size + L.cout) * 4;
            if (idx == 1 && stem2_active()) {                                        // fused stem: its FLOPs ride here, its output is never written
                const Layer& S = layers[0];
                o->variant = 100 + STEM2_VARIANT;
                o->flops_per_frame += 2ll * S.hout * S.wout * S.cout * S.cin * S.size * S.size;
                o->bytes_per_frame = (int64_t)S.hin * S.win * S.cin * 4 + out_b;
                o->weight_bytes += ((int64_t)S.cout * S.cin * S.size * S.size + S.cout) * 4;
            }
            if (l.pw_guest >= 0 && pw_active()) {
                const Layer& G = layers[launches[l.pw_guest].layer];
                o->fused_pointwise = 1;
                o->flops_per_frame += 2ll * G.hout * G.wout * G.cout * G.cin;
                o->bytes_per_frame += (int64_t)G.hout * G.wout * G.cout * 4;
                o->weight_bytes += ((int64_t)G.cout * G.cin + G.cout) * 4;
            }
            break;
        case LK_ADD: o->bytes_per_frame = 3 * out_b; break;
        default: o->bytes_per_frame = in_b + out_b; break;
    }
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
           << ",\"stride\":" << L.stride << ",\"pad\":" << L.pad << ",\"bn\":" << (L.bn ? "true" : "false") << ",\"leaky\":" << (L.leaky ? "true" : "false") << ",\"act\":" << L.act << ",\"decode_v5\":" << (L.decode_v5 ? "true" : "false") << ",\"nearest\":" << (L.nearest ? "true" : "false") << ",\"pool_pad\":" << L.pool_pad
           << ",\"srcs\":[";
        for (size_t s = 0; s < L.srcs.size(); ++s) os << (s ? "," : "") << L.srcs[s];
        os << "],\"anchors\":[";
        for (size_t a = 0; a < L.anchors.size(); ++a) os << (a ? "," : "") << "[" << L.anchors[a].first << "," << L.anchors[a].second << "]";
        os << "],\"classes\":" << L.classes << ",\"row_offset\":" << L.row_offset << ",\"rows\":" << L.rows << ",\"w_off\":" << L.w_off
           << ",\"fused_into\":" << ((i == 0 && (stem2_active() || stem_pool_fused())) ? 1 : bn_pool_fused((int)i) ? L.bn_pool : L.fused_into) << ",\"fused_away\":" << (L.fused_away ? "true" : "false") << ",\"alias_of\":" << L.alias_of
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
    os << "}";
    return os.str();
}

}  // namespace rtod
