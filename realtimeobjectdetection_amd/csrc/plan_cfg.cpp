// The cfg text -> the layer list with resolved shapes.  Host only: no HIP call in this file.  Behavioural sources in the reference
// (file:line into /root/reference): cfg grammar src/darknet.py:428-447; channel bookkeeping and module semantics
// src/darknet.py:449-603.
#include "plan.h"

#include <cctype>
#include <cstdlib>

namespace rtod {

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
            L.act = act->second == "leaky" ? 1 : (act->second == "silu" || act->second == "swish") ? 2 : 0;    // silu: cfg extension
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

}  // namespace rtod
