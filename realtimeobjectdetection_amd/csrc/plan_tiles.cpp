// Which kernel variant a conv launch runs: the exact-fp32 tiles, the split-f16 tile rules, autotune.
#include "plan.h"

#include <algorithm>
#include <mutex>

namespace rtod {

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

// Which tile a split-f16 conv launch runs is decided here and nowhere else: tile_legal (may it?), default_tile (the closed-form
// choice), variant_for (forced / tuned / default), tile_candidates (what autotune times); ids resolve through family_of
// (split_tiles.cpp).
//
// May launch `l` run tile `v` and give this layer's defined bits?  Does not depend on the batch; a one-workgroup-per-slice tile
// whose panels do not fit the scratch is legal here: variant_for runs schedule A of the same tile (same bits), set_tiles refuses it.
// Plain-f16 plans (precision 2) run the tiles that have an f16 instance (the f16 column of the family table): the generic, bandd
// (band layers, and the wide tile of the other 3x3 stride-1 layers), 1x1 slab, narrow and K-sliced tiles; never conv_band / ring /
// patch, and no hosted pointwise epilogue (LaunchForm::guest).
// A BatchNorm conv of a batch-statistics split plan (raw_launch) runs the tiles with a raw-sum instance (the raw column) that its
// family rules admit; for layers that are neither narrow nor sliced that is the set of a plain-f16 plan.
bool Plan::tile_legal(const Launch& l, int v) const {
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
    const bool hosts_pw = form(&l - &launches[0]).guest >= 0, plain = l.out_layer != -2 && !hosts_pw, same_map = L.hout == L.hin && L.wout == L.win;
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
        for (int m = 0; m < B.modes; ++m) if (tile_legal(l, B.base + m)) return B.base + m;
        return B.base + B.f16_from;
    }
    const int64_t gn = (L.cout + 127) / 128;
    const int g = L.cout <= 64 ? HV_128x64 : ((M + 127) / 128) * gn >= 512 ? HV_128x128 : ((M + 63) / 64) * gn >= 512 ? HV_64x128 : HV_64x64;
    return tile_legal(l, g) ? g : HV_128x128_8W;                                   // (host of a fused pointwise conv: one N tile)
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
    int v = want >= 0 && tile_legal(l, want) ? want : default_tile(l, batch);
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
            if (too_wide || (family_of(F.base + m).ks_sched_b() && !ks_b) || !tile_legal(l, F.base + m)) continue;
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
        if (!tile_legal(l, v)) { set_error("set_tiles: variant %d is not a valid tile of launch %d (layer %d)", v, i, l.layer); return RTOD_E_ARG; }
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

}  // namespace rtod
