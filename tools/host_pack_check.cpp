// Host-only check of the pieces the training path shares between host and device, meant to be built with the host sanitisers and
// run on the CPU (no GPU, no Python):
//   * f16_round.h: f32_to_f16_rn on the boundary inputs against the outputs of the host routine it replaced (the table below), and
//     f16_to_f32 of all 65536 halves against that routine's ldexp form;
//   * the slice rule of wgrad.hip (wgrad_schedule for its three rules, wgrad_check_shape, wgrad_workspace_bytes) on the shapes of the GPU tests;
//   * Plan::pack_conv through rtod_plan_pack_weights: the cfg given as argv[1] (cfgs.mini_cfg(64, 64) written to a file) packed
//     for the three precisions from a seeded weight stream.
// Build (from realtimeobjectdetection_amd/csrc, after `make`; SAN = -Xarch_host -fsanitize=address,undefined):
//   for f in capi plan_cfg plan_build plan_weights plan_tiles plan_forward split_tiles; do hipcc $CXXFLAGS $SAN -x hip -c $f.cpp -o san_$f.o; done
//   hipcc $CXXFLAGS $SAN -c wgrad.hip -o san_wgrad.o
//   hipcc $CXXFLAGS $SAN -x hip -c ../../tools/host_pack_check.cpp -o san_main.o
//   hipcc --offload-arch=gfx950 $SAN -o host_pack_check san_*.o <every other object of the Makefile's OBJS>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <vector>

#include "../realtimeobjectdetection_amd/csrc/f16_round.h"
#include "../realtimeobjectdetection_amd/csrc/rtod_internal.h"

using namespace rtod;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++fails; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

// the host routine before the merge (plan_weights.cpp), kept here as the reference of f16_to_f32
static float f16_to_f32_ldexp(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const int e = (h >> 10) & 0x1F; const uint32_t m = h & 0x3FFu;
    float v;
    if (e == 0) v = std::ldexp((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = std::ldexp((float)(m | 0x400u), e - 25);
    uint32_t x; memcpy(&x, &v, 4); x |= sign; memcpy(&v, &x, 4);
    return v;
}

int main(int argc, char** argv) {
    // f32 bits -> the half the earlier host routine gave
    static const struct { uint32_t in; uint16_t out; } table[] = {
        {0x33000000u, 0x0000}, {0x33000001u, 0x0001}, {0x387FFFFFu, 0x0400}, {0x38800000u, 0x0400}, {0x477FEFFFu, 0x7BFF}, {0x477FF000u, 0x7C00},
        {0xB3000000u, 0x8000}, {0xB3000001u, 0x8001}, {0xB87FFFFFu, 0x8400}, {0xB8800000u, 0x8400}, {0xC77FEFFFu, 0xFBFF}, {0xC77FF000u, 0xFC00},
        {0x7F800000u, 0x7C00}, {0xFF800000u, 0xFC00}, {0x7FC00000u, 0x7E00}, {0xFFC00001u, 0xFE00}, {0x7F800001u, 0x7E00},
        {0x00000000u, 0x0000}, {0x80000000u, 0x8000}, {0x00000001u, 0x0000}, {0x3F800000u, 0x3C00}, {0x3F801000u, 0x3C00}, {0x3F803000u, 0x3C02},
        {0x33800000u, 0x0001}, {0x33C00000u, 0x0002}, {0x387FC000u, 0x03FF}, {0x387FE000u, 0x0400},
    };
    for (const auto& t : table) {
        const uint16_t got = f32_to_f16_rn(f32_from_bits(t.in));
        CHECK(got == t.out, "f32_to_f16_rn(0x%08X) = 0x%04X, the table has 0x%04X", t.in, got, t.out);
    }
    for (uint32_t h = 0; h < 65536; ++h) {
        const uint32_t got = f32_bits(f16_to_f32((uint16_t)h)), want = f32_bits(f16_to_f32_ldexp((uint16_t)h));
        CHECK(got == want, "f16_to_f32(0x%04X) = 0x%08X, the ldexp form gives 0x%08X", h, got, want);
        if (((h >> 10) & 0x1F) != 31) CHECK(f32_to_f16_rn(f16_to_f32((uint16_t)h)) == h, "half 0x%04X does not survive the round trip", h);
    }

    // the slice rule on (B, Cout, Cin, H, W, size): S <= cap, the slices cover K, the workspace holds S partial dW and db
    static const int shapes[][6] = {{2, 18, 32, 2, 2, 1}, {3, 255, 96, 13, 13, 1}, {1, 64, 64, 127, 1, 1}, {2, 256, 928, 4, 4, 3}, {3, 255, 96, 13, 13, 3},
                                    {1, 1, 32, 1, 1, 3}, {8, 1024, 512, 13, 13, 3}, {1, 64, 64, 16, 8, 3}};
    for (const auto& s : shapes) {
        const int64_t K = (int64_t)s[0] * s[3] * s[4];
        for (WgradRule rule : {WGRAD_HEAD, WGRAD_TILED}) {
            const WgradSchedule sc = wgrad_schedule(rule, s[0], s[1], s[2], s[3], s[4], s[5], 1);
            const int64_t L = sc.slice_len, S = sc.slices;
            CHECK(sc.K == K && L % 8 == 0 && S >= 1 && S <= WGRAD_MAX_SLICES && S * L >= K && (S - 1) * L < K && sc.group == S && sc.tm == 64 && sc.tn == 64 && sc.db,
                  "slice rule %d: K %lld L %lld S %lld", (int)rule, (long long)K, (long long)L, (long long)S);
            CHECK(wgrad_workspace_bytes(sc, s[1], s[2], s[5]) == 4u * (size_t)S * ((size_t)s[1] * s[2] * s[5] * s[5] + s[1]), "workspace bytes");
            CHECK(wgrad_check_shape("check", rule, s[0], s[1], s[2], s[3], s[4], s[5], 1) == RTOD_OK, "shape refused");
        }
    }
    auto slices = [](WgradRule rule, int b, int cout, int cin, int h, int w, int size, int stride = 1) { return wgrad_schedule(rule, b, cout, cin, h, w, size, stride).slices; };
    // the tile cap: 524 tiles -> 2, 1 tile -> 16, 1152 tiles -> 1; the head rule does not see the tiles; stride 2: K of the output map
    CHECK(slices(WGRAD_TILED, 8, 256, 928, 13, 13, 3) == 2 && slices(WGRAD_TILED, 8, 64, 64, 13, 13, 1) == 16 && slices(WGRAD_TILED, 8, 1024, 512, 13, 13, 3) == 1 &&
          slices(WGRAD_HEAD, 8, 1024, 512, 13, 13, 1) == 16, "tile caps");
    CHECK(wgrad_schedule(WGRAD_TILED, 2, 64, 32, 13, 15, 3, 2).K == 2 * 7 * 8, "stride-2 K");
    CHECK(wgrad_check_shape("check", WGRAD_TILED, 1, 1, 16, 1, 1, 1, 1) == RTOD_E_ARG && wgrad_check_shape("check", WGRAD_TILED, 1, 1, 32, 1, 1, 2, 1) == RTOD_E_ARG &&
          wgrad_check_shape("check", WGRAD_TILED, 1, 1, 32, 4, 4, 1, 2) == RTOD_E_ARG && wgrad_check_shape("check", WGRAD_THIN, 1, 1, 0, 1, 1, 3, 1) == RTOD_E_ARG, "bad shapes accepted");
    // the thin rule on (B, Cout, Cin, H, W, size) -> (S, L): tests/test_train_bits_gpu.py's THIN_TREE_SHAPES, and layer 0 of YOLOv3-tiny at 416 x 416 batch 8
    static const int thin[][8] = {{1, 16, 3, 129, 130, 3, 66, 256}, {2, 40, 16, 96, 96, 3, 72, 256}, {1, 97, 16, 160, 240, 3, 127, 304}, {1, 1, 1, 1025, 1024, 1, 1025, 1024},
                                  {8, 16, 3, 416, 416, 3, 1352, 1024}, {1, 1, 1, 1, 1, 3, 1, 256}};
    for (const auto& s : thin) {
        const WgradSchedule sc = wgrad_schedule(WGRAD_THIN, s[0], s[1], s[2], s[3], s[4], s[5], 1);
        CHECK(wgrad_check_shape("check", WGRAD_THIN, s[0], s[1], s[2], s[3], s[4], s[5], 1) == RTOD_OK, "thin shape refused");
        CHECK(sc.slices == s[6] && sc.slice_len == s[7] && sc.group == WGRAD_THIN_GROUP && sc.tm == 32 && sc.tn == 128 && !sc.db, "thin rule: S %d L %d", sc.slices, sc.slice_len);
        CHECK(wgrad_workspace_bytes(sc, s[1], s[2], s[5]) == 4u * (size_t)s[6] * s[1] * s[2] * s[5] * s[5], "thin workspace bytes");
    }

    // pack the cfg's weights on the host for every precision
    if (argc > 1) {
        std::ifstream f(argv[1]);
        std::stringstream ss; ss << f.rdbuf();
        const std::string cfg = ss.str();
        CHECK(!cfg.empty(), "cannot read %s", argv[1]);
        for (int mode = 0; mode < 3 && !cfg.empty(); ++mode) {
            rtod_plan* plan = nullptr;
            CHECK(rtod_plan_create(cfg.data(), cfg.size(), 64, 64, 2, 0, &plan) == RTOD_OK, "plan_create");
            if (!plan) break;
            CHECK(rtod_plan_set_precision(plan, mode) == RTOD_OK, "set_precision %d", mode);
            rtod_plan_info info;
            CHECK(rtod_plan_get_info(plan, &info) == RTOD_OK, "get_info");
            std::vector<float> w((size_t)info.n_weight_floats);
            uint32_t lcg = 12345u + mode;
            for (auto& v : w) { lcg = lcg * 1664525u + 1013904223u; v = ((lcg >> 8) * (1.0f / 8388608.0f) - 1.0f) * ((lcg & 0xFF) < 8 ? 1e-6f : 0.5f); }
            for (size_t i = 0; i < w.size(); i += 97) w[i] = std::fabs(w[i]);      // (a stream position may be a variance; a negative one only yields NaN)
            size_t need = 0;
            CHECK(rtod_plan_pack_weights(plan, w.data(), w.size(), nullptr, 0, &need) == RTOD_OK && need > 0, "pack_weights size");
            std::vector<float> image(need);
            CHECK(rtod_plan_pack_weights(plan, w.data(), w.size(), image.data(), image.size(), nullptr) == RTOD_OK, "pack_weights");
            uint32_t sum = 0;
            for (float v : image) sum = sum * 31u + f32_bits(v);
            printf("precision %d: %lld stream floats -> %zu image floats, checksum %08x\n", mode, (long long)info.n_weight_floats, need, sum);
            rtod_plan_destroy(plan);
        }
    }
    printf(fails ? "%d check(s) FAILED\n" : "host pack check ok\n", fails);
    return fails ? 1 : 0;
}
