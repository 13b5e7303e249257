// 3x3 / pad 1 convolution over 2-D output tiles with an LDS-resident input patch (split-precision f16 MFMA), gfx950.
//
// Same contract, formats, K order and arithmetic as conv_igemm_f16s3.hip / conv_ring_f16s3.hip (reference: conv -> BN(eval)
// -> leaky, src/darknet.py:467-501; shortcut 263-268) — bit-identical results — for the 3x3 layers whose images are too wide
// for the band kernel (conv_band_f16s3.hip stages BM + 2W + 2 input pixels per tile: 5.8x the tile at W = 304).  On the
// per-tap gathering kernels those layers re-read every input pixel once per tap from L2 (9 x 95 MB for YOLOv3's layer 3 at
// 608x608 batch 8, 9 x 47 MB for layers 7 / 10: as much time as the layer's whole HBM traffic) and are bound by exactly that.
//
// A workgroup owns an 8 x 16 block of output pixels of one image and BN output channels.  Per 32-channel chunk it holds the
// 10 x 18 input pixels that block can touch (1.4x the tile; out-of-image pixels are zeros IN the patch, so no per-tap
// validity logic exists) in LDS; the A fragment of output row ty for tap (ky, kx) is patch rows (ty + ky) * 18 + kx + 0..15:
// a constant shift per tap, like the band kernel's.  Patches are double-buffered and arrive by LDS-DMA one chunk ahead;
// weights stream through an LDS-DMA ring of (chunk, tap) stages; the workgroup is persistent and both streams run across
// tile boundaries (conv_ring_f16s3.hip's scheme), the epilogue works straight from the accumulators (transposed product,
// conv_f16s3_common.h) with no barrier, so tile t+1's loads and first steps overlap tile t's stores.
#include "conv_f16s3_common.h"
#include <cstdio>

namespace rtod {

constexpr int PT_TH = 8, PT_TW = 16, PT_BM = PT_TH * PT_TW;            // output tile: 8 rows x 16 columns
constexpr int PT_PR = PT_TH + 2, PT_PC = PT_TW + 2, PT_PE = PT_PR * PT_PC;   // stride-1 patch: 10 x 18 = 180 input pixels
constexpr int PT_PROWS = (PT_PE + 15) / 16 * 16;                        // LDS rows per plane (192: the tail rows hold zeros)
constexpr int PT_PLANE = PT_PROWS * 64;                                 // bytes of one plane of one patch

// LDS: [2 patch buffers][hi plane | lo plane][192 rows x 64 B], then [STAGES][hi BN x 64 B | lo BN x 64 B] weight stages.
template <int BN, int NWM, int NWN, int STAGES, int MINW, int EPI>
__global__ __launch_bounds__(NWM * NWN * 64, MINW)
void conv_patch_f16s3_kernel(const ConvArgs a, const int tiles_x, const int tiles_y, const int grid_n) {
    constexpr int BM = PT_BM, WM = BM / NWM, WN = BN / NWN, NW = NWM * NWN;
    static_assert(WM % 16 == 0 && WN % 32 == 0 && BM % NWM == 0 && BN % NWN == 0, "wave tile (channel tiles come in pairs)");
    static_assert(EPI == EPI_SPLIT || EPI == EPI_SPLIT_RES, "patch kernel epilogues");
    constexpr int TM = WM / 16, TN = WN / 16;
    constexpr int PANEL_B = BN * 64, BST = 2 * PANEL_B, PATCH = 2 * PT_PLANE;
    constexpr int NPIECE = PT_PROWS / 16, PPW = (NPIECE + NW - 1) / NW;     // patch pieces (16 rows) and pieces per wave
    constexpr int RB_B = BN / 16, B_PER = (RB_B + NW - 1) / NW;
    constexpr int LB = 2 * B_PER, LP = 2 * PPW;                             // DMA instructions per wave: one weight stage, one patch
    static_assert(STAGES >= 3 && STAGES - 1 < 9 && (STAGES - 2) * LB + LP <= 20, "ring depth / vmcnt literals");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const wst = smem + 2 * PATCH;                 // weight stage ring

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n_tiles = a.B * tiles_y * tiles_x * grid_n;
    const unsigned PS = (unsigned)a.in_ldc * 4u, lo_plane = (unsigned)a.in_ldc * 2u;
    const int ncc = a.Cin / 32;
    const unsigned wchunk = (unsigned)a.Npad * (HBK * 2);
    const __amdgpu_buffer_rsrc_t rs_a = buffer_rsrc(a.in, a.in_bytes);
    const __amdgpu_buffer_rsrc_t rs_wh = buffer_rsrc(a.w_hi, a.w_bytes);
    const __amdgpu_buffer_rsrc_t rs_wl = buffer_rsrc(a.w_lo, a.w_bytes);
    const unsigned lds0 = (unsigned)(size_t)smem;

    // tile index -> (image, tile row, tile column, channel tile); XCD-aware remap as in conv_ring_f16s3.hip
    auto tile_of = [&](int t, int& b, int& y0, int& x0, int& bn) __attribute__((always_inline)) {
        int u = xcd_remap(t, n_tiles);
        bn = u % grid_n; u /= grid_n;
        x0 = (u % tiles_x) * PT_TW; u /= tiles_x;
        y0 = (u % tiles_y) * PT_TH; b = u / tiles_y;
    };

    // ---- loader state.  Patch piece j of this wave: 16 patch rows; lane l -> patch row q = 16*piece + l/4 = (py, px),
    // 16-byte position l&3 holding source chunk (l&3) ^ swizzle(q).  (py, px) do not depend on the tile.
    const int lrow = lane >> 2;
    int pc_piece[PPW], pdy[PPW], pdx[PPW]; unsigned pchunk[PPW];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        pc_piece[j] = (wave + j * NW) % NPIECE;
        const int q = pc_piece[j] * 16 + lrow;
        const int py = q / PT_PC, px = q - py * PT_PC;
        pdy[j] = q < PT_PE ? py - 1 : -(1 << 20);               // pad 1; rows beyond the patch: always out of the image -> zeros
        pdx[j] = px - 1;
        pchunk[j] = (unsigned)(((lane & 3) ^ ((q >> 1) & 3)) * 8) * 2u;
    }
    int blk_b[B_PER]; unsigned wrow[B_PER];
    const int lchunk = (lane & 3) ^ ((lrow >> 1) & 3);
#pragma unroll
    for (int j = 0; j < B_PER; ++j) blk_b[j] = (wave + j * NW) % RB_B;

    int ld_tile = blockIdx.x;                                    // tile / chunk / tap the WEIGHT loader is at
    int ld_cc = 0, ld_tap = 0;
    int ld_bn = 0;
    auto wload_enter_tile = [&]() __attribute__((always_inline)) {
        int b, y0, x0;
        tile_of(ld_tile < n_tiles ? ld_tile : 0, b, y0, x0, ld_bn);
#pragma unroll
        for (int j = 0; j < B_PER; ++j) {
            const int rho = blk_b[j] * 16 + lrow;
            wrow[j] = ld_tile < n_tiles ? (unsigned)((ld_bn * BN + tr_chan_of_row(rho)) * 32 + lchunk * 8) * 2u : OOB;
        }
        ld_cc = 0; ld_tap = 0;
    };
    auto wload_issue = [&](int slot) __attribute__((always_inline)) {
        const unsigned koff = (unsigned)(ld_cc * 9 + ld_tap) * wchunk;
        const unsigned sbase = lds0 + 2u * PATCH + (unsigned)slot * BST;
#pragma unroll
        for (int j = 0; j < B_PER; ++j) {
            const unsigned l = sbase + (unsigned)blk_b[j] * 1024u;
            lds_dma_pair(rs_wh, rs_wl, wrow[j], koff, koff, l, l + PANEL_B);
        }
        if (++ld_tap == 9) { ld_tap = 0; if (++ld_cc == ncc) { ld_tile += gridDim.x; wload_enter_tile(); } }
    };
    // patch of (tile pt, chunk pcc) into patch buffer pbuf
    auto patch_issue = [&](int pt, int pcc, int pbuf) __attribute__((always_inline)) {
        int b, y0, x0, bn_;
        tile_of(pt < n_tiles ? pt : 0, b, y0, x0, bn_);
        const unsigned soff = (unsigned)pcc * 64u;
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            const int iy = y0 + pdy[j], ix = x0 + pdx[j];        // stride 1: input pixel = output pixel + (ky - 1, kx - 1)
            const bool ok = pt < n_tiles && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
            const unsigned vo = ok ? (unsigned)((b * a.Hi + iy) * a.Wi + ix) * PS + (unsigned)a.in_coff * 2u + pchunk[j] : OOB;
            const unsigned l = lds0 + (unsigned)pbuf * PATCH + (unsigned)pc_piece[j] * 1024u;
            lds_dma_pair(rs_a, rs_a, vo, soff, soff + lo_plane, l, l + PT_PLANE);
        }
    };

    // ---- consumer state
    const int wm = wave / NWN, wn = wave - wm * NWN;
    const int lr = lane & 15, lh = lane >> 4;
    const int b_row = (wn * WN + lr) * 64 + ((lh ^ ((lr >> 1) & 3)) << 4);
    int a_base[TM];                                              // patch row of this lane's pixel for tap (0, 0)
#pragma unroll
    for (int i = 0; i < TM; ++i) a_base[i] = (wm * (WM / 16) + i) * PT_PC + lr;

    // prologue: the first patch, then STAGES-1 weight stages
    wload_enter_tile();
    patch_issue(blockIdx.x, 0, 0);
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s) wload_issue(s);
    int slot = 0, pbuf = 0;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int tb, y0, x0, bn;
        tile_of(tile, tb, y0, x0, bn);
        f32x4 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

#pragma unroll 1
        for (int cc = 0; cc < ncc; ++cc) {
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                // this wave's pieces of the current weight stage (and, being older, of the current patch) have landed; younger:
                // STAGES-2 weight stages and, for the STAGES-1 steps after a patch prefetch was issued, that patch
                if (tap >= 1 && tap <= STAGES - 1) vmcnt<(STAGES - 2) * LB + LP>();
                else vmcnt<(STAGES - 2) * LB>();
                __builtin_amdgcn_s_barrier();                    // ... and everybody's; the previous step's slot / the other patch buffer are free
                wload_issue(slot == 0 ? STAGES - 1 : slot - 1);  // the weight stage STAGES-1 steps ahead
                if (tap == 0) {                                  // next chunk's patch (of the next tile after the last chunk) into the other buffer
                    const bool last = cc + 1 == ncc;
                    patch_issue(last ? tile + (int)gridDim.x : tile, last ? 0 : cc + 1, pbuf ^ 1);
                }
                const unsigned char* pp = smem + pbuf * PATCH;
                const unsigned char* st = wst + slot * BST + b_row;
                const int shift = (tap / 3) * PT_PC + (tap % 3);
                f16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int q = a_base[i] + shift;
                    const int o = q * 64 + ((lh ^ ((q >> 1) & 3)) << 4);
                    ah[i] = *reinterpret_cast<const f16x8*>(pp + o);
                    al[i] = *reinterpret_cast<const f16x8*>(pp + PT_PLANE + o);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    bh[j] = *reinterpret_cast<const f16x8*>(st + j * 16 * 64);
                    bl[j] = *reinterpret_cast<const f16x8*>(st + PANEL_B + j * 16 * 64);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[j], al[i], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[j], ah[i], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[j], ah[i], acc[i][j], 0, 0, 0);
                    }
                slot = slot + 1 == STAGES ? 0 : slot + 1;
            }
            pbuf ^= 1;
        }
        // epilogue straight from the accumulators: pixel tile i is output row y0 + wm*(WM/16) + i, this lane's column x0 + lr
        int mrow[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int oy = y0 + wm * (WM / 16) + i, ox = x0 + lr;
            mrow[i] = (oy < a.Ho && ox < a.Wo) ? (tb * a.Ho + oy) * a.Wo + ox : -1;
        }
        conv_f16s3_epilogue_regs<WM, WN, EPI == EPI_SPLIT_RES>(a, acc, nullptr, mrow, bn * BN + wn * WN, tid, lh);
    }
    vmcnt<0>();                                                  // trailing (out-of-range) pieces: nothing may be in flight at exit
}

// ---- Weights-resident variant (mode PATCH_WRES_MODE): Cin = 32, Cout = 64 (YOLOv3's layer 3, 304x304 at 608x608).
// With K = 288 a tile is nine steps, and the streamed-weight kernel above moves 73 KB of weights per 128-pixel tile through
// L2 -> LDS: 5 776 tiles x 73 KB = 422 MB per launch, as much as the layer's activations.  Here the nine taps' weights stay
// in LDS for the lifetime of the persistent workgroup (one per CU): per tile one barrier, the next tile's patch by LDS-DMA
// under the nine taps, tap t + 1's fragments read while tap t's twelve MFMAs run (conv_stem2_f16s3.hip's tap loop, which
// runs at the MFMA rate).  Same K order and product order as every other tile of the layer: bit-identical.
constexpr int PW_W1 = 9 * 64 * 64;                                      // one plane of the resident weights: [tap][64 rows][64 B]
constexpr int PW_LDS = 4 * PT_PLANE + 2 * PW_W1;
template <int EPI>
__global__ __launch_bounds__(512, 2)
void conv_patch_wres_f16s3_kernel(const ConvArgs a, const int tiles_x, const int tiles_y) {
    constexpr int NWN = 2, NW = 8, WM = 32, WN = 32, TM = 2, TN = 2, PATCH = 2 * PT_PLANE;
    constexpr int NPIECE = PT_PROWS / 16, PPW = (NPIECE + NW - 1) / NW;
    static_assert(EPI == EPI_SPLIT || EPI == EPI_SPLIT_RES, "patch kernel epilogues");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const w1 = smem + 2 * PATCH;

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int n_tiles = a.B * tiles_y * tiles_x;
    const unsigned PS = (unsigned)a.in_ldc * 4u, lo_plane = (unsigned)a.in_ldc * 2u;
    const __amdgpu_buffer_rsrc_t rs_a = buffer_rsrc(a.in, a.in_bytes);
    const unsigned lds0 = (unsigned)(size_t)smem;

    auto tile_of = [&](int t, int& b, int& y0, int& x0) __attribute__((always_inline)) {
        int u = xcd_remap(t, n_tiles);
        x0 = (u % tiles_x) * PT_TW; u /= tiles_x;
        y0 = (u % tiles_y) * PT_TH; b = u / tiles_y;
    };

    // ---- once: the nine taps' weights -> LDS (rows in the transposed product's channel order, chunk swizzle on the source side)
    const int lrow = lane >> 2;
    {
        const __amdgpu_buffer_rsrc_t rs_wh = buffer_rsrc(a.w_hi, a.w_bytes);
        const __amdgpu_buffer_rsrc_t rs_wl = buffer_rsrc(a.w_lo, a.w_bytes);
        for (int p = wave; p < 9 * 4; p += NW) {                         // (tap, 16-row block): one hi + one lo piece each
            const int tap = p >> 2, rb = p & 3;
            const int rho = rb * 16 + lrow;
            const int ch = (lane & 3) ^ ((rho >> 1) & 3);
            const unsigned vo = (unsigned)(tr_chan_of_row(rho) * 32 + ch * 8) * 2u;      // planes are [chunk*9 + tap][Npad][32], Cin = 32: chunk 0
            const unsigned koff = (unsigned)tap * (unsigned)a.Npad * 64u;
            const unsigned l = lds0 + 2u * PATCH + (unsigned)(tap * 64 * 64 + rb * 1024);
            lds_dma_pair(rs_wh, rs_wl, vo, koff, koff, l, l + PW_W1);
        }
    }
    // ---- patch loader (as above, one chunk)
    int pc_piece[PPW], pdy[PPW], pdx[PPW]; unsigned pchunk[PPW];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
        pc_piece[j] = (wave + j * NW) % NPIECE;
        const int q = pc_piece[j] * 16 + lrow;
        const int py = q / PT_PC, px = q - py * PT_PC;
        pdy[j] = q < PT_PE ? py - 1 : -(1 << 20);
        pdx[j] = px - 1;
        pchunk[j] = (unsigned)(((lane & 3) ^ ((q >> 1) & 3)) * 8) * 2u;
    }
    auto patch_issue = [&](int pt, int pbuf) __attribute__((always_inline)) {
        int b, y0, x0;
        tile_of(pt < n_tiles ? pt : 0, b, y0, x0);
#pragma unroll
        for (int j = 0; j < PPW; ++j) {
            const int iy = y0 + pdy[j], ix = x0 + pdx[j];
            const bool ok = pt < n_tiles && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi;
            const unsigned vo = ok ? (unsigned)((b * a.Hi + iy) * a.Wi + ix) * PS + (unsigned)a.in_coff * 2u + pchunk[j] : OOB;
            const unsigned l = lds0 + (unsigned)pbuf * PATCH + (unsigned)pc_piece[j] * 1024u;
            lds_dma_pair(rs_a, rs_a, vo, 0u, lo_plane, l, l + PT_PLANE);
        }
    };

    // ---- consumer state: wave (wm, wn) owns output rows 2 wm, 2 wm + 1 of the tile and channels 32 wn .. 32 wn + 31
    const int wm = wave / NWN, wn = wave - wm * NWN;
    const int lr = lane & 15, lh = lane >> 4;
    const int w_lane = ((wn * 2) * 16 + lr) * 64 + ((lh ^ ((lr >> 1) & 3)) << 4);
    int a_base[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) a_base[i] = (wm * TM + i) * PT_PC + lr;

    patch_issue(blockIdx.x, 0);
    vmcnt<0>();                                                          // weights and the first patch: this wave's pieces
    int pbuf = 0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int tb, y0, x0;
        tile_of(tile, tb, y0, x0);
        __builtin_amdgcn_s_barrier();                                    // everybody's pieces of this tile's patch landed; the other buffer is free
        patch_issue(tile + (int)gridDim.x, pbuf ^ 1);                    // next tile's patch: in flight under the nine taps
        f32x4 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned char* pp = smem + pbuf * PATCH;
        f16x8 fah[2][TM], fal[2][TM], fbh[2][TN], fbl[2][TN];
        auto load_tap = [&](int tap, int buf) __attribute__((always_inline)) {
            const int shift = (tap / 3) * PT_PC + (tap % 3);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int q = a_base[i] + shift;
                const int o = q * 64 + ((lh ^ ((q >> 1) & 3)) << 4);
                fah[buf][i] = *reinterpret_cast<const f16x8*>(pp + o);
                fal[buf][i] = *reinterpret_cast<const f16x8*>(pp + PT_PLANE + o);
            }
            const unsigned char* wp = w1 + tap * 64 * 64 + w_lane;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                fbh[buf][j] = *reinterpret_cast<const f16x8*>(wp + j * 1024);
                fbl[buf][j] = *reinterpret_cast<const f16x8*>(wp + PW_W1 + j * 1024);
            }
        };
        load_tap(0, 0);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int cur = tap & 1;
            if (tap + 1 < 9) load_tap(tap + 1, cur ^ 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[cur][j], fal[cur][i], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbl[cur][j], fah[cur][i], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[cur][j], fah[cur][i], acc[i][j], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        vmcnt<0>();                                                      // this wave's pieces of the next patch (issued nine taps ago) and older stores
        int mrow[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int oy = y0 + wm * TM + i, ox = x0 + lr;
            mrow[i] = (oy < a.Ho && ox < a.Wo) ? (tb * a.Ho + oy) * a.Wo + ox : -1;
        }
        conv_f16s3_epilogue_regs<WM, WN, EPI == EPI_SPLIT_RES>(a, acc, nullptr, mrow, wn * WN, tid, lh);
        pbuf ^= 1;
    }
    vmcnt<0>();
}

bool conv_patch_supported(int ksize, int stride, int pad, int cin, int cout) {
    return ksize == 3 && stride == 1 && pad == 1 && cin % 32 == 0 && cout % 8 == 0;
}

// One list drives the mode table, the launch switch and the kernel names rocprofv3 prints:
//   X(mode, BN, waves along M, waves along N, STAGES, MINW)
#define RTOD_PATCH_TILES(X) X(0, 64, 4, 2, 4, 4) X(1, 128, 4, 2, 3, 2) X(2, 64, 4, 2, 3, 4) X(3, 128, 4, 2, 4, 2)

#define RTOD_X_INFO(mode, bn, nwm, nwn, st, minw) {PT_BM, bn, "conv_patch_f16s3<8x16x" #bn "," #nwm "x" #nwn ",s" #st ">"},
static const ConvVariantInfo kPatchModes[PATCH_MODES] = { RTOD_PATCH_TILES(RTOD_X_INFO) {PT_BM, 64, "conv_patch_f16s3<8x16x64,4x2,weights resident>"} };
#undef RTOD_X_INFO
static_assert(PATCH_WRES_MODE == PATCH_MODES - 1, "the weights-resident mode is the last patch mode");
const ConvVariantInfo& conv_patch_mode_info(int mode) { return kPatchModes[mode < 0 || mode >= PATCH_MODES ? 0 : mode]; }
bool conv_patch_mode_valid(int mode, int cin, int cout) {
    if (mode < 0 || mode >= PATCH_MODES) return false;
    return mode != PATCH_WRES_MODE || (cin == 32 && cout == 64);
}

int conv_patch_kernel_name(int mode, int epi, char* buf, size_t len) {
#define RTOD_X_NAME(m, bn, nwm, nwn, st, minw) \
    if (mode == m) return snprintf(buf, len, "void rtod::conv_patch_f16s3_kernel<" #bn ", " #nwm ", " #nwn ", " #st ", " #minw ", %d>(rtod::ConvArgs, int, int, int)", epi);
    RTOD_PATCH_TILES(RTOD_X_NAME)
#undef RTOD_X_NAME
    if (mode == PATCH_WRES_MODE) return snprintf(buf, len, "void rtod::conv_patch_wres_f16s3_kernel<%d>(rtod::ConvArgs, int, int)", epi);
    return -1;
}

template <int BN, int NWM, int NWN, int STAGES, int MINW>
static int launch_patch(const ConvArgs& a, hipStream_t s) {
    constexpr int NT = NWM * NWN * 64;
    const int tiles_x = (a.Wo + PT_TW - 1) / PT_TW, tiles_y = (a.Ho + PT_TH - 1) / PT_TH, gn = (a.Cout + BN - 1) / BN;
    const int lds = 4 * PT_PLANE + STAGES * 2 * BN * 64;
    const int cus = device_cu_count();
    if (cus <= 0) return hip_fail(hipGetLastError(), "conv_patch_f16s3 device query");
    const int by_lds = (160 * 1024) / lds, by_waves = (MINW * 4) / (NWM * NWN) > 0 ? (MINW * 4) / (NWM * NWN) : 1;
    const int per_cu = by_lds < by_waves ? by_lds : by_waves;
    const int64_t tiles = (int64_t)a.B * tiles_x * tiles_y * gn;
    const int slots = cus * (per_cu > 0 ? per_cu : 1);
    const int grid = (int)(tiles < slots ? tiles : slots);
    auto k_res = conv_patch_f16s3_kernel<BN, NWM, NWN, STAGES, MINW, EPI_SPLIT_RES>;
    auto k_plain = conv_patch_f16s3_kernel<BN, NWM, NWN, STAGES, MINW, EPI_SPLIT>;
    static std::atomic<unsigned long long> attr_done{0};
    if (int rc = lds_opt_in(attr_done, 160 * 1024, "conv_patch_f16s3", k_res, k_plain)) return rc;
    if (a.res) hipLaunchKernelGGL(k_res, dim3(grid), dim3(NT), lds, s, a, tiles_x, tiles_y, gn);
    else hipLaunchKernelGGL(k_plain, dim3(grid), dim3(NT), lds, s, a, tiles_x, tiles_y, gn);
    return hip_fail(hipGetLastError(), "conv_patch_f16s3 launch");
}

int launch_conv_patch_f16s3(const ConvArgs& a, int mode, hipStream_t s) {
    if (int rc = check_split_conv_args(a, "launch_conv_patch", false)) return rc;
    if (!conv_patch_supported(a.kh, a.stride, a.pad, a.Cin, a.Cout) || a.kw != 3 || a.Ho != a.Hi || a.Wo != a.Wi || a.dec.enabled || a.pw_wh) {
        set_error("launch_conv_patch: unsupported layer (k=%d s=%d pad=%d Cin=%d)", a.kh, a.stride, a.pad, a.Cin); return RTOD_E_ARG;
    }
    if (a.in_ldc % 8 || a.in_coff % 8 || a.out_ldc % 8 || a.out_coff % 8 || a.K != a.Kpad || a.K != 9 * a.Cin) { set_error("launch_conv_patch: bad view / K"); return RTOD_E_ARG; }
    if (mode == PATCH_WRES_MODE) {
        if (a.Cin != 32 || a.Cout != 64 || a.Npad < 64) { set_error("launch_conv_patch: the weights-resident tile needs Cin = 32, Cout = 64"); return RTOD_E_ARG; }
        const int tiles_x = (a.Wo + PT_TW - 1) / PT_TW, tiles_y = (a.Ho + PT_TH - 1) / PT_TH;
        const int cus = device_cu_count();
        if (cus <= 0) return hip_fail(hipGetLastError(), "conv_patch_f16s3 device query");
        const int64_t tiles = (int64_t)a.B * tiles_x * tiles_y;
        if (tiles >= (1ll << 30)) { set_error("launch_conv_patch: too many tiles"); return RTOD_E_ARG; }
        const int grid = (int)(tiles < cus ? tiles : cus);
        auto k_res = conv_patch_wres_f16s3_kernel<EPI_SPLIT_RES>;
        auto k_plain = conv_patch_wres_f16s3_kernel<EPI_SPLIT>;
        static std::atomic<unsigned long long> attr_done{0};
        if (int rc = lds_opt_in(attr_done, 160 * 1024, "conv_patch_f16s3", k_res, k_plain)) return rc;
        static_assert(PW_LDS <= 160 * 1024, "LDS budget");
        if (a.res) hipLaunchKernelGGL(k_res, dim3(grid), dim3(512), PW_LDS, s, a, tiles_x, tiles_y);
        else hipLaunchKernelGGL(k_plain, dim3(grid), dim3(512), PW_LDS, s, a, tiles_x, tiles_y);
        return hip_fail(hipGetLastError(), "conv_patch_wres_f16s3 launch");
    }
    switch (mode) {
#define RTOD_X_CASE(m, bn, nwm, nwn, st, minw) case m: return launch_patch<bn, nwm, nwn, st, minw>(a, s);
        RTOD_PATCH_TILES(RTOD_X_CASE)
#undef RTOD_X_CASE
    }
    set_error("launch_conv_patch: mode %d unsupported", mode);
    return RTOD_E_ARG;
}

}  // namespace rtod
