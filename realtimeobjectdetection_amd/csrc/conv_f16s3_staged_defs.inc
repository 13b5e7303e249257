// The stage operations of the LDS-staged main loop (conv_f16s3_staged.h), included ONCE in the body of each kernel that runs it:
// conv_igemm_f16s3.hip, conv_c16_f16s3.hip, conv_ks_f16s3.hip; conv_f16s3_staged_run.inc is the schedule that calls them.  Text,
// not functions, on purpose: see "Why includes" in conv_f16s3_staged.h.
//
// In scope before the include:
//   Tile            StagedTile<BM, BN, NWM, NWN, F16> of the kernel, and BM, BN, NWN, F16 themselves
//   A_AHEAD         constexpr bool: the A fragments of a chunk are read ahead of the wait for the next stage set (generic, K-sliced)
//                   or with the B fragments, after the staging (16-channel tiles)
//   smem, tid       the kernel's LDS allocation (Tile::SMEM bytes, 16-byte aligned) and threadIdx.x
//   acc             f32x4 [Tile::TM][Tile::TN]
// Defined here: the stage sets S0, S1, lds_write, read_a, compute for conv_f16s3_staged_run.inc, and for the kernel's epilogue
// wm, wn (wave position in the tile), lr, lh (lane position in a 16x16 MFMA tile).
    typename Tile::Regs S0, S1;
    // LDS image: panel row r, 16-B chunk c at byte r*64 + ((c ^ ((r>>1)&3)) << 4)
    const int st_row = tid >> 2;                                        // this thread stages chunk tid & 3 of rows st_row + i RPP
    const int wr_swz = ((tid & 3) ^ ((st_row >> 1) & 3)) << 4;         // RPP % 8 == 0 -> same swizzle for every slot
    auto lds_write = [&](const typename Tile::Regs& S, int buf) {
        unsigned char* st = smem + buf * Tile::STAGE;
#pragma unroll
        for (int i = 0; i < Tile::A_SLOTS; ++i) {
            const int o = (st_row + i * Tile::RPP) * 64 + wr_swz;
            if ((i + 1) * Tile::RPP <= BM || st_row + i * Tile::RPP < BM) {
                *reinterpret_cast<u32x4*>(st + o) = S.ah[i];
                if constexpr (!F16) *reinterpret_cast<u32x4*>(st + Tile::PANEL_A + o) = S.al[i];
            }
        }
#pragma unroll
        for (int i = 0; i < Tile::B_SLOTS; ++i) {
            const int o = (st_row + i * Tile::RPP) * 64 + wr_swz;
            if ((i + 1) * Tile::RPP <= BN || st_row + i * Tile::RPP < BN) {
                *reinterpret_cast<u32x4*>(st + Tile::PANEL_B0 + o) = S.bh[i];
                if constexpr (!F16) *reinterpret_cast<u32x4*>(st + Tile::PANEL_B0 + Tile::PANEL_B + o) = S.bl[i];
            }
        }
    };

    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave / NWN, wn = wave - wm * NWN;
    const int lr = lane & 15, lh = lane >> 4;
    const int co = (lh ^ ((lr >> 1) & 3)) << 4;                  // WM, WN % 16 == 0: the row's swizzle is the lane's
    const int a_row = (wm * Tile::WM + lr) * 64 + co, b_row = Tile::PANEL_B0 + (wn * Tile::WN + lr) * 64 + co;

    f16x8 ah[Tile::TM], al[Tile::TM];
    auto read_a = [&](int buf) {
        const unsigned char* st = smem + buf * Tile::STAGE + a_row;
#pragma unroll
        for (int i = 0; i < Tile::TM; ++i) {
            ah[i] = *reinterpret_cast<const f16x8*>(st + i * 16 * 64);
            if constexpr (!F16) al[i] = *reinterpret_cast<const f16x8*>(st + Tile::PANEL_A + i * 16 * 64);
        }
    };
    // the MFMA step over a staged chunk: three products for f16s3, one for plain f16, fp32 accumulate
    auto compute = [&](int buf) {
        const unsigned char* st = smem + buf * Tile::STAGE + b_row;
        f16x8 ch[Tile::TM], cl[Tile::TM], bh[Tile::TN], bl[Tile::TN];
        if constexpr (!A_AHEAD) {                                 // the A fragments are read here, into ch / cl
            const unsigned char* sa = smem + buf * Tile::STAGE + a_row;
#pragma unroll
            for (int i = 0; i < Tile::TM; ++i) {
                ch[i] = *reinterpret_cast<const f16x8*>(sa + i * 16 * 64);
                if constexpr (!F16) cl[i] = *reinterpret_cast<const f16x8*>(sa + Tile::PANEL_A + i * 16 * 64);
            }
        }
#pragma unroll
        for (int j = 0; j < Tile::TN; ++j) {
            bh[j] = *reinterpret_cast<const f16x8*>(st + j * 16 * 64);
            if constexpr (!F16) bl[j] = *reinterpret_cast<const f16x8*>(st + Tile::PANEL_B + j * 16 * 64);
        }
#pragma unroll
        for (int j = 0; j < Tile::TN; ++j)
#pragma unroll
            for (int i = 0; i < Tile::TM; ++i) {
                const f16x8& xh = A_AHEAD ? ah[i] : ch[i];
                const f16x8& xl = A_AHEAD ? al[i] : cl[i];
                if constexpr (F16) { acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, bh[j], acc[i][j], 0, 0, 0); continue; }
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, bh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, bh[j], acc[i][j], 0, 0, 0);
            }
    };
