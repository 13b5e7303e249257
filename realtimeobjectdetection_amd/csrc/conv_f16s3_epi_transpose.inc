// Kernel-body text of the two LDS-transposed epilogues (conv_f16s3_epilogue in conv_f16s3_common.h, bandd_epilogue in
// conv_bandd_common.h), inside their loop over passes of RG rows: K group 1 of a two-group tile deposits its raw accumulators in the
// fp32 transpose tile T; the other (or only) group adds its own, scales, activates (the statements of epi_scale_act1 behind the
// uniform branch of epi_by_activation, conv_f16s3_common.h) and writes T.  The barrier that follows is the includer's.
// Text and not a function, scalar statements written out and not called: as __forceinline__ functions taking the row predicate as
// a functor, the same statements moved the VGPR count of 59 of 316 instances and cost nine of them a wave per SIMD, and this text
// calling epi_scale_act1 still moved the plain-f16 generic instances (profiles/experiments/epilogue_share_resource_usage.txt).
//
// The includer defines which accumulator rows belong to pass `rg` and undefines the three afterwards:
//   EPI_WAVE_IN_PASS      bool: any row of this wave (decided once per wave where a pass takes whole waves)
//   EPI_TILE_IN_PASS(i)   bool: the wave's 16-row tile i (decided per tile where a pass takes part of a wave's rows)
//   EPI_TILE_ROW(i)       first row of tile i inside T
// Names read: a, acc, T, TS, TM, TN, MT, KG, kg, RAW, wn, WN, lr, lh, bias_j, inv_j, escale.
        if constexpr (KG == 2) {
            if (kg == 1 && EPI_WAVE_IN_PASS) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if (EPI_TILE_IN_PASS(i)) {
#pragma unroll
                        for (int j = 0; j < TN; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) T[(EPI_TILE_ROW(i) + e + 4 * lh) * TS + wn * WN + j * MT + lr] = acc[i][j][e];
                    }
                }
            }
            __syncthreads();
        }
        if ((KG == 1 || kg == 0) && EPI_WAVE_IN_PASS) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int nl = wn * WN + j * MT + lr;
                const float bias = bias_j[j] * escale, inv = inv_j[j] * escale;
                auto col = [&](auto act) {                                   // 0 linear, 1 leaky, 2 SiLU
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        if (EPI_TILE_IN_PASS(i)) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int rl = EPI_TILE_ROW(i) + e + 4 * lh;
                                float s = acc[i][j][e];
                                if constexpr (KG == 2) s += T[rl * TS + nl];
                                if constexpr (RAW) { T[rl * TS + nl] = s * inv; continue; }      // the convolution sum: exact undo of the pre-scales
                                float v = s * inv + bias;                                        // (compiles to one fma: epi_scale_act1)
                                if constexpr (decltype(act)::value == 2) v = silu_scaled(v, 1.0f / escale);
                                else if constexpr (decltype(act)::value == 1) v = __builtin_fmaxf(v, v * 0.1f);   // == v > 0 ? v : 0.1 v, bit for bit (signed zeros, infinities, NaN)
                                T[rl * TS + nl] = v;
                            }
                        }
                    }
                };
                // uniform three-way branch around the loop: a per-value `if (a.leaky)` was a compare, a mask OR and a select per element
                if constexpr (RAW) col(std::integral_constant<int, 0>{});
                else if (a.leaky == 2) col(std::integral_constant<int, 2>{});
                else if (a.leaky) col(std::integral_constant<int, 1>{});
                else col(std::integral_constant<int, 0>{});
            }
        }
