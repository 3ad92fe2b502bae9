// One filter stage of the fp32 F(4x4) kernels (conv_wino4_kernel, conv_wino4r_kernel), included inside the kernel body: column transform of
// two channels of t[], three filter reads, 12 MFMAs with the LDS-DMA of later stages pinned behind them.
// Expects: t[6], acc[6], Bw (the wave's first filter stage), lane, dma_filter_piece, dma_halo_piece; defines mfma_stage(ss, fbuf, next_stage, halo_grp).
// W4_MFMA(ACC, A, B): one v_mfma_f32_32x32x2_f32, unless an A/B build of the including file defined a timing-only stand-in.
#ifndef W4_MFMA
#define W4_MFMA(ACC, A, B) ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A, B, ACC, 0, 0, 0)
#endif
    // ss: channel pair of t[] (channels 2 ss, 2 ss + 1), fbuf: filter buffer; next_stage: filter stage to stream into the other buffer;
    // halo_grp: halo group to prefetch, < 0: none
    auto mfma_stage = [&](int ss, int fbuf, int next_stage, int halo_grp) __attribute__((always_inline)) {
        const int nbuf = fbuf ^ 1;
        float V[6][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {   // V[nu] = sum_j B^T[nu][j] t[j]; scalar fmas on purpose (-fno-slp-vectorize): packed f32 VALU ops stall the SIMD beside MFMAs
            const int c = 2 * ss + e;
            const float u0 = t[0][c], u1 = t[1][c], u2 = t[2][c], u3 = t[3][c], u4 = t[4][c], u5 = t[5][c];
            // points +-a share an even part (u4 - b2 u2) and an odd part (u3 - b2 u1), points +-b likewise with a2
            const float ea = __builtin_fmaf(-KB2, u2, u4), oa = __builtin_fmaf(-KB2, u1, u3);
            const float eb = __builtin_fmaf(-KA2, u2, u4), ob = __builtin_fmaf(-KA2, u1, u3);
            V[0][e] = __builtin_fmaf(KP, u0, __builtin_fmaf(KS, u2, u4));
            V[1][e] = __builtin_fmaf(KA, oa, ea);
            V[2][e] = __builtin_fmaf(-KA, oa, ea);
            V[3][e] = __builtin_fmaf(KB, ob, eb);
            V[4][e] = __builtin_fmaf(-KB, ob, eb);
            V[5][e] = __builtin_fmaf(KP, u1, __builtin_fmaf(KS, u3, u5));
        }
        f32x2 w2[6];
        const f32x4* Bp = Bw + W4Lds::bw_stage(0, fbuf) + W4Lds::bw_read(lane, 0);        // three 16-byte reads: the fragments of point pairs (0, 1), (2, 3), (4, 5)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const f32x4 w4 = Bp[W4Lds::bw_read(0, k)];
            w2[2 * k] = f32x2{w4[0], w4[1]};
            w2[2 * k + 1] = f32x2{w4[2], w4[3]};
        }
        // 12 MFMAs, channel-major: consecutive MFMAs hit different accumulators (dependency distance 6), so even a lone
        // wave keeps the matrix pipe full.  The next stage's three filter pieces go out one at a time behind MFMAs 2, 4
        // and 6 (pinned): the wave's issue slot is free while the pipe works, and the load path never sees a burst.
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int v = 0; v < 6; ++v) {
                W4_MFMA(acc[v], V[v][e], w2[v][e]);
                if (e == 0 && (v == 1 || v == 3 || v == 5)) {
                    W4_SB();
                    if (v == 1) dma_filter_piece(next_stage, nbuf, std::integral_constant<int, 0>{});
                    if (v == 3) dma_filter_piece(next_stage, nbuf, std::integral_constant<int, 1>{});
                    if (v == 5) dma_filter_piece(next_stage, nbuf, std::integral_constant<int, 2>{});
                    W4_SB();
                }
                if (e == 1 && (v == 1 || v == 3) && halo_grp >= 0) {       // behind MFMAs 8 and 10
                    W4_SB();
                    if (v == 1) dma_halo_piece(halo_grp, std::integral_constant<int, 0>{});
                    if (v == 3) dma_halo_piece(halo_grp, std::integral_constant<int, 1>{});
                    W4_SB();
                }
            }
    };
