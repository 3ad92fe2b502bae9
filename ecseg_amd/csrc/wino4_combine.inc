// Shared output stage of the F(4x4) kernels, included inside the pass loop after the exchange image Rs holds R = M A for the 32
// output channels of `pass`: Y = A^T R + bias, activation, 16-byte stores, fused 2x2 max-pool, partial logits of a fused 1x1 head.
// Expects: Rs, pass, nb, tid, bvp[2], hl[2][4][4], r_img / r_y0 / r_x0, p, H, W, Cout, HEAD.
//
// Round 6: the stage is bound by the vector pipe (in-kernel stamps: ~1 500 cycles per round of ~120 vector instructions x 3 waves per
// SIMD, six rounds per workgroup = 9 000 of the 12 000 - 17 000 cycles a workgroup spends after its K loop).  It used to run 2048 HALF
// items (channel quad, column, tile, row pair) in three rounds and rebuilt tile, region, image and the 64-bit output address of every
// item from the thread index.  Now: 1024 WHOLE items (the four rows of a tile column: the +- sums and the address are shared by the
// row pairs), a wave owns the tile PAIR nw = wave + 12 k - tile row, region, image and the output base are wave-uniform and live in
// scalar registers - and a lane's channel quad, column and byte offset are the same in every round.  Waves 0-3 (one per SIMD) take a
// second round: 4 wave-rounds of ~90 vector instructions per SIMD and pass instead of 8 of ~120.
        const int n0 = nb * 64 + pass * 32;
        // The bias quads are waited for HERE, in straight-line code: left to the compiler the wait lands behind the first round's
        // (conditional) body and is repeated as s_waitcnt vmcnt(0) in the later rounds - vmcnt counts the output stores too.
        asm volatile("" :: "v"(bvp[0]), "v"(bvp[1]));
        const f32x4 bv = pass ? bvp[1] : bvp[0];
        const int cq = tid & 7, cx = (tid >> 3) & 3, nlo = (tid >> 5) & 1;          // channel quad, column of the tile, tile of the pair
        const int cwave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int co = n0 + 4 * cq;
        const bool co_ok = co + 3 < Cout;
        const float* rlane = Rs + W4Lds::r_comb(cx, nlo, cq, 0);           // (the function is a sum of a lane part and a tile-pair part)
        const unsigned out_lane = (unsigned)((4 * nlo + cx) * p.out.cs + co);       // floats from the tile pair's first output pixel
        const unsigned out_row = (unsigned)(W * p.out.cs);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int nw = cwave + 12 * k;                   // tile pair: tiles 2 nw, 2 nw + 1 (columns 0 / 1 or 2 / 3 of tile row nw >> 1)
            if (nw >= 16) break;
            const int nq8 = nw >> 1;
            const int g = W4_QUAD_REGION(nq8), nty = nq8 >> 1;
            const int img = g ? r_img[1] : r_img[0];
            if (img < 0) continue;
            const float* r = rlane + W4Lds::r_comb(0, 0, 0, nw);
            const f32x4 q0 = *reinterpret_cast<const f32x4*>(r);
            const f32x4 q1 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 1));
            const f32x4 q2 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 2));
            const f32x4 q3 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 3));
            const f32x4 q4 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 4));
            const f32x4 q5 = *reinterpret_cast<const f32x4*>(r + W4Lds::r_plane(4 * 5));
            const f32x4 s12 = q1 + q2, d12 = q1 - q2, s34 = q3 + q4, d34 = q3 - q4;
            f32x4 y[4];                                      // (the expressions of the half-item form, term for term: results are bit-identical)
            y[0] = q0 + s12 + s34 + bv;
            y[1] = KA * d12 + KB * d34 + bv;
            y[2] = KA2 * s12 + KB2 * s34 + bv;
            y[3] = KA3 * d12 + KB3 * d34 + q5 + bv;
            if (p.act == ECSEG_ACT_RELU) {
                // one v_max per value (fmaxf costs a second one that quiets a signalling NaN first; v_max does both under IEEE mode)
#pragma unroll
                for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float t = y[yy][c];
                        asm("v_max_f32_e32 %0, 0, %1" : "=v"(t) : "v"(t));
                        y[yy][c] = t;
                    }
            } else if (p.act != ECSEG_ACT_LINEAR) {
#pragma unroll
                for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                    for (int c = 0; c < 4; ++c) y[yy][c] = apply_act_core(y[yy][c], p.act, p.alpha);
            }
            const int oy = (g ? r_y0[1] : r_y0[0]) + 4 * nty, ox = (g ? r_x0[1] : r_x0[0]) + 8 * (nw & 1);       // wave-uniform
            if (!HEAD && co_ok) {                            // (a fused head is the only reader of the features: the launchers check head_only)
                float* ob = p.out.p + (((size_t)img * H + oy) * W + ox) * p.out.cs;
                // non-temporal: the tensor (0.6 - 9.4 GB per launch) fits no cache and is read by a later launch; +0.7 % end to end
                // (A/B round 4: 64 -> 64 at 256x256 10.79 - 10.92 -> 10.58 - 10.63 ms, the deep layers +-0)
#pragma unroll
                for (int yy = 0; yy < 4; ++yy)
                    __builtin_nontemporal_store(y[yy], reinterpret_cast<f32x4*>(ob + (size_t)(out_lane + (unsigned)yy * out_row)));
            }
            if (HEAD) {                                      // this lane's 4 channels x 4 classes of the 1x1 head
                const f32x4* hw = reinterpret_cast<const f32x4*>(p.head_w) + co;
                const f32x4 w0 = hw[0], w1 = hw[1], w2 = hw[2], w3 = hw[3];
#pragma unroll
                for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        hl[k][yy][c] += y[yy][0] * w0[c] + y[yy][1] * w1[c] + y[yy][2] * w2[c] + y[yy][3] * w3[c];
            }
            if (!HEAD && p.pool.p != nullptr) {             // (never with a fused head: plan_run.hip fuses a head only where no pool is)
                // fused MaxPooling2D(2x2, stride 2): the row pairs are in registers, the column partner (cx ^ 1) is lane ^ 8 of
                // the same tile, hence of the same region: it is active whenever this lane is
                float* pb = p.pool.p + (((size_t)img * p.pool.h + (oy >> 1)) * p.pool.w + (ox >> 1)) * p.pool.cs;
                const unsigned pool_lane = (unsigned)((2 * nlo + (cx >> 1)) * p.pool.cs + co);
#pragma unroll
                for (int yp = 0; yp < 2; ++yp) {
                    f32x4 m;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float a = fmaxf(y[2 * yp][c], y[2 * yp + 1][c]);
                        m[c] = fmaxf(a, __shfl_xor(a, 8));
                    }
                    if (!(cx & 1) && co_ok)
                        *reinterpret_cast<f32x4*>(pb + (size_t)(pool_lane + (unsigned)(yp * p.pool.w * p.pool.cs))) = m;
                }
            }
        }
