// Shared tail of the F(4x4) kernels' output stage: finishes the fused 1x1 head (<= 4 classes) from the partial logits hl[][][].
    if (HEAD) {
        // the eight lanes q = 0..7 of a pixel column hold partial logits of 8 output channels each: butterfly over q,
        // then lane q < 4 finishes row q of the tile column (bias, softmax / activation over head_k classes) and stores it
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int q = tid & 7, x = (tid >> 3) & 3, nlo = (tid >> 5) & 1;
            const int nw = __builtin_amdgcn_readfirstlane(tid >> 6) + 12 * k;          // the item order of wino4_combine.inc
            if (nw >= 16) break;
            const int nq8 = nw >> 1, ntx = 2 * (nw & 1) + nlo;
            const int g = W4_QUAD_REGION(nq8), nty = nq8 >> 1;
            const int img = g ? r_img[1] : r_img[0];
            if (img < 0) continue;
            f32x4 mine = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float v = hl[k][yy][c];
                    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
                    if (q == yy) mine[c] = v;
                }
            if (q < 4) {
                const f32x4 hb = *reinterpret_cast<const f32x4*>(p.head_b);
                float l[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) l[c] = mine[c] + hb[c];
                if (p.head_act == ECSEG_ACT_SOFTMAX) {
                    float m = l[0];
#pragma unroll
                    for (int c = 1; c < 4; ++c) if (c < p.head_k) m = fmaxf(m, l[c]);
                    float sum = 0.f;
#pragma unroll
                    for (int c = 0; c < 4; ++c) { l[c] = c < p.head_k ? expf(l[c] - m) : 0.f; sum += l[c]; }
#pragma unroll
                    for (int c = 0; c < 4; ++c) l[c] = l[c] / sum;
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) l[c] = apply_act_core(l[c], p.head_act, p.alpha);
                }
                const int oy = (g ? r_y0[1] : r_y0[0]) + 4 * nty + q, ox = (g ? r_x0[1] : r_x0[0]) + 4 * ntx + x;
                float* ho = p.head_out.p + (((size_t)img * H + oy) * W + ox) * p.head_out.cs;
#pragma unroll
                for (int c = 0; c < 4; ++c) if (c < p.head_k) ho[c] = l[c];
            }
        }
    }
