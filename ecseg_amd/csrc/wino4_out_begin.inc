// Start of the output stage of the F(4x4) kernels, included inside the kernel body right behind the K loop.
// Expects: smem, p, nb, tid, HEAD; defines Rs (the exchange image, over whatever the K loop left in LDS), Cout, hl[2][4][4], bvp[2].
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the compiler does not see the asm LDS-DMAs
    float* Rs = reinterpret_cast<float*>(smem);
    const int Cout = p.out.c;
    float hl[2][4][4];                                       // fused 1x1 head: partial logits [round][row of the tile][class]; named only in HEAD arms
    if constexpr (HEAD) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int c = 0; c < 4; ++c) hl[a][b][c] = 0.f;
    }
    // the bias quads of both passes are fetched here, under the K loop's drain and the first barrier: a global load inside
    // the combine step would queue behind the previous pass's output stores (one in-order vmcnt)
    f32x4 bvp[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (p.bias != nullptr) {
        bvp[0] = *reinterpret_cast<const f32x4*>(p.bias + nb * 64 + 4 * (tid & 7));
        if (nb * 64 + 32 < Cout) bvp[1] = *reinterpret_cast<const f32x4*>(p.bias + nb * 64 + 32 + 4 * (tid & 7));
    }
