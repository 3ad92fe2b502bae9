// Filter LDS-DMA of the F(4x4) kernels, included inside the kernel body: every wave streams its own 3-KB stage as three 1-KB pieces into a
// private double buffer, ordered by its own counted vmcnt only.
// Expects: w_base (global byte address of the wave's stage 0), wave, lane, lds_base; defines lane16, dma_filter_piece(stage, buf, piece).
// W4_FILTER_STRIDE: global bytes from one stage of a wave to its next; W4_FILTER_LDS(buf): LDS byte offset of the wave's stage buffer `buf`.
    const unsigned lane16 = (unsigned)lane * 16u;            // the address is a scalar base (advanced per stage by scalar adds) + the lane's constant 16-byte offset
    auto dma_filter_piece = [&](int stage, int buf, auto kk) __attribute__((always_inline)) {
        W4_DIAG_SKIP_FILTER_DMA();
        constexpr int k = decltype(kk)::value;
        const unsigned long long g = w_base + (unsigned long long)W4_DIAG_FILTER_STAGE(stage) * W4_FILTER_STRIDE;
        const unsigned dst = lds_base + (unsigned)W4_FILTER_LDS(buf);
        const unsigned l16 = lane16;
        unsigned keep;
        // the instruction offset advances the global AND the LDS address: one M0 for the three pieces
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3 offset:%4\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(l16), "s"(dst), "s"(g), "n"(k * 1024) : "memory");
    };
