// Shared by the three F(4x4) kernels (wino4_kernel.hip, wino4r_kernel.hip, wino4s_kernel.hip), included inside the kernel body:
// block order, the two 16x16 regions of the workgroup, their input boxes, and the halo LDS-DMA (dma_halo_piece).
// Expects: p, regs_x, regs_y, npairs, wave, lane, lds_base; defines bid, nb, pair, H, W, ngroups, tail4, r_img / r_y0 / r_x0 / r_win,
// hrsrc, hoff[2], dma_halo_piece(grp, piece).  W4_HALO_RING: depth of the halo ring in LDS (buffers of W4_HS slots from lds_base on);
// W4_HALO_L: the strides of the kernel's raw image (W4Lds::Raw / W4Lds::Ring, wino4_lds_layout.h) - slot REGION * region + ROW * r + cc, cc < COLS;
// W4_HALO_SLOT(r, cc) / W4_HALO_UPPER(cc): what (r, cc) holds - halo row hy, column hx, channel half h.
    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    // Block order: output-channel blocks in groups of G = 4 (2) next to each other, region pairs next, groups slowest.  The
    // workgroups running together on an XCD then share each input halo in L2 between G of them and keep only G filter
    // slabs streaming (spatial position fastest alone re-read the input Cout / 64 times from the Infinity Cache: 11-13x
    // the algorithmic bytes on the Cin = 1024 layers; channel block fastest alone streams Cout / 64 slabs at once): +1.4 %.
    const unsigned nblk_all = gridDim.x / (unsigned)npairs;
#ifdef ECSEG_W4_G                                               // (A/B builds only: tools/build_variants.sh ECSEG_W4_G=8)
    const unsigned G = (nblk_all % ECSEG_W4_G) == 0 ? ECSEG_W4_G : (nblk_all & 3u) == 0 ? 4u : (nblk_all & 1u) == 0 ? 2u : 1u;
#else
    const unsigned G = (nblk_all & 3u) == 0 ? 4u : (nblk_all & 1u) == 0 ? 2u : 1u;
#endif
    const unsigned lo = bid % G, rest = bid / G;
    const int pair = (int)(rest % (unsigned)npairs);
    const int nb = (int)((rest / (unsigned)npairs) * G + lo);
    const int H = p.in.h, W = p.in.w;                        // output extent == input extent
    const int ngroups = p.cin_chunks;                        // 8 input channels each
    const int nstages = 2 * ngroups;
    const bool tail4 = (p.in.c & 7) != 0;                    // (pointers are 16-byte aligned: bits 0 / 1 carry lane flags)

    // the two 16 x 16 regions of this workgroup: consecutive in (patch, region row, region column) order
    int r_img[2], r_y0[2], r_x0[2], r_win[2] = {-1, -1};     // r_win: window within its image (known for free in a cropped launch)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int rid = 2 * pair + g;
        int rx, ry, img;
        if (p.lut != nullptr) {                              // cropped launch: the regions some later stage reads
            const int i = rid / p.lut_len, v = p.lut[rid - i * p.lut_len];
            img = i * p.per_image + (v >> 16); ry = (v >> 8) & 255; rx = v & 255;      // origins in 4-pixel tiles
            if (i >= p.n / p.per_image) img = p.n;
            r_img[g] = img < p.n ? img : -1;
            r_y0[g] = ry * 4; r_x0[g] = rx * 4;
            r_win[g] = v >> 16;
            continue;
        } else {
            rx = rid % regs_x;
            const int t = rid / regs_x;
            ry = t % regs_y; img = t / regs_y;
        }
        r_img[g] = img < p.n ? img : -1;
        r_y0[g] = ry * 16; r_x0[g] = rx * 16;
    }

    // input rows / columns the two regions may read (ConvParams::in_box: the receptive field of the needed outputs of a cropped
    // plan; the whole image otherwise) - everything outside reads as zero
    int r_by0[2] = {0, 0}, r_by1[2] = {H - 1, H - 1}, r_bx0[2] = {0, 0}, r_bx1[2] = {W - 1, W - 1};
    if (p.in_box != nullptr) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (r_img[g] < 0) continue;
            const int32_t* bx = p.in_box + 4 * (r_win[g] >= 0 ? r_win[g] : (r_img[g] + p.box_first) % p.per_image);
            r_by0[g] = bx[0]; r_by1[g] = bx[1]; r_bx0[g] = bx[2]; r_bx1[g] = bx[3];
        }
    }
    // ---- halo DMA: every wave fills slots 64 k + lane, k = wave and wave + 12, two groups ahead of its use (3-deep
    //      ring: nobody ever waits for a halo piece to land) ----
    // Round 4: the halo goes through a BUFFER descriptor - a workgroup-uniform base (the first of its two windows) in four SGPRs
    // + one 32-bit byte offset per lane and piece, kept in two registers; lanes that have to read zeros (padding, pixels outside
    // the image, the missing channel half of a Cin % 8 == 4 tail) hold an out-of-range offset and the hardware returns 0 (no zero
    // page); the 8-channel group advances through the instruction's scalar offset.  Rounds 1-3 parked 64-bit pointers in LDS
    // and rebuilt the address of every piece from them: 2 LDS reads + ~20 vector instructions per group - each LDS read beside
    // the MFMA stream costs the matrix pipe ~14 cycles, each vector instruction ~2.2 (tools/micro/mfma_mix.hip).
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const int img_lo = r_img[0] >= 0 ? (r_img[1] >= 0 && r_img[1] < r_img[0] ? r_img[1] : r_img[0]) : (r_img[1] >= 0 ? r_img[1] : 0);
    const unsigned long long hb = (unsigned long long)(size_t)(p.in.p + (size_t)img_lo * H * W * p.in.cs);
    i32x4 hrsrc;                                             // V#: base, stride 0, 2 GB of records, gfx9 raw-buffer word 3
    hrsrc[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)hb);
    hrsrc[1] = __builtin_amdgcn_readfirstlane((int)((unsigned)(hb >> 32) & 0xffffu));
    hrsrc[2] = 0x7fff0000;
    hrsrc[3] = 0x00020000;
    unsigned hoff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int a = 64 * (wave + 12 * i) + lane;
        unsigned off = 0xffffffffu;
        if (a < W4_HALO_L::USED) {
            const int g = a >= W4_HALO_L::REGION ? 1 : 0, rem = a - g * W4_HALO_L::REGION;
            const int r = rem / W4_HALO_L::ROW, cc = rem - r * W4_HALO_L::ROW;
            if (W4_HALO_L::ROW == W4_HALO_L::COLS || cc < W4_HALO_L::COLS) {      // (not a pad slot)
            W4_HALO_SLOT(r, cc);                                 // -> h (channel half), hy / hx (halo row / column 0..17) of slot (r, cc) of the kernel's raw image
            const int img = g ? r_img[1] : r_img[0];
            const int iy = (g ? r_y0[1] : r_y0[0]) - 1 + hy, ix = (g ? r_x0[1] : r_x0[0]) - 1 + hx;
            if (img >= 0 && iy >= (g ? r_by0[1] : r_by0[0]) && iy <= (g ? r_by1[1] : r_by1[0]) && ix >= (g ? r_bx0[1] : r_bx0[0]) &&
                ix <= (g ? r_bx1[1] : r_bx1[0]))                         // (two neighbouring windows: far below 2 GB)
                off = (unsigned)(((((size_t)(img - img_lo) * H + iy) * W + ix) * p.in.cs + 4 * h) * 4);
            }
        }
        hoff[i] = off;
        W4_DIAG_HALO_OFFSET(hoff[i], a);
    }
    auto dma_halo_piece = [&](int grp, auto ii) __attribute__((always_inline)) {            // piece ii (0 | 1) of halo group grp (< ngroups)
        W4_DIAG_SKIP_HALO_DMA();
        constexpr int i = decltype(ii)::value;
        unsigned off = hoff[i];
        if (tail4 && grp == ngroups - 1) {                   // Cin % 8 == 4: the upper channel half of the last group does not exist
            const int a = 64 * (wave + 12 * i) + lane;
            const int cc = W4_HALO_L::REGION % W4_HALO_L::ROW == 0 ? a % W4_HALO_L::ROW : (a - (a >= W4_HALO_L::REGION ? W4_HALO_L::REGION : 0)) % W4_HALO_L::ROW;
            if (W4_HALO_UPPER(cc)) off = 0xffffffffu;
        }
        const unsigned dst = lds_base + (unsigned)((grp % W4_HALO_RING) * W4_HS + 64 * (wave + 12 * i)) * 16u;
        const i32x4 rs = hrsrc;                              // (local copies: asm operands do not capture in a generic lambda)
        const int soff = grp * 32;
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(off), "s"(dst), "s"(rs), "s"(soff) : "memory");
    };
