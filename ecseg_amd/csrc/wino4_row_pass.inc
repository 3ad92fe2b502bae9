// The row transform of conv_wino4r_kernel / conv_wino4s_kernel, ONCE per workgroup and 8-channel group, included inside the kernel body:
// all 768 threads turn the raw halo into the t image (t[xi][j] = B^T[xi,:] d[:,j]); a wave then reads the columns of ITS row (load_t).
// Expects: smem, wave, lane, W4_HS (the t image follows two raw buffers); defines rp_raw, rp_t, row_pass(grp).
//
// This file is the one statement of the transform's operation order: t[xi] = c0 d[r0] + c1 d[r1] + c2 d[r2] + d[r3] as ONE fma chain per row,
// innermost term first - fma(c0, d[r0], fma(c1, d[r1], fma(c2, d[r2], d[r3]))), rows 0 and 5 with three terms - which is also the order of
// the per-wave row transform of conv_wino4_kernel (wino4_kernel.hip: transform).  Every F(4x4) kernel therefore forms bit-identical t, and
// the fp32 kernels bit-identical results.  (A first version shared the even / odd parts of the +- rows, 12 instead of 16 fmas per channel:
// the smooth fixture model's wrong-pixel total rose from 11 to 19 of ~15 hard pixels per image.)
//
// History (round 6, EXPERIMENTS.md): before, every wave read the raw halo rows of its transform row itself - in conv_wino4s_kernel 20
// ds_read_b128 per wave and group, 240 KB of LDS reads per group for 21 KB of data, and with the channel sum three times faster that traffic
// (+ 144 KB of filter reads + 134 KB of LDS-DMA writes = 518 KB at 128 B / clock) - not the matrix pipe, not the vector pipe - set the pace
// (tools/experiments/w4s_ablate.sh).  Now: raw 28 KB + t 28 KB written + 60 KB read.

    // row_pass's item and its two LDS byte addresses (raw buffer 0, transform row 0) do not depend on the group: formed once and pinned - left alone the
    // compiler rebuilds them (~20 vector instructions beside the MFMA stream) in every copy of the pass
    unsigned rp_raw, rp_t;
    {
        const int item = wave * 48 + lane, cpair = item & 1, h = (item >> 1) & 1, k = item >> 2;
        const int x = k % 18, r2 = k / 18, tyy = r2 & 3, tgg = r2 >> 2;
        rp_raw = (unsigned)(W4Lds::raw_read(0, tgg, tyy, x, h) * 16 + cpair * 8);
        rp_t = (unsigned)((2 * W4_HS + W4Lds::t_write(tgg, tyy, h, x)) * 16 + cpair * 8);
        asm volatile("" : "+v"(rp_raw), "+v"(rp_t));
    }
    auto row_pass = [&](int grp) __attribute__((always_inline)) {
        // 576 half items (region, tile row, channel half, column, channel PAIR) over the 12 waves x 48 lanes: every wave carries the
        // same share (a pass run by five waves alone left the other seven waiting at the barrier behind it), 8-byte accesses,
        // neighbouring lanes on neighbouring addresses
        if (lane >= 48) return;
        const f32x2* R = reinterpret_cast<const f32x2*>(smem + rp_raw + (unsigned)(W4Lds::raw_read(grp & 1, 0, 0, 0, 0) * 16));     // raw row 4 tyy + i: + i rows
        constexpr int RR = 2 * W4Lds::raw_row();
        const f32x2 d0 = R[RR * 0], d1 = R[RR * 1], d2 = R[RR * 2], d3 = R[RR * 3], d4 = R[RR * 4], d5 = R[RR * 5];
        f32x2* T = reinterpret_cast<f32x2*>(smem + rp_t);                            // + xi transform rows
        f32x2 o;
#define W4_ROW3(XI, A0, DA, A1, DB, DC) do { _Pragma("unroll") for (int c = 0; c < 2; ++c) o[c] = __builtin_fmaf(A0, DA[c], __builtin_fmaf(A1, DB[c], DC[c])); T[2 * (XI) * W4Lds::t_xi()] = o; } while (0)
#define W4_ROW4(XI, A0, DA, A1, DB, A2, DC, DD) do { _Pragma("unroll") for (int c = 0; c < 2; ++c) \
            o[c] = __builtin_fmaf(A0, DA[c], __builtin_fmaf(A1, DB[c], __builtin_fmaf(A2, DC[c], DD[c]))); T[2 * (XI) * W4Lds::t_xi()] = o; } while (0)
        W4_ROW3(0, KP, d0, KS, d2, d4);
        W4_ROW3(5, KP, d1, KS, d3, d5);
        W4_ROW4(1, -KA * KB2, d1, -KB2, d2, KA, d3, d4);
        W4_ROW4(2, KA * KB2, d1, -KB2, d2, -KA, d3, d4);
        W4_ROW4(3, -KA2 * KB, d1, -KA2, d2, KB, d3, d4);
        W4_ROW4(4, KA2 * KB, d1, -KA2, d2, -KB, d3, d4);
#undef W4_ROW3
#undef W4_ROW4
    };
