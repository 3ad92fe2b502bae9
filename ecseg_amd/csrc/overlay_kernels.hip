// Component counts and the meta_overlay row for gfx950: run_count_coloc, run_count_hsr and run_overlay as schedules of labelling
// passes (the engine behind ccl.h), flag queries on their roots and the mask / aux / gather kernels below.  gather_slot_kernel and
// keep_large_kernel are launched from this file alone and stay file-local.
#include "ccl.h"

namespace ecseg {

__global__ void gather_slot_kernel(const int32_t* __restrict__ G_all, int n_img, int slot, int key_for_quirk,
                                   long long full_px, int32_t* __restrict__ out32, long long* __restrict__ out64,
                                   int out_stride, int out_off) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    const int32_t* G = G_all + (size_t)i * G_IMG;
    int v = G[G_CNT0 + slot];
    // np.unique(regs)[1:] (src/image_tools.py:107,129) drops the only component of a mask without background
    if (key_for_quirk && G[G_NPX + key_for_quirk] == full_px) v = 0;
    if (out32) out32[(size_t)i * out_stride + out_off] = v;
    if (out64) out64[(size_t)i * out_stride + out_off] = v;
}
// After a LUT_NONZERO pass with AUX_IMAGE and NEED_NPX on ws.g: the roots whose flag word has bit 0, per image, into
// out32 / out64 [i * stride + off] (either may be null) - one query into slot 0, gathered with the full-mask quirk on key 1
static void count_bit0_roots(PostWorkspace& ws, const CclGeom& g, const uint8_t* key_img, size_t px, int32_t* out32, long long* out64,
                             int stride, int off, hipStream_t s) {
    launch_flagged_counts(ws, g, key_img, LUT_NONZERO, FlagQueries{1, {0}, {1u}, {0}}, s);
    hipLaunchKernelGGL(gather_slot_kernel, dim3((g.n_img + 63) / 64), dim3(64), 0, s, ws.g, g.n_img, 0, 1, (long long)px, out32, out64,
                       stride, off);
}

__global__ __launch_bounds__(256) void mask_to_bits_kernel(const uint8_t* __restrict__ a, uint8_t* __restrict__ out, size_t total) {
    PX_LOOP(total) out[t] = a[t] ? 1 : 0;
}

hipError_t run_count_coloc(PostWorkspace& ws, const uint8_t* ob1, const uint8_t* ob2, int n_img, int H, int W, int32_t* n_dev,
                           hipStream_t s) {
    if (n_img <= 0) return hipSuccess;
    const CclGeom g = make_geom(n_img, H, W);
    const size_t px = (size_t)H * W, total = px * n_img;
    hipLaunchKernelGGL(mask_to_bits_kernel, dim3(px_grid(total)), dim3(256), 0, s, ob2, ws.tmpA, total);
    CclPass p{ob1, LUT_NONZERO, 8, 0, AUX_IMAGE, 0, ws.tmpA, NEED_NPX};
    hipError_t e = run_ccl_pass(ws, g, p, s);
    if (e != hipSuccess) return e;
    count_bit0_roots(ws, g, ob1, px, n_dev, nullptr, 1, 0, s);
    return hipGetLastError();
}

// remove_small_objects(fish, thr) on a bool image: 4-connected components with area < thr are dropped
__global__ __launch_bounds__(256) void keep_large_kernel(const int32_t* __restrict__ L, const uint32_t* __restrict__ area,
                                                         uint8_t* __restrict__ out, size_t total, size_t px, int thr, int bit) {
    PX_LOOP(total) {
        const int o = L[t];                                    // (non-sparse labelling: unkeyed pixels hold -1)
        uint8_t v = out[t];
        if (o >= 0) {
            const size_t ib = (t / px) * px;
            if (area[ib + L[ib + o]] >= (uint32_t)thr) v |= (uint8_t)(1u << bit);
        }
        out[t] = v;
    }
}

__global__ __launch_bounds__(256) void zero_u8_kernel(uint8_t* __restrict__ out, size_t total) {
    PX_LOOP(total) out[t] = 0;
}

hipError_t run_count_hsr(PostWorkspace& ws, const uint8_t* chrom, const uint8_t* fish, int n_img, int H, int W, int thr,
                         int32_t* n_dev, hipStream_t s) {
    if (n_img <= 0) return hipSuccess;
    const CclGeom g = make_geom(n_img, H, W);
    const size_t px = (size_t)H * W, total = px * n_img;
    CclPass p1{fish, LUT_NONZERO, 4, STAT_AREA, AUX_NONE, 0, nullptr, 0};
    hipError_t e = run_ccl_pass(ws, g, p1, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(zero_u8_kernel, dim3(px_grid(total)), dim3(256), 0, s, ws.tmpA, total);
    hipLaunchKernelGGL(keep_large_kernel, dim3(px_grid(total)), dim3(256), 0, s, ws.L, ws.area, ws.tmpA, total, px, thr, 0);
    CclPass p2{chrom, LUT_NONZERO, 8, 0, AUX_IMAGE, 0, ws.tmpA, NEED_NPX};
    if ((e = run_ccl_pass(ws, g, p2, s)) != hipSuccess) return e;
    count_bit0_roots(ws, g, chrom, px, n_dev, nullptr, 1, 0, s);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// meta_overlay row (src/meta_overlay.py:59-95)
// ---------------------------------------------------------------------------------------------------------------
// which: 0 fish  = green & ~nuclei      1 fish2 = red & ~nuclei
//        2 A     = fish  & ~chrom       3 B     = fish2 & ~chrom
__global__ __launch_bounds__(256) void overlay_mask_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ rgb,
                                                           int C, int sens, int which, uint8_t* __restrict__ out, size_t total) {
    PX_LOOP(total) {
        const uint8_t v = labels[t];
        const bool red = rgb[t * C + 0] > sens, green = rgb[t * C + 1] > sens;
        bool m = (which & 1) ? red : green;
        m = m && v != 1;
        if (which >= 2) m = m && v != 2;
        out[t] = m ? 1 : 0;
    }
}

// aux bits for the (chromosome, ecDNA) labelling: bit0 fish, bit1 fish2, bit2 fish & fish2 (ecDNA colocalisation);
// bits 3 / 4 (size-filtered fish2 / fish, for HSR) are OR-ed in afterwards by keep_large_kernel.
// The first kernel of the row also folds label bytes above 3 to 0 in the driver's copy of the labels: the reference takes
// nuclei / chromosomes / ecDNA as labels == 1 / 2 / 3, so such a byte is background, while key_of looks at the low two
// bits only (6 would be labelled as a chromosome, 7 and 255 as ecDNA).  A store happens only for such a byte, and it comes
// last: in front of the colour loads it made them wait for the label byte (two memory round trips per pixel instead of one).
__global__ __launch_bounds__(256) void overlay_aux_kernel(uint8_t* __restrict__ labels, const uint8_t* __restrict__ rgb,
                                                          int C, int sens, uint8_t* __restrict__ aux, size_t total) {
    PX_LOOP(total) {
        const uint8_t v = labels[t];
        const bool fish2 = rgb[t * C + 0] > sens && v != 1, fish = rgb[t * C + 1] > sens && v != 1;
        aux[t] = (uint8_t)((fish ? 1 : 0) | (fish2 ? 2 : 0) | ((fish && fish2) ? 4 : 0));
        if (v > 3) labels[t] = 0;
    }
}

__global__ void overlay_cc_gather_kernel(const int32_t* __restrict__ G_all, int n_img, int key, long long full_px,
                                         long long* __restrict__ out, int off) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    const int n = G_all[(size_t)i * G_IMG + G_NCOMP + key];
    const long long px = G_all[(size_t)i * G_IMG + G_NPX + key];
    out[(size_t)i * 12 + off] = n;
    out[(size_t)i * 12 + off + 1] = (n == 0 || px == full_px) ? -1 : px;
}

hipError_t run_overlay(PostWorkspace& ws, uint8_t* labels, const uint8_t* rgb, int n_img, int H, int W, int C, int sens,
                       int hsr_thr, long long* out, hipStream_t s) {
    if (n_img <= 0) return hipSuccess;
    const CclGeom g = make_geom(n_img, H, W);
    const size_t px = (size_t)H * W, total = px * n_img;
    const unsigned pg = px_grid(total);
    const unsigned ig = (n_img + 63) / 64;
    uint8_t* aux = ws.tmpB;    // flag bits for the (chrom, ec) labelling
    uint8_t* msk = ws.tmpA;    // mask being labelled
    hipError_t e;
    hipLaunchKernelGGL(overlay_aux_kernel, dim3(pg), dim3(256), 0, s, labels, rgb, C, sens, aux, total);
    // HSR: size-filtered fish2 (red) -> bit3, fish (green) -> bit4   (4-connectivity, src/image_tools.py:104)
    for (int k = 0; k < 2; ++k) {
        const int which = (k == 0) ? 1 : 0;
        hipLaunchKernelGGL(overlay_mask_kernel, dim3(pg), dim3(256), 0, s, labels, rgb, C, sens, which, msk, total);
        CclPass p{msk, LUT_NONZERO, 4, STAT_AREA, AUX_NONE, 0, nullptr, 0};
        if ((e = run_ccl_pass(ws, g, p, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(keep_large_kernel, dim3(pg), dim3(256), 0, s, ws.L, ws.area, aux, total, px, hsr_thr, 3 + k);
    }
    // chromosomes (key 2) and ecDNA (key 3) in one labelling
    {
        const uint32_t lut = 0x03020000u;
        CclPass p{labels, lut, 8, 0, AUX_IMAGE, 0, aux, NEED_NCOMP | NEED_NPX};
        if ((e = run_ccl_pass(ws, g, p, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(overlay_cc_gather_kernel, dim3(ig), dim3(64), 0, s, ws.g, n_img, 3, (long long)px, out, 0);
        const struct { int key; uint32_t need; int slot; int off; } q[5] = {
            {3, 1u, 0, 6}, {3, 2u, 1, 7}, {3, 4u, 2, 9}, {2, 8u, 3, 10}, {2, 16u, 4, 11}};
        FlagQueries Q{5, {}, {}, {}};
        for (int k = 0; k < 5; ++k) { Q.key[k] = q[k].key; Q.need[k] = q[k].need; Q.slot[k] = q[k].slot; }
        launch_flagged_counts(ws, g, labels, lut, Q, s);
        for (int k = 0; k < 5; ++k) {
            hipLaunchKernelGGL(gather_slot_kernel, dim3(ig), dim3(64), 0, s, ws.g, n_img, q[k].slot, q[k].key, (long long)px,
                               (int32_t*)nullptr, out, 12, q[k].off);
        }
    }
    // A = fish & ~chrom: count_cc(A), coloc(A, B)
    {
        hipLaunchKernelGGL(overlay_mask_kernel, dim3(pg), dim3(256), 0, s, labels, rgb, C, sens, 2, msk, total);
        hipLaunchKernelGGL(overlay_mask_kernel, dim3(pg), dim3(256), 0, s, labels, rgb, C, sens, 3, aux, total);
        CclPass p{msk, LUT_NONZERO, 8, 0, AUX_IMAGE, 0, aux, NEED_NCOMP | NEED_NPX};
        if ((e = run_ccl_pass(ws, g, p, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(overlay_cc_gather_kernel, dim3(ig), dim3(64), 0, s, ws.g, n_img, 1, (long long)px, out, 2);
        count_bit0_roots(ws, g, msk, px, nullptr, out, 12, 8, s);
    }
    // B = fish2 & ~chrom: count_cc(B)
    {
        CclPass p{aux, LUT_NONZERO, 8, 0, AUX_NONE, 0, nullptr, NEED_NCOMP | NEED_NPX};
        if ((e = run_ccl_pass(ws, g, p, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(overlay_cc_gather_kernel, dim3(ig), dim3(64), 0, s, ws.g, n_img, 1, (long long)px, out, 4);
    }
    return hipGetLastError();
}

}  // namespace ecseg
