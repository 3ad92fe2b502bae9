// The interSeg drivers (src/interseg.py:113-235; kernels in interseg_kernels.hip): the regions of a nucleus mask, which leave their
// label map and image on the handle, and the crops cut from those.
#include "driver_util.h"

using namespace ecseg;

extern "C" {

int ecseg_nuclei_regions(ecseg_ctx* h, const uint8_t* seg, int H, int W, const uint8_t* img, int img_h, int img_w, int C,
                         int channel0, int capacity, int64_t* records, int32_t* n_regions) {
    DRIVER_OPEN(h);
    h->iseg_n = -1;
    if (!seg || !img || !n_regions || H <= 0 || W <= 0 || img_h < H || img_w < W || C < 1 || channel0 < 0 || channel0 >= C ||
        capacity < 0 || (capacity > 0 && !records))
        return fail(h, ECSEG_E_INVALID, "nuclei_regions: bad arguments (the segmentation must not be larger than the image)");
    if (!px_below_2_31(H, W) || (long long)H * img_w * C >= (1ll << 40)) return fail(h, ECSEG_E_INVALID, "image too large");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W, img_bytes = (size_t)H * img_w * C;
    int rc;
    RegionBufs b{};
    if ((rc = ensure_post(h, 1, px))) return rc;
    if ((rc = h->d_gray.ensure(h, px))) return rc;
    if ((rc = lay_out(h, h->keep_arena, [&](Carver& c) { h->iseg = region_map_bufs(c, H, W, img_w, C); }))) return rc;
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = region_bufs(c, H, W, capacity); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(h->d_gray, seg, px, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(h->iseg.img, img, img_bytes, hipMemcpyHostToDevice, s));   // the first H rows: I[:imheight, :imwidth]
    TIMED(h, s, 0, 1,
          HIP_TRY(h, run_ccl_labels(h->ws, h->d_gray, 1, H, W, 8, h->iseg.lab, s));
          HIP_TRY(h, run_nuclei_regions(h->d_gray, h->iseg.img, H, W, img_w, C, channel0, h->iseg.lab, b, s)));
    int32_t misc[4];
    HIP_TRY(h, hipMemcpyAsync(misc, b.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);
    const int n = misc[0], vmax = misc[1], vmin = 255 - misc[2];
    if (n > 0 && vmin != vmax)
        return fail(h, ECSEG_E_INVALID, "segmentation holds the non-zero values " + std::to_string(vmin) + " .. " + std::to_string(vmax) +
                                            ": only 0 / non-zero nucleus masks are supported, not instance-id maps");
    *n_regions = n;
    if (n <= capacity && n > 0) {
        HIP_TRY(h, hipMemcpyAsync(records, b.rec, (size_t)n * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    h->iseg_H = H; h->iseg_W = W; h->iseg_img_w = img_w; h->iseg_C = C; h->iseg_n = n;
    return ECSEG_OK;
}

int ecseg_nucleus_crops(ecseg_ctx* h, const int32_t* crops, int n_crops, const int32_t* channel_order, uint8_t* out,
                        int32_t* channel_max) {
    DRIVER_OPEN(h);
    if (n_crops < 0 || (n_crops > 0 && (!crops || !channel_order || !out || !channel_max)))
        return fail(h, ECSEG_E_INVALID, "nucleus_crops: bad arguments");
    if (n_crops == 0) return ECSEG_OK;
    if (h->iseg_n < 0) return fail(h, ECSEG_E_INVALID, "nucleus_crops: no region map on the handle (call ecseg_nuclei_regions first)");
    int order[3];
    for (int c = 0; c < 3; ++c) {
        order[c] = channel_order[c];
        if (order[c] < 0 || order[c] >= h->iseg_C) return fail(h, ECSEG_E_INVALID, "nucleus_crops: channel_order out of range");
    }
    for (int k = 0; k < n_crops; ++k) {
        const int32_t* d = crops + (size_t)k * 5;
        if (d[0] < 0 || d[0] >= h->iseg_n || d[1] < 0 || d[2] < 0 || d[3] < 1 || d[3] > 256 || d[4] < 1 || d[4] > 256 ||
            d[1] > h->iseg_H - d[3] || d[2] > h->iseg_W - d[4])
            return fail(h, ECSEG_E_INVALID, "nucleus_crops: crop " + std::to_string(k) + " is not a 1..256 x 1..256 window of a region");
    }
    USE_DEVICE(h);
    const int chunk = 256;                                   // 48 MiB of crops per launch
    const size_t crop_bytes = (size_t)256 * 256 * 3;
    const int nc = std::min(n_crops, chunk);
    int rc;
    CropBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = crop_bufs(c, nc); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    for (int k0 = 0; k0 < n_crops; k0 += chunk) {
        const int k = std::min(chunk, n_crops - k0);
        HIP_TRY(h, hipMemcpyAsync(b.desc, crops + (size_t)k0 * 5, (size_t)k * 5 * sizeof(int32_t), hipMemcpyHostToDevice, s));
        TIMED(h, s, 0, 1, HIP_TRY(h, run_nucleus_crops(h->iseg.lab, h->iseg.img, h->iseg_W, h->iseg_img_w, h->iseg_C, b.desc, k, order, b.crops, b.max, s)));
        HIP_TRY(h, hipMemcpyAsync(out + (size_t)k0 * crop_bytes, b.crops, (size_t)k * crop_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(channel_max + (size_t)k0 * 3, b.max, (size_t)k * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        WAIT_ADD(h, s, 0, 1);
    }
    return ECSEG_OK;
}

}  // extern "C"
