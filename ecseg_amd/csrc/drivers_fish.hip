// The FISH drivers: the per-nucleus distances (fishdist_kernels.hip), stat_fish's spots and its three colour files
// (fishspot_kernels.hip; as TIFF files through tiff_collect of drivers_files.hip) and the min-cut tasks (mincut_kernels.hip).
#include <algorithm>

#include "driver_util.h"

using namespace ecseg;

// The opening phase of ecseg_fish_distances and ecseg_fish_spots: the label map and the image on the device, the dense cell index
// (stage_ms[ECSEG_T_COUNT] = its device time) and the number of cells.  `who` prefixes the refusal of a label above H * W.  `b`
// lies in the call arena: what the caller sizes by the cell count goes to the count arena.
static int open_dense_cells(ecseg_ctx* h, const char* who, const int32_t* labels, int H, int W, const uint8_t* img, int C, CellIndexBufs& b,
                            int32_t* n_cells) {
    const size_t px = (size_t)H * W;
    if (int rc = lay_out(h, h->call_arena, [&](Carver& c) { b = cell_index_bufs(c, H, W, C); })) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(b.lab, labels, px * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.img, img, px * C, hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_dense_cells(b.lab, H, W, b, s)));
    int32_t misc[4];
    HIP_TRY(h, hipMemcpyAsync(misc, b.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);
    if (misc[3])
        return fail(h, ECSEG_E_INVALID, std::string(who) + ": the label map holds a label larger than H * W = " + std::to_string(px) +
                                            " (renumber the labels by rank first)");
    *n_cells = misc[0];
    return ECSEG_OK;
}

// the argument rules ecseg_fish_render and ecseg_fish_render_tiff share; ch: the validated channel indices
static int fish_render_check(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels, const uint8_t* thresholded,
                             int n_probe, const uint8_t* boundaries, int ch[4]) {
    if (!img || !channels || !thresholded || !boundaries || H <= 0 || W <= 0) return fail(h, ECSEG_E_INVALID, "fish_render: bad arguments");
    if (C < 3 || C > 4) return fail(h, ECSEG_E_INVALID, "fish_render: the image must have 3 or 4 channels, not " + std::to_string(C));
    if (n_probe != C - 1)
        return fail(h, ECSEG_E_INVALID, "fish_render: n_probe must be C - 1 = " + std::to_string(C - 1) + " (one mask per FISH channel)");
    for (int j = 0; j < 4; ++j) ch[j] = 0;
    for (int j = 0; j < C; ++j) {
        ch[j] = channels[j];
        if (ch[j] < 0 || ch[j] >= C)
            return fail(h, ECSEG_E_INVALID, "fish_render: channel index out of range (the image has " + std::to_string(C) + " channels)");
    }
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, "fish_render: image too large (H * W must be below 2^31)");
    return ECSEG_OK;
}

// One group of ecseg_fish_distances_batch: consecutive images of the chunk that share one pass over the driver's own scratch buffer
// (fishdist_batch.h).  The buffer is carved in two parts with the arenas' three steps - measure, ensure, place - written out here:
// it is no arena of ctx.h and joins none of their rows.
struct FdbRun { FdbLayout L; FdbPixelBufs b; std::vector<int32_t> plan; int cells = 0; };

// The first part: measured TOGETHER with the most the second part can need (the buffer must not grow while the first part is in
// use), grown if need be, placed; then the uploads, the dense cell index of the whole group and the plan on the host.
static int fdb_open_group(ecseg_ctx* h, const int32_t* const* labels, const uint8_t* const* lsqs, const int32_t* shapes, FdbGroup g, int capacity,
                          FdbRun& r) {
    const std::string me = "fish_distances_batch: ";
    const std::string bad = fdb_layout(shapes, g.first, g.n, r.L);
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    const size_t n = (size_t)g.n, bound = (size_t)fdb_cell_bound(r.L.px, capacity);
    Carver measure;
    (void)fdb_pixel_bufs(measure, r.L);
    if ((long long)measure.used != fdb_pixel_bytes(r.L)) return fail(h, ECSEG_E_INVALID, me + "fdb_pixel_bytes does not restate fdb_pixel_bufs");
    (void)fdb_cell_bufs(measure, bound, bound + FDB_SLICE_BUDGET);
    if ((long long)measure.used != fdb_group_bytes(r.L, capacity)) return fail(h, ECSEG_E_INVALID, me + "fdb_group_bytes does not restate the two parts");
    if (int rc = h->fishdist_batch_buf.ensure(h, measure.used)) return rc;
    Carver place(h->fishdist_batch_buf.p);
    r.b = fdb_pixel_bufs(place, r.L);
    hipStream_t s = h->stream;
    for (size_t k = 0; k < n; ++k) {
        const FdbImage& t = r.L.tab[k];
        const size_t px = (size_t)t.H * t.W;
        HIP_TRY(h, hipMemcpyAsync(r.b.lab + t.px0, labels[(size_t)g.first + k], px * sizeof(int32_t), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(r.b.lsq + t.lsq0, lsqs[(size_t)g.first + k], px * t.C, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(h, hipMemcpyAsync(r.b.tab, r.L.tab.data(), n * sizeof(FdbImage), hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_fishdist_batch_open(r.L, r.b, s)));
    r.plan.assign((n + 1) * 2, 0);
    HIP_TRY(h, hipMemcpyAsync(r.plan.data(), r.b.plan, r.plan.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));   // every image's cells in one copy
    WAIT_ADD(h, s, 0, 1);
    r.cells = r.plan[2 * n];
    return ECSEG_OK;
}

// The second part, carved behind the first now that the group's cells are known, and the group's records at `records`
static int fdb_finish_group(ecseg_ctx* h, const FdbRun& r, int fi, int ci, int64_t* records) {
    if (r.cells == 0) return ECSEG_OK;
    const size_t cells = (size_t)r.cells;
    Carver place(h->fishdist_batch_buf.p);
    (void)fdb_pixel_bufs(place, r.L);
    const FdbCellBufs c = fdb_cell_bufs(place, cells, cells * (size_t)fishdist_slices(r.cells));
    if (place.used > h->fishdist_batch_buf.cap) return fail(h, ECSEG_E_INVALID, "fish_distances_batch: the second part leaves the measured buffer");
    hipStream_t s = h->stream;
    TIMED(h, s, 2, 3, HIP_TRY(h, run_fishdist_batch_records(r.L, r.b, c, r.cells, fi, ci, s)));
    HIP_TRY(h, hipMemcpyAsync(records, c.rec, cells * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    WAIT_ADD(h, s, 2, 3);
    return ECSEG_OK;
}

extern "C" {

// ---- fish_distance_calculation (src/fish_distance_calculation.py:16-46) ---------------------------------------------------
int ecseg_fish_distances(ecseg_ctx* h, const int32_t* labels, int H, int W, const uint8_t* lsq, int C, int fish_channel,
                         int centromere_channel, int capacity, int64_t* records, int32_t* n_cells) {
    DRIVER_OPEN(h);
    if (n_cells) *n_cells = 0;
    if (!labels || !lsq || !n_cells || H <= 0 || W <= 0 || capacity < 0 || (capacity > 0 && !records))
        return fail(h, ECSEG_E_INVALID, "fish_distances: bad arguments");
    if (C < 2) return fail(h, ECSEG_E_INVALID, "fish_distances: the lsq image needs at least 2 channels (the gate reads channels 0 and 1)");
    if (fish_channel < 0 || fish_channel >= C || centromere_channel < 0 || centromere_channel >= C)
        return fail(h, ECSEG_E_INVALID, "fish_distances: channel out of range (the lsq image has " + std::to_string(C) + " channels)");
    if (!px_below_2_31(H, W) || (long long)H * W * C >= (1ll << 40))
        return fail(h, ECSEG_E_INVALID, "fish_distances: image too large (H * W must be below 2^31, H * W * C below 2^40)");
    USE_DEVICE(h);
    int rc;
    CellIndexBufs cells{};
    if ((rc = open_dense_cells(h, "fish_distances", labels, H, W, lsq, C, cells, n_cells))) return rc;
    const int n = *n_cells;
    if (n == 0 || n > capacity) return ECSEG_OK;             // the cell count alone: the caller comes back with a larger buffer
    // the rest is sized by the number of cells, which is known only now
    FishDistBufs b{};
    if ((rc = lay_out(h, h->count_arena, [&](Carver& c) { b = fishdist_bufs(c, cells, H, W, n, fishdist_slices(n)); }))) return rc;
    hipStream_t s = h->stream;
    TIMED(h, s, 2, 3, HIP_TRY(h, run_fishdist_records(cells.lab, cells.img, H, W, C, fish_channel, centromere_channel, n, b, s)));
    HIP_TRY(h, hipMemcpyAsync(records, b.rec, (size_t)n * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    WAIT_ADD(h, s, 2, 3);
    return ECSEG_OK;
}


// ---- fish_distance_calculation.batch: the same for a chunk of images in one call (layout: fishdist_batch.h) ----------------------
int ecseg_fish_distances_batch(ecseg_ctx* h, int n_images, const int32_t* const* labels, const uint8_t* const* lsqs, const int32_t* shapes,
                               int fish_channel, int centromere_channel, int record_capacity, int64_t* records, int32_t* n_cells,
                               int32_t* status) {
    DRIVER_OPEN(h);
    static_assert(FDB_MAX_IMAGES == ECSEG_FISH_DISTANCES_BATCH_MAX_IMAGES, "fishdist_batch.h and the header disagree");
    const std::string me = "fish_distances_batch: ";
    if (n_images < 0 || record_capacity < 0 || (record_capacity > 0 && !records) || (n_images > 0 && (!labels || !lsqs || !shapes || !n_cells || !status)))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    clear_timings(h);
    if (n_images == 0) return ECSEG_OK;
    if (n_images > FDB_MAX_IMAGES) return fail(h, ECSEG_E_INVALID, me + "more than " + std::to_string(FDB_MAX_IMAGES) + " images");
    FdbRun run;
    const std::string bad = fdb_layout(shapes, 0, n_images, run.L);          // the limits of the whole chunk
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    for (int i = 0; i < n_images; ++i) {
        const std::string who = me + "image " + std::to_string(i) + ": ";
        const int C = shapes[3 * (size_t)i + 2];
        if (!labels[i] || !lsqs[i]) return fail(h, ECSEG_E_INVALID, who + "bad arguments (no label map or no lsq image)");
        if (fish_channel < 0 || fish_channel >= C || centromere_channel < 0 || centromere_channel >= C)
            return fail(h, ECSEG_E_INVALID, who + "channel out of range (the lsq image has " + std::to_string(C) + " channels)");
        n_cells[i] = 0;
        status[i] = ECSEG_OK;
    }
    const std::vector<FdbGroup> groups = fdb_groups(shapes, n_images, record_capacity);
    USE_DEVICE(h);
    int rc;
    // the counts first: of the only group on its way, of several groups in a pass of their own (nothing is written above the capacity)
    long long total = 0;
    for (const FdbGroup& g : groups) {
        if ((rc = fdb_open_group(h, labels, lsqs, shapes, g, record_capacity, run))) return rc;
        for (int k = 0; k < g.n; ++k) {
            n_cells[g.first + k] = run.plan[2 * (size_t)k + 2] - run.plan[2 * (size_t)k];
            status[g.first + k] = run.plan[2 * (size_t)k + 1] ? ECSEG_E_INVALID : ECSEG_OK;
        }
        total += run.cells;
    }
    if (total > record_capacity) return ECSEG_OK;            // the counts alone: the caller comes back with a larger buffer
    long long at = 0;
    for (const FdbGroup& g : groups) {
        if (groups.size() > 1 && (rc = fdb_open_group(h, labels, lsqs, shapes, g, record_capacity, run))) return rc;
        if ((rc = fdb_finish_group(h, run, fish_channel, centromere_channel, records + at * 8))) return rc;
        at += run.cells;
    }
    return ECSEG_OK;
}

// ---- stat_fish behind nuclei_segment (src/stat_fish.py:73-107,134-142,226-300) --------------------------------------------------
int ecseg_fish_spots(ecseg_ctx* h, const int32_t* labels, int H, int W, const uint8_t* img, int C, const int32_t* probe_channels,
                     int n_probe, const double* weights, int K, double normal_threshold, const double* intensity_thresholds,
                     int min_cc_size, int line_thickness, int capacity, uint8_t* thresholded, uint8_t* boundaries,
                     int64_t* records, int32_t* n_cells) {
    DRIVER_OPEN(h);
    if (n_cells) *n_cells = 0;
    if (!labels || !img || !probe_channels || !weights || !intensity_thresholds || !thresholded || !boundaries || !n_cells || H <= 0 ||
        W <= 0 || C < 1 || capacity < 0 || (capacity > 0 && !records))
        return fail(h, ECSEG_E_INVALID, "fish_spots: bad arguments");
    if (n_probe < 1 || n_probe > 3) return fail(h, ECSEG_E_INVALID, "fish_spots: n_probe must be 1, 2 or 3");
    int ch[3] = {0, 0, 0};
    double ithr[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < n_probe; ++j) {
        ch[j] = probe_channels[j];
        ithr[j] = intensity_thresholds[j];
        if (ch[j] < 0 || ch[j] >= C)
            return fail(h, ECSEG_E_INVALID, "fish_spots: probe channel out of range (the image has " + std::to_string(C) + " channels)");
    }
    if (K < 1 || K > ECSEG_FISH_SPOT_MAX_KERNEL || K % 2 == 0)
        return fail(h, ECSEG_E_INVALID, "fish_spots: the kernel side must be odd and between 1 and " + std::to_string(ECSEG_FISH_SPOT_MAX_KERNEL));
    if (line_thickness < 1 || line_thickness > ECSEG_FISH_SPOT_MAX_LINE)
        return fail(h, ECSEG_E_INVALID, "fish_spots: line_thickness must be between 1 and " + std::to_string(ECSEG_FISH_SPOT_MAX_LINE));
    if (!px_below_2_31(H, W) || (long long)H * W * C >= (1ll << 40))
        return fail(h, ECSEG_E_INVALID, "fish_spots: image too large (H * W must be below 2^31, H * W * C below 2^40)");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W, np = (size_t)n_probe;
    int rc;
    CellIndexBufs cells{};
    if ((rc = open_dense_cells(h, "fish_spots", labels, H, W, img, C, cells, n_cells))) return rc;
    const int n = *n_cells;
    if (n > capacity) return ECSEG_OK;                       // the cell count alone: the caller comes back with a larger buffer
    if (n == 0) {                                            // no cell: nothing is thresholded and no rank differs from 0
        std::fill(thresholded, thresholded + px * np, (uint8_t)0);
        std::fill(boundaries, boundaries + px, (uint8_t)0);
        return ECSEG_OK;
    }
    FishSpotBufs b{};
    if ((rc = lay_out(h, h->count_arena, [&](Carver& c) { b = fishspot_bufs(c, cells, H, W, n_probe, K, n); }))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(b.w, weights, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice, s));
    TIMED(h, s, 2, 3, HIP_TRY(h, run_fishspot(cells.lab, cells.img, H, W, C, n_probe, ch, b.w, K, normal_threshold, ithr, min_cc_size, line_thickness, n, b, s)));
    HIP_TRY(h, hipMemcpyAsync(thresholded, b.thr, px * np, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(boundaries, b.bnd, px, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(records, b.rec, (size_t)n * ECSEG_FISH_SPOT_INT64 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    WAIT_ADD(h, s, 2, 3);
    return ECSEG_OK;
}

// ---- stat_fish's three colour files (src/stat_fish.py:110-115,295-300) ------------------------------------------------------------
int ecseg_fish_render(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels, const uint8_t* thresholded,
                      int n_probe, const uint8_t* boundaries, uint8_t* original, uint8_t* with_segmentation, uint8_t* lsq) {
    DRIVER_OPEN(h);
    if (!original || !with_segmentation || !lsq) return fail(h, ECSEG_E_INVALID, "fish_render: bad arguments");
    int ch[4], rc;
    if ((rc = fish_render_check(h, img, H, W, C, channels, thresholded, n_probe, boundaries, ch))) return rc;
    USE_DEVICE(h);
    const size_t px = (size_t)H * W;
    FishRenderBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = fish_render_bufs(c, H, W, C); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(b.img, img, px * C, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.thr, thresholded, px * n_probe, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.bnd, boundaries, px, hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_fish_render(H, W, C, ch, b, s)));
    HIP_TRY(h, hipMemcpyAsync(original, b.orig, px * 3, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(with_segmentation, b.seg, px * 3, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(lsq, b.lsq, px * 3, hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);
    return ECSEG_OK;
}

// the same, and the three images as TIFF files encoded on the device: here the raw images are optional
int ecseg_fish_render_tiff(ecseg_ctx* h, const uint8_t* img, int H, int W, int C, const int32_t* channels, const uint8_t* thresholded,
                           int n_probe, const uint8_t* boundaries, uint8_t* const* files, long long file_cap, long long* file_bytes,
                           uint8_t* original, uint8_t* with_segmentation, uint8_t* lsq) {
    DRIVER_OPEN(h);
    if (!files || !files[0] || !files[1] || !files[2] || !file_bytes || file_cap < 0) return fail(h, ECSEG_E_INVALID, "fish_render_tiff: bad arguments");
    int ch[4], rc;
    if ((rc = fish_render_check(h, img, H, W, C, channels, thresholded, n_probe, boundaries, ch))) return rc;
    if (!tiff_args_ok(H, W, 3)) return fail(h, ECSEG_E_INVALID, "fish_render_tiff: the TIFF writer takes lines below 2^30 bytes");
    file_bytes[0] = file_bytes[1] = file_bytes[2] = 0;
    USE_DEVICE(h);
    const size_t px = (size_t)H * W;
    FishRenderBufs b{};
    TiffEncodeBufs t{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = fish_render_bufs(c, H, W, C); t = tiff_encode_bufs(c, H, W, 3, 3, false); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(b.img, img, px * C, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.thr, thresholded, px * n_probe, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.bnd, boundaries, px, hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1,
          HIP_TRY(h, run_fish_render(H, W, C, ch, b, s));
          HIP_TRY(h, run_tiff_encode(TiffSources{{b.orig, b.seg, b.lsq}, 0}, 3, H, W, 3, 0, t, s)));
    if (original) HIP_TRY(h, hipMemcpyAsync(original, b.orig, px * 3, hipMemcpyDeviceToHost, s));
    if (with_segmentation) HIP_TRY(h, hipMemcpyAsync(with_segmentation, b.seg, px * 3, hipMemcpyDeviceToHost, s));
    if (lsq) HIP_TRY(h, hipMemcpyAsync(lsq, b.lsq, px * 3, hipMemcpyDeviceToHost, s));
    if ((rc = tiff_collect(h, "fish_render_tiff", 3, H, W, 3, t, files, file_cap, file_bytes, true))) return rc;   // (waits for the stream)
    timed_set(h, 0, 1);
    return ECSEG_OK;
}

// the same for n images, with up to two further rasters per image (the mask, (H, W); the min-cut picture, (H, W, 3)) encoded beside the
// three rendered ones: every file of every image goes through ONE batched encode (tiff_encode_batch.h)
int ecseg_fish_render_tiff_batch(ecseg_ctx* h, int n_images, const uint8_t* const* imgs, const int32_t* shapes, const int32_t* channels,
                                 const uint8_t* const* thresholded, const uint8_t* const* boundaries, const uint8_t* const* masks,
                                 const uint8_t* const* pictures, uint8_t* out, long long out_cap, int64_t* out_ranges) {
    DRIVER_OPEN(h);
    const std::string me = "fish_render_tiff_batch: ";
    if (n_images < 0 || out_cap < 0 || (n_images > 0 && (!imgs || !shapes || !channels || !thresholded || !boundaries || !out || !out_ranges)))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    if ((long long)n_images * 5 >= 65536) return fail(h, ECSEG_E_INVALID, me + "65536 files or more");
    clear_timings(h);
    if (n_images == 0) return ECSEG_OK;
    const size_t n = (size_t)n_images;
    // one device buffer holds, per image, the inputs and the rasters that are encoded, every one on a multiple of 256 bytes
    struct Place { size_t img, thr, bnd, file[5]; bool has[5]; int ch[4]; };
    std::vector<Place> at(n);
    std::vector<int64_t> rows;
    size_t work = 0;
    auto take = [&](size_t bytes) { const size_t o = work; work += (bytes + 255) / 256 * 256; return o; };
    int rc;
    for (size_t i = 0; i < n; ++i) {
        const int H = shapes[3 * i], W = shapes[3 * i + 1], C = shapes[3 * i + 2];
        Place& p = at[i];
        if ((rc = fish_render_check(h, imgs[i], H, W, C, channels + 4 * i, thresholded[i], C - 1, boundaries[i], p.ch))) return rc;
        if (!tiff_args_ok(H, W, 3)) return fail(h, ECSEG_E_INVALID, me + "the TIFF writer takes lines below 2^30 bytes");
        const size_t px = (size_t)H * W;
        p.img = take(px * C); p.thr = take(px * (C - 1)); p.bnd = take(px);
        for (int k = 0; k < 5; ++k) {
            const int spp = k == 3 ? 1 : 3;
            p.has[k] = k < 3 || (k == 3 ? masks && masks[i] : pictures && pictures[i]);
            if (!p.has[k]) continue;
            p.file[k] = take(px * spp);
            const int64_t row[5] = {(int64_t)p.file[k], H, W, spp, 0};
            rows.insert(rows.end(), row, row + 5);
        }
    }
    const int n_files = (int)(rows.size() / 5);
    std::vector<TeFileIn> in;
    TeBatchLayout L;
    std::string bad = tiff_encode_batch_plan(rows.data(), n_files, (long long)work, in);
    if (bad.empty()) bad = te_batch_layout(in, L);
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    USE_DEVICE(h);
    uint8_t* d = nullptr;
    TiffEncodeBatchBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { d = c.take<uint8_t>(work); b = tiff_encode_batch_bufs(c, L, false); }))) return rc;
    b.src = d + L.src_base;                                  // (the table's offsets count from the first raster)
    hipStream_t s = h->stream;
    for (size_t i = 0; i < n; ++i) {
        const size_t px = (size_t)shapes[3 * i] * shapes[3 * i + 1], C = (size_t)shapes[3 * i + 2];
        HIP_TRY(h, hipMemcpyAsync(d + at[i].img, imgs[i], px * C, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(d + at[i].thr, thresholded[i], px * (C - 1), hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(d + at[i].bnd, boundaries[i], px, hipMemcpyHostToDevice, s));
        if (at[i].has[3]) HIP_TRY(h, hipMemcpyAsync(d + at[i].file[3], masks[i], px, hipMemcpyHostToDevice, s));
        if (at[i].has[4]) HIP_TRY(h, hipMemcpyAsync(d + at[i].file[4], pictures[i], px * 3, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(h, hipMemcpyAsync(b.tab, L.tab.data(), L.tab.size() * sizeof(TeFile), hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1,
          for (size_t i = 0; i < n; ++i) {
              const Place& p = at[i];
              const FishRenderBufs r{d + p.img, d + p.thr, d + p.bnd, d + p.file[0], d + p.file[1], d + p.file[2]};
              HIP_TRY(h, run_fish_render(shapes[3 * i], shapes[3 * i + 1], shapes[3 * i + 2], p.ch, r, s));
          }
          HIP_TRY(h, run_tiff_encode_batch(b, L, s)));
    std::vector<int64_t> ranges(2 * (size_t)n_files);
    if ((rc = tiff_batch_collect(h, "fish_render_tiff_batch", L, b, out, out_cap, ranges.data()))) return rc;   // (waits for the stream)
    timed_set(h, 0, 1);
    size_t f = 0;
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 5; ++k) {
            int64_t* q = out_ranges + 2 * (5 * i + k);
            q[0] = at[i].has[k] ? ranges[2 * f] : 0;
            q[1] = at[i].has[k] ? ranges[2 * f + 1] : 0;
            f += at[i].has[k];
        }
    return ECSEG_OK;
}

// ---- stat_fish.batch: mask to file images for a chunk of images in one call (layout: fish_batch.h) ---------------------------------
}  // extern "C"

// What ecseg_stat_fish_batch and ecseg_stat_fish_batch_bytes plan alike: the chunk's layout and, over its encoded rasters, the
// batched encoder's.  Empty string, or what is wrong.
struct FsBatchPlan { FsBatchLayout L; TeBatchLayout T; };
static std::string fs_batch_plan(const std::vector<FsImageIn>& in, FsBatchPlan& p) {
    std::string bad = fs_batch_layout(in, p.L);
    if (!bad.empty()) return bad;
    std::vector<TeFileIn> files;
    bad = tiff_encode_batch_plan(p.L.files.data(), (int)(p.L.files.size() / 5), (long long)p.L.work, files);
    if (bad.empty()) bad = te_batch_layout(files, p.T);
    return bad;
}

extern "C" {

long long ecseg_stat_fish_batch_bytes(int n_images, const int32_t* shapes, const int32_t* kernel_sizes, const int32_t* flags,
                                      int record_capacity) {
    if (n_images == 0) return 0;
    if (n_images < 0 || !shapes || !kernel_sizes || !flags || record_capacity < 0) return -1;
    std::vector<FsImageIn> in((size_t)n_images);
    for (size_t i = 0; i < in.size(); ++i) {
        in[i].H = shapes[3 * i]; in[i].W = shapes[3 * i + 1]; in[i].C = shapes[3 * i + 2]; in[i].K = kernel_sizes[i];
        in[i].given_labels = flags[i] & 1; in[i].mask_file = flags[i] & 2; in[i].mask_is_file = flags[i] & 4; in[i].picture = flags[i] & 8;
    }
    FsBatchPlan p;
    if (!fs_batch_plan(in, p).empty()) return -1;
    Carver c, cells;
    (void)fs_batch_bufs(c, p.L);
    (void)tiff_encode_batch_bufs(c, p.T, false);
    (void)fs_batch_cell_bufs(cells, (size_t)record_capacity);
    return (long long)(c.used + cells.used);
}

int ecseg_stat_fish_batch(ecseg_ctx* h, int n_images, const uint8_t* const* imgs, const int32_t* shapes, const int32_t* channels,
                          const uint8_t* const* masks, const int32_t* const* labels, const int32_t* kernel_sizes,
                          const double* const* weights, const double* normal_thresholds, const double* intensity_thresholds,
                          const int32_t* min_cc_sizes, int line_thickness, const uint8_t* const* mask_files,
                          const uint8_t* const* pictures, int record_capacity, int32_t* ranks, int64_t* records, int32_t* n_cells,
                          uint8_t* out, long long out_cap, int64_t* out_ranges, uint8_t* thresholded_debug, uint8_t* boundaries_debug) {
    DRIVER_OPEN(h);
    static_assert(FSB_MAX_IMAGES == ECSEG_STAT_FISH_BATCH_MAX_IMAGES && FSB_MAX_KERNEL == ECSEG_FISH_SPOT_MAX_KERNEL, "fish_batch.h and the header disagree");
    const std::string me = "stat_fish_batch: ";
    if (n_images < 0 || out_cap < 0 || record_capacity < 0 || (record_capacity > 0 && !records) ||
        (n_images > 0 && (!imgs || !shapes || !channels || (!masks && !labels) || !kernel_sizes || !weights || !normal_thresholds ||
                          !intensity_thresholds || !min_cc_sizes || !ranks || !n_cells || !out || !out_ranges)))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    if (line_thickness < 1 || line_thickness > ECSEG_FISH_SPOT_MAX_LINE)
        return fail(h, ECSEG_E_INVALID, me + "line_thickness must be between 1 and " + std::to_string(ECSEG_FISH_SPOT_MAX_LINE));
    clear_timings(h);
    if (n_images == 0) return ECSEG_OK;
    if (n_images > FSB_MAX_IMAGES) return fail(h, ECSEG_E_INVALID, me + "more than " + std::to_string(FSB_MAX_IMAGES) + " images");
    const size_t n = (size_t)n_images;
    std::vector<FsImageIn> in(n);
    for (size_t i = 0; i < n; ++i) {
        const std::string who = me + "image " + std::to_string(i) + ": ";
        const bool has_mask = masks && masks[i], has_labels = labels && labels[i];
        if (!imgs[i] || !weights[i]) return fail(h, ECSEG_E_INVALID, who + "bad arguments (no image or no weights)");
        if (has_mask == has_labels) return fail(h, ECSEG_E_INVALID, who + "exactly one of the mask and the label map must be given");
        const int C = shapes[3 * i + 2];
        if (C < 3 || C > 4) return fail(h, ECSEG_E_INVALID, who + "the image must have 3 or 4 channels, not " + std::to_string(C));
        for (int j = 0; j < C; ++j)
            if (channels[4 * i + j] < 0 || channels[4 * i + j] >= C)
                return fail(h, ECSEG_E_INVALID, who + "channel index out of range (the image has " + std::to_string(C) + " channels)");
        FsImageIn& f = in[i];
        f.H = shapes[3 * i]; f.W = shapes[3 * i + 1]; f.C = C; f.K = kernel_sizes[i];
        f.given_labels = has_labels; f.mask_file = mask_files && mask_files[i]; f.picture = pictures && pictures[i];
        f.mask_is_file = f.mask_file && has_mask && mask_files[i] == masks[i];
    }
    FsBatchPlan p;
    const std::string bad = fs_batch_plan(in, p);
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    FsBatchLayout& L = p.L;
    for (size_t i = 0; i < n; ++i) {
        FsImage& t = L.tab[i];
        for (int j = 0; j < 4; ++j) t.ch[j] = j < t.C ? channels[4 * i + j] : 0;
        for (int j = 0; j < 3; ++j) t.ithr[j] = j < t.np ? intensity_thresholds[3 * i + j] : 0.0;
        t.normal_thr = normal_thresholds[i]; t.min_cc = min_cc_sizes[i];
        n_cells[i] = 0;
    }
    {
        Carver measure;
        (void)fs_batch_bufs(measure, L);
        if ((long long)measure.used != fs_batch_bytes(L)) return fail(h, ECSEG_E_INVALID, me + "fs_batch_bytes does not restate fs_batch_bufs");
    }
    USE_DEVICE(h);
    int rc;
    FsBatchBufs b{};
    TiffEncodeBatchBufs t{};
    if (L.n_pad > 0 && (rc = ensure_post(h, L.n_pad, (size_t)L.Hm * L.Wm))) return rc;
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = fs_batch_bufs(c, L); t = tiff_encode_batch_bufs(c, p.T, false); }))) return rc;
    t.src = b.work + p.T.src_base;                           // (the table's offsets count from the first encoded raster)
    hipStream_t s = h->stream;
    const std::vector<IsegImage> ptab = fs_batch_pad_table(L);
    for (size_t i = 0; i < n; ++i) {
        const FsImage& r = L.tab[i];
        const size_t px = (size_t)r.H * r.W;
        HIP_TRY(h, hipMemcpyAsync(b.work + r.img, imgs[i], px * r.C, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.w + r.w, weights[i], (size_t)r.K * r.K * sizeof(double), hipMemcpyHostToDevice, s));
        if (in[i].given_labels) HIP_TRY(h, hipMemcpyAsync(b.lab + r.lab, labels[i], px * sizeof(int32_t), hipMemcpyHostToDevice, s));
        else HIP_TRY(h, hipMemcpyAsync(b.work + r.msk, masks[i], px, hipMemcpyHostToDevice, s));
        if (in[i].mask_file && !in[i].mask_is_file) HIP_TRY(h, hipMemcpyAsync(b.work + r.file[3], mask_files[i], px, hipMemcpyHostToDevice, s));
        if (in[i].picture) HIP_TRY(h, hipMemcpyAsync(b.work + r.file[4], pictures[i], px * 3, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(h, hipMemcpyAsync(b.tab, L.tab.data(), n * sizeof(FsImage), hipMemcpyHostToDevice, s));
    if (!ptab.empty()) HIP_TRY(h, hipMemcpyAsync(b.ptab, ptab.data(), ptab.size() * sizeof(IsegImage), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(t.tab, p.T.tab.data(), p.T.tab.size() * sizeof(TeFile), hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_fishspot_batch_open(L, b, h->ws, s)));
    std::vector<int32_t> plan((n + 1) * 2);
    HIP_TRY(h, hipMemcpyAsync(plan.data(), b.plan, plan.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));   // every image's cells in one copy
    WAIT_SET(h, s, 0, 1);
    int max_cells = 0;
    for (size_t i = 0; i < n; ++i) {
        if (plan[2 * i + 1])
            return fail(h, ECSEG_E_INVALID, me + "image " + std::to_string(i) + ": the label map holds a label larger than H * W = " +
                                                std::to_string((long long)L.tab[i].H * L.tab[i].W) + " (renumber the labels by rank first)");
        n_cells[i] = plan[2 * i];
        max_cells = std::max(max_cells, plan[2 * i]);
    }
    const int cells = plan[2 * n];
    if (cells > record_capacity) return ECSEG_OK;           // the counts alone: the caller comes back with a larger buffer
    FsBatchCellBufs c{};
    if ((rc = lay_out(h, h->count_arena, [&](Carver& cv) { c = fs_batch_cell_bufs(cv, (size_t)cells); }))) return rc;
    TIMED(h, s, 2, 3,
          HIP_TRY(h, run_fishspot_batch(L, b, c, cells, max_cells, line_thickness, s));
          for (size_t i = 0; i < n; ++i) {
              const FsImage& r = L.tab[i];
              const FishRenderBufs fr{b.work + r.img, b.work + r.thr, b.work + r.bnd, b.work + r.file[0], b.work + r.file[1], b.work + r.file[2]};
              HIP_TRY(h, run_fish_render(r.H, r.W, r.C, r.ch, fr, s));
          }
          HIP_TRY(h, run_tiff_encode_batch(t, p.T, s)));
    std::vector<int64_t> ranges(2 * p.T.tab.size());
    if ((rc = tiff_batch_collect(h, "stat_fish_batch", p.T, t, out, out_cap, ranges.data()))) return rc;   // (waits for the stream; too small: nothing written)
    timed_add(h, 2, 3);
    HIP_TRY(h, hipMemcpyAsync(ranks, b.lab, L.px * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (cells > 0) HIP_TRY(h, hipMemcpyAsync(records, c.rec, (size_t)cells * ECSEG_FISH_SPOT_INT64 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    size_t f = 0, thr_at = 0, bnd_at = 0;
    for (size_t i = 0; i < n; ++i) {
        const FsImage& r = L.tab[i];
        const size_t px = (size_t)r.H * r.W;
        if (thresholded_debug) HIP_TRY(h, hipMemcpyAsync(thresholded_debug + thr_at, b.work + r.thr, px * r.np, hipMemcpyDeviceToHost, s));
        if (boundaries_debug) HIP_TRY(h, hipMemcpyAsync(boundaries_debug + bnd_at, b.work + r.bnd, px, hipMemcpyDeviceToHost, s));
        thr_at += px * r.np; bnd_at += px;
        for (int k = 0; k < FSB_FILES; ++k) {
            int64_t* q = out_ranges + 2 * (FSB_FILES * i + k);
            const bool has = r.file[k] >= 0;
            q[0] = has ? ranges[2 * f] : 0;
            q[1] = has ? ranges[2 * f + 1] : 0;
            f += has;
        }
    }
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

// ---- the min-cut splitter's max-flow tasks (src/max_flow_binary_mask.py:59-116) ------------------------------------------------
int ecseg_min_cut(ecseg_ctx* h, const uint8_t* masks, long long mask_bytes, const int32_t* tasks, int n_tasks, int dist, uint8_t* side,
                  int32_t* flow) {
    DRIVER_OPEN(h);
    if (n_tasks < 0 || mask_bytes < 0 || (n_tasks > 0 && (!masks || !tasks || !side || !flow)))
        return fail(h, ECSEG_E_INVALID, "min_cut: bad arguments");
    if (dist < 1 || dist > ECSEG_MIN_CUT_MAX_DIST)
        return fail(h, ECSEG_E_INVALID, "min_cut: dist must be between 1 and " + std::to_string(ECSEG_MIN_CUT_MAX_DIST));
    if (mask_bytes > ECSEG_MIN_CUT_MAX_BYTES)
        return fail(h, ECSEG_E_INVALID, "min_cut: more than " + std::to_string(ECSEG_MIN_CUT_MAX_BYTES) + " bytes of windows in one call");
    clear_timings(h);                                        // (before the tasks are checked: a refused task leaves zeros)
    if (n_tasks == 0) return ECSEG_OK;
    std::vector<long long> soff((size_t)n_tasks, -1);
    long long end = 0;
    size_t scratch = 0;
    int n_global = 0;
    for (int i = 0; i < n_tasks; ++i) {
        const int32_t* t = tasks + 8 * (size_t)i;
        const std::string who = "min_cut: task " + std::to_string(i);
        const long long off = t[0], th = t[1], tw = t[2];
        if (th < 1 || tw < 1 || th * tw > ECSEG_MIN_CUT_MAX_PIXELS)
            return fail(h, ECSEG_E_INVALID, who + ": the window must hold between 1 and " + std::to_string(ECSEG_MIN_CUT_MAX_PIXELS) + " pixels");
        if (off < end || off + th * tw > mask_bytes)
            return fail(h, ECSEG_E_INVALID, who + ": the window overlaps the one in front or leaves the buffer");
        end = off + th * tw;
        if (t[3] < 0 || t[3] >= th || t[4] < 0 || t[4] >= tw || t[5] < 0 || t[5] >= th || t[6] < 0 || t[6] >= tw)
            return fail(h, ECSEG_E_INVALID, who + ": source or sink outside the window");
        if (t[3] == t[5] && t[4] == t[6]) return fail(h, ECSEG_E_INVALID, who + ": source and sink are the same pixel");
        if (!masks[off + t[3] * tw + t[4]] || !masks[off + t[5] * tw + t[6]])
            return fail(h, ECSEG_E_INVALID, who + ": source or sink on a zero pixel");
        if (th * tw > h->min_cut_lds_pixels) {
            soff[(size_t)i] = (long long)scratch;
            ++n_global;
            scratch += mincut_scratch_bytes((int)th, (int)tw);
        }
    }
    USE_DEVICE(h);
    const size_t nb = (size_t)mask_bytes, nt = (size_t)n_tasks;
    int rc;
    MinCutBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = mincut_bufs(c, nb, n_tasks, scratch); }))) return rc;
    hipStream_t s = h->stream;
    HIP_TRY(h, hipMemcpyAsync(b.mask, masks, nb, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.desc, tasks, nt * 8 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.soff, soff.data(), nt * sizeof(long long), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemsetAsync(b.side, 0, nb, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_mincut(b.mask, b.desc, b.soff, n_tasks, n_global, dist, b.scratch, b.side, b.flow, s)));
    HIP_TRY(h, hipMemcpyAsync(side, b.side, nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(flow, b.flow, nt * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);                     // (soff is read by the copy above: it lives until here)
    return ECSEG_OK;
}

// ---- the min-cut splitter before its first max-flow: labels, selection, windows and centres (src/max_flow_binary_mask.py:143-216) ----
int ecseg_min_cut_regions(ecseg_ctx* h, const uint8_t* mask, int H, int W, double coeff, int min_rad, int region_capacity,
                          int center_capacity, long long window_capacity, int32_t* labels, int32_t* n_cells, int32_t* regions,
                          int32_t* n_regions, int32_t* centers, int32_t* n_centers, uint8_t* windows, int32_t* comp, long long* window_pixels) {
    DRIVER_OPEN(h);
    static_assert(MCR_LDS_PIXELS == ECSEG_MIN_CUT_CENTERS_LDS_PIXELS && MCR_MAX_PIXELS == ECSEG_MIN_CUT_MAX_PIXELS &&
                  MCR_MAX_BYTES == ECSEG_MIN_CUT_MAX_BYTES, "mincut_regions.h and the header disagree");
    const std::string me = "min_cut_regions: ";
    if (n_cells) *n_cells = 0;
    if (n_regions) *n_regions = 0;
    if (n_centers) *n_centers = 0;
    if (window_pixels) *window_pixels = 0;
    if (!mask || !labels || !n_cells || !n_regions || !n_centers || !window_pixels || region_capacity < 0 || center_capacity < 0 ||
        window_capacity < 0 || (region_capacity > 0 && !regions) || (center_capacity > 0 && !centers) || (window_capacity > 0 && (!windows || !comp)))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    if (H < 1 || W < 1) return fail(h, ECSEG_E_INVALID, me + "H and W must be at least 1");
    if (!px_below_2_31(H, W)) return fail(h, ECSEG_E_INVALID, me + "image too large (H * W must be below 2^31)");
    if (min_rad < 0) return fail(h, ECSEG_E_INVALID, me + "min_rad must not be negative");
    if (!(coeff - coeff == 0.0)) return fail(h, ECSEG_E_INVALID, me + "coeff must be finite");
    USE_DEVICE(h);
    const size_t px = (size_t)H * W;
    int rc;
    McrOpenBufs o{};
    if ((rc = ensure_post(h, 1, px))) return rc;
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { o = mcr_open_bufs(c, H, W); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(o.mask, mask, px, hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_mcr_label(h->ws, H, W, o, s)));
    int32_t n = 0;
    HIP_TRY(h, hipMemcpyAsync(&n, o.misc, sizeof(n), hipMemcpyDeviceToHost, s));
    WAIT_SET(h, s, 0, 1);
    *n_cells = n;
    if (n == 0) {                                            // an empty mask: no label, no region
        std::fill(labels, labels + px, (int32_t)0);
        return ECSEG_OK;
    }
    // the areas and boxes are sized by the number of labels, which is known only now
    int32_t* d_stats = nullptr;
    if ((rc = lay_out(h, h->count_arena, [&](Carver& c) { d_stats = c.take<int32_t>((size_t)n * 5); }))) return rc;
    TIMED(h, s, 2, 3, HIP_TRY(h, run_mcr_stats(H, W, n, o, d_stats, s)));
    std::vector<int32_t> stats((size_t)n * 5);
    HIP_TRY(h, hipMemcpyAsync(stats.data(), d_stats, stats.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(labels, o.lab, px * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    WAIT_ADD(h, s, 2, 3);
    McrPlan P;
    const std::string bad = mcr_plan(stats.data(), n, coeff, h->min_cut_centers_lds_pixels, P);
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    *n_regions = P.n_regions;
    *window_pixels = P.window_pixels;
    if (P.n_regions == 0) return ECSEG_OK;
    // a region's accumulators: at most one 8-connected component per 2 x 2 block of its interior
    std::vector<int32_t> slot((size_t)P.n_regions);
    size_t slots = 0;
    for (int i = 0; i < P.n_regions; ++i) {
        const int rh = P.regions[(size_t)i * MCR_REC + 3], rw = P.regions[(size_t)i * MCR_REC + 4];
        slot[(size_t)i] = (int32_t)slots;
        slots += mcr_center_bound(rh, rw);
    }
    McrRegionBufs b{};                                       // (the statistics are on the host: their arena is laid out anew)
    if ((rc = lay_out(h, h->count_arena, [&](Carver& c) { b = mcr_region_bufs(c, P.n_regions, (size_t)P.window_pixels, slots); }))) return rc;
    HIP_TRY(h, hipMemcpyAsync(b.regions, P.regions.data(), P.regions.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.slot, slot.data(), slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    TIMED(h, s, 0, 1, HIP_TRY(h, run_mcr_centers(o.lab, W, P.n_regions, P.n_lds, min_rad, h->min_cut_centers_lds_pixels, b, s)));
    std::vector<int32_t> counts((size_t)P.n_regions);
    HIP_TRY(h, hipMemcpyAsync(counts.data(), b.counts, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    WAIT_ADD(h, s, 0, 1);
    const long long nc = mcr_place_centers(P, counts.data());
    if (nc < 0 || nc > (long long)slots) return fail(h, ECSEG_E_INVALID, me + "the component counts leave their bound");
    *n_centers = (int32_t)nc;
    if (!mcr_fits(P.n_regions, nc, P.window_pixels, region_capacity, center_capacity, window_capacity))
        return ECSEG_OK;                                     // the counts alone: the caller comes back with larger buffers
    std::copy(P.regions.begin(), P.regions.end(), regions);
    if (nc > 0) HIP_TRY(h, hipMemcpyAsync(centers, b.centers, (size_t)nc * MCR_REC * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(windows, b.windows, (size_t)P.window_pixels, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(comp, b.comp, (size_t)P.window_pixels * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return ECSEG_OK;
}

}  // extern "C"
