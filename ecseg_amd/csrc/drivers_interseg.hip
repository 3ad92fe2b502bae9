// The interSeg drivers (src/interseg.py:113-235; kernels in interseg_kernels.hip): the regions of a nucleus mask, which leave their
// label map and image on the handle, and the crops cut from those; and all of it for the images of a chunk in one call
// (ecseg_interseg_batch, planned by iseg_batch.h).
#include <climits>

#include "driver_util.h"
#include "iseg_batch.h"
#include "iseg_classify.h"

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

// The descriptors and the channel order of ecseg_nucleus_crops / ecseg_classify_nucleus_crops (`who`) against the region map on the
// handle; order: channel_order, checked.
static int check_crops(ecseg_ctx* h, const std::string& who, const int32_t* crops, int n_crops, const int32_t* channel_order, int order[3]) {
    if (h->iseg_n < 0) return fail(h, ECSEG_E_INVALID, who + ": no region map on the handle (call ecseg_nuclei_regions first)");
    for (int c = 0; c < 3; ++c) {
        order[c] = channel_order[c];
        if (order[c] < 0 || order[c] >= h->iseg_C) return fail(h, ECSEG_E_INVALID, who + ": channel_order out of range");
    }
    for (int k = 0; k < n_crops; ++k) {
        const int32_t* d = crops + (size_t)k * 5;
        if (d[0] < 0 || d[0] >= h->iseg_n || d[1] < 0 || d[2] < 0 || d[3] < 1 || d[3] > 256 || d[4] < 1 || d[4] > 256 ||
            d[1] > h->iseg_H - d[3] || d[2] > h->iseg_W - d[4])
            return fail(h, ECSEG_E_INVALID, who + ": crop " + std::to_string(k) + " is not a 1..256 x 1..256 window of a region");
    }
    return ECSEG_OK;
}

// Empty, or why `m` cannot serve as the classifier `name`: a loaded plan from compact (256, 256, c_in) patches to n_out values.
static std::string classifier_plan_error(const ecseg_ctx* m, const char* call, const char* name, int c_in, int n_out) {
    const std::string who = std::string(call) + ": the " + name + " handle ";
    if (!m->has_model) return who + "has no model loaded";
    const ecseg_tensor_desc& ti = m->tensors[m->input_tensor];
    const ecseg_tensor_desc& to = m->tensors[m->output_tensor];
    if (ti.h != 256 || ti.w != 256 || ti.c != c_in || ti.c_stride != ti.c || ti.c_offset != 0 || to.h != 1 || to.w != 1 || to.c != n_out)
        return who + "holds a plan from (" + std::to_string(ti.h) + ", " + std::to_string(ti.w) + ", " + std::to_string(ti.c) + ") to " +
               std::to_string((long long)to.h * to.w * to.c) + " values; " + name + " takes (256, 256, " + std::to_string(c_in) + ") and yields " +
               std::to_string(n_out);
    return std::string();
}

}  // extern "C"

// ---- what ecseg_classify_nucleus_crops and ecseg_interseg_batch share: the two models' checks, their share of a call, and the runs
// of one classifier chunk ------------------------------------------------------------------------------------------------------------
static int classifier_models_check(ecseg_ctx* h, const char* call, ecseg_ctx* model_i, ecseg_ctx* model_c) {
    std::string why = classifier_plan_error(model_i, call, "ecSeg-i", 1, 3);
    if (why.empty() && model_c) why = classifier_plan_error(model_c, call, "ecSeg-c", 3, 1);
    if (!why.empty()) return fail(h, ECSEG_E_INVALID, why);
    if (model_i->device != h->device || (model_c && model_c->device != h->device))
        return fail(h, ECSEG_E_INVALID, std::string(call) + ": the crops handle and the model handles are not on one device");
    return ECSEG_OK;
}

// a model's share of the call: its handle, the crops it takes per run, what one run leaves per crop, and where the rows go
struct ClassifySide { ecseg_ctx* m = nullptr; int per_group = 1, n_out = 0; float* pred = nullptr; std::vector<int32_t> sel; int n_sel = 0; std::vector<float> stage; };

// side[0] ecSeg-i, side[1] ecSeg-c (m null without one), for chunks of at most nc crops
static int classify_sides_open(ecseg_ctx* h, ecseg_ctx* model_i, ecseg_ctx* model_c, int nc, float* pred_i, float* pred_c, ClassifySide side[2]) {
    side[0].m = model_i; side[0].n_out = 3; side[0].pred = pred_i;
    side[1].m = model_c; side[1].n_out = 1; side[1].pred = pred_c;
    for (int q = 0; q < 2; ++q) {
        ClassifySide& sd = side[q];
        if (!sd.m) continue;
        sd.per_group = std::max(1, windows_per_group(sd.m));
        sd.sel.resize(nc);
        sd.stage.resize((size_t)std::min(nc, sd.per_group) * sd.n_out);       // the rows of one run, compact
        if (int rc = ensure_patches(sd.m, std::min(nc, sd.per_group))) return fail(h, rc, sd.m->err);
        if (sd.m != h) clear_timings(sd.m);
        prof_begin(sd.m);
    }
    if (!model_c) side[1].sel.resize(nc);                    // (iseg_select writes no entry there: centromeric is off)
    return ECSEG_OK;
}

// The chosen crops of one chunk (side[q].sel, n_sel: indices into b.crop) through the models; the rows go to side[q].pred + (k0 + crop) * n_out.
static int classify_chunk_runs(ecseg_ctx* h, ClassifySide side[2], const ClassifyBufs& b, size_t k0) {
    hipStream_t s = h->stream;
    ecseg_ctx* model_i = side[0].m;
    ecseg_ctx* model_c = side[1].m;
    int rc;
    if (side[0].n_sel) HIP_TRY(h, hipMemcpyAsync(b.sel_i, side[0].sel.data(), (size_t)side[0].n_sel * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (side[1].n_sel) HIP_TRY(h, hipMemcpyAsync(b.sel_c, side[1].sel.data(), (size_t)side[1].n_sel * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int rounds = std::max(iseg_sub_count(side[0].n_sel, side[0].per_group), side[1].m ? iseg_sub_count(side[1].n_sel, side[1].per_group) : 0);
    // Round r: sub-chunk r of either list (a list that has run out takes no part).  The crops handle's stream is idle but for
    // the input kernel, whose end (ev[3]) the model streams wait for; the crop buffer, the lists and the input tensors are not
    // written again before both models' rows have arrived.
    for (int r = 0; r < rounds; ++r) {
        int at[2] = {0, 0}, cnt[2] = {0, 0};
        for (int q = 0; q < 2; ++q)
            if (side[q].m && r < iseg_sub_count(side[q].n_sel, side[q].per_group)) {
                at[q] = r * side[q].per_group;
                cnt[q] = iseg_sub_len(side[q].n_sel, side[q].per_group, r);
            }
        float* in_i = view_of(model_i, model_i->input_tensor).p;
        float* in_c = model_c ? view_of(model_c, model_c->input_tensor).p : nullptr;
        TIMED(h, s, 2, 3, HIP_TRY(h, run_iseg_classifier_inputs(b.crop.crops, b.crop.max, b.sel_i + at[0], cnt[0], b.sel_c + at[1], cnt[1], in_i, in_c, s)));
        for (int q = 0; q < 2; ++q) {
            ClassifySide& sd = side[q];
            if (!cnt[q]) continue;
            hipStream_t ms = sd.m->stream;
            if (ms != s) HIP_TRY(h, hipStreamWaitEvent(ms, h->ev[3], 0));
            HIP_TRY(h, hipEventRecord(sd.m->ev[4], ms));
            if ((rc = run_plan_to_host(sd.m, cnt[q], sd.stage.data()))) return sd.m == h ? rc : fail(h, rc, sd.m->err);
            HIP_TRY(h, hipEventRecord(sd.m->ev[5], ms));
        }
        for (int q = 0; q < 2; ++q) {
            ClassifySide& sd = side[q];
            if (!cnt[q]) continue;
            HIP_TRY(h, hipStreamSynchronize(sd.m->stream));
            timed_add(sd.m, 4, 5, ECSEG_T_UNET);
            for (int j = 0; j < cnt[q]; ++j)
                std::copy_n(sd.stage.data() + (size_t)j * sd.n_out, sd.n_out, sd.pred + (k0 + (size_t)sd.sel[at[q] + j]) * sd.n_out);
        }
        HIP_TRY(h, hipStreamSynchronize(s));
        timed_add(h, 2, 3, ECSEG_T_TILE);
    }
    return ECSEG_OK;
}

extern "C" {

int ecseg_nucleus_crops(ecseg_ctx* h, const int32_t* crops, int n_crops, const int32_t* channel_order, uint8_t* out,
                        int32_t* channel_max) {
    DRIVER_OPEN(h);
    if (n_crops < 0 || (n_crops > 0 && (!crops || !channel_order || !out || !channel_max)))
        return fail(h, ECSEG_E_INVALID, "nucleus_crops: bad arguments");
    if (n_crops == 0) return ECSEG_OK;
    int order[3];
    if (int rc = check_crops(h, "nucleus_crops", crops, n_crops, channel_order, order)) return rc;
    USE_DEVICE(h);
    const int chunk = ISEG_CHUNK;                            // 48 MiB of crops per launch
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

int ecseg_classify_nucleus_crops(ecseg_ctx* h, ecseg_ctx* model_i, ecseg_ctx* model_c, const int32_t* crops, int n_crops,
                                 const int32_t* channel_order, const uint8_t* from_patches, int centromeric, int32_t* channel_max,
                                 float* pred_i, uint8_t* ran_i, float* pred_c, uint8_t* ran_c, uint8_t* crops_out) {
    DRIVER_OPEN(h);
    if (!model_i) return fail(h, ECSEG_E_INVALID, "classify_nucleus_crops: bad arguments (no ecSeg-i handle)");
    drop_sent_ahead(model_i);
    if (model_c) drop_sent_ahead(model_c);
    if (n_crops < 0 || (n_crops > 0 && (!crops || !channel_order || !from_patches || !channel_max || !pred_i || !ran_i || !ran_c ||
                                        (model_c && !pred_c))))
        return fail(h, ECSEG_E_INVALID, "classify_nucleus_crops: bad arguments");
    int rc;
    if ((rc = classifier_models_check(h, "classify_nucleus_crops", model_i, model_c))) return rc;
    if (n_crops == 0) return ECSEG_OK;
    int order[3];
    if ((rc = check_crops(h, "classify_nucleus_crops", crops, n_crops, channel_order, order))) return rc;
    USE_DEVICE(h);
    const size_t crop_bytes = (size_t)256 * 256 * 3;
    const int nc = std::min(n_crops, ISEG_CHUNK);
    ClassifySide side[2];
    if ((rc = classify_sides_open(h, model_i, model_c, nc, pred_i, pred_c, side))) return rc;
    ClassifyBufs b{};
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = classify_bufs(c, nc); }))) return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    for (int k0 = 0; k0 < n_crops; k0 += ISEG_CHUNK) {
        const int k = std::min(ISEG_CHUNK, n_crops - k0);
        HIP_TRY(h, hipMemcpyAsync(b.crop.desc, crops + (size_t)k0 * 5, (size_t)k * 5 * sizeof(int32_t), hipMemcpyHostToDevice, s));
        TIMED(h, s, 0, 1, HIP_TRY(h, run_nucleus_crops(h->iseg.lab, h->iseg.img, h->iseg_W, h->iseg_img_w, h->iseg_C, b.crop.desc, k, order, b.crop.crops, b.crop.max, s)));
        if (crops_out) HIP_TRY(h, hipMemcpyAsync(crops_out + (size_t)k0 * crop_bytes, b.crop.crops, (size_t)k * crop_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(channel_max + (size_t)k0 * 3, b.crop.max, (size_t)k * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        WAIT_ADD(h, s, 0, 1);
        iseg_select(channel_max + (size_t)k0 * 3, from_patches + k0, k, centromeric && model_c, side[0].sel.data(), &side[0].n_sel,
                    side[1].sel.data(), &side[1].n_sel, ran_i + k0, ran_c + k0);
        if ((rc = classify_chunk_runs(h, side, b, (size_t)k0))) return rc;
    }
    for (ClassifySide& sd : side) if (sd.m) prof_end(sd.m);
    return ECSEG_OK;
}

int ecseg_interseg_batch(ecseg_ctx* h, ecseg_ctx* model_i, ecseg_ctx* model_c, const uint8_t* packed, long long packed_bytes,
                         const int64_t* images, int n_images, int fish_index, int record_capacity, int crop_capacity, int32_t* out,
                         int64_t* records, int32_t* crop_region, int32_t* channel_max, float* pred_i, uint8_t* ran_i, float* pred_c,
                         uint8_t* ran_c) {
    DRIVER_OPEN(h);
    static_assert(ISEG_ST_OK == ECSEG_ISEG_OK && ISEG_ST_INSTANCE_IDS == ECSEG_ISEG_INSTANCE_IDS && ISEG_ST_RECORDS_OVERFLOW == ECSEG_ISEG_RECORDS_OVERFLOW &&
                  ISEG_ST_CROPS_OVERFLOW == ECSEG_ISEG_CROPS_OVERFLOW && ISEG_BATCH_MAX_IMAGES == ECSEG_INTERSEG_BATCH_MAX_IMAGES, "iseg_batch.h and the header disagree");
    const std::string me = "interseg_batch: ";
    if (!model_i) return fail(h, ECSEG_E_INVALID, me + "bad arguments (no ecSeg-i handle)");
    drop_sent_ahead(model_i);
    if (model_c) drop_sent_ahead(model_c);
    if (n_images < 0 || n_images > ISEG_BATCH_MAX_IMAGES)
        return fail(h, ECSEG_E_INVALID, me + "n_images must be between 0 and " + std::to_string(ISEG_BATCH_MAX_IMAGES));
    if (packed_bytes < 0 || record_capacity < 0 || crop_capacity < 0 || (fish_index != 0 && fish_index != 1) ||
        (n_images > 0 && (!packed || !images || !out)) || (record_capacity > 0 && !records) ||
        (crop_capacity > 0 && (!crop_region || !channel_max || !pred_i || !ran_i || !ran_c || (model_c && !pred_c))))
        return fail(h, ECSEG_E_INVALID, me + "bad arguments");
    int rc;
    if ((rc = classifier_models_check(h, "interseg_batch", model_i, model_c))) return rc;
    clear_timings(h);
    if (n_images == 0) return ECSEG_OK;
    std::vector<IsegImage> tab;
    const std::string bad = iseg_batch_table(images, n_images, packed_bytes, tab);    // the geometry first: nothing is read through a bad offset
    if (!bad.empty()) return fail(h, ECSEG_E_INVALID, me + bad);
    USE_DEVICE(h);
    const int order[3] = {fish_index, 1 - fish_index, 2};                             // the reorder of src/interseg.py:119
    ClassifySide side[2];
    const bool classify = crop_capacity > 0;
    if (classify && (rc = classify_sides_open(h, model_i, model_c, std::min(crop_capacity, ISEG_CHUNK), pred_i, pred_c, side))) return rc;
    hipStream_t s = h->stream;
    int rec_used = 0, crop_used = 0;
    for (const IsegGroup& g : iseg_batch_groups(tab, record_capacity)) {
        const int cap = record_capacity - rec_used, crop_base = crop_used;
        {
            Carver measure;
            iseg_batch_bufs(measure, g.n, g.Hm, g.Wm, (size_t)g.span, cap);
            if ((long long)measure.used != iseg_batch_bytes(g.n, g.Hm, g.Wm, g.span, cap))
                return fail(h, ECSEG_E_INVALID, me + "iseg_batch_bytes does not restate iseg_batch_bufs");
        }
        IsegBatchBufs b{};
        if ((rc = ensure_post(h, g.n, (size_t)g.Hm * g.Wm))) return rc;
        if ((rc = lay_out(h, h->call_arena, [&](Carver& c) { b = iseg_batch_bufs(c, g.n, g.Hm, g.Wm, (size_t)g.span, cap); }))) return rc;
        std::vector<IsegImage> gt(tab.begin() + g.first, tab.begin() + g.first + g.n);   // offsets from the group's first byte
        for (IsegImage& t : gt) { t.img_off -= g.base; t.seg_off -= g.base; }
        const size_t ni = (size_t)g.n;
        HIP_TRY(h, hipMemcpyAsync(b.packed, packed + g.base, (size_t)g.span, hipMemcpyHostToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(b.tab, gt.data(), ni * sizeof(IsegImage), hipMemcpyHostToDevice, s));
        TIMED(h, s, 0, 1, HIP_TRY(h, run_iseg_batch_regions(g.n, g.Hm, g.Wm, fish_index, b, h->ws, s)));
        std::vector<int32_t> plan(ni * ISEG_PLAN), imisc(ni * 4);
        int32_t misc[4] = {0, 0, 0, 0};
        HIP_TRY(h, hipMemcpyAsync(plan.data(), b.plan, plan.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(imisc.data(), b.imisc, imisc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(h, hipMemcpyAsync(misc, b.misc, sizeof(misc), hipMemcpyDeviceToHost, s));
        WAIT_ADD(h, s, 0, 1);
        const int taken = misc[3];
        if (taken < 0 || taken > cap) return fail(h, ECSEG_E_HIP, me + "the device plan took more records than there is room for");
        if (taken > 0) {
            HIP_TRY(h, hipMemcpyAsync(records + (size_t)rec_used * 8, b.rec, (size_t)taken * 8 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(h, hipStreamSynchronize(s));
        }
        // per image: its status, and the crops of its regions into the group's list while the caller has room for them
        std::vector<int32_t> desc;
        std::vector<uint8_t> tiled;
        for (int i = 0; i < g.n; ++i) {
            int32_t* o = out + (size_t)(g.first + i) * 8;
            const int n = plan[(size_t)i * ISEG_PLAN + 1], off = plan[(size_t)i * ISEG_PLAN + 2];
            const int vmax = imisc[(size_t)i * 4 + 1], vmin = 255 - imisc[(size_t)i * 4 + 2];
            o[1] = n; o[2] = o[3] = o[4] = -1; o[5] = n > 0 ? vmin : 0; o[6] = n > 0 ? vmax : 0; o[7] = 0;
            if (off < 0 || off + n > taken) { o[0] = ISEG_ST_RECORDS_OVERFLOW; continue; }
            if (n > 0 && vmin != vmax) { o[0] = ISEG_ST_INSTANCE_IDS; continue; }
            o[2] = rec_used + off;
            const int64_t* rec = records + (size_t)o[2] * 8;
            long long need = 0;
            for (int r = 0; r < n; ++r) need += iseg_region_crops(rec + (size_t)r * 8);
            o[3] = (int32_t)std::min<long long>(need, INT32_MAX);
            const int at = need <= INT32_MAX ? iseg_take((int)need, &crop_used, crop_capacity) : -1;
            if (at < 0) { o[0] = ISEG_ST_CROPS_OVERFLOW; continue; }
            o[0] = ISEG_ST_OK; o[4] = at;
            for (int r = 0; r < n; ++r) iseg_region_descs(rec + (size_t)r * 8, i, r, desc, tiled);
        }
        rec_used += taken;
        // the classifier chunks run over the group's whole list: only its last one can be partial
        const int total = (int)tiled.size();
        for (int j = 0; j < total; ++j) {                    // (what check_crops holds the caller's descriptors to, here for the records')
            const int32_t* d = desc.data() + (size_t)j * ISEG_DESC;
            const IsegImage& t = gt[(size_t)d[0]];
            if (d[2] < 0 || d[3] < 0 || d[4] < 1 || d[4] > 256 || d[5] < 1 || d[5] > 256 || d[2] > t.h - d[4] || d[3] > t.w - d[5])
                return fail(h, ECSEG_E_HIP, me + "a region record of image " + std::to_string(g.first + d[0]) + " lies outside its segmentation");
        }
        for (int j = 0; j < total; ++j) crop_region[(size_t)crop_base + j] = desc[(size_t)j * ISEG_DESC + 1];
        for (int k0 = 0; k0 < total; k0 += ISEG_CHUNK) {
            const int k = std::min(ISEG_CHUNK, total - k0);
            const int32_t* d = desc.data() + (size_t)k0 * ISEG_DESC;
            const size_t c0 = (size_t)crop_base + k0;
            HIP_TRY(h, hipMemcpyAsync(b.desc, d, (size_t)k * ISEG_DESC * sizeof(int32_t), hipMemcpyHostToDevice, s));
            TIMED(h, s, 0, 1, HIP_TRY(h, run_iseg_batch_crops(g.Hm, g.Wm, b, k, order, s)));
            HIP_TRY(h, hipMemcpyAsync(channel_max + c0 * 3, b.cls.crop.max, (size_t)k * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            WAIT_ADD(h, s, 0, 1);
            side[0].n_sel = side[1].n_sel = 0;
            for (int a = 0; a < k;) {                        // ecSeg-c applies per image: iseg_select run by run
                const int e = iseg_run_end(d, a, k);
                const int centromeric = model_c && gt[(size_t)d[(size_t)a * ISEG_DESC]].run_c;
                int32_t* si = side[0].sel.data() + side[0].n_sel;
                int32_t* sc = side[1].sel.data() + side[1].n_sel;
                int n_i = 0, n_c = 0;
                iseg_select(channel_max + (c0 + a) * 3, tiled.data() + k0 + a, e - a, centromeric, si, &n_i, sc, &n_c, ran_i + c0 + a, ran_c + c0 + a);
                for (int j = 0; j < n_i; ++j) si[j] += a;    // from the run's index to the chunk's
                for (int j = 0; j < n_c; ++j) sc[j] += a;
                side[0].n_sel += n_i; side[1].n_sel += n_c;
                a = e;
            }
            if ((rc = classify_chunk_runs(h, side, b.cls, c0))) return rc;
        }
    }
    if (classify) for (ClassifySide& sd : side) if (sd.m) prof_end(sd.m);
    return ECSEG_OK;
}

int ecseg_iseg_classifier_inputs_debug(ecseg_ctx* h, const uint8_t* crops, int k, const int32_t* channel_max, const int32_t* sel_i,
                                       int n_i, const int32_t* sel_c, int n_c, float* out_i, float* out_c) {
    DRIVER_OPEN(h);
    if (!crops || !channel_max || k < 1 || k > ISEG_CHUNK || n_i < 0 || n_i > ISEG_CHUNK || n_c < 0 || n_c > ISEG_CHUNK ||
        (n_i > 0 && (!sel_i || !out_i)) || (n_c > 0 && (!sel_c || !out_c)))
        return fail(h, ECSEG_E_INVALID, "iseg_classifier_inputs_debug: bad arguments");
    for (int j = 0; j < n_i; ++j) if (sel_i[j] < 0 || sel_i[j] >= k) return fail(h, ECSEG_E_INVALID, "iseg_classifier_inputs_debug: sel_i out of range");
    for (int j = 0; j < n_c; ++j) if (sel_c[j] < 0 || sel_c[j] >= k) return fail(h, ECSEG_E_INVALID, "iseg_classifier_inputs_debug: sel_c out of range");
    USE_DEVICE(h);
    const size_t crop_bytes = (size_t)256 * 256 * 3, px = (size_t)256 * 256;
    ClassifyBufs b{};
    float* d_i = nullptr;
    float* d_c = nullptr;
    int rc;
    if ((rc = lay_out(h, h->call_arena, [&](Carver& c) {
            b = classify_bufs(c, ISEG_CHUNK); d_i = c.take<float>((size_t)n_i * px); d_c = c.take<float>((size_t)n_c * px * 3); })))
        return rc;
    hipStream_t s = h->stream;
    clear_timings(h);
    HIP_TRY(h, hipMemcpyAsync(b.crop.crops, crops, (size_t)k * crop_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemcpyAsync(b.crop.max, channel_max, (size_t)k * 3 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (n_i) HIP_TRY(h, hipMemcpyAsync(b.sel_i, sel_i, (size_t)n_i * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (n_c) HIP_TRY(h, hipMemcpyAsync(b.sel_c, sel_c, (size_t)n_c * sizeof(int32_t), hipMemcpyHostToDevice, s));
    TIMED(h, s, 2, 3, HIP_TRY(h, run_iseg_classifier_inputs(b.crop.crops, b.crop.max, b.sel_i, n_i, b.sel_c, n_c, d_i, d_c, s)));
    if (n_i) HIP_TRY(h, hipMemcpyAsync(out_i, d_i, (size_t)n_i * px * sizeof(float), hipMemcpyDeviceToHost, s));
    if (n_c) HIP_TRY(h, hipMemcpyAsync(out_c, d_c, (size_t)n_c * px * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    timed_set(h, 2, 3, ECSEG_T_TILE);
    return ECSEG_OK;
}

}  // extern "C"
