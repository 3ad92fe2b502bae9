// C ABI of libecseg_hip.so (see include/ecseg_hip.h): the handle's life cycle, errors, options, page-locked host memory and the
// timing / profile getters.  The rest of the host side: model_load.hip, plan_run.hip, segment.hip, drivers_*.hip (ctx.h: what they share).
#include <cstdio>
#include <cstdlib>
#include "ctx.h"

namespace ecseg {

namespace { std::string g_create_error; }

int fail(ecseg_ctx* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}
int fail_hip(ecseg_ctx* h, hipError_t e, const char* what) {
    return fail(h, ECSEG_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int check_model(ecseg_ctx* h) {
    if (!h) return ECSEG_E_INVALID;
    if (!h->has_model) return fail(h, ECSEG_E_NOMODEL, "no model loaded (call ecseg_model_load first)");
    return ECSEG_OK;
}

// The three tiff_*_on_device options are a bit each of the handle's kinds word.
static void set_tiff_kind(ecseg_ctx* h, unsigned bit, int on) { h->tiff_kinds = on ? h->tiff_kinds | bit : h->tiff_kinds & ~bit; }

}  // namespace ecseg

using namespace ecseg;

extern "C" {

int ecseg_abi_version(void) { return ECSEG_ABI_VERSION; }

int ecseg_create(ecseg_ctx** out, int device_id) {
    if (!out) return fail(nullptr, ECSEG_E_INVALID, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(nullptr, ECSEG_E_HIP, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, ECSEG_E_INVALID, "device_id out of range");
    if ((e = hipSetDevice(device_id)) != hipSuccess) return fail_hip(nullptr, e, "hipSetDevice");
    // Waiting host threads sleep instead of spinning: with this runtime's default (hipDeviceScheduleAuto = spin when the host has
    // more cores than GPUs) a thread inside a segment call burns a whole core for the length of the call - measured 1.35 cores
    // busy per waiting call, 0.13 with this flag and the blocking event of wait_stream, at the same wall time
    // (tools/experiments/wait_cpu.py).  The flag belongs to the DEVICE, i.e. to every HIP user of it in this process (torch tensors
    // of an embedding application included): INTEGRATION.md says so next to the ABI notes, and ECSEG_SPIN_WAIT=1 leaves the runtime's
    // default alone.  Round 6 tried to make it opt-in and took that back: under the default scheduling mode hipFree
    // hung for ever in ecseg_destroy - device idle, hipDeviceSynchronize returning hipSuccess - once a process had created and
    // closed several handles (gpurun_out/r06_gputest_i.log: tests/test_gpu_unet.py then tests/test_gpu_configs.py; never with the flag).
    if (!getenv("ECSEG_SPIN_WAIT") || atoi(getenv("ECSEG_SPIN_WAIT")) == 0) {
        if (hipSetDeviceFlags(hipDeviceScheduleBlockingSync) != hipSuccess) (void)hipGetLastError();    // (not fatal: the default stays)
    }
    ecseg_ctx* h = new ecseg_ctx();
    h->device = device_id;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
        snprintf(h->devname, sizeof(h->devname), "%s (%s)", prop.name, prop.gcnArchName);
    }
    if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) {
        delete h;
        return fail_hip(nullptr, e, "hipStreamCreate");
    }
    if ((e = hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking)) != hipSuccess) {
        (void)hipStreamDestroy(h->stream);
        delete h;
        return fail_hip(nullptr, e, "hipStreamCreate");
    }
    for (auto& ev : h->ev) (void)hipEventCreate(&ev);
    for (auto& ev : h->ev_files) (void)hipEventCreate(&ev);
    for (auto& ev : h->ev_read) (void)hipEventCreate(&ev);
    if (hipMalloc(reinterpret_cast<void**>(&h->zero_page), 1024) == hipSuccess) (void)hipMemset(h->zero_page, 0, 1024);
    else h->zero_page = nullptr;
    *out = h;
    return ECSEG_OK;
}

void ecseg_destroy(ecseg_ctx* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamSynchronize(h->stream2);
    free_model(h);
    if (h->zero_page) (void)hipFree(h->zero_page);
    // the handle's device memory goes HERE, before the events and streams (a hipFree after them has hung: see ecseg_create), not
    // with `delete h` below
    { DevMem dying(std::move(static_cast<DevMem&>(*h))); }
    for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : h->ev_files) if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : h->ev_read) if (ev) (void)hipEventDestroy(ev);
    if (h->ev_block) (void)hipEventDestroy(h->ev_block);
    if (h->stream_in) { (void)hipStreamSynchronize(h->stream_in); (void)hipStreamDestroy(h->stream_in); }
    if (h->ev_pre) (void)hipEventDestroy(h->ev_pre);
    for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->grp_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->lane_events) (void)hipEventDestroy(e);
    for (hipStream_t ls : h->lane_streams) { (void)hipStreamSynchronize(ls); (void)hipStreamDestroy(ls); }
    (void)hipStreamDestroy(h->stream2);
    (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* ecseg_last_error(ecseg_ctx* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ecseg_device_name(ecseg_ctx* h, char* buf, int buflen) {
    if (!h || !buf || buflen <= 0) return ECSEG_E_INVALID;
    snprintf(buf, buflen, "%s", h->devname);
    return ECSEG_OK;
}

void* ecseg_stream(ecseg_ctx* h) { return h ? (void*)h->stream : nullptr; }

int ecseg_set_images_per_group(ecseg_ctx* h, int n) {
    if (!h || n < 0) return ECSEG_E_INVALID;               // 0: automatic (windows_per_group)
    h->images_per_group = n;
    return ECSEG_OK;
}

int ecseg_set_option(ecseg_ctx* h, const char* key, int value) {
    if (!h || !key) return ECSEG_E_INVALID;
    const std::string k(key);
    if (k == "overlap_post") h->overlap_post = value != 0;
    else if (k == "blocking_wait") h->blocking_wait = value != 0;
    else if (k == "fuse_pool") h->fuse_pool = value != 0;
    else if (k == "fuse_head") h->fuse_head = value != 0;
    else if (k == "wino_resident") h->wino_resident = value != 0;
    else if (k == "wino16") h->wino16 = value != 0;
    else if (k == "fuse_first") h->fuse_first = value != 0;
    else if (k == "wino4_split") h->wino4_split = value != 0;
    else if (k == "crop") h->crop = value != 0;
    else if (k == "winograd") {                            // 0 direct, 1 F(2x2), 2 F(4x4), 3 F(4x4) on the bf16 pipe with 3-way split operands
        h->use_winograd = value < 0 ? 0 : value > 3 ? 3 : (int)value;
        return ensure_split_images(h);
    }
    else if (k == "post_chunk" && value >= 1) h->post_chunk = value;
    else if (k == "images_per_group" && value >= 0) h->images_per_group = value;     // 0: automatic
    else if (k == "crop_mask") h->crop_mask = value != 0;
    else if (k == "unet_lanes" && value >= 0 && value <= 8) h->unet_lanes = value;   // 0: automatic
    else if (k == "lane_auto_windows" && value >= 0) h->lane_auto_windows = value;
    else if (k == "tiff_deflate_on_device") set_tiff_kind(h, ECSEG_TIFF_DEFLATE, value);
    else if (k == "tiff_tiled_on_device") set_tiff_kind(h, ECSEG_TIFF_TILED, value);
    else if (k == "tiff_packbits_on_device") set_tiff_kind(h, ECSEG_TIFF_PACKBITS, value);
    else if (k == "min_cut_lds_pixels" && value >= 0 && value <= ECSEG_MIN_CUT_LDS_PIXELS) h->min_cut_lds_pixels = value;   // 0: every window in global memory
    else if (k == "min_cut_centers_lds_pixels" && value >= 0 && value <= ECSEG_MIN_CUT_CENTERS_LDS_PIXELS) h->min_cut_centers_lds_pixels = value;   // 0: every crop in global memory
    else return fail(h, ECSEG_E_INVALID, "unknown option or bad value: " + k);
    return ECSEG_OK;
}

// Page-locked host memory: hipMemcpyAsync from / to it is a DMA transfer the host thread does not wait for (pageable
// memory is staged through the runtime's own pinned chunks by the calling thread).  These two calls read nothing of the
// handle but its device number and never write its error string: they may run on another thread while the handle is
// inside a call (`make metaseg` page-locks batch buffers on a helper thread, ecseg_amd/metaseg.py: _PinnedPool).
int ecseg_host_alloc(ecseg_ctx* h, size_t bytes, void** out) {
    if (!h || !out) return ECSEG_E_INVALID;
    *out = nullptr;
    if (bytes == 0) return ECSEG_OK;
    if (hipSetDevice(h->device) != hipSuccess) { (void)hipGetLastError(); return ECSEG_E_HIP; }
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocPortable);
    if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return e == hipErrorOutOfMemory ? ECSEG_E_NOMEM : ECSEG_E_HIP; }
    return ECSEG_OK;
}

int ecseg_host_free(ecseg_ctx* h, void* p) {
    if (!h) return ECSEG_E_INVALID;
    if (!p) return ECSEG_OK;
    if (hipSetDevice(h->device) != hipSuccess || hipHostFree(p) != hipSuccess) { (void)hipGetLastError(); return ECSEG_E_HIP; }
    return ECSEG_OK;
}

int ecseg_get_timings(ecseg_ctx* h, float* ms_out) {
    if (!h || !ms_out) return ECSEG_E_INVALID;
    for (int k = 0; k < ECSEG_T_N; ++k) ms_out[k] = h->stage_ms[k];
    return ECSEG_OK;
}

int ecseg_set_kernel_profiling(ecseg_ctx* h, int enabled) {
    if (!h) return ECSEG_E_INVALID;
    h->profile_kernels = enabled != 0;
    return ECSEG_OK;
}

int ecseg_get_conv_profile(ecseg_ctx* h, double* total_ms, int64_t* launches, double* flops) {
    if (!h) return ECSEG_E_INVALID;
    if (total_ms) *total_ms = h->last_conv_ms;
    if (launches) *launches = h->last_conv_launches;
    if (flops) *flops = h->last_conv_flops;
    return ECSEG_OK;
}

// Diagnostics: floats 16.. of the zero page (in-kernel cycle stamps); only in -DECSEG_DIAG builds (tools/build_variants.sh).
int ecseg_debug_peek(ecseg_ctx* h, float* out, int n) {
#ifdef ECSEG_DIAG
    if (!h || !out || n < 0 || n > 240 || !h->zero_page) return ECSEG_E_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipMemcpy(out, h->zero_page + 16, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return ECSEG_OK;
#else
    (void)out; (void)n;
    return fail(h, ECSEG_E_UNSUPPORTED, "ecseg_debug_peek: the shipped library carries no diagnostic kernels (build with -DECSEG_DIAG)");
#endif
}

int ecseg_get_conv_launch_profile(ecseg_ctx* h, int max_records, int32_t* op_index, int32_t* kind, float* ms, double* flops,
                                  double* executed_flops) {
    if (!h || max_records < 0) return ECSEG_E_INVALID;
    const int n = (int)std::min<size_t>(h->prof_recs.size(), (size_t)max_records);
    for (int k = 0; k < n; ++k) {
        const ecseg_ctx::ProfRec& r = h->prof_recs[k];
        if (op_index) op_index[k] = r.op;
        if (kind) kind[k] = r.kind;
        if (ms) ms[k] = r.ms;
        if (flops) flops[k] = r.flops;
        if (executed_flops) executed_flops[k] = r.exec_flops;
    }
    return n;
}

int ecseg_get_conv_executed_flops(ecseg_ctx* h, double* flops) {
    if (!h || !flops) return ECSEG_E_INVALID;
    *flops = h->last_conv_exec_flops;
    return ECSEG_OK;
}

}  // extern "C"
