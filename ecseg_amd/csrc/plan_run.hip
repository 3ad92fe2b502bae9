// The plan interpreter: activation buffers, crop look-up tables, run_plan / run_plan_op (which kernel launch each operator
// becomes, with its fusions and window lanes), the per-launch profile, and the entry points that run the bare network.
#include "ctx.h"

namespace ecseg {

int ensure_patches(ecseg_ctx* h, int n) {
    if (n <= h->cap_patches) return ECSEG_OK;
    for (float*& p : h->bufs) { if (p) (void)hipFree(p); p = nullptr; }
    h->bufs.assign(h->n_buffers, nullptr);
    h->cap_patches = 0;
    for (int b = 0; b < h->n_buffers; ++b) {
        const size_t bytes = std::max<size_t>(h->buf_floats[b], 4) * (size_t)n * sizeof(float);
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->bufs[b]), bytes);
        if (e != hipSuccess) return fail(h, ECSEG_E_NOMEM, std::string("hipMalloc(activations): ") + hipGetErrorString(e));
    }
    h->cap_patches = n;
    return ECSEG_OK;
}

// Windows per U-Net launch group.  An explicit images_per_group counts 35-window images (1040 x 1392).  Automatic: as many
// windows as fit ~48 GB of activations, between 16 and 64 such images - 16 for the canonical base-64 U-Net (82 MB per
// window), 32 for base 32, 64 for base 16, whose short kernels gain 5-6 % from the longer launches (base-16 bench model:
// 799 / 836 / 851 images/s at 16 / 32 / 64 images per group).
int windows_per_group(const ecseg_ctx* h) {
    if (h->images_per_group > 0) return h->images_per_group * 35;
    size_t per_window = 0;
    for (size_t f : h->buf_floats) per_window += std::max<size_t>(f, 4) * sizeof(float);
    const size_t budget = (size_t)48 << 30;
    size_t img = per_window ? budget / (per_window * 35) : 16;
    int g = 16;
    while (g < 64 && (size_t)(2 * g) <= img) g *= 2;
    return g * 35;
}

namespace {

hipEvent_t* prof_pair(ecseg_ctx* h) {
    if (h->prof_used + 2 > h->prof_events.size()) {
        for (int k = 0; k < 2; ++k) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            h->prof_events.push_back(e);
        }
    }
    hipEvent_t* p = &h->prof_events[h->prof_used];
    h->prof_used += 2;
    return p;
}

// The end of a profiled launch (prof_pair at its start): closes the event pair and books the launch under plan op `op`
void prof_record(ecseg_ctx* h, hipEvent_t* ev, hipStream_t s, int op, int kind, double flops, double exec_flops) {
    (void)hipEventRecord(ev[1], s);
    h->prof_flops += flops; h->prof_exec_flops += exec_flops;
    h->prof_recs.push_back({op, kind, flops, exec_flops, 0.f});
}

// A crop table on the device; false (and an empty buffer) when it cannot be allocated or copied
bool to_device(DevBuf<int32_t>& dev, const std::vector<int32_t>& t) {
    if (hipMalloc(reinterpret_cast<void**>(&dev.p), t.size() * sizeof(int32_t)) == hipSuccess &&
        hipMemcpy(dev.p, t.data(), t.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess) { dev.cap = t.size(); return true; }
    DevBuf<int32_t>().swap(dev);
    return false;
}

// Need box of window i under a crop recipe: the stitch's bounding box, grown by one pixel per 'd' (a 3x3 convolution
// behind) and halved per 'h' (a stride-2 up-convolution behind).  False: nothing of this window is ever read.
bool recipe_box(const StitchPlan* sp, const std::string& code, int i, int b[4]) {
    for (int k = 0; k < 4; ++k) b[k] = sp->box[4 * i + k];
    if (b[1] < 0) return false;
    int sz = 256;
    for (char c : code) {
        if (c == 'd') { b[0] = std::max(b[0] - 1, 0); b[1] = std::min(b[1] + 1, sz - 1); b[2] = std::max(b[2] - 1, 0); b[3] = std::min(b[3] + 1, sz - 1); }
        else { sz /= 2; for (int k = 0; k < 4; ++k) b[k] /= 2; }
    }
    return true;
}

// Device table (n_pos, 4) of the need boxes of a recipe (ConvParams::in_box); null on allocation failure (no masking).
const int32_t* get_crop_box(StitchPlan* sp, const std::string& code) {
    auto it = sp->boxes.find(code);
    if (it != sp->boxes.end()) return it->second;
    std::vector<int32_t> t((size_t)sp->n_pos * 4);
    for (int i = 0; i < sp->n_pos; ++i) {
        int b[4];
        if (!recipe_box(sp, code, i, b)) { b[0] = 1; b[1] = 0; b[2] = 1; b[3] = 0; }      // empty: everything reads as zero
        for (int k = 0; k < 4; ++k) t[4 * i + k] = b[k];
    }
    DevBuf<int32_t> dev;
    (void)to_device(dev, t);
    return sp->boxes.emplace(code, std::move(dev)).first->second;
}

// Region list of a crop recipe: per window the stitch's bounding box is grown / halved as the recipe says, then covered
// by rh x rw regions whose origins are multiples of 4 pixels (the Winograd tile) and stay inside the tensor.  Entry =
// window << 16 | (y origin / 4) << 8 | (x origin / 4).  len 0: nothing to gain (or an extent the kernel cannot take).
const CropLut* get_crop_lut(StitchPlan* sp, const std::string& code, int rh = 16, int rw = 16) {
    const std::string key = code + ":" + std::to_string(rh) + "x" + std::to_string(rw);
    auto it = sp->luts.find(key);
    if (it != sp->luts.end()) return &it->second;
    CropLut cl;
    int size = 256;
    for (char c : code) if (c == 'h') size /= 2;
    cl.size = size;
    std::vector<int32_t> lut;
    const int rdim[2] = {rh, rw};
    if (size >= 16 && size % 16 == 0) {
        for (int i = 0; i < sp->n_pos; ++i) {
            int b[4];
            cl.start.push_back((int)lut.size());
            if (!recipe_box(sp, code, i, b)) continue;         // nothing of this window is ever read
            int o[2], nr[2];
            for (int a = 0; a < 2; ++a) {
                const int lo = b[2 * a], hi = b[2 * a + 1];
                const int R = rdim[a];
                o[a] = lo & ~3;                                // tile-aligned start
                nr[a] = (hi - o[a]) / R + 1;
                if (R * nr[a] >= size) { nr[a] = (size + R - 1) / R; o[a] = 0; }
                else if (o[a] + R * nr[a] > size) o[a] = size - R * nr[a];
            }
            for (int ry = 0; ry < nr[0]; ++ry)
                for (int rx = 0; rx < nr[1]; ++rx) lut.push_back((i << 16) | (((o[0] + rh * ry) / 4) << 8) | ((o[1] + rw * rx) / 4));
        }
        cl.start.push_back((int)lut.size());
        if (lut.size() >= (size_t)sp->n_pos * ((size + rh - 1) / rh) * ((size + rw - 1) / rw)) lut.clear();     // nothing to gain
    }
    if (!lut.empty() && to_device(cl.dev, lut)) cl.len = (int)lut.size();
    return &sp->luts.emplace(key, std::move(cl)).first->second;
}

// The network's first layer (Conv2D 3x3 'same', 1 -> 16 channels) in front of a 16 -> 16 convolution that conv_wino16_kernel
// takes and that is its only reader: the second convolution's launch computes the first one into its own halo (FIRST); the
// 16-channel tensor between them is never written.  True: op oi is such a first layer and op oi + 1 carries it.
bool first_layer_fusable(const ecseg_ctx* h, size_t oi, bool cropped_plan) {
    if (!(h->fuse_first && h->use_winograd && h->wino16 && oi + 1 < h->ops.size())) return false;
    const OpRt& a = h->ops[oi];
    const OpRt& b = h->ops[oi + 1];
    const ecseg_tensor_desc& ta = h->tensors[a.d.in0];
    const ecseg_tensor_desc& tm = h->tensors[a.d.out];
    const ecseg_tensor_desc& tb = h->tensors[b.d.out];
    auto core = [](const ecseg_op_desc& q) { return q.act <= ECSEG_ACT_ELU && q.act != ECSEG_ACT_SOFTMAX && !(q.act == ECSEG_ACT_ELU && q.alpha != 1.f); };
    return a.d.op == ECSEG_OP_CONV && a.path == PATH_SMALL_CIN && a.d.kh == 3 && a.d.kw == 3 && a.d.stride == 1 && a.d.pad_top == 1 &&
           a.d.pad_left == 1 && a.d.dilation <= 1 && ta.c == 1 && ta.c_stride == 1 && (tm.c == 16 || tm.c == 32) && tm.h == ta.h && tm.w == ta.w && core(a.d) &&
           b.d.op == ECSEG_OP_CONV && b.path == PATH_MFMA && b.wt_wino16 != nullptr && b.d.in0 == a.d.out && h->consumers[a.d.out] == 1 &&
           a.d.out != h->output_tensor && b.d.kh == 3 && b.d.kw == 3 && b.d.stride == 1 && b.d.pad_top == 1 && b.d.pad_left == 1 &&
           tb.c == tm.c && tb.h == tm.h && tb.w == tm.w && tm.w % 4 == 0 && core(b.d) && !(cropped_plan && h->crop && b.crop_ok);
}

// ConvParams of a PATH_MFMA / PATH_TAP op from its descriptor: views, filter image, activation and the geometry of a forward
// convolution, of the sub-pixel form of a k x k / stride-2 transposed convolution, or of a one-tap (k = stride) transposed one
ConvParams conv_params(const ecseg_ctx* h, const OpRt& o, const TView& in, const TView& out, int n, int act) {
    const ecseg_op_desc& d = o.d;
    ConvParams p{};
    p.in = in; p.out = out; p.wt = o.wt; p.bias = o.bias; p.n = n;
    p.act = act; p.alpha = d.alpha; p.cin_chunks = o.cin_chunks; p.coutp = o.coutp; p.zero = h->zero_page;
    if (d.op == ECSEG_OP_CONV) {
        p.R = d.kh; p.S = d.kw; p.pad_top = d.pad_top; p.pad_left = d.pad_left; p.convt = 0; p.stride = d.stride;
    } else if (o.subpixel) {
        // 2x2 taps over input rows / columns (i - 1, i); tiles walk one position past the input (the last output
        // row / column of the full result comes from tap d = -1 alone)
        p.R = 2; p.S = 2; p.pad_top = 1; p.pad_left = 1; p.convt = 1; p.kT = 2;
        // (that position only matters when a kept output row / column lies at or beyond 2 x the input extent:
        // 4x4 'same' and every 'valid' layer, not 3x3 'same' - whose 16 x 16 inputs then tile exactly)
        p.convt_ext = (out.h + d.pad_top > 2 * in.h || out.w + d.pad_left > 2 * in.w) ? 1 : 0;
        p.crop_top = d.pad_top; p.crop_left = d.pad_left;
        // tap t = (d + 1) * 2 + (e + 1), phase (a, b): kernel index (a - 2 d, b - 2 e) >= k means a zero block (relayout_convt_subpixel)
        for (int dd = -1; dd <= 0; ++dd)
            for (int ee = -1; ee <= 0; ++ee)
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b)
                        if (a - 2 * dd >= d.kh || b - 2 * ee >= d.kw) p.tap_zero_mask |= 1 << (((dd + 1) * 2 + (ee + 1)) * 4 + a * 2 + b);
    } else {
        p.R = 1; p.S = 1; p.pad_top = 0; p.pad_left = 0; p.convt = 1; p.kT = d.kh;
        p.crop_top = d.pad_top; p.crop_left = d.pad_left;
    }
    const int npt = p.convt ? p.kT * p.kT * o.coutp : o.coutp;
    p.wt_chunk_stride = wt_chunk_pitch(npt); p.wt_tap_stride = wt_tap_pitch(npt, o.cin_chunks);
    return p;
}

// `crop`: the stitch that will read the model output (segment path), or null when every output pixel matters.
// Window lanes (round 4): a LaneSpec runs the plan on windows [w0, w0 + cnt) of the `n_all` windows whose input has been
// written, on stream `s` - several lanes of one small batch run beside each other on their own streams, so the
// half-empty last round of workgroups of one lane's deep layers (35 windows: 288 / 560 workgroups on 256 CUs) is filled by
// another lane's next layer.  Same kernels, same per-window arithmetic: results do not depend on the lanes.  A lane is
// either whole images or a part of ONE image (cropped launches then take a slice of the window-major region list).
// Launch op `oi` of the plan (and the ops its kernel takes over: a following pool / head - `oi` is advanced past them) for one
// lane (null: all n_all windows on the main stream).
int run_plan_op(ecseg_ctx* h, size_t& oi, int n_all, StitchPlan* crop, const LaneSpec* ls) {
    hipStream_t s = ls ? ls->s : h->stream;
    const bool lane = ls != nullptr;
    const int n = lane ? ls->cnt : n_all;
    const int w0 = lane ? ls->w0 : 0, cnt = n;
    const bool part = lane && crop && (w0 % crop->n_pos != 0 || cnt % crop->n_pos != 0);
    const int wbase = part ? (w0 / crop->n_pos) * crop->n_pos : w0;     // cropped launches of a partial lane: views at the image's first window
    if (part && w0 + cnt > wbase + crop->n_pos) return fail(h, ECSEG_E_INVALID, "window lane crosses an image boundary");
    // A lane's windows of tensor t.  Buffers are shared by tensors of different sizes (liveness re-use), so lanes that run at
    // different points of the plan must not share ANY byte of a buffer: a lane owns the slice [w0, w0 + cnt) x (the buffer's
    // floats per window) of every buffer and packs its windows of whatever tensor lives there at the slice's start.  The
    // model input and output keep the plain window order (the tiling kernel / the stitch address them for all lanes at
    // once): their buffers hold nothing of another size (checked at load: lanes_ok).  `rebase`: views of a partial
    // lane's cropped launch - the kernel adds (window index within the image) x (window size) itself.
    auto at = [&](int t, bool rebase = false) {
        if (t < 0) return TView{};
        TView v = view_of(h, t);
        if (!lane) return v;
        const ecseg_tensor_desc& td = h->tensors[t];
        const ptrdiff_t hwc = (ptrdiff_t)v.h * v.w * v.cs;
        const bool io = t == h->input_tensor || t == h->output_tensor;
        ptrdiff_t off = io ? (ptrdiff_t)w0 * hwc : (ptrdiff_t)w0 * (ptrdiff_t)std::max<size_t>(h->buf_floats[td.buffer], 4);
        if (rebase) off -= (ptrdiff_t)(w0 - wbase) * hwc;
        v.p += off;
        return v;
    };
    const OpRt* first = nullptr;                             // != null: op oi - 1 rides on op oi's launch
    if (first_layer_fusable(h, oi, crop != nullptr)) first = &h->ops[oi++];
    {
        const OpRt& o = h->ops[oi];
        const ecseg_op_desc& d = o.d;
        const TView in = first ? at(first->d.in0) : at(d.in0), out = at(d.out);
        hipError_t e = hipSuccess;
        switch (d.op) {
            case ECSEG_OP_CONV:
            case ECSEG_OP_CONVT: {
                const bool softmax = d.act == ECSEG_ACT_SOFTMAX;
                const int act = (softmax && o.path != PATH_HEAD) ? ECSEG_ACT_LINEAR : d.act;
                if (o.path == PATH_MFMA) {
                    const size_t oi_first = oi;                 // (fusions below advance oi)
                    ConvParams p = conv_params(h, o, in, out, n, act);
                    if (d.op == ECSEG_OP_CONV && d.kh == 1 && d.kw == 1 && in.h == 1 && in.w == 1 && out.h == 1 && out.w == 1) {
                        // Dense layer: the batch is the GEMM's M dimension - one "patch" whose pixels are the samples
                        p.in.w = n; p.out.w = n; p.n = 1;
                    }
                    bool rebased = false;                      // views of this launch start at the image's first window
                    // region list of a cropped launch; a partial lane takes the slice of its windows (entries keep their window
                    // index within the image, so the views go back to the image's first window)
                    auto use_lut = [&](const CropLut* cl) {
                        p.lut = cl->dev; p.lut_len = cl->len; p.per_image = crop->n_pos;
                        if (part) {
                            const int a = cl->start[w0 - wbase], b = cl->start[w0 - wbase + cnt];
                            p.lut = cl->dev + a; p.lut_len = b - a; p.n = crop->n_pos;
                            rebased = true;
                            p.box_first = 0;
                            p.in = at(d.in0, true); p.out = at(d.out, true);
                        }
                    };
                    hipEvent_t* ev = h->profile_kernels ? prof_pair(h) : nullptr;
                    if (ev) (void)hipEventRecord(ev[0], s);
                    double computed = 1.0;                     // fraction of the layer a cropped launch really computes
                    // conv_wino4 / conv_wino16 implement activation codes 0..6 with ELU's alpha = 1 (device_util.h: apply_act_core)
                    const bool act_core_ok = act <= ECSEG_ACT_ELU && !(act == ECSEG_ACT_ELU && d.alpha != 1.f);
                    if (first) {
                        p.first_w = first->wt; p.first_b = first->bias; p.first_act = first->d.act; p.first_alpha = first->d.alpha;
                    }
                    const bool wino4 = !first && h->use_winograd >= 2 && o.wt_wino4 && act_core_ok && conv_wino4_supported(p);   // (wt_wino* exist only for stride-1 3x3 'same' layers)
                    const bool wino = !wino4 && h->use_winograd && o.wt_wino && out.h >= 4 && out.w >= 8;
                    bool w16 = false, split1 = false;
                    // a 3x3 convolution of the cropped chain on a Winograd kernel reads its input only inside the receptive field
                    // of the outputs somebody needs (ConvParams::in_box): results do not depend on what a cropped producer left
                    // outside it
                    const bool crop_on = crop && h->crop && o.crop_ok && (part || n % crop->n_pos == 0);
                    if (crop_on && h->crop_mask && d.op == ECSEG_OP_CONV && d.kh == 3 && d.kw == 3 && (wino4 || wino)) {
                        p.in_box = get_crop_box(crop, o.crop_code + "d");
                        p.per_image = crop->n_pos;
                        p.box_first = part ? w0 - wbase : 0;
                    }
                    // Winograd output stages can write the 2x2 max-pool of their result themselves: a MaxPooling2D(2x2, stride
                    // 2) that follows directly (even extents, its own buffer) is then done with the convolution
                    auto fuse_following_pool = [&]() {
                        if (oi + 1 >= h->ops.size()) return;
                        const ecseg_op_desc& nx = h->ops[oi + 1].d;
                        const TView po = nx.op == ECSEG_OP_MAXPOOL ? at(nx.out, rebased) : TView{};
                        if (nx.op == ECSEG_OP_MAXPOOL && nx.mode == 0 /* max, not average */ && nx.in0 == d.out && nx.kh == 2 && nx.kw == 2 && nx.stride == 2 &&
                            h->fuse_pool && !softmax && po.h * 2 == out.h && po.w * 2 == out.w && po.c == out.c && po.cs % 4 == 0 &&
                            reinterpret_cast<uintptr_t>(po.p) % 16 == 0 &&
                            h->tensors[nx.out].buffer != h->tensors[d.in0].buffer && h->tensors[nx.out].buffer != h->tensors[d.out].buffer) {
                            p.pool = po;
                            ++oi;                              // the pooling op is done
                        }
                    };
                    // a 1x1 head (<= 4 classes) that is the only reader of this convolution's output is computed by the same output
                    // stage (conv_wino4: 64 channels, conv_wino16: 16 / 32); the feature tensor is then never written
                    auto fuse_following_head = [&](int channels) {
                        if (p.pool.p != nullptr || oi + 1 >= h->ops.size() || !h->fuse_head || out.c != channels || softmax) return;
                        const OpRt& hx = h->ops[oi + 1];
                        const ecseg_tensor_desc& td = h->tensors[d.out];
                        if (hx.d.op == ECSEG_OP_CONV && hx.path == PATH_HEAD && hx.head_w4 && hx.d.in0 == d.out && hx.d.act <= ECSEG_ACT_TANH &&
                            hx.d.act != ECSEG_ACT_LEAKY /* (the fused stage has the convolution's alpha, not the head's) */ &&
                            h->consumers[d.out] == 1 && d.out != h->output_tensor && td.c_stride == td.c && td.c_offset == 0 &&
                            // workgroups write head pixels while others still read the convolution's input halo
                            h->tensors[hx.d.out].buffer != h->tensors[d.in0].buffer &&
                            h->tensors[hx.d.out].buffer != td.buffer) {
                            p.head_w = hx.head_w4; p.head_b = hx.head_b4; p.head_out = at(hx.d.out, rebased);
                            p.head_k = p.head_out.c; p.head_act = hx.d.act; p.head_only = 1;
                            ++oi;                              // the head op is done
                        }
                    };
                    const bool wino4s = wino4 && h->use_winograd >= 3 && o.wt_wino4s && conv_wino4s_supported(p);
                    if (wino4) {
                        p.wt = wino4s ? reinterpret_cast<const float*>(o.wt_wino4s) : o.wt_wino4; p.coutp = out.c; p.w4_split = h->wino4_split;
                        if (crop_on) {
                            const CropLut* cl = get_crop_lut(crop, o.crop_code);
                            if (cl->len > 0 && out.h == cl->size && out.w == cl->size && conv_wino4_span_ok(p, crop->n_pos)) {
                                use_lut(cl);
                                computed = (double)cl->len / ((double)crop->n_pos * (out.h / 16) * (out.w / 16));
                            }
                        }
                        // a MaxPooling2D(2x2, stride 2) that follows directly is written by the same output stage
                        fuse_following_pool();
                        fuse_following_head(64);
                        e = wino4s ? launch_conv_wino4s(p, s) : conv_wino4r_supported(p) ? launch_conv_wino4r(p, s) : launch_conv_wino4(p, s);
                    } else if (wino && h->wino16 && o.wt_wino16 && act_core_ok && (first ? conv_wino16_first_supported(p) : conv_wino16_supported(p))) {
                        w16 = true;
                        p.wt = o.wt_wino16;
                        if (crop_on) {
                            // cropped launch: only the 16 x 32 blocks some later stage reads
                            const CropLut* cl = get_crop_lut(crop, o.crop_code, 16, 32);
                            if (cl->len > 0 && out.h == cl->size && out.w == cl->size) {
                                use_lut(cl);
                                computed = (double)cl->len / ((double)crop->n_pos * (out.h / 16) * (out.w / 32));
                            }
                        }
                        fuse_following_pool();
                        fuse_following_head(out.c);
                        e = launch_conv_wino16(p, s);
                    } else if (wino) {
                        p.wt = o.wt_wino; p.coutp = o.coutp_wino;
                        p.wt_chunk_stride = wt_chunk_pitch(o.coutp_wino); p.wt_tap_stride = wt_tap_pitch(o.coutp_wino, o.cin_chunks);
                        p.resident = h->wino_resident;
                        if (out.c % 4 == 0) fuse_following_pool();
                        e = launch_conv_wino(p, s);
                    } else {
                        if (crop_on && p.convt && in.h == in.w) {
                            // cropped up-convolution: only the input tiles whose outputs somebody reads; of the two tile
                            // shapes (4 x 32, 8 x 16) the one that needs fewer tiles
                            const CropLut* a = get_crop_lut(crop, o.crop_code, 4, 32);
                            const CropLut* b = get_crop_lut(crop, o.crop_code, 8, 16);
                            const CropLut* cl = nullptr; int tw = 0;
                            if (a->len > 0 && a->size == in.h && in.w >= 32 && (b->len == 0 || b->size != in.h || a->len <= b->len)) { cl = a; tw = 32; }
                            else if (b->len > 0 && b->size == in.h) { cl = b; tw = 16; }
                            if (cl) {
                                use_lut(cl); p.force_tw = tw;
                                const int th = 128 / tw;
                                computed = (double)cl->len / ((double)crop->n_pos * ((in.h + th - 1) / th) * ((in.w + tw - 1) / tw));
                            }
                        }
                        if (o.subpixel && o.ph_wt[0] != nullptr) {
                            // phase by phase (see OpRt::ph_wt): tiles walk the input positions j of the outputs 2 j + c that exist
                            p.tap_zero_mask = 0;
                            p.crop_top = 0; p.crop_left = 0;
                            p.convt_ext = ((out.h + 1) / 2 > in.h || (out.w + 1) / 2 > in.w) ? 1 : 0;
                            for (int ph = 0; ph < 4 && e == hipSuccess; ++ph) {
                                p.wt = o.ph_wt[ph]; p.R = o.ph_R[ph]; p.S = o.ph_S[ph]; p.pad_top = o.ph_pt[ph]; p.pad_left = o.ph_pl[ph];
                                p.phase_a = ph >> 1; p.phase_b = ph & 1;
                                p.convt = 2;                   // one output phase per launch: N = coutp
                                p.wt_chunk_stride = wt_chunk_pitch(o.coutp);
                                p.wt_tap_stride = wt_tap_pitch(o.coutp, o.cin_chunks);
                                e = launch_conv_mfma(p, s);
                            }
                        } else if (h->use_winograd >= 3 && o.wt_split1 != nullptr && p.convt == 1 && convs_supported(p)) {
                            p.wt = reinterpret_cast<const float*>(o.wt_split1);
                            split1 = true;
                            e = launch_convs(p, s);
                        } else {
                            e = launch_conv_mfma(p, s);
                        }
                    }
                    if (first && !w16 && e == hipSuccess) e = hipErrorInvalidValue;     // (the eligibility test above and the launcher's disagree)
                    if (ev) {
                        const double fl1 = first ? first->flops * n : 0.0;     // the first layer riding along (its 9 taps are padded to 12 on the MFMA)
                        // multiplies actually issued (sub-pixel transposed convolution: 4 taps x 4 phases per input pixel minus the all-zero blocks the kernel skips)
                        const double ex = o.flops * n * computed * (wino4 ? 0.25 : wino ? 16.0 / 36.0 : (o.subpixel && o.ph_wt[0] == nullptr) ? (16.0 - __builtin_popcount((unsigned)p.tap_zero_mask)) / (d.kh * d.kw) : 1.0);
                        const bool res = wino && p.resident && p.coutp == 32 && p.cin_chunks <= 4;
                        // kind: bits 0-7 the kernel, bit 8: the following 2x2 max-pool was written by this launch, bit 9: the following 1x1 head was
                        prof_record(h, ev, s, (int)oi_first, (split1 ? 6 : wino4s ? 5 : wino4 ? 2 : w16 ? 4 : res ? 3 : wino ? 1 : 0) | (p.pool.p != nullptr ? 0x100 : 0) |
                                    (p.head_w != nullptr ? 0x200 : 0) | (first ? 0x400 : 0), o.flops * n + fl1, ex + fl1 * 12.0 / 9.0);
                    }
                } else if (o.path == PATH_TAP) {
                    const ConvParams p = conv_params(h, o, in, out, n, act);
                    hipEvent_t* ev = h->profile_kernels ? prof_pair(h) : nullptr;
                    if (ev) (void)hipEventRecord(ev[0], s);
                    e = launch_conv_mfma_tap(p, d.dilation, s);
                    if (ev) prof_record(h, ev, s, (int)oi, 0, o.flops * n, o.flops * n);
                } else if (o.path == PATH_SMALL_CIN) {
                    e = launch_conv_small_cin(in, out, o.wt, o.bias, n, d.kh, d.kw, d.pad_top, d.pad_left, act, d.alpha, s);
                } else if (o.path == PATH_HEAD) {
                    e = launch_conv_head(in, out, o.wt, o.bias, n, d.act, d.alpha, s);
                } else if (d.op == ECSEG_OP_CONV) {
                    e = launch_conv_generic(in, out, o.wt, o.bias, n, d.kh, d.kw, d.stride, (d.mode & 0xff) ? (d.mode & 0xff) : d.stride, d.dilation > 1 ? d.dilation : 1,
                                            ((d.mode >> 8) & 0xff) ? ((d.mode >> 8) & 0xff) : (d.dilation > 1 ? d.dilation : 1), d.pad_top, d.pad_left, act, d.alpha, s);
                } else {
                    e = launch_convt_generic(in, out, o.wt, o.bias, n, d.kh, d.kw, d.stride, d.pad_top, d.pad_left, act, d.alpha, s);
                }
                if (e == hipSuccess && softmax && o.path != PATH_HEAD) e = launch_softmax(out, out, n, s);
                break;
            }
            case ECSEG_OP_MAXPOOL:
                if (d.pad_top || d.pad_left || (out.h - 1) * d.stride + d.kh > in.h || (out.w - 1) * d.stride + d.kw > in.w)
                    e = launch_pool_pad(in, out, n, d.kh, d.kw, d.stride, d.pad_top, d.pad_left, d.mode, s);     // padding = 'same'
                else e = launch_maxpool(in, out, n, d.kh, d.kw, d.stride, d.mode, s);
                break;
            case ECSEG_OP_DWCONV: {
                const bool softmax = d.act == ECSEG_ACT_SOFTMAX;
                e = launch_dwconv(in, out, o.wt, o.bias, n, d.kh, d.kw, d.stride, d.dilation, d.pad_top, d.pad_left, d.mode,
                                  softmax ? ECSEG_ACT_LINEAR : d.act, d.alpha, s);
                if (e == hipSuccess && softmax) e = launch_softmax(out, out, n, s);
                break;
            }
            case ECSEG_OP_PRELU: e = launch_prelu(in, out, o.wt, n, d.mode, s); break;
            case ECSEG_OP_LAYERNORM: e = launch_layernorm(in, out, o.scale, o.shift, n, d.alpha, s); break;
            case ECSEG_OP_GLOBALPOOL: e = launch_global_pool(in, out, n, d.mode, s); break;
            case ECSEG_OP_UPSAMPLE: e = launch_upsample(in, out, n, d.stride, d.mode, s); break;
            case ECSEG_OP_AFFINE:
                if (d.act == ECSEG_ACT_SOFTMAX) {
                    e = launch_affine(in, out, o.scale, o.shift, n, ECSEG_ACT_LINEAR, d.alpha, s);
                    if (e == hipSuccess) e = launch_softmax(out, out, n, s);
                } else {
                    e = launch_affine(in, out, o.scale, o.shift, n, d.act, d.alpha, s);
                }
                break;
            case ECSEG_OP_ACT:
                if (d.act == ECSEG_ACT_SOFTMAX) e = launch_softmax(in, out, n, s);
                else e = launch_affine(in, out, nullptr, nullptr, n, d.act, d.alpha, s);
                break;
            case ECSEG_OP_ADD: {
                const TView b = at(d.in1);
                e = launch_binary(in, b, out, n, d.mode, d.act == ECSEG_ACT_SOFTMAX ? ECSEG_ACT_LINEAR : d.act, d.alpha, s);
                if (e == hipSuccess && d.act == ECSEG_ACT_SOFTMAX) e = launch_softmax(out, out, n, s);
                break;
            }
            case ECSEG_OP_COPY: e = launch_copy(in, out, n, d.pad_top, d.pad_left, s); break;
            default: return fail(h, ECSEG_E_INVALID, "unknown op in plan");
        }
        if (e != hipSuccess) return fail_hip(h, e, "plan kernel launch");
    }
    return ECSEG_OK;
}

}  // namespace

// The whole plan on n_all patches whose input tensor has been written; with lanes, op by op for every lane in turn (the lanes'
// kernels are enqueued interleaved, so the streams start together)
int run_plan(ecseg_ctx* h, int n_all, StitchPlan* crop, const std::vector<LaneSpec>* lanes) {
    for (size_t oi = 0; oi < h->ops.size(); ++oi) {
        int rc;
        if (!lanes || lanes->empty()) {
            if ((rc = run_plan_op(h, oi, n_all, crop, nullptr))) return rc;
        } else {
            size_t last = oi;
            for (const LaneSpec& l : *lanes) {
                size_t o2 = oi;
                if (l.cnt > 0 && (rc = run_plan_op(h, o2, n_all, crop, &l))) return rc;
                if (l.cnt > 0) last = o2;
            }
            oi = last;
        }
    }
    return ECSEG_OK;
}

// The plan on ni patches whose input tensor has been filled, then their rows of the output tensor on the way to `out` (compact), all on
// the handle's stream: the caller waits for it.  Shared by forward_host and ecseg_classify_nucleus_crops (drivers_interseg.hip).
int run_plan_to_host(ecseg_ctx* h, int ni, float* out) {
    if (int rc = run_plan(h, ni)) return rc;
    const ecseg_tensor_desc& to = h->tensors[h->output_tensor];
    const TView ov = view_of(h, h->output_tensor);
    HIP_TRY(h, hipMemcpy2DAsync(out, (size_t)to.c * sizeof(float), ov.p, (size_t)ov.cs * sizeof(float), (size_t)to.c * sizeof(float),
                                (size_t)to.h * to.w * ni, hipMemcpyDeviceToHost, h->stream));
    return ECSEG_OK;
}

void prof_begin(ecseg_ctx* h) { h->prof_used = 0; h->prof_flops = 0.0; h->prof_exec_flops = 0.0; h->prof_recs.clear(); }
void prof_end(ecseg_ctx* h) {   // stream must be idle
    double ms = 0.0;
    for (size_t k = 0; k + 1 < h->prof_used; k += 2) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, h->prof_events[k], h->prof_events[k + 1]) == hipSuccess) ms += t;
        if (k / 2 < h->prof_recs.size()) h->prof_recs[k / 2].ms = t;
    }
    h->last_conv_ms = ms; h->last_conv_launches = (long long)(h->prof_used / 2); h->last_conv_flops = h->prof_flops;
    h->last_conv_exec_flops = h->prof_exec_flops;
}

}  // namespace ecseg

using namespace ecseg;

static int forward_host(ecseg_ctx* h, const void* patches, bool is_f32, int n, float* out) {
    if (h) drop_sent_ahead(h);
    int rc = check_model(h);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!patches || !out))) return fail(h, ECSEG_E_INVALID, "forward_patches: bad arguments");
    if (n == 0) return ECSEG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const ecseg_tensor_desc& ti = h->tensors[h->input_tensor];
    const ecseg_tensor_desc& to = h->tensors[h->output_tensor];
    if (ti.c_stride != ti.c || ti.c_offset != 0) return fail(h, ECSEG_E_INVALID, "input tensor must be compact");
    const size_t in_per = (size_t)ti.h * ti.w * ti.c, out_per = (size_t)to.h * to.w * to.c;
    const int chunk = std::max(1, windows_per_group(h));
    if ((rc = ensure_patches(h, std::min(n, chunk)))) return rc;
    if (!is_f32 && (rc = h->d_u8in.ensure(h, in_per * std::min(n, chunk)))) return rc;
    hipStream_t s = h->stream;
    prof_begin(h);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int ni = std::min(chunk, n - i0);
        if (is_f32) {
            HIP_TRY(h, hipMemcpyAsync(view_of(h, h->input_tensor).p, static_cast<const float*>(patches) + (size_t)i0 * in_per,
                                      in_per * ni * sizeof(float), hipMemcpyHostToDevice, s));
        } else {
            HIP_TRY(h, hipMemcpyAsync(h->d_u8in, static_cast<const uint8_t*>(patches) + (size_t)i0 * in_per, in_per * ni, hipMemcpyHostToDevice, s));
            HIP_TRY(h, launch_u8_to_f32(h->d_u8in, view_of(h, h->input_tensor).p, in_per * ni, s));
        }
        if ((rc = run_plan_to_host(h, ni, out + (size_t)i0 * out_per))) return rc;
        HIP_TRY(h, hipStreamSynchronize(s));
    }
    prof_end(h);
    return ECSEG_OK;
}

extern "C" {

int ecseg_forward_patches(ecseg_ctx* h, const uint8_t* patches, int n, float* out) { return forward_host(h, patches, false, n, out); }
int ecseg_forward_patches_f32(ecseg_ctx* h, const float* patches, int n, float* out) { return forward_host(h, patches, true, n, out); }

int ecseg_read_tensor(ecseg_ctx* h, int tensor, int n, float* out) {
    int rc = check_model(h);
    if (rc) return rc;
    if (tensor < 0 || tensor >= (int)h->tensors.size() || n <= 0 || n > h->cap_patches || !out)
        return fail(h, ECSEG_E_INVALID, "read_tensor: bad arguments");
    HIP_TRY(h, hipSetDevice(h->device));
    const ecseg_tensor_desc& t = h->tensors[tensor];
    const TView v = view_of(h, tensor);
    HIP_TRY(h, hipMemcpy2DAsync(out, (size_t)t.c * sizeof(float), v.p, (size_t)v.cs * sizeof(float), (size_t)t.c * sizeof(float),
                                (size_t)t.h * t.w * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return ECSEG_OK;
}

}  // extern "C"
