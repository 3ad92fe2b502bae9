// The model loader: validates a plan, chooses the kernel path of every operator (the if chain in ecseg_model_load IS the kernel-
// selection policy), uploads the weights in the layout that path wants and marks the operators a cropped launch may shorten.
#include <cstdlib>
#include "ctx.h"

namespace ecseg {

void free_model(ecseg_ctx* h) {
    for (float* p : h->dev_allocs) (void)hipFree(p);
    h->dev_allocs.clear();
    for (float* p : h->bufs) if (p) (void)hipFree(p);
    h->bufs.clear();
    h->cap_patches = 0;
    h->ops.clear(); h->tensors.clear();
    h->has_model = false;
    h->nuset_cls_t = h->nuset_bbox_t = -1;
}

int upload(ecseg_ctx* h, const std::vector<float>& host, float** dev) {
    float* p = nullptr;
    const size_t n = host.empty() ? 1 : host.size();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(float));
    if (e != hipSuccess) return fail(h, ECSEG_E_NOMEM, std::string("hipMalloc(weights): ") + hipGetErrorString(e));
    h->dev_allocs.push_back(p);
    if (!host.empty()) {
        e = hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail_hip(h, e, "hipMemcpy(weights)");
    }
    *dev = p;
    return ECSEG_OK;
}

// "winograd" = 3: every layer that has an F(4x4) filter image and whole 64-channel output blocks gets the bf16x3 stage image of
// conv_wino4s_kernel, written by a device kernel from the fp32 image (U rounded to float32 as the fp32 kernel uses it, then split
// EXACTLY into three bf16 pieces).  Done when the option is set or a model is loaded under it - never inside a forward pass.
int ensure_split_images(ecseg_ctx* h) {
    if (h->use_winograd < 3) return ECSEG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    bool any = false;
    for (OpRt& o : h->ops) {
        if (!o.wt_wino4 || o.wt_wino4s || o.w4_cout % 64 != 0) continue;
        void* d = nullptr;
        const hipError_t e = hipMalloc(&d, wino4s_image_bytes(o.w4_cin, o.w4_cout));
        if (e != hipSuccess) return fail(h, ECSEG_E_NOMEM, std::string("hipMalloc(split filter image): ") + hipGetErrorString(e));
        h->dev_allocs.push_back(reinterpret_cast<float*>(d));
        HIP_TRY(h, launch_wino4s_filter(o.wt_wino4, d, o.w4_cin, o.w4_cout, h->stream));
        o.wt_wino4s = d;
        any = true;
    }
    for (OpRt& o : h->ops) {
        if (!o.s1_np || o.wt_split1 || !o.wt) continue;
        void* d = nullptr;
        const hipError_t e = hipMalloc(&d, convs_image_bytes(o.s1_cin, o.s1_np));
        if (e != hipSuccess) return fail(h, ECSEG_E_NOMEM, std::string("hipMalloc(split filter image): ") + hipGetErrorString(e));
        h->dev_allocs.push_back(reinterpret_cast<float*>(d));
        HIP_TRY(h, launch_convs_filter(o.wt, d, o.s1_cin, o.s1_np, h->stream));
        o.wt_split1 = d;
        any = true;
    }
    if (any) HIP_TRY(h, hipStreamSynchronize(h->stream));
    return ECSEG_OK;
}

}  // namespace ecseg

using namespace ecseg;

// Crop recipes (OpRt::crop_ok / crop_code): walk back from the model output.  A 1x1 convolution passes its reader's need on, a
// 3x3 'same' convolution needs its input one pixel further out ('d'); a concatenation is followed through the view written
// by a 2x2 / stride-2 transposed convolution (which itself computes everything, from an input needed at half the
// coordinates, 'h'); skip connections and anything with several readers keep their full extent and end the walk
static void assign_crop_recipes(ecseg_ctx* h) {
    const std::vector<ecseg_tensor_desc>& tensors = h->tensors;
    int t = h->output_tensor, reader = (int)h->ops.size();
    std::string code;
    for (int guard = 0; guard < 32 && code.size() < 16; ++guard) {
        int prod = -1, nprod = 0;
        for (int k = 0; k < reader; ++k) if (h->ops[k].d.out == t) { prod = k; ++nprod; }
        if (nprod == 0) {
            const ecseg_tensor_desc& tt = tensors[t];
            int up = -1;
            for (int k = 0; k < reader; ++k) {
                const ecseg_op_desc& od = h->ops[k].d;
                const ecseg_tensor_desc& tv = tensors[od.out];
                if (od.op == ECSEG_OP_CONVT && tv.buffer == tt.buffer && tv.h == tt.h && tv.w == tt.w && tv.c_stride == tt.c_stride &&
                    tv.c < tt.c && h->consumers[od.out] == 0) up = k;                  // the last such writer before the reader
            }
            if (up < 0) break;
            const ecseg_op_desc& ud = h->ops[up].d;
            const ecseg_tensor_desc& ui = tensors[ud.in0];
            if (!(ud.kh == 2 && ud.kw == 2 && ud.stride == 2 && ud.pad_top == 0 && ud.pad_left == 0 && ui.h * 2 == tt.h && ui.w * 2 == tt.w)) break;
            if (h->consumers[ud.in0] != 1 || ui.c_stride != ui.c || ui.c_offset != 0) break;
            code += 'h';
            h->ops[up].crop_ok = true; h->ops[up].crop_code = code;      // the part of its INPUT that matters
            t = ud.in0; reader = up;
            continue;
        }
        if (nprod != 1) break;
        OpRt& o = h->ops[prod];
        const ecseg_tensor_desc& ti = tensors[o.d.in0];
        if (o.d.op != ECSEG_OP_CONV || o.d.dilation > 1 || o.d.stride != 1 || (o.d.mode & 0xffff)) break;
        o.crop_ok = true; o.crop_code = code;
        if (o.d.kh == 3 && o.d.kw == 3 && o.d.pad_top == 1 && o.d.pad_left == 1) code += 'd';
        else if (!(o.d.kh == 1 && o.d.kw == 1)) break;
        if (h->consumers[o.d.in0] != 1 || ti.c_stride != ti.c || ti.c_offset != 0) break;
        t = o.d.in0; reader = prod;
    }
}

extern "C" {

int ecseg_model_load(ecseg_ctx* h, const ecseg_tensor_desc* tensors, int n_tensors, int n_buffers, const ecseg_op_desc* ops,
                     int n_ops, const float* const* weights, const int64_t* weight_len, int n_weights, int input_tensor,
                     int output_tensor) {
    if (!h) return ECSEG_E_INVALID;
    drop_sent_ahead(h);
    if (!tensors || !ops || n_tensors <= 0 || n_ops <= 0 || n_buffers <= 0) return fail(h, ECSEG_E_INVALID, "empty plan");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_model(h);
    h->tensors.assign(tensors, tensors + n_tensors);
    h->n_buffers = n_buffers;
    h->buf_floats.assign(n_buffers, 0);
    for (int t = 0; t < n_tensors; ++t) {
        const ecseg_tensor_desc& d = tensors[t];
        if (d.buffer < 0 || d.buffer >= n_buffers || d.h <= 0 || d.w <= 0 || d.c <= 0 || d.c_offset < 0 ||
            d.c_stride < d.c_offset + d.c)
            return fail(h, ECSEG_E_INVALID, "bad tensor descriptor " + std::to_string(t));
        h->buf_floats[d.buffer] = std::max(h->buf_floats[d.buffer], (size_t)d.h * d.w * d.c_stride);
    }
    if (input_tensor < 0 || input_tensor >= n_tensors || output_tensor < 0 || output_tensor >= n_tensors)
        return fail(h, ECSEG_E_INVALID, "bad input/output tensor index");
    h->input_tensor = input_tensor; h->output_tensor = output_tensor;
    h->flops_per_patch = 0.0; h->mfma_flops_per_patch = 0.0;

    auto W = [&](int idx, int64_t expect, const char* what, const float** out) -> int {
        *out = nullptr;
        if (idx < 0) return ECSEG_OK;
        if (idx >= n_weights || !weights || !weights[idx]) return fail(h, ECSEG_E_INVALID, std::string("missing weight for ") + what);
        if (weight_len[idx] != expect)
            return fail(h, ECSEG_E_INVALID, std::string("weight size mismatch for ") + what + ": got " +
                                                std::to_string(weight_len[idx]) + ", expected " + std::to_string(expect));
        *out = weights[idx];
        return ECSEG_OK;
    };

    for (int k = 0; k < n_ops; ++k) {
        OpRt o;
        o.d = ops[k];
        const ecseg_op_desc& d = o.d;
        if (d.in0 < 0 || d.in0 >= n_tensors || d.out < 0 || d.out >= n_tensors || (d.op == ECSEG_OP_ADD && (d.in1 < 0 || d.in1 >= n_tensors)))
            return fail(h, ECSEG_E_INVALID, "bad tensor index in op " + std::to_string(k));
        const ecseg_tensor_desc& ti = tensors[d.in0];
        const ecseg_tensor_desc& to = tensors[d.out];
        o.path = PATH_OTHER;
        int rc;
        if (d.op == ECSEG_OP_CONV || d.op == ECSEG_OP_CONVT) {
            if (d.kh <= 0 || d.kw <= 0 || d.stride <= 0) return fail(h, ECSEG_E_INVALID, "bad conv geometry in op " + std::to_string(k));
            const int cin = ti.c, cout = to.c;
            const float *kw = nullptr, *kb = nullptr;
            if ((rc = W(d.w0, (int64_t)d.kh * d.kw * cin * cout, "conv kernel", &kw))) return rc;
            if (!kw) return fail(h, ECSEG_E_INVALID, "conv without kernel in op " + std::to_string(k));
            if ((rc = W(d.w1, cout, "conv bias", &kb))) return rc;
            if (kb) { if ((rc = upload(h, std::vector<float>(kb, kb + cout), &o.bias))) return rc; }
            const bool in_al = (ti.c_stride % 4 == 0) && (ti.c_offset % 4 == 0) && (cin % 4 == 0);
            const bool out_al = (to.c_stride % 4 == 0) && (to.c_offset % 4 == 0);
            // the kernels that take the Keras kernel as it is (HWIO; transposed convolutions: HWOI)
            auto raw_path = [&](int path) -> int {
                o.path = path;
                return upload(h, std::vector<float>(kw, kw + (size_t)d.kh * d.kw * cin * cout), &o.wt);
            };
            auto generic_path = [&]() -> int { return raw_path(PATH_GENERIC); };
            // the matrix-core kernels: Cout padded to whole N tiles of `bn` columns, Cin to 8-channel chunks, and the image that
            // `relayout` makes of the kernel for them
            auto mfma_path = [&](int path, int bn, auto relayout) -> int {
                o.path = path;
                o.coutp = (cout + bn - 1) / bn * bn;
                o.cin_chunks = (cin + 7) / 8;
                const int rc2 = upload(h, relayout(), &o.wt);
                if (!rc2) h->mfma_flops_per_patch += o.flops;
                return rc2;
            };
            // (tests/conv_exact_cases.py: conv_paths restates the choice of kernel below, for the kernels the launch profile does not
            // report; a change of these rules belongs there too)
            if (d.op == ECSEG_OP_CONV) {
                const int dil = d.dilation > 1 ? d.dilation : 1;
                // anisotropic strides / dilation rates (round 6): CONV's `mode` carries the HORIZONTAL stride (bits 0-7) and dilation rate (bits
                // 8-15) where they differ from the vertical ones in `stride` / `dilation` (0: the same) - such layers take the scalar kernel
                const int sx = (d.mode & 0xff) ? (d.mode & 0xff) : d.stride, dx = ((d.mode >> 8) & 0xff) ? ((d.mode >> 8) & 0xff) : dil;
                if ((to.h - 1) * d.stride + 1 > ti.h + (d.kh - 1) * dil || (to.w - 1) * sx + 1 > ti.w + (d.kw - 1) * dx)
                    return fail(h, ECSEG_E_INVALID, "conv output larger than its input in op " + std::to_string(k));
                o.flops = 2.0 * d.kh * d.kw * cin * cout * (double)to.h * to.w;
                if (sx != d.stride || dx != dil) {
                    if ((rc = generic_path())) return rc;
                    h->flops_per_patch += o.flops;
                    h->ops.push_back(o);
                    continue;
                }
                const bool taps_ok = d.kh == d.kw && (d.kh == 1 || d.kh == 2 || d.kh == 3);
                auto conv_image = [&]() { return relayout_conv(kw, d.kh, d.kw, cin, cout, o.cin_chunks, o.coutp); };
                // the tap-by-tap MFMA kernel takes whatever the halo-staged kernels do not: dilated taps, taps other than 1x1 / 2x2 /
                // 3x3 (5x5, 7x7, 1x3 ...), strides above 2
                auto tap_path = [&]() -> int { return mfma_path(PATH_TAP, conv_mfma_ntile(cout), conv_image); };
                const bool tap_ok = in_al && cin >= 8 && cout >= 8;
                if (dil > 1 && !(d.kh == 1 && d.kw == 1)) {
                    if ((rc = tap_ok ? tap_path() : generic_path())) return rc;
                } else if (d.stride != 1) {
                    // strided convolutions (classifier stems, down-sampling convolutions): the direct MFMA kernel gathers a
                    // strided halo (stride 2, 1x1 / 2x2 / 3x3 taps); anything else takes the generic kernel
                    if (d.stride == 2 && taps_ok && in_al && cin >= 8) {
                        if ((rc = mfma_path(PATH_MFMA, conv_mfma_ntile(cout), conv_image))) return rc;
                    } else if ((rc = tap_ok ? tap_path() : generic_path())) return rc;
                } else if (cin <= 4 && cout % 4 == 0 && out_al) {
                    if ((rc = raw_path(PATH_SMALL_CIN))) return rc;
                } else if (d.kh == 1 && d.kw == 1 && cout <= 8 && in_al) {
                    if ((rc = raw_path(PATH_HEAD))) return rc;
                    if (cout <= 4) {
                        std::vector<float> w4((size_t)cin * 4, 0.f), b4(4, 0.f);
                        for (int ci = 0; ci < cin; ++ci)
                            for (int co = 0; co < cout; ++co) w4[(size_t)ci * 4 + co] = kw[(size_t)ci * cout + co];
                        for (int co = 0; co < cout && kb; ++co) b4[co] = kb[co];
                        if ((rc = upload(h, w4, &o.head_w4))) return rc;
                        if ((rc = upload(h, b4, &o.head_b4))) return rc;
                    }
                } else if (taps_ok && in_al && cin >= 8 && (cout >= 16 || (d.kh >= 2 && cin >= 16))) {
                    // (a 2x2 / 3x3 convolution to a FEW channels - NuSeT's 3x3 'final' layer, src/model_layers/models.py:134 - still
                    // belongs on the matrix cores: a mostly empty 32-column tile beats the scalar kernel by an order of magnitude)
                    if ((rc = mfma_path(PATH_MFMA, conv_mfma_ntile(cout), conv_image))) return rc;
                    if (d.kh == 3 && d.pad_top == 1 && d.pad_left == 1 && to.h == ti.h && to.w == ti.w && cout >= 16 && cout % 4 == 0 && out_al) {
                        const int bnw = conv_wino_ntile(cout);
                        o.coutp_wino = (cout + bnw - 1) / bnw * bnw;
                        const std::vector<float> u = winograd_filter(kw, cin, cout);
                        if ((rc = upload(h, relayout_conv(u.data(), 4, 4, cin, cout, o.cin_chunks, o.coutp_wino), &o.wt_wino))) return rc;
                        if ((cin == 16 || cin == 32) && (cout == 16 || cout == 32) && to.h >= 16 && to.w >= 32)
                            if ((rc = upload(h, relayout_wino16(u, cin, cout), &o.wt_wino16))) return rc;
                        // F(4x4): a lone 32-channel block wastes its second channel-half waves on zeros; measured on
                        // MI355X (profiles/r02_kernel_map.json) that still beats F(2x2) once the K loop is long enough
                        if (cin % 4 == 0 && cin >= 8 && cout % 32 == 0 && (cout != 32 || cin >= 64) && to.h % 16 == 0 && to.w % 16 == 0) {
                            if ((rc = upload(h, winograd4_filter(kw, cin, cout), &o.wt_wino4))) return rc;
                            o.w4_cin = cin; o.w4_cout = cout;
                        }
                    }
                } else if (tap_ok && !taps_ok) {
                    if ((rc = tap_path())) return rc;
                } else if ((rc = generic_path())) return rc;
            } else {
                o.flops = 2.0 * d.kh * d.kw * cin * cout * (double)ti.h * ti.w;
                if (d.kh == d.kw && d.kh == d.stride && in_al && cin >= 8 && cout >= 16 && d.pad_top == 0 && d.pad_left == 0) {
                    const int bn = cout <= 16 && d.kh == 2 ? 16 : conv_mfma_ntile(cout);   // 2x2, <= 16 channels: all four phases in one 64-column tile
                    if ((rc = mfma_path(PATH_MFMA, bn, [&]() { return relayout_convt(kw, d.kh, cin, cout, o.cin_chunks, o.coutp); }))) return rc;
                    if (d.kh == 2 && o.coutp % 32 == 0 && cin >= 16 && cin % 4 == 0) { o.s1_cin = cin; o.s1_np = d.kh * d.kh * o.coutp; }
                } else if (d.kh == d.kw && (d.kh == 3 || d.kh == 4) && d.stride == 2 && in_al && cin >= 8 && d.pad_top >= 0 && d.pad_left >= 0) {
                    // k x k / stride 2, k != stride (a common Keras up-sampler; NuSeT's U-Net: src/model_layers/models.py:78-80):
                    // four sub-pixel convolutions as ONE 2x2-tap convolution over the input with N = 4 x Cout
                    o.subpixel = 1;
                    if ((rc = mfma_path(PATH_MFMA, cout <= 16 ? 16 : conv_mfma_ntile(cout),
                                        [&]() { return relayout_convt_subpixel(kw, d.kh, cin, cout, o.cin_chunks, o.coutp); }))) return rc;
                    if (cout >= 32 && d.pad_top <= 1 && d.pad_left <= 1) {      // phase by phase (OpRt::ph_wt)
                        const std::array<PhaseFilter, 4> phases = convt_phase_filters(kw, d.kh, cin, cout, d.pad_top, d.pad_left);
                        for (int ph = 0; ph < 4; ++ph) {
                            const PhaseFilter& f = phases[ph];
                            o.ph_R[ph] = f.R; o.ph_S[ph] = f.S; o.ph_pt[ph] = f.pt; o.ph_pl[ph] = f.pl;
                            if ((rc = upload(h, relayout_conv(f.hwio.data(), f.R, f.S, cin, cout, o.cin_chunks, o.coutp), &o.ph_wt[ph]))) return rc;
                        }
                    }
                } else if ((rc = generic_path())) return rc;
            }
            h->flops_per_patch += o.flops;
        } else if (d.op == ECSEG_OP_AFFINE) {
            const float *sc = nullptr, *sh = nullptr;
            if ((rc = W(d.w0, to.c, "affine scale", &sc))) return rc;
            if ((rc = W(d.w1, to.c, "affine shift", &sh))) return rc;
            if (!sc || !sh) return fail(h, ECSEG_E_INVALID, "affine without scale/shift in op " + std::to_string(k));
            if ((rc = upload(h, std::vector<float>(sc, sc + to.c), &o.scale))) return rc;
            if ((rc = upload(h, std::vector<float>(sh, sh + to.c), &o.shift))) return rc;
        } else if (d.op == ECSEG_OP_DWCONV) {
            const int mult = d.mode;
            if (d.kh <= 0 || d.kw <= 0 || d.stride <= 0 || mult < 1 || to.c != ti.c * mult)
                return fail(h, ECSEG_E_INVALID, "bad depthwise-conv geometry in op " + std::to_string(k));
            const int dil = d.dilation > 1 ? d.dilation : 1;
            if ((to.h - 1) * d.stride + 1 > ti.h + (d.kh - 1) * dil || (to.w - 1) * d.stride + 1 > ti.w + (d.kw - 1) * dil || d.pad_top < 0 || d.pad_left < 0)
                return fail(h, ECSEG_E_INVALID, "depthwise-conv output larger than its input in op " + std::to_string(k));
            const float *kw = nullptr, *kb = nullptr;
            if ((rc = W(d.w0, (int64_t)d.kh * d.kw * to.c, "depthwise kernel", &kw))) return rc;
            if (!kw) return fail(h, ECSEG_E_INVALID, "depthwise conv without kernel in op " + std::to_string(k));
            if ((rc = W(d.w1, to.c, "depthwise bias", &kb))) return rc;
            if ((rc = upload(h, std::vector<float>(kw, kw + (size_t)d.kh * d.kw * to.c), &o.wt))) return rc;
            if (kb) { if ((rc = upload(h, std::vector<float>(kb, kb + to.c), &o.bias))) return rc; }
            o.flops = 2.0 * d.kh * d.kw * to.c * (double)to.h * to.w;
            h->flops_per_patch += o.flops;
        } else if (d.op == ECSEG_OP_PRELU) {
            const float* a = nullptr;
            const int64_t len = d.mode ? (int64_t)to.h * to.w * to.c : (int64_t)to.c;
            if ((rc = W(d.w0, len, "PReLU slopes", &a))) return rc;
            if (!a) return fail(h, ECSEG_E_INVALID, "PReLU without slopes in op " + std::to_string(k));
            if ((rc = upload(h, std::vector<float>(a, a + len), &o.wt))) return rc;
        } else if (d.op == ECSEG_OP_LAYERNORM) {
            const float *g = nullptr, *b = nullptr;
            if ((rc = W(d.w0, to.c, "LayerNormalization gamma", &g))) return rc;
            if ((rc = W(d.w1, to.c, "LayerNormalization beta", &b))) return rc;
            if (g) { if ((rc = upload(h, std::vector<float>(g, g + to.c), &o.scale))) return rc; }
            if (b) { if ((rc = upload(h, std::vector<float>(b, b + to.c), &o.shift))) return rc; }
        } else if (d.op == ECSEG_OP_MAXPOOL || d.op == ECSEG_OP_UPSAMPLE) {
            if (d.stride <= 0) return fail(h, ECSEG_E_INVALID, "bad stride in op " + std::to_string(k));
            // 'valid' pooling stays inside the input; 'same' (pad_top / pad_left given, or the last window overhanging) may not
            // start a window beyond it
            if (d.op == ECSEG_OP_MAXPOOL && (d.kh <= 0 || d.kw <= 0 || d.pad_top < 0 || d.pad_left < 0 || d.pad_top >= d.kh || d.pad_left >= d.kw ||
                                             (to.h - 1) * d.stride - d.pad_top >= ti.h || (to.w - 1) * d.stride - d.pad_left >= ti.w))
                return fail(h, ECSEG_E_INVALID, "max-pool window leaves the input in op " + std::to_string(k));
            if (d.op == ECSEG_OP_UPSAMPLE && (to.h != ti.h * d.stride || to.w != ti.w * d.stride))
                return fail(h, ECSEG_E_INVALID, "bad upsample shape in op " + std::to_string(k));
        } else if (d.op == ECSEG_OP_GLOBALPOOL) {
            if (to.h != 1 || to.w != 1 || to.c != ti.c) return fail(h, ECSEG_E_INVALID, "bad global-pool shape in op " + std::to_string(k));
        } else if (d.op == ECSEG_OP_ADD) {
            if (d.mode < ECSEG_BIN_ADD || d.mode > ECSEG_BIN_MIN) return fail(h, ECSEG_E_INVALID, "bad binary mode in op " + std::to_string(k));
            for (const ecseg_tensor_desc* tb : {&ti, &tensors[d.in1]})
                if ((tb->h != to.h && tb->h != 1) || (tb->w != to.w && tb->w != 1) || (tb->c != to.c && tb->c != 1))
                    return fail(h, ECSEG_E_INVALID, "shapes cannot be broadcast in op " + std::to_string(k));
        } else if (d.op == ECSEG_OP_ACT || d.op == ECSEG_OP_COPY) {
            // nothing to prepare
        } else {
            return fail(h, ECSEG_E_INVALID, "unknown op code in op " + std::to_string(k));
        }
        if (d.op != ECSEG_OP_CONV && d.op != ECSEG_OP_CONVT && d.op != ECSEG_OP_MAXPOOL && d.op != ECSEG_OP_UPSAMPLE && d.op != ECSEG_OP_DWCONV &&
            d.op != ECSEG_OP_ADD && d.op != ECSEG_OP_COPY && d.op != ECSEG_OP_GLOBALPOOL && (ti.h != to.h || ti.w != to.w || ti.c != to.c))
            return fail(h, ECSEG_E_INVALID, "shape mismatch in element-wise op " + std::to_string(k));
        h->ops.push_back(o);
    }
    // window lanes (run_plan) address the model input and output in plain window order: allowed when their buffers hold
    // only tensors of exactly the buffer's per-window size (keras_plan gives both a buffer of their own)
    h->lanes_ok = true;
    for (int io : {input_tensor, output_tensor}) {
        const int b = h->tensors[io].buffer;
        for (const ecseg_tensor_desc& t : h->tensors)
            if (t.buffer == b && (size_t)t.h * t.w * t.c_stride != std::max<size_t>(h->buf_floats[b], 4)) h->lanes_ok = false;
    }
    h->consumers.assign(n_tensors, 0);
    for (const OpRt& o : h->ops) {
        if (o.d.in0 >= 0) ++h->consumers[o.d.in0];
        if (o.d.op == ECSEG_OP_ADD && o.d.in1 >= 0) ++h->consumers[o.d.in1];
    }
    assign_crop_recipes(h);
    h->has_model = true;
    return ensure_split_images(h);                         // ("winograd" = 3 set before the load)
}

int ecseg_model_flops_per_patch(ecseg_ctx* h, double* flops) {
    int rc = check_model(h);
    if (rc) return rc;
    if (flops) *flops = h->flops_per_patch;
    return ECSEG_OK;
}

}  // extern "C"
