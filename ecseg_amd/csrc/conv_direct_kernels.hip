// Direct (non-matrix-core) convolutions of the plan interpreter for gfx950 (MI355X): small Cin, the first layer, the 1x1 head, the
// generic convolution and transposed convolution, depthwise convolutions.  NHWC float32 views (common.h: TView).
#include "common.h"
#include "device_util.h"

namespace ecseg {

// ------------------------------------------------------------------------------------------------------------
// Direct kernels (HBM-bound layers: first conv with Cin <= 4, the 1x1 head, and generic fall-backs)
// ------------------------------------------------------------------------------------------------------------

// Cin <= 4, Cout % 4 == 0: thread = (pixel, 4 output channels); a wave writes 1 KiB contiguous.
__global__ __launch_bounds__(256) void conv_small_cin_kernel(TView in, TView out, const float* __restrict__ w,
                                                             const float* __restrict__ bias, size_t total, int R, int S,
                                                             int pad_top, int pad_left, int act, float alpha) {
    const int quads = out.c >> 2;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(t % quads);
        size_t pix = t / quads;
        const int ox = (int)(pix % out.w); pix /= out.w;
        const int oy = (int)(pix % out.h);
        const size_t img = pix / out.h;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (bias) acc = *reinterpret_cast<const f32x4*>(bias + q * 4);
        for (int r = 0; r < R; ++r) {
            const int iy = oy - pad_top + r;
            if (iy < 0 || iy >= in.h) continue;
            for (int s = 0; s < S; ++s) {
                const int ix = ox - pad_left + s;
                if (ix < 0 || ix >= in.w) continue;
                const float* ip = in.p + ((img * in.h + iy) * in.w + ix) * in.cs;
                for (int ci = 0; ci < in.c; ++ci) {
                    const float v = ip[ci];
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + ((size_t)((r * S + s) * in.c + ci)) * out.c + q * 4);
                    acc[0] = fmaf(v, wv[0], acc[0]); acc[1] = fmaf(v, wv[1], acc[1]);
                    acc[2] = fmaf(v, wv[2], acc[2]); acc[3] = fmaf(v, wv[3], acc[3]);
                }
            }
        }
        float* op = out.p + ((img * out.h + oy) * out.w + ox) * out.cs + q * 4;
        f32x4 o;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
        o = apply_act4(o, act, alpha);
        *reinterpret_cast<f32x4*>(op) = o;
    }
}

// First layer of the U-Net (Cin = 1, 3x3, 4.4 flop/B: HBM-bound on its output).  Thread = 4 output channels x 8 consecutive
// ROWS of one pixel column: consecutive lanes are the channel quads of a pixel, then the next pixel of the row, so that every
// store instruction of a wave writes 1 KiB of CONTIGUOUS output (16 pixels x 64 B at 16 channels, 4 pixels x 256 B at 64) -
// with the 8 pixels of a thread along the row instead (rounds 1-2) a store instruction wrote 16 separate 64-byte pieces
// 512 bytes apart at 16 channels and the layer ran at 2.1 - 2.5 TB/s.  The nine filter taps live in registers; the 10 x 3
// input window streams through three registers per row (lanes of one pixel read the same address: one broadcast fetch).
__global__ __launch_bounds__(256) void conv_first_kernel(TView in, TView out, const float* __restrict__ w,
                                                         const float* __restrict__ bias, size_t total, int pad_top,
                                                         int pad_left, int act, float alpha) {
    constexpr int PY = 8;
    const int quads = out.c >> 2;
    const int gy = (out.h + PY - 1) / PY;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int q = (int)(t % quads);
        size_t g = t / quads;
        const int ox = (int)(g % out.w); g /= out.w;
        const int y0 = (int)(g % gy) * PY;
        const size_t img = g / gy;
        f32x4 wt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wt[k] = *reinterpret_cast<const f32x4*>(w + (size_t)k * out.c + q * 4);
        f32x4 acc[PY];
        const f32x4 b4 = bias ? *reinterpret_cast<const f32x4*>(bias + q * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < PY; ++i) acc[i] = b4;
        const float* col = in.p + (img * in.h * in.w) * in.cs;
#pragma unroll
        for (int r = 0; r < PY + 2; ++r) {                   // input row r of the window feeds output rows r - 2 .. r
            const int iy = y0 - pad_top + r;
            float v[3];
#pragma unroll
            for (int sx = 0; sx < 3; ++sx) {
                const int ix = ox - pad_left + sx;
                v[sx] = (iy >= 0 && iy < in.h && ix >= 0 && ix < in.w) ? col[((size_t)iy * in.w + ix) * in.cs] : 0.f;
            }
#pragma unroll
            for (int kr = 0; kr < 3; ++kr) {
                const int i = r - kr;                         // output row of the thread that sees this input row as tap row kr
                if (i < 0 || i >= PY) continue;
#pragma unroll
                for (int sx = 0; sx < 3; ++sx) {
                    const f32x4 k4 = wt[kr * 3 + sx];
                    acc[i][0] = fmaf(v[sx], k4[0], acc[i][0]); acc[i][1] = fmaf(v[sx], k4[1], acc[i][1]);
                    acc[i][2] = fmaf(v[sx], k4[2], acc[i][2]); acc[i][3] = fmaf(v[sx], k4[3], acc[i][3]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < PY; ++i) {
            if (y0 + i < out.h) {
                f32x4 o;
                o[0] = acc[i][0]; o[1] = acc[i][1]; o[2] = acc[i][2]; o[3] = acc[i][3];
                o = apply_act4(o, act, alpha);
                __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(out.p + ((img * out.h + y0 + i) * out.w + ox) * out.cs + q * 4));
            }
        }
    }
}

hipError_t launch_conv_small_cin(const TView& in, const TView& out, const float* w, const float* bias, int n, int R, int S,
                                 int pad_top, int pad_left, int act, float alpha, hipStream_t s) {
    if (in.c == 1 && R == 3 && S == 3) {
        const size_t tot = (size_t)n * ((out.h + 7) / 8) * out.w * (out.c / 4);
        if (!tot) return hipSuccess;
        hipLaunchKernelGGL(conv_first_kernel, dim3(grid_for(tot)), dim3(256), 0, s, in, out, w, bias, tot, pad_top, pad_left, act, alpha);
        return hipGetLastError();
    }
    const size_t total = (size_t)n * out.h * out.w * (out.c / 4);
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(conv_small_cin_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, w, bias, total, R, S, pad_top,
                       pad_left, act, alpha);
    return hipGetLastError();
}

// 1x1 conv with few outputs (the 4-class head) + optional channel softmax.  LPP lanes share one pixel (16 at Cin >= 64,
// 8 / 4 for narrower inputs - with 16 lanes on a 16-channel pixel twelve of them idled and the layer ran at 1 TB/s): each
// lane reads float4 slices of the pixel's channel vector (256 B contiguous per pixel at Cin = 64), partial sums are
// reduced with wave shuffles, lane 0 of the group finishes bias / softmax and writes the pixel.
template <int COUT, int LPP>
__global__ __launch_bounds__(256) void conv_head_kernel(TView in, TView out, const float* __restrict__ w,
                                                        const float* __restrict__ bias, size_t npix, int act, float alpha) {
    constexpr int PPW = 64 / LPP;                              // pixels per wave
    const int sub = threadIdx.x & (LPP - 1);
    const int c4n = in.c >> 2;
    for (size_t pix = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / LPP; ; pix += ((size_t)gridDim.x * blockDim.x) / LPP) {
        // all LPP lanes of a group share `pix`; groups of one wave may run out at different times, so keep the whole
        // wave in the loop and mask the work instead of breaking (shuffles need every lane present)
        const size_t wave_first = pix - (((size_t)threadIdx.x & 63) / LPP);
        if (wave_first >= npix) break;
        (void)PPW;
        const bool live = pix < npix;
        float acc[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
        if (live) {
            const float* ip = in.p + pix * in.cs;
            for (int c4 = sub; c4 < c4n; c4 += LPP) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(ip + c4 * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* wr = w + (size_t)(c4 * 4 + e) * COUT;
#pragma unroll
                    for (int o = 0; o < COUT; ++o) acc[o] = fmaf(v[e], wr[o], acc[o]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < COUT; ++o) {
            float v = acc[o];
#pragma unroll
            for (int d = LPP / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
            acc[o] = v;
        }
        if (live && sub == 0) {
#pragma unroll
            for (int o = 0; o < COUT; ++o) acc[o] += bias ? bias[o] : 0.f;
            if (act == ECSEG_ACT_SOFTMAX) {
                float m = acc[0];
#pragma unroll
                for (int o = 1; o < COUT; ++o) m = fmaxf(m, acc[o]);
                float sum = 0.f;
#pragma unroll
                for (int o = 0; o < COUT; ++o) { acc[o] = expf(acc[o] - m); sum += acc[o]; }
#pragma unroll
                for (int o = 0; o < COUT; ++o) acc[o] = acc[o] / sum;
            } else {
#pragma unroll
                for (int o = 0; o < COUT; ++o) acc[o] = apply_act(acc[o], act, alpha);
            }
            float* op = out.p + pix * out.cs;
#pragma unroll
            for (int o = 0; o < COUT; ++o) op[o] = acc[o];
        }
    }
}

template <int LPP>
static hipError_t launch_conv_head_l(const TView& in, const TView& out, const float* w, const float* bias, size_t npix, int act,
                                     float alpha, hipStream_t s) {
    size_t blocks = (npix * LPP + 255) / 256;
    if (blocks > 65536 * 8) blocks = 65536 * 8;
#define HEAD_CASE(C) case C: hipLaunchKernelGGL((conv_head_kernel<C, LPP>), dim3((unsigned)blocks), dim3(256), 0, s, in, out, w, bias, npix, act, alpha); break;
    switch (out.c) {
        HEAD_CASE(1) HEAD_CASE(2) HEAD_CASE(3) HEAD_CASE(4) HEAD_CASE(5) HEAD_CASE(6) HEAD_CASE(7) HEAD_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef HEAD_CASE
    return hipGetLastError();
}

hipError_t launch_conv_head(const TView& in, const TView& out, const float* w, const float* bias, int n, int act,
                            float alpha, hipStream_t s) {
    const size_t npix = (size_t)n * out.h * out.w;
    if (!npix) return hipSuccess;
    const int c4n = in.c >> 2;                               // lanes per pixel: as many as there are 4-channel slices, up to 16
    if (c4n >= 16) return launch_conv_head_l<16>(in, out, w, bias, npix, act, alpha, s);
    if (c4n >= 8) return launch_conv_head_l<8>(in, out, w, bias, npix, act, alpha, s);
    return launch_conv_head_l<4>(in, out, w, bias, npix, act, alpha, s);
}

// Generic direct convolution: thread = (pixel, output channel), with dilation rates and per-axis strides.  Correctness fall-back for
// shapes the MFMA kernels do not take (odd channel counts, large taps, Cin % 4 != 0, unaligned views) and for every layer with
// ANISOTROPIC strides / dilation rates.
__global__ __launch_bounds__(256) void conv_generic_kernel(TView in, TView out, const float* __restrict__ w, const float* __restrict__ bias,
                                                           size_t total, int R, int S, int stride, int stride_x, int dil, int dil_x, int pad_top, int pad_left,
                                                           int act, float alpha) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(t % out.c);
        size_t pix = t / out.c;
        const int ox = (int)(pix % out.w); pix /= out.w;
        const int oy = (int)(pix % out.h);
        const size_t img = pix / out.h;
        float acc = bias ? bias[co] : 0.f;
        for (int r = 0; r < R; ++r) {
            const int iy = oy * stride - pad_top + r * dil;
            if (iy < 0 || iy >= in.h) continue;
            for (int s = 0; s < S; ++s) {
                const int ix = ox * stride_x - pad_left + s * dil_x;
                if (ix < 0 || ix >= in.w) continue;
                const float* ip = in.p + ((img * in.h + iy) * in.w + ix) * in.cs;
                const float* wp = w + (size_t)(r * S + s) * in.c * out.c + co;
                for (int ci = 0; ci < in.c; ++ci) acc = fmaf(ip[ci], wp[(size_t)ci * out.c], acc);
            }
        }
        out.p[((img * out.h + oy) * out.w + ox) * out.cs + co] = apply_act(acc, act, alpha);
    }
}

hipError_t launch_conv_generic(const TView& in, const TView& out, const float* w, const float* bias, int n, int R, int S, int stride, int stride_x,
                               int dil, int dil_x, int pad_top, int pad_left, int act, float alpha, hipStream_t s) {
    const size_t total = (size_t)n * out.h * out.w * out.c;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(conv_generic_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, w, bias, total, R, S, stride, stride_x,
                       dil < 1 ? 1 : dil, dil_x < 1 ? 1 : dil_x, pad_top, pad_left, act, alpha);
    return hipGetLastError();
}

// Generic transposed convolution (Keras kernel layout (kh, kw, out, in)): thread = (output pixel, output channel),
// gathers every (input pixel, tap) pair that lands on it.
__global__ __launch_bounds__(256) void convt_generic_kernel(TView in, TView out, const float* __restrict__ w,
                                                            const float* __restrict__ bias, size_t total, int R, int S,
                                                            int stride, int crop_top, int crop_left, int act, float alpha) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(t % out.c);
        size_t pix = t / out.c;
        const int ox = (int)(pix % out.w); pix /= out.w;
        const int oy = (int)(pix % out.h);
        const size_t img = pix / out.h;
        float acc = bias ? bias[co] : 0.f;
        const int fy = oy + crop_top, fx = ox + crop_left;   // coordinates in the uncropped output
        for (int a = 0; a < R; ++a) {
            const int ny = fy - a;
            if (ny < 0 || ny % stride) continue;
            const int iy = ny / stride;
            if (iy >= in.h) continue;
            for (int b = 0; b < S; ++b) {
                const int nx = fx - b;
                if (nx < 0 || nx % stride) continue;
                const int ix = nx / stride;
                if (ix >= in.w) continue;
                const float* ip = in.p + ((img * in.h + iy) * in.w + ix) * in.cs;
                const float* wp = w + ((size_t)(a * S + b) * out.c + co) * in.c;
                for (int ci = 0; ci < in.c; ++ci) acc = fmaf(ip[ci], wp[ci], acc);
            }
        }
        out.p[((img * out.h + oy) * out.w + ox) * out.cs + co] = apply_act(acc, act, alpha);
    }
}

hipError_t launch_convt_generic(const TView& in, const TView& out, const float* w, const float* bias, int n, int R, int S,
                                int stride, int crop_top, int crop_left, int act, float alpha, hipStream_t s) {
    const size_t total = (size_t)n * out.h * out.w * out.c;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(convt_generic_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, w, bias, total, R, S, stride,
                       crop_top, crop_left, act, alpha);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------
// DepthwiseConv2D (depth multiplier 1, channels % 4 == 0): HBM-bound - every input value is used kh * kw times by
// neighbouring outputs of ITS channel only, so the work is one pass over the tensor if the halo is kept on chip.
// Workgroup = DW_TY x DW_TX output pixels x CQ channel quads (<= 64 channels): the input halo of the tile is staged in
// LDS with 16-byte loads (consecutive lanes = consecutive channel quads of a pixel: 256 contiguous bytes per pixel at 64
// channels), every work item then reads its kh * kw taps from LDS (consecutive lanes = consecutive 16-byte slots:
// conflict-free) and writes 4 channels with one 16-byte store.  Filter [tap][channel] (Keras' (kh, kw, cin, 1)) in LDS too.
// LDS == false: the same arithmetic straight from global memory (L2), for halos that do not fit 64 KB.
// ------------------------------------------------------------------------------------------------------------
constexpr int DW_TY = 8, DW_TX = 8;

template <bool LDS>
__global__ __launch_bounds__(256) void dwconv_kernel(TView in, TView out, const float* __restrict__ w, const float* __restrict__ bias,
                                                     int kh, int kw, int stride, int dil, int pad_top, int pad_left, int act,
                                                     float alpha, int tiles_x, int tiles_y, int cq, int nblk_c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    unsigned bid = blockIdx.x;
    const int cb = bid % nblk_c; bid /= nblk_c;
    const int bx = bid % tiles_x; bid /= tiles_x;
    const int by = bid % tiles_y; bid /= tiles_y;
    const size_t img = bid;
    const int q0 = cb * cq;                                   // first channel quad of this workgroup
    const int nq = min(cq, in.c / 4 - q0);
    const int oy0 = by * DW_TY, ox0 = bx * DW_TX;
    const int hh = (DW_TY - 1) * stride + (kh - 1) * dil + 1, hw = (DW_TX - 1) * stride + (kw - 1) * dil + 1;
    const int iy0 = oy0 * stride - pad_top, ix0 = ox0 * stride - pad_left;
    f32x4* Hs = reinterpret_cast<f32x4*>(smem);              // [hh][hw][cq]
    f32x4* Ws = Hs + (LDS ? hh * hw * cq : 0);               // [kh * kw][cq]
    const float* ip = in.p + img * (size_t)in.h * in.w * in.cs + q0 * 4;
    for (int t = tid; t < kh * kw * cq; t += 256) {
        const int tap = t / cq, q = t - tap * cq;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < nq) v = *reinterpret_cast<const f32x4*>(w + (size_t)tap * in.c + (q0 + q) * 4);
        Ws[t] = v;
    }
    if (LDS) {
        for (int t = tid; t < hh * hw * cq; t += 256) {
            const int q = t % cq, pix = t / cq;
            const int hy = pix / hw, hx = pix - hy * hw;
            const int iy = iy0 + hy, ix = ix0 + hx;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q < nq && iy >= 0 && iy < in.h && ix >= 0 && ix < in.w)
                v = *reinterpret_cast<const f32x4*>(ip + ((size_t)iy * in.w + ix) * in.cs + q * 4);
            Hs[t] = v;
        }
    }
    __syncthreads();
    for (int t = tid; t < DW_TY * DW_TX * cq; t += 256) {
        const int q = t % cq, pix = t / cq;
        const int py = pix / DW_TX, px = pix - py * DW_TX;
        const int oy = oy0 + py, ox = ox0 + px;
        if (q >= nq || oy >= out.h || ox >= out.w) continue;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (bias != nullptr) acc = *reinterpret_cast<const f32x4*>(bias + (q0 + q) * 4);
        for (int r = 0; r < kh; ++r)
            for (int s = 0; s < kw; ++s) {
                f32x4 v;
                if (LDS) v = Hs[((py * stride + r * dil) * hw + px * stride + s * dil) * cq + q];
                else {
                    const int iy = iy0 + py * stride + r * dil, ix = ix0 + px * stride + s * dil;
                    v = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (iy >= 0 && iy < in.h && ix >= 0 && ix < in.w) v = *reinterpret_cast<const f32x4*>(ip + ((size_t)iy * in.w + ix) * in.cs + q * 4);
                }
                const f32x4 k4 = Ws[(r * kw + s) * cq + q];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = fmaf(v[c], k4[c], acc[c]);
            }
        acc = apply_act_ext4(acc, act, alpha);
        *reinterpret_cast<f32x4*>(out.p + ((img * out.h + oy) * out.w + ox) * out.cs + (q0 + q) * 4) = acc;
    }
}

// Any depth multiplier / channel count / alignment: thread = (output pixel, output channel); kernel (kh, kw, cin, mult)
__global__ __launch_bounds__(256) void dwconv_generic_kernel(TView in, TView out, const float* __restrict__ w, const float* __restrict__ bias,
                                                             size_t total, int kh, int kw, int stride, int dil, int pad_top, int pad_left,
                                                             int mult, int act, float alpha) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(t % out.c);
        size_t pix = t / out.c;
        const int ox = (int)(pix % out.w); pix /= out.w;
        const int oy = (int)(pix % out.h);
        const size_t img = pix / out.h;
        const int ci = co / mult;
        float acc = bias ? bias[co] : 0.f;
        for (int r = 0; r < kh; ++r) {
            const int iy = oy * stride - pad_top + r * dil;
            if (iy < 0 || iy >= in.h) continue;
            for (int s = 0; s < kw; ++s) {
                const int ix = ox * stride - pad_left + s * dil;
                if (ix < 0 || ix >= in.w) continue;
                acc = fmaf(in.p[((img * in.h + iy) * in.w + ix) * in.cs + ci], w[(size_t)(r * kw + s) * out.c + co], acc);
            }
        }
        out.p[((img * out.h + oy) * out.w + ox) * out.cs + co] = apply_act_ext(acc, act, alpha);
    }
}

hipError_t launch_dwconv(const TView& in, const TView& out, const float* w, const float* bias, int n, int kh, int kw, int stride,
                         int dil, int pad_top, int pad_left, int mult, int act, float alpha, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (dil < 1) dil = 1;
    const bool vec = mult == 1 && in.c % 4 == 0 && in.cs % 4 == 0 && out.cs % 4 == 0 && out.c == in.c &&
                     ((((uintptr_t)in.p) | ((uintptr_t)out.p)) & 15) == 0 && (bias == nullptr || (((uintptr_t)bias) & 15) == 0) &&
                     (((uintptr_t)w) & 15) == 0;
    if (!vec) {
        const size_t total = (size_t)n * out.h * out.w * out.c;
        if (!total) return hipSuccess;
        hipLaunchKernelGGL(dwconv_generic_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, w, bias, total, kh, kw, stride, dil,
                           pad_top, pad_left, mult, act, alpha);
        return hipGetLastError();
    }
    const int quads = in.c / 4;
    const int cq = quads < 16 ? quads : 16;
    const int nblk_c = (quads + cq - 1) / cq;
    const int tiles_x = (out.w + DW_TX - 1) / DW_TX, tiles_y = (out.h + DW_TY - 1) / DW_TY;
    const size_t grid = (size_t)n * tiles_x * tiles_y * nblk_c;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t hh = (size_t)(DW_TY - 1) * stride + (size_t)(kh - 1) * dil + 1, hw = (size_t)(DW_TX - 1) * stride + (size_t)(kw - 1) * dil + 1;
    const size_t halo = hh * hw * cq * 16, wbytes = (size_t)kh * kw * cq * 16;
    if (wbytes > 60000) {                                       // (a > 60 x 60-tap depthwise kernel)
        const size_t total = (size_t)n * out.h * out.w * out.c;
        hipLaunchKernelGGL(dwconv_generic_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, w, bias, total, kh, kw, stride, dil,
                           pad_top, pad_left, mult, act, alpha);
        return hipGetLastError();
    }
    if (halo + wbytes <= 64 * 1024)
        hipLaunchKernelGGL(dwconv_kernel<true>, dim3((unsigned)grid), dim3(256), halo + wbytes, s, in, out, w, bias, kh, kw, stride, dil,
                           pad_top, pad_left, act, alpha, tiles_x, tiles_y, cq, nblk_c);
    else
        hipLaunchKernelGGL(dwconv_kernel<false>, dim3((unsigned)grid), dim3(256), wbytes, s, in, out, w, bias, kh, kw, stride, dil,
                           pad_top, pad_left, act, alpha, tiles_x, tiles_y, cq, nblk_c);
    return hipGetLastError();
}

}  // namespace ecseg
