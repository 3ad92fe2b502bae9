// Every plan-interpreter kernel that is not a convolution, for gfx950 (MI355X): pooling ('valid', 'same', global), up-sampling,
// affine / activation, binary ops with broadcasting (Add / Multiply / Subtract / Maximum / Minimum), PReLU, LayerNormalization,
// pad / crop / copy, softmax, and the input side (u8_to_f32, tile_patches).  NHWC float32 views (common.h: TView).
#include "common.h"
#include "device_util.h"

namespace ecseg {

// ------------------------------------------------------------------------------------------------------------
// Element-wise / resampling kernels (HBM-bound; float4 fast path when every view is 16-byte aligned)
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool view_vec4(const TView& v) {
    return (v.c % 4 == 0) && (v.cs % 4 == 0) && ((((uintptr_t)v.p) & 15) == 0);
}

// MaxPooling2D (mode 0) / AveragePooling2D (mode 1), 'valid'
template <bool VEC>
__global__ __launch_bounds__(256) void maxpool_kernel(TView in, TView out, size_t total, int kh, int kw, int stride, int mode) {
    constexpr int V = VEC ? 4 : 1;
    const int cq = out.c / V;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(t % cq) * V;
        size_t pix = t / cq;
        const int ox = (int)(pix % out.w); pix /= out.w;
        const int oy = (int)(pix % out.h);
        const size_t img = pix / out.h;
        float m[V];
#pragma unroll
        for (int e = 0; e < V; ++e) m[e] = mode ? 0.f : -INFINITY;
        for (int r = 0; r < kh; ++r)
            for (int s = 0; s < kw; ++s) {
                const float* ip = in.p + ((img * in.h + (oy * stride + r)) * in.w + (ox * stride + s)) * in.cs + c;
                if (VEC) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(ip);
#pragma unroll
                    for (int e = 0; e < V; ++e) m[e] = mode ? m[e] + v[e] : fmaxf(m[e], v[e]);
                } else {
                    m[0] = mode ? m[0] + ip[0] : fmaxf(m[0], ip[0]);
                }
            }
        if (mode) {
            const float inv = 1.f / (float)(kh * kw);
#pragma unroll
            for (int e = 0; e < V; ++e) m[e] *= inv;
        }
        float* op = out.p + ((img * out.h + oy) * out.w + ox) * out.cs + c;
        if (VEC) {
            f32x4 o; o[0] = m[0]; o[1] = m[V > 1 ? 1 : 0]; o[2] = m[V > 2 ? 2 : 0]; o[3] = m[V > 3 ? 3 : 0];
            *reinterpret_cast<f32x4*>(op) = o;
        } else {
            op[0] = m[0];
        }
    }
}

hipError_t launch_maxpool(const TView& in, const TView& out, int n, int kh, int kw, int stride, int mode, hipStream_t s) {
    const bool vec = (in.c % 4 == 0) && (in.cs % 4 == 0) && (out.cs % 4 == 0) && ((((uintptr_t)in.p) | ((uintptr_t)out.p)) & 15) == 0;
    const size_t total = (size_t)n * out.h * out.w * (vec ? out.c / 4 : out.c);
    if (!total) return hipSuccess;
    if (vec) hipLaunchKernelGGL(maxpool_kernel<true>, dim3(grid_for(total)), dim3(256), 0, s, in, out, total, kh, kw, stride, mode);
    else hipLaunchKernelGGL(maxpool_kernel<false>, dim3(grid_for(total)), dim3(256), 0, s, in, out, total, kh, kw, stride, mode);
    return hipGetLastError();
}

// MaxPooling2D / AveragePooling2D with padding='same': the window starts (pad_top, pad_left) before the input; the maximum
// and the average run over the pixels that lie inside it (TensorFlow's average excludes the padding from the divisor)
__global__ __launch_bounds__(256) void pool_pad_kernel(TView in, TView out, size_t total, int kh, int kw, int stride, int pad_top,
                                                       int pad_left, int mode) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(t % out.c);
        size_t pix = t / out.c;
        const int ox = (int)(pix % out.w); pix /= out.w;
        const int oy = (int)(pix % out.h);
        const size_t img = pix / out.h;
        float m = mode ? 0.f : -INFINITY;
        int cnt = 0;
        for (int r = 0; r < kh; ++r) {
            const int iy = oy * stride - pad_top + r;
            if (iy < 0 || iy >= in.h) continue;
            for (int s = 0; s < kw; ++s) {
                const int ix = ox * stride - pad_left + s;
                if (ix < 0 || ix >= in.w) continue;
                const float v = in.p[((img * in.h + iy) * in.w + ix) * in.cs + c];
                m = mode ? m + v : fmaxf(m, v);
                ++cnt;
            }
        }
        if (mode) m = cnt ? m / (float)cnt : 0.f;
        out.p[((img * out.h + oy) * out.w + ox) * out.cs + c] = m;
    }
}

hipError_t launch_pool_pad(const TView& in, const TView& out, int n, int kh, int kw, int stride, int pad_top, int pad_left, int mode,
                           hipStream_t s) {
    const size_t total = (size_t)n * out.h * out.w * out.c;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(pool_pad_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, total, kh, kw, stride, pad_top, pad_left, mode);
    return hipGetLastError();
}

// GlobalAveragePooling2D (mode 1) / GlobalMaxPooling2D (mode 0): workgroup = (patch, 64 channels); lane = channel
// (coalesced 256-B rows), the four waves split the pixels and meet in LDS.  Fixed summation order: run-to-run identical.
__global__ __launch_bounds__(256) void global_pool_kernel(TView in, TView out, int mode) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const size_t img = blockIdx.y;
    const int npx = in.h * in.w;
    float acc = mode ? 0.f : -INFINITY;
    if (c < in.c) {
        const float* ip = in.p + img * (size_t)npx * in.cs + c;
        for (int q = wave; q < npx; q += 4) {
            const float v = ip[(size_t)q * in.cs];
            acc = mode ? acc + v : fmaxf(acc, v);
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && c < in.c) {
        float r = part[0][lane];
#pragma unroll
        for (int k = 1; k < 4; ++k) r = mode ? r + part[k][lane] : fmaxf(r, part[k][lane]);
        if (mode) r *= 1.f / (float)npx;
        out.p[img * (size_t)out.cs + c] = r;
    }
}

hipError_t launch_global_pool(const TView& in, const TView& out, int n, int mode, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(global_pool_kernel, dim3((unsigned)((in.c + 63) / 64), (unsigned)n), dim3(256), 0, s, in, out, mode);
    return hipGetLastError();
}

template <bool VEC>
__global__ __launch_bounds__(256) void upsample_kernel(TView in, TView out, size_t total, int f, int mode) {
    constexpr int V = VEC ? 4 : 1;
    const int cq = out.c / V;
    const float inv = 1.f / (float)f;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(t % cq) * V;
        size_t pix = t / cq;
        const int ox = (int)(pix % out.w); pix /= out.w;
        const int oy = (int)(pix % out.h);
        const size_t img = pix / out.h;
        float o[V];
        if (mode == 0) {
            const float* ip = in.p + ((img * in.h + oy / f) * in.w + ox / f) * in.cs + c;
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = ip[e];
        } else {
            // half-pixel centres: src = (dst + 0.5) / f - 0.5, edges clamped
            const float sy = ((float)oy + 0.5f) * inv - 0.5f, sx = ((float)ox + 0.5f) * inv - 0.5f;
            const float fy = floorf(sy), fx = floorf(sx);
            const int y0 = max((int)fy, 0), y1 = min((int)ceilf(sy), in.h - 1);
            const int x0 = max((int)fx, 0), x1 = min((int)ceilf(sx), in.w - 1);
            const float ly = sy - fy, lx = sx - fx;
            const float* r0 = in.p + (img * in.h + y0) * (size_t)in.w * in.cs + c;
            const float* r1 = in.p + (img * in.h + min(y1, in.h - 1)) * (size_t)in.w * in.cs + c;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float tl = r0[(size_t)x0 * in.cs + e], tr = r0[(size_t)x1 * in.cs + e];
                const float bl = r1[(size_t)x0 * in.cs + e], br = r1[(size_t)x1 * in.cs + e];
                const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
                o[e] = top + (bot - top) * ly;
            }
        }
        float* op = out.p + ((img * out.h + oy) * out.w + ox) * out.cs + c;
#pragma unroll
        for (int e = 0; e < V; ++e) op[e] = o[e];
    }
}

hipError_t launch_upsample(const TView& in, const TView& out, int n, int factor, int mode, hipStream_t s) {
    const bool vec = (in.c % 4 == 0);
    const size_t total = (size_t)n * out.h * out.w * (vec ? out.c / 4 : out.c);
    if (!total) return hipSuccess;
    if (vec) hipLaunchKernelGGL(upsample_kernel<true>, dim3(grid_for(total)), dim3(256), 0, s, in, out, total, factor, mode);
    else hipLaunchKernelGGL(upsample_kernel<false>, dim3(grid_for(total)), dim3(256), 0, s, in, out, total, factor, mode);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void affine_kernel(TView in, TView out, const float* __restrict__ scale,
                                                     const float* __restrict__ shift, size_t total, int act, float alpha) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(t % out.c);
        const size_t pix = t / out.c;
        float v = in.p[pix * in.cs + c];
        if (scale) v = v * scale[c] + shift[c];
        out.p[pix * out.cs + c] = apply_act_ext(v, act, alpha);
    }
}

hipError_t launch_affine(const TView& in, const TView& out, const float* scale, const float* shift, int n, int act,
                         float alpha, hipStream_t s) {
    const size_t total = (size_t)n * out.h * out.w * out.c;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(affine_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, scale, shift, total, act, alpha);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------
// y = act(a (+) b) with numpy-style broadcasting of extents of 1 (h, w, c of either input)
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bin_op(float a, float b, int mode) {
    switch (mode) {
        case ECSEG_BIN_MUL: return a * b;
        case ECSEG_BIN_SUB: return a - b;
        case ECSEG_BIN_MAX: return fmaxf(a, b);
        case ECSEG_BIN_MIN: return fminf(a, b);
        default: return a + b;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void binary_kernel(TView a, TView b, TView out, size_t total, int mode, int act, float alpha) {
    constexpr int V = VEC ? 4 : 1;
    const int cq = out.c / V;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(t % cq) * V;
        size_t pix = t / cq;
        const int x = (int)(pix % out.w); pix /= out.w;
        const int y = (int)(pix % out.h);
        const size_t img = pix / out.h;
        const float* ap = a.p + ((img * a.h + (a.h > 1 ? y : 0)) * a.w + (a.w > 1 ? x : 0)) * a.cs + (a.c > 1 ? c : 0);
        const float* bp = b.p + ((img * b.h + (b.h > 1 ? y : 0)) * b.w + (b.w > 1 ? x : 0)) * b.cs + (b.c > 1 ? c : 0);
        float* op = out.p + ((img * out.h + y) * out.w + x) * out.cs + c;
        if (VEC) {                                            // (both inputs carry all channels)
            const f32x4 av = *reinterpret_cast<const f32x4*>(ap), bv = *reinterpret_cast<const f32x4*>(bp);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = bin_op(av[e], bv[e], mode);
            *reinterpret_cast<f32x4*>(op) = apply_act_ext4(o, act, alpha);
        } else {
            op[0] = apply_act_ext(bin_op(ap[0], bp[0], mode), act, alpha);
        }
    }
}

hipError_t launch_binary(const TView& a, const TView& b, const TView& out, int n, int mode, int act, float alpha, hipStream_t s) {
    auto v4 = [&](const TView& v) { return v.c == out.c && v.c % 4 == 0 && v.cs % 4 == 0 && ((((uintptr_t)v.p) & 15) == 0); };
    const bool vec = v4(a) && v4(b) && v4(out);
    const size_t total = (size_t)n * out.h * out.w * (vec ? out.c / 4 : out.c);
    if (!total) return hipSuccess;
    if (vec) hipLaunchKernelGGL(binary_kernel<true>, dim3(grid_for(total)), dim3(256), 0, s, a, b, out, total, mode, act, alpha);
    else hipLaunchKernelGGL(binary_kernel<false>, dim3(grid_for(total)), dim3(256), 0, s, a, b, out, total, mode, act, alpha);
    return hipGetLastError();
}

// PReLU: slope per channel (per_element == 0) or per (y, x, channel) of the patch
__global__ __launch_bounds__(256) void prelu_kernel(TView in, TView out, const float* __restrict__ slope, size_t total, int per_element) {
    const size_t per_patch = (size_t)out.h * out.w;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(t % out.c);
        const size_t pix = t / out.c;
        const float v = in.p[pix * in.cs + c];
        const float a = slope[per_element ? (pix % per_patch) * out.c + c : (size_t)c];
        out.p[pix * out.cs + c] = v > 0.f ? v : a * v;
    }
}

hipError_t launch_prelu(const TView& in, const TView& out, const float* slope, int n, int per_element, hipStream_t s) {
    const size_t total = (size_t)n * out.h * out.w * out.c;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(prelu_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, slope, total, per_element);
    return hipGetLastError();
}

// LayerNormalization over the channels of a pixel: LPP lanes share one pixel (strided channel reads, shuffle reductions);
// mean, then variance of the centred values (tf.nn.moments), then x * inv + (beta - mean * inv) with inv = rsqrt(var + eps) * gamma
template <int LPP>
__global__ __launch_bounds__(256) void layernorm_kernel(TView in, TView out, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        size_t npix, float eps) {
    const int sub = threadIdx.x & (LPP - 1);
    const float inv_c = 1.f / (float)in.c;
    for (size_t pix = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / LPP; ; pix += ((size_t)gridDim.x * blockDim.x) / LPP) {
        const size_t wave_first = pix - (((size_t)threadIdx.x & 63) / LPP);
        if (wave_first >= npix) break;                        // (whole waves stay in the loop: the shuffles need every lane)
        const bool live = pix < npix;
        const float* ip = in.p + (live ? pix : 0) * in.cs;
        float sum = 0.f;
        if (live) for (int c = sub; c < in.c; c += LPP) sum += ip[c];
#pragma unroll
        for (int d = LPP / 2; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        const float mean = sum * inv_c;
        float sq = 0.f;
        if (live) for (int c = sub; c < in.c; c += LPP) { const float dlt = ip[c] - mean; sq = fmaf(dlt, dlt, sq); }
#pragma unroll
        for (int d = LPP / 2; d >= 1; d >>= 1) sq += __shfl_xor(sq, d, 64);
        const float rstd = rsqrtf(sq * inv_c + eps);
        if (live) {
            float* op = out.p + pix * out.cs;
            for (int c = sub; c < in.c; c += LPP) {
                const float inv = rstd * (gamma ? gamma[c] : 1.f);
                op[c] = fmaf(ip[c], inv, (beta ? beta[c] : 0.f) - mean * inv);
            }
        }
    }
}

hipError_t launch_layernorm(const TView& in, const TView& out, const float* gamma, const float* beta, int n, float eps, hipStream_t s) {
    const size_t npix = (size_t)n * out.h * out.w;
    if (!npix) return hipSuccess;
    if (in.c >= 64) {
        size_t blocks = (npix * 64 + 255) / 256; if (blocks > 65536 * 8) blocks = 65536 * 8;
        hipLaunchKernelGGL(layernorm_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, s, in, out, gamma, beta, npix, eps);
    } else if (in.c >= 16) {
        size_t blocks = (npix * 16 + 255) / 256; if (blocks > 65536 * 8) blocks = 65536 * 8;
        hipLaunchKernelGGL(layernorm_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, s, in, out, gamma, beta, npix, eps);
    } else {
        size_t blocks = (npix * 4 + 255) / 256; if (blocks > 65536 * 8) blocks = 65536 * 8;
        hipLaunchKernelGGL(layernorm_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, in, out, gamma, beta, npix, eps);
    }
    return hipGetLastError();
}

// y[oy][ox] = x[oy - off_y][ox - off_x] or 0 outside: ZeroPadding2D (off > 0), Cropping2D (off < 0), plain copy (0)
__global__ __launch_bounds__(256) void copy_kernel(TView in, TView out, size_t total, int off_y, int off_x) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(t % out.c);
        size_t pix = t / out.c;
        const int ox = (int)(pix % out.w); pix /= out.w;
        const int oy = (int)(pix % out.h);
        const size_t img = pix / out.h;
        const int iy = oy - off_y, ix = ox - off_x;
        float v = 0.f;
        if (iy >= 0 && iy < in.h && ix >= 0 && ix < in.w) v = in.p[((img * in.h + iy) * in.w + ix) * in.cs + c];
        out.p[((img * out.h + oy) * out.w + ox) * out.cs + c] = v;
    }
}

hipError_t launch_copy(const TView& in, const TView& out, int n, int off_y, int off_x, hipStream_t s) {
    const size_t total = (size_t)n * out.h * out.w * out.c;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(copy_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, total, off_y, off_x);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void softmax_kernel(TView in, TView out, size_t npix) {
    for (size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pix < npix; pix += (size_t)gridDim.x * blockDim.x) {
        const float* ip = in.p + pix * in.cs;
        float* op = out.p + pix * out.cs;
        float m = ip[0];
        for (int c = 1; c < in.c; ++c) m = fmaxf(m, ip[c]);
        float sum = 0.f;
        for (int c = 0; c < in.c; ++c) sum += expf(ip[c] - m);
        for (int c = 0; c < in.c; ++c) op[c] = expf(ip[c] - m) / sum;
    }
}

hipError_t launch_softmax(const TView& in, const TView& out, int n, hipStream_t s) {
    const size_t npix = (size_t)n * out.h * out.w;
    if (!npix) return hipSuccess;
    hipLaunchKernelGGL(softmax_kernel, dim3(grid_for(npix)), dim3(256), 0, s, in, out, npix);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void u8_to_f32_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, size_t count) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (size_t)gridDim.x * blockDim.x)
        out[t] = (float)in[t];
}

hipError_t launch_u8_to_f32(const uint8_t* in, float* out, size_t count, hipStream_t s) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(u8_to_f32_kernel, dim3(grid_for(count)), dim3(256), 0, s, in, out, count);
    return hipGetLastError();
}

// im2patches_overlap (reference src/image_tools.py:181-184): patch k of image i = gray[i, y0:y0+256, x0:x0+256]
__global__ __launch_bounds__(256) void tile_patches_kernel(const uint8_t* __restrict__ gray, int H, int W,
                                                           const int32_t* __restrict__ pos, int n_pos,
                                                           float* __restrict__ out, size_t total) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(t & 255), y = (int)((t >> 8) & 255);
        const size_t pk = t >> 16;
        const int k = (int)(pk % n_pos);
        const size_t img = pk / n_pos;
        out[t] = (float)gray[(img * H + pos[2 * k] + y) * W + pos[2 * k + 1] + x];
    }
}

hipError_t launch_tile_patches(const uint8_t* gray, int n_img, int H, int W, const int32_t* pos_yx, int n_pos, float* out,
                               hipStream_t s) {
    const size_t total = (size_t)n_img * n_pos * 65536;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(tile_patches_kernel, dim3(grid_for(total)), dim3(256), 0, s, gray, H, W, pos_yx, n_pos, out, total);
    return hipGetLastError();
}

}  // namespace ecseg
