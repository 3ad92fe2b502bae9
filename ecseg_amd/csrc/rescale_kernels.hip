// The two rescale calls of NuSeT's nuclei_segment on gfx950 (reference src/utils.py:136 and :157-162) as scikit-image 0.18.3 /
// scipy 1.7.1 compute them, one image, bit for bit in float64 (this file is compiled with -ffp-contract=off: a * b + c rounds
// twice, and every sum below is written in the order of the libraries' loops).
//
// Down, rescale(image_u8, s, anti_aliasing=True):
//   * rs_gauss_y_kernel, then rs_gauss_x_kernel: scipy.ndimage.gaussian_filter on the uint8 array, axis 0 first, each pass
//     writing uint8 by truncation.  One output per thread in scipy's symmetric-kernel order, tmp = in[i] * w[0], then for
//     j = -r .. -1: tmp += (in[i + j] + in[i - j]) * w[j]; indices mirrored without repeating the edge (mode 'mirror'; r < n, so
//     one reflection suffices).  The y pass reads rows of lanes (lane = column, every tap one coalesced row segment); the x pass
//     stages its row segment with the halo in LDS.  The weights come from the host (2 r + 1 float64) and sit in LDS.
//   * rs_bilinear_kernel: the order-1 warp, mode 'reflect', on the exact map y = f * (r + 0.5) - 0.5 of filtered / 255.
// Up, rescale(cleaned_u8, 1 / s) and the threshold behind it:
//   * rs_bilinear_kernel again (no filter: f < 1), with the minimum and maximum of the output: the values are >= +0, so their bit
//     patterns order as unsigned integers and atomicMax (on the complement for the minimum, so that one memset presets both)
//     gives a result that does not depend on the order;
//   * rs_threshold_kernel: uint8(((v - vmin) / (vmax - vmin)) * 255) > 0, i.e. that float64 >= 1 (0 / 0 = NaN: false, an image of
//     one value comes out all zero), presets the union-find parents;
//   * rs_unite_kernel (uf_unite_back, 4-connected), uf_size_kernel (cell_util.h) and rs_final_kernel: remove_small_objects.
#include "common.h"
#include "cell_util.h"

namespace ecseg {
namespace {

constexpr int RS_R = ECSEG_RESCALE_MAX_RADIUS;

// mirror without repeating the edge sample (-1 -> 1, n -> n - 2); the clamp keeps a caller's mistake inside the array
__device__ __forceinline__ int rs_mirror(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return min(max(i, 0), n - 1);
}

// axis 0: out[y][x] from in[y + j][x]
__global__ __launch_bounds__(256) void rs_gauss_y_kernel(const uint8_t* __restrict__ in, int H, int W, const double* __restrict__ w, int r,
                                                         uint8_t* __restrict__ out) {
    __shared__ double s_w[RS_R + 1];
    for (int i = threadIdx.x; i <= r; i += 256) s_w[i] = w[i];           // w[0 .. r - 1]: j = -r .. -1, w[r]: the centre
    __syncthreads();
    const unsigned tiles_x = ((unsigned)W + 63u) / 64u;                  // 1-D grid: tiles_x * ceil(H / 4) < 2^31
    const unsigned x = (blockIdx.x % tiles_x) * 64u + (threadIdx.x & 63u);
    const int y = (int)(blockIdx.x / tiles_x) * 4 + (int)(threadIdx.x >> 6);
    if (x >= (unsigned)W || y >= H) return;
    const uint8_t* col = in + x;
    double tmp = (double)col[(size_t)y * W] * s_w[r];
    for (int j = -r; j < 0; ++j) {
        const int a = col[(size_t)rs_mirror(y + j, H) * W], b = col[(size_t)rs_mirror(y - j, H) * W];
        tmp += (double)(a + b) * s_w[r + j];                             // the pair sum is exact
    }
    out[(size_t)y * W + x] = (uint8_t)tmp;                               // 0 <= tmp < 256: truncation
}

// axis 1: out[y][x] from in[y][x + j]; 256 consecutive columns of one row per workgroup
__global__ __launch_bounds__(256) void rs_gauss_x_kernel(const uint8_t* __restrict__ in, int H, int W, const double* __restrict__ w, int r,
                                                         uint8_t* __restrict__ out) {
    __shared__ double s_w[RS_R + 1];
    __shared__ uint8_t s_in[256 + 2 * RS_R];
    const unsigned tiles_x = ((unsigned)W + 255u) / 256u;                // 1-D grid: tiles_x * H < 2^31
    const int t = threadIdx.x, x0 = (int)(blockIdx.x % tiles_x) * 256, y = (int)(blockIdx.x / tiles_x);
    const uint8_t* row = in + (size_t)y * W;
    for (int i = t; i <= r; i += 256) s_w[i] = w[i];
    for (int i = t; i < 256 + 2 * r; i += 256) s_in[i] = row[rs_mirror(x0 - r + i, W)];
    __syncthreads();
    const int x = x0 + t;
    if (x >= W) return;
    const uint8_t* c = s_in + t + r;
    double tmp = (double)c[0] * s_w[r];
    for (int j = -r; j < 0; ++j) tmp += (double)((int)c[j] + (int)c[-j]) * s_w[r + j];
    out[(size_t)y * W + x] = (uint8_t)tmp;
}

// skimage's bilinear_interpolation at output pixel (r, c) of src / 255
__device__ __forceinline__ double rs_bilinear(const uint8_t* __restrict__ src, int H, int W, double fy, double fx, int r, int c) {
    const double y = fy * ((double)r + 0.5) - 0.5, x = fx * ((double)c + 0.5) - 0.5;
    const double y0f = floor(y), x0f = floor(x);
    const double dy = y - y0f, dx = x - x0f;
    const size_t r0 = (size_t)rs_mirror((int)y0f, H) * W, r1 = (size_t)rs_mirror((int)ceil(y), H) * W;
    const int c0 = rs_mirror((int)x0f, W), c1 = rs_mirror((int)ceil(x), W);
    const double p00 = (double)src[r0 + c0] / 255.0, p01 = (double)src[r0 + c1] / 255.0;
    const double p10 = (double)src[r1 + c0] / 255.0, p11 = (double)src[r1 + c1] / 255.0;
    const double top = (1.0 - dx) * p00 + dx * p01;
    const double bottom = (1.0 - dx) * p10 + dx * p11;
    return (1.0 - dy) * top + dy * bottom;
}

// out (oh, ow) float64; mm (may be null): [0] = ~min, [1] = max of the output as bit patterns (preset to 0)
__global__ __launch_bounds__(256) void rs_bilinear_kernel(const uint8_t* __restrict__ src, int H, int W, int oh, int ow, double fy, double fx,
                                                          double* __restrict__ out, u64* __restrict__ mm) {
    const unsigned pu = blockIdx.x * 256u + threadIdx.x;                 // oh * ow < 2^31: no wrap
    const bool in = pu < (unsigned)(oh * ow);
    double v = 0.0;
    if (in) {
        const int p = (int)pu, r = p / ow, c = p - r * ow;
        v = rs_bilinear(src, H, W, fy, fx, r, c);
        out[p] = v;
    }
    if (!mm) return;
    double lo = in ? v : __longlong_as_double(0x7ff0000000000000ll), hi = v;     // v >= +0 everywhere
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, d));
        hi = fmax(hi, __shfl_xor(hi, d));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(mm + 0, ~(u64)__double_as_longlong(lo));
        atomicMax(mm + 1, (u64)__double_as_longlong(hi));
    }
}

// par[p] = p where uint8(((v - vmin) / (vmax - vmin)) * 255) > 0, else -1
__global__ __launch_bounds__(256) void rs_threshold_kernel(const double* __restrict__ v, int px, const u64* __restrict__ mm,
                                                           int32_t* __restrict__ par, int32_t* __restrict__ sz) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)px) return;
    const double vmin = __longlong_as_double((long long)~mm[0]), vmax = __longlong_as_double((long long)mm[1]);
    const double t = ((v[p] - vmin) / (vmax - vmin)) * 255.0;
    par[p] = t >= 1.0 ? (int)p : -1;                                     // NaN: false
    sz[p] = 0;
}

__global__ __launch_bounds__(256) void rs_unite_kernel(int H, int W, int32_t* par) {
    const unsigned pu = blockIdx.x * 256u + threadIdx.x;
    if (pu >= (unsigned)(H * W)) return;
    const int p = (int)pu;
    if (uf_load(par, p) < 0) return;
    const int y = p / W, x = p - y * W;
    uf_unite_back(par, p, y, x, W, 0, [](int) { return true; });
}

// out = 255 on the components of at least `min_size` pixels
__global__ __launch_bounds__(256) void rs_final_kernel(int px, int min_size, const int32_t* __restrict__ par, const int32_t* __restrict__ sz,
                                                       uint8_t* __restrict__ out) {
    const unsigned pu = blockIdx.x * 256u + threadIdx.x;
    if (pu >= (unsigned)px) return;
    const int q = par[(int)pu];
    out[pu] = (q >= 0 && sz[uf_find(par, q)] >= min_size) ? 255 : 0;
}

}  // namespace

hipError_t run_rescale_down(const uint8_t* img, int H, int W, int oh, int ow, const double* wy, int ry, const double* wx, int rx,
                            uint8_t* tmp, uint8_t* filtered, double* out, hipStream_t s) {
    const uint8_t* src = img;
    hipError_t e;
    if (ry > 0) {
        hipLaunchKernelGGL(rs_gauss_y_kernel, dim3((((unsigned)W + 63u) / 64u) * (((unsigned)H + 3u) / 4u)), dim3(256), 0, s, src, H, W, wy, ry, tmp);
        src = tmp;
    }
    if (rx > 0) {
        hipLaunchKernelGGL(rs_gauss_x_kernel, dim3((((unsigned)W + 255u) / 256u) * (unsigned)H), dim3(256), 0, s, src, H, W, wx, rx, filtered);
    } else if ((e = hipMemcpyAsync(filtered, src, (size_t)H * W, hipMemcpyDeviceToDevice, s)) != hipSuccess) {
        return e;
    }
    const unsigned opx = (unsigned)oh * (unsigned)ow;
    hipLaunchKernelGGL(rs_bilinear_kernel, dim3((opx + 255u) / 256u), dim3(256), 0, s, filtered, H, W, oh, ow, (double)H / (double)oh,
                       (double)W / (double)ow, out, static_cast<u64*>(nullptr));
    return hipGetLastError();
}

hipError_t run_rescale_mask_up(const uint8_t* cleaned, int H, int W, int oh, int ow, int nuclei_size_t, const RescaleUpBufs& b, hipStream_t s) {
    const int opx = oh * ow;
    const dim3 g(((unsigned)opx + 255u) / 256u), t(256);
    hipError_t e;
    if ((e = hipMemsetAsync(b.mm, 0, 2 * sizeof(u64), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(rs_bilinear_kernel, g, t, 0, s, cleaned, H, W, oh, ow, (double)H / (double)oh, (double)W / (double)ow, b.v, b.mm);
    hipLaunchKernelGGL(rs_threshold_kernel, g, t, 0, s, b.v, opx, b.mm, b.par, b.sz);
    hipLaunchKernelGGL(rs_unite_kernel, g, t, 0, s, oh, ow, b.par);
    hipLaunchKernelGGL(uf_size_kernel, g, t, 0, s, opx, b.par, b.sz, static_cast<int32_t*>(nullptr));
    hipLaunchKernelGGL(rs_final_kernel, g, t, 0, s, opx, nuclei_size_t, b.par, b.sz, b.out);
    return hipGetLastError();
}

}  // namespace ecseg
