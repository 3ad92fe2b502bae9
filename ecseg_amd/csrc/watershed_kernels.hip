// The clean-up behind NuSeT's marker watershed on gfx950: clean_image (reference src/nuset_utils/normalization.py:25-37) and the final
// threshold of nuclei_segment (src/utils.py:159-162), one image, no host round trip.  Every step is a component labelling with
// per-component areas (union-find over pixel indices: uf_unite_back and uf_size_kernel of cell_util.h) followed by a per-pixel
// decision, so no result depends on the order of the atomics:
//   1. 4-connected components of mask != 0 -> the number of cells n and the pixel sum s; mean_area = float32(s) / n in float64 and
//      the size threshold t = mean_area / 5 (n = 0: NaN, every comparison below is false and nothing is removed);
//   2. remove_small_objects(connectivity=2): 8-connected components of the mask with area < t go;
//   3. remove_small_holes(connectivity=2): 8-connected components of the COMPLEMENT with area < t are filled, at the border too;
//   4. min-max scaling of the result: an image of one value divides 0 by 0 and comes out all zero, otherwise > 0 -> 255;
//   5. remove_small_objects(bool, NUCLEI_SIZE_T) with its default connectivity of 1: 4-connected components with area < T go
//      (T = 0 returns the image as it is).
// The marker watershed (src/model_layers/marker_watershed.py:82-91) from the host's ordered marker list: marker image and disk(3)
// maximum, binary_fill_holes (4-connected background components off the border), the exact squared Euclidean distance transform
// in int32 (column pass, then the row minimum), and scikit-image 0.18's flood with lines.  The flood's result IS the order of its
// binary heap - marker pixels of equal d^2 carry equal (value, age) keys and leave the heap as its sift rules decide - so it runs
// as one serial stream that replays that heap; everything around it is parallel.  A batch of images
// (run_marker_watershed_batch) gives every image such a stream of its own, side by side: the floods of different images share nothing.
#include "common.h"
#include "cell_util.h"

namespace ecseg {
namespace {

// par[p] = p where (img[p] != 0) == (want != 0), else -1
__device__ __forceinline__ void wk_init_px(const uint8_t* __restrict__ img, int px, int want, int32_t* __restrict__ par, int32_t* __restrict__ sz,
                                           unsigned p) {
    if (p >= (unsigned)px) return;                           // H * W < 2^31: no wrap
    par[p] = ((img[p] != 0) == (want != 0)) ? (int)p : -1;
    sz[p] = 0;
}
__global__ __launch_bounds__(256) void wk_init_kernel(const uint8_t* __restrict__ img, int px, int want, int32_t* __restrict__ par,
                                                      int32_t* __restrict__ sz) {
    wk_init_px(img, px, want, par, sz, blockIdx.x * 256u + threadIdx.x);
}

// unite every keyed pixel with its W / N (and, conn8, NW / NE) neighbour when that is keyed too
__device__ __forceinline__ void wk_unite_px(int H, int W, int conn8, int32_t* par, unsigned pu) {
    if (pu >= (unsigned)(H * W)) return;
    const int p = (int)pu;
    if (uf_load(par, p) < 0) return;
    const int y = p / W, x = p - y * W;
    uf_unite_back(par, p, y, x, W, conn8, [](int) { return true; });
}
__global__ __launch_bounds__(256) void wk_unite_kernel(int H, int W, int conn8, int32_t* par) {
    wk_unite_px(H, W, conn8, par, blockIdx.x * 256u + threadIdx.x);
}

// dbl[0] = mean_area = float32(pixels) / cells in float64 (normalization.py:30), dbl[1] = mean_area / 5 (:34,36)
__global__ void wk_mean_kernel(const int32_t* __restrict__ cnt, double* __restrict__ dbl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double mean = (double)(float)cnt[1] / (double)cnt[0];
    dbl[0] = mean;
    dbl[1] = mean / 5.0;
}

// fill = 0: out = in with the keyed (foreground) components of area < t cleared; fill = 1: the keyed components are background
// and those of area < t are set.  flags (may be null): |= 1 when out holds a 0, |= 2 when it holds a 1.
__global__ __launch_bounds__(256) void wk_small_kernel(const uint8_t* __restrict__ in, int px, int fill, const int32_t* __restrict__ par,
                                                       const int32_t* __restrict__ sz, const double* __restrict__ dbl,
                                                       uint8_t* __restrict__ out, int32_t* __restrict__ flags) {
    const unsigned pu = blockIdx.x * 256u + threadIdx.x;
    int v = -1;
    if (pu < (unsigned)px) {
        const int p = (int)pu, q = par[p];
        v = in[p] != 0 ? 1 : 0;
        if (q >= 0 && (double)sz[uf_find(par, q)] < dbl[1]) v = fill;     // NaN: false, nothing changes
        out[p] = (uint8_t)v;
    }
    if (flags) {
        const bool any0 = __ballot(v == 0) != 0ull, any1 = __ballot(v == 1) != 0ull;
        if ((threadIdx.x & 63) == 0 && (any0 || any1)) atomicOr(flags, (any0 ? 1 : 0) | (any1 ? 2 : 0));
    }
}

// out = 255 on the keyed components with at least `min_size` pixels when the cleaned image holds both values, else 0
__global__ __launch_bounds__(256) void wk_final_kernel(int px, int min_size, const int32_t* __restrict__ par, const int32_t* __restrict__ sz,
                                                       const int32_t* __restrict__ flags, uint8_t* __restrict__ out) {
    const unsigned pu = blockIdx.x * 256u + threadIdx.x;
    if (pu >= (unsigned)px) return;
    const int p = (int)pu, q = par[p];
    out[p] = (*flags == 3 && q >= 0 && sz[uf_find(par, q)] >= min_size) ? 255 : 0;
}


// ---- the marker watershed (src/model_layers/marker_watershed.py:82-91) ----------------------------------------------------------
constexpr int WS_INF = 1 << 30;

// Every stage below is stated once, as a function of the thread's pixel (marker, column) index over ONE image's buffers; the
// single-image kernels and the batched ones (blockIdx.y = the image, the pointers moved to its offset) are wrappers around it.

// idx[pixel] = 1 + the LAST list entry on that pixel (later markers overwrite earlier ones)
__device__ __forceinline__ void ws_scatter_px(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, int n, int W,
                                              int32_t* __restrict__ idx, unsigned i) {
    if (i >= (unsigned)n) return;
    atomicMax(idx + (size_t)rows[i] * W + cols[i], (int)i + 1);   // coordinates validated by the caller
}

// rw = morphology.dilation(markers, disk(3)) * mask: the maximum label over the 29 offsets with dy^2 + dx^2 <= 9
__device__ __forceinline__ void ws_dilate_px(const int32_t* __restrict__ idx, const int32_t* __restrict__ labels, const uint8_t* __restrict__ mask,
                                             int H, int W, int32_t* __restrict__ rw, unsigned pu) {
    if (pu >= (unsigned)(H * W)) return;
    const int p = (int)pu, y = p / W, x = p - y * W;
    int best = 0;
    if (mask[p]) {
        for (int dy = -3; dy <= 3; ++dy)
            for (int dx = -3; dx <= 3; ++dx) {
                if (dy * dy + dx * dx > 9 || y + dy < 0 || y + dy >= H || x + dx < 0 || x + dx >= W) continue;
                const int k = idx[p + dy * W + dx];
                if (k > 0) best = max(best, labels[k - 1]);
            }
    }
    rw[p] = best;
}

// after the 4-connected labelling of the background: sz[root] = 1 for every background component on the border
__device__ __forceinline__ void ws_border_px(int H, int W, const int32_t* __restrict__ par, int32_t* __restrict__ sz, unsigned pu) {
    if (pu >= (unsigned)(H * W)) return;
    const int p = (int)pu, y = p / W, x = p - y * W;
    if ((y == 0 || y == H - 1 || x == 0 || x == W - 1) && par[p] >= 0) sz[uf_find(par, p)] = 1;
}

// filled = binary_fill_holes(mask): the mask plus the background components that do not reach the border; *anyzero |= 1 when a 0 is
// left.  Whole waves call it (the ballot).
__device__ __forceinline__ void ws_filled_px(const uint8_t* __restrict__ mask, int px, const int32_t* __restrict__ par, const int32_t* __restrict__ sz,
                                             uint8_t* __restrict__ filled, int32_t* __restrict__ anyzero, unsigned pu) {
    int v = 1;
    if (pu < (unsigned)px) {
        const int p = (int)pu;
        v = (mask[p] || (par[p] >= 0 && sz[uf_find(par, p)] == 0)) ? 1 : 0;
        filled[p] = (uint8_t)v;
    }
    const bool z = __ballot(v == 0) != 0ull;
    if ((threadIdx.x & 63) == 0 && z) atomicOr(anyzero, 1);
}

// g[y][x] = distance along the column to the nearest zero of `filled`, WS_INF when the column holds none
__device__ __forceinline__ void ws_edt_col(const uint8_t* __restrict__ filled, int H, int W, int32_t* __restrict__ g, unsigned x) {
    if (x >= (unsigned)W) return;
    int d = WS_INF;
    for (int y = 0; y < H; ++y) {
        const size_t p = (size_t)y * W + x;
        d = filled[p] ? (d < WS_INF ? d + 1 : WS_INF) : 0;
        g[p] = d;
    }
    d = WS_INF;
    for (int y = H - 1; y >= 0; --y) {
        const size_t p = (size_t)y * W + x;
        d = filled[p] ? (d < WS_INF ? d + 1 : WS_INF) : 0;
        if (d < g[p]) g[p] = d;
    }
}

// d2 = the exact squared Euclidean distance to the nearest zero of `filled` on the mask's pixels (0 elsewhere): the minimum over
// the row of dx^2 + g^2, scanned outwards until dx^2 reaches the best.  No zero at all: scipy's answer, the distance to (-1, 0).
__device__ __forceinline__ void ws_edt_row_px(const uint8_t* __restrict__ mask, const int32_t* __restrict__ g, int H, int W,
                                              const int32_t* __restrict__ anyzero, int32_t* __restrict__ d2, unsigned pu) {
    if (pu >= (unsigned)(H * W)) return;
    const int p = (int)pu, y = p / W, x = p - y * W;
    if (!mask[p]) { d2[p] = 0; return; }
    if (!*anyzero) { d2[p] = (y + 1) * (y + 1) + x * x; return; }
    const int32_t* row = g + (size_t)y * W;
    int best = row[x] < WS_INF ? row[x] * row[x] : 0x7fffffff;
    for (int dx = 1; dx < W; ++dx) {
        if (dx * dx >= best) break;
        if (x - dx >= 0) { const int v = row[x - dx]; if (v < WS_INF) best = min(best, dx * dx + v * v); }
        if (x + dx < W) { const int v = row[x + dx]; if (v < WS_INF) best = min(best, dx * dx + v * v); }
    }
    d2[p] = best;
}

// out = pred_mask * (contour != 0)
__device__ __forceinline__ void ws_result_px(const uint8_t* __restrict__ mask, const int32_t* __restrict__ lab, int px, uint8_t* __restrict__ out,
                                             unsigned p) {
    if (p >= (unsigned)px) return;
    out[p] = lab[p] != 0 ? mask[p] : (uint8_t)0;
}

__global__ __launch_bounds__(256) void ws_scatter_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, int n, int W,
                                                         int32_t* __restrict__ idx) {
    ws_scatter_px(rows, cols, n, W, idx, blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(256) void ws_dilate_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ labels,
                                                        const uint8_t* __restrict__ mask, int H, int W, int32_t* __restrict__ rw) {
    ws_dilate_px(idx, labels, mask, H, W, rw, blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(256) void ws_border_kernel(int H, int W, const int32_t* __restrict__ par, int32_t* __restrict__ sz) {
    ws_border_px(H, W, par, sz, blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(256) void ws_filled_kernel(const uint8_t* __restrict__ mask, int px, const int32_t* __restrict__ par,
                                                        const int32_t* __restrict__ sz, uint8_t* __restrict__ filled, int32_t* __restrict__ anyzero) {
    ws_filled_px(mask, px, par, sz, filled, anyzero, blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(64) void ws_edt_cols_kernel(const uint8_t* __restrict__ filled, int H, int W, int32_t* __restrict__ g) {
    ws_edt_col(filled, H, W, g, blockIdx.x * 64u + threadIdx.x);
}
__global__ __launch_bounds__(256) void ws_edt_rows_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ g, int H, int W,
                                                          const int32_t* __restrict__ anyzero, int32_t* __restrict__ d2) {
    ws_edt_row_px(mask, g, H, W, anyzero, d2, blockIdx.x * 256u + threadIdx.x);
}
__global__ __launch_bounds__(256) void ws_result_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ lab, int px,
                                                        uint8_t* __restrict__ out) {
    ws_result_px(mask, lab, px, out, blockIdx.x * 256u + threadIdx.x);
}

// scikit-image 0.18's binary heap on (value, age) as ONE 64-bit key: push swims up while strictly smaller, pop moves the last
// element to the root and sinks it towards the smaller child, the left one on a tie.  Elements move through a hole instead of
// being swapped: the same comparisons, the same final arrangement.
struct WsHeap { unsigned long long* K; int2* P; int n; int cap; int overflow; };
__device__ __forceinline__ unsigned long long ws_key(int d2, int age) {
    return ((unsigned long long)(unsigned)(0x7fffffff - d2) << 32) | (unsigned)age;   // value = -d^2: the larger distance first
}
__device__ __forceinline__ void ws_push(WsHeap& h, unsigned long long key, int index, int source) {
    if (h.n >= h.cap) { h.overflow = 1; return; }
    int c = h.n++;
    while (c > 0) {
        const int p = (c + 1) / 2 - 1;
        const unsigned long long kp = h.K[p];
        if (!(key < kp)) break;
        h.K[c] = kp; h.P[c] = h.P[p];
        c = p;
    }
    h.K[c] = key; h.P[c] = make_int2(index, source);
}
__device__ __forceinline__ int2 ws_pop(WsHeap& h) {
    const int2 top = h.P[0];
    const int n = --h.n;
    if (n == 0) return top;
    const unsigned long long x = h.K[n];
    const int2 px = h.P[n];
    int i = 0;
    for (;;) {
        const int l = 2 * i + 1, r = l + 1;
        if (l >= n) break;
        int s = i;
        unsigned long long ks = x;
        const unsigned long long kl = h.K[l], kr = r < n ? h.K[r] : ~0ull;
        if (kl < ks) { s = l; ks = kl; }
        if (r < n && kr < ks) { s = r; ks = kr; }
        if (s == i) break;
        h.K[i] = ks; h.P[i] = h.P[s];
        i = s;
    }
    h.K[i] = x; h.P[i] = px;
    return top;
}

// The flood, one serial stream (lane 0 of one wave; the other lanes only help to find the marker pixels): the order of the heap is
// the result.  m: working copy of the mask (line pixels leave it); lab: labels, zeroed by the caller; misc[1] = 1 on a heap overflow.
__device__ __forceinline__ void ws_flood(uint8_t* m, const int32_t* __restrict__ rw, const int32_t* __restrict__ d2, int H, int W,
                                         unsigned long long* K, int2* P, int cap, int32_t* lab, int32_t* misc) {
    const int lane = threadIdx.x, px = H * W;
    WsHeap h{K, P, 0, cap, 0};
    for (int base = 0; base < px; base += 64) {              // markers in raster order, age 0
        const int p = base + lane;
        unsigned long long bits = __ballot(p < px && rw[p] != 0);
        if (lane == 0)
            while (bits) {
                const int q = base + __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                lab[q] = rw[q];
                ws_push(h, ws_key(d2[q], 0), q, q);
            }
    }
    if (lane != 0) return;
    int age = 0;
    while (h.n > 0) {
        const int2 e = ws_pop(h);
        const int i = e.x, y = i / W, x = i - y * W;
        if (i != e.y && lab[i] != 0) continue;               // in the heap more than once
        const int q[4] = {i - W, i - 1, i + 1, i + W};       // raveled neighbour order
        const bool in[4] = {y > 0, x > 0, x + 1 < W, y + 1 < H};
        int l[4];
        bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok[k] = in[k] && m[in[k] ? q[k] : i] != 0;
            l[k] = ok[k] ? lab[q[k]] : 0;
        }
        int first = 0;
        bool line = false;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (l[k]) { if (!first) first = l[k]; else if (l[k] != first) line = true; }
        if (line) { m[i] = 0; continue; }                    // a line pixel leaves the mask; a marker pixel keeps its label
        lab[i] = lab[e.y];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ok[k] && l[k] == 0) ws_push(h, ws_key(d2[q[k]], ++age), q[k], e.y);
    }
    if (h.overflow) misc[1] = 1;
}

__global__ __launch_bounds__(64) void ws_flood_kernel(uint8_t* m, const int32_t* __restrict__ rw, const int32_t* __restrict__ d2, int H, int W,
                                                      unsigned long long* K, int2* P, int cap, int32_t* lab, int32_t* misc) {
    ws_flood(m, rw, d2, H, W, K, P, cap, lab, misc);
}

// ---- the batch: blockIdx.y (the flood: blockIdx.x) is the image, every pointer moves to the image's own offset -------------------
// A block past its image's pixels (markers, columns) returns at once; the union-find parents are indices INSIDE the image.
#define WSB_IMAGE(count)                                                   \
    const WsImage im = b.tab[blockIdx.y];                                  \
    const int px = im.H * im.W;                                            \
    if (blockIdx.x * blockDim.x >= (unsigned)(count)) return;              \
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;              \
    (void)px
__global__ __launch_bounds__(256) void wsb_scatter_kernel(WatershedBatchBufs b) {
    WSB_IMAGE(im.n_markers);
    ws_scatter_px(b.rows + im.first_marker, b.cols + im.first_marker, im.n_markers, im.W, b.idx + im.off, t);
}
__global__ __launch_bounds__(256) void wsb_dilate_kernel(WatershedBatchBufs b) {
    WSB_IMAGE(px);
    ws_dilate_px(b.idx + im.off, b.labels + im.first_marker, b.mask + im.off, im.H, im.W, b.rw + im.off, t);
}
__global__ __launch_bounds__(256) void wsb_init_kernel(WatershedBatchBufs b) {                // the background, 4-connected
    WSB_IMAGE(px);
    wk_init_px(b.mask + im.off, px, 0, b.par + im.off, b.sz + im.off, t);
}
__global__ __launch_bounds__(256) void wsb_unite_kernel(WatershedBatchBufs b) {
    WSB_IMAGE(px);
    wk_unite_px(im.H, im.W, 0, b.par + im.off, t);
}
__global__ __launch_bounds__(256) void wsb_border_kernel(WatershedBatchBufs b) {
    WSB_IMAGE(px);
    ws_border_px(im.H, im.W, b.par + im.off, b.sz + im.off, t);
}
__global__ __launch_bounds__(256) void wsb_filled_kernel(WatershedBatchBufs b) {
    WSB_IMAGE(px);
    ws_filled_px(b.mask + im.off, px, b.par + im.off, b.sz + im.off, b.filled + im.off, b.misc + 4 * blockIdx.y, t);
}
__global__ __launch_bounds__(64) void wsb_edt_cols_kernel(WatershedBatchBufs b) {
    WSB_IMAGE(im.W);
    ws_edt_col(b.filled + im.off, im.H, im.W, b.g + im.off, t);
}
__global__ __launch_bounds__(256) void wsb_edt_rows_kernel(WatershedBatchBufs b) {
    WSB_IMAGE(px);
    ws_edt_row_px(b.mask + im.off, b.g + im.off, im.H, im.W, b.misc + 4 * blockIdx.y, b.d2 + im.off, t);
}
__global__ __launch_bounds__(64) void wsb_flood_kernel(WatershedBatchBufs b) {               // one wave per image
    const WsImage im = b.tab[blockIdx.x];
    ws_flood(b.work + im.off, b.rw + im.off, b.d2 + im.off, im.H, im.W, b.heap_k + im.heap_off, b.heap_p + im.heap_off, im.heap_cap,
             b.lab + im.off, b.misc + 4 * blockIdx.x);
}
__global__ __launch_bounds__(256) void wsb_result_kernel(WatershedBatchBufs b) {
    WSB_IMAGE(px);
    ws_result_px(b.mask + im.off, b.lab + im.off, px, b.out + im.off, t);
}
#undef WSB_IMAGE

}  // namespace

hipError_t run_marker_watershed(const uint8_t* mask, int H, int W, const int32_t* rows, const int32_t* cols, const int32_t* labels, int n,
                                int heap_cap, const WatershedBufs& b, hipStream_t s) {
    const int px = H * W;
    const dim3 g(((unsigned)px + 255u) / 256u), t(256);
    hipError_t e;
    if ((e = hipMemsetAsync(b.misc, 0, 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.idx, 0, (size_t)px * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.lab, 0, (size_t)px * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(b.work, mask, (size_t)px, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    if (n > 0) hipLaunchKernelGGL(ws_scatter_kernel, dim3(((unsigned)n + 255u) / 256u), t, 0, s, rows, cols, n, W, b.idx);
    hipLaunchKernelGGL(ws_dilate_kernel, g, t, 0, s, b.idx, labels, mask, H, W, b.rw);
    hipLaunchKernelGGL(wk_init_kernel, g, t, 0, s, mask, px, 0, b.par, b.sz);          // the background, 4-connected
    hipLaunchKernelGGL(wk_unite_kernel, g, t, 0, s, H, W, 0, b.par);
    hipLaunchKernelGGL(ws_border_kernel, g, t, 0, s, H, W, b.par, b.sz);
    hipLaunchKernelGGL(ws_filled_kernel, g, t, 0, s, mask, px, b.par, b.sz, b.filled, b.misc);
    hipLaunchKernelGGL(ws_edt_cols_kernel, dim3(((unsigned)W + 63u) / 64u), dim3(64), 0, s, b.filled, H, W, b.g);
    hipLaunchKernelGGL(ws_edt_rows_kernel, g, t, 0, s, mask, b.g, H, W, b.misc, b.d2);
    hipLaunchKernelGGL(ws_flood_kernel, dim3(1), dim3(64), 0, s, b.work, b.rw, b.d2, H, W, b.heap_k, b.heap_p, heap_cap, b.lab, b.misc);
    hipLaunchKernelGGL(ws_result_kernel, g, t, 0, s, mask, b.lab, px, b.out);
    return hipGetLastError();
}

hipError_t run_marker_watershed_batch(int n_images, size_t span, int max_px, int max_w, int max_markers, const WatershedBatchBufs& b,
                                      hipStream_t s) {
    const unsigned N = (unsigned)n_images;
    const dim3 g(((unsigned)max_px + 255u) / 256u, N), t(256);
    hipError_t e;
    if ((e = hipMemsetAsync(b.misc, 0, (size_t)N * 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.idx, 0, span * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.lab, 0, span * sizeof(int32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(b.out, 0, span, s)) != hipSuccess) return e;         // the bytes between the images stay 0
    if ((e = hipMemcpyAsync(b.work, b.mask, span, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    if (max_markers > 0) hipLaunchKernelGGL(wsb_scatter_kernel, dim3(((unsigned)max_markers + 255u) / 256u, N), t, 0, s, b);
    hipLaunchKernelGGL(wsb_dilate_kernel, g, t, 0, s, b);
    hipLaunchKernelGGL(wsb_init_kernel, g, t, 0, s, b);
    hipLaunchKernelGGL(wsb_unite_kernel, g, t, 0, s, b);
    hipLaunchKernelGGL(wsb_border_kernel, g, t, 0, s, b);
    hipLaunchKernelGGL(wsb_filled_kernel, g, t, 0, s, b);
    hipLaunchKernelGGL(wsb_edt_cols_kernel, dim3(((unsigned)max_w + 63u) / 64u, N), dim3(64), 0, s, b);
    hipLaunchKernelGGL(wsb_edt_rows_kernel, g, t, 0, s, b);
    hipLaunchKernelGGL(wsb_flood_kernel, dim3(N), dim3(64), 0, s, b);
    hipLaunchKernelGGL(wsb_result_kernel, g, t, 0, s, b);
    return hipGetLastError();
}

hipError_t run_clean_nuclei(const uint8_t* mask, int H, int W, int nuclei_size_t, const CleanBufs& b, hipStream_t s) {
    const int px = H * W;
    const dim3 g(((unsigned)px + 255u) / 256u), t(256);
    hipError_t e;
    if ((e = hipMemsetAsync(b.misc, 0, 4 * sizeof(int32_t), s)) != hipSuccess) return e;
    auto label = [&](const uint8_t* img, int want, int conn8, int32_t* cnt) {
        hipLaunchKernelGGL(wk_init_kernel, g, t, 0, s, img, px, want, b.par, b.sz);
        hipLaunchKernelGGL(wk_unite_kernel, g, t, 0, s, H, W, conn8, b.par);
        hipLaunchKernelGGL(uf_size_kernel, g, t, 0, s, px, b.par, b.sz, cnt);
    };
    label(mask, 1, 0, b.misc);                               // misc[0] cells, misc[1] pixels
    hipLaunchKernelGGL(wk_mean_kernel, dim3(1), dim3(64), 0, s, b.misc, b.dbl);
    label(mask, 1, 1, nullptr);
    hipLaunchKernelGGL(wk_small_kernel, g, t, 0, s, mask, px, 0, b.par, b.sz, b.dbl, b.tmp, static_cast<int32_t*>(nullptr));
    label(b.tmp, 0, 1, nullptr);
    hipLaunchKernelGGL(wk_small_kernel, g, t, 0, s, b.tmp, px, 1, b.par, b.sz, b.dbl, b.cleaned, b.misc + 2);
    label(b.cleaned, 1, 0, nullptr);
    hipLaunchKernelGGL(wk_final_kernel, g, t, 0, s, px, nuclei_size_t, b.par, b.sz, b.misc + 2, b.out);
    return hipGetLastError();
}

}  // namespace ecseg
