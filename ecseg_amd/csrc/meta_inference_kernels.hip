// The meta_inference clean-up schedule for gfx950 (run_meta_inference): labelling passes of the engine behind ccl.h and, after
// each, the kernels below that apply the reference's rule to what the pass left - fill, threshold / band, nucleus test (pair and
// binned), kill, merge / open.  HBM/latency-bound integer work on uint8 label images (n_img, H, W); no MFMA.
#include <algorithm>

#include "ccl.h"

namespace ecseg {

// ---- per-pixel "apply" kernels of the schedule (one thread per pixel, grid-stride over the batch) --------------------------
// fill_holes (src/image_tools.py:36-39): pixels != c whose 4-connected background component does not reach the border
__global__ __launch_bounds__(256) void apply_fill_kernel(uint8_t* __restrict__ img, const int32_t* __restrict__ L,
                                                         const uint32_t* __restrict__ flag, int n_img, size_t px, int c, uint32_t lut) {
    IMG_PX_LOOP(n_img, px) {
        if (!key_of(img[t], lut)) continue;                    // not part of the labelled background: its parent is stale
        const int r = L[ib + L[t]];                            // pixel -> owner (tile root) -> global root
        if (!(flag[ib + r] & 1u)) img[t] = (uint8_t)c;
    }
}

// The same per labelling tile (fill passes run with full-tile nodes): a full tile asks once - its root's component either
// reaches the image border (nothing to do) or the whole tile lies inside a hole; a tile without a keyed pixel has nothing to
// fill; the others go pixel by pixel.
__global__ __launch_bounds__(256) void apply_fill_tile_kernel(CclGeom g, uint8_t* __restrict__ img_all, const int32_t* __restrict__ L_all,
                                                              const uint32_t* __restrict__ flag_all, int c, uint32_t lut,
                                                              const uint8_t* __restrict__ tile_any, const uint32_t* __restrict__ own_bits) {
    int img, y0, cx;
    if (!decode_block(g, img, y0, cx)) return;
    const size_t ti = tile_index(g, img);
    const int ta = tile_any[ti];
    if (!ta) return;
    const size_t base = (size_t)img * g.H * g.W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = cx * 64 + lane;
    if (ta == 1) {
        // Holes are rare: when every component of the tile (its owners, from the owner bits; their parents are the global roots
        // since ccl_resolve) reaches the image border there is nothing to fill here - decided from a handful of look-ups
        // instead of two gathers per pixel (round 4).
        const int yblk = y0 - wave * CCL_ROWS;
        uint32_t bits = thread_owner_bits(ta, own_bits, ti, threadIdx.x);
        int open_all = 1;
        while (bits) {
            const int p = pop_owner(bits, g, threadIdx.x, yblk, cx);
            if (!(flag_all[base + L_all[base + p]] & 1u)) open_all = 0;
        }
        if (__syncthreads_and(open_all)) return;
    }
    bool fill_all = false;
    if (ta == 2) {
        const int p0 = (y0 - wave * CCL_ROWS) * g.W + cx * 64;
        const int r = L_all[base + L_all[base + p0]];          // (the tile's first pixel is its own owner: -> global root)
        if (flag_all[base + r] & 1u) return;                   // background connected to the image border
        fill_all = true;
    }
#pragma unroll
    for (int r = 0; r < CCL_ROWS; ++r) {
        const int y = y0 + r;
        if (y >= g.H || x >= g.W) continue;
        const size_t t = base + (size_t)y * g.W + x;
        if (fill_all) { img_all[t] = (uint8_t)c; continue; }
        if (!key_of(img_all[t], lut)) continue;
        const int root = L_all[base + L_all[t]];
        if (!(flag_all[base + root] & 1u)) img_all[t] = (uint8_t)c;
    }
}

// The class-2 root indices that ccl_flatten appended (first word of every 16-byte slot) become regionprops centroids
// (mean of the pixel coordinates, float64) in place.
__global__ __launch_bounds__(256) void centroids_kernel(const uint32_t* __restrict__ area, const u64* __restrict__ sumy,
                                                        const u64* __restrict__ sumx, const int32_t* __restrict__ G_all,
                                                        double2* __restrict__ list2, size_t px, size_t cap) {
    const int im = blockIdx.y;
    const int n2 = G_all[(size_t)im * G_IMG + G_NLIST2];
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n2; k += gridDim.x * blockDim.x) {
        double2* slot = list2 + (size_t)im * cap + k;
        const int root = *reinterpret_cast<const int32_t*>(slot);
        const size_t t = (size_t)im * px + root;
        const double a = (double)area[t];
        *slot = make_double2((double)sumy[t] / a, (double)sumx[t] / a);
    }
}

// which of the two nucleus-test kernels takes an image (see bin_centroids_kernel below)
__device__ __forceinline__ bool nucleus_binned_ok(int n2, int H, int W, size_t binned_cap) {
    return H <= NUCLEUS_BIN_EXTENT && W <= NUCLEUS_BIN_EXTENT && (size_t)n2 <= binned_cap;
}

// Nucleus-in-metaphase test (src/image_tools.py:72-81): more than five chromosome centroids strictly inside each of
// the four 70-px half bands -> the nucleus is erased.  One wavefront per nucleus (grid-stride), lanes stride over the
// chromosome list; the scan stops as soon as all four counts exceed the threshold.
__global__ __launch_bounds__(256) void nucleus_test_kernel(const uint32_t* __restrict__ area, const u64* __restrict__ sumy,
                                                           const u64* __restrict__ sumx, const int32_t* __restrict__ G_all,
                                                           const int32_t* __restrict__ list1, const double2* __restrict__ list2,
                                                           uint32_t* __restrict__ flag, size_t px, size_t cap,
                                                           int blocks_per_img, double v, int min_count, int H, int W,
                                                           size_t binned_cap) {
    const int im = blockIdx.x / blocks_per_img, j = blockIdx.x % blocks_per_img;
    const int32_t* G = G_all + (size_t)im * G_IMG;
    const int n1 = G[G_NLIST1], n2 = G[G_NLIST2];
    if (nucleus_binned_ok(n2, H, W, binned_cap)) return;            // handled by nucleus_test_binned_kernel
    const int lane = threadIdx.x & 63;
    const int wave = j * 4 + (threadIdx.x >> 6), nwaves = blocks_per_img * 4;
    for (int k = wave; k < n1; k += nwaves) {                       // wave-uniform loop
        const int root = list1[(size_t)im * cap + k];
        const size_t slot = (size_t)im * px + root;
        const double a = (double)area[slot];
        const double ny = (double)sumy[slot] / a, nx = (double)sumx[slot] / a;
        int cl = 0, cr = 0, cb = 0, ct = 0;
        for (int c0 = 0; c0 < n2; c0 += 64) {
            const int c = c0 + lane;
            bool l = false, r = false, b = false, tp = false;
            if (c < n2) {
                const double2 cc = list2[(size_t)im * cap + c];   // (cy, cx)
                l = (cc.y > nx) && (cc.y < nx + v);
                r = (cc.y < nx) && (cc.y > nx - v);
                b = (cc.x < ny) && (cc.x > ny - v);
                tp = (cc.x > ny) && (cc.x < ny + v);
            }
            cl += __popcll(__ballot(l)); cr += __popcll(__ballot(r));
            cb += __popcll(__ballot(b)); ct += __popcll(__ballot(tp));
            if (cl > min_count && cr > min_count && cb > min_count && ct > min_count) break;
        }
        if (lane == 0 && cl > min_count && cr > min_count && cb > min_count && ct > min_count) flag[slot] |= 2u;
    }
}

// The four band tests only look at ONE coordinate each (left / right: the centroid's x, bottom / top: its y), so a count is
// "how many coordinates lie in an open interval".  bin_centroids_kernel groups the coordinates of an image by integer bin
// (counting sort: LDS histogram, scan, scatter; one workgroup per image and axis); a query then takes whole bins from the
// prefix array and compares only the entries of the two end bins: O(n1 + n2) per image for any reasonable spread instead of
// the n1 * n2 pair tests of nucleus_test_kernel (the speckled output of a random-weight base-16 model - 10^4..10^5 nuclei and
// chromosomes per image - spent 0.37 ms per image there).  The comparisons are the reference's own (strict, on the same
// doubles).  Images wider / taller than NUCLEUS_BIN_EXTENT or with more chromosomes than `binned` holds go to the pair test.
// `converted` == 0: the list still holds the roots (first word of every slot, as ccl_resolve left them) and the centroid is
// computed here from the root's area / coordinate sums - the same float64 quotients centroids_kernel would have stored.
__device__ __forceinline__ double list_centroid(const double2* __restrict__ src, int i, int axis, int converted,
                                                const uint32_t* __restrict__ area, const u64* __restrict__ sumy,
                                                const u64* __restrict__ sumx, size_t ib) {
    if (converted) return axis ? src[i].y : src[i].x;
    const size_t t = ib + (size_t)*reinterpret_cast<const int32_t*>(src + i);
    return (double)(axis ? sumx[t] : sumy[t]) / (double)area[t];
}

__global__ __launch_bounds__(1024) void bin_centroids_kernel(const int32_t* __restrict__ G_all, const double2* __restrict__ list2,
                                                             double* __restrict__ binned, int32_t* __restrict__ binstart,
                                                             size_t cap, size_t binned_cap, int H, int W,
                                                             const uint32_t* __restrict__ area, const u64* __restrict__ sumy,
                                                             const u64* __restrict__ sumx, size_t px, int converted) {
    extern __shared__ __attribute__((aligned(16))) char dyn_smem[];
    int* hist = reinterpret_cast<int*>(dyn_smem);                        // [E + 1]: counts, then bin starts, then cursors
    __shared__ int part[1024];
    const int im = blockIdx.y, axis = blockIdx.x;                       // axis 0: y (double2.x), 1: x (double2.y)
    const int n2 = G_all[(size_t)im * G_IMG + G_NLIST2];
    if (n2 <= 0 || !nucleus_binned_ok(n2, H, W, binned_cap)) return;
    const int E = axis ? W : H;
    const int tid = threadIdx.x;
    for (int i = tid; i <= E; i += 1024) hist[i] = 0;
    __syncthreads();
    const double2* src = list2 + (size_t)im * cap;
    const size_t ib = (size_t)im * px;
    for (int i = tid; i < n2; i += 1024) {
        const double c = list_centroid(src, i, axis, converted, area, sumy, sumx, ib);
        int b = (int)c;                                                  // centroids are means of pixel coordinates: 0 <= c <= E - 1
        b = b < 0 ? 0 : (b > E - 1 ? E - 1 : b);
        atomicAdd(&hist[b], 1);
    }
    __syncthreads();
    // exclusive scan of hist[0..E]: serial chunks per thread + a scan of the 1024 chunk sums
    const int chunk = (E + 1 + 1023) / 1024;
    const int lo = tid * chunk, hi = min(lo + chunk, E + 1);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += hist[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;                                           // exclusive prefix of this thread's chunk
    int32_t* st = binstart + ((size_t)im * 2 + axis) * (NUCLEUS_BIN_EXTENT + 2);
    for (int i = lo; i < hi; ++i) { const int c = hist[i]; hist[i] = run; st[i] = run; run += c; }
    __syncthreads();
    double* out = binned + ((size_t)im * 2 + axis) * binned_cap;
    for (int i = tid; i < n2; i += 1024) {
        const double c = list_centroid(src, i, axis, converted, area, sumy, sumx, ib);
        int b = (int)c;
        b = b < 0 ? 0 : (b > E - 1 ? E - 1 : b);
        out[atomicAdd(&hist[b], 1)] = c;
    }
}

// #{c in the binned coordinates : lo < c < hi}
__device__ __forceinline__ int count_open_interval(const double* __restrict__ c, const int32_t* __restrict__ st, int E, double lo,
                                                   double hi) {
    if (!(lo < hi)) return 0;
    // floor() as integers, clamped to [-1, E]: bins strictly between the two end bins lie wholly inside the interval
    const double fl_d = floor(lo), fh_d = floor(hi);
    const int fl = fl_d < -1.0 ? -1 : (fl_d > (double)E ? E : (int)fl_d);
    const int fh = fh_d < -1.0 ? -1 : (fh_d > (double)E ? E : (int)fh_d);
    int n = 0;
    if (fh > fl + 1) n = st[fh > E ? E : fh] - st[fl + 1];
    if (fl >= 0 && fl < E)
        for (int i = st[fl]; i < st[fl + 1]; ++i) n += (c[i] > lo && c[i] < hi) ? 1 : 0;
    if (fh != fl && fh >= 0 && fh < E)
        for (int i = st[fh]; i < st[fh + 1]; ++i) n += (c[i] > lo && c[i] < hi) ? 1 : 0;
    return n;
}

// thread = nucleus: the four counts of nucleus_test_kernel from the binned coordinates
__global__ __launch_bounds__(256) void nucleus_test_binned_kernel(const uint32_t* __restrict__ area, const u64* __restrict__ sumy,
                                                                  const u64* __restrict__ sumx, const int32_t* __restrict__ G_all,
                                                                  const int32_t* __restrict__ list1, const double* __restrict__ binned,
                                                                  const int32_t* __restrict__ binstart, uint32_t* __restrict__ flag,
                                                                  size_t px, size_t cap, size_t binned_cap, int H, int W, double v,
                                                                  int min_count) {
    const int im = blockIdx.y;
    const int32_t* G = G_all + (size_t)im * G_IMG;
    const int n1 = G[G_NLIST1], n2 = G[G_NLIST2];
    if (n2 <= min_count || !nucleus_binned_ok(n2, H, W, binned_cap)) return;   // no band can hold more than min_count / pair test
    const double* cy = binned + (size_t)im * 2 * binned_cap;
    const double* cx = cy + binned_cap;
    const int32_t* sty = binstart + (size_t)im * 2 * (NUCLEUS_BIN_EXTENT + 2);
    const int32_t* stx = sty + (NUCLEUS_BIN_EXTENT + 2);
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n1; k += gridDim.x * blockDim.x) {
        const int root = list1[(size_t)im * cap + k];
        const size_t slot = (size_t)im * px + root;
        const double a = (double)area[slot];
        const double ny = (double)sumy[slot] / a, nx = (double)sumx[slot] / a;
        if (count_open_interval(cx, stx, W, nx, nx + v) <= min_count) continue;     // left:   nx < cx < nx + v
        if (count_open_interval(cx, stx, W, nx - v, nx) <= min_count) continue;     // right:  nx - v < cx < nx
        if (count_open_interval(cy, sty, H, ny - v, ny) <= min_count) continue;     // bottom: ny - v < cy < ny
        if (count_open_interval(cy, sty, H, ny, ny + v) <= min_count) continue;     // top:    ny < cy < ny + v
        flag[slot] |= 2u;
    }
}

__global__ __launch_bounds__(256) void apply_nucleus_kill_kernel(uint8_t* __restrict__ img, const int32_t* __restrict__ L,
                                                                 const uint32_t* __restrict__ flag, int n_img, size_t px) {
    IMG_PX_LOOP(n_img, px) {
        if (img[t] != 1) continue;
        const int r = L[ib + L[t]];
        if (flag[ib + r] & 2u) img[t] = 0;
    }
}

// The nucleus kill, four pixels per thread (px % 4 == 0, 4-byte-aligned images): one 32-bit load decides for four pixels whether
// anything is a nucleus at all - on a realistic label map 94 % of the pixels are background.
__global__ __launch_bounds__(256) void nucleus_kill4_kernel(uint8_t* __restrict__ img, const int32_t* __restrict__ L,
                                                            const uint32_t* __restrict__ flag, int n_img, size_t px4) {
    IMG_PX_LOOP(n_img, px4) {                                  // t, ib: in 4-pixel groups
        const size_t p0 = t * 4, ibp = ib * 4;
        const uint32_t w = *reinterpret_cast<const uint32_t*>(img + p0);
        uint32_t o = w;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (((w >> (8 * k)) & 0xffu) != 1u) continue;
            const int r = L[ibp + L[p0 + k]];
            if (flag[ibp + r] & 2u) o &= ~(0xffu << (8 * k));
        }
        if (o != w) *reinterpret_cast<uint32_t*>(img + p0) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Fused tile kernels of the clean-up schedule (round 5).  Rounds 1-4 ran every step of the schedule as a pass of its own over
// the whole batch - applier (gathers through the parent image), then each 3x3 stencil: 14 launches and as many round trips
// of the label images through HBM.  Here a workgroup owns one 64 x 32 labelling tile (same blockIdx -> tile map as the CCL
// kernels, so the parents / flags it gathers are in its XCD's L2), evaluates the applier on the tile plus the halo the
// stencils behind it need, keeps the intermediate images in LDS and writes only the final one:
//   thresh_band_kernel    size_thresh applier (src/image_tools.py:41-59) + ecDNA band removal (:64)                halo 1
//   merge_open_kernel     merge_comp applier (:19-30) + grey erosion + grey dilation / combine (:31-32)            halo 2
//                         FINAL: + the last ecDNA dilation (:83)                                                    halo 3
// Halo columns are staged in whole 4-pixel words (4 columns either side); W % 4 == 0 reads the images with 32-bit loads and
// skips the gathers of a word without a labelled pixel at once (94 % of a realistic label map is background).
// ---------------------------------------------------------------------------------------------------------------
constexpr int FT_HX = 4;                     // halo columns staged either side (a whole word)
constexpr int FT_HW = 64 + 2 * FT_HX;        // LDS row pitch in pixels (72 = 18 words)

template <bool W4>
__device__ __forceinline__ uint32_t ft_load_word(const uint8_t* __restrict__ im, size_t p, int x, int W) {
    if (W4) return *reinterpret_cast<const uint32_t*>(im + p);
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (x + k >= 0 && x + k < W) w |= (uint32_t)im[p + k] << (8 * k);
    return w;
}

template <bool W4>
__global__ __launch_bounds__(256) void thresh_band_kernel(CclGeom g, const uint8_t* __restrict__ img_all, uint8_t* __restrict__ out_all,
                                                          const int32_t* __restrict__ L_all, const uint32_t* __restrict__ area_all,
                                                          const int32_t* __restrict__ G_all, int ec_thresh) {
    constexpr int R = 1, HH = CCL_BLOCK_ROWS + 2 * R;
    __shared__ __attribute__((aligned(16))) uint8_t T[HH * FT_HW];
    __shared__ long long gs[4];
    int img, y0, cx;
    if (!decode_block(g, img, y0, cx)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int yblk = y0 - wave * CCL_ROWS, x0 = cx * 64;
    const int H = g.H, W = g.W;
    const size_t base = (size_t)img * H * W;
    if (tid < 4) gs[tid] = g_fold_sum(G_all + (size_t)img * G_IMG, tid == 0 ? G_NCOMP + 2 : tid == 1 ? G_NPX + 2 : tid == 2 ? G_NCOMP + 3 : G_NPX + 3);
    __syncthreads();
    // stage 1: thresholded labels of the tile + halo
    for (int i = tid; i < HH * (FT_HW / 4); i += 256) {
        const int hy = i / (FT_HW / 4), wx = i - hy * (FT_HW / 4);
        const int y = yblk - R + hy, x = x0 - FT_HX + wx * 4;
        uint32_t o = 0;
        if (y >= 0 && y < H && x + 3 >= 0 && x < W) {
            const size_t p0 = (size_t)y * W + x;             // (W4: x is a multiple of 4 inside [0, W))
            const uint32_t w = ft_load_word<W4>(img_all + base, p0, x, W);
            o = w;
            if (w) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t v = (w >> (8 * k)) & 0xffu;
                    if (!v) continue;                          // LUT_MULTI: key = value
                    const int r = L_all[base + L_all[base + p0 + k]];
                    // area < mean(areas) = S / n, evaluated exactly in integers: area * n < S.  (The reference compares in float64;
                    // S / n is an integer or at least 1 / n away from one, far more than a rounding error, so both orders agree.
                    // n == 0: the reference's mean is NaN and every comparison false; here S == 0 gives the same.)
                    const long long a = (long long)area_all[base + r];
                    uint32_t nv = v;
                    if (v == 1) { if (a * gs[0] < gs[1]) nv = 0; }
                    else if (v == 2) { if (a * gs[2] < gs[3]) nv = 3; }
                    else if (v == 3) { if (a < (long long)ec_thresh) nv = 0; }
                    o = (o & ~(0xffu << (8 * k))) | (nv << (8 * k));
                }
            }
        }
        *reinterpret_cast<uint32_t*>(T + hy * FT_HW + wx * 4) = o;
    }
    __syncthreads();
    // stage 2: img[dilate(img == 3) ^ erode(img == 3)] = 0 (dilation pads with 0, erosion with 1)
#pragma unroll
    for (int r = 0; r < CCL_ROWS; ++r) {
        const int y = y0 + r, x = x0 + lane;
        if (y >= H || x >= W) continue;
        const uint8_t* c = T + (wave * CCL_ROWS + r + R) * FT_HW + lane + FT_HX;
        const uint8_t v = c[0];
        const bool cc = v == 3;
        const bool hn = y > 0, hs = y < H - 1, hw = x > 0, he = x < W - 1;
        const bool nn = hn && c[-FT_HW] == 3, ss = hs && c[FT_HW] == 3, ww = hw && c[-1] == 3, ee = he && c[1] == 3;
        const bool dil = cc | nn | ss | ww | ee;
        const bool ero = cc & (hn ? nn : true) & (hs ? ss : true) & (hw ? ww : true) & (he ? ee : true);
        out_all[base + (size_t)y * W + x] = (dil != ero) ? (uint8_t)0 : v;
    }
}

template <bool FINAL, bool W4>
__global__ __launch_bounds__(256) void merge_open_kernel(CclGeom g, const uint8_t* __restrict__ cur_all, uint8_t* __restrict__ out_all,
                                                         const int32_t* __restrict__ L_all, const uint32_t* __restrict__ flag_all,
                                                         const int32_t* __restrict__ G_all, int c, int m, uint32_t lut) {
    constexpr int R = FINAL ? 3 : 2, HH = CCL_BLOCK_ROWS + 2 * R;
    __shared__ __attribute__((aligned(16))) uint8_t Tm[HH * FT_HW];      // merge_comp's working image t (0xff outside the image)
    __shared__ __attribute__((aligned(16))) uint8_t Or[HH * FT_HW];      // the label image itself
    __shared__ __attribute__((aligned(16))) uint8_t Er[HH * FT_HW];      // grey erosion of t (0 outside the image)
    __shared__ __attribute__((aligned(16))) uint8_t Cm[FINAL ? HH * FT_HW : 16];   // FINAL: merged result before the last dilation
    __shared__ int s_last;
    int img, y0, cx;
    if (!decode_block(g, img, y0, cx)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int yblk = y0 - wave * CCL_ROWS, x0 = cx * 64;
    const int H = g.H, W = g.W;
    const size_t base = (size_t)img * H * W;
    if (tid == 0) s_last = g_fold_max(G_all + (size_t)img * G_IMG, G_LAST_ROOT) - 1;
    __syncthreads();
    const int last = s_last;
    // stage 1: t = the image with class m lifted out and every component (of the remaining non-zero pixels) that holds a class-c
    // pixel turned into c - except the component with the highest scipy label (src/image_tools.py:27: range(1, num))
    for (int i = tid; i < HH * (FT_HW / 4); i += 256) {
        const int hy = i / (FT_HW / 4), wx = i - hy * (FT_HW / 4);
        const int y = yblk - R + hy, x = x0 - FT_HX + wx * 4;
        uint32_t t = 0xffffffffu, orig = 0;
        if (y >= 0 && y < H && x + 3 >= 0 && x < W) {
            const size_t p0 = (size_t)y * W + x;
            const uint32_t w = ft_load_word<W4>(cur_all + base, p0, x, W);
            orig = w;
            t = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t v = (w >> (8 * k)) & 0xffu;
                uint32_t tv = (v == (uint32_t)m) ? 0u : v;
                if (!W4 && (x + k < 0 || x + k >= W)) tv = 0xffu;
                else if (v && key_of((uint8_t)v, lut)) {
                    const int r = L_all[base + L_all[base + p0 + k]];
                    if ((flag_all[base + r] & 1u) && r != last) tv = (uint32_t)c;
                }
                t |= tv << (8 * k);
            }
        }
        *reinterpret_cast<uint32_t*>(Tm + hy * FT_HW + wx * 4) = t;
        *reinterpret_cast<uint32_t*>(Or + hy * FT_HW + wx * 4) = orig;
    }
    __syncthreads();
    // stage 2: grey erosion with the 3x3 cross, out-of-image neighbours ignored (0xff never wins a minimum of labels)
    for (int i = tid; i < (HH - 2) * (FT_HW - 2); i += 256) {
        const int hy = 1 + i / (FT_HW - 2), hx = 1 + i % (FT_HW - 2);
        const uint8_t* p = Tm + hy * FT_HW + hx;
        uint8_t v = p[0];
        if (v != 0xff) v = min(min(min(v, p[-1]), min(p[1], p[-FT_HW])), p[FT_HW]);
        Er[hy * FT_HW + hx] = v == 0xff ? (uint8_t)0 : v;
    }
    __syncthreads();
    // stage 3: grey dilation of the eroded image (= opening; the 0 of out-of-image pixels never wins a maximum), pixels whose
    // opened value equals c become c, lifted class m is restored
    auto combine = [&](int hy, int hx) -> uint8_t {
        const uint8_t* e = Er + hy * FT_HW + hx;
        const uint8_t mx = max(max(max(e[0], e[-1]), max(e[1], e[-FT_HW])), e[FT_HW]);
        const uint8_t orig = Or[hy * FT_HW + hx];
        return (orig == m) ? (uint8_t)m : (mx == c ? (uint8_t)c : Tm[hy * FT_HW + hx]);
    };
    if (!FINAL) {
#pragma unroll
        for (int r = 0; r < CCL_ROWS; ++r) {
            const int y = y0 + r, x = x0 + lane;
            if (y >= H || x >= W) continue;
            out_all[base + (size_t)y * W + x] = combine(wave * CCL_ROWS + r + R, lane + FT_HX);
        }
        return;
    }
    // FINAL: the merged image on the tile + 1 pixel, then img[dilate(img == 3)] = 3 (out-of-image neighbours ignored)
    for (int i = tid; i < (CCL_BLOCK_ROWS + 2) * 66; i += 256) {
        const int hy = R - 1 + i / 66, hx = FT_HX - 1 + i % 66;
        const int y = yblk - R + hy, x = x0 - FT_HX + hx;
        Cm[hy * FT_HW + hx] = (y >= 0 && y < H && x >= 0 && x < W) ? combine(hy, hx) : (uint8_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < CCL_ROWS; ++r) {
        const int y = y0 + r, x = x0 + lane;
        if (y >= H || x >= W) continue;
        const uint8_t* q = Cm + (wave * CCL_ROWS + r + R) * FT_HW + lane + FT_HX;
        const bool d = q[0] == 3 || q[-1] == 3 || q[1] == 3 || q[-FT_HW] == 3 || q[FT_HW] == 3;
        out_all[base + (size_t)y * W + x] = d ? (uint8_t)3 : q[0];
    }
}
template <bool FINAL>
static void launch_merge_open(bool v4, const CclGeom& g, const uint8_t* in, uint8_t* out, const PostWorkspace& ws, const int32_t* G,
                              int c, int m, uint32_t lut, hipStream_t s) {
    auto* k = v4 ? merge_open_kernel<FINAL, true> : merge_open_kernel<FINAL, false>;
    hipLaunchKernelGGL(k, dim3(geom_grid(g)), dim3(256), 0, s, g, in, out, ws.L, ws.flag, G, c, m, lut);
}

// test-only (stages_debug): which nucleus pixels the metaphase test erases, read from the flag words before the kill kernel runs
__global__ __launch_bounds__(256) void export_nucleus_kill_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ L,
                                                                  const uint32_t* __restrict__ flag, int n_img, size_t px,
                                                                  uint8_t* __restrict__ kill) {
    IMG_PX_LOOP(n_img, px) kill[t] = (img[t] == 1 && (flag[ib + L[ib + L[t]]] & 2u)) ? 1 : 0;
}

// Stages first..last of the clean-up (1 fill_holes(1), 2 fill_holes(2), 3 size_thresh + band, 4 nucleus test, 5 merge_comp(1),
// 6 merge_comp(2) + final dilation): `img` holds the input of stage `first` and receives the image after stage `last`.  1..6 is
// the production schedule, launch for launch; a partial range (test-only) adds the copies into the buffer a stage expects
// (ws.tmpA from stage 4 on) and out of the one it leaves its result in.  kill_dev (test-only, with stage 4): see above.
hipError_t run_meta_inference(PostWorkspace& ws, uint8_t* img, int n_img, int H, int W, int32_t* n_ec_dev, hipStream_t s,
                              int first, int last, uint8_t* kill_dev) {
    if (n_img <= 0) return hipSuccess;
    if (first < 1 || last > 6 || first > last) return hipErrorInvalidValue;
    const CclGeom g = make_geom(n_img, H, W);
    const size_t px = (size_t)H * W;
    const dim3 ig = img_grid(px, n_img);
    const unsigned tg = geom_grid(g);
    // W % 4 == 0 and 4-byte-aligned images: 32-bit loads in the fused tile kernels, four pixels per thread in the nucleus kill
    const bool v4 = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(ws.tmpA) |
                                      reinterpret_cast<uintptr_t>(ws.tmpB)) & 3) == 0;
    const dim3 ig4 = img_grid(px / 4, n_img);
    hipError_t e;
    // one counter block per labelling that produces counters, all zeroed here: no zeroing / folding launches in between
    // (a kernel, not hipMemsetAsync: when these launches were replayed from a captured graph, the memset node of ROCm 7.2 was not ordered
    // before the kernels behind it and zeroed list counters in mid-use: a memory fault on speckled images, round 5)
    const size_t gslot = (size_t)ws.cap_img * G_IMG;
    launch_zero_g(ws.g, (int)((n_ec_dev ? 5 : 4) * gslot), s);
    // 1. fill_holes(1), fill_holes(2)
    for (int c = 1; c <= 2; ++c) {
        if (c < first || c > last) continue;
        CclPass p{img, lut_ne(c), 4, 0, AUX_BORDER, 0, nullptr, 0};
        p.sparse = true;
        p.allow_full = true;
        if ((e = run_ccl_pass(ws, g, p, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(apply_fill_tile_kernel, dim3(tg), dim3(256), 0, s, g, img, ws.L, ws.flag, c, lut_ne(c), ws.tile_any, ws.own_bits);
    }
    // 2-5. size_thresh + ecDNA band removal -> ws.tmpA (the caller's buffer is free from here until the last step writes the
    // result into it)
    uint8_t* cur = ws.tmpA;
    uint8_t* nxt = ws.tmpB;
    const size_t tot = px * (size_t)n_img;
    if (first > 3 && (e = hipMemcpyAsync(cur, img, tot, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;    // (partial range)
    if (first <= 3 && last >= 3) {
        CclPass p{img, LUT_MULTI, 8, STAT_AREA, AUX_NONE, 0, nullptr, NEED_NCOMP | NEED_NPX};
        p.sparse = true;
        p.g = ws.g + 0 * gslot;
        if ((e = run_ccl_pass(ws, g, p, s)) != hipSuccess) return e;
        if (v4) hipLaunchKernelGGL(thresh_band_kernel<true>, dim3(tg), dim3(256), 0, s, g, img, cur, ws.L, ws.area, p.g, 15);
        else hipLaunchKernelGGL(thresh_band_kernel<false>, dim3(tg), dim3(256), 0, s, g, img, cur, ws.L, ws.area, p.g, 15);
    }
    // 6. nucleus-in-metaphase test
    if (first <= 4 && last >= 4) {
        const size_t cap = px / 4 + (size_t)(H + W) / 2 + 4;
        int32_t* list1 = ws.list;
        double2* list2 = reinterpret_cast<double2*>(ws.list + (((size_t)n_img * cap + 3) & ~(size_t)3));
        CclPass p{cur, LUT_MULTI, 8, STAT_AREA | STAT_SUMS, AUX_NONE, 0, nullptr, NEED_LISTS};
        p.sparse = true;
        p.g = ws.g + 1 * gslot;
        p.list1 = list1; p.list2 = reinterpret_cast<int32_t*>(list2); p.list_cap = cap;
        if ((e = run_ccl_pass(ws, g, p, s)) != hipSuccess) return e;
        const bool binned = H <= NUCLEUS_BIN_EXTENT && W <= NUCLEUS_BIN_EXTENT;
        // the pair test is only ever needed for images the binned test cannot take: extents beyond the LDS histogram, or more
        // chromosomes than `binned` holds (n2 <= cap); it reads the centroids that centroids_kernel leaves in the list
        const bool pairs = !binned || cap > ws.binned_cap;
        if (pairs) hipLaunchKernelGGL(centroids_kernel, dim3(8, n_img), dim3(256), 0, s, ws.area, ws.sumy, ws.sumx, p.g, list2, px, cap);
        if (binned) {
            const size_t bin_lds = (size_t)(std::max(H, W) + 2) * sizeof(int);
            static DeviceOnce bin_attr;                            // up to 128 KB of dynamic LDS: per-device function attribute
            e = bin_attr.run([] {
                return hipFuncSetAttribute(reinterpret_cast<const void*>(bin_centroids_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)((NUCLEUS_BIN_EXTENT + 2) * sizeof(int)));
            });
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(bin_centroids_kernel, dim3(2, n_img), dim3(1024), bin_lds, s, p.g, list2, ws.binned, ws.binstart,
                               cap, ws.binned_cap, H, W, ws.area, ws.sumy, ws.sumx, px, pairs ? 1 : 0);
            hipLaunchKernelGGL(nucleus_test_binned_kernel, dim3(32, n_img), dim3(256), 0, s, ws.area, ws.sumy, ws.sumx, p.g,
                               list1, ws.binned, ws.binstart, ws.flag, px, cap, ws.binned_cap, H, W, 70.0, 5);
        }
        if (pairs) {
            const int bpi = 32;
            hipLaunchKernelGGL(nucleus_test_kernel, dim3(n_img * bpi), dim3(256), 0, s, ws.area, ws.sumy, ws.sumx, p.g, list1,
                               list2, ws.flag, px, cap, bpi, 70.0, 5, H, W, ws.binned_cap);
        }
        if (kill_dev) hipLaunchKernelGGL(export_nucleus_kill_kernel, ig, dim3(256), 0, s, cur, ws.L, ws.flag, n_img, px, kill_dev);
        if (v4) hipLaunchKernelGGL(nucleus_kill4_kernel, ig4, dim3(256), 0, s, cur, ws.L, ws.flag, n_img, px / 4);
        else hipLaunchKernelGGL(apply_nucleus_kill_kernel, ig, dim3(256), 0, s, cur, ws.L, ws.flag, n_img, px);
    }
    // 7-8. merge_comp(1), merge_comp(2); 9. the final ecDNA dilation rides on the second one, which writes the caller's buffer
    for (int c = 1; c <= 2; ++c) {
        if (c + 4 < first || c + 4 > last) continue;
        const int m = (c == 1) ? 2 : 1;
        const uint32_t lut = lut_nonzero_except(m);
        CclPass p{cur, lut, 8, 0, AUX_VALUE_EQ, c, nullptr, NEED_LAST};
        p.sparse = true;
        p.g = ws.g + (size_t)(1 + c) * gslot;
        if ((e = run_ccl_pass(ws, g, p, s)) != hipSuccess) return e;
        if (c == 1) {
            launch_merge_open<false>(v4, g, cur, nxt, ws, p.g, c, m, lut, s);
            std::swap(cur, nxt);
        } else {
            launch_merge_open<true>(v4, g, cur, img, ws, p.g, c, m, lut, s);
        }
    }
    if (last >= 3 && last <= 5 && (e = hipMemcpyAsync(img, cur, tot, hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;   // (partial range)
    // 10. count_cc(img == 3)[0]
    if (n_ec_dev && last == 6) {
        CclPass p{img, lut_eq(3), 8, 0, AUX_NONE, 0, nullptr, NEED_NCOMP | NEED_NPX, true};
        p.sparse = true;
        p.g = ws.g + 4 * gslot;
        if ((e = run_ccl_pass(ws, g, p, s)) != hipSuccess) return e;
        launch_gather_counts(p.g, n_img, 1, n_ec_dev, nullptr, (long long)px, 1, s);
    }
    return hipGetLastError();
}

}  // namespace ecseg
