// Host and device: the layout of ecseg_min_cut_regions (drivers_fish.hip, mincut_centers_kernels.hip), stated once and shared with
// the host program that walks it under ASan + UBSan (tools/asan/min_cut_regions_check.cpp).  No HIP in here.
//
// The call labels the nucleus mask 4-connected, 1..n in raster order of first pixels, and takes the driver through three counts:
// the cells, then - from their areas and boxes - the selected regions with their windows, then the centre components per region.
//   * selection (src/max_flow_binary_mask.py:205-206,214): np.median of the n areas in double - the middle value, or the mean of the
//     two middle values - and the labels with (double)area > coeff * median, strictly, in ascending label order;
//   * windows: the bounding-box crops labels[box] == k, uint8, row-major, back to back: region i starts at the sum of the sizes of
//     the regions in front, which is the layout ecseg_min_cut takes for `masks`.  `comp` (int32) is laid out alike, by element;
//   * the centre kernel keeps ONE int32 per pixel of a crop - first its distance, then its union-find parent: in LDS, rows
//     mcr_stride(w) apart, for crops that mcr_in_lds admits, else in the crop's own elements of `comp` (stride w);
//   * centre records: region i's records start at the sum of the component counts of the regions in front.
// The capacity rule (the ecseg_fish_spots protocol): the three counts are always written; the buffers only when all three fit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MCR_HD __host__ __device__
#else
#define MCR_HD
#endif

#include <algorithm>
#include <string>
#include <vector>

#include "scratch.h"

namespace ecseg {

constexpr int MCR_LDS_PIXELS = 8192;                   // ECSEG_MIN_CUT_CENTERS_LDS_PIXELS: the default threshold
constexpr int MCR_LDS_CELLS = 10240;                   // int32 cells of LDS state (40 KiB): a crop's h * mcr_stride(w) must fit
constexpr int MCR_MAX_PIXELS = 1 << 22;                // ECSEG_MIN_CUT_MAX_PIXELS
constexpr long long MCR_MAX_BYTES = 1ll << 28;         // ECSEG_MIN_CUT_MAX_BYTES
constexpr int MCR_FAR = 1 << 30;                       // the distance in a crop without a zero pixel
constexpr int MCR_REC = 8;                             // int32 per region record and per centre record

// Row stride of the LDS state: odd, so that the row pass - one thread per row, all lanes at the same column - puts 64 consecutive
// rows on 64 different banks (64 banks of 4 bytes: r * stride mod 64 is a bijection of r mod 64 exactly for an odd stride).
MCR_HD inline int mcr_stride(int w) { return w | 1; }
// Whether a crop's state lives in LDS under the threshold lds_pixels (the option min_cut_centers_lds_pixels).
MCR_HD inline bool mcr_in_lds(int h, int w, int lds_pixels) {
    const long long n = (long long)h * w;
    return n <= lds_pixels && (long long)h * mcr_stride(w) <= MCR_LDS_CELLS;
}
// FAR + 1 stays FAR (both passes of the distance transform add 1 to a neighbour's value).
MCR_HD inline int mcr_sat_inc(int v) { return v >= MCR_FAR ? MCR_FAR : v + 1; }
// The centroid of n pixels with coordinate sum S under np.round, i.e. half to even, in integers: floor(S / n + 1/2), one less when
// the mean is exactly k + 1/2 (2 S == n (2 k + 1)) and that floor is odd.
MCR_HD inline int mcr_round_mean(long long S, long long n) {
    const long long q = (2 * S + n) / (2 * n), r = (2 * S + n) % (2 * n);
    return (int)((r == 0 && (q & 1)) ? q - 1 : q);
}

// The most 8-connected components the centre pixels of an h x w crop can form: they lie in its (h - 2) x (w - 2) interior, and two
// pixels of one 2 x 2 block always touch.
MCR_HD inline int mcr_center_bound(int h, int w) { return (h < 3 || w < 3) ? 0 : ((h - 1) / 2) * ((w - 1) / 2); }

// np.median over int32 areas, in double.  n >= 1.
inline double mcr_median(const int32_t* areas, int n) {
    std::vector<int32_t> v(areas, areas + n);
    std::sort(v.begin(), v.end());
    return (n & 1) ? (double)v[(size_t)n / 2] : ((double)v[(size_t)n / 2 - 1] + (double)v[(size_t)n / 2]) / 2.0;
}

struct McrPlan {
    std::vector<int32_t> regions;                      // (n_regions, MCR_REC): label, r0, c0, h, w, window offset, 0, 0
    long long window_pixels = 0;
    int n_regions = 0, n_lds = 0;                      // n_lds: regions whose state is in LDS
    size_t max_pixels = 0;                             // the largest window
};

// stats: (n, 5) int32 per label 1..n: area, first row, last row, first column, last column.  Empty string and P, or what is wrong.
inline std::string mcr_plan(const int32_t* stats, int n, double coeff, int lds_pixels, McrPlan& P) {
    P = McrPlan();
    if (n <= 0) return std::string();
    std::vector<int32_t> areas((size_t)n);
    for (int k = 0; k < n; ++k) areas[(size_t)k] = stats[5 * (size_t)k];
    const double bound = coeff * mcr_median(areas.data(), n);
    for (int k = 0; k < n; ++k) {
        const int32_t* q = stats + 5 * (size_t)k;
        if (!((double)q[0] > bound)) continue;
        const long long h = (long long)q[2] - q[1] + 1, w = (long long)q[4] - q[3] + 1;
        if (h < 1 || w < 1) return "label " + std::to_string(k + 1) + " has an empty bounding box";
        if (h * w > MCR_MAX_PIXELS)
            return "the crop of label " + std::to_string(k + 1) + " holds " + std::to_string(h * w) + " pixels, more than ECSEG_MIN_CUT_MAX_PIXELS = " +
                   std::to_string(MCR_MAX_PIXELS);
        if (P.window_pixels + h * w > MCR_MAX_BYTES)
            return "the windows hold more than ECSEG_MIN_CUT_MAX_BYTES = " + std::to_string(MCR_MAX_BYTES) + " bytes (at label " + std::to_string(k + 1) + ")";
        const int32_t rec[MCR_REC] = {k + 1, q[1], q[3], (int32_t)h, (int32_t)w, (int32_t)P.window_pixels, 0, 0};
        P.regions.insert(P.regions.end(), rec, rec + MCR_REC);
        P.window_pixels += h * w;
        P.n_regions += 1;
        P.n_lds += mcr_in_lds((int)h, (int)w, lds_pixels);
        P.max_pixels = std::max(P.max_pixels, (size_t)(h * w));
    }
    return std::string();
}

// Fills [6] (first centre record) and [7] (components) of every region from the device's counts -> the number of centre records,
// or -1 when it leaves int32.
inline long long mcr_place_centers(McrPlan& P, const int32_t* counts) {
    long long at = 0;
    for (int i = 0; i < P.n_regions; ++i) {
        P.regions[(size_t)i * MCR_REC + 6] = (int32_t)at;
        P.regions[(size_t)i * MCR_REC + 7] = counts[i];
        at += counts[i];
        if (at >= (1ll << 31)) return -1;
    }
    return at;
}

// The capacity rule: all three must fit, or none of the capacity-bound buffers is written.
inline bool mcr_fits(int n_regions, long long n_centers, long long window_pixels, int region_capacity, int center_capacity,
                     long long window_capacity) {
    return n_regions <= region_capacity && n_centers <= center_capacity && window_pixels <= window_capacity;
}

// ---- the arena slots ---------------------------------------------------------------------------------------------------------------
// Device buffers of ecseg_min_cut_regions that the image alone sizes: the mask, the labels, the dense index rid over the root
// flags with its scan blocks, and misc ([0] = number of labels).
struct McrOpenBufs { uint8_t* mask; int32_t* lab; int32_t* rid; int32_t* blk; int32_t* misc; };
inline McrOpenBufs mcr_open_bufs(Carver& c, int H, int W) {
    const size_t px = (size_t)H * W;
    McrOpenBufs b;
    b.mask = c.take<uint8_t>(px); b.lab = c.take<int32_t>(px); b.rid = c.take<int32_t>(px); b.blk = c.take<int32_t>((px + 1023) / 1024);
    b.misc = c.take<int32_t>(4);
    return b;
}
// What the selection sizes: the region records, per region its component count, first record and accumulator slot, the total, the
// windows and components (window_pixels each), and `slots` components' worth of accumulators and centre records.
struct McrRegionBufs { int32_t* regions; int32_t* counts; int32_t* first; int32_t* slot; int32_t* total; uint8_t* windows; int32_t* comp;
                       unsigned long long* acc; int32_t* centers; };
inline McrRegionBufs mcr_region_bufs(Carver& c, int n_regions, size_t window_pixels, size_t slots) {
    const size_t n = (size_t)n_regions;
    McrRegionBufs b;
    b.regions = c.take<int32_t>(n * MCR_REC); b.counts = c.take<int32_t>(n); b.first = c.take<int32_t>(n); b.slot = c.take<int32_t>(n);
    b.total = c.take<int32_t>(1); b.windows = c.take<uint8_t>(window_pixels); b.comp = c.take<int32_t>(window_pixels);
    b.acc = c.take<unsigned long long>(slots * 3); b.centers = c.take<int32_t>(slots * MCR_REC);
    return b;
}

}  // namespace ecseg
