// Stand-alone check of the drivers' scratch layouts (tests/test_scratch_layout.py builds it with the host compiler and
// -fsanitize=address,undefined; no HIP call is made).  For every layout function of csrc/common.h and each shape: the measuring
// and the placing pass agree, every slot is 256-byte aligned, lies inside the measured total and apart from the others, and
// holds exactly the bytes that the driver's own allocation of that buffer held before the arenas (the formulae below are those
// allocations' sizes, written out).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "../ecseg_amd/csrc/common.h"

using namespace ecseg;

struct Want { const char* name; const void* ptr; size_t bytes; };
struct Slot { size_t off, bytes; };
struct Recorder : Carver {                                   // the library's carver, with every slot handed out written down
    std::vector<Slot> slots;
    explicit Recorder(void* arena = nullptr) : Carver(arena) {}
    uintptr_t take_bytes(size_t bytes) override {
        slots.push_back({used, bytes});
        return Carver::take_bytes(bytes);
    }
};
typedef std::function<std::vector<Want>(Carver&)> Layout;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; printf("FAIL %s: ", family); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check(const char* family, const Layout& layout) {
    Recorder m;
    const std::vector<Want> wm = layout(m);
    const std::vector<Slot>& tm = m.slots;
    CHECK(m.used > 0 && m.used % 256 == 0, "measured total %zu", m.used);
    uint8_t* arena = static_cast<uint8_t*>(aligned_alloc(256, m.used));
    if (!arena) { printf("no memory for %s\n", family); exit(2); }
    memset(arena, 0, m.used);
    Recorder p(arena);
    const std::vector<Want> wp = layout(p);
    const std::vector<Slot>& tp = p.slots;
    CHECK(p.used == m.used, "totals differ: %zu measured, %zu placed", m.used, p.used);
    CHECK(tm.size() == tp.size() && wm.size() == wp.size() && wm.size() == tm.size(), "%zu slots measured, %zu placed, %zu fields listed",
          tm.size(), tp.size(), wm.size());
    for (size_t i = 0; i < wm.size() && i < wp.size(); ++i) {
        const size_t om = reinterpret_cast<uintptr_t>(wm[i].ptr), op = static_cast<const uint8_t*>(wp[i].ptr) - arena;
        const char* name = wm[i].name;
        CHECK(om == op, "%s: offset %zu measured, %zu placed", name, om, op);
        CHECK(op % 256 == 0, "%s: offset %zu is not 256-byte aligned", name, op);
        CHECK(wm[i].bytes == wp[i].bytes, "%s: the check itself is inconsistent", name);
        size_t carved = (size_t)-1, hits = 0;
        for (const Slot& s : tp) if (s.off == op) { carved = s.bytes; ++hits; }
        CHECK(hits == 1, "%s: %zu slots at offset %zu", name, hits, op);
        CHECK(carved == wp[i].bytes, "%s: %zu bytes carved, %zu wanted", name, carved, wp[i].bytes);
        CHECK(op + std::max<size_t>(wp[i].bytes, 1) <= m.used, "%s: [%zu, +%zu) leaves the total %zu", name, op, wp[i].bytes, m.used);
        if (op + wp[i].bytes <= m.used) memset(arena + op, (int)(i + 1), wp[i].bytes);   // (ASan: inside the allocation)
    }
    for (size_t i = 0; i < wp.size(); ++i) {                 // nobody wrote over anybody: the slots are disjoint
        const uint8_t* q = static_cast<const uint8_t*>(wp[i].ptr);
        size_t bad = 0;
        for (size_t k = 0; k < wp[i].bytes; ++k) bad += q[k] != (uint8_t)(i + 1);
        CHECK(bad == 0, "%s: %zu bytes overwritten by another slot", wp[i].name, bad);
    }
    std::vector<Slot> sorted = tp;
    std::sort(sorted.begin(), sorted.end(), [](const Slot& a, const Slot& b) { return a.off < b.off; });
    for (size_t i = 0; i + 1 < sorted.size(); ++i)
        CHECK(sorted[i].off + std::max<size_t>(sorted[i].bytes, 1) <= sorted[i + 1].off, "slots at %zu and %zu overlap", sorted[i].off, sorted[i + 1].off);
    for (size_t i = 0; i < tm.size() && i < tp.size(); ++i)
        CHECK(tm[i].off == tp[i].off && tm[i].bytes == tp[i].bytes, "slot %zu: measured (%zu, %zu), placed (%zu, %zu)", i, tm[i].off, tm[i].bytes,
              tp[i].off, tp[i].bytes);
    free(arena);
    ++g_checked;
}

// the helpers of the kernel files that size a buffer, restated
static int slices_of(int n) { return n <= 0 ? 1 : (4096 / n < 1 ? 1 : (4096 / n > 256 ? 256 : 4096 / n)); }
static int sort_len_of(int N) { int P = 2048; while (P < N) P <<= 1; return P; }
static size_t mincut_scratch_of(int h, int w) { const size_t n4 = ((size_t)h * w + 3) / 4 * 4; return (2 * n4 + 4 * (size_t)h * w + 15) / 16 * 16; }

#define W(b, f, bytes) Want{#f, (b).f, (size_t)(bytes)}

static void check_shape(int H, int W_, int n, int C, int n_img) {
    const int Wd = W_;
    const size_t px = (size_t)H * Wd, nn = (size_t)n;
    char tag[64];
    snprintf(tag, sizeof(tag), " %d x %d", H, Wd);
    auto name = [&](const char* f) { static char buf[128]; snprintf(buf, sizeof(buf), "%s%s", f, tag); return buf; };

    {   // ensure_post(n_img, px)
        const size_t ni = (size_t)n_img, tot = ni * px, list_cap = px / 4 + px / 2 + 8, binned_cap = std::min(list_cap, (size_t)1 << 20);
        check(name("post_workspace"), [&](Carver& c) {
            const PostWorkspace w = post_workspace(c, n_img, px);
            if (w.cap_img != n_img || w.cap_px != px || w.binned_cap != binned_cap) { ++g_failed; printf("FAIL post_workspace: capacities\n"); }
            return std::vector<Want>{W(w, L, tot * 4), W(w, area, tot * 4), W(w, sumy, tot * 8), W(w, sumx, tot * 8), W(w, flag, tot * 4), W(w, tmpA, tot),
                                     W(w, tmpB, tot), W(w, list, ni * list_cap * 20 + 256), W(w, g, (size_t)G_SLOTS * ni * G_STRIDE * G_SHARDS * 4),
                                     W(w, tile_any, ni * (px / 16 + 2)), W(w, own_bits, ni * (px / 31 + 4) * 256),
                                     W(w, binned, ni * 2 * binned_cap * sizeof(double)), W(w, binstart, ni * 2 * (NUCLEUS_BIN_EXTENT + 2) * sizeof(int32_t))};
        });
    }
    {   // ecseg_nuclei_regions: image of (H, W + 3, C), capacity n
        const int img_w = Wd + 3;
        check(name("region_map_bufs"), [&](Carver& c) {
            const RegionMapBufs b = region_map_bufs(c, H, Wd, img_w, C);
            return std::vector<Want>{W(b, lab, px * 4), W(b, img, (size_t)H * img_w * C)};
        });
        check(name("region_bufs"), [&](Carver& c) {
            const RegionBufs b = region_bufs(c, H, Wd, n);
            if (b.cap != n) { ++g_failed; printf("FAIL region_bufs: cap\n"); }
            return std::vector<Want>{W(b, rid, px * 4), W(b, blk, (px + 1023) / 1024 * 4), W(b, misc, 4 * 4), W(b, acc, nn * 4 * 8), W(b, bb, nn * 4 * 4),
                                     W(b, rec, nn * 8 * 8)};
        });
        const int nc = std::min(n, 256);
        check(name("crop_bufs"), [&](Carver& c) {
            const CropBufs b = crop_bufs(c, nc);
            return std::vector<Want>{W(b, desc, (size_t)nc * 5 * 4), W(b, crops, (size_t)nc * 256 * 256 * 3), W(b, max, (size_t)nc * 3 * 4)};
        });
    }
    CellIndexBufs cells{};
    {   // open_dense_cells
        check(name("cell_index_bufs"), [&](Carver& c) {
            cells = cell_index_bufs(c, H, Wd, C);
            return std::vector<Want>{W(cells, lab, px * 4), W(cells, img, px * C), W(cells, rid, px * 4), W(cells, blk, (px + 1023) / 1024 * 4),
                                     W(cells, misc, 4 * 4)};
        });
    }
    {   // ecseg_fish_distances
        const size_t parts = nn * (size_t)slices_of(n);
        check(name("fishdist_bufs"), [&](Carver& c) {
            const FishDistBufs b = fishdist_bufs(c, cells, H, Wd, n, slices_of(n));
            if (b.rid != cells.rid || b.blk != cells.blk || b.misc != cells.misc) { ++g_failed; printf("FAIL fishdist_bufs: the cell index\n"); }
            return std::vector<Want>{W(b, par, px * 4), W(b, flist, px * 8), W(b, clist, px * 8), W(b, acc, nn * 4 * 4), W(b, val, nn * 4), W(b, off, nn * 2 * 4),
                                     W(b, cur, nn * 2 * 4), W(b, rec, nn * 8 * 8), W(b, pbest, parts * 8), W(b, proots, parts * 4)};
        });
    }
    for (int np = 1; np <= 3; np += 2) {   // ecseg_fish_spots
        const int K = np == 1 ? 1 : 7;
        check(name("fishspot_bufs"), [&](Carver& c) {
            const FishSpotBufs b = fishspot_bufs(c, cells, H, Wd, np, K, n);
            if (b.rid != cells.rid) { ++g_failed; printf("FAIL fishspot_bufs: the cell index\n"); }
            return std::vector<Want>{W(b, mx, 4 * 4), W(b, w, (size_t)K * K * 8), W(b, thr, px * np), W(b, bnd, px), W(b, par, px * 4 * 4), W(b, sz, px * 4 * 4),
                                     W(b, acc, nn * 12 * 8), W(b, cnt, nn * 8 * 4), W(b, val, nn * 4), W(b, rec, nn * ECSEG_FISH_SPOT_INT64 * 8)};
        });
    }
    for (int global = 0; global <= 1; ++global) {   // ecseg_min_cut: n windows of H x W (capped), in LDS or all in global memory
        const int th = std::min(H, 100), tw = std::min(Wd, 120);
        const size_t nb = nn * th * tw, scratch = global ? nn * mincut_scratch_of(th, tw) : 0;
        check(name("mincut_bufs"), [&](Carver& c) {
            const MinCutBufs b = mincut_bufs(c, nb, n, scratch);
            return std::vector<Want>{W(b, mask, nb), W(b, side, nb), W(b, desc, nn * 8 * 4), W(b, soff, nn * 8), W(b, flow, nn * 4), W(b, scratch, scratch)};
        });
    }
    {   // ecseg_nuset_forward
        check(name("nuset_mask_bufs"), [&](Carver& c) {
            const NusetMaskBufs b = nuset_mask_bufs(c, H, Wd);
            return std::vector<Want>{W(b, mask, px)};
        });
    }
    for (int upload = 0; upload <= 1; ++upload) {   // ecseg_rpn_proposals / ecseg_rpn_proposals_last on the stride-16 feature map
        const int fh = (H + 15) / 16, fw = (Wd + 15) / 16, A = H == 1 ? 1 : 9, pre = 6000, post = 800;
        const size_t fpx = (size_t)fh * fw, N = fpx * A, K = std::min<size_t>(pre, N), words = (K + 63) / 64, no = std::min<size_t>(post, K);
        check(name("rpn_bufs"), [&](Carver& c) {
            const RpnBufs b = rpn_bufs(c, fh, fw, A, sort_len_of((int)N), pre, post, upload != 0);
            return std::vector<Want>{W(b, ref, (size_t)A * 4 * 8), W(b, boxes, N * 16), W(b, scores, N * 4), W(b, keys, (size_t)sort_len_of((int)N) * 8),
                                     W(b, mat, K * words * 8), W(b, misc, 2 * 4), W(b, out_scores, no * 4), W(b, out_boxes, no * 16), W(b, out_idx, no * 4),
                                     W(b, cls, upload ? fpx * 2 * A * 4 : 0), W(b, bbox, upload ? fpx * 4 * A * 4 : 0)};
        });
    }
    {   // ecseg_clean_nuclei
        check(name("clean_bufs"), [&](Carver& c) {
            const CleanBufs b = clean_bufs(c, H, Wd);
            return std::vector<Want>{W(b, mask, px), W(b, tmp, px), W(b, cleaned, px), W(b, out, px), W(b, par, px * 4), W(b, sz, px * 4), W(b, misc, 4 * 4),
                                     W(b, dbl, 2 * 8)};
        });
    }
    for (int full = 0; full <= 1; ++full) {   // ecseg_marker_watershed: n markers (and none), the heap of a half and of a full mask
        const int nm = full ? n : 0;
        const size_t fg = full ? px : px / 2, cap = 5 * fg + 1;
        check(name("watershed_bufs"), [&](Carver& c) {
            const WatershedBufs b = watershed_bufs(c, H, Wd, nm, (int)cap);
            return std::vector<Want>{W(b, mask, px), W(b, out, px), W(b, par, px * 4), W(b, sz, px * 4), W(b, misc, 4 * 4), W(b, idx, px * 4), W(b, rw, px * 4),
                                     W(b, g, px * 4), W(b, d2, px * 4), W(b, lab, px * 4), W(b, work, px), W(b, filled, px), W(b, rows, (size_t)nm * 4),
                                     W(b, cols, (size_t)nm * 4), W(b, labels, (size_t)nm * 4), W(b, heap_k, cap * 8), W(b, heap_p, cap * 8)};
        });
    }
    {   // ecseg_rescale_down to half the extent, ecseg_rescale_mask_up back from it
        const int oh = (H + 1) / 2, ow = (Wd + 1) / 2;
        const size_t opx = (size_t)oh * ow, wlen = 2 * ECSEG_RESCALE_MAX_RADIUS + 1;
        check(name("rescale_down_bufs"), [&](Carver& c) {
            const RescaleDownBufs b = rescale_down_bufs(c, H, Wd, oh, ow);
            return std::vector<Want>{W(b, img, px), W(b, tmp, px), W(b, filtered, px), W(b, v, opx * 8), W(b, wy, wlen * 8), W(b, wx, wlen * 8)};
        });
        check(name("rescale_up_bufs"), [&](Carver& c) {
            const RescaleUpBufs b = rescale_up_bufs(c, oh, ow, H, Wd);
            return std::vector<Want>{W(b, cleaned, opx), W(b, out, px), W(b, par, px * 4), W(b, sz, px * 4), W(b, v, px * 8), W(b, mm, 2 * 8)};
        });
    }
}

int main() {
    {   // the carver itself: zero elements still make a slot of their own
        const char* family = "carver";
        Carver c;
        int* a = c.take<int>(0);
        char* b = c.take<char>(1);
        double* d = c.take<double>(33);
        CHECK(reinterpret_cast<uintptr_t>(a) == 0 && reinterpret_cast<uintptr_t>(b) == 256 && reinterpret_cast<uintptr_t>(d) == 512 && c.used == 1024,
              "offsets %zu %zu %zu, total %zu", (size_t)reinterpret_cast<uintptr_t>(a), (size_t)reinterpret_cast<uintptr_t>(b),
              (size_t)reinterpret_cast<uintptr_t>(d), c.used);
    }
    check_shape(1, 1, 1, 1, 1);           // the smallest: one cell, one marker, one task, one image
    check_shape(33, 70, 7, 3, 65);        // no multiple of the 64 x 32 tile; post_chunk + 1 images
    check_shape(1040, 1392, 300, 4, 2);
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("scratch_layout ok: %d layouts\n", g_checked);
    return 0;
}
