// Host check of csrc/fishdist_batch.h, the layout of ecseg_fish_distances_batch, under ASan + UBSan (make asan_fishdist_batch; CPU
// only): the layout function walked over seeded shape lists - extents of 1, single rows and columns, ragged last tiles of the 64 x 32
// statistics tile, mixed C, in call order and reversed - and held to
//   * the lookup: EVERY tile index and EVERY 256-pixel block index of the chunk maps to the image a plain loop gives it, and every
//     thread of it to a local pixel inside that image or to nothing; every pixel of every image is visited exactly once by each walk;
//   * the bases: the images' shares of the pixel axis and of the lsq bytes are disjoint, in call order and without a gap;
//   * the byte counts: pixels, lsq bytes, tiles and blocks against a plain loop, fdb_pixel_bytes / fdb_cell_bytes / fdb_group_bytes
//     against what the Carver measures, the second part for fewer cells inside the room measured for the bound;
//   * the groups: consecutive, complete, each within the limit unless it is a single image;
//   * the refusals: exactly at the limits (one image, the chunk's pixels, the chunk's lsq bytes, the image count), naming the image.
// The per-pixel arrays are written through the offsets into real memory of exactly the measured size: a wrong offset is a heap overflow.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>

#include "../../ecseg_amd/csrc/fishdist_batch.h"

using namespace ecseg;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "fishdist_batch_check: %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Recorder : Carver {                               // a measuring carver that keeps every slot
    std::vector<std::pair<size_t, size_t>> slots;        // offset, bytes
    uintptr_t take_bytes(size_t bytes) override {
        const size_t off = used;
        const uintptr_t p = Carver::take_bytes(bytes);
        slots.push_back({off, bytes});
        return p;
    }
};

static int slices(int n) { return n <= 0 ? 1 : (4096 / n < 1 ? 1 : (4096 / n > 256 ? 256 : 4096 / n)); }   // fishdist_slices

static void check(const std::vector<int32_t>& shapes, int capacity) {
    const int n = (int)(shapes.size() / 3);
    FdbLayout L;
    REQUIRE(fdb_layout(shapes.data(), 0, n, L).empty());
    REQUIRE((int)L.tab.size() == n);
    // the bases and the counts against a plain loop
    long long px = 0, lsq = 0, tiles = 0, blocks = 0;
    int ext = 0;
    for (int i = 0; i < n; ++i) {
        const int H = shapes[3 * i], W = shapes[3 * i + 1], C = shapes[3 * i + 2];
        const FdbImage& t = L.tab[(size_t)i];
        REQUIRE(t.H == H && t.W == W && t.C == C);
        REQUIRE(t.px0 == px && t.lsq0 == lsq && t.tile0 == tiles && t.blk0 == blocks);       // back to back: disjoint, no gap
        px += (long long)H * W; lsq += (long long)H * W * C;
        tiles += (long long)((W + 63) / 64) * ((H + 31) / 32);
        blocks += ((long long)H * W + 255) / 256;
        ext = std::max(ext, std::max(H, W));
    }
    REQUIRE(L.px == px && L.lsq == lsq && L.tiles == tiles && L.blocks == blocks && L.max_extent == ext);
    // the arena of the first part, placed in real memory
    Recorder rec;
    (void)fdb_pixel_bufs(rec, L);
    REQUIRE((long long)rec.used == fdb_pixel_bytes(L));
    long long end = 0;
    for (const auto& s : rec.slots) { REQUIRE(s.first % 256 == 0 && (long long)s.first >= end); end = (long long)(s.first + s.second); }
    REQUIRE(end <= (long long)rec.used);
    const long long bound = fdb_cell_bound(L.px, capacity);
    REQUIRE(bound <= L.px && bound <= capacity && (bound == L.px || bound == capacity));
    Recorder both;
    (void)fdb_pixel_bufs(both, L);
    (void)fdb_cell_bufs(both, (size_t)bound, (size_t)bound + FDB_SLICE_BUDGET);
    REQUIRE((long long)both.used == fdb_group_bytes(L, capacity) && (long long)(both.used - rec.used) == fdb_cell_bytes(bound, bound + FDB_SLICE_BUDGET));
    std::vector<uint8_t> arena(both.used);
    Carver place(arena.data());
    const FdbPixelBufs b = fdb_pixel_bufs(place, L);
    REQUIRE(reinterpret_cast<uintptr_t>(b.tab) % alignof(FdbImage) == 0 && reinterpret_cast<uintptr_t>(b.lab) % alignof(int32_t) == 0);
    std::memset(b.lab, 0, (size_t)px * 4);
    std::memset(b.par, 0, (size_t)px * 4);
    std::memset(b.lsq, 0, (size_t)lsq);
    std::memcpy(b.tab, L.tab.data(), (size_t)n * sizeof(FdbImage));
    b.rid[px - 1] = 1; b.blk[(px + 1023) / 1024 - 1] = 1; b.flist[2 * px - 1] = 1; b.clist[2 * px - 1] = 1;
    b.status[n - 1] = 1; b.plan[2 * n + 1] = 1; b.misc[3] = 1;
    // every block index: its image and its threads' pixels, as fdb_mark_kernel and fdb_fill_unite_kernel walk them (lab counts the visits)
    int img = 0;
    for (unsigned blk = 0; blk < L.blocks; ++blk) {
        while (img + 1 < n && (unsigned)L.tab[(size_t)img + 1].blk0 <= blk) ++img;           // the plain loop
        REQUIRE(fdb_find(b.tab, n, false, blk) == img);
        const FdbImage& t = b.tab[img];
        for (unsigned th = 0; th < 256; ++th) {
            const unsigned p = (blk - (unsigned)t.blk0) * 256u + th;
            if (p >= (unsigned)(t.H * t.W)) continue;
            const int y = (int)p / t.W, x = (int)p - y * t.W;
            REQUIRE(y < t.H && x < t.W);
            b.lab[t.px0 + (int)p] += 1;
            b.lsq[t.lsq0 + (long long)p * t.C + (t.C - 1)] += 1;                            // (the last channel of the pixel: inside the raster)
        }
    }
    // every tile index: its image and its lanes' pixels, as fdb_cell_stats_kernel walks them (par counts the visits)
    img = 0;
    for (unsigned tile = 0; tile < L.tiles; ++tile) {
        while (img + 1 < n && (unsigned)L.tab[(size_t)img + 1].tile0 <= tile) ++img;
        REQUIRE(fdb_find(b.tab, n, true, tile) == img);
        const FdbImage& t = b.tab[img];
        const unsigned local = tile - (unsigned)t.tile0, tiles_x = ((unsigned)t.W + 63u) / 64u;
        REQUIRE(local < fdb_tiles(t.H, t.W));
        const unsigned xb = (local % tiles_x) * 64u;
        const int yb = (int)(local / tiles_x) * FDB_TILE_H;
        REQUIRE(yb < t.H && xb < (unsigned)t.W);                                             // no tile lies wholly outside its image
        for (int y = yb; y < yb + FDB_TILE_H && y < t.H; ++y)
            for (unsigned x = xb; x < xb + 64u && x < (unsigned)t.W; ++x) b.par[(size_t)t.px0 + (size_t)y * t.W + x] += 1;
    }
    for (long long p = 0; p < px; ++p) REQUIRE(b.lab[p] == 1 && b.par[p] == 1);
    for (int i = 0; i < n; ++i) {
        const FdbImage& t = b.tab[i];
        for (long long p = 0; p < (long long)t.H * t.W; ++p) REQUIRE(b.lsq[t.lsq0 + p * t.C + (t.C - 1)] == 1);
    }
    // the second part, for every cell count that may follow: behind the first, inside the measured room
    const long long counts[] = {bound, bound / 2, bound > 0 ? 1 : 0, 17 <= bound ? 17 : bound, 4097 <= bound ? 4097 : bound};
    for (long long cells : counts) {
        if (cells <= 0) continue;
        const long long parts = cells * slices((int)cells);
        REQUIRE(parts <= cells + FDB_SLICE_BUDGET);
        Carver q(arena.data());
        (void)fdb_pixel_bufs(q, L);
        const size_t first = q.used;
        const FdbCellBufs c = fdb_cell_bufs(q, (size_t)cells, (size_t)parts);
        REQUIRE(q.used <= arena.size() && (long long)(q.used - first) == fdb_cell_bytes(cells, parts));
        c.acc[cells * 4 - 1] = 1; c.val[cells - 1] = 1; c.img[cells - 1] = 1; c.off[cells * 2 - 1] = 1; c.cur[cells * 2 - 1] = 1;
        c.rec[cells * 8 - 1] = 1; c.pbest[parts - 1] = 1; c.proots[parts - 1] = 1;
    }
    // the groups under a limit that forces splits: consecutive, complete, within the limit unless alone; each lays out from its first image
    for (long long limit : {FDB_SCRATCH_LIMIT, fdb_group_bytes(L, capacity), fdb_group_bytes(L, capacity) / 2, (long long)1}) {
        const std::vector<FdbGroup> groups = fdb_groups(shapes.data(), n, capacity, limit);
        int at = 0;
        for (const FdbGroup& g : groups) {
            REQUIRE(g.first == at && g.n >= 1);
            FdbLayout G;
            REQUIRE(fdb_layout(shapes.data(), g.first, g.n, G).empty() && G.tab[0].px0 == 0 && G.tab[0].lsq0 == 0 && G.tab[0].tile0 == 0);
            REQUIRE(g.n == 1 || fdb_group_bytes(G, capacity) <= limit);
            if (g.first + g.n < n) {                                                         // ... and the next image would not have fitted
                FdbLayout M;
                REQUIRE(fdb_layout(shapes.data(), g.first, g.n + 1, M).empty() && fdb_group_bytes(M, capacity) > limit);
            }
            at += g.n;
        }
        REQUIRE(at == n);
        if (limit >= fdb_group_bytes(L, capacity)) REQUIRE(groups.size() == 1);
        if (limit == 1) REQUIRE((int)groups.size() == n);
    }
}

static std::string layout_of(const std::vector<int32_t>& shapes) {
    FdbLayout L;
    return fdb_layout(shapes.data(), 0, (int)(shapes.size() / 3), L);
}

int main() {
    std::mt19937 rng(20261);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    const int edges[][2] = {{1, 1}, {1, 300}, {300, 1}, {3, 64}, {65, 63}, {33, 70}, {64, 64}, {96, 130}, {32, 64}, {33, 65}, {1, 256}, {1, 257}, {256, 1}, {31, 63}};
    int chunks = 0;
    for (int round = 0; round < 60; ++round) {
        const int n = round < 9 ? round + 1 : pick(1, 17);
        std::vector<int32_t> shapes;
        for (int i = 0; i < n; ++i) {
            const int e = pick(0, 20);
            const int H = e < 14 ? edges[e][0] : pick(1, 140), W = e < 14 ? edges[e][1] : pick(1, 270);
            shapes.insert(shapes.end(), {H, W, pick(2, 4)});
        }
        for (int capacity : {4096, 0, 7}) check(shapes, capacity);
        std::vector<int32_t> rev;
        for (int i = n - 1; i >= 0; --i) rev.insert(rev.end(), shapes.begin() + 3 * i, shapes.begin() + 3 * i + 3);
        check(rev, 4096);
        chunks += 4;
    }
    // refusals exactly at the limits, naming the image
    REQUIRE(layout_of({5, 6, 3, 0, 6, 3}).rfind("image 1: ", 0) == 0 && layout_of({5, 6, 3, 5, 0, 3}).rfind("image 1: ", 0) == 0);
    REQUIRE(layout_of({5, 6, 3, 5, 6, 1}).rfind("image 1: ", 0) == 0 && layout_of({5, 6, 2}).empty());
    REQUIRE(layout_of({32768, 65535, 2}).empty());                                           // 2^31 - 32768 pixels: the largest one image may hold
    REQUIRE(layout_of({32768, 65536, 2}).rfind("image 0: ", 0) == 0);                        // 2^31 pixels
    REQUIRE(layout_of({32768, 32768, 2, 32768, 32767, 2, 1, 32767, 2}).empty());             // 2^31 - 1 pixels in the chunk
    REQUIRE(layout_of({32768, 32768, 2, 32768, 32767, 2, 1, 32768, 2}).rfind("image 2: ", 0) == 0);   // 2^31
    REQUIRE(layout_of({32768, 32768, 2, 32768, 32768, 2}).rfind("image 1: ", 0) == 0);
    REQUIRE(layout_of({32768, 65535, 511}).empty());                                         // just below 2^40 lsq bytes in one image
    REQUIRE(layout_of({32768, 65535, 513}).rfind("image 0: ", 0) == 0);
    const int32_t rest = 1024 * 1024 * 1024 + 1023 * 32768;                                  // 2^40 - 32768 * 32767 * 1023
    REQUIRE(layout_of({32768, 32767, 1023, 1, 1, rest}).rfind("image 1: ", 0) == 0 && layout_of({32768, 32767, 1023, 1, 1, rest}).find("2^40") != std::string::npos);
    REQUIRE(layout_of({32768, 32767, 1023, 1, 1, rest - 1}).empty());                        // ... and in the chunk
    {
        std::vector<int32_t> many;
        for (int i = 0; i < FDB_MAX_IMAGES; ++i) many.insert(many.end(), {1, 1, 2});
        REQUIRE(layout_of(many).empty());
        FdbLayout L;
        REQUIRE(fdb_layout(many.data(), 0, FDB_MAX_IMAGES, L).empty() && L.tiles == (unsigned)FDB_MAX_IMAGES && L.blocks == (unsigned)FDB_MAX_IMAGES);
        for (unsigned k = 0; k < (unsigned)FDB_MAX_IMAGES; ++k) REQUIRE(fdb_find(L.tab.data(), FDB_MAX_IMAGES, k & 1, k) == (int)k);
        many.insert(many.end(), {1, 1, 2});
        REQUIRE(layout_of(many).find("more than") != std::string::npos);
    }
    std::printf("fishdist_batch_check: ok (%d chunks)\n", chunks);
    return 0;
}
