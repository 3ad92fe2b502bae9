// Host program for csrc/iseg_batch.h under ASan + UBSan (`make asan_iseg_batch`; tests/test_interseg_batch.py builds and runs it): the
// planning arithmetic of ecseg_interseg_batch, from the text the driver and the kernels compile - the table of a chunk's images, its
// groups, the capacities handed out image by image, the crop windows of a region and the runs of a classifier chunk.
//
//   iseg_batch_check            every walk with the checks this program can make on its own; prints "ok"
//   iseg_batch_check windows    one line per bbox "h w | dy dx th tw ..." for the test to hold against interseg.crop_windows
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../ecseg_amd/csrc/iseg_batch.h"

using namespace ecseg;

static int fails = 0;
static void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
    if (!ok) { printf("FAILED %s (%lld, %lld)\n", what, a, b); ++fails; }
}

// n images of extents from a small cycle, packed with `gap` bytes in front of every raster
static std::vector<int64_t> layout(int n, int gap, long long* bytes) {
    const int ext[4][5] = {{40, 56, 3, 40, 56}, {41, 43, 4, 30, 43}, {300, 280, 3, 300, 280}, {7, 9, 3, 1, 1}};
    std::vector<int64_t> t((size_t)n * ISEG_BATCH_COLS);
    long long off = 0;
    for (int i = 0; i < n; ++i) {
        const int* e = ext[i % 4];
        int64_t* r = &t[(size_t)i * ISEG_BATCH_COLS];
        off += gap + i % 3;
        r[0] = off; r[1] = e[0]; r[2] = e[1]; r[3] = e[2];
        off += (long long)e[0] * e[1] * e[2] + gap;
        r[4] = off; r[5] = e[3]; r[6] = e[4]; r[7] = i % 2;
        off += (long long)e[3] * e[4];
    }
    *bytes = off;
    return t;
}

static void walk_tables() {
    for (int n : {0, 1, 2, 5, 9})
        for (int gap : {0, 1, 7}) {
            long long bytes = 0;
            const std::vector<int64_t> t = layout(n, gap, &bytes);
            std::vector<IsegImage> tab;
            expect(iseg_batch_table(t.data(), n, bytes, tab).empty() && (int)tab.size() == n, "a packed layout is accepted", n, gap);
            if (n) expect(!iseg_batch_table(t.data(), n, bytes - 1, tab).empty(), "the last raster must end inside the buffer", n, gap);
            // every raster's bytes are inside the buffer: read them all from a buffer of exactly that size (ASan's to judge)
            std::vector<uint8_t> buf((size_t)bytes, 1);
            long long sum = 0;
            for (const IsegImage& im : tab) {
                for (long long p = 0; p < (long long)im.H * im.W * im.C; ++p) sum += buf[(size_t)(im.img_off + p)];
                for (long long p = 0; p < (long long)im.h * im.w; ++p) sum += buf[(size_t)(im.seg_off + p)];
            }
            expect(sum <= bytes, "rasters do not overlap", sum, bytes);
            if (n >= 2) {
                std::vector<int64_t> rev = t;                // the rows in reversed order: image 0 now lies behind image 1
                for (int i = 0; i < n; ++i) memcpy(&rev[(size_t)i * ISEG_BATCH_COLS], &t[(size_t)(n - 1 - i) * ISEG_BATCH_COLS], ISEG_BATCH_COLS * sizeof(int64_t));
                expect(!iseg_batch_table(rev.data(), n, bytes, tab).empty(), "rasters in descending order are refused", n, gap);
                std::vector<int64_t> bad = t;
                bad[ISEG_BATCH_COLS] -= gap + 1 + 1;         // image 1 one byte into segmentation 0
                expect(!iseg_batch_table(bad.data(), n, bytes, tab).empty(), "an overlap is refused", n, gap);
            }
            for (int col : {1, 2, 3, 5, 6, 7})
                for (long long v : {-1ll, 0ll, 1ll << 31, 1ll << 62}) {
                    if (!n || (col == 7 && v == 0)) continue;
                    std::vector<int64_t> bad = t;
                    bad[(size_t)(n - 1) * ISEG_BATCH_COLS + col] = v;
                    expect(!iseg_batch_table(bad.data(), n, bytes, tab).empty(), "a bad extent is refused", col, v);
                }
            for (long long v : {-1ll, bytes, 1ll << 62})
                for (int col : {0, 4}) {
                    if (!n) continue;
                    std::vector<int64_t> bad = t;
                    bad[(size_t)(n - 1) * ISEG_BATCH_COLS + col] = v;
                    expect(!iseg_batch_table(bad.data(), n, bytes, tab).empty(), "a bad offset is refused", col, v);
                }
            // groups: consecutive, covering, each within the limit unless it is one image; offsets stay inside the group's span
            iseg_batch_table(t.data(), n, bytes, tab);
            for (long long limit : {0ll, 60ll << 20, ISEG_BATCH_ARENA_LIMIT}) {
                int next = 0;
                for (const IsegGroup& g : iseg_batch_groups(tab, 100, limit)) {
                    expect(g.first == next && g.n >= 1, "groups are consecutive", g.first, next);
                    expect(g.n == 1 || iseg_batch_bytes(g.n, g.Hm, g.Wm, g.span, 100) <= limit, "a group of several images is within the limit", g.n, limit);
                    for (int i = g.first; i < g.first + g.n; ++i) {
                        const IsegImage& im = tab[(size_t)i];
                        expect(im.h <= g.Hm && im.w <= g.Wm && im.img_off >= g.base && im.seg_off + (long long)im.h * im.w <= g.base + g.span, "an image inside its group", i);
                    }
                    next = g.first + g.n;
                }
                expect(next == n, "the groups cover the images", next, n);
                if (limit == 0) expect((int)iseg_batch_groups(tab, 100, limit).size() == n, "no room: one image per group", n);
            }
        }
}

static void walk_capacities() {
    const int needs[6] = {3, 0, 5, 1, 0, 2};                 // zero-nucleus images among them
    for (int cap = 0; cap <= 12; ++cap) {                    // 11 in all: one short and less
        std::vector<int> buf((size_t)cap, -1);               // exactly cap entries: a write beyond is ASan's to find
        int used = 0, placed = 0;
        for (int i = 0; i < 6; ++i) {
            const int before = used, off = iseg_take(needs[i], &used, cap);
            if (off < 0) { expect(used == before && needs[i] > cap - before, "an image that does not fit takes nothing", i, cap); continue; }
            expect(off == before && used == before + needs[i] && used <= cap, "offsets are consecutive", i, cap);
            for (int j = 0; j < needs[i]; ++j) { expect(buf[(size_t)(off + j)] == -1, "no slot given twice", i, j); buf[(size_t)(off + j)] = i; }
            placed += needs[i];
        }
        expect(cap < 11 || placed == 11, "with room for all, all are placed", cap, placed);
        expect(cap != 10 || placed == 9, "one short: only the last image, of 2, is reported", cap, placed);
    }
    int used = 5;
    expect(iseg_take(-1, &used, 10) == -1 && iseg_take(INT32_MAX, &used, 10) == -1 && used == 5, "no overflow in the comparison");
}

static void walk_windows(bool print) {
    const int sizes[] = {1, 2, 255, 256, 257, 300, 511, 512, 513, 530, 600, 1040};
    for (int bh : sizes)
        for (int bw : sizes) {
            const int64_t rec[8] = {100, 10, 20, 10 + bh, 20 + bw, 0, 0, 1275};   // sum / area = 12.75: not below the gate
            std::vector<int32_t> desc;
            std::vector<uint8_t> fp;
            iseg_region_descs(rec, 3, 7, desc, fp);
            const int n = iseg_region_crops(rec);
            expect((int)fp.size() == n && (int)desc.size() == n * ISEG_DESC && n >= 1, "as many descriptors as counted", bh, bw);
            if (print) printf("%d %d |", bh, bw);
            for (int k = 0; k < n; ++k) {
                const int32_t* d = &desc[(size_t)k * ISEG_DESC];
                expect(d[0] == 3 && d[1] == 7 && d[4] >= 1 && d[4] <= 256 && d[5] >= 1 && d[5] <= 256 && d[2] >= 10 && d[3] >= 20 &&
                       d[2] + d[4] <= 10 + bh && d[3] + d[5] <= 20 + bw, "a window inside the bbox", bh, bw);
                expect(fp[(size_t)k] == (bh > 256 || bw > 256), "from_patches", bh, bw);
                if (print) printf(" %d %d %d %d", d[2] - 10, d[3] - 20, d[4], d[5]);
            }
            if (print) printf("\n");
        }
    const int64_t low[8] = {100, 0, 0, 5, 5, 0, 0, 1274};
    expect(iseg_region_crops(low) == 0 && iseg_region_low(low), "below the gate: no crop");
    // runs of one image inside a chunk
    const int imgs[9] = {0, 0, 2, 2, 2, 3, 5, 5, 5};
    std::vector<int32_t> desc(9 * ISEG_DESC, 0);
    for (int k = 0; k < 9; ++k) desc[(size_t)k * ISEG_DESC] = imgs[k];
    for (int from = 0; from < 9; ++from)
        for (int to = from + 1; to <= 9; ++to) {
            int a = from, runs = 0;
            while (a < to) {
                const int e = iseg_run_end(desc.data(), a, to);
                expect(e > a && e <= to, "a run advances and stays inside", a, e);
                for (int k = a; k < e; ++k) expect(imgs[k] == imgs[a], "one image per run", a, k);
                expect(e == to || imgs[e] != imgs[a], "a run is maximal", a, e);
                a = e; ++runs;
            }
            expect(runs >= 1, "runs", from, to);
        }
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "windows")) {
        walk_windows(true);
        return fails ? 1 : 0;
    }
    walk_tables();
    walk_capacities();
    walk_windows(false);
    if (fails) return 1;
    printf("iseg_batch_check: ok\n");
    return 0;
}
