// Host check of csrc/fish_batch.h, the layout of ecseg_stat_fish_batch, under ASan + UBSan (make asan_fish_batch; CPU only):
// the layout function walked over seeded chunks - mixed extents, C = 3 / 4, mixed K, masks and given labels, with and without the
// mask file and the picture, in call order and reversed, zero-nucleus images (which the layout cannot tell from others: they take
// the same room), and the capacities one short of a chunk's cells - and held to
//   * no overlap: every raster of `work`, every image's share of the typed arrays, every slot of the arena;
//   * alignment: every raster of `work` on 256 bytes, every typed slot on 256 bytes (so on its element size), every image's
//     element offset inside its array;
//   * the byte count: fs_batch_bytes / fs_batch_cell_bytes against what the Carver measures.
// The rasters are then written through the offsets into real memory of exactly that size: a wrong offset is a heap overflow here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>

#include "../../ecseg_amd/csrc/fish_batch.h"

using namespace ecseg;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "fish_batch_check: %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Recorder : Carver {                               // a measuring carver that keeps every slot
    std::vector<std::pair<size_t, size_t>> slots;        // offset, bytes
    uintptr_t take_bytes(size_t bytes) override {
        const size_t off = used;
        const uintptr_t p = Carver::take_bytes(bytes);
        slots.push_back({off, bytes});
        return p;
    }
};

static void no_overlap(std::vector<std::pair<long long, long long>> spans, long long limit) {
    std::sort(spans.begin(), spans.end());
    long long end = 0;
    for (const auto& s : spans) {
        REQUIRE(s.first >= end && s.second >= 0);
        end = s.first + s.second;
    }
    REQUIRE(end <= limit);
}

static void check(const std::vector<FsImageIn>& in, const std::vector<int>& cells) {
    FsBatchLayout L;
    const std::string bad = fs_batch_layout(in, L);
    REQUIRE(bad.empty());
    const size_t n = in.size();
    REQUIRE(L.tab.size() == n);
    // `work`: rasters on 256 bytes, clear of each other, inside the buffer; the encoder's rows name the same rasters in order
    std::vector<std::pair<long long, long long>> spans;
    std::vector<uint8_t> work(L.work ? L.work : 1, 0);
    size_t row = 0, px_sum = 0, w_sum = 0;
    int pads = 0;
    for (size_t i = 0; i < n; ++i) {
        const FsImage& t = L.tab[i];
        const long long px = (long long)t.H * t.W;
        REQUIRE(t.H == in[i].H && t.W == in[i].W && t.C == in[i].C && t.np == t.C - 1 && t.K == in[i].K);
        auto raster = [&](long long off, long long bytes, uint8_t tag) {
            REQUIRE(off >= 0 && off % 256 == 0 && off + bytes <= (long long)L.work);
            spans.push_back({off, bytes});
            std::memset(work.data() + off, tag, (size_t)bytes);           // (ASan: inside the allocation)
        };
        raster(t.img, px * t.C, 1); raster(t.thr, px * t.np, 2); raster(t.bnd, px, 3);
        for (int k = 0; k < FSB_FILES; ++k) {
            const bool has = k < 3 || (k == 3 ? in[i].mask_file : in[i].picture);
            REQUIRE((t.file[k] >= 0) == has);
            if (!has) continue;
            const int spp = k == 3 ? 1 : 3;
            raster(t.file[k], px * spp, (uint8_t)(4 + k));
            REQUIRE(row + 5 <= L.files.size() && L.files[row] == t.file[k] && L.files[row + 1] == t.H && L.files[row + 2] == t.W && L.files[row + 3] == spp);
            row += 5;
        }
        if (in[i].given_labels) {
            REQUIRE(t.msk == -1 && t.pad == -1);
        } else {
            if (in[i].mask_file && in[i].mask_is_file) REQUIRE(t.msk == t.file[3]);
            else raster(t.msk, px, 9);
            REQUIRE(t.pad == (long long)pads * L.Hm * L.Wm && t.H <= L.Hm && t.W <= L.Wm);
            ++pads;
        }
        // the typed arrays: element offsets, the images back to back
        REQUIRE(t.lab == (long long)px_sum && t.w == (long long)w_sum);
        px_sum += (size_t)px; w_sum += (size_t)t.K * t.K;
        REQUIRE(L.max_px >= px && L.max_H >= t.H && L.max_W >= t.W);
    }
    REQUIRE(row == L.files.size() && px_sum == L.px && w_sum == L.w && pads == L.n_pad);
    no_overlap(spans, (long long)L.work);
    // the arena: slots on 256 bytes, clear of each other, and the restated byte counts
    Recorder rec;
    const FsBatchBufs b = fs_batch_bufs(rec, L);
    REQUIRE((long long)rec.used == fs_batch_bytes(L));
    std::vector<std::pair<long long, long long>> slots;
    for (const auto& s : rec.slots) { REQUIRE(s.first % 256 == 0); slots.push_back({(long long)s.first, (long long)s.second}); }
    no_overlap(slots, (long long)rec.used);
    REQUIRE(reinterpret_cast<uintptr_t>(b.lab) % alignof(int32_t) == 0 && reinterpret_cast<uintptr_t>(b.w) % alignof(double) == 0 &&
            reinterpret_cast<uintptr_t>(b.tab) % alignof(FsImage) == 0 && reinterpret_cast<uintptr_t>(b.ptab) % alignof(IsegImage) == 0);
    // ... placed in real memory: the last element of every image's share of every typed array is inside its slot
    std::vector<uint8_t> arena(rec.used);
    Carver place(arena.data());
    const FsBatchBufs q = fs_batch_bufs(place, L);
    for (size_t i = 0; i < n; ++i) {
        const FsImage& t = L.tab[i];
        const size_t px = (size_t)t.H * t.W;
        q.lab[t.lab + px - 1] = 1; q.rid[t.lab + px - 1] = 1;
        q.par[4 * t.lab + 4 * px - 1] = 1; q.sz[4 * t.lab + 4 * px - 1] = 1;
        q.w[t.w + (size_t)t.K * t.K - 1] = 1.0;
        q.mx[4 * i + 3] = 1; q.plan[2 * i + 1] = 1;
        if (t.pad >= 0) { q.pmask[t.pad + (size_t)(t.H - 1) * L.Wm + t.W - 1] = 1; q.plab[t.pad + (size_t)(t.H - 1) * L.Wm + t.W - 1] = 1; }
    }
    q.plan[2 * n + 1] = 1; q.total[3] = 1; q.blk[(L.px + 1023) / 1024 - 1] = 1;
    const std::vector<IsegImage> pt = fs_batch_pad_table(L);
    REQUIRE((int)pt.size() == L.n_pad);
    for (const IsegImage& p : pt) REQUIRE(p.seg_off >= 0 && p.seg_off + (long long)p.h * p.w <= (long long)L.work);
    // the cell-sized buffers, for the chunk's cells and for one fewer (the count-only return keeps them unused, but they must lay out)
    long long total = 0;
    for (int c : cells) total += c;
    for (long long cap : {total, total > 0 ? total - 1 : 0}) {
        Recorder cr;
        (void)fs_batch_cell_bufs(cr, (size_t)cap);
        REQUIRE((long long)cr.used == fs_batch_cell_bytes(cap));
        std::vector<uint8_t> ca(cr.used);
        Carver cp(ca.data());
        const FsBatchCellBufs c = fs_batch_cell_bufs(cp, (size_t)cap);
        if (cap > 0) { c.acc[cap * 12 - 1] = 1; c.cnt[cap * 8 - 1] = 1; c.val[cap - 1] = 1; c.rec[cap * 24 - 1] = 1; }
    }
}

int main() {
    std::mt19937 rng(20260);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    const int Ks[] = {1, 3, 7, 63};
    int chunks = 0;
    for (int round = 0; round < 80; ++round) {
        const int n = round < 8 ? round + 1 : pick(1, 16);
        std::vector<FsImageIn> in((size_t)n);
        std::vector<int> cells((size_t)n);
        for (int i = 0; i < n; ++i) {
            FsImageIn& f = in[(size_t)i];
            const int shape = pick(0, 5);
            f.H = shape == 0 ? 1 : shape == 1 ? 41 : shape == 2 ? 128 : pick(1, 100);
            f.W = shape == 0 ? 1 : shape == 1 ? 43 : shape == 2 ? 127 : pick(1, 130);
            f.C = pick(3, 4); f.K = Ks[pick(0, 3)];
            f.given_labels = pick(0, 2) == 0; f.mask_file = pick(0, 3) != 0; f.mask_is_file = !f.given_labels && pick(0, 1); f.picture = pick(0, 2) == 0;
            cells[(size_t)i] = pick(0, 3) == 0 ? 0 : pick(1, 50);            // a zero-nucleus image beside others
        }
        check(in, cells);
        std::reverse(in.begin(), in.end()); std::reverse(cells.begin(), cells.end());
        check(in, cells);
        chunks += 2;
    }
    // what the layout refuses, and that it names the image
    FsBatchLayout L;
    std::vector<FsImageIn> in(3);
    for (FsImageIn& f : in) { f.H = 5; f.W = 6; f.C = 3; f.K = 3; }
    REQUIRE(fs_batch_layout(in, L).empty());
    struct { int H, W, C, K; } bads[] = {{0, 6, 3, 3}, {5, 0, 3, 3}, {5, 6, 2, 3}, {5, 6, 5, 3}, {5, 6, 3, 2}, {5, 6, 3, 65}, {5, 6, 3, 0}, {65536, 32768, 3, 3}};
    for (const auto& b : bads) {
        std::vector<FsImageIn> bad = in;
        bad[1].H = b.H; bad[1].W = b.W; bad[1].C = b.C; bad[1].K = b.K;
        REQUIRE(fs_batch_layout(bad, L).rfind("image 1: ", 0) == 0);
    }
    std::vector<FsImageIn> many((size_t)FSB_MAX_IMAGES + 1, in[0]);
    REQUIRE(!fs_batch_layout(many, L).empty());
    std::vector<FsImageIn> huge(3, in[0]);
    for (FsImageIn& f : huge) { f.H = 32768; f.W = 32767; }
    REQUIRE(fs_batch_layout(huge, L).find("2^31") != std::string::npos);
    std::printf("fish_batch_check: ok (%d chunks)\n", chunks);
    return 0;
}
