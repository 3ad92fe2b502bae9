// Host check of csrc/mincut_regions.h, the layout of ecseg_min_cut_regions, under ASan + UBSan (make asan_min_cut_regions; CPU only):
// the plan walked over seeded lists of labels (areas and boxes), zero regions and single labels, and held to
//   * the selection: np.median restated with nth_element, strictly greater, ascending labels;
//   * the windows: back to back in selection order, their total, the refusals above ECSEG_MIN_CUT_MAX_PIXELS / _MAX_BYTES;
//   * the centre records: first index = sum of the counts in front, accumulator slots = prefix of mcr_center_bound;
//   * the capacity rule with each of the three capacities one short;
//   * the arena: every slot clear of the others, and every region's window, components, accumulators and records written through
//     the offsets into real memory of exactly the measured size: a wrong offset is a heap overflow here;
//   * the small rules the kernels share: the odd stride's bank spread, mcr_in_lds against the LDS cells, FAR + 1 = FAR, and the
//     half-to-even centroid against a brute-force statement.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <utility>

#include "../../ecseg_amd/csrc/mincut_regions.h"

using namespace ecseg;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "min_cut_regions_check: %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Recorder : Carver {                               // a placing carver that keeps every slot
    explicit Recorder(void* base) : Carver(base) {}
    std::vector<std::pair<size_t, size_t>> slots;        // offset, bytes
    uintptr_t take_bytes(size_t bytes) override {
        const size_t off = used;
        const uintptr_t p = Carver::take_bytes(bytes);
        slots.push_back({off, bytes});
        return p;
    }
};

static double median_nth(std::vector<int32_t> v) {
    const size_t n = v.size();
    std::nth_element(v.begin(), v.begin() + n / 2, v.end());
    const double hi = v[n / 2];
    if (n & 1) return hi;
    return ((double)*std::max_element(v.begin(), v.begin() + n / 2) + hi) / 2.0;
}

static void check(const std::vector<int32_t>& stats, double coeff, int lds_pixels, std::mt19937& rng) {
    const int n = (int)(stats.size() / 5);
    McrPlan P;
    REQUIRE(mcr_plan(stats.data(), n, coeff, lds_pixels, P).empty());
    REQUIRE(P.regions.size() == (size_t)P.n_regions * MCR_REC);
    // the selection and the windows
    long long at = 0;
    int sel = 0, lds = 0;
    if (n > 0) {
        std::vector<int32_t> areas;
        for (int k = 0; k < n; ++k) areas.push_back(stats[5 * (size_t)k]);
        const double med = median_nth(areas);
        REQUIRE(med == mcr_median(areas.data(), n));
        for (int k = 0; k < n; ++k) {
            if (!((double)areas[(size_t)k] > coeff * med)) continue;
            REQUIRE(sel < P.n_regions);
            const int32_t* r = &P.regions[(size_t)sel * MCR_REC];
            const int32_t* q = &stats[5 * (size_t)k];
            REQUIRE(r[0] == k + 1 && r[1] == q[1] && r[2] == q[3] && r[3] == q[2] - q[1] + 1 && r[4] == q[4] - q[3] + 1 && r[5] == at);
            at += (long long)r[3] * r[4];
            lds += mcr_in_lds(r[3], r[4], lds_pixels);
            ++sel;
        }
    }
    REQUIRE(sel == P.n_regions && at == P.window_pixels && lds == P.n_lds);
    // counts within the bound, first records, slots
    std::vector<int32_t> counts((size_t)P.n_regions), slot((size_t)P.n_regions);
    size_t slots = 0;
    for (int i = 0; i < P.n_regions; ++i) {
        const int bound = mcr_center_bound(P.regions[(size_t)i * MCR_REC + 3], P.regions[(size_t)i * MCR_REC + 4]);
        counts[(size_t)i] = bound ? (int32_t)(rng() % (unsigned)(bound + 1)) : 0;
        slot[(size_t)i] = (int32_t)slots;
        slots += (size_t)bound;
    }
    const long long nc = mcr_place_centers(P, counts.data());
    long long sum = 0;
    for (int i = 0; i < P.n_regions; ++i) {
        REQUIRE(P.regions[(size_t)i * MCR_REC + 6] == sum && P.regions[(size_t)i * MCR_REC + 7] == counts[(size_t)i]);
        sum += counts[(size_t)i];
    }
    REQUIRE(nc == sum && nc <= (long long)slots);
    // the capacity rule
    REQUIRE(mcr_fits(P.n_regions, nc, P.window_pixels, P.n_regions, (int)nc, P.window_pixels));
    if (P.n_regions > 0) REQUIRE(!mcr_fits(P.n_regions, nc, P.window_pixels, P.n_regions - 1, (int)nc, P.window_pixels));
    if (nc > 0) REQUIRE(!mcr_fits(P.n_regions, nc, P.window_pixels, P.n_regions, (int)nc - 1, P.window_pixels));
    if (P.window_pixels > 0) REQUIRE(!mcr_fits(P.n_regions, nc, P.window_pixels, P.n_regions, (int)nc, P.window_pixels - 1));
    // the arena: measured, then placed in memory of exactly that size and written through
    Carver measure;
    (void)mcr_region_bufs(measure, P.n_regions, (size_t)P.window_pixels, slots);
    std::vector<uint8_t> arena(measure.used);
    Recorder place(arena.data());
    const McrRegionBufs b = mcr_region_bufs(place, P.n_regions, (size_t)P.window_pixels, slots);
    REQUIRE(place.used == measure.used);
    size_t end = 0;
    for (const auto& s : place.slots) {
        REQUIRE(s.first >= end && s.first % 256 == 0);
        end = s.first + s.second;
    }
    REQUIRE(end <= arena.size());
    if (P.n_regions > 0) std::memcpy(b.regions, P.regions.data(), P.regions.size() * sizeof(int32_t));
    *b.total = (int32_t)nc;
    for (int i = 0; i < P.n_regions; ++i) {
        const int32_t* r = &P.regions[(size_t)i * MCR_REC];
        const size_t px = (size_t)r[3] * r[4];
        b.counts[i] = r[7]; b.first[i] = r[6]; b.slot[i] = slot[(size_t)i];
        std::memset(b.windows + r[5], 1, px);
        for (size_t p = 0; p < px; ++p) b.comp[(size_t)r[5] + p] = (int32_t)p;
        for (int j = 0; j < r[7]; ++j) {
            unsigned long long* a = b.acc + 3 * ((size_t)slot[(size_t)i] + j);
            a[0] = a[1] = a[2] = 1;
            int32_t* c = b.centers + MCR_REC * ((size_t)r[6] + j);
            for (int f = 0; f < MCR_REC; ++f) c[f] = i;
        }
    }
}

static int32_t between(std::mt19937& rng, int lo, int hi) { return lo + (int32_t)(rng() % (unsigned)(hi - lo + 1)); }

int main() {
    std::mt19937 rng(20240611);
    int scenes = 0;
    for (int round = 0; round < 400; ++round) {              // random label lists
        const int n = round < 4 ? round : between(rng, 1, 60);
        std::vector<int32_t> stats;
        for (int k = 0; k < n; ++k) {
            const int32_t r0 = between(rng, 0, 900), c0 = between(rng, 0, 900), h = between(rng, 1, round % 7 == 0 ? 400 : 90),
                          w = between(rng, 1, round % 7 == 0 ? 400 : 90);
            const int32_t row[5] = {between(rng, 1, h * w), r0, r0 + h - 1, c0, c0 + w - 1};
            stats.insert(stats.end(), row, row + 5);
        }
        const double coeffs[4] = {0.0, 0.5, 1.25, 1e9};      // everything, most, some, nothing (zero regions)
        check(stats, coeffs[round % 4], round % 3 == 0 ? 0 : MCR_LDS_PIXELS, rng);
        ++scenes;
    }
    {   // the issue's selection cases
        McrPlan P;
        const int32_t a[15] = {4, 0, 1, 0, 1, 4, 0, 1, 4, 5, 5, 3, 4, 8, 10};
        REQUIRE(mcr_plan(a, 3, 1.25, MCR_LDS_PIXELS, P).empty() && P.n_regions == 0);            // 5 > 5.0 is false
        int32_t b[15];
        std::memcpy(b, a, sizeof(a));
        b[10] = 6;
        REQUIRE(mcr_plan(b, 3, 1.25, MCR_LDS_PIXELS, P).empty() && P.n_regions == 1 && P.regions[0] == 3 && P.window_pixels == 6);
        const int32_t one[5] = {36, 1, 6, 1, 6};
        REQUIRE(mcr_plan(one, 1, 1.25, MCR_LDS_PIXELS, P).empty() && P.n_regions == 0);
        REQUIRE(mcr_plan(one, 1, 0.5, MCR_LDS_PIXELS, P).empty() && P.n_regions == 1);
        REQUIRE(mcr_plan(one, 0, 0.5, MCR_LDS_PIXELS, P).empty() && P.n_regions == 0 && P.window_pixels == 0);
        const int32_t even[20] = {4, 0, 1, 0, 1, 4, 0, 1, 4, 5, 6, 3, 4, 8, 10, 10, 6, 7, 0, 4};  // median (4 + 6) / 2 = 5: bound 6.25
        REQUIRE(mcr_plan(even, 4, 1.25, MCR_LDS_PIXELS, P).empty() && P.n_regions == 1 && P.regions[0] == 4);
        const int32_t huge[5] = {5000000, 0, 2048, 0, 2048};                                   // 2049 x 2049 > ECSEG_MIN_CUT_MAX_PIXELS
        const std::string bad = mcr_plan(huge, 1, 0.5, MCR_LDS_PIXELS, P);
        REQUIRE(bad.find("label 1") != std::string::npos);
    }
    for (int w = 1; w <= 300; ++w) {                         // the odd stride spreads 64 consecutive rows over the 64 banks
        const int st = mcr_stride(w);
        REQUIRE(st >= w && st <= w + 1 && (st & 1));
        std::set<int> banks;
        for (int r = 0; r < 64; ++r) banks.insert((r * st) % 64);
        REQUIRE(banks.size() == 64);
        for (int h = 1; h <= 300; h += 7)
            if (mcr_in_lds(h, w, MCR_LDS_PIXELS)) REQUIRE((long long)h * st <= MCR_LDS_CELLS && h * w <= MCR_LDS_PIXELS);
        REQUIRE(!mcr_in_lds(1, w, 0));
    }
    REQUIRE(mcr_sat_inc(MCR_FAR) == MCR_FAR && mcr_sat_inc(MCR_FAR - 1) == MCR_FAR && mcr_sat_inc(0) == 1);
    for (long long n = 1; n <= 40; ++n)                      // half to even against its definition on exact halves and everything else
        for (long long S = 0; S <= 40 * n; ++S) {
            const long long twice = 2 * S;                   // mean = twice / (2 n)
            long long want = twice / (2 * n);                // floor
            const long long rem = twice % (2 * n);
            if (rem > n || (rem == n && (want & 1))) ++want;
            REQUIRE(mcr_round_mean(S, n) == want);
        }
    REQUIRE(mcr_round_mean(3ll << 40, 1ll << 21) == (3 << 19) && mcr_center_bound(2, 9) == 0 && mcr_center_bound(3, 3) == 1 && mcr_center_bound(6, 7) == 6);
    std::printf("min_cut_regions_check: ok (%d label lists)\n", scenes);
    return 0;
}
