// Host program for csrc/iseg_classify.h under ASan + UBSan (`make asan_iseg_classify`; tests/test_iseg_classify.py builds and runs it):
// the per-element function of the ecSeg-c input, compiled for the host from the text the kernel compiles, and the selection and
// chunk planning of ecseg_classify_nucleus_crops.
//
//   iseg_classify_check                 both walks with the checks this program can make on its own; prints "ok"
//   iseg_classify_check values <file>   the float32 bit patterns of iseg_c_value(x, max), 256 x 256 uint32, index max * 256 + x
//   iseg_classify_check plan            one line per case, chunk and model, for the test to hold against its restatement of
//                                       interseg.classify_crops:  n per_group pattern centromeric chunk model | crops.. | run lengths..
//
// Cases: n = 0, 1, 255, 256, 257, 600; per_group = 1, 7, 64; pattern 0 all chosen, 1 none, 2 every other one, 3 the gate (probe
// maxima 10 and 11 in turn, all-zero crops that are no tiles).  The maxima of crop j under a pattern are case_max below.
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../ecseg_amd/csrc/iseg_classify.h"

using namespace ecseg;

static void case_crop(int pattern, int j, int32_t m[3], uint8_t* from_patches) {
    switch (pattern) {
        case 0: m[0] = 20; m[1] = 20 + j % 200; m[2] = 7; *from_patches = (uint8_t)(j % 3 == 0); break;
        case 1: m[0] = m[1] = m[2] = 0; *from_patches = 1; break;
        case 2:
            if (j % 2 == 0) { m[0] = 5; m[1] = 11; m[2] = 0; } else { m[0] = m[1] = m[2] = 0; }
            *from_patches = 1;
            break;
        default:
            m[0] = 0; m[1] = j % 4 == 0 ? 10 : j % 4 == 1 ? 11 : 0; m[2] = 0; *from_patches = 0;
            break;
    }
}

static int fails = 0;
static void expect(bool ok, const char* what, int a, int b, int c) {
    if (!ok) { printf("FAILED %s (%d, %d, %d)\n", what, a, b, c); ++fails; }
}

static void walk_plan(bool print) {
    const int ns[] = {0, 1, 255, 256, 257, 600}, groups[] = {1, 7, 64};
    for (int n : ns)
        for (int per_group : groups)
            for (int pattern = 0; pattern < 4; ++pattern)
                for (int centromeric = 0; centromeric < 2; ++centromeric) {
                    std::vector<int32_t> mx((size_t)n * 3 + 3);
                    std::vector<uint8_t> fp(n + 1), ran_i(n + 1, 9), ran_c(n + 1, 9);
                    for (int j = 0; j < n; ++j) case_crop(pattern, j, &mx[(size_t)j * 3], &fp[j]);
                    int covered = 0;
                    const int chunks = iseg_chunk_count(n);
                    for (int ch = 0; ch < chunks; ++ch) {
                        const int k0 = ch * ISEG_CHUNK, k = iseg_chunk_len(n, ch);
                        expect(k >= 1 && k <= ISEG_CHUNK && k0 + k <= n, "chunk inside the crops", n, ch, k);
                        covered += k;
                        // exactly k entries each: a write beyond the chosen count is ASan's to find
                        std::vector<int32_t> sel_i(k), sel_c(k);
                        int n_i = -1, n_c = -1;
                        iseg_select(&mx[(size_t)k0 * 3], &fp[k0], k, centromeric, sel_i.data(), &n_i, sel_c.data(), &n_c, &ran_i[k0], &ran_c[k0]);
                        expect(n_i >= 0 && n_i <= k && n_c >= 0 && n_c <= n_i, "counts", n, n_i, n_c);
                        const int32_t* sel[2] = {sel_i.data(), sel_c.data()};
                        const int cnt[2] = {n_i, n_c};
                        for (int q = 0; q < 2; ++q) {
                            int seen = 0;
                            for (int j = 0; j < cnt[q]; ++j) {
                                expect(sel[q][j] >= 0 && sel[q][j] < k && (j == 0 || sel[q][j] > sel[q][j - 1]), "ascending indices inside the chunk", n, q, j);
                                expect((q ? ran_c : ran_i)[k0 + sel[q][j]] == 1, "a chosen crop is marked", n, q, j);
                            }
                            for (int j = 0; j < k; ++j) seen += (q ? ran_c : ran_i)[k0 + j];
                            expect(seen == cnt[q], "as many marks as chosen crops", n, q, seen);
                            const int subs = iseg_sub_count(cnt[q], per_group);
                            int total = 0;
                            if (print) {
                                printf("%d %d %d %d %d %c |", n, per_group, pattern, centromeric, ch, q ? 'c' : 'i');
                                for (int j = 0; j < cnt[q]; ++j) printf(" %d", k0 + sel[q][j]);
                                printf(" |");
                            }
                            for (int sb = 0; sb < subs; ++sb) {
                                const int len = iseg_sub_len(cnt[q], per_group, sb);
                                expect(len >= 1 && len <= per_group && (sb == subs - 1 || len == per_group), "run length", n, sb, len);
                                total += len;
                                if (print) printf(" %d", len);
                            }
                            if (print) printf("\n");
                            expect(total == cnt[q], "the runs cover the chosen crops", n, total, cnt[q]);
                        }
                    }
                    expect(covered == n, "the chunks cover the crops", n, covered, chunks);
                    expect(ran_i[n] == 9 && ran_c[n] == 9, "nothing written behind the last crop", n, ran_i[n], ran_c[n]);
                }
}

static std::vector<uint32_t> walk_values() {
    std::vector<uint32_t> bits(256 * 256);
    for (int m = 0; m < 256; ++m)
        for (int x = 0; x < 256; ++x) {
            const float v = iseg_c_value((uint32_t)x, m);
            memcpy(&bits[(size_t)m * 256 + x], &v, 4);
            if (m == 0) expect(x == 0 ? std::isnan(v) : std::isinf(v), "x / 0", x, m, 0);
            else if (x <= m) expect(v >= 0.f && v <= 1.f && (x != m || v == 1.f) && (x != 0 || v == 0.f), "inside [0, 1]", x, m, 0);
        }
    return bits;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "values")) {
        const std::vector<uint32_t> bits = walk_values();
        FILE* f = fopen(argv[2], "wb");
        if (!f || fwrite(bits.data(), 4, bits.size(), f) != bits.size() || fclose(f)) { printf("cannot write %s\n", argv[2]); return 2; }
        return fails ? 1 : 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "plan")) {
        walk_plan(true);
        return fails ? 1 : 0;
    }
    walk_values();
    walk_plan(false);
    if (fails) return 1;
    printf("iseg_classify_check: ok (65536 values, 6 x 3 x 4 x 2 plans)\n");
    return 0;
}
