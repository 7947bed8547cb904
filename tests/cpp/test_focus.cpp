// test_focus.cpp — focus.h on the CPU: the six sums of a page as the plain loop (focus_sums_page) and the measures from them
// (focus_from_sums); built with g++ -ffp-contract=off by tests/test_focus_cpu.py, which compares the output with tests/focus_ref.py.
//   test_focus <rows> <cols> <channels> <teng_ksize> <step> <page.raw>
//       reads rows * step bytes and prints, per channel, a line "c s0 s1 s2 s3 s4 s5 m0 m1 m2 m3": the sums in decimal, the
//       measures as the 16 hex digits of their float64 bits
//   test_focus self
//       focus_reflect101 and focus_terms on hand-computed cases
#include "../../prlib_amd/csrc/focus.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace prl_hip;

static int failures = 0;
#define CHECK(cond, what)                                                  \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL: %s (line %d)\n", what, __LINE__);           \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static int self_mode()
{
    CHECK(focus_reflect101(-1, 5) == 1 && focus_reflect101(5, 5) == 3 && focus_reflect101(2, 5) == 2, "reflect, n = 5");
    CHECK(focus_reflect101(-1, 2) == 1 && focus_reflect101(2, 2) == 0, "reflect, n = 2");
    CHECK(focus_reflect101(-1, 1) == 0 && focus_reflect101(1, 1) == 0 && focus_reflect101(0, 1) == 0, "reflect, n = 1");
    CHECK(focus_ksize_ok(1) && focus_ksize_ok(3) && !focus_ksize_ok(5) && !focus_ksize_ok(-1) && !focus_ksize_ok(0), "ksize");
    int out[kFocusSums];
    const int peak[3][3] = {{0, 0, 0}, {0, 255, 0}, {0, 0, 0}};
    focus_terms(peak, 3, out);
    CHECK(out[0] == 255 && out[1] == 65025 && out[2] == -1020 && out[3] == 1040400 && out[4] == 2040 && out[5] == 0, "a peak");
    const int edge[3][3] = {{0, 0, 255}, {0, 0, 255}, {0, 0, 255}};
    focus_terms(edge, 3, out);
    CHECK(out[2] == 255 && out[4] == 1020 && out[5] == 1020 * 1020, "a vertical edge, ksize 3");
    focus_terms(edge, 1, out);
    CHECK(out[5] == 255 * 255, "a vertical edge, ksize 1");
    const int corner[3][3] = {{255, 255, 255}, {255, 0, 0}, {255, 0, 0}};
    focus_terms(corner, 3, out);   // gx = -(255 + 510 + 255) + 255 = -765, gy the same
    CHECK(out[5] == 2 * 765 * 765 && out[2] == 510 && out[4] == 2 * 765, "a corner");
    // one pixel of 255 in a 5 x 5 page of zeros
    std::vector<uint8_t> page(25, 0);
    page[12] = 255;
    int64_t s[kFocusSums];
    focus_sums_page(page.data(), 5, 5, 5, 1, 3, s);
    CHECK(s[0] == 255 && s[1] == 65025 && s[2] == 0 && s[3] == 1300500 && s[4] == 8160 && s[5] == 1560600, "the 5 x 5 known answer");
    if (failures == 0) std::printf("focus self: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "self") return self_mode();
    if (argc < 7) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), cn = std::atoi(argv[3]), ks = std::atoi(argv[4]);
    const size_t step = (size_t)std::atol(argv[5]);
    std::vector<uint8_t> page((size_t)rows * step);
    FILE* f = std::fopen(argv[6], "rb");
    if (!f || std::fread(page.data(), 1, page.size(), f) != page.size()) return 3;
    std::fclose(f);
    std::vector<int64_t> sums((size_t)cn * kFocusSums);
    focus_sums_page(page.data(), step, cols, rows, cn, ks, sums.data());
    for (int c = 0; c < cn; ++c) {
        double m[kFocusMeasures];
        focus_from_sums(sums.data() + c * kFocusSums, cols, rows, m);
        std::printf("%d", c);
        for (int k = 0; k < kFocusSums; ++k) std::printf(" %lld", (long long)sums[c * kFocusSums + k]);
        for (int k = 0; k < kFocusMeasures; ++k) {
            unsigned long long bits;
            std::memcpy(&bits, &m[k], 8);
            std::printf(" %016llx", bits);
        }
        std::printf("\n");
    }
    return 0;
}
