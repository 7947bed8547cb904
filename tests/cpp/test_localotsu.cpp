// test_localotsu.cpp — gauss8.h (the 8.8 weights of the 8-bit cv::GaussianBlur and the separable integer filter as plain loops) and
// the external-rectangle scanner of contour.h on the CPU: a program of its own, built by tests/test_localotsu_cpu.py with
// -fsanitize=address,undefined.  Known answers from include/prl_hip.h; the comparison with the numpy restatement is the Python
// tests' part.
#include "../../prlib_amd/csrc/contour.h"
#include "../../prlib_amd/csrc/gauss8.h"

#include <cstdio>
#include <cstring>
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

static bool weights_are(int n, std::vector<int> want)
{
    std::vector<uint16_t> w((size_t)n);
    gauss8_kernel(n, 0.0, w.data());
    for (int i = 0; i < n; ++i)
        if (w[(size_t)i] != want[(size_t)i]) return false;
    return true;
}

static void test_weights()
{
    CHECK(weights_are(1, {256}), "n = 1");
    CHECK(weights_are(3, {64, 128, 64}), "n = 3");
    CHECK(weights_are(5, {16, 64, 96, 64, 16}), "n = 5");
    CHECK(weights_are(7, {8, 28, 56, 72, 56, 28, 8}), "n = 7");
    CHECK(weights_are(9, {4, 13, 30, 51, 60, 51, 30, 13, 4}), "n = 9");
    CHECK(weights_are(19, {1, 1, 3, 5, 10, 15, 20, 27, 30, 32, 30, 27, 20, 15, 10, 5, 3, 1, 1}), "n = 19");
    double worst = 0.5;
    for (int n = 1; n <= kGaussMaxSide; n += 2)
        for (double sigma : {0.0, 0.1, 0.7, 3.0, 100.0}) {
            uint16_t w[kGaussMaxSide];
            double margin;
            gauss8_kernel(n, sigma, w, &margin);
            int sum = 0;
            for (int i = 0; i < n; ++i) sum += w[i];
            CHECK(sum == 256, "a side sums to 256");
            CHECK(w[n / 2] <= 256, "the centre is not negative");
            for (int i = 0; i < n; ++i) CHECK(w[i] == w[n - 1 - i], "symmetric");
            if (margin < worst) worst = margin;
        }
    CHECK(worst > 1e-9, "no adj near a rounding tie");
    uint16_t w25[25];
    gauss8_kernel(25, 0.0, w25);
    CHECK(w25[11] == 25 && w25[12] == 24 && w25[13] == 25, "n = 25: the centre is not the largest weight");
}

static std::vector<uint8_t> noise(size_t n, unsigned seed)
{
    std::vector<uint8_t> v(n);
    unsigned s = seed;
    for (size_t i = 0; i < n; ++i) {
        s = s * 1664525u + 1013904223u;
        v[i] = (uint8_t)(s >> 24);
    }
    return v;
}

static void test_filter()
{
    uint16_t w[kGaussMaxSide], w3[3];
    {   // a constant page blurs to itself; all 255 with the largest side stays 255
        for (int v : {0, 1, 77, 255}) {
            std::vector<uint8_t> src(9 * 11, (uint8_t)v), dst(9 * 11, 7);
            gauss8_kernel(19, 0.0, w);
            sep_filter_u8_page(src.data(), 11, 11, 9, 1, w, 19, w, 19, dst.data(), 11);
            CHECK(dst == src, "a constant page");
        }
        std::vector<uint8_t> src(5 * 6, 255), dst(5 * 6, 0);
        gauss8_kernel(255, 0.0, w);
        sep_filter_u8_page(src.data(), 6, 6, 5, 1, w, 255, w, 255, dst.data(), 6);
        CHECK(dst == src, "all 255 with n = 255");
    }
    {   // 5 x 7, two channels, pitched rows: the separable form equals the direct double sum; bytes outside the rows stay
        const int W = 5, H = 7, C = 2;
        const size_t step = W * C + 3, dstep = W * C + 5;
        std::vector<uint8_t> src = noise(step * H, 5), dst(dstep * H, 0xA5);
        gauss8_kernel(5, 0.0, w);
        gauss8_kernel(3, 0.0, w3);
        sep_filter_u8_page(src.data(), step, W, H, C, w, 5, w3, 3, dst.data(), dstep);
        bool same = true, outside = true;
        for (int y = 0; y < H; ++y) {
            for (int x = 0; x < W; ++x)
                for (int c = 0; c < C; ++c) {
                    unsigned a = 32768;
                    for (int j = 0; j < 3; ++j)
                        for (int i = 0; i < 5; ++i)
                            a += (unsigned)w3[j] * w[i] * src[(size_t)gauss_reflect101(y + j - 1, H) * step + (size_t)gauss_reflect101(x + i - 2, W) * C + c];
                    same = same && dst[(size_t)y * dstep + (size_t)x * C + c] == (uint8_t)(a >> 16);
                }
            for (size_t k = W * C; k < dstep; ++k) outside = outside && dst[(size_t)y * dstep + k] == 0xA5;
        }
        CHECK(same, "separable == direct");
        CHECK(outside, "nothing outside the rows is written");
    }
    {   // thin pages and a side far wider than the page: the reflection folds more than once
        gauss8_kernel(255, 0.0, w);
        for (int W : {1, 2, 5})
            for (int H : {1, 3}) {
                std::vector<uint8_t> src = noise((size_t)W * H * 3, 9), dst((size_t)W * H * 3);
                sep_filter_u8_page(src.data(), (size_t)W * 3, W, H, 3, w, 255, w, 255, dst.data(), (size_t)W * 3);
                if (W == 1 && H == 1) CHECK(dst == src, "a 1 x 1 page is its own blur");
            }
        const uint16_t one[1] = {256};
        std::vector<uint8_t> src = noise(6 * 4, 11), dst(6 * 4);
        sep_filter_u8_page(src.data(), 6, 6, 4, 1, one, 1, one, 1, dst.data(), 6);
        CHECK(dst == src, "a 1 x 1 kernel copies");
    }
}

static std::vector<CtRect> rects_of(const std::vector<std::vector<int>>& rows, int* found, size_t pad = 0)
{
    const int h = (int)rows.size(), w = (int)rows[0].size();
    const size_t step = (size_t)w + pad;
    std::vector<uint8_t> map(step * h, 0);   // (the padding is background: never read)
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) map[(size_t)y * step + x] = rows[(size_t)y][(size_t)x] ? 255 : 0;
    std::vector<CtRect> r;
    *found = ct_external_rects(map.data(), step, w, h, &r);
    for (const CtRect& q : r) CHECK(q.x >= 0 && q.y >= 0 && q.w >= 1 && q.h >= 1 && q.x + q.w <= w && q.y + q.h <= h, "a rectangle on the page");
    return r;
}

static void test_rects()
{
    int found;
    std::vector<CtRect> r = rects_of({{0, 0, 0}, {0, 0, 0}}, &found);
    CHECK(found == 0 && r.empty(), "an empty map");
    r = rects_of({{1}}, &found);
    CHECK(found == 1 && r.empty(), "1 x 1: one contour of one point, dropped");
    r = rects_of({{0, 0, 0}, {0, 1, 0}, {0, 0, 0}}, &found);
    CHECK(found == 1 && r.empty(), "one pixel");
    r = rects_of({{0, 0, 0, 0}, {0, 1, 1, 0}, {0, 0, 0, 0}}, &found, 3);
    CHECK(found == 1 && r.empty(), "a two-pixel line has two points");
    r = rects_of({{1, 1, 1}, {1, 1, 1}}, &found);
    CHECK(found == 1 && r.size() == 1 && r[0].x == 0 && r[0].y == 0 && r[0].w == 3 && r[0].h == 2, "a full page");
    r = rects_of({{1, 1, 1, 1, 1, 1, 1, 0},
                  {1, 1, 1, 1, 1, 1, 1, 0},
                  {1, 1, 0, 0, 0, 1, 1, 0},
                  {1, 1, 0, 1, 0, 1, 1, 0},
                  {1, 1, 0, 0, 0, 1, 1, 0},
                  {1, 1, 1, 1, 1, 1, 1, 0},
                  {1, 1, 1, 1, 1, 1, 1, 1}}, &found);
    CHECK(found == 1 && r.size() == 1 && r[0].w == 8 && r[0].h == 7, "a thick ring: the blob in its hole is not external");
    r = rects_of({{1, 1, 0, 1, 1}, {1, 1, 0, 1, 1}, {0, 0, 0, 0, 0}, {1, 1, 0, 1, 1}, {1, 1, 0, 1, 1}}, &found);
    CHECK(found == 4 && r.size() == 4, "a block in each corner");
    std::vector<std::vector<int>> checker(9, std::vector<int>(11));
    for (int y = 0; y < 9; ++y)
        for (int x = 0; x < 11; ++x) checker[(size_t)y][(size_t)x] = (x + y) & 1;
    r = rects_of(checker, &found);
    CHECK(found == 1 && r.size() == 1 && r[0].w == 11 && r[0].h == 9, "a checkerboard is one 8-connected component");
    r = rects_of({{1, 0, 1, 1, 1, 0, 1}}, &found);
    CHECK(found == 3 && r.size() == 0, "1 x N: runs are contours of one or two points");
    unsigned s = 12345;
    for (int it = 0; it < 200; ++it) {   // random maps: memory safety, and the counts agree
        s = s * 1664525u + 1013904223u;
        const int w = 1 + (int)((s >> 8) % 40), h = 1 + (int)((s >> 20) % 40);
        std::vector<std::vector<int>> m((size_t)h, std::vector<int>((size_t)w));
        const unsigned density = 26 + (unsigned)(it % 9) * 25;
        for (auto& row : m)
            for (int& v : row) {
                s = s * 1664525u + 1013904223u;
                v = (s >> 24) < density;
            }
        r = rects_of(m, &found, (size_t)(it % 3));
        CHECK((int)r.size() <= found, "kept <= found");
    }
}

int main()
{
    test_weights();
    test_filter();
    test_rects();
    if (failures == 0) std::printf("localotsu: OK\n");
    return failures ? 1 : 0;
}
