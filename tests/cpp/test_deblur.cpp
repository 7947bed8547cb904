// test_deblur.cpp — gauss.h on the CPU: the float32 cv::GaussianBlur of an 8-bit page and prl::basicDeblur as plain loops; built
// with g++ -ffp-contract=off by tests/test_deblur_cpu.py, which compares the output with tests/deblur_ref.py bit for bit, and once
// more with -fsanitize=address,undefined for the `narrow` mode.
//   test_deblur blur <rows> <cols> <channels> <kw> <kh> <sigma_x> <sigma_y> <step> <page.raw> <out.raw>
//       reads rows * step bytes, writes rows * cols * channels float32
//   test_deblur deblur <rows> <cols> <channels> <k> <sigma_x> <sigma_y> <weight> <step> <page.raw> <out.raw>
//       writes rows * cols * channels bytes
//   test_deblur weights <n> <sigma>
//       prints the n weights as the 8 hex digits of their float32 bits
//   test_deblur self
//       gauss_reflect101, gauss_plan, gauss_sat_u8 and a 1 x 5 page with n = 3 on hand-computed answers
//   test_deblur narrow
//       pages narrower and shorter than the radius (the border reflects more than once), every channel count, tightly
//       allocated: the run a sanitizer build is made for
#include "../../prlib_amd/csrc/gauss.h"

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
    CHECK(gauss_reflect101(-1, 5) == 1 && gauss_reflect101(5, 5) == 3 && gauss_reflect101(2, 5) == 2, "reflect, n = 5");
    CHECK(gauss_reflect101(-36, 3) == 0 && gauss_reflect101(-35, 3) == 1 && gauss_reflect101(38, 3) == 2 && gauss_reflect101(7, 3) == 1,
          "reflect more than once, n = 3");
    CHECK(gauss_reflect101(-3, 2) == 1 && gauss_reflect101(-2, 2) == 0 && gauss_reflect101(5, 2) == 1, "reflect, n = 2");
    CHECK(gauss_reflect101(-9, 1) == 0 && gauss_reflect101(9, 1) == 0 && gauss_reflect101(0, 1) == 0, "reflect, n = 1");
    GaussPlan p = gauss_plan(0, 0, 9.0, 0.0);
    CHECK(p.nx == 73 && p.ny == 73 && p.shared && p.sx == 9.0 && p.sy == 9.0, "the header default: 73 x 73");
    p = gauss_plan(0, 0, 1.0, 3.0);
    CHECK(p.nx == 9 && p.ny == 25 && !p.shared, "k = 0, sigma 1 and 3: 9 x 25");
    p = gauss_plan(5, 5, 9.0, 0.0);
    CHECK(p.nx == 5 && p.ny == 5 && p.shared && p.sx == 9.0, "5 x 5 with sigma 9");
    p = gauss_plan(0, 0, 0.0, 0.0);
    CHECK(p.nx == 0 && p.ny == 0, "no size and no sigma");
    p = gauss_plan(4, 4, 1.0, 1.0);
    CHECK(p.nx == 0 && p.ny == 0, "an even size");
    p = gauss_plan(3, 0, 0.0, -1.0);
    CHECK(p.nx == 3 && p.ny == 0 && p.sx == 0.0, "one side without a sigma");
    p = gauss_plan(1LL << 32 | 3, 3, 1.0, 1.0);
    CHECK(p.nx == 0 && p.ny == 3, "a size beyond int");
    p = gauss_plan(7, 7, 2.0, 2.0 + 1e-9);
    CHECK(p.nx == 7 && !p.shared, "sigmas that differ");
    CHECK(gauss_sat_u8(0.5f) == 0 && gauss_sat_u8(1.5f) == 2 && gauss_sat_u8(2.5f) == 2 && gauss_sat_u8(254.5f) == 254 && gauss_sat_u8(255.5f) == 255,
          "half to even");
    CHECK(gauss_sat_u8(-0.5f) == 0 && gauss_sat_u8(-300.f) == 0 && gauss_sat_u8(1e9f) == 255 && gauss_sat_u8(3e9f) == 0 && gauss_sat_u8(-3e9f) == 0 &&
              gauss_sat_u8(std::nanf("")) == 0 && gauss_sat_u8(INFINITY) == 0,
          "clamping, and 0 outside int32");
    float w[7];
    gauss_kernel(3, 0.0, w);
    CHECK(w[0] == 0.25f && w[1] == 0.5f && w[2] == 0.25f, "the table for 3");
    gauss_kernel(3, 1.0, w);
    CHECK(w[0] == w[2] && w[1] > 0.5f - 0.06f && w[1] < 0.5f && w[0] != 0.25f, "3 with a sigma: no table");
    gauss_kernel(1, 2.0, w);
    CHECK(w[0] == 1.0f, "n = 1");
    // 1 x 5, n = 3, the table (1/4, 1/2, 1/4): every value exact.  One row: the column pass sees the same row three times.
    const uint8_t page[5] = {10, 20, 30, 40, 250};
    float g[5];
    gauss_kernel(3, 0.0, w);
    gauss_blur_page(page, 5, 5, 1, 1, 3, 3, w, w, g);
    CHECK(g[0] == 15.f && g[1] == 20.f && g[2] == 30.f && g[3] == 90.f && g[4] == 145.f, "1 x 5: the border is 20 | 10 ... 250 | 40");
    uint8_t out[5];
    deblur_page(page, 5, 5, 1, 1, 3, 3, w, w, 0.75, out, 5);   // 1.5 x - 0.5 g = 7.5, 20, 30, 15, 302.5
    CHECK(out[0] == 8 && out[1] == 20 && out[2] == 30 && out[3] == 15 && out[4] == 255, "1 x 5 deblurred, weight 0.75");
    deblur_page(page, 5, 5, 1, 1, 3, 3, w, w, 0.0, out, 5);    // -2 g
    CHECK(out[0] == 0 && out[4] == 0, "weight 0: saturation at 0");
    deblur_page(page, 5, 5, 1, 1, 3, 3, w, w, 0.5, out, 5);    // x + (-1) g
    CHECK(out[0] == 0 && out[1] == 0 && out[2] == 0 && out[3] == 0 && out[4] == 105, "weight 0.5: alpha 1, beta -1");
    // 5 x 1: the same along y
    gauss_blur_page(page, 1, 1, 5, 1, 3, 3, w, w, g);
    CHECK(g[0] == 15.f && g[1] == 20.f && g[2] == 30.f && g[3] == 90.f && g[4] == 145.f, "5 x 1");
    // two interleaved channels: the tap stride is the channel count
    const uint8_t two[10] = {10, 1, 20, 2, 30, 3, 40, 4, 250, 5};
    float g2[10];
    gauss_blur_page(two, 10, 5, 1, 2, 3, 3, w, w, g2);
    CHECK(g2[0] == 15.f && g2[2] == 20.f && g2[8] == 145.f && g2[1] == 1.5f && g2[3] == 2.f && g2[9] == 4.5f, "1 x 5 x 2");
    if (failures == 0) std::printf("deblur self: OK\n");
    return failures ? 1 : 0;
}

static int narrow_mode()
{
    unsigned s = 88172645u;
    for (int C = 1; C <= 4; ++C)
        for (int H : {1, 2, 3, 7})
            for (int W : {1, 2, 3, 7}) {
                std::vector<uint8_t> page((size_t)H * W * C), out((size_t)H * W * C);
                for (auto& v : page) {
                    s = s * 1664525u + 1013904223u;
                    v = (uint8_t)(s >> 24);
                }
                for (int n : {1, 3, 5, 9, 73, kGaussMaxSide}) {
                    std::vector<float> w((size_t)n), wy(9);
                    gauss_kernel(n, n == 73 ? 9.0 : 0.0, w.data());
                    gauss_kernel(9, 1.0, wy.data());
                    deblur_page(page.data(), (size_t)W * C, W, H, C, n, n, w.data(), w.data(), 0.75, out.data(), (size_t)W * C);
                    std::vector<float> g((size_t)H * W * C);
                    gauss_blur_page(page.data(), (size_t)W * C, W, H, C, n, 9, w.data(), wy.data(), g.data());
                    // a convex combination of bytes (the weights sum to 1 within a few ulp)
                    for (float v : g) CHECK(v >= 0.f && v <= 255.01f, "a blurred sample leaves [0, 255]");
                }
            }
    if (failures == 0) std::printf("deblur narrow: OK\n");
    return failures ? 1 : 0;
}

static bool read_page(const char* path, std::vector<uint8_t>& page)
{
    FILE* f = std::fopen(path, "rb");
    const bool ok = f && std::fread(page.data(), 1, page.size(), f) == page.size();
    if (f) std::fclose(f);
    return ok;
}

static bool write_all(const char* path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path, "wb");
    const bool ok = f && std::fwrite(p, 1, bytes, f) == bytes;
    if (f) std::fclose(f);
    return ok;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "self";
    if (mode == "self") return self_mode();
    if (mode == "narrow") return narrow_mode();
    if (mode == "weights" && argc == 4) {
        const int n = std::atoi(argv[2]);
        if (n <= 0 || n % 2 == 0) return 2;
        std::vector<float> w((size_t)n);
        gauss_kernel(n, std::atof(argv[3]), w.data());
        for (float v : w) {
            unsigned bits;
            std::memcpy(&bits, &v, 4);
            std::printf("%08x\n", bits);
        }
        return 0;
    }
    if ((mode != "blur" && mode != "deblur") || argc != 12) return 2;
    const bool fused = mode == "deblur";
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), cn = std::atoi(argv[4]);
    const long long kw = std::atoll(argv[5]), kh = fused ? kw : std::atoll(argv[6]);
    const double sx = std::atof(argv[fused ? 6 : 7]), sy = std::atof(argv[fused ? 7 : 8]), weight = fused ? std::atof(argv[8]) : 0.0;
    const size_t step = (size_t)std::atol(argv[9]);
    std::vector<uint8_t> page((size_t)rows * step);
    if (!read_page(argv[10], page)) return 3;
    const GaussPlan p = gauss_plan(kw, kh, sx, sy);
    if (p.nx == 0 || p.ny == 0) return 4;
    std::vector<float> wx((size_t)p.nx), wy((size_t)p.ny);
    gauss_kernel(p.nx, p.sx, wx.data());
    if (p.shared) wy = wx;
    else gauss_kernel(p.ny, p.sy, wy.data());
    const size_t n = (size_t)rows * cols * cn;
    if (fused) {
        std::vector<uint8_t> out(n);
        deblur_page(page.data(), step, cols, rows, cn, p.nx, p.ny, wx.data(), wy.data(), weight, out.data(), (size_t)cols * cn);
        return write_all(argv[11], out.data(), n) ? 0 : 5;
    }
    std::vector<float> g(n);
    gauss_blur_page(page.data(), step, cols, rows, cn, p.nx, p.ny, wx.data(), wy.data(), g.data());
    return write_all(argv[11], g.data(), n * 4) ? 0 : 5;
}
