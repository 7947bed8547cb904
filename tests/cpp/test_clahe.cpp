// test_clahe.cpp — clahe.h on the CPU: cv::CLAHE::apply, cv::equalizeHist and one after the other as plain loops; built with
// g++ -ffp-contract=off by tests/test_clahe_cpu.py, and once more with -fsanitize=address,undefined for the `narrow` mode.
//   test_clahe golden <vectors.bin>
//       every record of tests/golden/clahe_vectors.bin (written by tests/clahe_ref.py, whose golden_bytes states the layout in
//       its docstring) bit for bit
//   test_clahe run <rows> <cols> <channels> <tiles_x> <tiles_y> <clip_limit> <clahe 0|1> <equalize 0|1> <step> <page.raw> <out.raw>
//       reads rows * step bytes, writes rows * cols * channels bytes
//   test_clahe self
//       the reflection, the geometry with its quirk, sat_u8, the stepped residual against the literal loop, the weights
//   test_clahe narrow
//       pages of 1 to 9 a side on grids up to 64 x 64 (the pad longer than the side), every channel count, tightly allocated: the
//       run a sanitizer build is made for
#include "../../prlib_amd/csrc/clahe.h"

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

static void enhance(const uint8_t* page, size_t step, int w, int h, int c, int tx, int ty, double clip_limit, bool with_clahe, bool equalize,
                    uint8_t* out, size_t out_step)
{
    const uint8_t* cur = page;
    size_t cur_step = step;
    if (with_clahe) {
        clahe_page(page, step, w, h, c, tx, ty, clip_limit, out, out_step);
        cur = out;
        cur_step = out_step;
    }
    if (equalize) equalize_page(cur, cur_step, w, h, c, out, out_step);
}

static int self_mode()
{
    CHECK(clahe_reflect101(-1, 5) == 1 && clahe_reflect101(5, 5) == 3 && clahe_reflect101(2, 5) == 2, "reflect, n = 5");
    CHECK(clahe_reflect101(7, 3) == 1 && clahe_reflect101(8, 3) == 0 && clahe_reflect101(9, 3) == 1 && clahe_reflect101(10, 3) == 2, "reflect more than once");
    CHECK(clahe_reflect101(2, 2) == 0 && clahe_reflect101(3, 2) == 1 && clahe_reflect101(7, 2) == 1, "reflect, n = 2");
    CHECK(clahe_reflect101(7, 1) == 0 && clahe_reflect101(0, 1) == 0, "a side of 1");
    ClaheGeom g = clahe_geometry(16, 16, 8, 8, 40.0);
    CHECK(g.ext_w == 16 && g.ext_h == 16 && g.tile_w == 2 && g.tile_h == 2 && g.clip == 1, "both sides divide: no extension");
    g = clahe_geometry(16, 13, 8, 8, 40.0);
    CHECK(g.ext_w == 24 && g.ext_h == 16 && g.tile_w == 3 && g.tile_h == 2, "a divisible side grows by a whole `tiles`");
    g = clahe_geometry(1, 1, 8, 8, 0.0);
    CHECK(g.ext_w == 8 && g.ext_h == 8 && g.tile_w == 1 && g.clip == 0 && g.lut_scale == 255.0f, "1 x 1, no clipping");
    g = clahe_geometry(2480, 3508, 8, 8, 2.0);
    CHECK(g.ext_w == 2488 && g.tile_w == 311 && g.tile_h == 439 && g.clip == 1066, "an A4 page: (int)(2 * 136529 / 256)");
    CHECK(clahe_geometry(64, 64, 8, 8, 0.5).clip == 1 && clahe_geometry(64, 64, 8, 8, -3.0).clip == 0, "clip >= 1; a negative limit");
    CHECK(clahe_geometry(64, 64, 8, 8, 1e300).clip == 1 && clahe_geometry(64, 64, 8, 8, INFINITY).clip == 1, "beyond int: INT_MIN, hence 1");
    CHECK(clahe_sat_u8(0.5f) == 0 && clahe_sat_u8(1.5f) == 2 && clahe_sat_u8(2.5f) == 2 && clahe_sat_u8(254.5f) == 254 && clahe_sat_u8(255.5f) == 255 &&
              clahe_sat_u8(-0.5f) == 0 && clahe_sat_u8(300.f) == 255,
          "half to even, clamping");
    // the stepped residual: 300 over the clip in one bin -> batch 1, residual 44, step 5: bins 0, 5, ..., 215 get one more
    int sum = 0;
    for (int i = 0; i < 256; ++i) {
        const int add = clahe_redistributed(i, 300);
        CHECK(add == 1 + (i % 5 == 0 && i < 220 ? 1 : 0), "the stepped rule, bin by bin");
        sum += add;
    }
    CHECK(sum == 300, "the redistribution keeps the total");
    uint8_t a[256], b[256];
    unsigned s = 12345u;
    for (int round = 0; round < 400; ++round) {
        uint32_t h[256];
        int area = 0;
        for (int i = 0; i < 256; ++i) {
            s = s * 1664525u + 1013904223u;
            h[i] = (s >> 24) < (unsigned)(round % 7) * 40u ? 0u : (s >> 12) % (1u + (unsigned)round * 3u);
            area += (int)h[i];
        }
        if (area == 0) continue;
        for (int clip : {0, 1, 2, 3, 17, 255, 256, 1000}) {
            clahe_tile_lut(h, clip, 255.0f / (float)area, a);
            clahe_tile_lut_literal(h, clip, 255.0f / (float)area, b);
            CHECK(std::memcmp(a, b, 256) == 0, "closed form == the literal loop");
            CHECK(a[255] == 255, "a table ends at 255");
        }
    }
    int t1, t2;
    float w, w1;
    clahe_axis(0, 0.5f, 8, &t1, &t2, &w, &w1);
    CHECK(t1 == 0 && t2 == 0 && w == 0.5f && w1 == 0.5f, "x = 0, tile 2: floor(-0.5) = -1, both indices 0");
    clahe_axis(1, 0.5f, 8, &t1, &t2, &w, &w1);
    CHECK(t1 == 0 && t2 == 1 && w == 0.0f && w1 == 1.0f, "x = 1, tile 2");
    clahe_axis(15, 0.5f, 8, &t1, &t2, &w, &w1);
    CHECK(t1 == 7 && t2 == 7 && w == 0.0f, "the last column");
    clahe_axis(5, 1.0f, 8, &t1, &t2, &w, &w1);
    CHECK(t1 == 4 && t2 == 5 && w == 0.5f && w1 == 0.5f, "tile 1: every weight a half");
    CHECK(clahe_blend(1, 2, 1, 2, 0.5f, 0.5f, 0.5f, 0.5f) == 2 && clahe_blend(2, 3, 2, 3, 0.5f, 0.5f, 0.5f, 0.5f) == 2, "ties go to even: 1.5 -> 2, 2.5 -> 2");
    uint32_t e[256] = {0};
    e[9] = 70;
    uint8_t lut[256];
    equalize_lut(e, lut);
    CHECK(lut[9] == 9 && lut[0] == 0 && lut[255] == 255, "one value: the identity");
    e[200] = 1;
    equalize_lut(e, lut);
    CHECK(lut[9] == 0 && lut[199] == 0 && lut[200] == 255 && lut[255] == 255, "all but one pixel in the first bin");
    if (failures == 0) std::printf("clahe self: OK\n");
    return failures ? 1 : 0;
}

static int narrow_mode()
{
    unsigned s = 88172645u;
    for (int C = 1; C <= 4; ++C)
        for (int H : {1, 2, 3, 9})
            for (int W : {1, 2, 5, 9}) {
                std::vector<uint8_t> page((size_t)H * W * C), out((size_t)H * W * C), again((size_t)H * W * C);
                for (auto& v : page) {
                    s = s * 1664525u + 1013904223u;
                    v = (uint8_t)(s >> 24);
                }
                for (int tx : {1, 3, 8, 64})
                    for (int ty : {1, 5, 8, 64})
                        for (double clip : {0.0, 0.5, 40.0}) {
                            enhance(page.data(), (size_t)W * C, W, H, C, tx, ty, clip, true, true, out.data(), (size_t)W * C);
                            again = page;   // in place
                            enhance(again.data(), (size_t)W * C, W, H, C, tx, ty, clip, true, true, again.data(), (size_t)W * C);
                            CHECK(out == again, "in place gives the same bytes");
                        }
            }
    if (failures == 0) std::printf("clahe narrow: OK\n");
    return failures ? 1 : 0;
}

static bool read_file(const char* path, std::vector<uint8_t>& bytes)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    bytes.resize(n > 0 ? (size_t)n : 0);
    const bool ok = std::fread(bytes.data(), 1, bytes.size(), f) == bytes.size();
    std::fclose(f);
    return ok;
}

static int golden_mode(const char* path)
{
    std::vector<uint8_t> file;
    if (!read_file(path, file)) return 3;
    size_t at = 0;
    int records = 0;
    auto i32 = [&]() {
        int32_t v = 0;
        if (at + 4 <= file.size()) std::memcpy(&v, file.data() + at, 4);
        at += 4;
        return (int)v;
    };
    while (at + 4 <= file.size()) {
        const int kind = i32();
        if (kind == 0) break;
        if (kind == 1) {   // a page: h w c tiles_x tiles_y clahe equalize, clip_limit, in, out
            const int h = i32(), w = i32(), c = i32(), tx = i32(), ty = i32(), with_clahe = i32(), eq = i32();
            double clip = 0;
            const size_t n = (size_t)h * w * c;
            if (h < 1 || w < 1 || c < 1 || c > 4 || at + 8 + 2 * n > file.size()) return 4;
            std::memcpy(&clip, file.data() + at, 8);
            at += 8;
            std::vector<uint8_t> out(n);
            enhance(file.data() + at, (size_t)w * c, w, h, c, tx, ty, clip, with_clahe != 0, eq != 0, out.data(), (size_t)w * c);
            if (std::memcmp(out.data(), file.data() + at + n, n) != 0) {
                std::printf("FAIL: record %d (%d x %d x %d, grid %d x %d, clip %g, clahe %d, equalize %d)\n", records, h, w, c, tx, ty, clip, with_clahe, eq);
                ++failures;
            }
            at += 2 * n;
        } else if (kind == 2) {   // a tile: clip area, 256 bins, 256 entries
            const int clip = i32(), area = i32();
            if (area < 1 || at + 1024 + 256 > file.size()) return 4;
            uint32_t hist[256];
            uint8_t lut[256];
            std::memcpy(hist, file.data() + at, 1024);
            clahe_tile_lut(hist, clip, (float)255 / (float)area, lut);
            if (std::memcmp(lut, file.data() + at + 1024, 256) != 0) {
                std::printf("FAIL: record %d (a tile, clip %d, area %d)\n", records, clip, area);
                ++failures;
            }
            at += 1024 + 256;
        } else {
            return 4;
        }
        ++records;
    }
    if (records == 0) return 4;
    if (failures == 0) std::printf("clahe golden: OK (%d records)\n", records);
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "self";
    if (mode == "self") return self_mode();
    if (mode == "narrow") return narrow_mode();
    if (mode == "golden" && argc == 3) return golden_mode(argv[2]);
    if (mode != "run" || argc != 13) return 2;
    const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), cn = std::atoi(argv[4]), tx = std::atoi(argv[5]), ty = std::atoi(argv[6]);
    const double clip = std::atof(argv[7]);
    const bool with_clahe = std::atoi(argv[8]) != 0, eq = std::atoi(argv[9]) != 0;
    const size_t step = (size_t)std::atol(argv[10]);
    std::vector<uint8_t> page;
    if (!read_file(argv[11], page) || page.size() != (size_t)rows * step) return 3;
    std::vector<uint8_t> out((size_t)rows * cols * cn);
    enhance(page.data(), step, cols, rows, cn, tx, ty, clip, with_clahe, eq, out.data(), (size_t)cols * cn);
    FILE* f = std::fopen(argv[12], "wb");
    const bool ok = f && std::fwrite(out.data(), 1, out.size(), f) == out.size();
    if (f) std::fclose(f);
    return ok ? 0 : 5;
}
