// test_houghline.cpp — prlib_amd/csrc/houghline.h on the CPU, a program of its own (tests/test_houghline_cpu.py builds it with
// g++ under AddressSanitizer and UndefinedBehaviorSanitizer).
//   test_houghline
//       facts worked out by hand: the geometry, a full row's peak, a rectangle's four lines, three lines, parallel lines
//   test_houghline lines <width> <height> <threshold> <map.raw>
//       the plain C++ transform (hl_vote, hl_peaks) on width x height bytes: prints "cells <n> sum <votes> hash <fnv1a of the
//       accumulator's int32 cells>" and one "line <rho bits> <theta bits>" per line, in order
//   test_houghline quad <width> <height> <n> <lines.raw>
//       hl_quad on n (rho, theta) float32 pairs: prints "found 0|1" and "quad x0 y0 ... x3 y3"
//   test_houghline time <width> <height> <reps> <map.raw>
//       the wall time of hl_vote, one thread: prints "vote_ms <t>" per repeat (tools/bench_houghline.py's yardstick)
#include "../../prlib_amd/csrc/houghline.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace prl_hip;

static int failures = 0;
#define CHECK(cond, what)                                                  \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL: %s (line %d)\n", what, __LINE__);           \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static uint32_t bits_of(float v)
{
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

static bool read_all(const char* path, void* dst, size_t bytes)
{
    FILE* f = std::fopen(path, "rb");
    const bool ok = f && std::fread(dst, 1, bytes, f) == bytes;
    if (f) std::fclose(f);
    return ok;
}

static int selftest()
{
    CHECK(hl_numrho(2480, 3508) == 11977 && hl_numrho(1, 1) == 5 && hl_numrho(32768, 32768) == 131073, "numrho");
    CHECK(hl_accum_cells(1, 1) == (size_t)182 * 7, "accumulator cells");
    float tc[kHlNumAngle], ts[kHlNumAngle];
    hl_trig_table(tc, ts);
    CHECK(tc[0] == 1.f && ts[0] == 0.f && tc[90] != 0.f && std::fabs(tc[90]) < 2e-6f && ts[90] == 1.f, "the table's ends");
    {   // one full row, y = 17, of a 70 x 40 map: 70 votes at theta = 90 steps, rho = 17
        const int W = 70, H = 40, numrho = hl_numrho(W, H);
        std::vector<uint8_t> map((size_t)W * H, 0);
        for (int x = 0; x < W; ++x) map[(size_t)17 * W + x] = 255;
        std::vector<int32_t> acc(hl_accum_cells(W, H));
        hl_vote(map.data(), W, W, H, acc.data());
        long long sum = 0;
        for (int32_t v : acc) sum += v;
        CHECK(sum == 70LL * kHlNumAngle, "every point votes once per angle");
        CHECK(acc[(size_t)(90 + 1) * (numrho + 2) + (17 + (numrho - 1) / 2) + 1] == 70, "the row's cell");
        for (int n = 0; n < kHlNumAngle + 2; ++n) CHECK(acc[(size_t)n * (numrho + 2)] == 0 && acc[(size_t)n * (numrho + 2) + numrho + 1] == 0, "frame columns");
        std::vector<HlPeak> pk;
        hl_peaks(acc.data(), numrho, 50, &pk);
        CHECK(!pk.empty() && pk[0].count == 70, "the first peak");
        float rho, theta;
        hl_line_of(pk[0].cell, numrho, &rho, &theta);
        CHECK(rho == 17.f && theta == 90.f * hl_theta(), "its line");
        for (size_t i = 1; i < pk.size(); ++i)
            CHECK(pk[i - 1].count > pk[i].count || (pk[i - 1].count == pk[i].count && pk[i - 1].cell < pk[i].cell), "the order");
    }
    {   // x = 10, x = 100, y = 20, y = 80 in a 120 x 100 map
        const float half_pi = 90.f * hl_theta();
        const float lines[8] = {10.f, 0.f, 20.f, half_pi, 100.f, 0.f, 80.f, half_pi};
        int32_t q[8] = {0};
        CHECK(hl_quad(lines, 4, 120, 100, q), "a rectangle is found");
        bool seen[4] = {false, false, false, false};
        for (int k = 0; k < 4; ++k)
            for (int c = 0; c < 4; ++c)
                if (q[2 * k] == (c == 0 || c == 3 ? 10 : 100) && q[2 * k + 1] == (c < 2 ? 20 : 80)) seen[c] = true;
        CHECK(seen[0] && seen[1] && seen[2] && seen[3], "its four corners");
        CHECK(!hl_quad(lines, 3, 120, 100, q), "three lines: no quad");
        CHECK(!hl_quad(lines, 4, 90, 100, q), "a corner beyond the width: no quad");
        CHECK(hl_quad(lines, 4, 100, 80, q), "corners on x == width and y == height are kept");
        const float par[8] = {10.f, 0.f, 30.f, 0.f, 50.f, 0.f, 70.f, 0.f};
        CHECK(!hl_quad(par, 4, 120, 100, q), "parallel lines: no quad");
        HlPointF r;
        const HlSegment a = hl_from_vec2f(10.f, 0.f), b = hl_from_vec2f(30.f, 0.f);
        CHECK(a.a.x == 10.f && a.a.y == 1000.f && a.b.x == 10.f && a.b.y == -1000.f, "fromVec2f");
        CHECK(!hl_intersection(a.a, a.b, b.a, b.b, &r), "a zero cross product");
        CHECK(hl_distance_to_line(a.a, a.b, b.a) == 20.0, "distanceToLine");
    }
    if (failures == 0) std::printf("houghline: OK\n");
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "lines" && argc >= 6) {
        const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), threshold = std::atoi(argv[4]), numrho = hl_numrho(W, H);
        std::vector<uint8_t> map((size_t)W * H);
        if (!read_all(argv[5], map.data(), map.size())) return 3;
        std::vector<int32_t> acc(hl_accum_cells(W, H));
        hl_vote(map.data(), (size_t)W, W, H, acc.data());
        long long sum = 0;
        uint32_t hash = 2166136261u;
        for (int32_t v : acc) {
            sum += v;
            for (int k = 0; k < 4; ++k) hash = (hash ^ (((uint32_t)v >> (8 * k)) & 255u)) * 16777619u;
        }
        std::printf("cells %zu sum %lld hash %u\n", acc.size(), sum, hash);
        std::vector<HlPeak> pk;
        hl_peaks(acc.data(), numrho, threshold, &pk);
        for (const HlPeak& p : pk) {
            float rho, theta;
            hl_line_of(p.cell, numrho, &rho, &theta);
            std::printf("line %u %u\n", bits_of(rho), bits_of(theta));
        }
        return 0;
    }
    if (mode == "quad" && argc >= 6) {
        const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), n = std::atoi(argv[4]);
        std::vector<float> lines((size_t)2 * (size_t)n + 1);
        if (n > 0 && !read_all(argv[5], lines.data(), (size_t)n * 8)) return 3;
        int32_t q[8] = {0};
        const bool found = hl_quad(lines.data(), n, W, H, q);
        std::printf("found %d\n", found ? 1 : 0);
        if (found) std::printf("quad %d %d %d %d %d %d %d %d\n", q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]);
        return 0;
    }
    if (mode == "time" && argc >= 6) {
        const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), reps = std::atoi(argv[4]);
        std::vector<uint8_t> map((size_t)W * H);
        if (!read_all(argv[5], map.data(), map.size())) return 3;
        std::vector<int32_t> acc(hl_accum_cells(W, H));
        for (int i = 0; i < reps; ++i) {
            const auto t0 = std::chrono::steady_clock::now();
            hl_vote(map.data(), (size_t)W, W, H, acc.data());
            const auto t1 = std::chrono::steady_clock::now();
            std::printf("vote_ms %.3f\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
        return acc[1] == -1;   // (the accumulator is read)
    }
    return selftest();
}
