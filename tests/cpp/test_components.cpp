// test_components.cpp — rule R and the labelling of prlib_amd/csrc/components.h on the CPU: plain C++, no device, no library.
// tests/test_components_cpu.py builds it with -fsanitize=address,undefined and runs it.  Without an argument it holds rule R
// (cc_external_rects) against the literal scan (ct_external_rects of contour.h) on families it makes itself - every 4 x 4 map,
// every 1 x 12 and 12 x 1 map, random maps raw and dilated, rings - and checks the labels' own properties; with a file of cases
// (maps and the values of tests/components_ref.py, written by the Python test) it holds components.h against those.
#include "../../prlib_amd/csrc/components.h"
#include "../../prlib_amd/csrc/contour.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace prl_hip;

static int failures = 0;
#define CHECK(cond, what)                                                  \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 20) std::printf("FAIL: %s (line %d)\n", what, __LINE__); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Map {
    int w, h;
    std::vector<uint8_t> px;
    Map(int w_, int h_) : w(w_), h(h_), px((size_t)w_ * h_, 0) {}
    uint8_t& at(int x, int y) { return px[(size_t)y * w + x]; }
};

static Map dilated(const Map& m)
{
    Map d(m.w, m.h);
    for (int y = 0; y < m.h; ++y)
        for (int x = 0; x < m.w; ++x)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx, yy = y + dy;
                    if (xx >= 0 && xx < m.w && yy >= 0 && yy < m.h && m.px[(size_t)yy * m.w + xx]) d.at(x, y) = 255;
                }
    return d;
}

static long n_maps = 0;

// rule R against the literal scan, as ordered lists, and the labels' own properties
static void check_map(const Map& m, const char* family)
{
    ++n_maps;
    std::vector<CtRect> want;
    const int want_found = ct_external_rects(m.px.data(), (size_t)m.w, m.w, m.h, &want);
    std::vector<int32_t> got;
    const int found = cc_external_rects(m.px.data(), (size_t)m.w, m.w, m.h, &got);
    bool same = found == want_found && got.size() == 4 * want.size();
    for (size_t i = 0; same && i < want.size(); ++i)
        same = got[4 * i] == want[i].x && got[4 * i + 1] == want[i].y && got[4 * i + 2] == want[i].w && got[4 * i + 3] == want[i].h;
    if (!same && failures < 20) {
        std::printf("%s %d x %d: found %d / %d, kept %zu / %zu\n", family, m.w, m.h, found, want_found, got.size() / 4, want.size());
        for (int y = 0; y < m.h; ++y) {
            for (int x = 0; x < m.w; ++x) std::putchar(m.px[(size_t)y * m.w + x] ? '#' : '.');
            std::putchar('\n');
        }
    }
    CHECK(same, family);
    int k_prev = 0;
    for (int conn = 8; conn >= 4; conn -= 4) {
        std::vector<int32_t> labels;
        std::vector<CcStat> stats;
        const int k = cc_components(m.px.data(), (size_t)m.w, m.w, m.h, conn, &labels, &stats);
        long area = 0, fg = 0;
        int next = 1;   // labels appear in increasing order along the raster
        bool ok = (int)stats.size() == k;
        for (int y = 0; ok && y < m.h; ++y)
            for (int x = 0; x < m.w; ++x) {
                const int l = labels[(size_t)y * m.w + x];
                const bool f = m.px[(size_t)y * m.w + x] != 0;
                fg += f;
                if ((l != 0) != f || l > k || l > next) { ok = false; break; }
                if (l == next) ++next;
                if (l) {
                    const CcStat& s = stats[(size_t)l - 1];
                    if (x < s.left || x >= s.left + s.width || y < s.top || y >= s.top + s.height) { ok = false; break; }
                    if (x + 1 < m.w && m.px[(size_t)y * m.w + x + 1] && labels[(size_t)y * m.w + x + 1] != l) { ok = false; break; }
                    if (y + 1 < m.h && m.px[(size_t)(y + 1) * m.w + x] && labels[(size_t)(y + 1) * m.w + x] != l) { ok = false; break; }
                }
            }
        for (const CcStat& s : stats) area += s.area;
        CHECK(ok && next == k + 1 && area == fg, "labels and statistics agree with the map");
        if (conn == 4) CHECK(k >= k_prev, "4-connected components are pieces of the 8-connected ones");
        k_prev = k;
    }
}

static unsigned rng_state = 12345u;
static unsigned rnd() { return rng_state = rng_state * 1664525u + 1013904223u, rng_state >> 8; }

static void own_families()
{
    for (int bits = 0; bits < 65536; ++bits) {
        Map m(4, 4);
        for (int i = 0; i < 16; ++i) m.px[(size_t)i] = (bits >> i) & 1 ? 255 : 0;
        check_map(m, "4 x 4");
    }
    for (int bits = 0; bits < 4096; ++bits) {
        Map a(12, 1), b(1, 12);
        for (int i = 0; i < 12; ++i) a.px[(size_t)i] = b.px[(size_t)i] = (bits >> i) & 1 ? 255 : 0;
        check_map(a, "1 x 12");
        check_map(b, "12 x 1");
    }
    for (int i = 0; i < 4000; ++i) {
        Map m(1 + (int)(rnd() % 24), 1 + (int)(rnd() % 24));
        const unsigned density = 1 + rnd() % 60;
        for (uint8_t& p : m.px) p = rnd() % 100 < density ? 255 : 0;
        check_map(m, "random");
        Map d = m;
        for (int t = 0; t < 3; ++t) {
            d = dilated(d);
            check_map(d, "random, dilated");
        }
    }
    for (int i = 0; i < 2000; ++i) {   // one-pixel outlines, some with cut corners and a pixel in the hole, nested once
        Map m(3 + (int)(rnd() % 22), 3 + (int)(rnd() % 22));
        const int x0 = (int)(rnd() % 3), y0 = (int)(rnd() % 3), x1 = m.w - 1 - (int)(rnd() % 3), y1 = m.h - 1 - (int)(rnd() % 3);
        if (x1 - x0 < 2 || y1 - y0 < 2) continue;
        for (int x = x0; x <= x1; ++x) m.at(x, y0) = m.at(x, y1) = 255;
        for (int y = y0; y <= y1; ++y) m.at(x0, y) = m.at(x1, y) = 255;
        if (rnd() & 1) m.at(x0, y0) = 0;
        if (rnd() & 1) m.at(x1, y1) = 0;
        if (rnd() & 1) m.at(x1, y0) = 0;
        if (rnd() & 1) m.at((x0 + x1) / 2, (y0 + y1) / 2) = 255;
        if (x1 - x0 >= 6 && y1 - y0 >= 6 && (rnd() & 1)) {
            for (int x = x0 + 2; x <= x1 - 2; ++x) m.at(x, y0 + 2) = m.at(x, y1 - 2) = 255;
            for (int y = y0 + 2; y <= y1 - 2; ++y) m.at(x0 + 2, y) = m.at(x1 - 2, y) = 255;
        }
        check_map(m, "outline");
        check_map(dilated(m), "outline, dilated");
    }
}

static bool read_i32(std::FILE* f, int32_t* v, size_t n = 1) { return std::fread(v, sizeof(int32_t), n, f) == n; }

// the cases of the Python test: w, h, the map, found, kept, the rectangles; then a flag and, if set, for connectivity 8 and 4: K,
// the statistics, the labels
static void file_cases(const char* path)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::printf("cannot open %s\n", path);
        ++failures;
        return;
    }
    int32_t n = 0;
    bool ok = read_i32(f, &n);
    for (int32_t i = 0; ok && i < n; ++i) {
        int32_t wh[2], head[2], flag = 0;
        if (!(ok = read_i32(f, wh, 2) && wh[0] > 0 && wh[1] > 0 && wh[0] <= 4096 && wh[1] <= 4096)) break;
        Map m(wh[0], wh[1]);
        if (!(ok = std::fread(m.px.data(), 1, m.px.size(), f) == m.px.size() && read_i32(f, head, 2) && head[1] >= 0 && head[1] <= wh[0] * wh[1])) break;
        std::vector<int32_t> want((size_t)head[1] * 4), got;
        if (!(ok = (want.empty() || read_i32(f, want.data(), want.size())) && read_i32(f, &flag))) break;
        ++n_maps;
        const int found = cc_external_rects(m.px.data(), (size_t)m.w, m.w, m.h, &got);
        CHECK(found == head[0] && got == want, "rule R equals the restatement");
        for (int conn = 8; flag && conn >= 4; conn -= 4) {
            int32_t k = 0;
            if (!(ok = read_i32(f, &k) && k >= 0 && k <= wh[0] * wh[1])) break;
            std::vector<int32_t> want_stats((size_t)k * 5), want_labels(m.px.size()), labels;
            if (!(ok = (k == 0 || read_i32(f, want_stats.data(), want_stats.size())) && read_i32(f, want_labels.data(), want_labels.size()))) break;
            std::vector<CcStat> stats;
            const int got_k = cc_components(m.px.data(), (size_t)m.w, m.w, m.h, conn, &labels, &stats);
            bool same = got_k == k && labels == want_labels;
            for (int c = 0; same && c < k; ++c) {
                const int32_t* s = &want_stats[(size_t)c * 5];
                const CcStat& t = stats[(size_t)c];
                same = t.left == s[0] && t.top == s[1] && t.width == s[2] && t.height == s[3] && t.area == s[4];
            }
            CHECK(same, "labels and statistics equal the restatement");
        }
    }
    CHECK(ok, "the case file is well formed");
    std::fclose(f);
}

int main(int argc, char** argv)
{
    if (argc > 1) file_cases(argv[1]);
    else own_families();
    CHECK(!cc_kept(1, 1, 1) && !cc_kept(5, 1, 5) && !cc_kept(1, 7, 7) && !cc_kept(4, 4, 4), "straight lines are not kept");
    CHECK(cc_kept(2, 2, 3) && cc_kept(2, 2, 4) && cc_kept(3, 2, 3) && cc_kept(5, 1, 4) == true, "everything else is");
    std::printf("components: %ld maps, %d failures\n", n_maps, failures);
    if (failures) return 1;
    std::printf("components: OK\n");
    return 0;
}
