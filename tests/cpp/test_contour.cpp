// test_contour.cpp — the quad search of prl::documentContour (prlib_amd/csrc/contour.h) on hand-made maps, on the CPU: plain C++,
// no device, no library.  tests/test_contour_cpu.py builds it with -fsanitize=address,undefined and runs it: every index the
// border follower, the polygon approximation and the ordering touch is then checked.
#include "../../prlib_amd/csrc/contour.h"

#include <cstdio>
#include <cstdlib>
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

struct Map {
    int w, h;
    std::vector<uint8_t> px;
    Map(int w_, int h_, uint8_t v = 0) : w(w_), h(h_), px((size_t)w_ * h_, v) {}
    void set(int x, int y)
    {
        if (x >= 0 && x < w && y >= 0 && y < h) px[(size_t)y * w + x] = 255;
    }
    void line(int x0, int y0, int x1, int y1)   // Bresenham
    {
        const int dx = std::abs(x1 - x0), dy = -std::abs(y1 - y0), sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
        int err = dx + dy;
        for (;;) {
            set(x0, y0);
            if (x0 == x1 && y0 == y1) return;
            const int e2 = 2 * err;
            if (e2 >= dy) { err += dy; x0 += sx; }
            if (e2 <= dx) { err += dx; y0 += sy; }
        }
    }
    void outline(const int (*c)[2], int n)
    {
        for (int i = 0; i < n; ++i) line(c[i][0], c[i][1], c[(i + 1) % n][0], c[(i + 1) % n][1]);
    }
    void fill_rect(int x0, int y0, int x1, int y1)
    {
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) set(x, y);
    }
};

// every border point is a foreground pixel of the page, every approximation keeps points of its input only; returns the answer
static bool run(const Map& m, CtPoint quad[4], int* n_outer = nullptr, int* n_hole = nullptr)
{
    std::vector<CtPoint> pts;
    std::vector<CtContour> cs;
    ct_find_contours(m.px.data(), (size_t)m.w, m.w, m.h, &pts, &cs);
    int outer = 0, hole = 0;
    for (const CtContour& c : cs) {
        (c.hole ? hole : outer)++;
        CHECK(c.count >= 1, "a border has a point");
        for (int i = 0; i < c.count; ++i) {
            const CtPoint p = pts[(size_t)(c.first + i)];
            CHECK(p.x >= 0 && p.x < m.w && p.y >= 0 && p.y < m.h && m.px[(size_t)p.y * m.w + p.x] != 0, "border point on the foreground");
        }
        std::vector<CtPoint> cur(pts.begin() + c.first, pts.begin() + c.first + c.count), out(cur.size());
        for (double eps = 0.0; eps < 6.0; eps += 1.0) {
            const int k = ct_approx_closed(cur.data(), (int)cur.size(), eps, out.data());
            CHECK(k >= 1 && k <= (int)cur.size(), "approximation size");
            for (int i = 0; i < k; ++i) {
                bool in = false;
                for (const CtPoint& q : cur) in = in || (q.x == out[(size_t)i].x && q.y == out[(size_t)i].y);
                CHECK(in, "approximation keeps input points");
            }
        }
    }
    if (n_outer) *n_outer = outer;
    if (n_hole) *n_hole = hole;
    return ct_document_quad(m.px.data(), (size_t)m.w, m.w, m.h, quad);
}

static bool same_cycle(const CtPoint q[4], const int (*want)[2])
{
    for (int s = 0; s < 4; ++s) {
        bool fwd = true, bwd = true;
        for (int i = 0; i < 4; ++i) {
            fwd = fwd && q[i].x == want[(s + i) & 3][0] && q[i].y == want[(s + i) & 3][1];
            bwd = bwd && q[i].x == want[(s - i) & 3][0] && q[i].y == want[(s - i) & 3][1];
        }
        if (fwd || bwd) return true;
    }
    return false;
}

int main()
{
    CtPoint q[4];
    int outer = 0, hole = 0;
    const int rect[4][2] = {{8, 6}, {30, 6}, {30, 22}, {8, 22}};
    {
        Map m(40, 30);
        m.fill_rect(8, 6, 30, 22);
        CHECK(run(m, q, &outer, &hole) && same_cycle(q, rect), "filled rectangle");
        CHECK(outer == 1 && hole == 0, "filled rectangle: one outer border");
    }
    {
        Map m(40, 30);
        m.outline(rect, 4);
        CHECK(run(m, q, &outer, &hole) && same_cycle(q, rect), "one-pixel outline");
        CHECK(outer == 1 && hole == 1, "one-pixel outline: an outer and a hole border");
        float out[8];
        const int32_t quad[8] = {q[0].x, q[0].y, q[1].x, q[1].y, q[2].x, q[2].y, q[3].x, q[3].y};
        CHECK(ct_finish(quad, 40, 30, 80, 90, out), "finish");
        CHECK(out[0] == 16.f && out[1] == 18.f && out[2] == 60.f && out[3] == 18.f && out[4] == 60.f && out[5] == 66.f && out[6] == 16.f &&
                  out[7] == 66.f,
              "finish: top left, top right, bottom right, bottom left, scaled");
    }
    {
        const int c[4][2] = {{0, 0}, {39, 0}, {39, 29}, {0, 29}};
        Map m(40, 30);
        m.outline(c, 4);
        CHECK(run(m, q) && same_cycle(q, c), "outline on the page border");
    }
    {
        const int c[4][2] = {{30, 4}, {58, 30}, {32, 58}, {5, 31}};
        Map m(64, 64);
        m.outline(c, 4);
        CHECK(run(m, q), "rotated quadrilateral");
    }
    {
        const int c[4][2] = {{20, 6}, {44, 6}, {60, 40}, {4, 40}};
        Map m(64, 48);
        m.outline(c, 4);
        CHECK(!run(m, q), "trapezoid: the 0.85 side test");
    }
    {
        const int c[4][2] = {{10, 10}, {20, 10}, {20, 20}, {10, 20}};
        Map m(64, 64);
        m.outline(c, 4);
        CHECK(!run(m, q), "below 5 % of the map");
    }
    {
        const int c[5][2] = {{32, 4}, {60, 26}, {48, 58}, {16, 58}, {4, 26}};
        Map m(64, 64);
        m.outline(c, 5);
        (void)run(m, q);
    }
    {
        Map m(9, 9);
        m.set(4, 4);
        CHECK(!run(m, q, &outer, &hole) && outer == 1 && hole == 0, "isolated pixel");
    }
    {
        Map m(17, 12);
        CHECK(!run(m, q, &outer, &hole) && outer == 0 && hole == 0, "empty map");
    }
    {
        Map m(17, 12, 255);
        (void)run(m, q, &outer, &hole);
        CHECK(outer == 1 && hole == 0, "full map: one outer border");
    }
    {
        Map m(1, 1, 255);
        CHECK(!run(m, q), "1 x 1");
    }
    {
        Map m(9, 1);
        for (int x : {0, 2, 3, 6, 7, 8}) m.set(x, 0);
        CHECK(!run(m, q, &outer, &hole) && outer == 3, "1 x 9: three runs");
    }
    {
        Map m(511, 3);
        for (int x = 0; x < 511; ++x) {
            m.set(x, 0);
            m.set(x, 2);
        }
        m.set(0, 1);
        m.set(200, 1);
        m.set(510, 1);
        (void)run(m, q, &outer, &hole);
        CHECK(outer == 1 && hole == 2, "511 x 3: two holes");
    }
    {   // corners that are not in strictly convex position: refused, nothing read past the hull
        const int32_t line[8] = {0, 0, 5, 5, 10, 10, 0, 10}, inside[8] = {0, 0, 10, 0, 3, 2, 0, 10}, twice[8] = {0, 0, 10, 0, 10, 0, 0, 10};
        float out[8];
        CHECK(!ct_finish(line, 10, 10, 20, 20, out) && !ct_finish(inside, 10, 10, 20, 20, out) && !ct_finish(twice, 10, 10, 20, 20, out),
              "finish refuses");
    }
    std::printf(failures ? "contour: %d FAILED\n" : "contour: OK\n", failures);
    return failures ? 1 : 0;
}
