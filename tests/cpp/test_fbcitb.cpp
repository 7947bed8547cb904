// test_fbcitb.cpp - bilateral.h, the contour tree of contour.h and fbcitb.h on the CPU, a program of its own: tests/test_fbcitb_cpu.py
// builds it with -fsanitize=address,undefined and runs it.  Without arguments it checks what can be said without a reference; with
//     filter <in> <W> <H> <d> <sigmaColor> <sigmaSpace> <out>
// it filters a raw W x H plane with bilateral.h's loop, which the Python test compares with the numpy restatement byte for byte.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../../prlib_amd/csrc/bilateral.h"
#include "../../prlib_amd/csrc/fbcitb.h"

using namespace prl_hip;

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static int run_filter(char** a)
{
    const int W = std::atoi(a[1]), H = std::atoi(a[2]), d = std::atoi(a[3]);
    const double sc = std::atof(a[4]), ss = std::atof(a[5]);
    std::vector<uint8_t> in((size_t)W * H), out((size_t)W * H);
    FILE* f = std::fopen(a[0], "rb");
    if (!f || std::fread(in.data(), 1, in.size(), f) != in.size()) return 2;
    std::fclose(f);
    BilTables t;
    if (!bil_tables(d, sc, ss, &t)) return 3;
    bil_filter_plane(in.data(), (size_t)W, 1, W, H, t, out.data(), (size_t)W, 1);
    f = std::fopen(a[6], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}

static void test_bilateral()
{
    BilTables t;
    CHECK(bil_radius(-1, 2.0) == 3 && bil_radius(0, 3.0) == 4 && bil_radius(0, 1.0) == 2 && bil_radius(0, 0.0) == 2);
    CHECK(bil_radius(1, 9.0) == 1 && bil_radius(4, 9.0) == 2 && bil_radius(31, 9.0) == 15 && bil_radius(0, 1e300) == 2147483647);
    CHECK(bil_tables(5, 150.0, 150.0, &t) && t.radius == 2 && t.n_taps == 12);
    CHECK(t.dy[0] == -2 && t.dx[0] == 0 && t.dy[1] == -1 && t.dx[1] == -1 && t.dy[11] == 2 && t.dx[11] == 0);
    CHECK(bil_tables(31, 1.0, 1.0, &t) && t.n_taps == kBilMaxTaps);
    CHECK(t.color[0] == 1.0f && t.color[14] > 0.0f && t.color[14] < 1.17549435e-38f);   // a denormal weight
    CHECK(!bil_tables(33, 1.0, 1.0, &t) && t.radius == 16);
    // the tie page of tests/fbcitb_ref.py: 10.5 and 11.5 round to even
    const double tie_sc = std::sqrt(0.5 / std::log(2.0));
    CHECK(bil_tables(3, tie_sc, 1e8, &t) && t.n_taps == 4 && t.space[0] == 1.0f && t.color[1] == 0.5f && t.color[2] == 0.0625f);
    std::vector<uint8_t> page(81, 200), out(81, 0);
    page[2 * 9 + 2] = 10; page[1 * 9 + 2] = 11; page[2 * 9 + 1] = 11;
    page[6 * 9 + 6] = 11; page[5 * 9 + 6] = 12; page[6 * 9 + 5] = 12;
    bil_filter_plane(page.data(), 9, 1, 9, 9, t, out.data(), 9, 1);
    CHECK(out[2 * 9 + 2] == 10 && out[6 * 9 + 6] == 12 && out[0] == 200);
    // a page smaller than the radius, interleaved channels through the pixel strides, a constant page
    CHECK(bil_tables(9, 50.0, 3.0, &t));
    const uint8_t small[2 * 3 * 2] = {1, 250, 9, 240, 200, 7, 90, 3, 4, 100, 50, 60};
    uint8_t sout[12] = {0};
    bil_filter_plane(small, 6, 2, 3, 2, t, sout, 6, 2);
    bil_filter_plane(small + 1, 6, 2, 3, 2, t, sout + 1, 6, 2);
    CHECK(bil_reflect101(-5, 3) == 1 && bil_reflect101(7, 3) == 1 && bil_reflect101(-9, 1) == 0);
    std::vector<uint8_t> flat(35, 77), fout(35, 0);
    bil_filter_plane(flat.data(), 7, 1, 7, 5, t, fout.data(), 7, 1);
    CHECK(fout == flat);
}

static std::vector<uint8_t> rings(int depth, int* side)
{
    const int n = 4 * depth + 7;
    std::vector<uint8_t> m((size_t)n * n, 0);
    for (int k = 0; k < depth; ++k) {
        const int a = 2 * k, b = n - 1 - 2 * k;
        for (int i = a; i <= b; ++i) m[(size_t)a * n + i] = m[(size_t)b * n + i] = m[(size_t)i * n + a] = m[(size_t)i * n + b] = 255;
    }
    m[(size_t)(n / 2) * n + n / 2 - 1] = m[(size_t)(n / 2) * n + n / 2 + 1] = 255;
    *side = n;
    return m;
}

static void test_tree()
{
    std::vector<CtPoint> pts, pts2;
    std::vector<CtNode> nodes;
    std::vector<CtContour> flat;
    int n;
    const std::vector<uint8_t> m = rings(3, &n);
    ct_find_contours_tree(m.data(), (size_t)n, n, n, &pts, &nodes);
    CHECK(nodes.size() == 8);   // three rings with a hole each, two blobs in the innermost hole
    for (int i = 0; i < 6 && nodes.size() == 8; ++i) CHECK(nodes[i].parent == i - 1 && nodes[i].hole == (i & 1) && nodes[i].child == i + 1 && nodes[i].next == -1);
    if (nodes.size() == 8) {
        CHECK(nodes[6].parent == 5 && nodes[7].parent == 5 && nodes[6].next == 7 && nodes[7].prev == 6 && nodes[7].next == -1);
        CHECK(pts[nodes[6].first].x > pts[nodes[7].first].x);   // the blob discovered last comes first
    }
    // every 4 x 4 map: the same borders as RETR_CCOMP gives, links that are each other's inverse, parents before children
    for (int bits = 0; bits < 65536; ++bits) {
        uint8_t map[16];
        for (int i = 0; i < 16; ++i) map[i] = (bits >> i) & 1 ? 255 : 0;
        ct_find_contours_tree(map, 4, 4, 4, &pts, &nodes);
        ct_find_contours(map, 4, 4, 4, &pts2, &flat);
        bool ok = nodes.size() == flat.size() && pts.size() == pts2.size();
        std::multiset<std::vector<int>> a, b;
        for (const CtNode& nd : nodes) {
            std::vector<int> key(1, nd.hole);
            for (int k = 0; k < nd.count; ++k) { key.push_back(pts[nd.first + k].x); key.push_back(pts[nd.first + k].y); }
            a.insert(key);
        }
        for (const CtContour& c : flat) {
            std::vector<int> key(1, c.hole);
            for (int k = 0; k < c.count; ++k) { key.push_back(pts2[c.first + k].x); key.push_back(pts2[c.first + k].y); }
            b.insert(key);
        }
        ok = ok && a == b;
        for (int i = 0; ok && i < (int)nodes.size(); ++i) {
            const CtNode& nd = nodes[i];
            ok = ok && nd.parent < i && (nd.parent < 0 ? !nd.hole : nodes[nd.parent].hole != nd.hole);
            if (nd.next >= 0) ok = ok && nodes[nd.next].prev == i && nodes[nd.next].parent == nd.parent && nd.next > i;
            if (nd.child >= 0) ok = ok && nd.child == i + 1 && nodes[nd.child].parent == i && nodes[nd.child].prev == -1;
            if (nd.prev < 0 && nd.parent >= 0) ok = ok && nodes[nd.parent].child == i;
        }
        if (!ok) {
            std::printf("FAILED: 4 x 4 map %d\n", bits);
            ++failures;
            break;
        }
    }
}

static std::vector<CtNode> chain_with_children(int top_points, int n_children, int grandchildren_of_first)
{
    // node 0 with n_children children, the first of which has `grandchildren_of_first` children; pre-order
    std::vector<CtNode> v;
    v.push_back(CtNode{0, top_points, 0, -1, -1, n_children ? 1 : -1, -1});
    int prev = -1;
    for (int c = 0; c < n_children; ++c) {
        const int at = (int)v.size();
        v.push_back(CtNode{0, 4, 1, -1, prev, -1, 0});
        if (prev >= 0) v[prev].next = at;
        prev = at;
        if (c == 0) {
            int gprev = -1;
            for (int g = 0; g < grandchildren_of_first; ++g) {
                const int ga = (int)v.size();
                v.push_back(CtNode{0, 4, 0, -1, gprev, -1, at});
                if (gprev >= 0) v[gprev].next = ga;
                else v[at].child = ga;
                gprev = ga;
            }
        }
    }
    return v;
}

static void test_remove_children()
{
    std::vector<uint8_t> ok;
    std::vector<CtNode> v = chain_with_children(10, 5, 0);   // 5 descendants: approved, the children ignored
    ct_remove_children(v, &ok);
    CHECK(ok[0] == 1 && ok[1] == 0 && ok[5] == 0);
    v = chain_with_children(10, 6, 0);                       // 6: ignored, and the walk descends: every child approved
    ct_remove_children(v, &ok);
    CHECK(ok[0] == 0 && ok[1] == 1 && ok[6] == 1);
    v = chain_with_children(10, 3, 2);                       // 5 descendants over two levels: the grandchildren are never visited
    ct_remove_children(v, &ok);
    CHECK(ok[0] == 1 && ok[1] == 0 && ok[2] == 0 && ok[3] == 0 && ok[4] == 0);
    v = chain_with_children(10, 2, 7);                       // 9 descendants: down; the first child has 7: down again
    ct_remove_children(v, &ok);
    CHECK(ok[0] == 0 && ok[1] == 0 && ok[2] == 1 && ok[8] == 1 && ok[9] == 1);
    v = chain_with_children(2, 6, 0);                        // a short contour at index 0: ignored, its children never visited
    v.push_back(CtNode{0, 5, 0, -1, 0, -1, -1});
    v[0].next = 7;
    ct_remove_children(v, &ok);
    CHECK(ok[0] == 0 && ok[1] == 0 && ok[6] == 0 && ok[7] == 1);
    v.clear();
    ct_remove_children(v, &ok);
    CHECK(ok.empty());
}

static void test_cut_contours_paint()
{
    CHECK(fb_variance_cut(0.0) == 0 && fb_variance_cut(0.005) == 0 && fb_variance_cut(-3.0) == 0);
    CHECK(fb_variance_cut(std::nan("")) == kFbVarianceNever && fb_variance_cut(1e30) == kFbVarianceNever);
    for (double thr : {0.01, 0.0123, 1.0, 200.0, 200.5, 16000.0}) {
        const int cut = fb_variance_cut(thr);
        CHECK(cut > 0 && cut < kFbVarianceNever && fb_variance_of(cut) > (float)thr && !(fb_variance_of(cut - 1) > (float)thr));
    }
    CHECK(fb_variance_cut(200.0) == 16201);   // 16200 / 81 = 200 is not above 200
    // a 30 x 24 page: a dark 8 x 6 frame on a light ground, its map the frame's outline
    const int W = 30, H = 24;
    std::vector<uint8_t> gray((size_t)W * H, 220), map((size_t)W * H, 0), out((size_t)W * H, 0);
    for (int y = 8; y < 14; ++y)
        for (int x = 10; x < 18; ++x) {
            const bool edge = y == 8 || y == 13 || x == 10 || x == 17;
            map[(size_t)y * W + x] = edge ? 255 : 0;
            gray[(size_t)y * W + x] = edge ? 40 : 60;
        }
    std::vector<FbRect> rects;
    FbCounts c = fb_contours(map.data(), (size_t)W, gray.data(), (size_t)W, W, H, 0.3, &rects);
    CHECK(c.found == 2 && c.approved == 1 && c.kept == 1 && rects.size() == 1);
    if (rects.size() == 1) {
        const FbRect r = rects[0];   // F = 40 on the dark frame, B = 220: F < B, white iff p >= 40
        CHECK(r.x == 10 && r.y == 8 && r.w == 8 && r.h == 6 && r.cut == 40 && r.below == 0);
    }
    c = fb_contours(map.data(), (size_t)W, gray.data(), (size_t)W, W, H, 48.0 / (W * H), &rects);
    CHECK(c.kept == 0 && c.approved == 1);   // area 48 is not below int(48)
    const FbRect two[2] = {{2, 2, 10, 10, 100, 0}, {6, 6, 10, 10, 100, 1}};
    const FbRect swapped[2] = {two[1], two[0]};
    std::vector<uint8_t> a((size_t)W * H), b((size_t)W * H);
    fb_paint(gray.data(), (size_t)W, W, H, two, 2, a.data(), (size_t)W);
    fb_paint(gray.data(), (size_t)W, W, H, swapped, 2, b.data(), (size_t)W);
    CHECK(a[(size_t)3 * W + 3] == 255 && a[(size_t)7 * W + 7] == 0 && b[(size_t)7 * W + 7] == 255 && a[0] == 255 && a != b);
    const FbRect off[3] = {{-1, 0, 4, 4, 0, 1}, {28, 0, 3, 3, 0, 1}, {0, 0, 0, 3, 0, 1}};
    fb_paint(gray.data(), (size_t)W, W, H, off, 3, a.data(), (size_t)W);
    CHECK(a == std::vector<uint8_t>((size_t)W * H, 255));   // rectangles that are not on the page are ignored
}

int main(int argc, char** argv)
{
    if (argc == 9 && std::strcmp(argv[1], "filter") == 0) return run_filter(argv + 2);
    test_bilateral();
    test_tree();
    test_remove_children();
    test_cut_contours_paint();
    if (failures) return 1;
    std::printf("fbcitb: OK\n");
    return 0;
}
