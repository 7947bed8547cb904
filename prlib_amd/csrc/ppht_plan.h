// ppht_plan.h — the host arithmetic of HoughLinesP on device memory.  The geometry of the group kernel (ppht_group.hip): how
// many workgroups share a page's accumulator, which angles each of them owns and where the cells of an angle start in its LDS.
// The workspace of one pass of the search (ppht.hip): its fixed blocks from the pass's shape, the point and segment lists from
// the counts the point stage reports, and how many pages a pass may take.  Plain C++17: no HIP header, no environment, no I/O -
// tests/cpp/test_ppht_plan.cpp drives it on the CPU (every cvRound(x cos + y sin) of a page must fall in the row the plan gives
// its angle, every list inside its block: an error of one cell or one entry would write into the neighbour's and fault nowhere).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "page_args.h"

namespace prl_hip {

constexpr int kNumAngle = 180;
constexpr int kMaxA = 180;              // angles per member (a small page is one member's)
constexpr int kMaxG = 32;               // members per group
constexpr int kMaxSide = 8000;          // |count| <= 2 max(W, H) < bias

struct GrpAngle {
    float c, s;   // the trig table's entries of this angle
    int base;     // cell index of r = 0 in this member's accumulator (may be negative: r starts at rmin)
    int n;        // the angle
};

// Geometry of the group kernel for W x H pages: members per group (0: the page does not qualify), angle tables.
struct GroupPlan {
    int G = 0;
    std::vector<GrpAngle> tab;     // [G][kMaxA]
    std::vector<int> tab_n, tab_dwords;
    size_t lds_bytes = 0;          // dynamic LDS of the launch
};

inline GroupPlan plan_group(int width, int height, int threshold, const float* ttab, size_t lds_budget, int min_g)
{
    GroupPlan gp;
    if (std::max(width, height) > kMaxSide || threshold < 1) return gp;
    // r = cvRound(x cos + y sin) over the page: between the projections of two opposite corners (float32 products and sum are
    // monotone in x and y), widened by one cell against the float32 roundings
    int rmin[kNumAngle], len[kNumAngle];
    for (int n = 0; n < kNumAngle; ++n) {
        const double c = ttab[2 * n], s = ttab[2 * n + 1];
        const double x_lo = c >= 0 ? 0 : width - 1, x_hi = c >= 0 ? width - 1 : 0;
        const double y_lo = s >= 0 ? 0 : height - 1, y_hi = s >= 0 ? height - 1 : 0;
        rmin[n] = (int)std::floor(x_lo * c + y_lo * s) - 1;
        const int rmax = (int)std::ceil(x_hi * c + y_hi * s) + 1;
        len[n] = rmax - rmin[n] + 1;
    }
    for (int G = std::max(1, min_g); G <= kMaxG; ++G) {
        if ((kNumAngle + G - 1) / G > kMaxA) continue;
        size_t worst = 0;
        for (int g = 0; g < G; ++g) {
            size_t cells = 0;
            for (int n = g; n < kNumAngle; n += G) cells += (size_t)len[n];
            worst = std::max(worst, (cells + 1) / 2 * 4);
        }
        if (worst > lds_budget) continue;
        gp.G = G;
        gp.lds_bytes = worst;
        gp.tab.assign((size_t)G * kMaxA, GrpAngle{0.f, 0.f, 0, 0});
        gp.tab_n.assign((size_t)G, 0);
        gp.tab_dwords.assign((size_t)G, 0);
        for (int g = 0; g < G; ++g) {
            int cells = 0, k = 0;
            for (int n = g; n < kNumAngle; n += G, ++k) {
                gp.tab[(size_t)g * kMaxA + k] = GrpAngle{ttab[2 * n], ttab[2 * n + 1], cells - rmin[n], n};
                cells += len[n];
            }
            gp.tab_n[(size_t)g] = k;
            gp.tab_dwords[(size_t)g] = (cells + 1) / 2;
        }
        return gp;
    }
    return gp;
}

// ---- the workspace of one pass of the search ----------------------------------------------------------------------

// The fixed part, one block after the other in this order, each rounded to 256 bytes: byte offsets from the workspace's start.
struct PphtFixed {
    size_t hist, thr;               // Otsu: 256 bins and a threshold per page
    size_t row_count, row_off;      // set pixels per mask row, their exclusive scan
    size_t count, n_lines, cap;     // per page: points, segments found, segments its list has room for
    size_t nz_off, lines_off;       // per page: where its point list / segment list starts (entries)
    size_t ttab;                    // kNumAngle x {cos, sin}
    size_t page_list;               // the pages left to the device-memory kernels
    size_t mask;                    // n_pages masks, mask_page bytes apart
    size_t total, mask_page;
};

inline PphtFixed ppht_fixed(int n_pages, int width, int height)
{
    PphtFixed f{};
    const size_t n = (size_t)n_pages;
    size_t at = 0;
    auto block = [&at](size_t bytes) { const size_t off = at; at += r256(bytes); return off; };
    f.mask_page = r256((size_t)width * height);
    f.hist = block(n * 256 * 4);
    f.thr = block(n * 4);
    f.row_count = block(n * height * 4);
    f.row_off = block(n * height * 4);
    f.count = block(n * 4);
    f.n_lines = block(n * 4);
    f.cap = block(n * 4);
    f.nz_off = block(n * 8);
    f.lines_off = block(n * 8);
    f.ttab = block(kNumAngle * 2 * 4);
    f.page_list = block(n * 4);
    f.mask = block(f.mask_page * n);
    f.total = at;
    return f;
}

// The two lists, sized from the points every page has.  A page's point list starts on a multiple of 64 entries.  A good line
// clears at least line_length / (line_gap + 1) points, which bounds the segments a page can produce: its capacity.
struct PphtLists {
    std::vector<unsigned long long> nz_off, lines_off;   // per page, in entries (a point: 4 bytes, a segment: 16)
    std::vector<unsigned> cap;
    unsigned long long nz_total = 0, lines_total = 0;
    size_t nz_bytes = 0, lines_bytes = 0;                // the point list's block, then the segment list's
};

inline PphtLists ppht_lists(const unsigned* count, int n_pages, int line_length, int line_gap)
{
    PphtLists l;
    l.nz_off.resize((size_t)n_pages);
    l.lines_off.resize((size_t)n_pages);
    l.cap.resize((size_t)n_pages);
    const unsigned per_line = (unsigned)std::max(1, line_length / (line_gap + 1));
    for (size_t i = 0; i < (size_t)n_pages; ++i) {
        l.nz_off[i] = l.nz_total;
        l.nz_total += (count[i] + 63) / 64 * 64;
        l.cap[i] = count[i] / per_line + 16;
        l.lines_off[i] = l.lines_total;
        l.lines_total += l.cap[i];
    }
    l.nz_bytes = r256(l.nz_total * 4 + 256);
    l.lines_bytes = r256(l.lines_total * 16 + 256);
    return l;
}

// What a page costs of a pass's budget: mask + gray page, accumulator in device memory, row counts and offsets, point list.
inline size_t ppht_bytes_per_page(int width, int height)
{
    const size_t numrho = (size_t)(width + height) * 2 + 1;
    return 2 * r256((size_t)width * height) + kNumAngle * numrho * 4 + (size_t)height * 8 + 2048 + (size_t)width * height / 2;
}

// pages per pass of the search: what the budget allows, one at least, 16384 at most
inline int ppht_pages_per_pass(int n_pages, int width, int height, size_t budget_bytes)
{
    return pages_per_chunk(n_pages, ppht_bytes_per_page(width, height), budget_bytes, 16384);
}

}  // namespace prl_hip
