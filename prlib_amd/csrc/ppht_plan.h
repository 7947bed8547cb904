// ppht_plan.h — the geometry of the HoughLinesP group kernel (ppht_group.hip): how many workgroups share a page's accumulator,
// which angles each of them owns and where the cells of an angle start in its LDS.  Plain C++17: no HIP header, no environment,
// no I/O - tests/cpp/test_ppht_plan.cpp drives it on the CPU (every cvRound(x cos + y sin) of a page must fall in the row the
// plan gives its angle: an error of one cell would vote into the neighbouring angle's cells and fault nowhere).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

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

}  // namespace prl_hip
