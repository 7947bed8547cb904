// fbcitb.h — the host half of prl::binarizeFBCITB (src/binarizations/binarizeFBCITB.cpp:73-404) behind its contour map: the integer
// cut of the variance mask, the contours kept (cv::findContours(RETR_TREE), RemoveChildrenContours, the rectangle filters), every
// kept contour's decision as (rectangle, integer cut, polarity), and the ordered paint as a plain loop (the rules:
// include/prl_hip.h, "binarizeFBCITB").  Plain C++17: no HIP header, no environment, no I/O - tests/cpp/test_fbcitb.cpp drives it on
// the CPU under the sanitizers.  fbcitb.hip runs the contours part per page on the host thread pool; the loop is for tests.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "contour.h"

namespace prl_hip {

// MatToLocalVarianceMap(page, 3) > threshold as a comparison of integers.  The map is max(float32(D) * (1 / (9f * 9f)), 0.01f) with
// D = 9 * sum(p^2) - sum(p)^2 over the 3 x 3 window, an integer below 2^24, and the comparison is made in float32 against
// (float)threshold [upstream: cv::compare converts the scalar to the array's depth].  The map is monotone in D: returns the
// smallest D that passes (0: every pixel does - a threshold below the 0.01 floor), or 1 << 24 when none can (a NaN threshold too).
constexpr int kFbVarianceNever = 1 << 24;
inline float fb_variance_of(int D)
{
    const float area = 9.0f;
    const volatile float scale = 1.0f / (area * area);
    const volatile float v = (float)D * scale;
    return v > 0.01f ? v : 0.01f;
}
inline int fb_variance_cut(double threshold)
{
    const float t = (float)threshold;
    if (!(fb_variance_of(kFbVarianceNever - 1) > t)) return kFbVarianceNever;
    int lo = 0, hi = kFbVarianceNever - 1;   // the smallest D with fb_variance_of(D) > t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (fb_variance_of(mid) > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// A kept contour's decision: inside the rectangle a pixel p of the gray plane becomes 255 iff (below ? p < cut : p >= cut), else 0
struct FbRect {
    int32_t x, y, w, h, cut, below;
};

struct FbCounts {
    int found, approved, kept;   // contours: all, after RemoveChildrenContours, after the rectangle filters
};

// binarizeFBCITB.cpp:196-357 on one page: `map` the contour map, `gray` the processed page after COLOR_BGR2GRAY.  max_area =
// boundingRectangleMaxArea.  The kept contours in index order (the paint's order).
//   filters    area > 10, area < int(max_area * cols * rows), width < int(0.8 * cols), height < int(0.8 * rows)
//   F          the float32 sum of the gray bytes at the contour's points, in point order, then F = (float)((double)F * (1. / N))
//              (cv::Vec3f /= int)
//   B          element size / 2 of the sorted gray bytes at those of the twelve corner neighbours (:284-331) that lie on the page.
//              The list is never empty for a kept contour: width <= int(0.8 cols) - 1 <= 0.8 cols - 1 gives cols - width >=
//              0.2 cols + 1 > 1, so at least two columns of the page lie outside the rectangle.  With x >= 1 the neighbour
//              (x - 1, y) is on the page; with x == 0 the neighbour (x + width + 1, y) is, since width + 1 <= cols - 1.  (y is a
//              row of the page in both.)  A page too narrow to leave two columns keeps no contour.
//   decision   F < B: white iff p >= F; else white iff p < F.  cv::compare of bytes with a scalar is the exact real comparison, and
//              for an integer p both are comparisons with ceil(F).
inline FbCounts fb_contours(const uint8_t* map, size_t map_step, const uint8_t* gray, size_t gray_step, int w, int h, double max_area,
                            std::vector<FbRect>* out)
{
    out->clear();
    std::vector<CtPoint> pts;
    std::vector<CtNode> nodes;
    ct_find_contours_tree(map, map_step, w, h, &pts, &nodes);
    FbCounts n{(int)nodes.size(), 0, 0};
    if (nodes.empty()) return n;
    std::vector<uint8_t> approved;
    ct_remove_children(nodes, &approved);
    const double area_limit = max_area * w * h;   // (the entries refuse a coefficient that is not finite)
    const int rect_max_area = area_limit >= 2147483647.0 ? 2147483647 : area_limit <= -2147483647.0 ? -2147483647 : (int)area_limit;
    const int max_w = (int)(0.8 * w), max_h = (int)(0.8 * h);
    for (size_t i = 0; i < nodes.size(); ++i) {
        if (!approved[i]) continue;
        ++n.approved;
        const CtPoint* p = pts.data() + nodes[i].first;
        const int cnt = nodes[i].count;
        int x0 = p[0].x, x1 = x0, y0 = p[0].y, y1 = y0;
        for (int k = 1; k < cnt; ++k) {
            x0 = std::min(x0, p[k].x); x1 = std::max(x1, p[k].x);
            y0 = std::min(y0, p[k].y); y1 = std::max(y1, p[k].y);
        }
        const int rw = x1 - x0 + 1, rh = y1 - y0 + 1;
        const long long area = (long long)rw * rh;
        if (!(area > 10 && area < rect_max_area && rw < max_w && rh < max_h)) continue;
        volatile float f = 0.f;
        for (int k = 0; k < cnt; ++k) f = f + (float)gray[(size_t)p[k].y * gray_step + p[k].x];
        const float F = (float)((double)f * (1. / cnt));
        uint8_t b[12];
        int nb = 0;
        const int bx[12] = {x0 - 1, x0 - 1, x0, x0 + rw + 1, x0 + rw, x0 + rw + 1, x0 - 1, x0 - 1, x0, x0 + rw + 1, x0 + rw, x0 + rw + 1};
        const int by[12] = {y0 - 1, y0, y0 - 1, y0 - 1, y0 - 1, y0, y0 + rh + 1, y0 + rh, y0 + rh + 1, y0 + rh + 1, y0 + rh + 1, y0 + rh};
        for (int k = 0; k < 12; ++k)
            if (bx[k] >= 0 && bx[k] < w && by[k] >= 0 && by[k] < h) b[nb++] = gray[(size_t)by[k] * gray_step + bx[k]];
        if (nb == 0) continue;   // (cannot happen, see above; the reference would read past an empty vector)
        std::sort(b, b + nb);
        const int B = b[nb / 2];
        const int cut = (int)std::ceil(F);
        out->push_back(FbRect{x0, y0, rw, rh, cut, F < (float)B ? 0 : 1});
        ++n.kept;
    }
    return n;
}

// combinationAND.copyTo(resultROI) for every rectangle in order on a page of 255: where rectangles overlap the later one wins
inline void fb_paint(const uint8_t* gray, size_t gray_step, int w, int h, const FbRect* rects, int n, uint8_t* dst, size_t dst_step)
{
    for (int y = 0; y < h; ++y) std::fill(dst + (size_t)y * dst_step, dst + (size_t)y * dst_step + w, (uint8_t)255);
    for (int k = 0; k < n; ++k) {
        const FbRect& r = rects[k];
        if (r.x < 0 || r.y < 0 || r.w <= 0 || r.h <= 0 || r.w > w - r.x || r.h > h - r.y) continue;   // not on the page: ignored
        for (int y = r.y; y < r.y + r.h; ++y)
            for (int x = r.x; x < r.x + r.w; ++x) {
                const int p = gray[(size_t)y * gray_step + x];
                dst[(size_t)y * dst_step + x] = (r.below ? p < r.cut : p >= r.cut) ? 255 : 0;
            }
    }
}

}  // namespace prl_hip
