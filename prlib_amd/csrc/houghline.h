// houghline.h — the host half of prl::findHoughLineContour (src/border_detection/houghLine.cpp:16-175, fromVec2f of
// imageLibCommon.cpp:929-941, intersection of autoCropUtils.cpp:350-366): the geometry and the trig table of cv::HoughLines,
// the order of its peaks, the line filter (deleteSimilarLines) and the quad search (findMaxValidContour).  It also carries the
// standard transform as a plain C++ loop (hl_vote, hl_peaks): the yardstick of tests/cpp/test_houghline.cpp and of
// tools/bench_houghline.py, never the product path.  The arithmetic is stated in include/prl_hip.h ("Hough lines") and restated
// in tests/houghline_ref.py.  Plain C++17: no HIP header, no environment, no I/O.  Build with -ffp-contract=off: the float32
// expressions below keep one rounding per operation.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace prl_hip {

constexpr int kHlNumAngle = 180;   // cvRound(CV_PI / theta), theta = (float)(CV_PI / 180): the rule of OpenCV 3.4 and 4.x

inline float hl_theta() { return (float)(3.1415926535897932384626433832795 / 180); }
inline int hl_numrho(int width, int height) { return (width + height) * 2 + 1; }   // cvRound(((W + H) * 2 + 1) / 1.0)
inline size_t hl_accum_cells(int width, int height) { return (size_t)(kHlNumAngle + 2) * (size_t)(hl_numrho(width, height) + 2); }

// createTrigTable [upstream]: the angle is accumulated in float32, sin / cos are the host's libm in float64
inline void hl_trig_table(float* tab_cos, float* tab_sin)
{
    const float theta = hl_theta(), irho = 1.f;
    float ang = 0.f;
    for (int n = 0; n < kHlNumAngle; ang += theta, ++n) {
        tab_sin[n] = (float)(std::sin((double)ang) * irho);
        tab_cos[n] = (float)(std::cos((double)ang) * irho);
    }
}

// a peak of the accumulator: its count and its cell index (n + 1) * (numrho + 2) + r + 1
struct HlPeak {
    uint32_t count, cell;
};

// OpenCV's order: by count, descending, then by cell index, ascending
inline void hl_sort_peaks(HlPeak* p, size_t n)
{
    std::sort(p, p + n, [](const HlPeak& a, const HlPeak& b) { return a.count > b.count || (a.count == b.count && a.cell < b.cell); });
}

// (rho, theta) of a cell
inline void hl_line_of(uint32_t cell, int numrho, float* rho, float* theta)
{
    const int n = (int)(cell / (uint32_t)(numrho + 2)) - 1, r = (int)(cell - (uint32_t)(n + 1) * (uint32_t)(numrho + 2)) - 1;
    *rho = ((float)r - (float)(numrho - 1) * 0.5f) * 1.f;
    *theta = (float)n * hl_theta();
}

// HoughLinesStandard's voting loop [upstream] on the CPU: accum has hl_accum_cells entries and is zeroed here
inline void hl_vote(const uint8_t* map, size_t step, int width, int height, int32_t* accum)
{
    const int numrho = hl_numrho(width, height);
    float tc[kHlNumAngle], ts[kHlNumAngle];
    hl_trig_table(tc, ts);
    std::fill(accum, accum + hl_accum_cells(width, height), 0);
    for (int i = 0; i < height; ++i)
        for (int j = 0; j < width; ++j) {
            if (map[(size_t)i * step + j] == 0) continue;
            for (int n = 0; n < kHlNumAngle; ++n) {
                const float a = (float)j * tc[n], b = (float)i * ts[n];
                const int r = (int)std::nearbyint(a + b) + (numrho - 1) / 2;   // (the default rounding mode: to nearest even)
                accum[(size_t)(n + 1) * (size_t)(numrho + 2) + (size_t)(r + 1)]++;
            }
        }
}

inline void hl_peaks(const int32_t* accum, int numrho, int threshold, std::vector<HlPeak>* out)
{
    out->clear();
    for (int n = 0; n < kHlNumAngle; ++n)
        for (int r = 0; r < numrho; ++r) {
            const size_t base = (size_t)(n + 1) * (size_t)(numrho + 2) + (size_t)(r + 1);
            const int32_t a = accum[base];
            if (a > threshold && a > accum[base - 1] && a >= accum[base + 1] && a > accum[base - numrho - 2] && a >= accum[base + numrho + 2])
                out->push_back(HlPeak{(uint32_t)a, (uint32_t)base});
        }
    hl_sort_peaks(out->data(), out->size());
}

// ---- the line filter and the quad search --------------------------------------------------------------------------------------

struct HlPointF {
    float x, y;
};
struct HlSegment {   // fromVec2f: two points 2000 apart on the line, both with integer coordinates
    HlPointF a, b;
};

inline int hl_round(double v) { return (int)std::nearbyint(v); }   // cvRound

// imageLibCommon.cpp:929-941.  std::cos / std::sin of a float are the float overloads: cosf, sinf
inline HlSegment hl_from_vec2f(float rho, float theta)
{
    const double a = std::cos(theta), b = std::sin(theta);
    const double x0 = a * rho, y0 = b * rho;
    HlSegment s;
    s.a.x = (float)hl_round(x0 + 1000 * (-b));
    s.a.y = (float)hl_round(y0 + 1000 * (a));
    s.b.x = (float)hl_round(x0 - 1000 * (-b));
    s.b.y = (float)hl_round(y0 - 1000 * (a));
    return s;
}

// houghLine.cpp:16-25; the float ends arrive as cv::Point (they hold integers, so the conversion is exact)
inline double hl_distance_to_line(HlPointF start, HlPointF end, HlPointF point)
{
    const int sx = (int)start.x, sy = (int)start.y, ex = (int)end.x, ey = (int)end.y, px = (int)point.x, py = (int)point.y;
    const double normal = std::hypot(ex - sx, ey - sy);
    const double distance = (double)((px - sx) * (ey - sy) - (py - sy) * (ex - sx)) / normal;
    return std::fabs(distance);
}

// houghLine.cpp:27-86 on (rho, theta) pairs
inline void hl_delete_similar_lines(std::vector<std::pair<float, float>>* lines, double min_dist, double step_dist, int max_lines)
{
    std::vector<std::pair<float, float>> tmp;
    std::vector<char> used(lines->size(), 0);
    std::vector<HlSegment> seg;
    while ((int)lines->size() > max_lines) {
        std::fill(used.begin(), used.end(), 0);
        tmp.clear();
        seg.resize(lines->size());
        for (size_t i = 0; i < lines->size(); ++i) seg[i] = hl_from_vec2f((*lines)[i].first, (*lines)[i].second);
        for (size_t i = 0; i < lines->size(); ++i) {
            if (used[i]) continue;
            used[i] = 1;
            tmp.push_back((*lines)[i]);
            const HlSegment v1 = seg[i];
            for (size_t j = i + 1; j < lines->size(); ++j) {
                if (used[j]) continue;
                const HlSegment v2 = seg[j];
                const double dist = std::min(std::min(hl_distance_to_line(v1.a, v1.b, v2.a), hl_distance_to_line(v1.a, v1.b, v2.b)),
                                             std::min(hl_distance_to_line(v2.a, v2.b, v1.a), hl_distance_to_line(v2.a, v2.b, v1.b)));
                if (dist < min_dist) used[j] = 1;
            }
        }
        if (tmp.size() < 4) {   // the reference gives up on the filter and keeps the first max_lines of this round's input
            lines->resize((size_t)max_lines);
            break;
        }
        *lines = tmp;
        min_dist += step_dist;
    }
}

// autoCropUtils.cpp:350-366: the cross product and the quotient in float32, eq_d's 1e-7, the scaling in float64
inline bool hl_intersection(HlPointF o1, HlPointF p1, HlPointF o2, HlPointF p2, HlPointF* r)
{
    const HlPointF x{o2.x - o1.x, o2.y - o1.y}, d1{p1.x - o1.x, p1.y - o1.y}, d2{p2.x - o2.x, p2.y - o2.y};
    const float m0 = d1.x * d2.y, m1 = d1.y * d2.x;
    const float cross = m0 - m1;
    if (std::fabs((double)cross - 0.0) <= 1e-7) return false;
    const float n0 = x.x * d2.y, n1 = x.y * d2.x;
    const float num = n0 - n1;
    const double t1 = num / cross;   // float / float, then widened
    const float sx = (float)(d1.x * t1), sy = (float)(d1.y * t1);   // Point2f * double
    r->x = o1.x + sx;
    r->y = o1.y + sy;
    return true;
}

// cv::contourArea [upstream] of float points: float64 sums of float32 products widened one factor at a time
inline double hl_contour_area(const HlPointF* p, int n)
{
    double a00 = 0;
    HlPointF prev = p[n - 1];
    for (int i = 0; i < n; ++i) {
        a00 += (double)prev.x * p[i].y - (double)prev.y * p[i].x;
        prev = p[i];
    }
    return std::fabs(a00 * 0.5);
}

// cv::isContourConvex [upstream, 3.4 / 4.x] of float points: every turn of one strict sign, decided in float32
inline bool hl_is_contour_convex(const HlPointF* p, int n)
{
    HlPointF prev = p[(n - 2 + n) % n], cur = p[n - 1];
    float dx0 = cur.x - prev.x, dy0 = cur.y - prev.y;
    int orientation = 0;
    for (int i = 0; i < n; ++i) {
        prev = cur;
        cur = p[i];
        const float dx = cur.x - prev.x, dy = cur.y - prev.y;
        const float dxdy0 = dx * dy0, dydx0 = dy * dx0;
        orientation |= (dydx0 > dxdy0) ? 1 : ((dydx0 < dxdy0) ? 2 : 3);
        if (orientation == 3) return false;
        dx0 = dx;
        dy0 = dy;
    }
    return true;
}

// IsQuadrangularConvex (imageLibCommon.cpp:821-833): cv::convexHull of the four float points has four vertices, that is the four
// are in strictly convex position: each lies strictly outside the triangle of the other three.  Decided on float64 cross products
// of the float32 coordinates (include/prl_hip.h says where OpenCV's float32 scan may differ).
inline bool hl_four_in_convex_position(const HlPointF* p)
{
    auto cross = [](HlPointF a, HlPointF b, HlPointF c) {
        return ((double)b.x - a.x) * ((double)c.y - a.y) - ((double)b.y - a.y) * ((double)c.x - a.x);
    };
    for (int i = 0; i < 4; ++i) {   // p[i] against the triangle of the others
        const HlPointF a = p[(i + 1) & 3], b = p[(i + 2) & 3], c = p[(i + 3) & 3], q = p[i];
        const double area = cross(a, b, c);
        if (area == 0) return false;   // three on a line
        const double s0 = cross(a, b, q), s1 = cross(b, c, q), s2 = cross(c, a, q);
        const bool inside = area > 0 ? (s0 >= 0 && s1 >= 0 && s2 >= 0) : (s0 <= 0 && s1 <= 0 && s2 <= 0);
        if (inside) return false;
    }
    return true;
}

// houghLine.cpp:88-175: every ordered choice of four lines; false: no quad
inline bool hl_find_max_valid_contour(const std::vector<std::pair<float, float>>& lines, int width, int height, HlPointF out[4])
{
    const size_t L = lines.size();
    std::vector<HlSegment> seg(L);
    for (size_t i = 0; i < L; ++i) seg[i] = hl_from_vec2f(lines[i].first, lines[i].second);
    // cross[a * L + b]: intersection(seg[a], seg[b]) as the loop below asks for it (it is a function of the ordered pair alone)
    std::vector<HlPointF> at(L * L);
    std::vector<char> ok(L * L, 0);
    for (size_t a = 0; a < L; ++a)
        for (size_t b = 0; b < L; ++b)
            if (a != b) ok[a * L + b] = hl_intersection(seg[a].a, seg[a].b, seg[b].a, seg[b].b, &at[a * L + b]) ? 1 : 0;
    double max_area = 0.0;
    bool found = false;
    for (size_t i = 0; i < L; ++i)
        for (size_t j = 0; j < L; ++j) {
            if (i == j || !ok[j * L + i]) continue;
            for (size_t k = 0; k < L; ++k) {
                if (i == k || j == k || !ok[k * L + j]) continue;
                for (size_t m = 0; m < L; ++m) {
                    if (i == m || j == m || k == m || !ok[m * L + k] || !ok[i * L + m]) continue;
                    const HlPointF pts[4] = {at[j * L + i], at[k * L + j], at[m * L + k], at[i * L + m]};
                    bool outside = false;   // (the reference's flag for this is named validCoord)
                    for (const HlPointF& v : pts)
                        if (v.x < 0 || v.x > (float)width || v.y < 0 || v.y > (float)height) {
                            outside = true;
                            break;
                        }
                    if (outside) continue;
                    const double area = hl_contour_area(pts, 4);
                    if (hl_is_contour_convex(pts, 4) && hl_four_in_convex_position(pts) && area > max_area) {
                        max_area = area;
                        std::copy(pts, pts + 4, out);
                        found = true;
                    }
                }
            }
        }
    return found;
}

// prl::findHoughLineContour from the line list on (houghLine.cpp:231-255): quad receives the four corners truncated to int
inline bool hl_quad(const float* lines, int n_lines, int width, int height, int32_t quad[8])
{
    if (n_lines < 4) return false;   // before the filter
    std::vector<std::pair<float, float>> v((size_t)n_lines);
    for (int i = 0; i < n_lines; ++i) v[(size_t)i] = {lines[2 * i], lines[2 * i + 1]};
    hl_delete_similar_lines(&v, 5.0, 5.0, 20);
    HlPointF p[4];
    if (!hl_find_max_valid_contour(v, width, height, p)) return false;
    for (int k = 0; k < 4; ++k) {
        quad[2 * k] = (int32_t)p[k].x;
        quad[2 * k + 1] = (int32_t)p[k].y;
    }
    return true;
}

}  // namespace prl_hip
