// contour.h — the quad search of prl::documentContour (src/border_detection/autoCropUtils.cpp:155-348) on an 8UC1 map of at most
// a few hundred pixels a side: cv::findContours(RETR_CCOMP, CHAIN_APPROX_SIMPLE), cv::approxPolyDP(closed), cv::contourArea, the
// reference's side / angle / area filters, cv::convexHull of four points, scaleContour and cropVerticesOrdering.  The arithmetic is
// stated in include/prl_hip.h ("document contour") and restated in tests/contour_ref.py.  Plain C++17: no HIP header, no
// environment, no I/O - tests/cpp/test_contour.cpp drives it on the CPU under the sanitizers.  Pages are independent: the batch
// entry (contour.hip) runs one search per page on the host thread pool.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace prl_hip {

struct CtPoint {
    int32_t x, y;
};

// points [first, first + count) of the list that comes with it; hole: a hole border
struct CtContour {
    int first, count, hole;
};

constexpr int kCtDx[8] = {1, 1, 0, -1, -1, -1, 0, 1};   // direction 0 = +x, then counter-clockwise on the screen (y grows downwards)
constexpr int kCtDy[8] = {0, -1, -1, -1, 0, 1, 1, 1};
constexpr signed char kCtMark = 2, kCtRightEnd = (signed char)(2 | -128);

// One border from its start pixel i0 (Suzuki-Abe as OpenCV follows it); pt: the start in page coordinates.
inline void ct_trace(signed char* i0, const int* deltas, bool hole, CtPoint pt, std::vector<CtPoint>* out)
{
    int s_end = hole ? 0 : 4, s = s_end;
    signed char* i1;
    do {   // the first neighbour: clockwise from s_end
        s = (s - 1) & 7;
        i1 = i0 + deltas[s];
    } while (*i1 == 0 && s != s_end);
    if (s == s_end) {   // an isolated pixel
        *i0 = kCtRightEnd;
        out->push_back(pt);
        return;
    }
    signed char *i3 = i0, *i4 = nullptr;
    int prev_s = s ^ 4;
    for (;;) {
        s_end = s;
        while (s < 15) {   // counter-clockwise from the direction after the arrival
            i4 = i3 + deltas[++s];
            if (*i4 != 0) break;
        }
        s &= 7;
        if ((unsigned)(s - 1) < (unsigned)s_end) *i3 = kCtRightEnd;   // the search passed the right-hand neighbour
        else if (*i3 == 1) *i3 = kCtMark;
        if (s != prev_s) {
            out->push_back(pt);
            prev_s = s;
        }
        pt.x += kCtDx[s];
        pt.y += kCtDy[s];
        if (i4 == i0 && i3 == i1) break;
        i3 = i4;
        s = (s + 4) & 7;
    }
}

// cv::findContours(map, RETR_CCOMP, CHAIN_APPROX_SIMPLE): every border, in OpenCV's output order.
inline void ct_find_contours(const uint8_t* map, size_t step, int w, int h, std::vector<CtPoint>* points, std::vector<CtContour>* contours)
{
    points->clear();
    contours->clear();
    const int pw = w + 2;
    std::vector<signed char> img((size_t)pw * (h + 2), 0);   // one pixel of background all round
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) img[(size_t)(y + 1) * pw + x + 1] = map[(size_t)y * step + x] != 0;
    int deltas[16];
    for (int d = 0; d < 16; ++d) deltas[d] = kCtDy[d & 7] * pw + kCtDx[d & 7];

    struct Found {
        int first, count, hole, parent;
    };
    std::vector<Found> found;
    std::vector<CtPoint> raw;
    std::vector<int32_t> component((size_t)pw * (h + 2), -1);   // per foreground pixel: its outer border, in discovery order
    std::vector<int> queue;
    int n_outer = 0;
    for (int y = 1; y <= h; ++y) {
        int prev = 0;
        for (int x = 1; x <= w; ++x) {
            signed char* row = img.data() + (size_t)y * pw;
            int p = row[x];
            if (p != prev) {
                bool start = true, hole = false;
                if (!(prev == 0 && p == 1)) {
                    hole = true;
                    if (p != 0 || prev < 1) start = false;
                }
                if (start) {
                    const int x0 = x - (hole ? 1 : 0);
                    const int first = (int)raw.size();
                    int parent = -1;
                    if (!hole) {   // label the component this border encloses (8-connected)
                        const int id = n_outer++;
                        queue.assign(1, y * pw + x0);
                        component[(size_t)y * pw + x0] = id;
                        while (!queue.empty()) {
                            const int at = queue.back();
                            queue.pop_back();
                            for (int d = 0; d < 8; ++d) {
                                const int to = at + deltas[d];
                                if (img[to] != 0 && component[to] < 0) {
                                    component[to] = id;
                                    queue.push_back(to);
                                }
                            }
                        }
                    } else {
                        parent = component[(size_t)y * pw + x0];
                    }
                    ct_trace(row + x0, deltas, hole, CtPoint{x0 - 1, y - 1}, &raw);
                    found.push_back({first, (int)raw.size() - first, hole ? 1 : 0, parent});
                    p = row[x];
                }
            }
            prev = p;
        }
    }
    // outer borders from the last discovered to the first, each followed by its component's hole borders, last discovered first
    std::vector<std::vector<int>> holes((size_t)n_outer);
    std::vector<int> outers;
    for (int i = 0; i < (int)found.size(); ++i) {
        if (found[i].hole) holes[(size_t)found[i].parent].push_back(i);
        else outers.push_back(i);
    }
    auto emit = [&](int i) {
        contours->push_back({(int)points->size(), found[i].count, found[i].hole});
        points->insert(points->end(), raw.begin() + found[i].first, raw.begin() + found[i].first + found[i].count);
    };
    for (int o = n_outer - 1; o >= 0; --o) {
        emit(outers[o]);
        for (int k = (int)holes[o].size() - 1; k >= 0; --k) emit(holes[o][k]);
    }
}

struct CtRect {
    int32_t x, y, w, h;
};

// cv::findContours(map, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), as prl::binarizeLocalOtsu uses it (binarizeLocalOtsu.cpp:100-160): the
// cv::boundingRect of every contour of at least 3 points (RemoveChildrenContours on a flat hierarchy drops the shorter ones), in
// discovery order.  Returns the number of contours found, the short ones included.  The raster scan of OpenCV's retrieval mode 0,
// literally [upstream, from memory]: lnbd is the column of the last border pixel passed in this row (the frame column at its
// start); a change prev -> p other than 0 -> 1 is either nothing (p != 0 or prev < 1) or a hole start, which moves lnbd to x - 1
// when prev is a traced pixel and is never traced in this mode; an outer start is skipped while the pixel at lnbd is positive
// (a traced pixel that is not a right end: the scan is inside that border).  The scan is restated as it is written, not replaced
// by a topological "outermost component" rule.
inline int ct_external_rects(const uint8_t* map, size_t step, int w, int h, std::vector<CtRect>* rects)
{
    rects->clear();
    const int pw = w + 2;
    std::vector<signed char> img((size_t)pw * (h + 2), 0);   // one pixel of background all round
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) img[(size_t)(y + 1) * pw + x + 1] = map[(size_t)y * step + x] != 0;
    int deltas[16];
    for (int d = 0; d < 16; ++d) deltas[d] = kCtDy[d & 7] * pw + kCtDx[d & 7];
    std::vector<CtPoint> pts;
    int found = 0;
    for (int y = 1; y <= h; ++y) {
        signed char* row = img.data() + (size_t)y * pw;
        int prev = 0, lnbd = 0;
        for (int x = 1; x <= w; ++x) {
            int p = row[x];
            if (p == prev) continue;
            bool start = true;
            if (!(prev == 0 && p == 1)) {
                if (p != 0 || prev < 1) {
                    start = false;
                } else {
                    if (prev & -2) lnbd = x - 1;
                    start = false;   // a hole start: not traced in this mode
                }
            } else if (row[lnbd] > 0) {
                start = false;
            }
            if (start) {
                pts.clear();
                ct_trace(row + x, deltas, false, CtPoint{x - 1, y - 1}, &pts);
                ++found;
                if (pts.size() >= 3) {
                    int x0 = pts[0].x, x1 = x0, y0 = pts[0].y, y1 = y0;
                    for (const CtPoint& q : pts) {
                        x0 = std::min(x0, q.x); x1 = std::max(x1, q.x);
                        y0 = std::min(y0, q.y); y1 = std::max(y1, q.y);
                    }
                    rects->push_back(CtRect{x0, y0, x1 - x0 + 1, y1 - y0 + 1});
                }
                p = row[x];
            }
            prev = p;
            if (prev & -2) lnbd = x;
        }
    }
    return found;
}

// points [first, first + count) of the list that comes with it, and cv::findContours' four hierarchy links (-1: none)
struct CtNode {
    int first, count, hole;
    int next, prev, child, parent;
};

// cv::findContours(map, RETR_TREE, CHAIN_APPROX_SIMPLE): every border with its hierarchy, in OpenCV's output order [upstream, from
// memory].  The scan and the border following are ct_find_contours'.  The parents are the topological ones: an outer border's
// parent is the hole border of the background region round its component (none for the outer background), a hole border's parent
// is the outer border of the component it lies in - what OpenCV's border numbers give, and what it falls back to by tracing when
// its 7-bit numbers collide.  A hole region (background, 4-connected) is labelled when its border starts: its first pixel in
// raster order comes before every component inside it.  A new border goes to the HEAD of its parent's child list, and the output
// is the pre-order walk: siblings appear last discovered first, as in ct_find_contours' RETR_CCOMP order.
inline void ct_find_contours_tree(const uint8_t* map, size_t step, int w, int h, std::vector<CtPoint>* points, std::vector<CtNode>* nodes)
{
    points->clear();
    nodes->clear();
    const int pw = w + 2;
    std::vector<signed char> img((size_t)pw * (h + 2), 0);   // one pixel of background all round
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) img[(size_t)(y + 1) * pw + x + 1] = map[(size_t)y * step + x] != 0;
    int deltas[16];
    for (int d = 0; d < 16; ++d) deltas[d] = kCtDy[d & 7] * pw + kCtDx[d & 7];

    struct Found {
        int first, count, hole, parent;   // parent: an index of `found`
    };
    std::vector<Found> found;
    std::vector<CtPoint> raw;
    // per foreground pixel: its component's outer border; per background pixel of a hole: the hole's border (indices of `found`)
    std::vector<int32_t> owner((size_t)pw * (h + 2), -1);
    std::vector<int> queue;
    for (int y = 1; y <= h; ++y) {
        int prev = 0;
        for (int x = 1; x <= w; ++x) {
            signed char* row = img.data() + (size_t)y * pw;
            int p = row[x];
            if (p != prev) {
                bool start = true, hole = false;
                if (!(prev == 0 && p == 1)) {
                    hole = true;
                    if (p != 0 || prev < 1) start = false;
                }
                if (start) {
                    const int x0 = x - (hole ? 1 : 0), id = (int)found.size();
                    const int first = (int)raw.size();
                    int parent;
                    if (!hole) {   // the component this border encloses (8-connected); the region to its left says where it lies
                        parent = owner[(size_t)y * pw + x0 - 1];
                        queue.assign(1, y * pw + x0);
                        owner[(size_t)y * pw + x0] = id;
                        while (!queue.empty()) {
                            const int at = queue.back();
                            queue.pop_back();
                            for (int d = 0; d < 8; ++d) {
                                const int to = at + deltas[d];
                                if (img[to] != 0 && owner[to] < 0) {
                                    owner[to] = id;
                                    queue.push_back(to);
                                }
                            }
                        }
                    } else {       // the hole this border encloses (4-connected): it never reaches the frame
                        parent = owner[(size_t)y * pw + x0];
                        queue.assign(1, y * pw + x);
                        owner[(size_t)y * pw + x] = id;
                        while (!queue.empty()) {
                            const int at = queue.back();
                            queue.pop_back();
                            for (int d = 0; d < 8; d += 2) {
                                const int to = at + deltas[d];
                                if (to < 0 || to >= (int)img.size()) continue;
                                if (img[to] == 0 && owner[to] < 0) {
                                    owner[to] = id;
                                    queue.push_back(to);
                                }
                            }
                        }
                    }
                    ct_trace(row + x0, deltas, hole, CtPoint{x0 - 1, y - 1}, &raw);
                    found.push_back({first, (int)raw.size() - first, hole ? 1 : 0, parent});
                    p = row[x];
                }
            }
            prev = p;
        }
    }
    // child lists, last discovered first; then the pre-order walk
    const int n = (int)found.size();
    std::vector<int> head((size_t)n + 1, -1), sibling((size_t)n, -1);   // head[n]: the top level
    for (int i = 0; i < n; ++i) {
        const int par = found[i].parent < 0 ? n : found[i].parent;
        sibling[i] = head[par];
        head[par] = i;
    }
    std::vector<int> out_of((size_t)n, -1), order, stack;
    for (int i = head[n]; i >= 0; i = sibling[i]) stack.push_back(i);
    std::reverse(stack.begin(), stack.end());
    while (!stack.empty()) {
        const int i = stack.back();
        stack.pop_back();
        out_of[i] = (int)order.size();
        order.push_back(i);
        const size_t at = stack.size();
        for (int c = head[i]; c >= 0; c = sibling[c]) stack.push_back(c);
        std::reverse(stack.begin() + at, stack.end());
    }
    nodes->resize((size_t)n);
    std::vector<int> last_child((size_t)n + 1, -1);   // per parent, the output index of the child emitted before
    for (int k = 0; k < n; ++k) {
        const Found& f = found[order[k]];
        CtNode& nd = (*nodes)[k];
        nd = CtNode{(int)points->size(), f.count, f.hole, -1, -1, -1, f.parent < 0 ? -1 : out_of[f.parent]};
        points->insert(points->end(), raw.begin() + f.first, raw.begin() + f.first + f.count);
        const int par = f.parent < 0 ? n : f.parent;
        if (last_child[par] >= 0) {
            nd.prev = last_child[par];
            (*nodes)[last_child[par]].next = k;
        } else if (f.parent >= 0) {
            (*nodes)[out_of[f.parent]].child = k;
        }
        last_child[par] = k;
    }
}

// RemoveChildrenContours with ContourChildrenCount and CheckHierarhyLevelRecursively (imageLibCommon.cpp:483-523, 641-780),
// literally, the recursion unrolled: the walk starts at contour 0 and follows the `next` links; a contour of fewer than 3 points is
// ignored (and its children never visited); one with no descendants is approved; with fewer than 6 descendants it is approved and
// its direct children are ignored (their own children are never visited); otherwise it is ignored and the walk descends into its
// children.  approved[i] = 1 for the contours the reference keeps, in index order.  Needs nodes in pre-order (a parent before its
// children), which ct_find_contours_tree gives.
inline void ct_remove_children(const std::vector<CtNode>& nodes, std::vector<uint8_t>* approved)
{
    const int n = (int)nodes.size();
    approved->assign((size_t)n, 0);
    if (n == 0) return;
    std::vector<int> descendants((size_t)n, 0);
    for (int i = n - 1; i >= 0; --i)
        if (nodes[i].parent >= 0) descendants[nodes[i].parent] += descendants[i] + 1;
    std::vector<signed char> state((size_t)n, 0);   // 0 not visited, 1 approved, -1 ignored
    std::vector<int> starts(1, 0);
    while (!starts.empty()) {
        int cur = starts.back();
        starts.pop_back();
        while (cur >= 0) {
            const CtNode& nd = nodes[cur];
            if (nd.count < 3) {
                state[cur] = -1;
            } else if (descendants[cur] < 6) {
                state[cur] = 1;
                for (int c = nd.child; c >= 0; c = nodes[c].next) state[c] = -1;
            } else {
                state[cur] = -1;
                starts.push_back(nd.child);
            }
            cur = nd.next;
        }
    }
    for (int i = 0; i < n; ++i) (*approved)[i] = state[i] == 1;
}

// cv::approxPolyDP(src, dst, eps, closed = true) on integer points; dst has room for n points; returns the new count.
inline int ct_approx_closed(const CtPoint* src, int n, double eps, CtPoint* dst)
{
    if (n == 0) return 0;
    const int count = n;
    eps *= eps;
    std::vector<std::pair<int, int>> stack;   // slices (start, end)
    int new_count = 0, pos = 0, right_start = 0;
    bool le_eps = false;
    CtPoint start_pt{-1000000, -1000000}, pt{0, 0};
    auto read = [&](int& at) {
        const CtPoint r = src[at];
        if (++at >= count) at = 0;
        return r;
    };
    // 1. three rounds of "farthest from the current start"
    for (int i = 0; i < 3; ++i) {
        double max_dist = 0;
        pos = (pos + right_start) % count;
        start_pt = read(pos);
        for (int j = 1; j < count; ++j) {
            pt = read(pos);
            const double dx = pt.x - start_pt.x, dy = pt.y - start_pt.y;
            const double dist = dx * dx + dy * dy;
            if (dist > max_dist) {
                max_dist = dist;
                right_start = j;
            }
        }
        le_eps = max_dist <= eps;
    }
    // 2. the two halves
    if (!le_eps) {
        const int s0 = pos % count, s1 = (right_start + s0) % count;
        stack.push_back({s1, s0});   // the right slice, popped second
        stack.push_back({s0, s1});
    } else {
        dst[new_count++] = start_pt;
    }
    // 3. split while a point lies farther than eps from the chord
    while (!stack.empty()) {
        std::pair<int, int> slice = stack.back();
        stack.pop_back();
        const CtPoint end_pt = src[slice.second];
        pos = slice.first;
        start_pt = read(pos);
        if (pos != slice.second) {
            const double dx = end_pt.x - start_pt.x, dy = end_pt.y - start_pt.y;
            double max_dist = 0;
            while (pos != slice.second) {
                pt = read(pos);
                const double dist = std::fabs((pt.y - start_pt.y) * dx - (pt.x - start_pt.x) * dy);
                if (dist > max_dist) {
                    max_dist = dist;
                    right_start = (pos + count - 1) % count;
                }
            }
            le_eps = max_dist * max_dist <= eps * (dx * dx + dy * dy);
        } else {
            le_eps = true;
            start_pt = src[slice.first];
        }
        if (le_eps) {
            dst[new_count++] = start_pt;
        } else {
            stack.push_back({right_start, slice.second});
            stack.push_back({slice.first, right_start});
        }
    }
    // 4. clean-up: drop a point that lies on the line through its neighbours, going forwards
    const int kept = new_count;
    auto read_dst = [&](int& at) {
        const CtPoint r = dst[at];
        if (++at >= kept) at = 0;
        return r;
    };
    pos = kept - 1;
    start_pt = read_dst(pos);
    int wpos = pos;
    pt = read_dst(pos);
    for (int i = 0; i < kept && new_count > 2; ++i) {
        const CtPoint end_pt = read_dst(pos);
        const double dx = end_pt.x - start_pt.x, dy = end_pt.y - start_pt.y;
        const double dist = std::fabs((pt.x - start_pt.x) * dy - (pt.y - start_pt.y) * dx);
        const int inner = (pt.x - start_pt.x) * (end_pt.x - pt.x) + (pt.y - start_pt.y) * (end_pt.y - pt.y);
        if (dist * dist <= 0.5 * eps * (dx * dx + dy * dy) && dx != 0 && dy != 0 && inner >= 0) {
            --new_count;
            dst[wpos] = start_pt = end_pt;
            if (++wpos >= kept) wpos = 0;
            pt = read_dst(pos);
            ++i;
            continue;
        }
        dst[wpos] = start_pt = pt;
        if (++wpos >= kept) wpos = 0;
        pt = end_pt;
    }
    return new_count;
}

// cv::contourArea(points), not oriented
inline double ct_area(const CtPoint* p, int n)
{
    if (n == 0) return 0.0;
    double a = 0;
    CtPoint prev = p[n - 1];
    for (int i = 0; i < n; ++i) {
        a += (double)prev.x * p[i].y - (double)p[i].x * prev.y;
        prev = p[i];
    }
    return std::fabs(a * 0.5);
}

inline int64_t ct_cross(const CtPoint& o, const CtPoint& a, const CtPoint& b)
{
    return (int64_t)(a.x - o.x) * (b.y - o.y) - (int64_t)(a.y - o.y) * (b.x - o.x);
}

// The convex hull of four points has four vertices: fills `order` with the hull's cycle, oriented so that the sum of
// x_i y_{i+1} - x_{i+1} y_i is positive (top left -> top right -> bottom right -> bottom left on the screen), starting at the point
// of smallest x, then smallest y.  Monotone chain with collinear points dropped; exact.
inline bool ct_hull4(const CtPoint q[4], int order[4])
{
    int idx[4] = {0, 1, 2, 3};
    std::sort(idx, idx + 4, [&](int a, int b) { return q[a].x != q[b].x ? q[a].x < q[b].x : q[a].y < q[b].y; });
    int hull[8], k = 0;
    for (int i = 0; i < 4; ++i) {   // the chain below the points on the screen's y, which is the positive orientation asked for
        while (k >= 2 && ct_cross(q[hull[k - 2]], q[hull[k - 1]], q[idx[i]]) <= 0) --k;
        hull[k++] = idx[i];
    }
    for (int i = 2, t = k + 1; i >= 0; --i) {
        while (k >= t && ct_cross(q[hull[k - 2]], q[hull[k - 1]], q[idx[i]]) <= 0) --k;
        hull[k++] = idx[i];
    }
    if (k - 1 != 4) return false;
    for (int i = 0; i < 4; ++i) order[i] = hull[i];
    return true;
}

inline double ct_norm(const CtPoint& a, const CtPoint& b)   // cv::norm(a - b)
{
    const double dx = a.x - b.x, dy = a.y - b.y;
    return std::sqrt(dx * dx + dy * dy);
}

// angleBetweenLinesInDegree (autoCropUtils.cpp:40-55), 3.14 included
inline double ct_angle(const CtPoint& s1, const CtPoint& e1, const CtPoint& s2, const CtPoint& e2)
{
    const double a1 = std::atan2((double)(s1.y - e1.y), (double)(s1.x - e1.x));
    const double a2 = std::atan2((double)(s2.y - e2.y), (double)(s2.x - e2.x));
    double r = (a2 - a1) * 180.0 / 3.14;
    if (r < 0.0) r += 360.0;
    if (r > 180.0) r = 360.0 - r;
    return r;
}

// The reference's loop over one border (autoCropUtils.cpp:184-191): approximations with eps = 1, 2, ... until at most four points
// remain; `cur` holds the border on entry and the polygon on return.
inline void ct_reduce(std::vector<CtPoint>* cur, std::vector<CtPoint>* tmp)
{
    double eps = 1.0;
    while (cur->size() > 4) {
        tmp->resize(cur->size());
        tmp->resize((size_t)ct_approx_closed(cur->data(), (int)cur->size(), eps, tmp->data()));
        eps += 1.0;
        cur->swap(*tmp);
    }
}

// findDocumentContour (autoCropUtils.cpp:155-262): the corners in the polygon's own order
inline bool ct_document_quad(const uint8_t* map, size_t step, int w, int h, CtPoint quad[4])
{
    std::vector<CtPoint> points, cur, tmp;
    std::vector<CtContour> contours;
    ct_find_contours(map, step, w, h, &points, &contours);
    const int cols_rows = w * h;   // the reference's int product
    double min_area = (double)cols_rows * 0.05;
    bool have = false;
    for (const CtContour& c : contours) {
        cur.assign(points.begin() + c.first, points.begin() + c.first + c.count);
        ct_reduce(&cur, &tmp);
        if (cur.size() < 4) continue;
        const CtPoint* p = cur.data();
        const double area = ct_area(p, 4);
        double side1 = ct_norm(p[0], p[1]), side2 = ct_norm(p[1], p[2]), side3 = ct_norm(p[2], p[3]), side4 = ct_norm(p[3], p[0]);
        if (side1 < side3) std::swap(side1, side3);
        if (side2 < side4) std::swap(side2, side4);
        if (side3 / side1 < 0.85) continue;
        if (side4 / side2 < 0.85) continue;
        if (ct_angle(p[0], p[1], p[2], p[3]) < 160.0) continue;
        if (ct_angle(p[1], p[2], p[3], p[0]) < 160.0) continue;
        if (area > cols_rows || area < min_area) continue;
        if (area > min_area) {
            min_area = area;
            for (int i = 0; i < 4; ++i) quad[i] = p[i];
            have = true;
        }
    }
    int order[4];
    return have && ct_hull4(quad, order);
}

// scaleContour, then cropVerticesOrdering (autoCropUtils.cpp:269-348); false: the corners are not in strictly convex position
inline bool ct_finish(const int32_t quad[8], int map_w, int map_h, int src_w, int src_h, float out[8])
{
    const CtPoint q[4] = {{quad[0], quad[1]}, {quad[2], quad[3]}, {quad[4], quad[5]}, {quad[6], quad[7]}};
    int order[4];
    if (!ct_hull4(q, order)) return false;
    const float xs = (float)src_w / (float)map_w, ys = (float)src_h / (float)map_h;
    float px[4], py[4];
    for (int i = 0; i < 4; ++i) {
        px[i] = (float)q[order[i]].x * xs;
        py[i] = (float)q[order[i]].y * ys;
    }
    int first = 0;
    double best = px[0] * px[0] + py[0] * py[0];   // float products and sum, as the reference writes them
    for (int i = 1; i < 4; ++i) {
        const double d = px[i] * px[i] + py[i] * py[i];
        if (d < best) {
            first = i;
            best = d;
        }
    }
    for (int i = 0; i < 4; ++i) {
        out[2 * i] = px[(first + i) & 3];
        out[2 * i + 1] = py[(first + i) & 3];
    }
    return true;
}

}  // namespace prl_hip
