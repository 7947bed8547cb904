// components.h — rule R (include/prl_hip.h, next to prl_hip_external_rects) and the labelling it rests on, as plain loops: the
// label plane components.hip builds (for every pixel the smallest linear index of its own-class component, foreground 8- or
// 4-connected, background 4-connected), the outer flags, the numbering of the roots, the statistics and the kept filter.  The
// pieces the kernels share (the label word's layout, the kept filter) are here once; the loops are the yardstick of
// tests/cpp/test_components.cpp and tests/test_components_cpu.py, never the product path.  Restated independently, with flood
// fills, in tests/components_ref.py.  Plain C++17: no HIP header, no environment, no I/O.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PRL_CC_FN __host__ __device__ inline
#else
#define PRL_CC_FN inline
#endif

namespace prl_hip {

constexpr int kCcTile = 32;   // the side of the tile a workgroup of components.hip labels in LDS

// A word of the label plane: bits 0 .. 29 an index (a page has at most 2^30 pixels), bit 30 a flag kept in a ROOT's own word only.
// Until the numbering the index is the pixel's root and the flag marks an outer background root; the numbering replaces a numbered
// foreground root's word by flag | its number on the page.
constexpr int32_t kCcIndex = 0x3fffffff, kCcFlag = 0x40000000;

struct CcStat {
    int32_t left, top, width, height, area;
};

// rule R's kept filter: everything but a straight one-pixel line (a contour of fewer than 3 points), a single pixel included
PRL_CC_FN bool cc_kept(int bw, int bh, int area)
{
    const int longer = bw > bh ? bw : bh, shorter = bw > bh ? bh : bw;
    return !(area == longer && (shorter == 1 || bw == bh));
}

inline int32_t cc_find(const std::vector<int32_t>& lab, int32_t p)
{
    while (lab[(size_t)p] != p) p = lab[(size_t)p];
    return p;
}

inline void cc_union(std::vector<int32_t>& lab, int32_t a, int32_t b)
{
    a = cc_find(lab, a);
    b = cc_find(lab, b);
    if (a != b) lab[(size_t)std::max(a, b)] = std::min(a, b);   // the smaller index stays the root: a root is its set's first pixel
}

// The label plane: labels[y * w + x] = the smallest linear index of the pixel's own-class component.
inline void cc_label_plane(const uint8_t* map, size_t step, int w, int h, int connectivity, std::vector<int32_t>* labels)
{
    std::vector<int32_t>& lab = *labels;
    lab.resize((size_t)w * h);
    for (size_t i = 0; i < lab.size(); ++i) lab[i] = (int32_t)i;
    auto fg = [&](int x, int y) { return map[(size_t)y * step + x] != 0; };
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const bool f = fg(x, y);
            const int32_t p = y * w + x;
            if (x > 0 && fg(x - 1, y) == f) cc_union(lab, p, p - 1);
            if (y > 0 && fg(x, y - 1) == f) cc_union(lab, p, p - w);
            if (f && connectivity == 8 && y > 0) {
                if (x > 0 && fg(x - 1, y - 1)) cc_union(lab, p, p - w - 1);
                if (x + 1 < w && fg(x + 1, y - 1)) cc_union(lab, p, p - w + 1);
            }
        }
    for (size_t i = 0; i < lab.size(); ++i) lab[i] = cc_find(lab, (int32_t)i);
}

// Numbers the foreground components of a label plane in increasing order of first pixel, all of them or (external_only) rule R's
// external ones: ids[p] = the number from 0 of the component of foreground pixel p, -1 for the background and for a component that
// is not numbered; stats: one entry per number.  Returns how many.
inline int cc_number(const uint8_t* map, size_t step, int w, int h, const std::vector<int32_t>& lab, bool external_only,
                     std::vector<int32_t>* ids, std::vector<CcStat>* stats)
{
    const size_t n = (size_t)w * h;
    auto fg = [&](size_t p) { return map[p / (size_t)w * step + p % (size_t)w] != 0; };
    std::vector<uint8_t> outer(n, 0);   // per background root
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            if ((x == 0 || y == 0 || x == w - 1 || y == h - 1) && !fg((size_t)y * w + x)) outer[(size_t)lab[(size_t)y * w + x]] = 1;
    std::vector<int32_t> number(n, -1);   // per foreground root
    int count = 0;
    for (size_t p = 0; p < n; ++p)
        if (fg(p) && lab[p] == (int32_t)p && (!external_only || p % (size_t)w == 0 || outer[(size_t)lab[p - 1]])) number[p] = count++;
    ids->assign(n, -1);
    stats->assign((size_t)count, CcStat{w, h, -1, -1, 0});   // left, top, then right and bottom until the end
    for (size_t p = 0; p < n; ++p) {
        if (!fg(p) || number[(size_t)lab[p]] < 0) continue;
        const int id = number[(size_t)lab[p]], x = (int)(p % (size_t)w), y = (int)(p / (size_t)w);
        (*ids)[p] = id;
        CcStat& s = (*stats)[(size_t)id];
        s.left = std::min(s.left, x); s.width = std::max(s.width, x);
        s.top = std::min(s.top, y); s.height = std::max(s.height, y);
        ++s.area;
    }
    for (CcStat& s : *stats) {
        s.width -= s.left - 1;
        s.height -= s.top - 1;
    }
    return count;
}

// cv::connectedComponentsWithStats' content in this library's order: labels 0 / 1 .. K by first pixel, the five numbers of each
inline int cc_components(const uint8_t* map, size_t step, int w, int h, int connectivity, std::vector<int32_t>* labels,
                         std::vector<CcStat>* stats)
{
    std::vector<int32_t> lab, ids;
    cc_label_plane(map, step, w, h, connectivity, &lab);
    const int k = cc_number(map, step, w, h, lab, false, &ids, stats);
    labels->resize(ids.size());
    for (size_t p = 0; p < ids.size(); ++p) (*labels)[p] = ids[p] + 1;
    return k;
}

// Rule R: the rectangles (x, y, w, h flattened) of the kept external components in order; returns n_found.
inline int cc_external_rects(const uint8_t* map, size_t step, int w, int h, std::vector<int32_t>* rects)
{
    std::vector<int32_t> lab, ids;
    std::vector<CcStat> stats;
    cc_label_plane(map, step, w, h, 8, &lab);
    const int found = cc_number(map, step, w, h, lab, true, &ids, &stats);
    rects->clear();
    for (const CcStat& s : stats)
        if (cc_kept(s.width, s.height, s.area)) rects->insert(rects->end(), {s.left, s.top, s.width, s.height});
    return found;
}

}  // namespace prl_hip
