// border.hip — the border detectors prl::documentContour (src/border_detection/autoCrop.cpp:43-175) and prl::findHoughLineContour
// (houghLine.cpp:177-256) on one procedure, edge_map_batch: a front stage yields the pages cv::Canny(25, 50) reads (canny.hip); the
// maps go to the caller, or stay in the workspace for a tail that searches them for a quad (contour.h, houghline.h: host code).
// The arithmetic is stated in include/prl_hip.h ("pyramid, edge map, resize", "document contour", "Hough lines") and restated in
// tests/edges_ref.py, tests/contour_ref.py and tests/houghline_ref.py.
#include <algorithm>
#include <cmath>
#include <vector>

#include "contour.h"
#include "houghline.h"
#include "prl_internal.h"

namespace prl_hip {

namespace {

template <int CH>
__global__ __launch_bounds__(256) void k_take_channel(PageSet src, PageSetOut dst, int W, const int* __restrict__ channel)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, page = blockIdx.z;
    if (x >= W) return;
    dst.page(page)[(size_t)y * dst.step + x] = src.page(page)[(size_t)y * src.step + (size_t)x * CH + channel[page]];
}

// ---- the shared procedure ----------------------------------------------------------------------------------------------------

// What a detector runs in front of cv::Canny: a map of map_w x map_h per page from `channels` channels, `scratch_per_page` bytes
// at the head of the workspace, `copy_per_page` bytes of the `small` block and as many pinned.  `run` enqueues the stage for the
// n pages from `first` on, of a call cut into chunks of `chunk` pages: `pages` come as the source's and leave as those Canny reads.
struct EdgeFront {
    int map_w = 0, map_h = 0, channels = 1;
    size_t scratch_per_page = 0, copy_per_page = 0;
    std::function<int(int first, int n, int chunk, const WorkScope& w, PageSet& pages)> run;
};

// What a detector hangs on a chunk (none: `run` is empty): the maps stay in the workspace (a.dst is null), tight pages of
// r256(map_w * map_h) bytes at the head of a tail of `scratch_per_page` bytes per page behind the edge detector's own work, and
// `run` gets every chunk once its maps are enqueued; cv::Canny has waited for the stream, so the `small` and pinned blocks are free.
struct EdgeTail {
    size_t scratch_per_page = 0, small_per_page = 0, pinned_per_page = 0;
    std::function<int(int first, int n, uint8_t* tail, const WorkScope& w)> run;
};

// the workspace of a chunk: [front stage | canny work | tail]
int edge_map_batch(const PageArgs& a, const EdgeFront& f, void* stream, const EdgeTail& t)
{
    if (a.n_pages == 0) return PRL_OK;
    const size_t per_page = f.scratch_per_page + t.scratch_per_page;
    const int chunk = canny_pages_per_chunk(a.n_pages, f.map_w, f.map_h, per_page);
    const size_t canny_bytes = r256(canny_work_bytes(chunk, f.map_w, f.map_h));
    WorkScope w;
    int st = w.open(stream, per_page * (size_t)chunk + canny_bytes, std::max(f.copy_per_page, t.small_per_page) * (size_t)chunk,
                    std::max(canny_pinned_bytes(chunk), std::max(f.copy_per_page, t.pinned_per_page) * (size_t)chunk));
    if (st != PRL_OK) return st;
    uint8_t* canny_work = w.scratch() + f.scratch_per_page * (size_t)chunk;
    uint8_t* tail_work = canny_work + canny_bytes;
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int n = std::min(chunk, a.n_pages - first);
        PageSet cur = src_pages(a, first);
        if ((st = f.run(first, n, chunk, w, cur)) != PRL_OK) return st;
        // (canny_run synchronises the stream before it touches the pinned block again: a front stage's last copy has left it)
        const PageSetOut maps = t.run ? page_set_out(tail_work, r256((size_t)f.map_w * (size_t)f.map_h), (size_t)f.map_w) : dst_pages(a, first);
        st = canny_run(f.map_w, f.map_h, 25, 50, cur, maps, n, canny_work, w.pinned<unsigned>(), w.stream, f.channels);
        if (st != PRL_OK) return st;
        if (t.run && (st = t.run(first, n, tail_work, w)) != PRL_OK) return st;
    }
    return PRL_OK;
}

// ---- prl::documentContour: the edge map (autoCrop.cpp:67-101), the quad search on the host (contour.h), one retry after a closing

void edges_geometry(int W, int H, int* levels, int* ow, int* oh)
{
    int n = 0, longSide = std::max(W, H);
    while (longSide / 2 >= 256) {   // autoCrop.cpp:74-81
        W = (W + 1) / 2;
        H = (H + 1) / 2;
        longSide = std::max(W, H);
        ++n;
    }
    *levels = n;
    *ow = W;
    *oh = H;
}

// the first maximum of cv::meanStdDev's standard deviations, from one page's per-channel bins
int most_informative_channel(const unsigned* hist, int channels, double pixels)
{
    int best = 0;
    double best_sd = -1;
    for (int ch = 0; ch < channels; ++ch) {
        unsigned long long s1 = 0, s2 = 0;
        for (int v = 0; v < 256; ++v) {
            s1 += (unsigned long long)hist[ch * 256 + v] * (unsigned)v;
            s2 += (unsigned long long)hist[ch * 256 + v] * (unsigned)(v * v);
        }
        const double mean = (double)s1 / pixels;
        const double sd = std::sqrt(std::max((double)s2 / pixels - mean * mean, 0.0));
        if (ch == 0 || best_sd < sd) {   // std::max_element keeps the first of equals
            best = ch;
            best_sd = sd;
        }
    }
    return best;
}

// EMPTY, BAD_CHANNELS, then BAD_ARG: the source's rows, a null result pointer (`results`: none is), the sides
int contour_checks(const PageArgs& a, int channels, bool results, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels != 1 && channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, 0, batch)) != PRL_OK) return st;
    return results ? pages_sides_ok(a) : PRL_ERR_BAD_ARG;
}

// the same, then the destination of the map
int doc_checks(const PageArgs& a, int channels, const int32_t* out_channel, bool batch)
{
    const int st = contour_checks(a, channels, out_channel != nullptr, batch);
    if (st != PRL_OK) return st;
    int levels, ow, oh;
    edges_geometry(a.width, a.height, &levels, &ow, &oh);
    return resized_dst_ok(a, 1, ow, oh, batch);
}

// front stage: [pyramid work | the last level | the chosen channel]; `small` and pinned: [bins of a chunk | channels]
int doc_batch(const PageArgs& a, int channels, int32_t* out_channel, void* stream, const EdgeTail& tail = {})
{
    int levels, ow, oh;
    edges_geometry(a.width, a.height, &levels, &ow, &oh);
    const size_t pyr_bytes = levels ? pyr_work_per_page(a.width, a.height, channels, levels) : 0;
    const size_t last_bytes = levels ? r256((size_t)ow * channels * (size_t)oh) : 0;   // the last level
    const size_t gray_bytes = channels > 1 ? r256((size_t)ow * (size_t)oh) : 0;        // the chosen channel
    const size_t bins = (size_t)channels * 256 * sizeof(unsigned);
    EdgeFront f{ow, oh, 1, pyr_bytes + last_bytes + gray_bytes, channels > 1 ? bins + sizeof(int) : 0};
    f.run = [&](int first, int n, int chunk, const WorkScope& w, PageSet& cur) -> int {
        const hipStream_t hs = w.stream;
        uint8_t* last = w.scratch() + pyr_bytes * (size_t)chunk;
        uint8_t* gray = last + last_bytes * (size_t)chunk;
        if (levels) {
            const PageSetOut l = page_set_out(last, last_bytes, (size_t)ow * channels);
            const int st = pyr_run(channels, cur, a.width, a.height, levels, l, n, w.scratch(), hs);
            if (st != PRL_OK) return st;
            cur = as_source(l);
        }
        if (channels > 1) {
            unsigned* d_hist = w.small<unsigned>();
            int* d_ch = reinterpret_cast<int*>(w.small() + bins * (size_t)chunk);
            const int st = prl_hip_histogram_batch_device(n, channels, cur.base, cur.page_stride, cur.step, ow, oh, d_hist, hs);
            if (st != PRL_OK) return st;
            // the one read-back of the call per chunk: the bins come down, the chosen channels go up
            unsigned* h_hist = w.pinned<unsigned>();
            int* h_ch = reinterpret_cast<int*>(w.pinned() + bins * (size_t)chunk);
            PRL_HIP_CHECK(hipMemcpyAsync(h_hist, d_hist, bins * (size_t)n, hipMemcpyDeviceToHost, hs));
            PRL_HIP_CHECK(hipStreamSynchronize(hs));
            for (int i = 0; i < n; ++i) {
                h_ch[i] = most_informative_channel(h_hist + (size_t)i * channels * 256, channels, (double)ow * (double)oh);
                if (out_channel) out_channel[first + i] = h_ch[i];
            }
            PRL_HIP_CHECK(hipMemcpyAsync(d_ch, h_ch, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, hs));
            const PageSetOut gp = page_set_out(gray, gray_bytes, (size_t)ow);
            const dim3 grid((unsigned)((ow + 255) / 256), (unsigned)oh, (unsigned)n);
            if (channels == 3) hipLaunchKernelGGL(k_take_channel<3>, grid, dim3(256), 0, hs, cur, gp, ow, d_ch);
            else hipLaunchKernelGGL(k_take_channel<4>, grid, dim3(256), 0, hs, cur, gp, ow, d_ch);
            PRL_HIP_CHECK(hipGetLastError());
            cur = as_source(gp);
        } else if (out_channel) {
            for (int i = 0; i < n; ++i) out_channel[first + i] = 0;
        }
        return PRL_OK;
    };
    return edge_map_batch(a, f, stream, tail);
}

int contour_batch(const PageArgs& a, int channels, float* quads, int32_t* found, int32_t* out_try, void* stream)
{
    int levels, ow, oh;
    edges_geometry(a.width, a.height, &levels, &ow, &oh);
    const int from_w = a.width >> levels, from_h = a.height >> levels;   // autoCrop.cpp:83: cols / 2^levels, not the pyramid's size
    const size_t map_bytes = r256((size_t)ow * (size_t)oh);
    // scratch: the map, then the closing's two planes; `small`: the table of the pages the closing takes; pinned: the map and the table
    EdgeTail tail{3 * map_bytes, sizeof(uint8_t*), map_bytes + sizeof(uint8_t*)};
    std::vector<int32_t> corners, again;
    tail.run = [&](int first, int n, uint8_t* maps, const WorkScope& w) -> int {
        uint8_t* h_maps = w.pinned();
        PRL_HIP_CHECK(hipMemcpyAsync(h_maps, maps, map_bytes * (size_t)n, hipMemcpyDeviceToHost, w.stream));
        PRL_HIP_CHECK(hipStreamSynchronize(w.stream));
        corners.assign((size_t)n * 8, 0);
        auto search = [&](int i) {
            CtPoint q[4];
            const bool ok = ct_document_quad(h_maps + map_bytes * (size_t)i, (size_t)ow, ow, oh, q);
            found[first + i] = ok ? 1 : 0;
            for (int k = 0; ok && k < 4; ++k) {
                corners[(size_t)i * 8 + 2 * k] = q[k].x;
                corners[(size_t)i * 8 + 2 * k + 1] = q[k].y;
            }
        };
        host_pool_for(n, search);
        again.clear();
        for (int i = 0; i < n; ++i) {
            if (out_try) out_try[first + i] = found[first + i] ? 0 : 1;
            if (!found[first + i]) again.push_back(i);
        }
        if (!again.empty()) {   // autoCrop.cpp:118-125, first round: CLOSE(2 x 2, iterations 2) on these pages only, in place
            const int m = (int)again.size();
            uint8_t** h_table = reinterpret_cast<uint8_t**>(h_maps + map_bytes * (size_t)n);
            for (int k = 0; k < m; ++k) h_table[k] = maps + map_bytes * (size_t)again[k];
            uint8_t** d_table = w.small<uint8_t*>();
            PRL_HIP_CHECK(hipMemcpyAsync(d_table, h_table, sizeof(uint8_t*) * (size_t)m, hipMemcpyHostToDevice, w.stream));
            const int st = gmorph_close_rect_table_run(2, 2, ow, oh, d_table, (size_t)ow, m, maps + map_bytes * (size_t)n, w.stream);
            if (st != PRL_OK) return st;
            for (int k = 0; k < m; ++k)
                PRL_HIP_CHECK(hipMemcpyAsync(h_maps + map_bytes * (size_t)again[k], h_table[k], (size_t)ow * (size_t)oh, hipMemcpyDeviceToHost,
                                             w.stream));
            PRL_HIP_CHECK(hipStreamSynchronize(w.stream));
            host_pool_for(m, [&](int k) { search(again[k]); });
        }
        for (int i = 0; i < n; ++i) {
            float* out = quads + (size_t)(first + i) * 8;
            if (!found[first + i] || !ct_finish(&corners[(size_t)i * 8], from_w, from_h, a.width, a.height, out)) {
                found[first + i] = 0;
                std::fill(out, out + 8, 0.0f);
            }
        }
        return PRL_OK;
    };
    return doc_batch(a, channels, nullptr, stream, tail);
}

// ---- prl::findHoughLineContour (houghLine.cpp:177-256): three medianBlur(3), three medianBlur(5), cv::Canny(25, 50) on the page's
// own channels, cv::HoughLines(1, pi / 180, 50) (hough.hip), the line filter and the quad search on the host (houghline.h) --------

int hough_edges_checks(const PageArgs& a, int channels, bool with_dst, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels != 1 && channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, with_dst ? 1 : 0, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    return with_dst && batch ? pages_overlap_ok(a, channels, 1, false) : PRL_OK;
}

// front stage: two images per page, the median passes go to and fro
int hough_edges_batch(const PageArgs& a, int channels, void* stream, const EdgeTail& tail = {})
{
    const int W = a.width, H = a.height;
    const size_t img_bytes = r256((size_t)W * channels * (size_t)H);
    EdgeFront f{W, H, channels, 2 * img_bytes};   // houghLine.cpp:215-218: Canny on the page's own channels
    f.run = [&](int, int n, int chunk, const WorkScope& w, PageSet& cur) -> int {
        const PageSetOut p[2] = {page_set_out(w.scratch(), img_bytes, (size_t)W * channels),
                                 page_set_out(w.scratch() + img_bytes * (size_t)chunk, img_bytes, (size_t)W * channels)};
        for (int pass = 0; pass < 6; ++pass) {   // houghLine.cpp:199-206
            const int st = median_pass_pages(W, H, channels, pass < 3 ? 3 : 5, cur, p[pass & 1], n, w.stream);
            if (st != PRL_OK) return st;
            cur = as_source(p[pass & 1]);
        }
        return PRL_OK;
    };
    return edge_map_batch(a, f, stream, tail);
}

int hough_contour_checks(const PageArgs& a, int channels, const int32_t* quads, const int32_t* found, bool batch)
{
    const int st = hough_edges_checks(a, channels, false, batch);
    if (st != PRL_OK) return st;
    return !quads || !found ? PRL_ERR_BAD_ARG : PRL_OK;
}

int hough_contour_batch(const PageArgs& a, int channels, int32_t* quads, int32_t* found, int32_t* out_lines, void* stream)
{
    const HoughPlan p = hough_plan(a.width, a.height);
    const size_t map_bytes = r256((size_t)a.width * (size_t)a.height);
    EdgeTail tail{map_bytes + hough_work_per_page(p), 2 * sizeof(unsigned)};
    std::vector<std::vector<float>> lines;
    tail.run = [&](int first, int n, uint8_t* maps, const WorkScope& w) -> int {
        lines.assign((size_t)n, std::vector<float>());
        // the one read-back of the chunk: the sorted line lists (houghLine.cpp:227-229, threshold 50)
        const int st = hough_lines_run(p, page_set(maps, map_bytes, (size_t)a.width), n, 50, maps + map_bytes * (size_t)n, w,
                                       [&](int i, const HlPeak* pk, size_t count) {
                                           lines[(size_t)i].resize(2 * count);
                                           for (size_t k = 0; k < count; ++k)
                                               hl_line_of(pk[k].cell, p.numrho, &lines[(size_t)i][2 * k], &lines[(size_t)i][2 * k + 1]);
                                       });
        if (st != PRL_OK) return st;
        host_pool_for(n, [&](int i) {
            int32_t* q = quads + (size_t)(first + i) * 8;
            std::fill(q, q + 8, 0);
            const int count = (int)std::min<size_t>(lines[(size_t)i].size() / 2, 0x7fffffff);
            found[first + i] = hl_quad(lines[(size_t)i].data(), count, a.width, a.height, q) ? 1 : 0;
            if (out_lines) out_lines[first + i] = count;
        });
        return PRL_OK;
    };
    return hough_edges_batch(a, channels, stream, tail);
}

}  // namespace
}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_document_edges_geometry(int width, int height, int* levels, int* out_w, int* out_h)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!levels || !out_w || !out_h) return PRL_ERR_BAD_ARG;
    edges_geometry(width, height, levels, out_w, out_h);
    return PRL_OK;
}

int prl_hip_document_edges_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                        int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, int32_t* out_channel,
                                        void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    const int st = doc_checks(a, channels, out_channel, true);
    return st != PRL_OK ? st : doc_batch(a, channels, out_channel, stream);
}

int prl_hip_document_edges_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step,
                                int32_t* out_channel)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = doc_checks(a, channels, out_channel, false);
    if (st != PRL_OK) return st;
    int levels, ow, oh;
    edges_geometry(width, height, &levels, &ow, &oh);
    return stage_host_pages(a, channels, 1, ow, oh, [&](const PageArgs& page, hipStream_t s) { return doc_batch(page, channels, out_channel, s); });
}

int prl_hip_find_contours(const uint8_t* map, size_t step, int width, int height, int32_t* points, int max_points, int32_t* contours,
                          int max_contours, int* n_points, int* n_contours)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!map || step < (size_t)width || !n_points || !n_contours || max_points < 0 || max_contours < 0 || (max_points && !points) ||
        (max_contours && !contours))
        return PRL_ERR_BAD_ARG;
    std::vector<CtPoint> pts;
    std::vector<CtContour> cs;
    ct_find_contours(map, step, width, height, &pts, &cs);
    *n_points = (int)pts.size();
    *n_contours = (int)cs.size();
    if ((int)pts.size() > max_points || (int)cs.size() > max_contours) return PRL_OK;   // the counts alone: call again with room
    for (size_t i = 0; i < pts.size(); ++i) {
        points[2 * i] = pts[i].x;
        points[2 * i + 1] = pts[i].y;
    }
    for (size_t i = 0; i < cs.size(); ++i) {
        contours[2 * i] = cs[i].count;
        contours[2 * i + 1] = cs[i].hole;
    }
    return PRL_OK;
}

int prl_hip_approx_poly_closed(const int32_t* points, int n_points, double epsilon, int32_t* out_points, int* n_out)
{
    if (n_points < 0 || (n_points && (!points || !out_points)) || !n_out || !(epsilon >= 0)) return PRL_ERR_BAD_ARG;
    std::vector<CtPoint> src((size_t)n_points), dst((size_t)n_points);
    for (int i = 0; i < n_points; ++i) src[(size_t)i] = CtPoint{points[2 * i], points[2 * i + 1]};
    *n_out = ct_approx_closed(src.data(), n_points, epsilon, dst.data());
    for (int i = 0; i < *n_out; ++i) {
        out_points[2 * i] = dst[(size_t)i].x;
        out_points[2 * i + 1] = dst[(size_t)i].y;
    }
    return PRL_OK;
}

int prl_hip_document_quad(const uint8_t* map, size_t step, int width, int height, int32_t quad[8], int* found)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!map || step < (size_t)width || !quad || !found || width > kStageMaxSide || height > kStageMaxSide) return PRL_ERR_BAD_ARG;
    CtPoint q[4];
    *found = ct_document_quad(map, step, width, height, q) ? 1 : 0;
    for (int k = 0; k < 4; ++k) {
        quad[2 * k] = *found ? q[k].x : 0;
        quad[2 * k + 1] = *found ? q[k].y : 0;
    }
    return PRL_OK;
}

int prl_hip_document_quad_finish(const int32_t quad[8], int map_width, int map_height, int src_width, int src_height, float out[8])
{
    if (map_width <= 0 || map_height <= 0 || src_width <= 0 || src_height <= 0) return PRL_ERR_EMPTY;
    if (!quad || !out) return PRL_ERR_BAD_ARG;
    float r[8];
    if (!ct_finish(quad, map_width, map_height, src_width, src_height, r)) return PRL_ERR_BAD_ARG;   // not strictly convex
    std::copy(r, r + 8, out);
    return PRL_OK;
}

int prl_hip_document_contour_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                          int height, float* quads, int32_t* found, int32_t* out_try, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, nullptr, 0, 0};
    const int st = contour_checks(a, channels, quads && found, true);
    return st != PRL_OK ? st : contour_batch(a, channels, quads, found, out_try, stream);
}

int prl_hip_document_contour_host(int channels, const uint8_t* src, size_t src_step, int width, int height, float quad[8], int32_t* found,
                                  int32_t* out_try)
{
    const PageArgs a{1, src, 0, src_step, width, height, nullptr, 0, 0};
    const int st = contour_checks(a, channels, quad && found, false);
    return st != PRL_OK ? st : stage_host_pages(a, channels, 0, 0, 0,
                            [&](const PageArgs& page, hipStream_t s) { return contour_batch(page, channels, quad, found, out_try, s); });
}

int prl_hip_hough_edges_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                     int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    const int st = hough_edges_checks(a, channels, true, true);
    return st != PRL_OK ? st : hough_edges_batch(a, channels, stream);
}

int prl_hip_hough_edges_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = hough_edges_checks(a, channels, true, false);
    return st != PRL_OK ? st : stage_host_pages(a, channels, 1, width, height, [&](const PageArgs& page, hipStream_t s) { return hough_edges_batch(page, channels, s); });
}

int prl_hip_hough_line_contour_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                            int width, int height, int32_t* quads, int32_t* found, int32_t* out_lines, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, nullptr, 0, 0};
    const int st = hough_contour_checks(a, channels, quads, found, true);
    return st != PRL_OK ? st : hough_contour_batch(a, channels, quads, found, out_lines, stream);
}

int prl_hip_hough_line_contour_host(int channels, const uint8_t* src, size_t src_step, int width, int height, int32_t quad[8], int32_t* found,
                                    int32_t* out_lines)
{
    const PageArgs a{1, src, 0, src_step, width, height, nullptr, 0, 0};
    const int st = hough_contour_checks(a, channels, quad, found, false);
    return st != PRL_OK ? st : stage_host_pages(a, channels, 0, 0, 0,
                            [&](const PageArgs& page, hipStream_t s) { return hough_contour_batch(page, channels, quad, found, out_lines, s); });
}

}  // extern "C"
