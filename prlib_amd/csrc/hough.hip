// hough.hip — cv::HoughLines(map, lines, 1, CV_PI / 180, threshold) on batched 8UC1 maps and the line entries of
// prl::findHoughLineContour (src/border_detection/houghLine.cpp:227-255).  The arithmetic is stated in include/prl_hip.h
// ("Hough lines") and restated in tests/houghline_ref.py; the trig table, the order of the peaks and the quad search are host
// code (houghline.h).  The standard transform's accumulator is an integer histogram, so the order of the votes does not matter.
//
//   k_hough_points   the non-zero pixels of every page as a list of (y << 16 | x), in no particular order: a wavefront's ballot
//                    takes one slot range from the page's counter.
//   k_hough_vote     a workgroup owns one angle of one page and one range of at most kHoughLdsCells rho cells (an A4 page's
//                    11 977 fit in one range; a row that does not fit is split over blockIdx.y, the same code with a range
//                    test).  It keeps its piece of the accumulator row in LDS, streams the page's point list, votes with LDS
//                    atomics and writes the piece out once, frame cells included.  The table comes as a kernel argument: the
//                    angle is the same for the whole workgroup, the device never evaluates sin or cos.  All points of one
//                    straight line hit one cell at that line's angle: a same-address LDS atomic, slow and correct.
//   k_hough_peaks    the local maxima above the threshold as (count, cell), appended per page through a wavefront's ballot.
// The lists come down once per chunk of pages and are sorted on the host.
#include <algorithm>
#include <cstring>
#include <vector>

#include "houghline.h"
#include "prl_internal.h"

namespace prl_hip {

namespace {

typedef unsigned long long u64;

constexpr int kHoughLdsCells = 12288;   // 48 KB of int32: three workgroups per CU
constexpr int kHoughThreads = 256;

struct HoughTab {   // a kernel argument: 1440 bytes
    float c[kHlNumAngle], s[kHlNumAngle];
};

// grid = (ceil(W / 256), H, pages)
__global__ __launch_bounds__(256) void k_hough_points(PageSet src, int W, unsigned* __restrict__ pts, size_t cap, unsigned* __restrict__ count)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, page = blockIdx.z;
    const bool on = x < W && src.page(page)[(size_t)y * src.step + x] != 0;
    const u64 m = __ballot(on);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(&count[page], (unsigned)__popcll(m));
    base = __shfl(base, 0);
    if (on) pts[(size_t)page * cap + base + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = ((unsigned)y << 16) | (unsigned)x;
}

// grid = (numangle + 2, ranges, pages): blockIdx.x is the accumulator's row, rows 0 and numangle + 1 are the frame
__global__ __launch_bounds__(kHoughThreads) void k_hough_vote(HoughTab tab, int numrho, int cells, const unsigned* __restrict__ pts, size_t cap,
                                                              const unsigned* __restrict__ count, int32_t* __restrict__ accum,
                                                              size_t accum_page)
{
    extern __shared__ int row[];
    const int t = threadIdx.x, a = blockIdx.x, page = blockIdx.z;
    const int lo = (int)blockIdx.y * cells, hi = min(numrho, lo + cells);   // the rho cells [lo, hi) of this row
    int32_t* out = accum + (size_t)page * accum_page + (size_t)a * (size_t)(numrho + 2);
    if (blockIdx.y == 0 && t == 0) out[0] = 0;
    if (hi == numrho && t == 0) out[numrho + 1] = 0;
    if (a == 0 || a == kHlNumAngle + 1) {
        for (int i = lo + t; i < hi; i += kHoughThreads) out[i + 1] = 0;
        return;
    }
    for (int i = t; i < hi - lo; i += kHoughThreads) row[i] = 0;
    __syncthreads();
    const float c = tab.c[a - 1], s = tab.s[a - 1];
    const int shift = (numrho - 1) / 2, n = (int)count[page];
    const unsigned* p = pts + (size_t)page * cap;
    for (int i = t; i < n; i += kHoughThreads) {
        const unsigned v = p[i];
        const float fx = __fmul_rn((float)(v & 0xffffu), c), fy = __fmul_rn((float)(v >> 16), s);
        const int r = (int)rintf(__fadd_rn(fx, fy)) + shift;
        if (r >= lo && r < hi) atomicAdd(&row[r - lo], 1);
    }
    __syncthreads();
    for (int i = t; i < hi - lo; i += kHoughThreads) out[lo + i + 1] = row[i];
}

// grid = (ceil(numrho / 256), numangle, pages)
__global__ __launch_bounds__(256) void k_hough_peaks(const int32_t* __restrict__ accum, size_t accum_page, int numrho, int threshold,
                                                     uint2* __restrict__ peaks, size_t cap, unsigned* __restrict__ count)
{
    const int r = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, page = blockIdx.z;
    const int32_t* A = accum + (size_t)page * accum_page;
    const size_t base = (size_t)(n + 1) * (size_t)(numrho + 2) + (size_t)(r + 1);
    bool peak = false;
    int a = 0;
    if (r < numrho) {
        a = A[base];
        peak = a > threshold && a > A[base - 1] && a >= A[base + 1] && a > A[base - numrho - 2] && a >= A[base + numrho + 2];
    }
    const u64 m = __ballot(peak);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    unsigned at = 0;
    if (lane == 0) at = atomicAdd(&count[page], (unsigned)__popcll(m));
    at = __shfl(at, 0);
    if (peak) {
        const size_t slot = (size_t)at + (size_t)__popcll(m & ((1ull << lane) - 1ull));
        if (slot < cap) peaks[(size_t)page * cap + slot] = make_uint2((unsigned)a, (unsigned)base);
    }
}

}  // namespace

HoughPlan hough_plan(int W, int H)
{
    HoughPlan p;
    p.W = W;
    p.H = H;
    p.numrho = hl_numrho(W, H);
    p.cells = std::min(p.numrho, kHoughLdsCells);
    p.ranges = (p.numrho + p.cells - 1) / p.cells;
    p.point_cap = (size_t)W * (size_t)H;
    p.points_bytes = r256(p.point_cap * sizeof(unsigned));
    p.accum_cells = hl_accum_cells(W, H);
    p.accum_bytes = r256(p.accum_cells * sizeof(int32_t));
    p.peak_cap = (size_t)kHlNumAngle * (size_t)((p.numrho + 1) / 2);   // two neighbours in a row are never both peaks
    p.peaks_bytes = r256(p.peak_cap * sizeof(uint2));
    return p;
}

// the framed accumulators of n maps into d_accum (pages accum_page cells apart); points: n * points_bytes, counters: n words.
// Enqueues only.
int hough_vote_run(const HoughPlan& p, const PageSet& maps, int n, uint8_t* points, unsigned* counters, int32_t* d_accum, size_t accum_page,
                   hipStream_t hs)
{
    HoughTab tab;
    hl_trig_table(tab.c, tab.s);
    const size_t cap = p.points_bytes / sizeof(unsigned);
    PRL_HIP_CHECK(hipMemsetAsync(counters, 0, sizeof(unsigned) * (size_t)n, hs));
    hipLaunchKernelGGL(k_hough_points, dim3((unsigned)((p.W + 255) / 256), (unsigned)p.H, (unsigned)n), dim3(256), 0, hs, maps, p.W,
                       reinterpret_cast<unsigned*>(points), cap, counters);
    PRL_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_hough_vote, dim3((unsigned)(kHlNumAngle + 2), (unsigned)p.ranges, (unsigned)n), dim3(kHoughThreads),
                       (size_t)p.cells * sizeof(int), hs, tab, p.numrho, p.cells, reinterpret_cast<const unsigned*>(points), cap, counters,
                       d_accum, accum_page);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// The peaks of n accumulators, sorted, per page: sink(page, peaks, count) runs on the calling thread for every page in turn.
// peaks: n * peaks_bytes of device memory, counters: n words; `w` owns the pinned block, which grows to the lists' size.
// Waits for the stream: the counts come down first, then all lists in one go.
int hough_peaks_run(const HoughPlan& p, const int32_t* d_accum, size_t accum_page, int n, int threshold, uint8_t* peaks, unsigned* counters,
                    const WorkScope& w, const std::function<void(int, const HlPeak*, size_t)>& sink)
{
    const hipStream_t hs = w.stream;
    const size_t cap = p.peaks_bytes / sizeof(uint2);
    PRL_HIP_CHECK(hipMemsetAsync(counters, 0, sizeof(unsigned) * (size_t)n, hs));
    hipLaunchKernelGGL(k_hough_peaks, dim3((unsigned)((p.numrho + 255) / 256), (unsigned)kHlNumAngle, (unsigned)n), dim3(256), 0, hs, d_accum,
                       accum_page, p.numrho, threshold, reinterpret_cast<uint2*>(peaks), cap, counters);
    PRL_HIP_CHECK(hipGetLastError());
    std::vector<unsigned> cnt((size_t)n);
    PRL_HIP_CHECK(hipMemcpyAsync(w.pinned(), counters, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost, hs));
    PRL_HIP_CHECK(hipStreamSynchronize(hs));
    std::memcpy(cnt.data(), w.pinned(), sizeof(unsigned) * (size_t)n);
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (cnt[(size_t)i] > cap) {   // (cannot happen: see hough_plan; loud, as HoughLinesP's segment lists are)
            set_error_detail("HoughLines: peak list overflow");
            return PRL_ERR_NOMEM;
        }
        total += cnt[(size_t)i];
    }
    const int st = ensure_pinned(w.ctx, std::max<size_t>(total, 1) * sizeof(HlPeak));
    if (st != PRL_OK) return st;
    HlPeak* h = w.pinned<HlPeak>();
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        if (cnt[(size_t)i])
            PRL_HIP_CHECK(hipMemcpyAsync(h + at, peaks + (size_t)i * p.peaks_bytes, sizeof(HlPeak) * (size_t)cnt[(size_t)i], hipMemcpyDeviceToHost,
                                         hs));
        at += cnt[(size_t)i];
    }
    PRL_HIP_CHECK(hipStreamSynchronize(hs));
    std::vector<size_t> first((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) first[(size_t)i + 1] = first[(size_t)i] + cnt[(size_t)i];
    host_pool_for(n, [&](int i) { hl_sort_peaks(h + first[(size_t)i], cnt[(size_t)i]); });
    for (int i = 0; i < n; ++i) sink(i, h + first[(size_t)i], cnt[(size_t)i]);
    return PRL_OK;
}

size_t hough_work_per_page(const HoughPlan& p) { return p.points_bytes + p.accum_bytes + p.peaks_bytes; }

// cv::HoughLines of n maps (a chunk): work holds n * hough_work_per_page bytes, small 2 * n words
int hough_lines_run(const HoughPlan& p, const PageSet& maps, int n, int threshold, uint8_t* work, const WorkScope& w,
                    const std::function<void(int, const HlPeak*, size_t)>& sink)
{
    uint8_t* points = work;
    int32_t* accum = reinterpret_cast<int32_t*>(work + p.points_bytes * (size_t)n);
    uint8_t* peaks = work + (p.points_bytes + p.accum_bytes) * (size_t)n;
    unsigned* counters = w.small<unsigned>();
    int st = hough_vote_run(p, maps, n, points, counters, accum, p.accum_bytes / sizeof(int32_t), w.stream);
    if (st != PRL_OK) return st;
    return hough_peaks_run(p, accum, p.accum_bytes / sizeof(int32_t), n, threshold, peaks, counters + n, w, sink);
}

namespace {

// EMPTY, then BAD_ARG: 8UC1 maps in, nothing out on the device
int map_checks(const PageArgs& a, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if ((st = pages_rows_ok(a, 1, 0, batch)) != PRL_OK) return st;
    return pages_sides_ok(a);
}

int lines_batch(const PageArgs& a, int threshold, float* lines, int max_lines, int32_t* n_lines, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const HoughPlan p = hough_plan(a.width, a.height);
    const int chunk = stage_chunk(a.n_pages, hough_work_per_page(p));
    WorkScope w;
    int st = w.open(stream, hough_work_per_page(p) * (size_t)chunk, 2 * sizeof(unsigned) * (size_t)chunk, sizeof(unsigned) * (size_t)chunk);
    if (st != PRL_OK) return st;
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int n = std::min(chunk, a.n_pages - first);
        st = hough_lines_run(p, src_pages(a, first), n, threshold, w.scratch(), w, [&](int i, const HlPeak* pk, size_t count) {
            n_lines[first + i] = (int32_t)std::min<size_t>(count, 0x7fffffff);
            float* out = lines + (size_t)(first + i) * 2 * (size_t)max_lines;
            for (size_t k = 0; k < std::min(count, (size_t)max_lines); ++k) hl_line_of(pk[k].cell, p.numrho, out + 2 * k, out + 2 * k + 1);
        });
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int lines_checks(const PageArgs& a, int threshold, const float* lines, int max_lines, const int32_t* n_lines, bool batch)
{
    const int st = map_checks(a, batch);
    if (st != PRL_OK) return st;
    if (threshold < 0 || max_lines < 0 || (max_lines && !lines) || !n_lines) return PRL_ERR_BAD_ARG;
    return PRL_OK;
}

}  // namespace
}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_hough_lines_geometry(int width, int height, int* numangle, int* numrho)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!numangle || !numrho || width > kStageMaxSide || height > kStageMaxSide) return PRL_ERR_BAD_ARG;
    *numangle = kHlNumAngle;
    *numrho = hl_numrho(width, height);
    return PRL_OK;
}

int prl_hip_hough_accumulator_batch_device(int n_pages, const uint8_t* d_map, size_t page_stride, size_t step, int width, int height,
                                           int32_t* d_accum, size_t accum_page_stride, void* stream)
{
    const PageArgs a{n_pages, d_map, page_stride, step, width, height, nullptr, 0, 0};
    int st = map_checks(a, true);
    if (st != PRL_OK) return st;
    if (!d_accum || ((size_t)d_accum & 3) || (accum_page_stride & 3) || accum_page_stride < hl_accum_cells(width, height) * sizeof(int32_t))
        return PRL_ERR_BAD_ARG;
    if (n_pages == 0) return PRL_OK;
    const HoughPlan p = hough_plan(width, height);
    const int chunk = stage_chunk(n_pages, p.points_bytes);
    WorkScope w;
    st = w.open(stream, p.points_bytes * (size_t)chunk, sizeof(unsigned) * (size_t)chunk, 0);
    if (st != PRL_OK) return st;
    for (int first = 0; first < n_pages; first += chunk) {
        st = hough_vote_run(p, src_pages(a, first), std::min(chunk, n_pages - first), w.scratch(), w.small<unsigned>(),
                            d_accum + (size_t)first * (accum_page_stride / sizeof(int32_t)), accum_page_stride / sizeof(int32_t), w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int prl_hip_hough_lines_batch_device(int n_pages, const uint8_t* d_map, size_t page_stride, size_t step, int width, int height, int threshold,
                                     float* lines, int max_lines, int32_t* n_lines, void* stream)
{
    const PageArgs a{n_pages, d_map, page_stride, step, width, height, nullptr, 0, 0};
    const int st = lines_checks(a, threshold, lines, max_lines, n_lines, true);
    if (st != PRL_OK) return st;
    return lines_batch(a, threshold, lines, max_lines, n_lines, stream);
}

int prl_hip_hough_lines_host(const uint8_t* map, size_t step, int width, int height, int threshold, float* lines, int max_lines,
                             int32_t* n_lines)
{
    const PageArgs a{1, map, 0, step, width, height, nullptr, 0, 0};
    const int st = lines_checks(a, threshold, lines, max_lines, n_lines, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(a, 1, 0, 0, 0,
                            [&](const PageArgs& page, hipStream_t s) { return lines_batch(page, threshold, lines, max_lines, n_lines, s); });
}

int prl_hip_hough_line_quad(const float* lines, int n_lines, int width, int height, int32_t quad[8], int* found)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (n_lines < 0 || (n_lines && !lines) || !quad || !found || width > kStageMaxSide || height > kStageMaxSide) return PRL_ERR_BAD_ARG;
    int32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    *found = hl_quad(lines, n_lines, width, height, q) ? 1 : 0;
    std::copy(q, q + 8, quad);
    return PRL_OK;
}

}  // extern "C"
