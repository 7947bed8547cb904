// localotsu.hip — prl::binarizeLocalOtsu (src/binarizations/binarizeLocalOtsu.cpp:37-163) on batched pages, and its own hot path:
// Otsu's threshold of every rectangle of a list, and the paint (the rules: include/prl_hip.h, "binarizeLocalOtsu").
//
//   mask = 255; for every rectangle r of the page: thr = getThreshVal_Otsu_8u(histogram of gray(r), scale 1 / (w h));
//   mask(r) = 0 where p <= thr (max value 255), or everywhere (any other max value)
//
// Rectangles run from 4 x 4 to the whole page, thousands per text page; they overlap, and all that is ever stored is 0, so the
// result does not depend on their order and concurrent stores are benign.
//
//   k_rect_small   a wavefront per rectangle of at most kRectSmallArea pixels: 256 bins in LDS, the float64 scan on one lane
//                  (otsu_scan, k_otsu's body), a second sweep that stores.  A larger rectangle's wavefront clears the rectangle's
//                  slab of bins in the workspace and appends its index to the list of large rectangles.
//   k_rect_large   (histogram form) the large ones, kRectSlices workgroups each (rows slice, slice + kRectSlices, ...): bins in LDS, then atomics
//                  into the slab.  A fixed grid walks the list, whose length never leaves the device.
//   k_rect_thr     the scan of every slab, a lane per rectangle.
//   k_rect_large   (paint form) the same walk, storing.
//
// The composed call: gray (COLOR_RGB2GRAY for colour pages), EnhanceLocalContrastByCLAHE (clahe.hip), CannyEdgeDetection
// (edgedet.hip), a 7 x 7 dilation (three iterations of 3 x 3; gmorph.hip), ONE read-back of the edge maps per chunk, the external
// bounding rectangles on the host thread pool (contour.h), their upload, and the kernels above.  The same rectangles from the
// device (components.hip: only the per-page counts cross to the host) measured no faster on whole calls (profiles/r24/INDEX.md):
// that path is kept behind the hooks build's PRL_HIP_LO_HOST_RECTS=0.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "contour.h"
#include "prl_device_math.h"
#include "prl_internal.h"

namespace prl_hip {

namespace {

constexpr int kRectSmallArea = PRL_RECT_OTSU_SMALL_AREA;
constexpr int kRectSlices = 32;        // workgroups per large rectangle
constexpr int kRectLargeGrid = 1024;   // workgroups of the two kernels that walk the list of large rectangles
constexpr int kRectChunk = 1 << 16;    // rectangles per pass: a slab of 256 words each

struct RectJob {
    int W, H;
    int r0, r1;           // rectangles [r0, r1) of the call ...
    int rect_base;        // ... of which `rects` holds those from rect_base on
    int n_pages;
    int all_black;        // the max value is not 255: every pixel of a rectangle is painted
    const int32_t* rects;      // x, y, w, h
    const int32_t* offsets;    // n_pages + 1: the rectangles of page i are [offsets[i], offsets[i + 1])
    int32_t* thr;              // rectangle r's threshold goes to thr[r - thr_base]
    int thr_base;
    unsigned* slabs;           // 256 words per rectangle of the pass
    unsigned* large;           // [0]: how many; then their indices
};

__device__ __forceinline__ int page_of(const RectJob& j, int r)
{
    int lo = 0, hi = j.n_pages - 1;   // the last page whose first rectangle is at or before r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (j.offsets[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// false: no such rectangle on the page (it is ignored)
__device__ __forceinline__ bool load_rect(const RectJob& j, int r, int* x, int* y, int* w, int* h)
{
    const int32_t* q = j.rects + 4 * (size_t)(r - j.rect_base);
    *x = q[0]; *y = q[1]; *w = q[2]; *h = q[3];
    return *x >= 0 && *y >= 0 && *w > 0 && *h > 0 && *w <= j.W - *x && *h <= j.H - *y;
}

// grid = ceil((r1 - r0) / 4) workgroups of four wavefronts
__global__ __launch_bounds__(256) void k_rect_small(RectJob j, PageSet gray, PageSetOut dst)
{
    __shared__ unsigned bins[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = j.r0 + blockIdx.x * 4 + wave;
    int x = 0, y = 0, w = 0, h = 0;
    const bool valid = r < j.r1 && load_rect(j, r, &x, &y, &w, &h);
    const int area = valid ? w * h : 0;   // (a side is at most 32768: the product fits)
    const bool small = valid && area <= kRectSmallArea;
    for (int i = lane; i < 256; i += 64) bins[wave][i] = 0;
    __syncthreads();
    const int page = valid ? page_of(j, r) : 0;
    const uint8_t* g = gray.page(page) + (size_t)y * gray.step + x;
    if (small) {
        for (int i = lane; i < area; i += 64) {
            const int yy = i / w, xx = i - yy * w;
            atomicAdd(&bins[wave][g[(size_t)yy * gray.step + xx]], 1u);
        }
    } else if (valid) {   // a large one: its slab starts empty, and the list gets it
        unsigned* slab = j.slabs + (size_t)(r - j.r0) * 256;
        for (int i = lane; i < 256; i += 64) slab[i] = 0;
        if (lane == 0) j.large[1 + atomicAdd(&j.large[0], 1u)] = (unsigned)r;
    }
    __syncthreads();
    if (!small) return;
    int thr = 0;
    if (lane == 0) thr = otsu_scan(bins[wave], 1. / ((double)w * h));
    thr = __shfl(thr, 0);
    if (lane == 0) j.thr[r - j.thr_base] = thr;
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + x;
    for (int i = lane; i < area; i += 64) {
        const int yy = i / w, xx = i - yy * w;
        if (j.all_black || (int)g[(size_t)yy * gray.step + xx] <= thr) d[(size_t)yy * dst.step + xx] = 0;
    }
}

// grid = kRectLargeGrid; item = (large rectangle, slice)
template <bool PAINT>
__global__ __launch_bounds__(256) void k_rect_large(RectJob j, PageSet gray, PageSetOut dst)
{
    __shared__ unsigned bins[256];
    const int t = threadIdx.x;
    const unsigned items = j.large[0] * (unsigned)kRectSlices;
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)j.large[1 + item / kRectSlices], slice = (int)(item % kRectSlices);
        int x, y, w, h;
        load_rect(j, r, &x, &y, &w, &h);   // (valid: k_rect_small listed it)
        if (slice >= h) continue;
        const int page = page_of(j, r);
        const uint8_t* g = gray.page(page) + (size_t)y * gray.step + x;
        if (PAINT) {
            const int thr = j.thr[r - j.thr_base];
            uint8_t* d = dst.page(page) + (size_t)y * dst.step + x;
            for (int yy = slice; yy < h; yy += kRectSlices)
                for (int xx = t; xx < w; xx += 256)
                    if (j.all_black || (int)g[(size_t)yy * gray.step + xx] <= thr) d[(size_t)yy * dst.step + xx] = 0;
        } else {
            bins[t] = 0;
            __syncthreads();
            for (int yy = slice; yy < h; yy += kRectSlices)
                for (int xx = t; xx < w; xx += 256) atomicAdd(&bins[g[(size_t)yy * gray.step + xx]], 1u);
            __syncthreads();
            if (bins[t]) atomicAdd(&j.slabs[(size_t)(r - j.r0) * 256 + t], bins[t]);
            __syncthreads();   // (the next item clears the bins)
        }
    }
}

// grid = kRectLargeGrid / 4 workgroups of 64: a lane per large rectangle
__global__ __launch_bounds__(64) void k_rect_thr(RectJob j)
{
    const unsigned n = j.large[0];
    for (unsigned i = blockIdx.x * 64 + threadIdx.x; i < n; i += gridDim.x * 64) {
        const int r = (int)j.large[1 + i];
        int x, y, w, h;
        load_rect(j, r, &x, &y, &w, &h);
        j.thr[r - j.thr_base] = otsu_scan(j.slabs + (size_t)(r - j.r0) * 256, 1. / ((double)w * h));
    }
}

// grid = (ceil(W / 1024), H, pages): four bytes a lane
__global__ __launch_bounds__(256) void k_fill255(PageSetOut dst, int W)
{
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= W) return;
    uint8_t* d = dst.page(blockIdx.z) + (size_t)blockIdx.y * dst.step + x0;
    if (W - x0 >= 4 && ((size_t)d & 3) == 0) *reinterpret_cast<unsigned*>(d) = 0xffffffffu;
    else
        for (int i = 0; i < min(4, W - x0); ++i) d[i] = 255;
}

// cv::cvtColor(COLOR_RGB2GRAY / RGBA2GRAY): (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14 (the weights of glue.hip's BGR adapter, swapped)
template <int CH>
__global__ __launch_bounds__(256) void k_rgb2gray(PageSet src, PageSetOut dst, int W)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const uint8_t* s = src.page(blockIdx.z) + (size_t)blockIdx.y * src.step + (size_t)x * CH;
    dst.page(blockIdx.z)[(size_t)blockIdx.y * dst.step + x] = (uint8_t)((4899u * s[0] + 9617u * s[1] + 1868u * s[2] + 8192u) >> 14);
}

// ---- the per-rectangle Otsu, enqueued ----------------------------------------------------------------------------------------

size_t rect_slab_bytes(int rects) { return r256((size_t)rects * 256 * sizeof(unsigned)); }
size_t rect_list_bytes(int rects) { return r256(((size_t)rects + 1) * sizeof(unsigned)); }
// the workspace of a pass of `rects` rectangles at most: [slabs | the list of large ones]
size_t rect_pass_bytes(int rects) { return rect_slab_bytes(rects) + rect_list_bytes(rects); }

// rectangles [r0, r1) of the call, r1 - r0 <= kRectChunk; j: everything but r0, r1, slabs, large
int rect_pass(RectJob j, int r0, int r1, uint8_t* work, const PageSet& gray, const PageSetOut& dst, hipStream_t hs)
{
    if (r1 <= r0) return PRL_OK;
    j.r0 = r0;
    j.r1 = r1;
    j.slabs = reinterpret_cast<unsigned*>(work);
    j.large = reinterpret_cast<unsigned*>(work + rect_slab_bytes(r1 - r0));
    PRL_HIP_CHECK(hipMemsetAsync(j.large, 0, sizeof(unsigned), hs));
    hipLaunchKernelGGL(k_rect_small, dim3((unsigned)((r1 - r0 + 3) / 4)), dim3(256), 0, hs, j, gray, dst);
    hipLaunchKernelGGL(k_rect_large<false>, dim3(kRectLargeGrid), dim3(256), 0, hs, j, gray, dst);
    hipLaunchKernelGGL(k_rect_thr, dim3(kRectLargeGrid / 4), dim3(64), 0, hs, j);
    hipLaunchKernelGGL(k_rect_large<true>, dim3(kRectLargeGrid), dim3(256), 0, hs, j, gray, dst);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

int fill255(const PageSetOut& dst, int n, int W, int H, hipStream_t hs)
{
    hipLaunchKernelGGL(k_fill255, dim3((unsigned)((W + 1023) / 1024), (unsigned)H, (unsigned)n), dim3(256), 0, hs, dst, W);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// saturate_cast<uchar>(cvRound(maxValue)) for a value in [0, 255]
int imax_of(double max_value) { return (int)std::nearbyint(max_value); }

int bad_arg(const char* why)
{
    set_error_detail(why);
    return PRL_ERR_BAD_ARG;
}

int rect_otsu_checks(const PageArgs& a, const int32_t* offsets, const int32_t* d_rects, double max_value)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (!(max_value >= 0 && max_value <= 255)) return bad_arg("rect_otsu: the max value is outside [0, 255]");
    if ((st = pages_rows_ok(a, 1, 1, true)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    if ((st = pages_overlap_ok(a, 1, 1, false)) != PRL_OK) return st;
    if (a.n_pages == 0) return PRL_OK;
    if (!offsets || offsets[0] != 0) return bad_arg("rect_otsu: the offsets must start at 0");
    for (int i = 0; i < a.n_pages; ++i)
        if (offsets[i + 1] < offsets[i]) return bad_arg("rect_otsu: the offsets must not decrease");
    if (offsets[a.n_pages] > 0 && !d_rects) return PRL_ERR_BAD_ARG;
    return PRL_OK;
}

// ---- prl::binarizeLocalOtsu ----------------------------------------------------------------------------------------------------

struct LoSpec {
    double max_value, clip_limit;
    CedSpec ced;
};

// EMPTY; the reference's argument checks (BAD_ARG); BAD_WINDOW; BAD_CHANNELS; BAD_ARG for the pages
int lo_checks(const PageArgs& a, int channels, const LoSpec& sp, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (!(sp.max_value >= 0 && sp.max_value <= 255)) return bad_arg("binarizeLocalOtsu: the max value is outside [0, 255]");
    if (ced_spec_check(sp.ced)) return PRL_ERR_BAD_ARG;
    if (sp.ced.size > PRL_GAUSS_MAX_SIDE) return PRL_ERR_BAD_WINDOW;
    if (channels != 1 && channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    if (sp.clip_limit != sp.clip_limit || sp.ced.iterations < -255 || sp.ced.iterations > 255) return PRL_ERR_BAD_ARG;
    if ((st = pages_rows_ok(a, channels, 1, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    return pages_overlap_ok(a, channels, 1, false);
}

// Steps 5 to 7 of a chunk with the rectangles from the host scan (contour.h), the call's path.  One read-back of the
// maps `D`, ct_external_rects per page on the host pool, the upload, kRectChunk rectangles a pass.
int lo_rects_host(const WorkScope& w, const uint8_t* D, size_t plane, int n, int W, int H, RectJob j, uint8_t* stage_work, size_t off_bytes,
                  const PageSet& gray, const PageSetOut& dst, int32_t* n_found, int32_t* n_kept)
{
    const hipStream_t hs = w.stream;
    uint8_t* h_maps = w.pinned();
    PRL_HIP_CHECK(hipMemcpyAsync(h_maps, D, plane * (size_t)n, hipMemcpyDeviceToHost, hs));
    PRL_HIP_CHECK(hipStreamSynchronize(hs));
    std::vector<std::vector<CtRect>> rects((size_t)n);
    host_pool_for(n, [&](int i) {
        const int found = ct_external_rects(h_maps + plane * (size_t)i, (size_t)W, W, H, &rects[(size_t)i]);
        if (n_found) n_found[i] = found;
        if (n_kept) n_kept[i] = (int32_t)rects[(size_t)i].size();
    });
    std::vector<int32_t> offsets((size_t)n + 1, 0), flat;
    for (int i = 0; i < n; ++i) {
        for (const CtRect& r : rects[(size_t)i]) flat.insert(flat.end(), {r.x, r.y, r.w, r.h});
        if (flat.size() / 4 > 0x7fffffffu) return bad_arg("binarizeLocalOtsu: too many rectangles");
        offsets[(size_t)i + 1] = (int32_t)(flat.size() / 4);
    }
    const int total = offsets[(size_t)n];
    int32_t* d_off = w.small<int32_t>();
    int32_t* d_rects = reinterpret_cast<int32_t*>(stage_work);
    uint8_t* pass_work = stage_work + r256((size_t)kRectChunk * 16);
    PRL_HIP_CHECK(hipMemcpyAsync(d_off, offsets.data(), ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, hs));
    j.rects = d_rects; j.offsets = d_off;
    j.thr = reinterpret_cast<int32_t*>(w.small() + off_bytes);
    int st;
    for (int r0 = 0; r0 < total; r0 += kRectChunk) {
        const int r1 = std::min(total, r0 + kRectChunk);
        PRL_HIP_CHECK(hipMemcpyAsync(d_rects, flat.data() + 4 * (size_t)r0, (size_t)(r1 - r0) * 16, hipMemcpyHostToDevice, hs));
        j.rect_base = r0;
        j.thr_base = r0;
        if ((st = rect_pass(j, r0, r1, pass_work, gray, dst, hs)) != PRL_OK) return st;
    }
    PRL_HIP_CHECK(hipStreamSynchronize(hs));   // (`flat` and `offsets` end with this scope)
    return PRL_OK;
}

// Steps 5 to 7 of a chunk on the device (components.hip): the labels of the maps, rule R's rectangles a statistics pass at a time
// where rect_pass reads them; the host sees the per-page counts only, from which it lays out the pass's offsets.  The same bytes
// as the host path, no faster: behind the hooks build's PRL_HIP_LO_HOST_RECTS=0, so that a test and the benchmark can run both.
int lo_rects_device(const WorkScope& w, const PageSet& maps, int n, int W, int H, RectJob j, uint8_t* cc_work, uint8_t* pass_work,
                    const PageSet& gray, const PageSetOut& dst, int32_t* n_found, int32_t* n_kept)
{
    const hipStream_t hs = w.stream;
    const size_t off_bytes = r256(((size_t)n + 1) * sizeof(int32_t));
    CcRun r;
    r.maps = maps;
    r.n = n; r.W = W; r.H = H;
    r.work = cc_work;
    r.small = w.small() + off_bytes + r256((size_t)kRectChunk * sizeof(int32_t));
    r.pinned = w.pinned<int32_t>();
    r.stream = hs;
    int st = cc_label(r);
    if (st != PRL_OK) return st;
    int found = 0;
    for (int i = 0; i < n; ++i) {
        found += r.pinned[i];
        if (n_found) n_found[i] = r.pinned[i];
        if (n_kept) n_kept[i] = 0;
    }
    int32_t* h_off = r.pinned + cc_pinned_bytes(n) / sizeof(int32_t);   // n + 1 values behind the labeller's
    std::vector<int32_t> seen((size_t)n, 0);
    j.rects = cc_pass_rects(r);
    int32_t* d_off = w.small<int32_t>();
    j.offsets = d_off;
    j.thr = reinterpret_cast<int32_t*>(w.small() + off_bytes);
    j.rect_base = 0;
    const int pass = cc_pass_components();
    for (int c0 = 0; c0 < found; c0 += pass) {
        if ((st = cc_stats_pass(r, c0, std::min(pass, found - c0), nullptr)) != PRL_OK) return st;
        if ((st = cc_read_kept(r)) != PRL_OK) return st;
        h_off[0] = 0;
        for (int i = 0; i < n; ++i) {   // the pass's rectangles lie page after page
            h_off[i + 1] = h_off[i] + (r.pinned[n + i] - seen[(size_t)i]);
            seen[(size_t)i] = r.pinned[n + i];
            if (n_kept) n_kept[i] = seen[(size_t)i];
        }
        const int total = h_off[n];
        PRL_HIP_CHECK(hipMemcpyAsync(d_off, h_off, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, hs));
        for (int r0 = 0; r0 < total; r0 += kRectChunk) {
            j.thr_base = r0;
            if ((st = rect_pass(j, r0, std::min(total, r0 + kRectChunk), pass_work, gray, dst, hs)) != PRL_OK) return st;
        }
        PRL_HIP_CHECK(hipStreamSynchronize(hs));   // (the next pass rewrites the pinned offsets and the pass's rectangles)
    }
    if (found == 0) PRL_HIP_CHECK(hipStreamSynchronize(hs));   // (the labeller's last upload reads the pinned block)
    return PRL_OK;
}

int lo_batch(const PageArgs& a, int C, const LoSpec& sp, int32_t* n_found, int32_t* n_kept, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const int W = a.width, H = a.height;
    const size_t plane = r256((size_t)W * H);
    const bool clahe = sp.clip_limit > 0;
    const bool host_rects = env_knobs().lo_host_rects;
    // a page's share of the workspace beside CannyEdgeDetection's: the gray page, the edge map, the dilated map, the dilation's
    // plane, and the labeller's (the label plane and its block counts)
    const size_t per_page = 4 * plane + (clahe ? enhance_contrast_work_per_page() : 0) + (host_rects ? 0 : cc_work_per_page(W, H));
    int chunk = ced_pages_per_chunk(sp.ced, a.n_pages, W, H, 1, per_page);
    if (host_rects) chunk = std::min(chunk, (int)std::max<size_t>(1, ((size_t)1 << 30) / plane));   // the read-back's pinned block: 1 GiB at most
    const size_t contrast_bytes = clahe ? r256(enhance_contrast_work_bytes(chunk)) : 0;
    const size_t ced_bytes = r256(ced_work_bytes(sp.ced, chunk, W, H, 1));
    // [gray | edges | dilated | dilation's plane | contrast | CannyEdgeDetection, later a pass of rect_pass (on the host path behind
    // its rectangles) | the labeller]
    const size_t rect_bytes = (host_rects ? r256((size_t)kRectChunk * 16) : 0) + rect_pass_bytes(kRectChunk);
    const size_t off_bytes = r256(((size_t)chunk + 1) * sizeof(int32_t));
    const size_t stage_bytes = std::max(ced_bytes, rect_bytes);
    WorkScope w;
    int st = w.open(stream, 4 * plane * (size_t)chunk + contrast_bytes + stage_bytes + (host_rects ? 0 : cc_work_bytes(chunk, W, H)),
                    std::max(ced_small_bytes(chunk, 1), off_bytes + r256((size_t)kRectChunk * sizeof(int32_t)) + (host_rects ? 0 : cc_small_bytes(chunk))),
                    std::max(ced_pinned_bytes(chunk, 1), host_rects ? plane * (size_t)chunk : cc_pinned_bytes(chunk) + off_bytes));
    if (st != PRL_OK) return st;
    const hipStream_t hs = w.stream;
    uint8_t* G = w.scratch();
    uint8_t* E = G + plane * (size_t)chunk;
    uint8_t* D = E + plane * (size_t)chunk;
    uint8_t* T = D + plane * (size_t)chunk;
    uint8_t* contrast_work = T + plane * (size_t)chunk;
    uint8_t* stage_work = contrast_work + contrast_bytes;
    uint8_t* cc_work = stage_work + stage_bytes;
    const int imax = imax_of(sp.max_value);
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int n = std::min(chunk, a.n_pages - first);
        const PageSet src = src_pages(a, first);
        const PageSetOut dst = dst_pages(a, first);
        const PageSetOut gp = page_set_out(G, plane, (size_t)W);
        const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)n);
        // 1. the gray page: a gray source is read where it lies (the stages below never write it)
        if (C == 3) hipLaunchKernelGGL(k_rgb2gray<3>, grid, dim3(256), 0, hs, src, gp, W);
        else if (C == 4) hipLaunchKernelGGL(k_rgb2gray<4>, grid, dim3(256), 0, hs, src, gp, W);
        PRL_HIP_CHECK(hipGetLastError());
        // 2. EnhanceLocalContrastByCLAHE(clip, true): a colour page's gray in place, a gray source into the plane
        if (clahe && (st = enhance_contrast_gray_run(sp.clip_limit, C == 1 ? src : as_source(gp), gp, n, W, H, chunk, contrast_work, hs)) != PRL_OK)
            return st;
        const PageSet gray = C == 1 && !clahe ? src : as_source(gp);
        // 3. CannyEdgeDetection; 4. dilate 3 x 3, three iterations
        const PageSetOut ep = page_set_out(E, plane, (size_t)W), dp = page_set_out(D, plane, (size_t)W);
        if ((st = ced_run(sp.ced, gray, ep, n, W, H, 1, stage_work, w.small(), w.pinned<unsigned>(), hs)) != PRL_OK) return st;
        if ((st = gmorph_dilate_rect_run(7, W, H, as_source(ep), dp, n, T, hs)) != PRL_OK) return st;
        if ((st = fill255(dst, n, W, H, hs)) != PRL_OK) return st;
        // 5. the labels; 6. the rectangles; 7. the thresholds and the paint, kRectChunk rectangles a pass
        RectJob j{};
        j.W = W; j.H = H; j.n_pages = n; j.all_black = imax != 255;
        int32_t* found = n_found ? n_found + first : nullptr;
        int32_t* kept = n_kept ? n_kept + first : nullptr;
        st = host_rects ? lo_rects_host(w, D, plane, n, W, H, j, stage_work, off_bytes, gray, dst, found, kept)
                        : lo_rects_device(w, as_source(dp), n, W, H, j, cc_work, stage_work, gray, dst, found, kept);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_external_rects(const uint8_t* map, size_t step, int width, int height, int32_t* rects, int max_rects, int* n_found, int* n_kept)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!map || step < (size_t)width || !n_found || !n_kept || max_rects < 0 || (max_rects && !rects) || width > kStageMaxSide ||
        height > kStageMaxSide)
        return PRL_ERR_BAD_ARG;
    std::vector<CtRect> rs;
    *n_found = ct_external_rects(map, step, width, height, &rs);
    *n_kept = (int)rs.size();
    if ((int)rs.size() > max_rects) return PRL_OK;   // the counts alone: call again with room
    for (size_t i = 0; i < rs.size(); ++i) {
        rects[4 * i] = rs[i].x;
        rects[4 * i + 1] = rs[i].y;
        rects[4 * i + 2] = rs[i].w;
        rects[4 * i + 3] = rs[i].h;
    }
    return PRL_OK;
}

int prl_hip_rect_otsu_batch_device(int n_pages, const int32_t* rect_offsets, const int32_t* d_rects, double max_value, const uint8_t* d_gray,
                                   size_t gray_page_stride, size_t gray_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                                   size_t dst_step, int32_t* d_thresholds, void* stream)
{
    const PageArgs a{n_pages, d_gray, gray_page_stride, gray_step, width, height, d_dst, dst_page_stride, dst_step};
    int st = rect_otsu_checks(a, rect_offsets, d_rects, max_value);
    if (st != PRL_OK || n_pages == 0) return st;
    const int total = rect_offsets[n_pages];
    const int page_chunk = stage_chunk(n_pages, 0);
    const size_t off_bytes = r256(((size_t)n_pages + 1) * sizeof(int32_t));
    WorkScope w;
    st = w.open(stream, rect_pass_bytes(std::min(total, kRectChunk)), off_bytes + (d_thresholds ? 0 : r256((size_t)total * sizeof(int32_t))),
                off_bytes);
    if (st != PRL_OK) return st;
    for (int first = 0; first < n_pages; first += page_chunk)
        if ((st = fill255(dst_pages(a, first), std::min(page_chunk, n_pages - first), width, height, w.stream)) != PRL_OK) return st;
    if (total == 0) return PRL_OK;
    // the offsets go up through the pinned block as warp.hip's page records do: the caller's array is free when the call returns
    DeviceCtx* ctx = w.ctx;
    if (ctx->pinned_use) PRL_HIP_CHECK(hipEventSynchronize(ctx->pinned_use));
    else PRL_HIP_CHECK(hipEventCreateWithFlags(&ctx->pinned_use, hipEventDisableTiming));
    std::memcpy(ctx->pinned, rect_offsets, ((size_t)n_pages + 1) * sizeof(int32_t));
    int32_t* d_off = w.small<int32_t>();
    PRL_HIP_CHECK(hipMemcpyAsync(d_off, ctx->pinned, ((size_t)n_pages + 1) * sizeof(int32_t), hipMemcpyHostToDevice, w.stream));
    PRL_HIP_CHECK(hipEventRecord(ctx->pinned_use, w.stream));
    RectJob j{};
    j.W = width; j.H = height; j.n_pages = n_pages; j.all_black = imax_of(max_value) != 255;
    j.rects = d_rects; j.offsets = d_off; j.rect_base = 0;
    j.thr = d_thresholds ? d_thresholds : reinterpret_cast<int32_t*>(w.small() + off_bytes);
    for (int r0 = 0; r0 < total; r0 += kRectChunk)
        if ((st = rect_pass(j, r0, std::min(total, r0 + kRectChunk), w.scratch(), src_pages(a, 0), dst_pages(a, 0), w.stream)) != PRL_OK) return st;
    return PRL_OK;
}

int prl_hip_binarize_local_otsu_batch_device(int n_pages, int channels, double max_value, double clahe_clip_limit, int blur_size,
                                             double upper_coeff, double lower_coeff, int morph_iterations, const uint8_t* d_src,
                                             size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                             size_t dst_page_stride, size_t dst_step, int32_t* n_found, int32_t* n_kept, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    const LoSpec sp{max_value, clahe_clip_limit, CedSpec{blur_size, upper_coeff, lower_coeff, morph_iterations}};
    const int st = lo_checks(a, channels, sp, true);
    return st != PRL_OK ? st : lo_batch(a, channels, sp, n_found, n_kept, stream);
}

int prl_hip_binarize_local_otsu_host(int channels, double max_value, double clahe_clip_limit, int blur_size, double upper_coeff,
                                     double lower_coeff, int morph_iterations, const uint8_t* src, size_t src_step, int width, int height,
                                     uint8_t* dst, size_t dst_step, int32_t* n_found, int32_t* n_kept)
{
    const PageArgs h{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const LoSpec sp{max_value, clahe_clip_limit, CedSpec{blur_size, upper_coeff, lower_coeff, morph_iterations}};
    const int st = lo_checks(h, channels, sp, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(h, channels, 1, width, height,
                            [&](const PageArgs& page, hipStream_t s) { return lo_batch(page, channels, sp, n_found, n_kept, s); });
}

}  // extern "C"
