// fbcitb.hip — prl::binarizeFBCITB (src/binarizations/binarizeFBCITB.cpp:73-404) on batched pages, and its own two device parts: the
// variance mask and the ordered paint of the kept contours' rectangles (the rules: include/prl_hip.h, "binarizeFBCITB"; the host
// half in C++: fbcitb.h, contour.h).
//
//   k_variance_mask   MatToLocalVarianceMap(page, 3) > threshold on every channel, AND-ed: the host turns the float32 comparison
//                     into an integer cut once per call (fb_variance_cut), the kernel compares 9 sum(p^2) - sum(p)^2 with it.
//   the paint         every kept contour is (rectangle, cut, polarity), and where rectangles overlap the LARGER INDEX wins
//                     (combinationAND.copyTo writes 0 and 255).  Nothing is serialised: an int32 owner plane per page is cleared,
//                     every rectangle raises its pixels to its index + 1 by atomicMax (k_paint_small: a wavefront per rectangle of
//                     at most kPaintSmallArea pixels; larger ones go to a device-side list that k_paint_large walks, kPaintSlices
//                     workgroups each, as localotsu.hip's k_rect_large does), and k_paint_resolve applies each pixel's owner.
//                     Passes of kPaintChunk rectangles run in index order, a later pass overwriting what it owns.
//
// The composed call: CLAHE per channel (clahe.hip), the bilateral filter per channel (bilateral.hip), CannyEdgeDetection
// (edgedet.hip), the variance mask of the ORIGINAL page and cv::Canny(64, 128) on it (canny.hip), their AND, the gray plane of the
// processed page, ONE read-back of map and gray plane per chunk, fb_contours per page on the host thread pool, the upload, the
// paint, and dilate(2) / erode(2) (morph.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "bilateral.h"
#include "fbcitb.h"
#include "prl_internal.h"

namespace prl_hip {

namespace {

constexpr int kPaintSmallArea = 4096;
constexpr int kPaintSlices = 32;        // workgroups per large rectangle
constexpr int kPaintLargeGrid = 1024;   // workgroups of the kernel that walks the list of large rectangles
constexpr int kPaintChunk = 1 << 16;    // rectangles per pass of the composed call
constexpr int kRectWords = 6;           // x, y, w, h, cut, below

// ---- the variance mask -------------------------------------------------------------------------------------------------------

// grid = (ceil(W / 256), H, pages); the window is cut from the edge-replicated page
template <int C>
__global__ __launch_bounds__(256) void k_variance_mask(PageSet src, PageSetOut dst, int W, int H, int cut)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const uint8_t* sp = src.page(blockIdx.z);
    int s[C], q[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) s[ch] = q[ch] = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const uint8_t* row = sp + (size_t)min(max(y + dy, 0), H - 1) * src.step;
        for (int dx = -1; dx <= 1; ++dx) {
            const uint8_t* px = row + (size_t)min(max(x + dx, 0), W - 1) * C;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const int p = px[ch];
                s[ch] += p;
                q[ch] += p * p;
            }
        }
    }
    bool all = true;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) all = all && 9 * q[ch] - s[ch] * s[ch] >= cut;
    dst.page(blockIdx.z)[(size_t)y * dst.step + x] = all ? 255 : 0;
}

int variance_mask_run(int C, int cut, const PageSet& src, const PageSetOut& dst, int n, int W, int H, hipStream_t hs)
{
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)n);
    if (C == 1) hipLaunchKernelGGL(k_variance_mask<1>, grid, dim3(256), 0, hs, src, dst, W, H, cut);
    else hipLaunchKernelGGL(k_variance_mask<3>, grid, dim3(256), 0, hs, src, dst, W, H, cut);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// a &= b; grid as above
__global__ __launch_bounds__(256) void k_and_planes(PageSetOut a, PageSet b, int W)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    uint8_t* p = a.page(blockIdx.z) + (size_t)blockIdx.y * a.step + x;
    *p = *p & b.page(blockIdx.z)[(size_t)blockIdx.y * b.step + x];
}

__global__ __launch_bounds__(256) void k_copy_plane(PageSet s, PageSetOut d, int W)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    d.page(blockIdx.z)[(size_t)blockIdx.y * d.step + x] = s.page(blockIdx.z)[(size_t)blockIdx.y * s.step + x];
}

// ---- the ordered paint ---------------------------------------------------------------------------------------------------------

struct PaintJob {
    int W, H;
    int r0, r1;           // rectangles [r0, r1) of the call ...
    int rect_base;        // ... of which `rects` holds those from rect_base on
    int n_pages;
    int fill;             // the resolve pass also writes 255 where no rectangle of this pass lies (the first pass)
    const int32_t* rects;      // x, y, w, h, cut, below
    const int32_t* offsets;    // n_pages + 1: the rectangles of page i are [offsets[i], offsets[i + 1])
    unsigned* large;           // [0]: how many; then their indices
    int32_t* owner;            // per page a plane of W * H words: the largest index + 1 of the pass's rectangles over the pixel
    size_t owner_page;         // words from page to page
};

__device__ __forceinline__ int paint_page_of(const PaintJob& j, int r)
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
__device__ __forceinline__ bool paint_load_rect(const PaintJob& j, int r, int* x, int* y, int* w, int* h)
{
    const int32_t* q = j.rects + kRectWords * (size_t)(r - j.rect_base);
    *x = q[0]; *y = q[1]; *w = q[2]; *h = q[3];
    return *x >= 0 && *y >= 0 && *w > 0 && *h > 0 && *w <= j.W - *x && *h <= j.H - *y;
}

// grid = ceil((r1 - r0) / 4) workgroups of four wavefronts
__global__ __launch_bounds__(256) void k_paint_small(PaintJob j)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = j.r0 + blockIdx.x * 4 + wave;
    int x = 0, y = 0, w = 0, h = 0;
    if (r >= j.r1 || !paint_load_rect(j, r, &x, &y, &w, &h)) return;
    const int area = w * h;   // (a side is at most 32768: the product fits)
    if (area > kPaintSmallArea) {
        if (lane == 0) j.large[1 + atomicAdd(&j.large[0], 1u)] = (unsigned)r;
        return;
    }
    int32_t* o = j.owner + (size_t)paint_page_of(j, r) * j.owner_page + (size_t)y * j.W + x;
    for (int i = lane; i < area; i += 64) {
        const int yy = i / w, xx = i - yy * w;
        atomicMax(&o[(size_t)yy * j.W + xx], r + 1);
    }
}

// grid = kPaintLargeGrid; item = (large rectangle, slice)
__global__ __launch_bounds__(256) void k_paint_large(PaintJob j)
{
    const int t = threadIdx.x;
    const unsigned items = j.large[0] * (unsigned)kPaintSlices;
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const int r = (int)j.large[1 + item / kPaintSlices], slice = (int)(item % kPaintSlices);
        int x, y, w, h;
        if (!paint_load_rect(j, r, &x, &y, &w, &h) || slice >= h) continue;
        int32_t* o = j.owner + (size_t)paint_page_of(j, r) * j.owner_page + (size_t)y * j.W + x;
        for (int yy = slice; yy < h; yy += kPaintSlices)
            for (int xx = t; xx < w; xx += 256) atomicMax(&o[(size_t)yy * j.W + xx], r + 1);
    }
}

// grid = (ceil(W / 256), H, pages)
__global__ __launch_bounds__(256) void k_paint_resolve(PaintJob j, PageSet gray, PageSetOut dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, page = blockIdx.z;
    if (x >= j.W) return;
    const int o = j.owner[(size_t)page * j.owner_page + (size_t)y * j.W + x];
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + x;
    if (o == 0) {
        if (j.fill) *d = 255;
        return;
    }
    const int32_t* q = j.rects + kRectWords * (size_t)(o - 1 - j.rect_base);
    const int p = gray.page(page)[(size_t)y * gray.step + x];
    *d = (q[5] ? p < q[4] : p >= q[4]) ? 255 : 0;
}

size_t owner_plane_bytes(int W, int H) { return r256((size_t)W * H * sizeof(int32_t)); }
size_t paint_list_bytes(int rects) { return r256(((size_t)rects + 1) * sizeof(unsigned)); }

// rectangles [r0, r1) of the call over n pages; j: everything but r0, r1, fill.  owner: n planes; j.large: r1 - r0 + 1 words.
int paint_pass(PaintJob j, int r0, int r1, bool fill, const PageSet& gray, const PageSetOut& dst, int n, hipStream_t hs)
{
    j.r0 = r0;
    j.r1 = r1;
    j.fill = fill;
    PRL_HIP_CHECK(hipMemsetAsync(j.owner, 0, j.owner_page * sizeof(int32_t) * (size_t)n, hs));
    if (r1 > r0) {
        PRL_HIP_CHECK(hipMemsetAsync(j.large, 0, sizeof(unsigned), hs));
        hipLaunchKernelGGL(k_paint_small, dim3((unsigned)((r1 - r0 + 3) / 4)), dim3(256), 0, hs, j);
        hipLaunchKernelGGL(k_paint_large, dim3(kPaintLargeGrid), dim3(256), 0, hs, j);
    }
    hipLaunchKernelGGL(k_paint_resolve, dim3((unsigned)((j.W + 255) / 256), (unsigned)j.H, (unsigned)n), dim3(256), 0, hs, j, gray, dst);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

int fb_bad_arg(const char* why)
{
    set_error_detail(why);
    return PRL_ERR_BAD_ARG;
}

int offsets_ok(const PageArgs& a, const int32_t* offsets, const int32_t* d_rects)
{
    if (!offsets || offsets[0] != 0) return fb_bad_arg("rect_paint: the offsets must start at 0");
    for (int i = 0; i < a.n_pages; ++i)
        if (offsets[i + 1] < offsets[i]) return fb_bad_arg("rect_paint: the offsets must not decrease");
    if (offsets[a.n_pages] > 0 && !d_rects) return PRL_ERR_BAD_ARG;
    return PRL_OK;
}

// ---- prl::binarizeFBCITB -----------------------------------------------------------------------------------------------------

struct FbSpec {
    bool canny_required, variances_required;   // the caller's flags
    bool use_canny, use_variances;             // both false switches both stages on, the flags "required" stay false
    bool clahe, bilateral, morphology, canny_on_variances;
    double variance_threshold, clip_limit, max_area;
    CedSpec ced;
    BilTables bil;
};

// EMPTY; BAD_CHANNELS; the parameters (BAD_ARG, BAD_WINDOW for a blur side above the limit); BAD_ARG for the pages
int fb_checks(const PageArgs& a, int channels, const prl_fbcitb_params* p, bool batch, FbSpec* sp)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels != 1 && channels != 3) return PRL_ERR_BAD_CHANNELS;
    if (!p) return PRL_ERR_BAD_ARG;
    for (double v : {p->variance_map_threshold, p->clahe_clip_limit, p->gaussian_blur_kernel_size, p->canny_upper_threshold_coeff,
                     p->canny_lower_threshold_coeff, p->bounding_rectangle_max_area, p->bilateral_kernel_intensity_sigma,
                     p->bilateral_kernel_spatial_sigma})
        if (!std::isfinite(v)) return fb_bad_arg("binarizeFBCITB: a parameter is not finite");
    sp->canny_required = p->use_canny != 0;
    sp->variances_required = p->use_variances_map != 0;
    sp->use_canny = sp->canny_required;
    sp->use_variances = sp->variances_required;
    if (!sp->canny_required && !sp->variances_required) sp->use_canny = sp->use_variances = true;
    sp->clahe = p->use_clahe != 0;
    sp->bilateral = p->use_bilateral != 0;
    sp->morphology = p->use_morphology != 0;
    sp->canny_on_variances = p->use_canny_on_variances != 0;
    sp->variance_threshold = p->variance_map_threshold;
    sp->clip_limit = p->clahe_clip_limit;
    sp->max_area = p->bounding_rectangle_max_area;
    if (sp->bilateral && !bil_tables(p->bilateral_kernel_size, p->bilateral_kernel_intensity_sigma, p->bilateral_kernel_spatial_sigma, &sp->bil))
        return fb_bad_arg("binarizeFBCITB: the bilateral filter's side 2 * radius + 1 is above 31");
    const double size = p->gaussian_blur_kernel_size;
    sp->ced = CedSpec{size >= 2147483647.0 ? 2147483647 : size <= -2147483647.0 ? -2147483647 : (int)size, p->canny_upper_threshold_coeff,
                      p->canny_lower_threshold_coeff, 1};
    if (sp->use_canny) {   // CannyEdgeDetection's own checks: the reference runs it (and throws) even where its map is not used
        if (ced_spec_check(sp->ced)) return fb_bad_arg("binarizeFBCITB: CannyEdgeDetection refuses its arguments");
        if (sp->ced.size > PRL_GAUSS_MAX_SIDE) return PRL_ERR_BAD_WINDOW;
    }
    if ((st = pages_rows_ok(a, channels, 1, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    return pages_overlap_ok(a, channels, 1, false);
}

int fb_batch(const PageArgs& a, int C, const FbSpec& sp, int32_t* counts, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const int W = a.width, H = a.height;
    const size_t plane = r256((size_t)W * H), cplane = r256((size_t)W * C * H), oplane = owner_plane_bytes(W, H);
    const bool run_canny = sp.canny_required;   // (without the flag the reference computes the map and drops it)
    const CedSpec ced = run_canny ? sp.ced : CedSpec{3, 0.0, 0.0, 1};
    // a page's share of the workspace beside CannyEdgeDetection's: two processed pages, the edge map, the variance mask and its
    // edges, the gray plane, the mask before the morphology, the owner plane, CLAHE's tables
    const size_t per_page = 2 * cplane + 5 * plane + oplane + (sp.clahe ? enhance_contrast_channels_work_per_page(C, false) : 0);
    int chunk = ced_pages_per_chunk(ced, a.n_pages, W, H, C, per_page);
    chunk = std::min(chunk, (int)std::max<size_t>(1, ((size_t)1 << 30) / (2 * plane)));   // the read-back's pinned block: 1 GiB at most
    const size_t contrast_bytes = sp.clahe ? r256(enhance_contrast_channels_work_bytes(C, false, chunk)) : 0;
    const size_t rect_bytes = r256((size_t)kPaintChunk * kRectWords * sizeof(int32_t));
    const size_t stage_bytes = std::max({r256(ced_work_bytes(ced, chunk, W, H, C)), r256(canny_work_bytes(chunk, W, H)), rect_bytes});
    const size_t off_bytes = r256(((size_t)chunk + 1) * sizeof(int32_t));
    WorkScope w;
    int st = w.open(stream, (2 * cplane + 5 * plane + oplane) * (size_t)chunk + contrast_bytes + stage_bytes,
                    std::max(ced_small_bytes(chunk, C), off_bytes + paint_list_bytes(kPaintChunk)),
                    std::max({ced_pinned_bytes(chunk, C), canny_pinned_bytes(chunk), 2 * plane * (size_t)chunk}));
    if (st != PRL_OK) return st;
    const hipStream_t hs = w.stream;
    uint8_t* P = w.scratch();                        // the processed pages (CLAHE)
    uint8_t* Q = P + cplane * (size_t)chunk;         // ... (the bilateral filter)
    uint8_t* E = Q + cplane * (size_t)chunk;         // CannyEdgeDetection's maps
    uint8_t* V = E + plane * (size_t)chunk;          // the variance masks
    uint8_t* V2 = V + plane * (size_t)chunk;         // cv::Canny of them
    uint8_t* G = V2 + plane * (size_t)chunk;         // the gray planes
    uint8_t* T = G + plane * (size_t)chunk;          // the painted masks before the morphology
    uint8_t* O = T + plane * (size_t)chunk;          // the owner planes
    uint8_t* contrast_work = O + oplane * (size_t)chunk;
    uint8_t* stage_work = contrast_work + contrast_bytes;
    const int cut = fb_variance_cut(sp.variance_threshold);
    for (int first = 0; first < a.n_pages; first += chunk) {
        const int n = std::min(chunk, a.n_pages - first);
        const PageSet src = src_pages(a, first);
        const PageSetOut dst = dst_pages(a, first);
        const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)n);
        // 1. EnhanceLocalContrastByCLAHE(clip, false) and cv::bilateralFilter, each per channel
        PageSet cur = src;
        if (sp.clahe) {
            const PageSetOut pp = page_set_out(P, cplane, (size_t)W * C);
            if ((st = enhance_contrast_channels_run(C, false, sp.clip_limit, cur, pp, n, W, H, chunk, contrast_work, hs)) != PRL_OK) return st;
            cur = as_source(pp);
        }
        if (sp.bilateral) {
            const PageArgs ba{n, cur.base, cur.page_stride, cur.step, W, H, Q, cplane, (size_t)W * C};
            if ((st = bilateral_planes_run(sp.bil, ba, C, hs)) != PRL_OK) return st;
            cur = page_set(Q, cplane, (size_t)W * C);
        }
        // 2. CannyEdgeDetection of the processed page
        const PageSetOut ep = page_set_out(E, plane, (size_t)W);
        if (run_canny && (st = ced_run(ced, cur, ep, n, W, H, C, stage_work, w.small(), w.pinned<unsigned>(), hs)) != PRL_OK) return st;
        // 3. the variance mask of the ORIGINAL page, cv::Canny(64, 128) on it, the AND
        PageSetOut map = ep;
        if (sp.use_variances) {
            map = page_set_out(V, plane, (size_t)W);
            if ((st = variance_mask_run(C, cut, src, map, n, W, H, hs)) != PRL_OK) return st;
            if (sp.canny_on_variances) {
                const PageSetOut v2 = page_set_out(V2, plane, (size_t)W);
                if ((st = canny_run(W, H, 64, 128, as_source(map), v2, n, stage_work, w.pinned<unsigned>(), hs)) != PRL_OK) return st;
                map = v2;
            }
            if (sp.canny_required && sp.variances_required) hipLaunchKernelGGL(k_and_planes, grid, dim3(256), 0, hs, map, as_source(ep), W);
        }
        // 4. the gray plane of the processed page (three equal channels stand for a gray source: the plane itself)
        const PageSetOut gp = page_set_out(G, plane, (size_t)W);
        if (C == 3) {
            if ((st = prl_hip_bgr2gray_batch_device(n, 3, cur.base, cur.page_stride, cur.step, W, H, G, plane, (size_t)W, hs)) != PRL_OK) return st;
        } else {
            hipLaunchKernelGGL(k_copy_plane, grid, dim3(256), 0, hs, cur, gp, W);
        }
        PRL_HIP_CHECK(hipGetLastError());
        // 5. ONE read-back: the maps, then the gray planes
        uint8_t* h_maps = w.pinned();
        uint8_t* h_gray = h_maps + plane * (size_t)n;
        PRL_HIP_CHECK(hipMemcpyAsync(h_maps, map.base, plane * (size_t)n, hipMemcpyDeviceToHost, hs));
        PRL_HIP_CHECK(hipMemcpyAsync(h_gray, G, plane * (size_t)n, hipMemcpyDeviceToHost, hs));
        PRL_HIP_CHECK(hipStreamSynchronize(hs));
        // 6. the contours, RemoveChildrenContours, the filters and every kept contour's decision, per page on the host pool
        std::vector<std::vector<FbRect>> rects((size_t)n);
        host_pool_for(n, [&](int i) {
            const FbCounts c = fb_contours(h_maps + plane * (size_t)i, (size_t)W, h_gray + plane * (size_t)i, (size_t)W, W, H, sp.max_area,
                                           &rects[(size_t)i]);
            if (counts) {
                int32_t* o = counts + 3 * (size_t)(first + i);
                o[0] = c.found; o[1] = c.approved; o[2] = c.kept;
            }
        });
        std::vector<int32_t> offsets((size_t)n + 1, 0), flat;
        for (int i = 0; i < n; ++i) {
            for (const FbRect& r : rects[(size_t)i]) flat.insert(flat.end(), {r.x, r.y, r.w, r.h, r.cut, r.below});
            if (flat.size() / kRectWords > 0x7ffffff0u) return fb_bad_arg("binarizeFBCITB: too many rectangles");
            offsets[(size_t)i + 1] = (int32_t)(flat.size() / kRectWords);
        }
        // 7. the upload and the paint, kPaintChunk rectangles a pass in index order; 8. dilate(2), erode(2)
        const int total = offsets[(size_t)n];
        int32_t* d_off = w.small<int32_t>();
        int32_t* d_rects = reinterpret_cast<int32_t*>(stage_work);
        PRL_HIP_CHECK(hipMemcpyAsync(d_off, offsets.data(), ((size_t)n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, hs));
        PaintJob j{};
        j.W = W; j.H = H; j.n_pages = n;
        j.rects = d_rects; j.offsets = d_off;
        j.large = reinterpret_cast<unsigned*>(w.small() + off_bytes);
        j.owner = reinterpret_cast<int32_t*>(O);
        j.owner_page = oplane / sizeof(int32_t);
        const PageSetOut painted = sp.morphology ? page_set_out(T, plane, (size_t)W) : dst;
        for (int r0 = 0; r0 == 0 || r0 < total; r0 += kPaintChunk) {
            const int r1 = std::min(total, r0 + kPaintChunk);
            if (r1 > r0)
                PRL_HIP_CHECK(hipMemcpyAsync(d_rects, flat.data() + (size_t)kRectWords * r0, (size_t)(r1 - r0) * kRectWords * sizeof(int32_t),
                                             hipMemcpyHostToDevice, hs));
            j.rect_base = r0;
            if ((st = paint_pass(j, r0, r1, r0 == 0, as_source(gp), painted, n, hs)) != PRL_OK) return st;
        }
        if (sp.morphology && (st = morph_run(2, as_source(painted), n, W, H, dst, hs)) != PRL_OK) return st;
        PRL_HIP_CHECK(hipStreamSynchronize(hs));   // (`flat` and `offsets` end with this scope)
    }
    return PRL_OK;
}

}  // namespace

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_variance_mask_batch_device(int n_pages, int channels, double threshold, const uint8_t* d_src, size_t src_page_stride,
                                       size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                       void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels != 1 && channels != 3) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, 1, true)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    if ((st = pages_overlap_ok(a, channels, 1, false)) != PRL_OK || n_pages == 0) return st;
    int dev;   // the device check alone: no workspace
    if ((st = current_device(&dev)) != PRL_OK) return st;
    const int cut = fb_variance_cut(threshold);
    const int chunk = stage_chunk(n_pages, 0);
    for (int first = 0; first < n_pages; first += chunk)
        if ((st = variance_mask_run(channels, cut, src_pages(a, first), dst_pages(a, first), std::min(chunk, n_pages - first), width, height,
                                    static_cast<hipStream_t>(stream))) != PRL_OK)
            return st;
    return PRL_OK;
}

int prl_hip_find_contours_tree(const uint8_t* map, size_t step, int width, int height, int32_t* points, int max_points, int32_t* contours,
                               int max_contours, int* n_points, int* n_contours)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!map || step < (size_t)width || !n_points || !n_contours || max_points < 0 || max_contours < 0 || (max_points && !points) ||
        (max_contours && !contours) || width > kStageMaxSide || height > kStageMaxSide)
        return PRL_ERR_BAD_ARG;
    std::vector<CtPoint> pts;
    std::vector<CtNode> nodes;
    ct_find_contours_tree(map, step, width, height, &pts, &nodes);
    *n_points = (int)pts.size();
    *n_contours = (int)nodes.size();
    if ((int)pts.size() > max_points || (int)nodes.size() > max_contours) return PRL_OK;   // the counts alone: call again with room
    for (size_t i = 0; i < pts.size(); ++i) {
        points[2 * i] = pts[i].x;
        points[2 * i + 1] = pts[i].y;
    }
    for (size_t i = 0; i < nodes.size(); ++i) {
        const CtNode& nd = nodes[i];
        const int32_t rec[6] = {nd.count, nd.hole, nd.next, nd.prev, nd.child, nd.parent};
        std::copy(rec, rec + 6, contours + 6 * i);
    }
    return PRL_OK;
}

int prl_hip_remove_children_contours(const int32_t* contours, int n_contours, uint8_t* approved)
{
    if (n_contours < 0 || (n_contours && (!contours || !approved))) return PRL_ERR_BAD_ARG;
    std::vector<CtNode> nodes((size_t)n_contours);
    for (int i = 0; i < n_contours; ++i) {
        const int32_t* q = contours + 6 * (size_t)i;
        nodes[(size_t)i] = CtNode{0, q[0], q[1], q[2], q[3], q[4], q[5]};
        for (int k = 2; k < 6; ++k)
            if (q[k] < -1 || q[k] >= n_contours) return PRL_ERR_BAD_ARG;
        if (q[5] >= i || (q[2] >= 0 && q[2] <= i) || (q[4] >= 0 && q[4] <= i))
            return fb_bad_arg("remove_children_contours: the contours must be in pre-order");
    }
    std::vector<uint8_t> ok;
    ct_remove_children(nodes, &ok);
    std::copy(ok.begin(), ok.end(), approved);
    return PRL_OK;
}

int prl_hip_fbcitb_contours(const uint8_t* map, size_t map_step, const uint8_t* gray, size_t gray_step, int width, int height,
                            double max_area, int32_t* rects, int max_rects, int32_t counts[3])
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!map || !gray || map_step < (size_t)width || gray_step < (size_t)width || !counts || max_rects < 0 || (max_rects && !rects) ||
        width > kStageMaxSide || height > kStageMaxSide || !std::isfinite(max_area))
        return PRL_ERR_BAD_ARG;
    std::vector<FbRect> rs;
    const FbCounts c = fb_contours(map, map_step, gray, gray_step, width, height, max_area, &rs);
    counts[0] = c.found; counts[1] = c.approved; counts[2] = c.kept;
    if (c.kept > max_rects) return PRL_OK;   // the counts alone: call again with room
    for (size_t i = 0; i < rs.size(); ++i) {
        const int32_t rec[kRectWords] = {rs[i].x, rs[i].y, rs[i].w, rs[i].h, rs[i].cut, rs[i].below};
        std::copy(rec, rec + kRectWords, rects + kRectWords * i);
    }
    return PRL_OK;
}

int prl_hip_rect_paint_batch_device(int n_pages, const int32_t* rect_offsets, const int32_t* d_rects, const uint8_t* d_gray,
                                    size_t gray_page_stride, size_t gray_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride,
                                    size_t dst_step, void* stream)
{
    const PageArgs a{n_pages, d_gray, gray_page_stride, gray_step, width, height, d_dst, dst_page_stride, dst_step};
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if ((st = pages_rows_ok(a, 1, 1, true)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    if ((st = pages_overlap_ok(a, 1, 1, false)) != PRL_OK || n_pages == 0) return st;
    if ((st = offsets_ok(a, rect_offsets, d_rects)) != PRL_OK) return st;
    const int total = rect_offsets[n_pages];
    const size_t oplane = owner_plane_bytes(width, height);
    const int chunk = stage_chunk(n_pages, oplane);
    const size_t off_bytes = r256(((size_t)n_pages + 1) * sizeof(int32_t));
    WorkScope w;
    if ((st = w.open(stream, oplane * (size_t)chunk, off_bytes + paint_list_bytes(total), off_bytes)) != PRL_OK) return st;
    // the offsets go up through the pinned block as localotsu.hip's do: the caller's array is free when the call returns
    DeviceCtx* ctx = w.ctx;
    if (ctx->pinned_use) PRL_HIP_CHECK(hipEventSynchronize(ctx->pinned_use));
    else PRL_HIP_CHECK(hipEventCreateWithFlags(&ctx->pinned_use, hipEventDisableTiming));
    std::memcpy(ctx->pinned, rect_offsets, ((size_t)n_pages + 1) * sizeof(int32_t));
    int32_t* d_off = w.small<int32_t>();
    PRL_HIP_CHECK(hipMemcpyAsync(d_off, ctx->pinned, ((size_t)n_pages + 1) * sizeof(int32_t), hipMemcpyHostToDevice, w.stream));
    PRL_HIP_CHECK(hipEventRecord(ctx->pinned_use, w.stream));
    PaintJob j{};
    j.W = width; j.H = height;
    j.rects = d_rects; j.rect_base = 0;
    j.large = reinterpret_cast<unsigned*>(w.small() + off_bytes);
    j.owner = w.scratch<int32_t>();
    j.owner_page = oplane / sizeof(int32_t);
    for (int first = 0; first < n_pages; first += chunk) {   // a chunk of pages and the rectangles of exactly those pages
        const int n = std::min(chunk, n_pages - first);
        j.n_pages = n;
        j.offsets = d_off + first;
        if ((st = paint_pass(j, rect_offsets[first], rect_offsets[first + n], true, src_pages(a, first), dst_pages(a, first), n, w.stream)) != PRL_OK)
            return st;
    }
    return PRL_OK;
}

void prl_hip_default_fbcitb_params(prl_fbcitb_params* p)
{
    if (!p) return;
    *p = prl_fbcitb_params{};
    p->use_canny = p->use_variances_map = p->use_clahe = p->use_bilateral = p->use_morphology = p->use_canny_on_variances = 1;
    p->use_other_colorspace = 0;
    p->bilateral_kernel_size = 5;
    p->variance_map_threshold = 200.0;
    p->clahe_clip_limit = 2.0;
    p->gaussian_blur_kernel_size = 9.0;
    p->canny_upper_threshold_coeff = 0.6;
    p->canny_lower_threshold_coeff = 0.4;
    p->bounding_rectangle_max_area = 0.3;
    p->bilateral_kernel_intensity_sigma = 150.0;
    p->bilateral_kernel_spatial_sigma = 150.0;
    p->bounding_rect_max_area_coeff = 0.3;
}

int prl_hip_binarize_fbcitb_batch_device(const prl_fbcitb_params* params, int n_pages, int channels, const uint8_t* d_src,
                                         size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                         size_t dst_page_stride, size_t dst_step, int32_t* counts, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    FbSpec sp;
    const int st = fb_checks(a, channels, params, true, &sp);
    return st != PRL_OK ? st : fb_batch(a, channels, sp, counts, stream);
}

int prl_hip_binarize_fbcitb_host(const prl_fbcitb_params* params, int channels, const uint8_t* src, size_t src_step, int width, int height,
                                 uint8_t* dst, size_t dst_step, int32_t* counts)
{
    const PageArgs h{1, src, 0, src_step, width, height, dst, 0, dst_step};
    FbSpec sp;
    const int st = fb_checks(h, channels, params, false, &sp);
    if (st != PRL_OK) return st;
    return stage_host_pages(h, channels, 1, width, height,
                            [&](const PageArgs& page, hipStream_t s) { return fb_batch(page, channels, sp, counts, s); });
}

}  // extern "C"
