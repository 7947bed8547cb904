// deskew.hip — prl::deskew for pages resident in device memory: the composition of the angle search
// (ppht.hip) and the rotation (rotate.hip).
//
// Reference: src/deskew/deskew.cpp:208-251 (gray -> Otsu -> findAngle -> rotate).  A pass of at most deskew_pages_per_pass pages
// is deskew_find (gray, Otsu, HoughLinesP, the angle vote: a WarpPage record per page) and deskew_apply (prl::rotate by those
// records); the chain (glue.hip) runs the two halves apart and sizes its passes with deskew_ink_census.
// findOrientation (deskew.cpp:238, Leptonica pixOrientDetectDwa) is a no-op for the 1-channel page prl::deskew hands it
// (oracle header); prl::findOrientation of the host layer returns that 0 (prl_host.cpp), no kernel is built for it.
// Also here: host_roundtrip, the single-page host path of the deskew, rotate and find_angle entries.
#include <algorithm>
#include <cfloat>
#include <vector>

#include "ppht_plan.h"
#include "prl_internal.h"

namespace prl_hip {

// pages per pass of prl::deskew: bounded by a workspace budget (mask + accumulator + point lists + gray page per page)
int deskew_pages_per_pass(int n_pages, int width, int height)
{
    return ppht_pages_per_pass(n_pages, width, height, env_knobs().deskew_work_mb << 20);
}

// Ink census (round 5): the number of points HoughLinesP will see on each page - the pixels at or below the page's Otsu threshold -
// from the gray histogram alone (one streaming read of the pages; no mask, no lists).  The chain sizes its passes with it: the
// search of a pass lasts as long as its heaviest page (0.6 us per point through one CU's atomic path), so a batch of photographs
// with a dark table in them wants few large passes, text scans the usual ones.  Synchronises `hs`.
int deskew_ink_census(DeviceCtx* ctx, int n_pages, int channels, const PageSet& src, int width, int height,
                      std::vector<unsigned>* points, hipStream_t hs)
{
    points->assign((size_t)n_pages, 0u);
    const size_t gray_page = r256((size_t)width * height);
    const int sub = channels == 1 ? std::min(n_pages, 4096) : (int)std::max<size_t>(1, std::min<size_t>((size_t)n_pages, ((size_t)512 << 20) / gray_page));
    std::lock_guard<std::mutex> lk(ctx->ppht_mu);
    int st = ensure_buffer(&ctx->ppht_buf[0], &ctx->ppht_bytes[0], r256((size_t)sub * 256 * 4) + r256((size_t)sub * 4));
    if (st != PRL_OK) return st;
    unsigned* d_hist = static_cast<unsigned*>(ctx->ppht_buf[0]);
    int* d_thr = reinterpret_cast<int*>(static_cast<uint8_t*>(ctx->ppht_buf[0]) + r256((size_t)sub * 256 * 4));
    if (channels != 1) {
        st = ensure_buffer(&ctx->ppht_buf[2], &ctx->ppht_bytes[2], gray_page * (size_t)sub);
        if (st != PRL_OK) return st;
    }
    std::vector<unsigned> h_hist((size_t)sub * 256);
    std::vector<int> h_thr((size_t)sub);
    for (int first = 0; first < n_pages; first += sub) {
        const int cnt = std::min(sub, n_pages - first);
        PageSet g = pages_from(src, first);
        if (channels != 1) {
            uint8_t* gray_ws = static_cast<uint8_t*>(ctx->ppht_buf[2]);
            st = prl_hip_bgr2gray_batch_device(cnt, channels, g.base, g.page_stride, g.step, width, height, gray_ws, gray_page,
                                               (size_t)width, hs);
            if (st != PRL_OK) return st;
            g = page_set(gray_ws, gray_page, (size_t)width);
        }
        if ((st = otsu_thresholds(g, width, height, cnt, d_hist, d_thr, hs)) != PRL_OK) return st;
        PRL_HIP_CHECK(hipMemcpyAsync(h_hist.data(), d_hist, (size_t)cnt * 256 * 4, hipMemcpyDeviceToHost, hs));
        PRL_HIP_CHECK(hipMemcpyAsync(h_thr.data(), d_thr, (size_t)cnt * 4, hipMemcpyDeviceToHost, hs));
        PRL_HIP_CHECK(hipStreamSynchronize(hs));
        for (int i = 0; i < cnt; ++i) {
            unsigned long long n = 0;
            for (int v = 0; v <= std::min(255, std::max(-1, h_thr[(size_t)i])); ++v) n += h_hist[(size_t)i * 256 + v];
            (*points)[(size_t)(first + i)] = (unsigned)std::min<unsigned long long>(n, 0xffffffffull);
        }
    }
    return PRL_OK;
}

// First half of prl::deskew on `cnt` pages (cnt <= deskew_pages_per_pass): gray -> Otsu -> HoughLinesP -> angle vote.
int deskew_find(DeviceCtx* ctx, int cnt, int channels, const PageSet& src, int width, int height, DeskewPlan* plan, hipStream_t hs,
                SearchStart* start)
{
    const size_t gray_page = r256((size_t)width * height);
    std::lock_guard<std::mutex> lk(ctx->ppht_mu);
    int st;
    PageSet g = src;
    if (channels != 1) {  // deskew.cpp:214-217
        st = ensure_buffer(&ctx->ppht_buf[2], &ctx->ppht_bytes[2], gray_page * (size_t)cnt);
        if (st != PRL_OK) return st;
        uint8_t* gray_ws = static_cast<uint8_t*>(ctx->ppht_buf[2]);
        st = prl_hip_bgr2gray_batch_device(cnt, channels, src.base, src.page_stride, src.step, width, height, gray_ws, gray_page,
                                           (size_t)width, hs);
        if (st != PRL_OK) return st;
        g = page_set(gray_ws, gray_page, (size_t)width);
    }
    std::vector<std::vector<int>> lines;
    // cv::threshold(..., THRESH_BINARY | THRESH_OTSU) (:224) + findAngle's bitwise_not (:146): points = (p <= otsu)
    st = find_angle_segments(ctx, cnt, g, width, height, true, &lines, hs, start);
    if (st != PRL_OK) return st;
    plan->warp.resize((size_t)cnt);
    plan->wh.resize(2 * (size_t)cnt);
    plan->angles.resize((size_t)cnt);
    plan->max_ow = plan->max_oh = 0;
    for (int i = 0; i < cnt; ++i) {
        const double angle = vote_angle(lines[(size_t)i].data(), (int)(lines[(size_t)i].size() / 4));
        plan->angles[(size_t)i] = angle;
        const bool rot = (angle != 0) && (angle <= DBL_MAX && angle >= -DBL_MAX);  // deskew.cpp:228
        WarpPage& wp = plan->warp[(size_t)i];
        fill_warp_page(width, height, angle, !rot, &wp);
        plan->wh[2 * (size_t)i] = wp.ow;
        plan->wh[2 * (size_t)i + 1] = wp.oh;
        plan->max_ow = std::max(plan->max_ow, wp.ow);
        plan->max_oh = std::max(plan->max_oh, wp.oh);
    }
    return PRL_OK;
}

// Second half: rotate.
int deskew_apply(DeviceCtx* ctx, const DeskewPlan& plan, int cnt, int channels, const PageSet& src, int width, int height,
                 const PageSetOut& dst, hipStream_t hs)
{
    if (plan.warp.size() != (size_t)cnt) return PRL_ERR_BAD_ARG;
    const size_t bytes = sizeof(WarpPage) * (size_t)cnt;
    WorkScope w;
    const int st = w.open_on(ctx, hs, 0, bytes, 0);
    if (st != PRL_OK) return st;
    PRL_HIP_CHECK(hipMemcpyAsync(w.small(), plan.warp.data(), bytes, hipMemcpyHostToDevice, hs));
    PRL_HIP_CHECK(hipStreamSynchronize(hs));  // pageable source
    return launch_warp(channels, src, dst, width, height, cnt, plan.max_ow, plan.max_oh, w.small<const WarpPage>(), hs);
}

int deskew_pages(DeviceCtx* ctx, int cnt, int channels, const PageSet& src, int width, int height, const PageSetOut& dst,
                 int32_t* out_wh, double* angles, hipStream_t hs)
{
    DeskewPlan plan;
    int st = deskew_find(ctx, cnt, channels, src, width, height, &plan, hs);
    if (st != PRL_OK) return st;
    std::copy(plan.wh.begin(), plan.wh.end(), out_wh);
    if (angles) std::copy(plan.angles.begin(), plan.angles.end(), angles);
    return deskew_apply(ctx, plan, cnt, channels, src, width, height, dst, hs);
}

int host_roundtrip(const PageArgs& h, int channels, int max_w, int max_h, const int* out_w, const int* out_h,
                   const std::function<int(const PageArgs&, hipStream_t)>& stage)
{
    DeviceCtx* ctx;
    int st = current_ctx(&ctx);
    if (st != PRL_OK) return st;
    const size_t in_row = (size_t)h.width * channels, out_row_max = (size_t)max_w * channels;
    const size_t in_bytes = r256(in_row * (size_t)h.height), out_bytes = h.dst ? r256(out_row_max * (size_t)max_h) : 0;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    // own buffers: the stage itself uses the shared staging area for its gray pages
    PRL_HIP_CHECK(hipMalloc(&d_in, in_bytes + 2 * out_bytes));
    struct Free { uint8_t* p; ~Free() { (void)hipFree(p); } } free_d_in{d_in};  // every exit, the error returns of PRL_HIP_CHECK included
    d_out = d_in + in_bytes;
    uint8_t* d_packed = d_out + out_bytes;  // the result with rows packed to its own width
    hipStream_t stream = nullptr;
    {
        std::lock_guard<std::mutex> slk(ctx->stage_mu);
        st = ensure_stage_pinned(ctx, std::max(in_bytes, out_bytes));
        if (st == PRL_OK) st = stage_upload(ctx, 0, h.src, h.src_step, in_row, h.height, d_in, stream);
        if (st == PRL_OK) st = hipStreamSynchronize(stream) == hipSuccess ? PRL_OK : PRL_ERR_HIP;
    }
    if (st == PRL_OK) st = stage(PageArgs{1, d_in, in_bytes, in_row, h.width, h.height, h.dst ? d_out : nullptr, out_bytes, out_row_max}, stream);
    if (st != PRL_OK || !h.dst) return st;
    if (h.dst_step < (size_t)*out_w * channels) return PRL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> slk(ctx->stage_mu);
    // rows of the result are out_row_max apart on the device: fetch them packed
    const size_t out_row = (size_t)*out_w * channels;
    PRL_HIP_CHECK(hipMemcpy2DAsync(d_packed, out_row, d_out, out_row_max, out_row, (size_t)*out_h, hipMemcpyDeviceToDevice, stream));
    return stage_download(ctx, 0, d_packed, out_row, *out_h, h.dst, h.dst_step, stream);
}

}  // namespace prl_hip

using namespace prl_hip;

namespace {
// The checks of prl_hip_deskew_batch_device, in the order tests/test_capi_cpu.py pins: empty; channels; then null pointers, a
// negative page count, source == destination, short rows - a result may be as wide as the page's longer side - and sides
// above 32767.
int deskew_checks(const PageArgs& a, int channels, const int32_t* out_wh)
{
    int st = pages_nonempty(a);   // CV_Assert(!inputImage.empty()), deskew.cpp:210
    if (st != PRL_OK) return st;
    if (channels != 1 && channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    const size_t len = (size_t)std::max(a.width, a.height);
    if ((st = pages_rows_ok(a, channels, 0, true)) != PRL_OK || !a.dst || a.src == a.dst || !out_wh || a.dst_step < len * channels)
        return PRL_ERR_BAD_ARG;
    return pages_sides_ok(a, 32767);
}
}  // namespace

extern "C" {

/*
 * prl::deskew on n_pages device pages (channels 1, 3 or 4).  Every page's result has its own size: len x len
 * (len = max(width, height)) when an angle was found, width x height otherwise (and transposed / same size for exactly
 * +-90 / 180 degrees); out_wh (host, 2 ints per page) receives it, angles (host, optional) findAngle's result in degrees.
 * d_dst pages must have room for len rows of dst_step >= len * channels bytes.  Synchronises the stream.
 */
int prl_hip_deskew_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                int32_t* out_wh, double* angles, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    int st = deskew_checks(a, channels, out_wh);
    if (st != PRL_OK) return st;
    if (n_pages == 0) return PRL_OK;
    DeviceCtx* ctx;
    if ((st = current_ctx(&ctx)) != PRL_OK) return st;
    const int chunk = deskew_pages_per_pass(n_pages, width, height);
    for (int first = 0; first < n_pages; first += chunk) {
        const int cnt = std::min(chunk, n_pages - first);
        st = deskew_pages(ctx, cnt, channels, src_pages(a, first), width, height, dst_pages(a, first), out_wh + 2 * first,
                          angles ? angles + first : nullptr, static_cast<hipStream_t>(stream));
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

/* prl::deskew on one host image; dst must have room for max(width,height)^2 pixels (dst_step >= the result's width * channels,
 * compared after the device stage); *out_w x *out_h is the size of the result, *angle (optional) findAngle's degrees.  The batch
 * entry refuses what is left: sides above 32767. */
int prl_hip_deskew_host(int channels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step,
                        int* out_w, int* out_h, double* angle)
{
    const PageArgs h{1, src, 0, src_step, width, height, dst, 0, dst_step};
    if (pages_nonempty(h) != PRL_OK || !src) return PRL_ERR_EMPTY;
    if (channels != 1 && channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    if (!dst || !out_w || !out_h || pages_rows_ok(h, channels, 0, false) != PRL_OK) return PRL_ERR_BAD_ARG;
    const int len = std::max(width, height);
    int32_t wh[2] = {0, 0};
    double ang = 0;
    const int st = host_roundtrip(h, channels, len, len, &wh[0], &wh[1], [&](const PageArgs& p, hipStream_t s) {
        return prl_hip_deskew_batch_device(1, channels, p.src, p.src_page_stride, p.src_step, width, height, p.dst, p.dst_page_stride,
                                           p.dst_step, wh, &ang, s);
    });
    *out_w = wh[0];
    *out_h = wh[1];
    if (angle) *angle = ang;
    return st;
}

}  // extern "C"
