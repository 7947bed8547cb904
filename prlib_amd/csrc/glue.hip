// glue.hip — SURVEY.md §8f rank 2: the channel adapters and the device-resident hand-off between the hot-path
// stages, so a page goes denoise -> gray -> binarize -> (invert) -> thinning without a host round trip.
//
//   k_bgr2gray : cv::cvtColor(COLOR_BGR2GRAY / BGRA2GRAY) on 8-bit data, the call every binarizer makes first for a
//                colour input (src/binarizations/binarizeSauvola.cpp:51; same line in Niblack/Wolf/NICK/Feng and in
//                src/thinning/thinZhangSuen.cpp:78): 14-bit fixed point (1868 B + 9617 G + 4899 R + 8192) >> 14
//                [upstream, SURVEY.md Appendix B], integer => bit-exact.
//   k_gray2bgr : cv::cvtColor(COLOR_GRAY2BGR): the replicate a user needs in front of prl::denoise, which only
//                accepts 3/4-channel input.
//   k_invert   : cv::bitwise_not: the binarizers emit white = background, thinning thins white (§3.4).
// All three are pure byte streams (HBM-bound: 4, 4 and 2 B per pixel); a thread handles 4 pixels with dword
// accesses when the rows are 4-byte aligned, byte accesses otherwise.
//
// prl_hip_chain_batch_device strings the public entry points together on one stream with its intermediates in the
// device staging workspace.  There is no such function in the reference (a user writes the calls one after the
// other, each through host memory); BASELINE config 5 is this chain.  With deskew it runs in passes: how many pages a pass
// takes and which kernel searches its angles is chain_schedule.h's business (the policy and its measured constants, tested
// on the CPU); here are the search worker (AngleSearch), the split of a pass into runs of equal page size (split_runs) and
// the two pass bodies (pass_whole, pass_split).
#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <thread>
#include <string>
#include <vector>

#include "chain_schedule.h"
#include "prl_internal.h"

namespace prl_hip {
namespace {

__device__ __forceinline__ unsigned gray14(unsigned b, unsigned g, unsigned r)
{
    return (b * 1868u + g * 9617u + r * 4899u + (1u << 13)) >> 14;
}

template <int CH>
__global__ void __launch_bounds__(256) k_bgr2gray(PageSet src, PageSetOut dst, int width, int height)
{
    const int page = blockIdx.z, y = blockIdx.y;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= width) return;
    const uint8_t* s = src.page(page) + (size_t)y * src.step + (size_t)x0 * CH;
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + x0;
    const int n = min(4, width - x0);
    unsigned g[4] = {0, 0, 0, 0};
    if (n == 4 && (((size_t)s) & 3) == 0) {
        const unsigned* q = reinterpret_cast<const unsigned*>(s);
        if (CH == 3) {
            const unsigned w0 = q[0], w1 = q[1], w2 = q[2];  // B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
            g[0] = gray14(w0 & 0xff, (w0 >> 8) & 0xff, (w0 >> 16) & 0xff);
            g[1] = gray14(w0 >> 24, w1 & 0xff, (w1 >> 8) & 0xff);
            g[2] = gray14((w1 >> 16) & 0xff, w1 >> 24, w2 & 0xff);
            g[3] = gray14((w2 >> 8) & 0xff, (w2 >> 16) & 0xff, w2 >> 24);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = gray14(q[i] & 0xff, (q[i] >> 8) & 0xff, (q[i] >> 16) & 0xff);
        }
    } else {
        for (int i = 0; i < n; ++i) g[i] = gray14(s[i * CH], s[i * CH + 1], s[i * CH + 2]);
    }
    if (n == 4 && (((size_t)d) & 3) == 0) {
        *reinterpret_cast<unsigned*>(d) = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
    } else {
        for (int i = 0; i < n; ++i) d[i] = (uint8_t)g[i];
    }
}

template <int CH>
__global__ void __launch_bounds__(256) k_gray2bgr(PageSet src, PageSetOut dst, int width, int height)
{
    const int page = blockIdx.z, y = blockIdx.y;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= width) return;
    const uint8_t* s = src.page(page) + (size_t)y * src.step + x0;
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + (size_t)x0 * CH;
    const int n = min(4, width - x0);
    unsigned g[4] = {0, 0, 0, 0};
    if (n == 4 && (((size_t)s) & 3) == 0) {
        const unsigned w = *reinterpret_cast<const unsigned*>(s);
        g[0] = w & 0xff; g[1] = (w >> 8) & 0xff; g[2] = (w >> 16) & 0xff; g[3] = w >> 24;
    } else {
        for (int i = 0; i < n; ++i) g[i] = s[i];
    }
    if (n == 4 && (((size_t)d) & 3) == 0) {
        unsigned* q = reinterpret_cast<unsigned*>(d);
        if (CH == 3) {
            q[0] = g[0] * 0x00010101u | (g[1] << 24);
            q[1] = g[1] * 0x00000101u | (g[2] * 0x01010000u);
            q[2] = g[2] | (g[3] * 0x01010100u);
        } else {  // alpha = 255 (cv::cvtColor GRAY2BGRA)
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = g[i] * 0x00010101u | 0xff000000u;
        }
    } else {
        for (int i = 0; i < n; ++i) {
            d[i * CH] = d[i * CH + 1] = d[i * CH + 2] = (uint8_t)g[i];
            if (CH == 4) d[i * CH + 3] = 255;
        }
    }
}

__global__ void __launch_bounds__(256) k_invert(PageSet src, PageSetOut dst, int width, int height)
{
    const int page = blockIdx.z, y = blockIdx.y;
    const uint8_t* s = src.page(page) + (size_t)y * src.step;
    uint8_t* d = dst.page(page) + (size_t)y * dst.step;
    // align on the destination: head bytes, then 16-byte stores (source fetched as dwords / bytes when it is not
    // co-aligned), tail bytes
    const int head = min(width, (int)((16 - ((size_t)d & 15)) & 15));
    if (blockIdx.x == 0 && (int)threadIdx.x < head) d[threadIdx.x] = (uint8_t)~s[threadIdx.x];
    const int x0 = head + (blockIdx.x * 256 + threadIdx.x) * 16;
    if (x0 >= width) return;
    if (x0 + 16 <= width) {
        uint4 w;
        const size_t sa = (size_t)(s + x0);
        if ((sa & 15) == 0) {
            w = *reinterpret_cast<const uint4*>(s + x0);
        } else if ((sa & 3) == 0) {
            const unsigned* q = reinterpret_cast<const unsigned*>(s + x0);
            w = make_uint4(q[0], q[1], q[2], q[3]);
        } else {  // aligned dwords + byte funnel
            const unsigned sh = (unsigned)(sa & 3);
            const unsigned* q = reinterpret_cast<const unsigned*>(s + x0 - sh);
            const unsigned a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4];  // q[4] holds bytes x0+16-sh.. : inside the row
            w = make_uint4(__builtin_amdgcn_alignbyte(a1, a0, sh), __builtin_amdgcn_alignbyte(a2, a1, sh),
                           __builtin_amdgcn_alignbyte(a3, a2, sh), __builtin_amdgcn_alignbyte(a4, a3, sh));
        }
        *reinterpret_cast<uint4*>(d + x0) = make_uint4(~w.x, ~w.y, ~w.z, ~w.w);
    } else {
        for (int i = x0; i < width; ++i) d[i] = (uint8_t)~s[i];
    }
}

struct Args {
    PageSet ps{};
    PageSetOut pd{};
    dim3 grid;
};

int common_args(int n_pages, const uint8_t* d_src, size_t sps, size_t sstep, size_t src_row_bytes, int width, int height,
                uint8_t* d_dst, size_t dps, size_t dstep, size_t dst_row_bytes, Args* a)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (n_pages < 0 || !d_src || !d_dst || sstep < src_row_bytes || dstep < dst_row_bytes) return PRL_ERR_BAD_ARG;
    if (height > 65535) return PRL_ERR_BAD_ARG;  // grid.y limit (one grid row per image row)
    a->ps = page_set(d_src, sps, sstep);
    a->pd = page_set_out(d_dst, dps, dstep);
    a->grid = dim3((unsigned)((width + 1023) / 1024), (unsigned)height, (unsigned)n_pages);  // 4 px per thread
    return PRL_OK;
}

// One launch per 32768 pages (grid.z holds at most 65535): launch(grid, src, dst) enqueues the adapter's kernel on those pages.
template <typename Launch>
int launch_page_chunks(const Args& a, int n_pages, Launch&& launch)
{
    int dev;
    const int st = current_device(&dev);
    if (st != PRL_OK) return st;
    for (int first = 0; first < n_pages; first += 32768) {
        dim3 grid = a.grid;
        grid.z = (unsigned)std::min(32768, n_pages - first);
        launch(grid, pages_from(a.ps, first), pages_from(a.pd, first));
        PRL_HIP_CHECK(hipGetLastError());
    }
    return PRL_OK;
}

}  // namespace
}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_bgr2gray_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                  int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                  void* stream)
{
    if (channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    Args a;
    const int st = common_args(n_pages, d_src, src_page_stride, src_step, (size_t)(width > 0 ? width : 0) * channels, width, height,
                               d_dst, dst_page_stride, dst_step, (size_t)(width > 0 ? width : 0), &a);
    if (st != PRL_OK || n_pages == 0) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_page_chunks(a, n_pages, [&](dim3 grid, const PageSet& ps, const PageSetOut& pd) {
        if (channels == 3) hipLaunchKernelGGL(k_bgr2gray<3>, grid, dim3(256), 0, s, ps, pd, width, height);
        else hipLaunchKernelGGL(k_bgr2gray<4>, grid, dim3(256), 0, s, ps, pd, width, height);
    });
}

int prl_hip_gray2bgr_batch_device(int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                  int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                  void* stream)
{
    if (channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    Args a;
    const int st = common_args(n_pages, d_src, src_page_stride, src_step, (size_t)(width > 0 ? width : 0), width, height, d_dst,
                               dst_page_stride, dst_step, (size_t)(width > 0 ? width : 0) * channels, &a);
    if (st != PRL_OK || n_pages == 0) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_page_chunks(a, n_pages, [&](dim3 grid, const PageSet& ps, const PageSetOut& pd) {
        if (channels == 3) hipLaunchKernelGGL(k_gray2bgr<3>, grid, dim3(256), 0, s, ps, pd, width, height);
        else hipLaunchKernelGGL(k_gray2bgr<4>, grid, dim3(256), 0, s, ps, pd, width, height);
    });
}

int prl_hip_invert_batch_device(int n_pages, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width,
                                int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    Args a;
    const int st = common_args(n_pages, d_src, src_page_stride, src_step, (size_t)(width > 0 ? width : 0), width, height, d_dst,
                               dst_page_stride, dst_step, (size_t)(width > 0 ? width : 0), &a);
    if (st != PRL_OK || n_pages == 0) return st;
    a.grid.x = (unsigned)((width + 15 + 4095) / 4096);  // 16 px per thread after a head of up to 15
    return launch_page_chunks(a, n_pages, [&](dim3 grid, const PageSet& ps, const PageSetOut& pd) {
        hipLaunchKernelGGL(k_invert, grid, dim3(256), 0, static_cast<hipStream_t>(stream), ps, pd, width, height);
    });
}

// [deskew] -> [denoise] -> [backgroundNormalization] -> gray -> binarize -> [thinning of the inverted mask]: BASELINE
// config 5's order.  Every deskewed page has its own size, so the stages after it run per RUN of consecutive pages of
// equal size (all pages of a skewed batch come out max(W,H) square: one run).
namespace {

struct ChainLayout {   // per page of a uniform run, each part rounded up to 256 B
    size_t denoised, normalised, gray, mask, total;
    int ch_after;      // channels of the page the gray conversion sees
};

ChainLayout chain_layout(const prl_chain_params* cp, int channels, int width, int height, const prl_binarize_geometry& g)
{
    ChainLayout l{};
    const size_t px = (size_t)width * height;
    int ch = channels;
    if (cp->denoise) l.denoised = r256(px * (size_t)ch);
    if (cp->background_normalization) {
        ch = prl_hip_bgnorm_out_channels(ch);
        l.normalised = r256(px * (size_t)ch);
    }
    l.ch_after = ch;
    if (ch != 1) l.gray = r256(px);
    if (cp->thin != PRL_CHAIN_NO_THINNING) l.mask = r256((size_t)g.out_w * g.out_h);
    l.total = l.denoised + l.normalised + l.gray + l.mask;
    return l;
}

// One run of a pass: run.cnt consecutive pages of one size from page r0 of the pass on, with the geometry and the workspace layout of
// that size and its slice of the workspace (ws: cnt * l.total bytes).  `cur` is where its pages stand as the stages advance, `w` the
// free workspace behind them.
struct Run {
    int r0, cnt, pw, ph;
    prl_binarize_geometry g;
    ChainLayout l;
    uint8_t* ws;
    uint8_t* planes;   // its Lab planes (pass_split)
    PageSet cur;
    uint8_t* w;
};

// a stage has written the run's pages to `out`, at the front of its free workspace
void advance(Run* run, const PageSetOut& out)
{
    run->cur = as_source(out);
    run->w = out.base + out.page_stride * (size_t)run->cnt;
}

// The runs of a pass of `cnt` pages (wh: width and height per page), laid out in the workspace from `ws` on; out_wh receives every
// page's result size.
int split_runs(const prl_chain_params* cp, int channels, const std::vector<int32_t>& wh, int cnt, uint8_t* ws, int32_t* out_wh,
               std::vector<Run>* runs)
{
    runs->clear();
    for (int r0 = 0; r0 < cnt;) {
        int r1 = r0 + 1;
        while (r1 < cnt && wh[2 * (size_t)r1] == wh[2 * (size_t)r0] && wh[2 * (size_t)r1 + 1] == wh[2 * (size_t)r0 + 1]) ++r1;
        Run run{};
        run.r0 = r0; run.cnt = r1 - r0; run.pw = wh[2 * (size_t)r0]; run.ph = wh[2 * (size_t)r0 + 1];
        const int st = prl_hip_binarize_geometry(&cp->binarize, run.pw, run.ph, &run.g);
        if (st != PRL_OK) return st;
        run.l = chain_layout(cp, channels, run.pw, run.ph, run.g);
        run.ws = run.w = ws;
        ws += run.l.total * (size_t)run.cnt;
        for (int i = r0; i < r1; ++i) {
            out_wh[2 * (size_t)i] = run.g.out_w;
            out_wh[2 * (size_t)i + 1] = run.g.out_h;
        }
        runs->push_back(run);
        r0 = r1;
    }
    return PRL_OK;
}

// The stages after deskew on one run, in two halves: chain_uniform_a is the denoise stage (NL-means: compute) on the pages `src`,
// chain_uniform_b the streaming stages that follow, from run.cur to the result pages `dst`; pass_split runs the first half in parts
// of its own.
int chain_uniform_a(const prl_chain_params* cp, int channels, Run& run, const PageSet& src, hipStream_t hs)
{
    run.cur = src;
    if (!cp->denoise) return PRL_OK;
    const PageSetOut out = page_set_out(run.w, run.l.denoised, (size_t)run.pw * channels);
    const int st = prl_hip_denoise_batch_device(run.cnt, channels, cp->denoise_strength, src.base, src.page_stride, src.step, run.pw, run.ph,
                                                out.base, out.page_stride, out.step, hs);
    if (st != PRL_OK) return st;
    advance(&run, out);
    return PRL_OK;
}

int chain_uniform_b(const prl_chain_params* cp, int channels, Run& run, const PageSetOut& dst, hipStream_t hs)
{
    const int cnt = run.cnt, width = run.pw, height = run.ph;
    int st, ch = channels;
    if (cp->background_normalization) {
        const int och = prl_hip_bgnorm_out_channels(ch);
        const PageSetOut out = page_set_out(run.w, run.l.normalised, (size_t)width * och);
        st = prl_hip_bgnorm_batch_device(cnt, ch, run.cur.base, run.cur.page_stride, run.cur.step, width, height, out.base, out.page_stride,
                                         out.step, hs);
        if (st != PRL_OK) return st;
        ch = och;
        advance(&run, out);
    }
    if (ch != 1) {
        const PageSetOut out = page_set_out(run.w, run.l.gray, (size_t)width);
        st = prl_hip_bgr2gray_batch_device(cnt, ch, run.cur.base, run.cur.page_stride, run.cur.step, width, height, out.base, out.page_stride,
                                           out.step, hs);
        if (st != PRL_OK) return st;
        advance(&run, out);
    }
    // The binarizer's source is this chain's own scratch, which the next pass / the next call overwrites: its flag check (and
    // the literal redo of an overflow-flagged page) must happen HERE, whatever prl_hip_set_deferred_completion says - a
    // pending call resolved later would redo the page from overwritten pixels.
    const bool thin = cp->thin != PRL_CHAIN_NO_THINNING;
    const PageSetOut mask = thin ? page_set_out(run.w, run.l.mask, (size_t)run.g.out_w) : dst;
    st = prl_hip_binarize_batch_device(&cp->binarize, cnt, run.cur.base, run.cur.page_stride, run.cur.step, width, height, mask.base,
                                       mask.page_stride, mask.step, hs);
    if (st != PRL_OK) return st;
    st = prl_hip_finish(hs);  // (the mask is final before it is thinned)
    if (st != PRL_OK || !thin) return st;
    // cv::bitwise_not between the two stages happens inside the thinning's bit packing (no pass of its own)
    return thin_batch_device(cp->thin, cnt, as_source(mask), run.g.out_w, run.g.out_h, dst, hs, true);
}

size_t chain_budget()
{
    return env_knobs().chain_work_mb << 20;  // intermediates of one pass (default 48 GiB: 288 GB of HBM, big passes, few launches)
}

int chain_check(const prl_chain_params* cp, int n_pages, int channels, const uint8_t* d_src, size_t src_step, int width, int height,
                uint8_t* d_dst)
{
    if (!cp) return PRL_ERR_BAD_ARG;
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (channels != 1 && channels != 3 && channels != 4) return PRL_ERR_BAD_CHANNELS;
    if (cp->denoise && channels == 1) return PRL_ERR_BAD_CHANNELS;  // fastNlMeansDenoisingColored asserts 8UC3 / 8UC4
    if (cp->thin != PRL_CHAIN_NO_THINNING && cp->thin != PRL_THIN_ZHANGSUEN && cp->thin != PRL_THIN_GUOHALL) return PRL_ERR_BAD_ARG;
    if (n_pages < 0 || !d_src || !d_dst || src_step < (size_t)width * channels) return PRL_ERR_BAD_ARG;
    // the angle search walks (x << 16) fixed-point coordinates, packs points as x | y << 16 and the warp's coordinates
    // saturate to short: the same limit prl_hip_deskew_batch_device / rotate / houghp enforce
    if (cp->deskew && std::max(width, height) > 32767) return PRL_ERR_BAD_ARG;
    return PRL_OK;
}

}  // namespace

extern "C++" {
namespace prl_hip {
// Pages per pass of the chain on n_pages pages of one size (workspace budgets of the chain and of the angle search), and the
// workspace bytes per page.  host_batch.hip sizes its device chunks in whole passes with it.
int chain_pass_layout(const prl_chain_params* cp, int n_pages, int channels, int width, int height, int* pass_pages, size_t* per_page_out,
                      size_t* desk_page_out)
{
    const int len = std::max(width, height);
    const int dw = cp->deskew ? len : width, dh = cp->deskew ? len : height;  // largest page the later stages can see
    prl_binarize_geometry gmax;
    int st = prl_hip_binarize_geometry(&cp->binarize, dw, dh, &gmax);
    if (st != PRL_OK) return st;
    const ChainLayout lmax = chain_layout(cp, channels, dw, dh, gmax);
    const size_t desk_page = cp->deskew ? r256((size_t)len * len * channels) : 0;
    const size_t per_page = desk_page + lmax.total;
    int chunk = per_page == 0 ? n_pages : (int)std::max<size_t>(1, std::min<size_t>((size_t)n_pages, chain_budget() / per_page));
    chunk = std::min(chunk, 32768);
    if (cp->deskew) chunk = std::min(chunk, deskew_pages_per_pass(n_pages, width, height));
    *pass_pages = std::max(1, chunk);
    if (per_page_out) *per_page_out = per_page;
    if (desk_page_out) *desk_page_out = desk_page;
    return PRL_OK;
}
}  // namespace prl_hip
}  // extern "C++"

namespace {

double wall_s() { return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count(); }   // (debug lines)
double seconds_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }

// The angle search of deskew (HoughLinesP: one wavefront per page waiting on scattered atomics, seconds per pass) runs
// for pass k+1 on the side stream, from a helper thread, while the rotation and the other stages of pass k (NL-means:
// ALU / LDS work that needs no memory bandwidth) run on the caller's stream.  Both only read the source pages.
struct AngleSearch {
    DeviceCtx* ctx;
    int dev, channels;
    PageSet src;           // the pages of the whole call
    int width, height;
    double seconds = 0.0;  // how long the last search took

    AngleSearch(DeviceCtx* ctx_, int dev_, int channels_, const PageSet& src_, int width_, int height_)
        : ctx(ctx_), dev(dev_), channels(channels_), src(src_), width(width_), height(height_) {}
    AngleSearch(const AngleSearch&) = delete;
    ~AngleSearch() { join(); if (started.ev) (void)hipEventDestroy(started.ev); }

    // the side stream (created on first use) behind the caller's stream `hs`, and the event of the searches' start
    int open(hipStream_t hs)
    {
        if (!ctx->side) {
            PRL_HIP_CHECK(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
            PRL_HIP_CHECK(hipEventCreateWithFlags(&ctx->side_ev, hipEventDisableTiming));
        }
        PRL_HIP_CHECK(hipEventRecord(ctx->side_ev, hs));  // the source pages may come from earlier work on the caller's stream
        PRL_HIP_CHECK(hipStreamWaitEvent(ctx->side, ctx->side_ev, 0));
        PRL_HIP_CHECK(hipEventCreateWithFlags(&started.ev, hipEventDisableTiming));
        return PRL_OK;
    }
    // search the angles of pages first .. first + cnt - 1; prefer_mw: SearchStart::prefer_mw
    void start(int first, int cnt, bool prefer_mw)
    {
        st = PRL_OK;
        started.reset();
        started.prefer_mw = prefer_mw;
        if (env_knobs().debug)
            std::fprintf(stderr, "[prl chain] search of pages %d..%d: %s\n", first, first + cnt - 1, prefer_mw ? "k_ppht_mw (hides behind NL-means)" : "group kernel");
        th = std::thread([this, first, cnt] {
            const auto t0 = std::chrono::steady_clock::now();
            if (hipSetDevice(dev) != hipSuccess) {
                st = PRL_ERR_NO_DEVICE;
            } else {
                const auto t1 = std::chrono::steady_clock::now();
                st = deskew_find(ctx, cnt, channels, pages_from(src, first), width, height, &plan, ctx->side, &started);
                if (st != PRL_OK) detail = prl_hip_last_error_detail();
                if (env_knobs().debug) std::fprintf(stderr, "[prl chain %.3f] angle search of pages %d..: %.3f s\n", wall_s(), first, seconds_since(t1));
            }
            seconds = seconds_since(t0);
            started.finish();
        });
    }
    void join() { if (th.joinable()) th.join(); }
    // the result of the search started last: its status (with the error detail of its thread) and, moved out, its plan
    int take(DeskewPlan* out)
    {
        join();
        if (st != PRL_OK) {
            set_error_detail(detail);
            return st;
        }
        *out = std::move(plan);
        plan = DeskewPlan();
        return PRL_OK;
    }
    // Beside a search only runs what is enqueued behind this: the caller's stream waits (on the device) for the streaming prelude
    // of the search to be through, the host for its Hough kernel to be submitted - a search that starts next to other kernels is
    // slowed for good, one whose wavefronts are resident first runs at its own speed.  No wall-clock guesses.
    int wait_started(hipStream_t hs)
    {
        if (started.wait()) PRL_HIP_CHECK(hipStreamWaitEvent(hs, started.ev, 0));
        return PRL_OK;
    }

private:
    std::thread th;
    int st = PRL_OK;
    std::string detail;
    DeskewPlan plan;
    SearchStart started;   // lets the caller wait for the Hough kernel of the search to be under way
};

struct EventOwner { hipEvent_t e = nullptr; ~EventOwner() { if (e) (void)hipEventDestroy(e); } };

// What the passes of one chain call share, and the two ways to run the stages of a pass after its rotation: `runs` are its runs,
// `cur` its pages (rotated, where the chain deskews), `first` its first page in the call.
struct ChainCall {
    const prl_chain_params* cp;
    int n_pages, channels, len;
    PageSetOut dst;
    DeviceCtx* ctx;
    hipStream_t hs;
    ChainSchedule& sched;
    AngleSearch& search;
    const std::vector<unsigned>& ink;   // points per page (deskew_ink_census), where the schedule wanted a census
    EventOwner body_done;

    void start_search(int first, int cnt, int beside_cnt) { search.start(first, cnt, sched.prefers_mw(ink, first, cnt, beside_cnt, len)); }

    int pass_whole(std::vector<Run>& runs, const PageSet& cur, int first)
    {
        for (Run& run : runs) {
            int st = chain_uniform_a(cp, channels, run, pages_from(cur, run.r0), hs);
            if (st == PRL_OK) st = chain_uniform_b(cp, channels, run, pages_from(dst, first + run.r0), hs);
            if (st != PRL_OK) return st;
        }
        return PRL_OK;
    }

    // chain_overlap == 2 (with deskew and denoise): a pass is cut in three.  HEAD - rotation and BGR->Lab, streaming kernels -
    // runs before the search of the next pass is started; BODY - the NL-means kernels, compute - beside that search;
    // TAIL - Lab->BGR and the stages after denoise, streaming again - after it.  Streaming kernels get a fraction of their
    // bandwidth while a search's atomics are in flight (16-50x their time in its first second) and hold up whatever is
    // queued behind them, and a search that starts beside them is slowed for good.  *ncnt: the size of the next pass.
    int pass_split(std::vector<Run>& runs, const PageSet& cur, int first, int cnt, int* ncnt)
    {
        size_t planes_need = 0;
        for (const Run& run : runs) planes_need += denoise_plane_bytes(run.pw, run.ph) * (size_t)run.cnt;
        int st = ensure_buffer(&ctx->chain_planes, &ctx->chain_planes_bytes, planes_need);
        if (st != PRL_OK) return st;
        uint8_t* pl = static_cast<uint8_t*>(ctx->chain_planes);
        for (Run& run : runs) {   // HEAD (the rotation was enqueued before)
            run.planes = pl;
            pl += denoise_plane_bytes(run.pw, run.ph) * (size_t)run.cnt;
            st = denoise_convert_in(ctx, run.cnt, channels, pages_from(cur, run.r0), run.pw, run.ph, run.planes, hs);
            if (st != PRL_OK) return st;
        }
        const int nfirst = first + cnt;
        const bool beside = nfirst < n_pages;
        if (beside) {
            PRL_HIP_CHECK(hipStreamSynchronize(hs));   // the head is through before the next search takes the memory system
            *ncnt = sched.next_count(nfirst);
            start_search(nfirst, *ncnt, cnt);
            st = search.wait_started(hs);
            if (st != PRL_OK) return st;
        }
        for (Run& run : runs) {   // BODY
            st = denoise_nlm(ctx, run.cnt, cp->denoise_strength, run.planes, run.pw, run.ph, hs);
            if (st != PRL_OK) return st;
        }
        if (beside) {
            if (!body_done.e) PRL_HIP_CHECK(hipEventCreateWithFlags(&body_done.e, hipEventDisableTiming));
            PRL_HIP_CHECK(hipEventRecord(body_done.e, hs));
        }
        search.join();
        if (beside) {
            // how the body compared with the search beside it sizes the searches that are still to start
            const bool early = hipEventQuery(body_done.e) == hipSuccess;
            if (!early) (void)hipGetLastError();   // ("not ready" is an answer, not an error to find later)
            const auto tj = std::chrono::steady_clock::now();
            if (!early) PRL_HIP_CHECK(hipEventSynchronize(body_done.e));   // (the tail is enqueued behind the body anyway)
            const double past = early ? 0.0 : seconds_since(tj);
            const std::pair<int, int> sz = sched.observe(search.seconds, past, early, *ncnt);
            if (env_knobs().debug && sz.second != sz.first)
                std::fprintf(stderr, "[prl chain] pass size %d -> %d (search %.3f s, NL-means %.3f s past it)\n", sz.first, sz.second, search.seconds, past);
            if (env_knobs().debug)
                std::fprintf(stderr, "[prl chain] pass at page %d: NL-means ran %.3f s past the search\n", first, past);
        }
        for (Run& run : runs) {   // TAIL
            const PageSetOut out = page_set_out(run.w, run.l.denoised, (size_t)run.pw * channels);
            st = denoise_convert_out(ctx, run.cnt, channels, run.planes, run.pw, run.ph, out, hs);
            if (st != PRL_OK) return st;
            advance(&run, out);
            st = chain_uniform_b(cp, channels, run, pages_from(dst, first + run.r0), hs);
            if (st != PRL_OK) return st;
        }
        return PRL_OK;
    }
};

// the chain behind its entries' argument checks (chain_check)
int chain_run(const prl_chain_params* cp, int n_pages, int channels, const PageSet& src, int width, int height, const PageSetOut& dst,
              int32_t* out_wh, double* angles, hipStream_t hs)
{
    int max_w = 0, max_h = 0;
    int st = prl_hip_chain_max_out_size(cp, width, height, &max_w, &max_h);
    if (st != PRL_OK) return st;
    if (dst.step < (size_t)max_w) return PRL_ERR_BAD_ARG;
    if (n_pages == 0) return PRL_OK;
    int dev;
    st = current_device(&dev);
    if (st != PRL_OK) return st;
    DeviceCtx* ctx = device_ctx(dev);
    std::lock_guard<std::mutex> slk(ctx->stage_mu);  // the staging workspace holds the intermediates

    const EnvKnobs& knobs = env_knobs();
    const int len = std::max(width, height);
    size_t per_page = 0, desk_page = 0;
    int chunk = 0;
    st = chain_pass_layout(cp, n_pages, channels, width, height, &chunk, &per_page, &desk_page);
    if (st != PRL_OK) return st;
    ChainSchedule sched(n_pages, chunk, cp->deskew != 0, cp->denoise != 0, knobs.chain_overlap, knobs.chain_pass, knobs.chain_first_pass);
    std::vector<unsigned> ink;
    if (sched.wants_census()) {   // (cheap: one streaming read of the pages)
        st = deskew_ink_census(ctx, n_pages, channels, src, width, height, &ink, hs);
        if (st != PRL_OK) return st;
        const int before = sched.main_sz;
        const unsigned heaviest = sched.extend_for_tail(ink);
        if (knobs.debug && sched.main_sz != before)
            std::fprintf(stderr, "[prl chain] tail-bound batch: heaviest page %u points, passes of %d pages\n", heaviest, sched.main_sz);
    }
    if (per_page) {
        st = ensure_stage(ctx, per_page * (size_t)sched.max_cnt);
        if (st != PRL_OK) return st;
    }
    st = stage_acquire(ctx, hs);  // another stream's chain / host call may still read the area
    if (st != PRL_OK) return st;
    StageRelease release{ctx, hs};
    AngleSearch search(ctx, dev, channels, src, width, height);   // (after `release`: a search still running at an early return is joined first)
    ChainCall c{cp, n_pages, channels, len, dst, ctx, hs, sched, search, ink, {}};
    if (cp->deskew) {
        st = search.open(hs);
        if (st != PRL_OK) return st;
    }
    const bool split = cp->deskew && cp->denoise && knobs.chain_overlap == 2;   // head / body / tail: pass_split
    if (split) {
        // the Lab planes of the largest pass, up front: growing the buffer later synchronises the device under a running search
        st = ensure_buffer(&ctx->chain_planes, &ctx->chain_planes_bytes, denoise_plane_bytes(len, len) * (size_t)sched.max_cnt);
        if (st != PRL_OK) return st;
    }
    std::vector<int32_t> wh((size_t)sched.max_cnt * 2);
    std::vector<Run> runs;
    DeskewPlan plan;
    int first = 0, cnt = sched.next_count(0);
    if (cp->deskew) c.start_search(0, cnt, 0);
    while (first < n_pages) {
        const int nfirst = first + cnt;
        int ncnt = 0;   // size of the next pass: fixed when its search starts
        uint8_t* ws = static_cast<uint8_t*>(ctx->stage);
        PageSet cur = pages_from(src, first);
        const auto t_pass = std::chrono::steady_clock::now();
        if (cp->deskew) {
            st = search.take(&plan);
            if (knobs.debug)
                std::fprintf(stderr, "[prl chain %.3f] pass at page %d waited %.3f s for its angles\n", wall_s(), first, seconds_since(t_pass));
            if (st != PRL_OK) return st;
            if (knobs.chain_overlap && !split && nfirst < n_pages) {   // (pass_split starts it after the streaming head of the pass)
                ncnt = sched.next_count(nfirst);
                c.start_search(nfirst, ncnt, 0);
                st = search.wait_started(hs);   // this pass's own work starts once the search is under way
                if (st != PRL_OK) return st;
            }
            const PageSetOut desk = page_set_out(ws, desk_page, (size_t)len * channels);
            ws += desk_page * (size_t)cnt;
            st = deskew_apply(ctx, plan, cnt, channels, cur, width, height, desk, hs);
            if (st != PRL_OK) return st;
            std::copy(plan.wh.begin(), plan.wh.end(), wh.begin());
            if (angles) std::copy(plan.angles.begin(), plan.angles.end(), angles + first);
            cur = as_source(desk);
        } else {
            for (int i = 0; i < cnt; ++i) { wh[2 * (size_t)i] = width; wh[2 * (size_t)i + 1] = height; }
            if (angles) for (int i = 0; i < cnt; ++i) angles[first + i] = 0.0;
        }
        st = split_runs(cp, channels, wh, cnt, ws, out_wh + 2 * (size_t)first, &runs);
        if (st == PRL_OK) st = split ? c.pass_split(runs, cur, first, cnt, &ncnt) : c.pass_whole(runs, cur, first);
        if (st != PRL_OK) return st;
        if (cp->deskew && !knobs.chain_overlap && nfirst < n_pages) {
            PRL_HIP_CHECK(hipStreamSynchronize(hs));
            ncnt = sched.next_count(nfirst);
            c.start_search(nfirst, ncnt, 0);
            search.join();
        }
        if (knobs.debug) {
            (void)hipStreamSynchronize(hs);
            std::fprintf(stderr, "[prl chain %.3f] pass at page %d (%d pages) done after %.3f s\n", wall_s(), first, cnt, seconds_since(t_pass));
        }
        first = nfirst;
        cnt = ncnt > 0 ? ncnt : (first < n_pages ? sched.next_count(first) : 0);
    }
    return PRL_OK;
}

}  // namespace

// The chain on pages whose results may differ in size (deskew): out_wh (host, 2 ints per page) receives each page's
// result size; d_dst pages need room for the largest possible result (prl_hip_chain_max_out_size) at dst_step bytes per row.
int prl_hip_chain_pages_device(const prl_chain_params* cp, int n_pages, int channels, const uint8_t* d_src, size_t src_page_stride,
                               size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                               int32_t* out_wh, double* angles, void* stream)
{
    const int st = chain_check(cp, n_pages, channels, d_src, src_step, width, height, d_dst);
    if (st != PRL_OK) return st;
    if (!out_wh) return PRL_ERR_BAD_ARG;
    return chain_run(cp, n_pages, channels, page_set(d_src, src_page_stride, src_step), width, height,
                     page_set_out(d_dst, dst_page_stride, dst_step), out_wh, angles, static_cast<hipStream_t>(stream));
}

int prl_hip_chain_max_out_size(const prl_chain_params* cp, int width, int height, int* out_w, int* out_h)
{
    if (!cp || !out_w || !out_h) return PRL_ERR_BAD_ARG;
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    const int len = std::max(width, height);
    prl_binarize_geometry g;
    int st = prl_hip_binarize_geometry(&cp->binarize, cp->deskew ? len : width, cp->deskew ? len : height, &g);
    if (st != PRL_OK) return st;
    *out_w = g.out_w;
    *out_h = g.out_h;
    if (cp->deskew) {  // pages without an angle keep width x height: their result can be larger in one dimension only if ... never
        prl_binarize_geometry g2;
        st = prl_hip_binarize_geometry(&cp->binarize, width, height, &g2);
        if (st != PRL_OK) return st;  // (a page that keeps its size must be binarizable too)
        *out_w = std::max(*out_w, g2.out_w);
        *out_h = std::max(*out_h, g2.out_h);
    }
    return PRL_OK;
}

// Uniform result size: the chain without deskew.  d_dst receives out_w x out_h bytes per page (prl_hip_binarize_geometry).
int prl_hip_chain_batch_device(const prl_chain_params* cp, int n_pages, int channels, const uint8_t* d_src,
                               size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                               size_t dst_page_stride, size_t dst_step, void* stream)
{
    if (cp && cp->deskew) return PRL_ERR_BAD_ARG;  // per-page result sizes: prl_hip_chain_pages_device
    int st = chain_check(cp, n_pages, channels, d_src, src_step, width, height, d_dst);
    if (st != PRL_OK) return st;
    std::vector<int32_t> wh((size_t)std::max(n_pages, 1) * 2);
    return chain_run(cp, n_pages, channels, page_set(d_src, src_page_stride, src_step), width, height,
                     page_set_out(d_dst, dst_page_stride, dst_step), wh.data(), nullptr, static_cast<hipStream_t>(stream));
}

void prl_hip_default_chain_params(prl_chain_params* out)
{
    if (!out) return;
    out->denoise = 0;
    out->denoise_strength = 5.5f;  // src/denoise/denoiseNLM.h:32
    prl_hip_default_params(PRL_SAUVOLA, &out->binarize);
    out->thin = PRL_CHAIN_NO_THINNING;
    out->deskew = 0;
    out->background_normalization = 0;
}

}  // extern "C"
