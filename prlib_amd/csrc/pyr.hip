// pyr.hip — cv::pyrDown on batched 8-bit pages (src/resize.cpp:53, src/border_detection/autoCrop.cpp:76) and the two paths of
// prl::resize (src/resize.cpp:29-62).  The arithmetic is stated in include/prl_hip.h ("pyramid, edge map, resize") and restated
// in tests/edges_ref.py; all of it is integer.
//
//   k_pyr_down<CH>   one pyramid level.  A workgroup owns kPyrTW output columns and walks down kPyrRows output rows.  Per output
//                    row it stages the two new source rows - the 2 kPyrTW + 3 source pixels its columns read of each - in LDS
//                    (addresses reflected, BORDER_REFLECT_101; dword loads inside the row; two buffers: one barrier per pair),
//                    every lane forms the 1 4 6 4 1 row sum of its column once per source row and keeps the last five of them in
//                    registers; the output row leaves as (v + 128) >> 8.  Source rows inside a run are read once; the rows
//                    above and below it are the run's halo (5 of 64 + 5).
//   k_replicate<CH>  cv::resize(INTER_AREA) by integer factors >= 1: a gather through the host's index tables.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "prl_internal.h"

namespace prl_hip {

// cv::borderInterpolate(p, len, BORDER_REFLECT_101)
__host__ __device__ inline int reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do p = p < 0 ? -p : 2 * len - 2 - p;
    while ((unsigned)p >= (unsigned)len);
    return p;
}

namespace {

constexpr int kPyrTW = 256;    // output columns per workgroup
constexpr int kPyrRows = 32;   // output rows per run
constexpr int kPyrMaxLevels = 16;   // a side of 32768 is 1 after 15 levels

template <int CH>
__global__ void __launch_bounds__(kPyrTW) k_pyr_down(PageSet src, PageSetOut dst, int W, int H, int OW, int OH)
{
    constexpr int SW = 2 * kPyrTW + 3;   // source columns 2 x0 - 2 .. 2 (x0 + kPyrTW - 1) + 2
    constexpr int SB = (SW * CH + 3) / 4 * 4;   // bytes of a staged row, whole dwords
    __shared__ __attribute__((aligned(4))) uint8_t srow[2][2][SB];   // [buffer][row of the pair]
    const int t = threadIdx.x, x0 = blockIdx.x * kPyrTW, x = x0 + t, page = blockIdx.z;
    const uint8_t* sp = src.page(page);
    uint8_t* dp = dst.page(page);
    const int y0 = blockIdx.y * kPyrRows, y1 = min(y0 + kPyrRows, OH);
    const int nstage = min(SW, 2 * (OW - x0) + 3) * CH;   // the bytes the block's live lanes read
    const int ndw = (nstage + 3) / 4;
    const bool live = x < OW;
    int r0[CH], r1[CH], r2[CH], r3[CH], r4[CH];   // row sums of the last five logical source rows
#pragma unroll
    for (int c = 0; c < CH; ++c) r0[c] = r1[c] = r2[c] = r3[c] = r4[c] = 0;
    // Two source rows a barrier: pair p holds the logical rows 2 y0 - 3 + 2 p and 2 y0 - 2 + 2 p.  The first row of pair 0 lies
    // above the window of output row y0 and has left the ring when that row is formed (pair 2); output row y0 + p - 2 leaves
    // after pair p.
    const int npairs = (y1 - y0) + 2;
    for (int p = 0; p < npairs; ++p) {
        // four staged bytes a lane and round: one dword load (at any alignment: global memory takes it on gfx9+) where all four
        // lie inside the row as they are, reflected byte loads at the page's edges
        for (int i = t; i < 2 * ndw; i += kPyrTW) {
            const int half = i >= ndw ? 1 : 0, b = 4 * (i - half * ndw);
            const uint8_t* prow = sp + (size_t)reflect101(2 * y0 - 3 + 2 * p + half, H) * src.step;
            uint8_t* sb = srow[p & 1][half];
            const long long g = (long long)(2 * x0 - 2) * CH + b;   // the first byte's place in the row, were nothing reflected
            if (g >= 0 && g + 4 <= (long long)W * CH && b + 4 <= nstage) {
                uint32_t v;
                __builtin_memcpy(&v, prow + g, 4);
                *reinterpret_cast<uint32_t*>(sb + b) = v;
            } else {
                for (int k = b; k < min(b + 4, nstage); ++k) {
                    const int col = k / CH, c = k - col * CH;
                    sb[k] = prow[(size_t)reflect101(2 * x0 - 2 + col, W) * CH + c];
                }
            }
        }
        __syncthreads();
        if (live) {
            const uint8_t* qa = srow[p & 1][0] + 2 * t * CH;
            const uint8_t* qb = srow[p & 1][1] + 2 * t * CH;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                r0[c] = r2[c]; r1[c] = r3[c]; r2[c] = r4[c];
                r3[c] = (int)qa[c] + 4 * (int)qa[CH + c] + 6 * (int)qa[2 * CH + c] + 4 * (int)qa[3 * CH + c] + (int)qa[4 * CH + c];
                r4[c] = (int)qb[c] + 4 * (int)qb[CH + c] + 6 * (int)qb[2 * CH + c] + 4 * (int)qb[3 * CH + c] + (int)qb[4 * CH + c];
            }
            if (p >= 2) {
                const int y = y0 + p - 2;
                uint8_t* d = dp + (size_t)y * dst.step + (size_t)x * CH;
#pragma unroll
                for (int c = 0; c < CH; ++c) d[c] = (uint8_t)((r0[c] + 4 * r1[c] + 6 * r2[c] + 4 * r3[c] + r4[c] + 128) >> 8);
            }
        }
    }
}

template <int CH>
__global__ void __launch_bounds__(256) k_replicate(PageSet src, PageSetOut dst, int OW, int OH, const int* __restrict__ tx,
                                                   const int* __restrict__ ty)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, page = blockIdx.z;
    if (x >= OW || y >= OH) return;
    const uint8_t* s = src.page(page) + (size_t)ty[y] * src.step + (size_t)tx[x] * CH;
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + (size_t)x * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) d[c] = s[c];
}

int bad_arg(const char* why)
{
    set_error_detail(why);
    return PRL_ERR_BAD_ARG;
}

int pyr_level(int channels, const PageSet& s, const PageSetOut& d, int W, int H, int n, hipStream_t stream)
{
    const int OW = (W + 1) / 2, OH = (H + 1) / 2;
    const dim3 grid((unsigned)((OW + kPyrTW - 1) / kPyrTW), (unsigned)((OH + kPyrRows - 1) / kPyrRows), (unsigned)n);
    switch (channels) {
    case 1: hipLaunchKernelGGL(k_pyr_down<1>, grid, dim3(kPyrTW), 0, stream, s, d, W, H, OW, OH); break;
    case 2: hipLaunchKernelGGL(k_pyr_down<2>, grid, dim3(kPyrTW), 0, stream, s, d, W, H, OW, OH); break;
    case 3: hipLaunchKernelGGL(k_pyr_down<3>, grid, dim3(kPyrTW), 0, stream, s, d, W, H, OW, OH); break;
    default: hipLaunchKernelGGL(k_pyr_down<4>, grid, dim3(kPyrTW), 0, stream, s, d, W, H, OW, OH); break;
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

size_t level_bytes(int W, int H, int channels, int level)
{
    for (int i = 0; i < level; ++i) { W = (W + 1) / 2; H = (H + 1) / 2; }
    return r256((size_t)W * channels * (size_t)H);
}

}  // namespace

// The intermediates of a pyramid of `levels` levels, per page: level 1 (and 3, 5 ...) in one block, level 2 (4, 6 ...) in another.
size_t pyr_work_per_page(int W, int H, int channels, int levels)
{
    return (levels >= 2 ? level_bytes(W, H, channels, 1) : 0) + (levels >= 3 ? level_bytes(W, H, channels, 2) : 0);
}

// `levels` >= 1 levels of n pages; `work`: n * pyr_work_per_page bytes.  Enqueues only; the caller holds the workspace.
int pyr_run(int channels, const PageSet& s, int W, int H, int levels, const PageSetOut& d, int n, uint8_t* work, hipStream_t stream)
{
    const size_t a_bytes = levels >= 2 ? level_bytes(W, H, channels, 1) : 0, b_bytes = levels >= 3 ? level_bytes(W, H, channels, 2) : 0;
    uint8_t* A = work;
    uint8_t* B = work + a_bytes * (size_t)n;
    PageSet cur = s;
    for (int k = 1; k <= levels; ++k) {
        const int OW = (W + 1) / 2;
        const PageSetOut out = k == levels ? d : (k & 1) ? page_set_out(A, a_bytes, (size_t)OW * channels) : page_set_out(B, b_bytes, (size_t)OW * channels);
        const int st = pyr_level(channels, cur, out, W, H, n, stream);
        if (st != PRL_OK) return st;
        cur = as_source(out);
        W = OW;
        H = (H + 1) / 2;
    }
    return PRL_OK;
}

void pyr_size(int W, int H, int levels, int* ow, int* oh)
{
    for (int i = 0; i < levels; ++i) { W = (W + 1) / 2; H = (H + 1) / 2; }
    *ow = W;
    *oh = H;
}

// A destination of another size than the source: its rows, and no byte shared with the source (never in place).
int resized_dst_ok(const PageArgs& a, int channels, int ow, int oh, bool batch)
{
    if (!a.dst || a.dst_step < (size_t)ow * channels) return PRL_ERR_BAD_ARG;
    if (!batch || a.n_pages <= 0) return PRL_OK;
    const size_t src_span = pages_span(a.n_pages, a.src_page_stride, a.height, a.src_step, (size_t)a.width * channels);
    const size_t dst_span = pages_span(a.n_pages, a.dst_page_stride, oh, a.dst_step, (size_t)ow * channels);
    return ranges_overlap(a.src, src_span, a.dst, dst_span) ? PRL_ERR_BAD_ARG : PRL_OK;
}

namespace {

int pyr_checks(const PageArgs& a, int channels, int levels, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, 0, batch)) != PRL_OK) return st;
    if (levels < 1 || levels > kPyrMaxLevels) return bad_arg("pyrDown: levels outside 1..16");
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    int ow, oh;
    pyr_size(a.width, a.height, levels, &ow, &oh);
    return resized_dst_ok(a, channels, ow, oh, batch);
}

int pyr_batch(const PageArgs& a, int channels, int levels, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const size_t per_page = pyr_work_per_page(a.width, a.height, channels, levels);
    const int chunk = stage_chunk(a.n_pages, per_page);
    WorkScope w;
    int st = w.open(stream, per_page * (size_t)chunk, 0, 0);
    if (st != PRL_OK) return st;
    for (int first = 0; first < a.n_pages; first += chunk) {
        st = pyr_run(channels, src_pages(a, first), a.width, a.height, levels, dst_pages(a, first), std::min(chunk, a.n_pages - first),
                     w.scratch(), w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

// sx(dx) = min(cvFloor(dx * (1.0 / scale)), len - 1): the float64 product cv::resize forms, not dx / scale
void replicate_table(int len, int scale, int* tab)
{
    const double inv = 1.0 / (double)scale;
    for (int d = 0; d < len * scale; ++d) tab[d] = std::min((int)std::floor((double)d * inv), len - 1);
}

int replicate_checks(const PageArgs& a, int channels, int scale_x, int scale_y, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, 0, batch)) != PRL_OK) return st;
    if (scale_x < 1 || scale_y < 1) return bad_arg("resize: a factor below 1");
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    if ((long long)a.width * scale_x > kStageMaxSide || (long long)a.height * scale_y > kStageMaxSide)
        return bad_arg("resize: a result side above 32768");
    return resized_dst_ok(a, channels, a.width * scale_x, a.height * scale_y, batch);
}

int replicate_batch(const PageArgs& a, int channels, int scale_x, int scale_y, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const int OW = a.width * scale_x, OH = a.height * scale_y;
    const size_t bytes = sizeof(int) * ((size_t)OW + OH);
    WorkScope w;
    int st = w.open(stream, 0, bytes, bytes);
    if (st != PRL_OK) return st;
    DeviceCtx* ctx = w.ctx;
    const hipStream_t hs = w.stream;
    // the tables go up through the pinned block as warp.hip's page records do
    if (ctx->pinned_use) PRL_HIP_CHECK(hipEventSynchronize(ctx->pinned_use));
    else PRL_HIP_CHECK(hipEventCreateWithFlags(&ctx->pinned_use, hipEventDisableTiming));
    int* h_tab = w.pinned<int>();
    replicate_table(a.width, scale_x, h_tab);
    replicate_table(a.height, scale_y, h_tab + OW);
    PRL_HIP_CHECK(hipMemcpyAsync(ctx->small, h_tab, bytes, hipMemcpyHostToDevice, hs));
    PRL_HIP_CHECK(hipEventRecord(ctx->pinned_use, hs));
    const int* tx = w.small<const int>();
    const int* ty = tx + OW;
    const int chunk = stage_chunk(a.n_pages, 0);
    for (int first = 0; first < a.n_pages; first += chunk) {
        const dim3 grid((unsigned)((OW + 255) / 256), (unsigned)OH, (unsigned)std::min(chunk, a.n_pages - first));
        const PageSet s = src_pages(a, first);
        const PageSetOut d = dst_pages(a, first);
        switch (channels) {
        case 1: hipLaunchKernelGGL(k_replicate<1>, grid, dim3(256), 0, hs, s, d, OW, OH, tx, ty); break;
        case 2: hipLaunchKernelGGL(k_replicate<2>, grid, dim3(256), 0, hs, s, d, OW, OH, tx, ty); break;
        case 3: hipLaunchKernelGGL(k_replicate<3>, grid, dim3(256), 0, hs, s, d, OW, OH, tx, ty); break;
        default: hipLaunchKernelGGL(k_replicate<4>, grid, dim3(256), 0, hs, s, d, OW, OH, tx, ty); break;
        }
        PRL_HIP_CHECK(hipGetLastError());
    }
    return PRL_OK;
}

}  // namespace
}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_pyr_down_size(int width, int height, int levels, int* out_w, int* out_h)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!out_w || !out_h || levels < 1 || levels > kPyrMaxLevels) return PRL_ERR_BAD_ARG;
    pyr_size(width, height, levels, out_w, out_h);
    return PRL_OK;
}

int prl_hip_pyr_down_batch_device(int n_pages, int channels, int levels, const uint8_t* d_src, size_t src_page_stride, size_t src_step,
                                  int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    const int st = pyr_checks(a, channels, levels, true);
    if (st != PRL_OK) return st;
    return pyr_batch(a, channels, levels, stream);
}

int prl_hip_pyr_down_host(int channels, int levels, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                          size_t dst_step)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = pyr_checks(a, channels, levels, false);
    if (st != PRL_OK) return st;
    int ow, oh;
    pyr_size(width, height, levels, &ow, &oh);
    return stage_host_pages(a, channels, channels, ow, oh, [&](const PageArgs& page, hipStream_t s) { return pyr_batch(page, channels, levels, s); });
}

int prl_hip_resize_pyramid_levels(int width, int height, int max_size, int* levels, int* out_w, int* out_h)
{
    if (width <= 0 || height <= 0) return PRL_ERR_EMPTY;
    if (!levels || !out_w || !out_h) return PRL_ERR_BAD_ARG;
    if (max_size < 1) return bad_arg("resize: maxSize < 1 never ends in the reference");
    int n = 0;
    while (std::max(width, height) > max_size) {
        width = (width + 1) / 2;
        height = (height + 1) / 2;
        ++n;
    }
    *levels = n;
    *out_w = width;
    *out_h = height;
    return PRL_OK;
}

int prl_hip_resize_replicate_batch_device(int n_pages, int channels, int scale_x, int scale_y, const uint8_t* d_src, size_t src_page_stride,
                                          size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                          void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    const int st = replicate_checks(a, channels, scale_x, scale_y, true);
    if (st != PRL_OK) return st;
    return replicate_batch(a, channels, scale_x, scale_y, stream);
}

int prl_hip_resize_replicate_host(int channels, int scale_x, int scale_y, const uint8_t* src, size_t src_step, int width, int height,
                                  uint8_t* dst, size_t dst_step)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = replicate_checks(a, channels, scale_x, scale_y, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(a, channels, channels, width * scale_x, height * scale_y,
                            [&](const PageArgs& page, hipStream_t s) { return replicate_batch(page, channels, scale_x, scale_y, s); });
}

}  // extern "C"
