// canny.hip — cv::Canny (8UC1, apertureSize 3, L1 magnitude) on batched pages.  The arithmetic is stated in include/prl_hip.h
// ("pyramid, edge map, resize") and restated in tests/edges_ref.py; all of it is integer.  What the border detectors (border.hip)
// need of it is declared in prl_internal.h; they are the only callers of the colour instantiations (CH = 3, 4) of the classes
// kernel: the public cv::Canny entries keep refusing colour pages.
//
//   k_canny_classes<BITS, CH>  Sobel, |dx| + |dy|, non-maximum suppression and the two thresholds.  A workgroup owns kCnTW columns and
//                          walks down kCnRows rows: per source row it stages the clamped pixels (BORDER_REPLICATE) in an LDS ring of
//                          three rows, forms the magnitudes of the row above for its columns and one halo column each side (zero
//                          outside the page) in a second ring of three rows, and decides the row above that.  BITS: a wavefront's
//                          two ballots go out as one word of the strong and one of the candidate plane (as k_adaptive does);
//                          else OpenCV's map codes leave as bytes.
//   k_edge_link            hysteresis as a fixpoint on the two planes: a workgroup holds a tile of kLkRows rows x kLkWords words of
//                          the strong plane plus a one-row / one-word halo in LDS and repeats S |= P & dilate8(S), filled along the
//                          runs of P within a word in log steps, until the tile stands still.  Passes over all tiles repeat until
//                          no page changed, with thin.hip's bookkeeping: per-page changed / done words, a tile is skipped while its
//                          3 x 3 tiles stood still in the previous pass, the host reads the done words back every few passes.  The
//                          plane is updated in place: it only ever gains bits, every bit it gains belongs to the answer, and the
//                          pass that ends the loop wrote nothing, so every tile then stands still against final neighbours.
//   k_plane_expand         the strong plane as 0 / 255 bytes.
#include <algorithm>
#include <cmath>

#include "prl_internal.h"

namespace prl_hip {

namespace {

typedef unsigned long long u64;

constexpr int kCnTW = 256;     // columns per workgroup of k_canny_classes: four plane words
constexpr int kCnRows = 64;    // rows per run
constexpr int kLkRows = 64;    // tile of k_edge_link: rows ...
constexpr int kLkWords = 4;    // ... x 64-column words; one lane per word

struct CannyCfg {
    int W, H, low, high;
    // per-page thresholds (CannyEdgeDetection, edgedet.hip): page i takes the pair lut[2 t], lut[2 t + 1] of its t = page_t[i], both
    // in device memory; null: low / high above for every page
    const int* lut = nullptr;
    const int* page_t = nullptr;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// grid = (ceil(W / kCnTW), ceil(H / kCnRows), pages)
template <bool BITS, int CH>
__global__ __launch_bounds__(kCnTW) void k_canny_classes(CannyCfg c, PageSet src, PageSetOut dst, u64* __restrict__ strong,
                                                         u64* __restrict__ cand, size_t plane_words, int wpr)
{
    __shared__ uint8_t px[3][(kCnTW + 4) * CH];   // pixel row j in slot (j + 3) % 3: columns x0 - 2 .. x0 + kCnTW + 1, clamped
    __shared__ unsigned short mg[3][kCnTW + 2];   // magnitudes of row r in slot (r + 3) % 3: columns x0 - 1 .. x0 + kCnTW
    const int t = threadIdx.x, x0 = blockIdx.x * kCnTW, x = x0 + t, page = blockIdx.z;
    const uint8_t* sp = src.page(page);
    const int y0 = blockIdx.y * kCnRows, y1 = min(y0 + kCnRows, c.H);
    int low = c.low, high = c.high;
    if (c.page_t) {   // uniform: scalar loads
        const int tv = c.page_t[page];
        low = c.lut[2 * tv];
        high = c.lut[2 * tv + 1];
    }
    int dx_prev = 0, dy_prev = 0, dx_cur = 0, dy_cur = 0;   // this lane's column: rows j - 2 and j - 1
    for (int j = y0 - 2; j <= y1 + 1; ++j) {
        {
            const uint8_t* prow = sp + (size_t)clampi(j, 0, c.H - 1) * src.step;
            uint8_t* pj = px[(j + 3) % 3];
            for (int i = t; i < (kCnTW + 4) * CH; i += kCnTW) pj[i] = prow[clampi(x0 - 2 + i / CH, 0, c.W - 1) * CH + i % CH];
        }
        __syncthreads();
        dx_prev = dx_cur;
        dy_prev = dy_cur;
        if (j >= y0) {   // pixel rows j - 2, j - 1, j are staged: the gradient of row r = j - 1
            const int r = j - 1;
            const uint8_t* pa = px[(r + 2) % 3];
            const uint8_t* pb = px[(r + 3) % 3];
            const uint8_t* pc = px[(r + 4) % 3];
            unsigned short* mr = mg[(r + 3) % 3];
            const bool row_in = r >= 0 && r < c.H;
            // magnitude column i is page column x0 - 1 + i and pixel column i + 1 of the ring.  Colour pages (CH > 1, the edge map
            // of prl::findHoughLineContour alone): the gradient of the channel of largest magnitude, the first of equals
            auto grad = [&](int i, int* gx, int* gy) {
                int best = -1;
#pragma unroll
                for (int ch = 0; ch < CH; ++ch) {
                    const int l = i * CH + ch, m = l + CH, r2 = l + 2 * CH;
                    const int dx = ((int)pa[r2] + 2 * (int)pb[r2] + (int)pc[r2]) - ((int)pa[l] + 2 * (int)pb[l] + (int)pc[l]);
                    const int dy = ((int)pc[l] + 2 * (int)pc[m] + (int)pc[r2]) - ((int)pa[l] + 2 * (int)pa[m] + (int)pa[r2]);
                    const int mag = abs(dx) + abs(dy);
                    if (mag > best) {
                        best = mag;
                        *gx = dx;
                        *gy = dy;
                    }
                }
                const int xc = x0 - 1 + i;
                mr[i] = (unsigned short)((row_in && xc >= 0 && xc < c.W) ? best : 0);
            };
            grad(t + 1, &dx_cur, &dy_cur);
            if (t < 2) {
                int gx, gy;
                grad(t ? kCnTW + 1 : 0, &gx, &gy);
            }
        }
        __syncthreads();
        if (j >= y0 + 2) {   // magnitudes of rows j - 3, j - 2, j - 1 are there: row y = j - 2 is decided
            const int y = j - 2;
            int cls = 1;
            if (x < c.W) {
                const unsigned short* mu = mg[(y + 2) % 3] + t + 1;
                const unsigned short* mc = mg[(y + 3) % 3] + t + 1;
                const unsigned short* md = mg[(y + 4) % 3] + t + 1;
                const int m = mc[0], dx = dx_prev, dy = dy_prev;
                if (m > low) {
                    const int ax = abs(dx), ay = abs(dy) << 15, tg = ax * 13573;
                    bool is_max;
                    if (ay < tg) is_max = m > (int)mc[-1] && m >= (int)mc[1];
                    else if (ay > tg + (ax << 16)) is_max = m > (int)mu[0] && m >= (int)md[0];
                    else {
                        const int s = (dx ^ dy) < 0 ? -1 : 1;
                        is_max = m > (int)mu[-s] && m > (int)md[s];
                    }
                    if (is_max) cls = m > high ? 2 : 0;
                }
                if (!BITS) dst.page(page)[(size_t)y * dst.step + x] = (uint8_t)cls;
            }
            if (BITS) {
                const u64 ms = __ballot(cls == 2), mc0 = __ballot(cls == 0);
                if ((t & 63) == 0 && x < c.W) {
                    const size_t w = (size_t)page * plane_words + (size_t)y * wpr + (size_t)(x >> 6);
                    strong[w] = ms;
                    cand[w] = mc0;
                }
            }
        }
    }
}

// a byte class map (2 = edge, 0 = candidate, anything else = nothing) as the two planes; grid = (ceil(W / 256), H, pages)
__global__ __launch_bounds__(256) void k_classes_pack(PageSet src, int W, u64* __restrict__ strong, u64* __restrict__ cand,
                                                      size_t plane_words, int wpr)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, page = blockIdx.z;
    const int v = x < W ? (int)src.page(page)[(size_t)y * src.step + x] : 1;
    const u64 ms = __ballot(v == 2), mc = __ballot(v == 0);
    if ((threadIdx.x & 63) == 0 && x < W) {
        const size_t w = (size_t)page * plane_words + (size_t)y * wpr + (size_t)(x >> 6);
        strong[w] = ms;
        cand[w] = mc;
    }
}

// g spread along the runs of p towards higher (UP) or lower bits, in log steps
template <bool UP>
__device__ __forceinline__ u64 run_fill(u64 g, u64 p)
{
#pragma unroll
    for (int s = 1; s < 64; s *= 2) {
        g |= p & (UP ? g << s : g >> s);
        p &= UP ? p << s : p >> s;
    }
    return g;
}

// one pass: grid = pages * tiles_y * tiles_x workgroups of kLkRows * kLkWords lanes
__global__ __launch_bounds__(kLkRows* kLkWords) void k_edge_link(u64* S, const u64* __restrict__ Cn, size_t plane_words, int wpr,
                                                                int H, int tiles_x, int tiles_y, unsigned* __restrict__ changed,
                                                                const unsigned* __restrict__ done,
                                                                const unsigned char* __restrict__ act_prev,
                                                                unsigned char* __restrict__ act_cur)
{
    __shared__ u64 s[kLkRows + 2][kLkWords + 2];
    const int t = threadIdx.x, per_page = tiles_x * tiles_y;
    const int page = (int)(blockIdx.x / (unsigned)per_page), rem = (int)(blockIdx.x - (unsigned)page * (unsigned)per_page);
    if (done[page]) return;   // finished: its plane is final
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    {   // a tile whose 3 x 3 tiles stood still in the previous pass sees what it saw then
        bool active = false;
        for (int a = -1; a <= 1; ++a)
            for (int b = -1; b <= 1; ++b) {
                const int y2 = ty + a, x2 = tx + b;
                if (y2 >= 0 && y2 < tiles_y && x2 >= 0 && x2 < tiles_x)
                    active |= act_prev[(size_t)page * per_page + (size_t)y2 * tiles_x + x2] != 0;
            }
        if (!active) {
            if (t == 0) act_cur[blockIdx.x] = 0;
            return;
        }
    }
    u64* Sp = S + (size_t)page * plane_words;
    const int lr = t / kLkWords, lk = t - lr * kLkWords;
    const int r = ty * kLkRows + lr, k = tx * kLkWords + lk;
    const bool in = r < H && k < wpr;
    for (int i = t; i < (kLkRows + 2) * (kLkWords + 2); i += kLkRows * kLkWords) {
        const int a = i / (kLkWords + 2), b = i - a * (kLkWords + 2);
        const int rr = ty * kLkRows - 1 + a, kk = tx * kLkWords - 1 + b;
        s[a][b] = (rr >= 0 && rr < H && kk >= 0 && kk < wpr) ? Sp[(size_t)rr * wpr + kk] : 0ull;
    }
    u64 P = in ? Cn[(size_t)page * plane_words + (size_t)r * wpr + k] : 0ull;
    __syncthreads();
    u64 cur = s[lr + 1][lk + 1];
    const u64 first = cur;
    P |= cur;
    for (;;) {
        u64 d = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const u64 l = s[lr + a][lk], m = s[lr + a][lk + 1], h = s[lr + a][lk + 2];
            d |= m | (m << 1) | (l >> 63) | (m >> 1) | (h << 63);
        }
        u64 g = cur | (P & d);
        g = run_fill<true>(g, P) | run_fill<false>(g, P);
        const int moved = g != cur;
        __syncthreads();   // every lane has read the words of this round
        s[lr + 1][lk + 1] = g;
        cur = g;
        if (!__syncthreads_or(moved)) break;
    }
    const int grew = cur != first;
    if (grew) Sp[(size_t)r * wpr + k] = cur;   // (P is zero outside the page, so such a lane never grows)
    const int tile_grew = __syncthreads_or(grew);
    if (t == 0) {
        act_cur[blockIdx.x] = tile_grew ? 1 : 0;
        if (tile_grew) changed[page] = 1u;
    }
}

// after a pass: a page the pass left as it was is final; `passes` counts the passes a page took part in
__global__ void k_link_endpass(unsigned* changed, unsigned* done, unsigned* passes, int n_pages)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pages) {
        if (!done[i]) {
            passes[i] += 1;
            if (changed[i] == 0) done[i] = 1;
        }
        changed[i] = 0;
    }
}

// a lane expands one byte of the plane: 8 pixels
__global__ __launch_bounds__(256) void k_plane_expand(const uint8_t* __restrict__ bits, size_t plane_bytes, size_t plane_step, PageSetOut dst,
                                                      int W)
{
    const int page = blockIdx.z, y = blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x, x = b * 8;
    if (x >= W) return;
    const uint32_t m = bits[(size_t)page * plane_bytes + (size_t)y * plane_step + b];
    uint8_t* d = dst.page(page) + (size_t)y * dst.step + x;
    const int n = min(8, W - x);
    if (n == 8 && ((size_t)d & 7) == 0) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo |= (((m >> i) & 1u) ? 255u : 0u) << (8 * i);
            hi |= (((m >> (4 + i)) & 1u) ? 255u : 0u) << (8 * i);
        }
        *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi);
    } else {
        for (int i = 0; i < n; ++i) d[i] = (uint8_t)(((m >> i) & 1u) ? 255u : 0u);
    }
}

int bad_arg(const char* why)
{
    set_error_detail(why);
    return PRL_ERR_BAD_ARG;
}

// ---- the workspace of n pages of W x H: [strong planes | candidate planes | changed | done | passes | activity 0 | activity 1] ----

struct LinkGeom {
    int W, H, wpr, tiles_x, tiles_y;
    size_t plane_words, plane_bytes;
};

LinkGeom link_geom(int W, int H)
{
    LinkGeom g;
    g.W = W;
    g.H = H;
    g.wpr = (W + 63) / 64;
    g.tiles_x = (g.wpr + kLkWords - 1) / kLkWords;
    g.tiles_y = (H + kLkRows - 1) / kLkRows;
    g.plane_words = r256((size_t)g.wpr * 8 * (size_t)H) / 8;
    g.plane_bytes = g.plane_words * 8;
    return g;
}

struct LinkWork {
    u64 *S, *C;
    unsigned *changed, *done, *passes;
    unsigned char *act0, *act1;
    size_t flags_bytes, act_bytes;
};

LinkWork link_work(const LinkGeom& g, int n, uint8_t* work)
{
    LinkWork w;
    w.flags_bytes = r256(sizeof(unsigned) * (size_t)n);
    w.act_bytes = r256((size_t)n * g.tiles_x * g.tiles_y);
    w.S = reinterpret_cast<u64*>(work);
    w.C = w.S + g.plane_words * (size_t)n;
    uint8_t* p = reinterpret_cast<uint8_t*>(w.C + g.plane_words * (size_t)n);
    w.changed = reinterpret_cast<unsigned*>(p);
    w.done = reinterpret_cast<unsigned*>(p + w.flags_bytes);
    w.passes = reinterpret_cast<unsigned*>(p + 2 * w.flags_bytes);
    w.act0 = p + 3 * w.flags_bytes;
    w.act1 = w.act0 + w.act_bytes;
    return w;
}

int classes_launch(const CannyCfg& c, bool bits, const PageSet& s, const PageSetOut& d, int n, const LinkGeom& g, const LinkWork& w,
                   hipStream_t hs, int channels = 1)
{
    const dim3 grid((unsigned)((c.W + kCnTW - 1) / kCnTW), (unsigned)((c.H + kCnRows - 1) / kCnRows), (unsigned)n);
    if (bits && channels == 3) hipLaunchKernelGGL((k_canny_classes<true, 3>), grid, dim3(kCnTW), 0, hs, c, s, d, w.S, w.C, g.plane_words, g.wpr);
    else if (bits && channels == 4) hipLaunchKernelGGL((k_canny_classes<true, 4>), grid, dim3(kCnTW), 0, hs, c, s, d, w.S, w.C, g.plane_words, g.wpr);
    else if (bits) hipLaunchKernelGGL((k_canny_classes<true, 1>), grid, dim3(kCnTW), 0, hs, c, s, d, w.S, w.C, g.plane_words, g.wpr);
    else hipLaunchKernelGGL((k_canny_classes<false, 1>), grid, dim3(kCnTW), 0, hs, c, s, d, (u64*)nullptr, (u64*)nullptr, (size_t)0, 0);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// The planes are in `w`: passes until no page changed, then the strong plane as bytes.  No cap on the passes: every pass that
// changes anything adds a bit, and a plane has finitely many.  h_flags: pinned, canny_pinned_bytes(n); synchronises the stream.
int link_and_expand(const LinkGeom& g, const LinkWork& w, int n, const PageSetOut& d, unsigned* h_flags, int32_t* out_passes, hipStream_t hs)
{
    PRL_HIP_CHECK(hipMemsetAsync(w.changed, 0, 3 * w.flags_bytes, hs));
    PRL_HIP_CHECK(hipMemsetAsync(w.act0, 1, w.act_bytes, hs));   // before the first pass every tile counts as changed
    const unsigned long long tiles = (unsigned long long)n * g.tiles_x * g.tiles_y;
    int group = 4;   // passes per host check, doubled each time (a pass over finished pages and idle tiles is nearly free)
    for (int pass = 0;;) {
        for (int i = 0; i < group; ++i, ++pass) {
            hipLaunchKernelGGL(k_edge_link, dim3((unsigned)tiles), dim3(kLkRows * kLkWords), 0, hs, w.S, w.C, g.plane_words, g.wpr, g.H,
                               g.tiles_x, g.tiles_y, w.changed, w.done, (pass & 1) ? w.act1 : w.act0, (pass & 1) ? w.act0 : w.act1);
            PRL_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_link_endpass, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs, w.changed, w.done, w.passes, n);
            PRL_HIP_CHECK(hipGetLastError());
        }
        PRL_HIP_CHECK(hipMemcpyAsync(h_flags, w.done, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost, hs));
        PRL_HIP_CHECK(hipMemcpyAsync(h_flags + n, w.passes, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost, hs));
        PRL_HIP_CHECK(hipStreamSynchronize(hs));
        if (std::all_of(h_flags, h_flags + n, [](unsigned v) { return v != 0; })) break;
        group = std::min(group * 2, 32);
    }
    if (out_passes)
        for (int i = 0; i < n; ++i) out_passes[i] = (int32_t)h_flags[n + i];
    const dim3 grid((unsigned)(((g.W + 7) / 8 + 255) / 256), (unsigned)g.H, (unsigned)n);
    hipLaunchKernelGGL(k_plane_expand, grid, dim3(256), 0, hs, reinterpret_cast<const uint8_t*>(w.S), g.plane_bytes, (size_t)g.wpr * 8, d, g.W);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

size_t work_per_page(const LinkGeom& g) { return 2 * g.plane_bytes + 3 * sizeof(unsigned) + 2 * (size_t)g.tiles_x * g.tiles_y; }

// threshold1 / threshold2 as cv::Canny reads them; false: a NaN
bool canny_thresholds(double t1, double t2, int* low, int* high)
{
    if (std::isnan(t1) || std::isnan(t2)) return false;
    if (t1 > t2) std::swap(t1, t2);
    *low = (int)std::min(2041.0, std::max(-1.0, std::floor(t1)));
    *high = (int)std::min(2041.0, std::max(-1.0, std::floor(t2)));
    return true;
}

// EMPTY, BAD_CHANNELS, BAD_ARG in this order; gray pages in, a byte map of the same size out, never in place
int gray_map_checks(const PageArgs& a, int channels, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (channels != 1) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, 1, 1, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    return batch ? pages_overlap_ok(a, 1, 1, false) : PRL_OK;
}

int canny_batch(const PageArgs& a, int low, int high, void* stream)
{
    if (a.n_pages == 0) return PRL_OK;
    const int chunk = canny_pages_per_chunk(a.n_pages, a.width, a.height, 0);
    WorkScope w;
    int st = w.open(stream, canny_work_bytes(chunk, a.width, a.height), 0, canny_pinned_bytes(chunk));
    if (st != PRL_OK) return st;
    for (int first = 0; first < a.n_pages; first += chunk) {
        st = canny_run(a.width, a.height, low, high, src_pages(a, first), dst_pages(a, first), std::min(chunk, a.n_pages - first), w.scratch(),
                       w.pinned<unsigned>(), w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

}  // namespace

// ---- what prl_internal.h declares of this file ---------------------------------------------------------------------------------

size_t canny_work_bytes(int n, int W, int H) { return work_per_page(link_geom(W, H)) * (size_t)n + 5 * 256; }   // (the five small blocks' rounding)
size_t canny_pinned_bytes(int n) { return 2 * sizeof(unsigned) * (size_t)n; }

int canny_pages_per_chunk(int n_pages, int W, int H, size_t extra_per_page)
{
    const LinkGeom g = link_geom(W, H);
    const int by_tiles = (int)std::max<unsigned long long>(1, 0x7fffffffull / ((unsigned long long)g.tiles_x * g.tiles_y));
    return stage_chunk(n_pages, work_per_page(g) + extra_per_page, (size_t)4 << 30, std::min(65535, by_tiles));
}

void canny_threshold_table(double upper_coeff, double lower_coeff, int* lut)
{
    for (int t = 0; t < 256; ++t) {   // imageLibCommon.cpp:302-306, in float64
        const double upper = upper_coeff * (double)t;
        const double lower = lower_coeff * upper;
        canny_thresholds(lower, upper, &lut[2 * t], &lut[2 * t + 1]);
    }
}

int canny_run(int W, int H, int low, int high, const PageSet& s, const PageSetOut& d, int n, uint8_t* work, unsigned* h_flags, hipStream_t hs,
              int channels, const int* d_lut, const int* d_page_t)
{
    const LinkGeom g = link_geom(W, H);
    const LinkWork w = link_work(g, n, work);
    CannyCfg cfg{W, H, low, high};
    cfg.lut = d_lut;
    cfg.page_t = d_page_t;
    const int st = classes_launch(cfg, true, s, d, n, g, w, hs, channels);
    if (st != PRL_OK) return st;
    return link_and_expand(g, w, n, d, h_flags, nullptr, hs);
}

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_canny_classes_batch_device(int n_pages, int channels, double threshold1, double threshold2, const uint8_t* d_src,
                                       size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                       size_t dst_page_stride, size_t dst_step, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    int st = gray_map_checks(a, channels, true);
    if (st != PRL_OK) return st;
    int low, high;
    if (!canny_thresholds(threshold1, threshold2, &low, &high)) return bad_arg("Canny: a threshold is a NaN");
    if (n_pages == 0) return PRL_OK;
    int dev;   // no workspace and no lock: the device check alone
    if ((st = current_device(&dev)) != PRL_OK) return st;
    const CannyCfg c{width, height, low, high};
    const LinkGeom g = link_geom(width, height);
    const int chunk = stage_chunk(n_pages, 0);
    for (int first = 0; first < n_pages; first += chunk) {
        st = classes_launch(c, false, src_pages(a, first), dst_pages(a, first), std::min(chunk, n_pages - first), g, LinkWork{},
                            static_cast<hipStream_t>(stream));
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int prl_hip_edge_link_batch_device(int n_pages, const uint8_t* d_classes, size_t src_page_stride, size_t src_step, int width, int height,
                                   uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, int32_t* out_passes, void* stream)
{
    const PageArgs a{n_pages, d_classes, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    int st = gray_map_checks(a, 1, true);
    if (st != PRL_OK) return st;
    if (n_pages == 0) return PRL_OK;
    const int chunk = canny_pages_per_chunk(n_pages, width, height, 0);
    WorkScope w;
    st = w.open(stream, canny_work_bytes(chunk, width, height), 0, canny_pinned_bytes(chunk));
    if (st != PRL_OK) return st;
    const LinkGeom g = link_geom(width, height);
    for (int first = 0; first < n_pages; first += chunk) {
        const int n = std::min(chunk, n_pages - first);
        const LinkWork lw = link_work(g, n, w.scratch());
        const dim3 grid((unsigned)((width + 255) / 256), (unsigned)height, (unsigned)n);
        hipLaunchKernelGGL(k_classes_pack, grid, dim3(256), 0, w.stream, src_pages(a, first), width, lw.S, lw.C, g.plane_words, g.wpr);
        PRL_HIP_CHECK(hipGetLastError());
        st = link_and_expand(g, lw, n, dst_pages(a, first), w.pinned<unsigned>(), out_passes ? out_passes + first : nullptr, w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int prl_hip_canny_batch_device(int n_pages, int channels, double threshold1, double threshold2, const uint8_t* d_src, size_t src_page_stride,
                               size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    const PageArgs a{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step};
    const int st = gray_map_checks(a, channels, true);
    if (st != PRL_OK) return st;
    int low, high;
    if (!canny_thresholds(threshold1, threshold2, &low, &high)) return bad_arg("Canny: a threshold is a NaN");
    return canny_batch(a, low, high, stream);
}

int prl_hip_canny_host(int channels, double threshold1, double threshold2, const uint8_t* src, size_t src_step, int width, int height,
                       uint8_t* dst, size_t dst_step)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = gray_map_checks(a, channels, false);
    if (st != PRL_OK) return st;
    int low, high;
    if (!canny_thresholds(threshold1, threshold2, &low, &high)) return bad_arg("Canny: a threshold is a NaN");
    return stage_host_pages(a, 1, 1, width, height, [&](const PageArgs& page, hipStream_t s) { return canny_batch(page, low, high, s); });
}

}  // extern "C"
