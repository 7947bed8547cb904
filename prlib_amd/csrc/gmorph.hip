// gmorph.hip — flat-element grayscale morphology on 8-bit pages of 1..4 interleaved channels: cv::erode / cv::dilate /
// cv::morphologyEx with cv::getStructuringElement(RECT | CROSS | ELLIPSE, Size(kw, kh)), an anchor and iterations, and on top of it
// prl::correctNUIL (src/correctNUIL.cpp:33-90): per channel, invert where the page's mean is below 128, then
// 255 - blackhat(channel, ellipse(size, size)).
//
//   dst(y, x, c) = min / max over the element's set pixels (i, j) of src(y + i - ay, x + j - ax, c), (ax, ay) the anchor (the
//   centre (kw/2, kh/2) unless the caller names one); taps outside the page are ignored (morphologyDefaultBorderValue); the
//   element is NOT reflected between the two operators.  n iterations of a full rectangle run once with the rectangle grown to
//   1 + n (k - 1) a side and the anchor n times as far [upstream]; any other element runs n passes (gm_add).
//
// Row i of every element is one half-open span [j1, j2) of columns (gm_spans).  So an output is a max over at most kh
// horizontal span maxima, and a span of w pixels is the max of two windows of 2^k <= w pixels that overlap.
//
// Two kernels (no user option; the hooks build forces the first with PRL_HIP_GMORPH_LITERAL=1):
//   k_gm_literal   the definition: a lane per output byte walks every set pixel of the element.  The executable
//                  specification, and the route of the elements whose tile does not fit k_gm_span's LDS budget.
//   k_gm_span<C>   a workgroup owns a tile of outputs plus the element's halo as BYTES in LDS.  Erosion runs as dilation of
//                  the complement (x ^ 255 on load and on store; out-of-page taps are 0), so there is one max engine.
//                  Level k holds, per byte column q of a row, the max of the 2^k pixels q, q + C, ..., q + (2^k - 1) C; it
//                  is built from level k - 1 by one doubling step over the whole buffer (two buffers, ping-pong, one barrier
//                  per level).  The element's rows are sorted by the level their span needs, and each lane keeps its 4
//                  output dwords as accumulators in registers while the levels go by: per element row and output dword two
//                  window reads, each = two aligned ds_read_b32 + two v_perm_b32 (which both shift to the byte offset and
//                  split even / odd bytes into halfwords) + two v_pk_max_u16.  The accumulators stay split until the store.
// Rectangles are separable: a kw x 1 pass, then a 1 x kh pass (each skipped when 1 wide), both through k_gm_span.
// The composite operators fuse their tail into the last pass: TOPHAT / BLACKHAT subtract against the original page there,
// correctNUIL also applies its final 255 - x, and its per-channel inversion is an XOR on the first pass's loads (the channel
// sums come from k_gm_sums into the device's small block: no host round trip).
// Intermediate planes live in the device context's scratch, at most two tight planes per page of a chunk.
#include "prl_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace prl_hip {

namespace {

constexpr int kGmMaxK = 255;          // element sizes 1..255 (the spans travel as bytes in the kernel arguments)
constexpr int kGmMaxIters = 16;        // cv::morphologyEx's `iterations`
constexpr int kGmThreads = 256;
constexpr int kGmItems = 4;           // output dwords per lane of k_gm_span
constexpr int kGmLdsBytes = 64 * 1024;   // both level buffers of a workgroup: at least two workgroups per CU (160 KiB)
constexpr int kGmSumThreads = 192;    // a multiple of 1, 2, 3 and 4: a lane's channel is fixed along a row
constexpr int kGmSumRows = 32;        // 32 rows x 131072 bytes x 255 < 2^32

enum { EP_NONE = 0, EP_TOPHAT = 1, EP_BLACKHAT = 2, EP_NUIL = 3 };

// The non-empty rows of an element, sorted by level = floor(log2(j2 - j1)).  A kernel argument (uniform loads).
struct GmElem {
    int kw, kh, ax, ay;   // size and anchor
    int n, levels;        // rows below; the highest level
    uint8_t row[kGmMaxK], j1[kGmMaxK], j2[kGmMaxK];
};

struct GmPass {
    int W, H, R;          // pixels; R = W * C row bytes
    int erode;            // 1: min, 0: max
    int ep;               // EP_*: what the pass does with its result v and the original page's o at the same byte
    int invert_src;       // this pass reads the original page: its loads take the channel inversion
    const unsigned long long* sums;   // correctNUIL: 4 channel sums per page (null otherwise); inverted where sum < half
    unsigned long long half;          // 128 * W * H
    PageSet orig;         // the original page (ep != EP_NONE)
};

struct GmTile {
    int th, twb;          // outputs: rows, bytes (a multiple of 4)
    int rows, pitch;      // LDS rows th + kh - 1 of pitch bytes (a multiple of 4)
    int lead;             // LDS column 0 is source byte xb0 - ax * C - lead, a multiple of 4
    int buf_dwords;       // one level buffer, slack for the doubling step's reads past the last row included
};

__device__ __forceinline__ int gm_finish(int v, int o, int ep)
{
    switch (ep) {
    case EP_TOPHAT: return max(o - v, 0);           // src - open, saturating
    case EP_BLACKHAT: return max(v - o, 0);         // close - src
    case EP_NUIL: return 255 - max(v - o, 0);
    default: return v;
    }
}

__device__ __forceinline__ uint32_t gm_channel_mask(const GmPass& p, int page, int c)
{
    return (p.sums && p.sums[(size_t)page * 4 + c] < p.half) ? 255u : 0u;
}

// ---- the definition ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kGmThreads) void k_gm_literal(PageSet src, PageSetOut dst, GmElem el, GmPass p, int C)
{
    const int b = blockIdx.x * kGmThreads + threadIdx.x;
    if (b >= p.R) return;
    const int y = blockIdx.y, page = blockIdx.z;
    const int x = b / C, c = b - (b / C) * C;
    const uint32_t cm = gm_channel_mask(p, page, c);
    const uint32_t lm = p.invert_src ? cm : 0u;
    const uint8_t* sp = src.page(page) + c;
    int acc = p.erode ? 255 : 0;
    for (int e = 0; e < el.n; ++e) {
        const int sy = y + (int)el.row[e] - el.ay;
        if (sy < 0 || sy >= p.H) continue;
        const uint8_t* row = sp + (size_t)sy * src.step;
        const int ja = max((int)el.j1[e], el.ax - x), jb = min((int)el.j2[e], p.W - x + el.ax);
        for (int j = ja; j < jb; ++j) {
            const int v = (int)(row[(size_t)(x + j - el.ax) * C] ^ lm);
            acc = p.erode ? min(acc, v) : max(acc, v);
        }
    }
    if (p.ep != EP_NONE) {
        const int o = (int)(p.orig.page(page)[(size_t)y * p.orig.step + b] ^ cm);
        acc = gm_finish(acc, o, p.ep);
    }
    dst.page(page)[(size_t)y * dst.step + b] = (uint8_t)acc;
}

// ---- the span engine -----------------------------------------------------------------------------------------------------
typedef unsigned short gm_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t gm_pk_max(uint32_t a, uint32_t b)   // v_pk_max_u16
{
    const gm_u16x2 r = __builtin_elementwise_max(__builtin_bit_cast(gm_u16x2, a), __builtin_bit_cast(gm_u16x2, b));
    return __builtin_bit_cast(uint32_t, r);
}

// byte i of a word that packs one mask byte per channel
__device__ __forceinline__ uint32_t gm_pick(uint32_t packed, int i) { return (packed >> (8 * i)) & 255u; }

// Bytes s, s + 2 (even) and s + 1, s + 3 (odd) of the 8 bytes {hi : lo}, each zero-extended to a halfword: v_perm_b32 with
// selector bytes 0..7 = a byte of {hi : lo}, 0x0c = 0.  `s` (0..3) is uniform over the wavefront.
__device__ __forceinline__ void gm_window(const uint32_t* buf, int byte_off, uint32_t& even, uint32_t& odd)
{
    const uint32_t lo = buf[byte_off >> 2], hi = buf[(byte_off >> 2) + 1];
    const uint32_t s = (uint32_t)byte_off & 3u;
    even = __builtin_amdgcn_perm(hi, lo, 0x0c020c00u + s * 0x00010001u);
    odd = __builtin_amdgcn_perm(hi, lo, 0x0c030c01u + s * 0x00010001u);
}

// grid = (ceil(R / twb), ceil(H / th), pages); dynamic LDS = 2 * buf_dwords * 4 bytes.
// al_src / al_dst / al_orig: the set's base, step and page stride are multiples of 4 (dword access).
template <int C>
__global__ __launch_bounds__(kGmThreads) void k_gm_span(PageSet src, PageSetOut dst, GmElem el, GmPass p, GmTile t, int al_src,
                                                        int al_dst)
{
    extern __shared__ uint32_t gm_lds[];
    uint32_t* cur = gm_lds;
    uint32_t* oth = gm_lds + t.buf_dwords;
    const int tid = threadIdx.x, page = blockIdx.z;
    const int y0 = blockIdx.y * t.th, xb0 = blockIdx.x * t.twb;
    const uint32_t flip = p.erode ? 255u : 0u;
    uint32_t cm = 0;   // byte c: channel c's inversion (0 / 255)
#pragma unroll
    for (int c = 0; c < C; ++c) cm |= gm_channel_mask(p, page, c) << (8 * c);
    const uint32_t lm = (p.invert_src ? cm : 0u) ^ (flip * 0x01010101u);   // what a load is XORed with, per channel

    {   // level 0: the tile and its halo; taps outside the page are 0 (the dilation's identity)
        const uint8_t* sp = src.page(page);
        const int pd = t.pitch >> 2;
        const int sb0 = xb0 - el.ax * C - t.lead;
        const int ndw = t.rows * pd;
        for (int d = tid; d < ndw; d += kGmThreads) {
            const int r = d / pd;
            const int sy = y0 - el.ay + r, sb = sb0 + (d - r * pd) * 4;
            uint32_t v = 0;
            if (sy >= 0 && sy < p.H && sb > -4 && sb < p.R) {
                const uint8_t* row = sp + (size_t)sy * src.step;
                const int c0 = (sb + 4 * C) % C;   // sb >= -3
                uint32_t m = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) m |= gm_pick(lm, (c0 + j) % C) << (8 * j);
                if (al_src && sb >= 0 && sb + 3 < p.R) {
                    v = *reinterpret_cast<const uint32_t*>(row + sb) ^ m;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (sb + j >= 0 && sb + j < p.R) v |= ((uint32_t)row[sb + j] ^ ((m >> (8 * j)) & 255u)) << (8 * j);
                }
            }
            cur[d] = v;
        }
    }
    __syncthreads();

    const int tq = t.twb >> 2;
    const int nitems = t.th * tq;
    int base[kGmItems];            // LDS byte of the item's element origin (row 0, column 0): a multiple of 4, plus lead
    uint32_t acc_e[kGmItems], acc_o[kGmItems];
#pragma unroll
    for (int k = 0; k < kGmItems; ++k) {
        const int idx = min(tid + k * kGmThreads, nitems - 1);   // (spare lanes redo the last item and do not store)
        const int ty = idx / tq;
        base[k] = ty * t.pitch + (idx - ty * tq) * 4 + t.lead;
        acc_e[k] = acc_o[k] = 0;
    }

    int e = 0;
    for (int lvl = 0; lvl <= el.levels; ++lvl) {
        if (lvl > 0) {   // level lvl from level lvl - 1, over the whole buffer (what spills over a row's end is never consumed)
            const int off = (C << (lvl - 1));
            const int ndw = t.rows * (t.pitch >> 2);
            for (int d = tid; d < ndw; d += kGmThreads) {
                const uint32_t a = cur[d];
                uint32_t be, bo;
                gm_window(cur, 4 * d + off, be, bo);
                const uint32_t me = gm_pk_max(a & 0x00ff00ffu, be), mo = gm_pk_max((a >> 8) & 0x00ff00ffu, bo);
                oth[d] = me | (mo << 8);
            }
            __syncthreads();
            uint32_t* x = cur;
            cur = oth;
            oth = x;
        }
        for (; e < el.n; ++e) {
            const int j1 = el.j1[e], j2 = el.j2[e];
            if (31 - __builtin_clz((unsigned)(j2 - j1)) != lvl) break;
            const int oa = (int)el.row[e] * t.pitch + j1 * C;
            const int ob = (int)el.row[e] * t.pitch + (j2 - (1 << lvl)) * C;
#pragma unroll
            for (int k = 0; k < kGmItems; ++k) {
                uint32_t we, wo;
                gm_window(cur, base[k] + oa, we, wo);
                acc_e[k] = gm_pk_max(acc_e[k], we);
                acc_o[k] = gm_pk_max(acc_o[k], wo);
                if (ob != oa) {
                    gm_window(cur, base[k] + ob, we, wo);
                    acc_e[k] = gm_pk_max(acc_e[k], we);
                    acc_o[k] = gm_pk_max(acc_o[k], wo);
                }
            }
        }
    }

    uint8_t* dp = dst.page(page);
    const uint8_t* op = p.ep != EP_NONE ? p.orig.page(page) : nullptr;
#pragma unroll
    for (int k = 0; k < kGmItems; ++k) {
        const int idx = tid + k * kGmThreads;
        if (idx >= nitems) continue;
        const int ty = idx / tq;
        const int y = y0 + ty, xb = xb0 + (idx - ty * tq) * 4;
        if (y >= p.H || xb >= p.R) continue;
        uint32_t v = (acc_e[k] | (acc_o[k] << 8)) ^ (flip * 0x01010101u);
        const int nb = min(4, p.R - xb);
        if (p.ep != EP_NONE) {
            const uint8_t* orow = op + (size_t)y * p.orig.step + xb;
            const int c0 = xb % C;
            uint32_t r = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nb) {
                    const int o = (int)((uint32_t)orow[j] ^ gm_pick(cm, (c0 + j) % C));
                    r |= (uint32_t)gm_finish((int)((v >> (8 * j)) & 255u), o, p.ep) << (8 * j);
                }
            }
            v = r;
        }
        uint8_t* drow = dp + (size_t)y * dst.step + xb;
        if (al_dst && nb == 4) {
            *reinterpret_cast<uint32_t*>(drow) = v;
        } else {
            for (int j = 0; j < nb; ++j) drow[j] = (uint8_t)(v >> (8 * j));
        }
    }
}

// correctNUIL's cv::mean, as integer channel sums: sums[page * 4 + c] += the bytes of channel c (zeroed by the caller)
__global__ __launch_bounds__(kGmSumThreads) void k_gm_sums(PageSet src, int R, int H, int C, unsigned long long* sums)
{
    __shared__ unsigned int part[4];
    const int tid = threadIdx.x, page = blockIdx.y;
    if (tid < 4) part[tid] = 0;
    __syncthreads();
    const int ya = blockIdx.x * kGmSumRows, yb = min(ya + kGmSumRows, H);
    const uint8_t* sp = src.page(page);
    unsigned int acc = 0;
    for (int y = ya; y < yb; ++y) {
        const uint8_t* row = sp + (size_t)y * src.step;
        for (int b = tid; b < R; b += kGmSumThreads) acc += row[b];
    }
    atomicAdd(&part[tid % C], acc);
    __syncthreads();
    if (tid < C) atomicAdd(&sums[(size_t)page * 4 + tid], (unsigned long long)part[tid]);
}

// ---- host ----------------------------------------------------------------------------------------------------------------

// cv::getStructuringElement(shape, Size(kw, kh)) with anchor (kw/2, kh/2) as row spans ([upstream] OpenCV 3.4 / 4.x)
void gm_spans(int shape, int kw, int kh, std::vector<int>* j1, std::vector<int>* j2)
{
    if (kw == 1 && kh == 1) shape = PRL_SHAPE_RECT;
    const int r = kh / 2, c = kw / 2;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    j1->assign(kh, 0);
    j2->assign(kh, 0);
    for (int i = 0; i < kh; ++i) {
        int a = 0, b = 0;
        if (shape == PRL_SHAPE_RECT || (shape == PRL_SHAPE_CROSS && i == r)) {
            b = kw;
        } else if (shape == PRL_SHAPE_CROSS) {
            a = c;
            b = c + 1;
        } else {
            const int dy = i - r;
            if (std::abs(dy) <= r) {
                const int dx = (int)std::nearbyint(c * std::sqrt((r * r - dy * dy) * inv_r2));   // cvRound: half to even
                a = std::max(c - dx, 0);
                b = std::min(c + dx + 1, kw);
            }
        }
        (*j1)[i] = a;
        (*j2)[i] = b;
    }
}

GmElem gm_elem(int kw, int kh, int ax, int ay, const std::vector<int>& j1, const std::vector<int>& j2)
{
    GmElem el{};
    el.kw = kw;
    el.kh = kh;
    el.ax = ax;
    el.ay = ay;
    auto level = [&](int i) { return 31 - __builtin_clz((unsigned)(j2[i] - j1[i])); };
    std::vector<int> rows;
    for (int i = 0; i < kh; ++i)
        if (j2[i] > j1[i]) rows.push_back(i);
    std::stable_sort(rows.begin(), rows.end(), [&](int a, int b) { return level(a) < level(b); });
    for (int i : rows) {
        el.row[el.n] = (uint8_t)i;
        el.j1[el.n] = (uint8_t)j1[i];
        el.j2[el.n] = (uint8_t)j2[i];
        el.levels = std::max(el.levels, level(i));
        ++el.n;
    }
    return el;
}

GmElem gm_rect(int kw, int kh, int ax, int ay)
{
    return gm_elem(kw, kh, ax, ay, std::vector<int>(kh, 0), std::vector<int>(kh, kw));
}

// The tile of k_gm_span for an element: the candidate with the most outputs per LDS byte whose two buffers fit.
bool gm_tile(const GmElem& el, int C, GmTile* out)
{
    const int lead = (4 - (el.ax * C) % 4) % 4;
    const int slack = (el.levels ? ((C << (el.levels - 1)) + 3) / 4 * 4 : 0) + 8;
    double best = 0.0;
    for (int th = 4; th <= 128; th *= 2)
        for (int twb = 32; twb <= 512; twb *= 2) {
            if (th * (twb / 4) > kGmThreads * kGmItems) continue;
            GmTile t{th, twb, th + el.kh - 1, (lead + twb + (el.kw - 1) * C + 3) / 4 * 4, lead, 0};
            const int bytes = t.rows * t.pitch + slack;
            t.buf_dwords = bytes / 4;
            if (2 * bytes > kGmLdsBytes) continue;
            const double score = (double)th * twb / ((double)t.rows * t.pitch);
            if (score > best) {
                best = score;
                *out = t;
            }
        }
    return best > 0.0;
}

template <typename Set> bool gm_aligned(const Set& s)
{
    return !s.table && ((reinterpret_cast<uintptr_t>(s.base) | s.page_stride | s.step) & 3u) == 0;
}

int gm_launch(const GmElem& el, const GmPass& p, int C, bool literal, const PageSet& s, const PageSetOut& d, int n, hipStream_t stream)
{
    GmTile t{};
    if (!literal && gm_tile(el, C, &t)) {
        const dim3 grid((unsigned)((p.R + t.twb - 1) / t.twb), (unsigned)((p.H + t.th - 1) / t.th), (unsigned)n);
        const size_t lds = (size_t)t.buf_dwords * 8;
        const int as = gm_aligned(s), ad = gm_aligned(d);
        switch (C) {
        case 1: hipLaunchKernelGGL(k_gm_span<1>, grid, dim3(kGmThreads), lds, stream, s, d, el, p, t, as, ad); break;
        case 2: hipLaunchKernelGGL(k_gm_span<2>, grid, dim3(kGmThreads), lds, stream, s, d, el, p, t, as, ad); break;
        case 3: hipLaunchKernelGGL(k_gm_span<3>, grid, dim3(kGmThreads), lds, stream, s, d, el, p, t, as, ad); break;
        default: hipLaunchKernelGGL(k_gm_span<4>, grid, dim3(kGmThreads), lds, stream, s, d, el, p, t, as, ad); break;
        }
    } else {
        const dim3 grid((unsigned)((p.R + kGmThreads - 1) / kGmThreads), (unsigned)p.H, (unsigned)n);
        hipLaunchKernelGGL(k_gm_literal, grid, dim3(kGmThreads), 0, stream, s, d, el, p, C);
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

struct GmStep {
    GmElem el;
    int erode;
};

// What one call runs: the passes in order, the tail the last one carries, whether the first one inverts on load.
struct GmPlan {
    std::vector<GmStep> steps;
    int ep = EP_NONE;
    bool nuil = false;
    int planes = 0;   // scratch planes per page
};

// erode / dilate with the element, `iters` times, anchor (ax, ay).  A full rectangle runs once, grown to 1 + iters (k - 1) a
// side with the anchor iters times as far [upstream, morph.cpp], as its two one-dimensional passes unless `literal`; any other
// element runs `iters` real passes.
void gm_add(GmPlan* plan, int shape, int kw, int kh, int ax, int ay, int iters, int erode, bool literal)
{
    std::vector<int> j1, j2;
    gm_spans(shape, kw, kh, &j1, &j2);
    bool rect = true;
    for (int i = 0; i < kh; ++i) rect = rect && j1[i] == 0 && j2[i] == kw;
    if (rect) {
        kw = 1 + iters * (kw - 1);
        kh = 1 + iters * (kh - 1);
        ax *= iters;
        ay *= iters;
        if (!literal && kw > 1 && kh > 1) {
            plan->steps.push_back({gm_rect(kw, 1, ax, 0), erode});
            plan->steps.push_back({gm_rect(1, kh, 0, ay), erode});
        } else {
            plan->steps.push_back({gm_rect(kw, kh, ax, ay), erode});
        }
        return;
    }
    for (int i = 0; i < iters; ++i) plan->steps.push_back({gm_elem(kw, kh, ax, ay, j1, j2), erode});
}

struct GmOp {
    int op, shape, kw, kh;
    bool nuil;
    int ax = -1, ay = -1;   // -1: the centre k / 2
    int iters = 1;
};

// every row of the element is full: what gm_add grows over the iterations
bool gm_is_rect(int shape, int kw, int kh)
{
    std::vector<int> j1, j2;
    gm_spans(shape, kw, kh, &j1, &j2);
    for (int i = 0; i < kh; ++i)
        if (j1[i] != 0 || j2[i] != kw) return false;
    return true;
}

GmPlan gm_plan(const GmOp& o, bool in_place, bool literal)
{
    GmPlan plan;
    plan.nuil = o.nuil;
    const int op = o.op, ax = o.ax < 0 ? o.kw / 2 : o.ax, ay = o.ay < 0 ? o.kh / 2 : o.ay;
    const bool first_erodes = op == PRL_MORPH_ERODE || op == PRL_MORPH_OPEN || op == PRL_MORPH_TOPHAT;
    gm_add(&plan, o.shape, o.kw, o.kh, ax, ay, o.iters, first_erodes ? 1 : 0, literal);
    if (op != PRL_MORPH_ERODE && op != PRL_MORPH_DILATE) gm_add(&plan, o.shape, o.kw, o.kh, ax, ay, o.iters, first_erodes ? 0 : 1, literal);
    if (op == PRL_MORPH_TOPHAT) plan.ep = EP_TOPHAT;
    if (op == PRL_MORPH_BLACKHAT) plan.ep = o.nuil ? EP_NUIL : EP_BLACKHAT;
    // a single pass must not write the pages whose neighbourhoods other workgroups still read: start from a copy
    if (in_place && plan.steps.size() == 1 && (plan.steps[0].el.kw > 1 || plan.steps[0].el.kh > 1))
        plan.steps.insert(plan.steps.begin(), {gm_rect(1, 1, 0, 0), 0});
    plan.planes = (int)std::min<size_t>(2, plan.steps.size() - 1);
    return plan;
}

// one chunk of pages; `tmp`: plan.planes tight planes (R * H bytes per page) one after the other; `sums`: 4 per page (nuil)
int gm_run(const GmPlan& plan, int W, int H, int C, bool literal, const PageSet& src, const PageSetOut& dst, int n, uint8_t* tmp,
           unsigned long long* sums, hipStream_t stream)
{
    const int R = W * C;
    GmPass p{};
    p.W = W;
    p.H = H;
    p.R = R;
    p.orig = src;
    if (plan.nuil) {
        PRL_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)n * 4 * sizeof(unsigned long long), stream));
        const dim3 grid((unsigned)((H + kGmSumRows - 1) / kGmSumRows), (unsigned)n);
        hipLaunchKernelGGL(k_gm_sums, grid, dim3(kGmSumThreads), 0, stream, src, R, H, C, sums);
        PRL_HIP_CHECK(hipGetLastError());
        p.sums = sums;
        p.half = 128ull * (unsigned long long)W * (unsigned long long)H;
    }
    const size_t plane = (size_t)R * H * (size_t)n;
    const PageSetOut t[2] = {page_set_out(tmp, (size_t)R * H, (size_t)R), page_set_out(tmp + plane, (size_t)R * H, (size_t)R)};
    PageSet cur = src;
    const size_t m = plan.steps.size();
    for (size_t i = 0; i < m; ++i) {
        const bool last = i + 1 == m;
        const PageSetOut& out = last ? dst : t[i & 1];
        p.erode = plan.steps[i].erode;
        p.invert_src = i == 0 ? 1 : 0;
        p.ep = last ? plan.ep : EP_NONE;
        const int st = gm_launch(plan.steps[i].el, p, C, literal, cur, out, n, stream);
        if (st != PRL_OK) return st;
        cur = as_source(out);
    }
    return PRL_OK;
}

bool gm_known_op(int op)
{
    return op == PRL_MORPH_ERODE || op == PRL_MORPH_DILATE || op == PRL_MORPH_OPEN || op == PRL_MORPH_CLOSE || op == PRL_MORPH_TOPHAT ||
           op == PRL_MORPH_BLACKHAT;
}

// the checks every entry makes, in the documented order (no device is touched); batch: a *_batch_device entry
int gm_checks(const PageArgs& a, int channels, const GmOp& o, bool batch)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (!gm_known_op(o.op) || o.shape < PRL_SHAPE_RECT || o.shape > PRL_SHAPE_ELLIPSE || o.kw < 1 || o.kh < 1 || o.kw > kGmMaxK ||
        o.kh > kGmMaxK)
        return PRL_ERR_BAD_ARG;
    if (o.ax < -1 || o.ax >= o.kw || o.ay < -1 || o.ay >= o.kh || o.iters < 1 || o.iters > kGmMaxIters) return PRL_ERR_BAD_ARG;
    if (o.iters > 1 && gm_is_rect(o.shape, o.kw, o.kh) && (1 + o.iters * (o.kw - 1) > kGmMaxK || 1 + o.iters * (o.kh - 1) > kGmMaxK))
        return PRL_ERR_BAD_ARG;
    if (channels < 1 || channels > 4) return PRL_ERR_BAD_CHANNELS;
    if ((st = pages_rows_ok(a, channels, channels, batch)) != PRL_OK) return st;
    if ((st = pages_sides_ok(a)) != PRL_OK) return st;
    // in place: the same pages at the same strides; any other overlap of source and destination is refused
    return batch ? pages_overlap_ok(a, channels, channels, true) : PRL_OK;
}

int gm_batch_device(const PageArgs& a, int channels, const GmOp& o, void* stream)
{
    int st = gm_checks(a, channels, o, true);
    if (st != PRL_OK) return st;
    if (a.n_pages == 0) return PRL_OK;
    const bool literal = env_knobs().gmorph_literal;
    const GmPlan plan = gm_plan(o, pages_in_place(a, channels, channels), literal);
    const size_t page_bytes = (size_t)a.width * channels * (size_t)a.height;
    // pages per launch: grid.z, and at most 4 GiB of scratch (one page at least)
    const int chunk = stage_chunk(a.n_pages, page_bytes * plan.planes);
    WorkScope w;   // `scratch`: the plan's planes; `small`: correctNUIL's sums
    st = w.open(stream, page_bytes * (size_t)chunk * plan.planes, o.nuil ? (size_t)chunk * 4 * sizeof(unsigned long long) : 0, 0);
    if (st != PRL_OK) return st;
    for (int first = 0; first < a.n_pages; first += chunk) {
        st = gm_run(plan, a.width, a.height, channels, literal, src_pages(a, first), dst_pages(a, first), std::min(chunk, a.n_pages - first),
                    w.scratch(), w.small<unsigned long long>(), w.stream);
        if (st != PRL_OK) return st;
    }
    return PRL_OK;
}

int gm_host(int channels, const GmOp& o, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step)
{
    const PageArgs a{1, src, 0, src_step, width, height, dst, 0, dst_step};
    const int st = gm_checks(a, channels, o, false);
    if (st != PRL_OK) return st;
    return stage_host_pages(a, channels, channels, width, height,
                            [&](const PageArgs& page, hipStream_t s) { return gm_batch_device(page, channels, o, s); });
}

}  // namespace

int gmorph_open_rect_run(int kw, int kh, int width, int height, const PageSet& src, const PageSetOut& dst, int n_pages, uint8_t* tmp,
                         hipStream_t stream)
{
    const GmPlan plan = gm_plan(GmOp{PRL_MORPH_OPEN, PRL_SHAPE_RECT, kw, kh, false}, false, false);
    return gm_run(plan, width, height, 1, false, src, dst, n_pages, tmp, nullptr, stream);
}

int gmorph_dilate_rect_run(int k, int width, int height, const PageSet& src, const PageSetOut& dst, int n_pages, uint8_t* tmp,
                           hipStream_t stream)
{
    const GmPlan plan = gm_plan(GmOp{PRL_MORPH_DILATE, PRL_SHAPE_RECT, k, k, false}, false, false);
    return gm_run(plan, width, height, 1, false, src, dst, n_pages, tmp, nullptr, stream);
}

int gmorph_close_rect_table_run(int k, int iterations, int width, int height, uint8_t* const* d_table, size_t step, int n_pages,
                                uint8_t* tmp, hipStream_t stream)
{
    const bool literal = env_knobs().gmorph_literal;
    GmOp o{PRL_MORPH_CLOSE, PRL_SHAPE_RECT, k, k, false};
    o.iters = iterations;
    const GmPlan plan = gm_plan(o, true, literal);
    const PageSetOut pages = page_table_out(d_table, step);
    return gm_run(plan, width, height, 1, literal, as_source(pages), pages, n_pages, tmp, nullptr, stream);
}

}  // namespace prl_hip

using namespace prl_hip;

extern "C" {

int prl_hip_morphology_batch_device(int n_pages, int channels, int op, int shape, int ksize_w, int ksize_h, const uint8_t* d_src,
                                    size_t src_page_stride, size_t src_step, int width, int height, uint8_t* d_dst,
                                    size_t dst_page_stride, size_t dst_step, void* stream)
{
    return gm_batch_device(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, channels,
                           GmOp{op, shape, ksize_w, ksize_h, false}, stream);
}

int prl_hip_morphology_host(int channels, int op, int shape, int ksize_w, int ksize_h, const uint8_t* src, size_t src_step, int width,
                            int height, uint8_t* dst, size_t dst_step)
{
    return gm_host(channels, GmOp{op, shape, ksize_w, ksize_h, false}, src, src_step, width, height, dst, dst_step);
}

int prl_hip_morphology_ex_batch_device(int n_pages, int channels, int op, int shape, int ksize_w, int ksize_h, int anchor_x, int anchor_y,
                                       int iterations, const uint8_t* d_src, size_t src_page_stride, size_t src_step, int width, int height,
                                       uint8_t* d_dst, size_t dst_page_stride, size_t dst_step, void* stream)
{
    return gm_batch_device(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, channels,
                           GmOp{op, shape, ksize_w, ksize_h, false, anchor_x, anchor_y, iterations}, stream);
}

int prl_hip_morphology_ex_host(int channels, int op, int shape, int ksize_w, int ksize_h, int anchor_x, int anchor_y, int iterations,
                               const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst, size_t dst_step)
{
    return gm_host(channels, GmOp{op, shape, ksize_w, ksize_h, false, anchor_x, anchor_y, iterations}, src, src_step, width, height, dst,
                   dst_step);
}

int prl_hip_correct_nuil_batch_device(int n_pages, int channels, int size, const uint8_t* d_src, size_t src_page_stride,
                                      size_t src_step, int width, int height, uint8_t* d_dst, size_t dst_page_stride, size_t dst_step,
                                      void* stream)
{
    return gm_batch_device(PageArgs{n_pages, d_src, src_page_stride, src_step, width, height, d_dst, dst_page_stride, dst_step}, channels,
                           GmOp{PRL_MORPH_BLACKHAT, PRL_SHAPE_ELLIPSE, size, size, true}, stream);
}

int prl_hip_correct_nuil_host(int channels, int size, const uint8_t* src, size_t src_step, int width, int height, uint8_t* dst,
                              size_t dst_step)
{
    return gm_host(channels, GmOp{PRL_MORPH_BLACKHAT, PRL_SHAPE_ELLIPSE, size, size, true}, src, src_step, width, height, dst, dst_step);
}

}  // extern "C"
