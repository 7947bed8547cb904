// components.hip — connected components of batched 8-bit maps and rule R's external rectangles (include/prl_hip.h, next to
// prl_hip_external_rects; the plain-loop form: components.h).
//
// One int32 plane per page: the word of pixel p (p = y W + x) ends as the smallest linear index of p's own-class component,
// foreground 8- (or 4-) connected, background 4-connected, both labelled by the same passes:
//
//   k_cc_tile      a workgroup per 32 x 32 tile: union-find in LDS over the tile's own pixels (left, up and, for the foreground,
//                  the two upper diagonals), flattened, stored as page indices.  A tile's order is the page's order, so a tile
//                  root is the first pixel of its piece.
//   k_cc_seam      a workgroup per tile: the pixels of its top row, left column and right column unite with their neighbours in
//                  the adjacent tiles (corners for the foreground only) by atomic minimum on the plane.
//   k_cc_flatten   every word becomes its root.
//
// A union links the larger root under the smaller; a word only ever decreases, a find walks strictly downwards and a failed
// atomic minimum retries from a smaller index: every loop ends, whatever another workgroup does, and nothing waits for anything.
//
//   k_cc_outer     the background pixels of the page's border flag their root (bit 30 of the root's own word): one flag per root.
//   k_cc_count<false>, k_cc_scan, k_cc_count<true>   the ordered prefix count of the roots to number (all foreground roots, or
//                  rule R's external ones: x == 0 or the left neighbour's root is flagged), 4096 pixels a workgroup; the root's
//                  word becomes flag | number.  A root is a first pixel: root order is the order asked for.
//   k_cc_stats     per pass of at most cc_pass_components() components: left, right, bottom and area by integer atomics, one
//                  set per run of equal numbers within a wavefront's 64 consecutive pixels; top is the root's row.
//   k_cc_kept<false>, k_cc_scan, k_cc_kept<true>   the kept filter and the second ordered compaction, 256 components a workgroup.
//   k_cc_labels    0 / 1 .. K into the caller's planes.
//
// Only the per-page counts cross to the host.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "components.h"
#include "prl_internal.h"

namespace prl_hip {

namespace {

constexpr int kT = kCcTile;
constexpr int kScanBlock = 4096;   // pixels a workgroup of the numbering counts
constexpr int kKeptBlock = 256;    // components a workgroup of the second compaction counts

struct CcDev {
    PageSet maps;
    int W, H, n;
    int fg8;          // the foreground unites across corners
    int external;
    int32_t* labels;  // n planes of `plane` words
    size_t plane;
    int32_t* bcount;  // n rows of nb_stride words: the numbering's block counts, then their exclusive prefix
    int nb, nb_stride;
    int32_t* count;   // n: components numbered per page
    int32_t* kept;    // n: rectangles kept per page
    int32_t* off;     // n + 1: the prefix sums of `count`
    int32_t* stats;   // a pass: left, top, right, bottom, area
    int32_t* rects;   // a pass: x, y, w, h of the kept
    int32_t* kbcount; // a pass: the compaction's block counts
};

// ---- labelling ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int lds_find(volatile int* lab, int p)
{
    int q;
    while ((q = lab[p]) != p) p = q;
    return p;
}

__device__ __forceinline__ void lds_union(int* lab, int a, int b)
{
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }   // a > b: a goes under b
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;   // a was no root any more: what it pointed to unites with b
    }
}

// grid = (tiles across, tiles down, pages)
__global__ __launch_bounds__(256) void k_cc_tile(CcDev d)
{
    __shared__ int lab[kT * kT];
    __shared__ uint8_t cls[kT * kT];   // 0 background, 1 foreground, 2 outside the page
    const int x0 = blockIdx.x * kT, y0 = blockIdx.y * kT;
    const uint8_t* m = d.maps.page(blockIdx.z);
    for (int l = threadIdx.x; l < kT * kT; l += 256) {
        const int x = x0 + (l & (kT - 1)), y = y0 + l / kT;
        cls[l] = x < d.W && y < d.H ? (m[(size_t)y * d.maps.step + x] != 0) : 2;
        lab[l] = l;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < kT * kT; l += 256) {
        const int c = cls[l], lx = l & (kT - 1), ly = l / kT;
        if (c == 2) continue;
        if (lx > 0 && cls[l - 1] == c) lds_union(lab, l, l - 1);
        if (ly > 0 && cls[l - kT] == c) lds_union(lab, l, l - kT);
        if (c == 1 && d.fg8 && ly > 0) {
            if (lx > 0 && cls[l - kT - 1] == 1) lds_union(lab, l, l - kT - 1);
            if (lx < kT - 1 && cls[l - kT + 1] == 1) lds_union(lab, l, l - kT + 1);
        }
    }
    __syncthreads();
    int32_t* L = d.labels + d.plane * blockIdx.z;
    for (int l = threadIdx.x; l < kT * kT; l += 256) {
        if (cls[l] == 2) continue;
        const int r = lds_find(lab, l);
        L[(size_t)(y0 + l / kT) * d.W + x0 + (l & (kT - 1))] = (y0 + r / kT) * d.W + x0 + (r & (kT - 1));
    }
}

__device__ __forceinline__ int g_load(const int32_t* L, int p) { return __hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int g_find(const int32_t* L, int p)
{
    int q;
    while ((q = g_load(L, p)) != p) p = q;
    return p;
}

__device__ __forceinline__ void g_union(int32_t* L, int a, int b)
{
    for (;;) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

// grid = (tiles across, tiles down, pages); 96 lanes at work: the tile's top row, left column, right column
__global__ __launch_bounds__(128) void k_cc_seam(CcDev d)
{
    const int role = threadIdx.x / kT, i = threadIdx.x & (kT - 1);
    if (role > 2) return;
    const int x0 = blockIdx.x * kT, y0 = blockIdx.y * kT;
    const int x = role == 0 ? x0 + i : role == 1 ? x0 : x0 + kT - 1, y = role == 0 ? y0 : y0 + i;
    if (x >= d.W || y >= d.H) return;
    const uint8_t* m = d.maps.page(blockIdx.z);
    const size_t step = d.maps.step;
    int32_t* L = d.labels + d.plane * blockIdx.z;
    const bool f = m[(size_t)y * step + x] != 0;
    const int p = y * d.W + x;
    if (role == 0) {
        if (y == 0) return;
        const uint8_t* up = m + (size_t)(y - 1) * step;
        if ((up[x] != 0) == f) g_union(L, p, p - d.W);
        if (f && d.fg8) {
            if (x > 0 && up[x - 1]) g_union(L, p, p - d.W - 1);
            if (x + 1 < d.W && up[x + 1]) g_union(L, p, p - d.W + 1);
        }
    } else if (role == 1) {
        if (x == 0) return;
        if ((m[(size_t)y * step + x - 1] != 0) == f) g_union(L, p, p - 1);
        if (f && d.fg8 && i > 0 && m[(size_t)(y - 1) * step + x - 1]) g_union(L, p, p - d.W - 1);   // (i == 0: the top row's)
    } else {
        if (i == 0 || x + 1 >= d.W || !f || !d.fg8) return;
        if (m[(size_t)(y - 1) * step + x + 1]) g_union(L, p, p - d.W + 1);
    }
}

// grid = (ceil(W H / 256), pages)
__global__ __launch_bounds__(256) void k_cc_flatten(CcDev d)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= d.W * d.H) return;
    int32_t* L = d.labels + d.plane * blockIdx.y;
    const int r = g_find(L, g_load(L, p));   // (a neighbour may have stored its root already: that is a shorter way to the same end)
    __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid = (ceil((2 W + 2 H) / 256), pages)
__global__ __launch_bounds__(256) void k_cc_outer(CcDev d)
{
    int i = blockIdx.x * 256 + threadIdx.x, x, y;
    if (i < d.W) { x = i; y = 0; }
    else if ((i -= d.W) < d.W) { x = i; y = d.H - 1; }
    else if ((i -= d.W) < d.H) { x = 0; y = i; }
    else if ((i -= d.H) < d.H) { x = d.W - 1; y = i; }
    else return;
    if (d.maps.page(blockIdx.y)[(size_t)y * d.maps.step + x]) return;
    int32_t* L = d.labels + d.plane * blockIdx.y;
    const int r = L[y * d.W + x] & kCcIndex;   // (the pixel may be the root, flagged a moment ago)
    L[r] = r | kCcFlag;
}

// ---- the numbering ----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool cc_numbered_root(const CcDev& d, const uint8_t* m, const int32_t* L, int p)
{
    const int y = p / d.W, x = p - y * d.W;
    if (!m[(size_t)y * d.maps.step + x] || L[p] != p) return false;
    if (!d.external || x == 0) return true;
    const int v = L[p - 1];   // the left neighbour of a first pixel is background
    return (v & kCcFlag) || (L[v] & kCcFlag);
}

// the rank of this lane's `sel` among the workgroup's (256 lanes, in lane order) and their total
__device__ __forceinline__ int block_rank(bool sel, int* sums, int* total)
{
    const unsigned long long mask = __ballot(sel);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();   // (the previous round's sums have been read)
    if (lane == 0) sums[wave] = __popcll(mask);
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += sums[w];
    *total = sums[0] + sums[1] + sums[2] + sums[3];
    return base + __popcll(mask & ((1ull << lane) - 1ull));
}

// grid = (nb, pages).  NUMBER = false: the block's count; true: the roots' words become flag | number
template <bool NUMBER>
__global__ __launch_bounds__(256) void k_cc_count(CcDev d)
{
    __shared__ int sums[4];
    const uint8_t* m = d.maps.page(blockIdx.y);
    int32_t* L = d.labels + d.plane * blockIdx.y;
    int32_t* bc = d.bcount + (size_t)d.nb_stride * blockIdx.y;
    const int wh = d.W * d.H;
    int run = NUMBER ? bc[blockIdx.x] : 0;
    for (int k = 0; k < kScanBlock / 256; ++k) {
        const int p = blockIdx.x * kScanBlock + k * 256 + threadIdx.x;   // (at most 2^30 + 4095)
        const bool sel = p < wh && cc_numbered_root(d, m, L, p);
        int total;
        const int rank = block_rank(sel, sums, &total);
        if (NUMBER && sel) L[p] = kCcFlag | (run + rank);
        run += total;
    }
    if (!NUMBER && threadIdx.x == 0) bc[blockIdx.x] = run;
}

// grid = pages: the exclusive prefix of a page's block counts, in place, and the page's total
__global__ __launch_bounds__(256) void k_cc_scan(int32_t* counts, int stride, int nb, int32_t* totals)
{
    __shared__ int sc[256];
    int32_t* bc = counts + (size_t)stride * blockIdx.x;
    int carry = 0;
    for (int base = 0; base < nb; base += 256) {
        const int i = base + threadIdx.x, v = i < nb ? bc[i] : 0;
        sc[threadIdx.x] = v;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {
            const int add = (int)threadIdx.x >= s ? sc[threadIdx.x - s] : 0;
            __syncthreads();
            sc[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nb) bc[i] = carry + sc[threadIdx.x] - v;
        carry += sc[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// ---- statistics -------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int page_of(const int32_t* off, int n, int c)
{
    int lo = 0, hi = n - 1;   // the last page whose first component is at or before c (pages without components are passed over)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= c) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// grid = ceil(m / 256)
__global__ __launch_bounds__(256) void k_cc_stats_init(int32_t* stats, int m)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= m) return;
    int32_t* s = stats + 5 * (size_t)c;
    s[0] = INT_MAX; s[1] = 0; s[2] = -1; s[3] = -1; s[4] = 0;
}

// grid = (ceil(W H / 256), pages): components [c0, c0 + m) of the chunk
__global__ __launch_bounds__(256) void k_cc_stats(CcDev d, int c0, int m)
{
    const int p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int32_t* L = d.labels + d.plane * blockIdx.y;
    const bool in = p < d.W * d.H;
    const int y = in ? p / d.W : 0, x = in ? p - y * d.W : 0;
    int c = -1;
    bool root = false;
    if (in && d.maps.page(blockIdx.y)[(size_t)y * d.maps.step + x]) {
        const int v = L[p];
        root = (v & kCcFlag) != 0;
        const int s = root ? v : L[v];
        if (s & kCcFlag) {
            c = d.off[blockIdx.y] + (s & kCcIndex) - c0;
            if (c < 0 || c >= m) c = -1;
        }
    }
    // a run: consecutive lanes of one row with one number; its first lane speaks for it
    const int before = __shfl_up(c, 1);
    const bool brk = lane == 0 || x == 0 || before != c;
    const unsigned long long breaks = __ballot(brk);
    if (c < 0) return;
    int32_t* s = d.stats + 5 * (size_t)c;
    if (root) s[1] = y;
    if (!brk) return;
    const unsigned long long later = lane == 63 ? 0ull : breaks >> (lane + 1);
    const int len = later ? __ffsll((long long)later) : 64 - lane;
    atomicMin(&s[0], x);
    atomicMax(&s[2], x + len - 1);
    atomicMax(&s[3], y);
    atomicAdd(&s[4], len);
}

// grid = ceil(m / 256): left, top, width, height, area of every component of the pass
__global__ __launch_bounds__(256) void k_cc_stats_out(const int32_t* stats, int m, int32_t* out)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= m) return;
    const int32_t* s = stats + 5 * (size_t)c;
    int32_t* o = out + 5 * (size_t)c;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2] - s[0] + 1; o[3] = s[3] - s[1] + 1; o[4] = s[4];
}

__device__ __forceinline__ bool stat_kept(const int32_t* s) { return cc_kept(s[2] - s[0] + 1, s[3] - s[1] + 1, s[4]); }

// grid = ceil(m / 256).  WRITE = false: the block's count of kept components, and every page's; true: their rectangles
template <bool WRITE>
__global__ __launch_bounds__(256) void k_cc_kept(CcDev d, int c0, int m)
{
    __shared__ int sums[4];
    const int c = blockIdx.x * kKeptBlock + threadIdx.x;
    const int32_t* s = d.stats + 5 * (size_t)(c < m ? c : 0);
    const bool kept = c < m && stat_kept(s);
    int total;
    const int rank = block_rank(kept, sums, &total);
    if (WRITE) {
        if (!kept) return;
        int32_t* o = d.rects + 4 * (size_t)(d.kbcount[blockIdx.x] + rank);
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2] - s[0] + 1; o[3] = s[3] - s[1] + 1;
    } else {
        if (threadIdx.x == 0) d.kbcount[blockIdx.x] = total;
        if (kept) atomicAdd(&d.kept[page_of(d.off, d.n, c0 + c)], 1);
    }
}

// grid = (ceil(W / 256), H, pages)
__global__ __launch_bounds__(256) void k_cc_labels(CcDev d, uint8_t* out, size_t page_stride, size_t step)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= d.W) return;
    const int32_t* L = d.labels + d.plane * blockIdx.z;
    int id = 0;
    if (d.maps.page(blockIdx.z)[(size_t)y * d.maps.step + x]) {
        const int v = L[y * d.W + x];
        id = (((v & kCcFlag) ? v : L[v]) & kCcIndex) + 1;   // (every foreground root is numbered here)
    }
    reinterpret_cast<int32_t*>(out + page_stride * blockIdx.z + step * (size_t)y)[x] = id;
}

// ---- the workspace ----------------------------------------------------------------------------------------------------------------

size_t plane_bytes(int W, int H) { return r256((size_t)W * H * sizeof(int32_t)); }
int scan_blocks(int W, int H) { return (int)(((size_t)W * H + kScanBlock - 1) / kScanBlock); }
size_t bcount_bytes(int W, int H) { return r256((size_t)scan_blocks(W, H) * sizeof(int32_t)); }
size_t pass_stats_bytes() { return r256((size_t)cc_pass_components() * 5 * sizeof(int32_t)); }
size_t pass_rects_bytes() { return r256((size_t)cc_pass_components() * 4 * sizeof(int32_t)); }
size_t pass_kb_bytes() { return r256((((size_t)cc_pass_components() + kKeptBlock - 1) / kKeptBlock + 1) * sizeof(int32_t)); }   // the block counts and their total
size_t small_part(int n) { return r256(((size_t)n + 1) * sizeof(int32_t)); }

CcDev cc_dev(const CcRun& r)
{
    CcDev d{};
    d.maps = r.maps;
    d.W = r.W; d.H = r.H; d.n = r.n;
    d.fg8 = r.connectivity == 8;
    d.external = r.external;
    d.plane = plane_bytes(r.W, r.H) / sizeof(int32_t);
    d.nb = scan_blocks(r.W, r.H);
    d.nb_stride = (int)(bcount_bytes(r.W, r.H) / sizeof(int32_t));
    uint8_t* at = r.work;
    d.labels = reinterpret_cast<int32_t*>(at); at += plane_bytes(r.W, r.H) * (size_t)r.n;
    d.bcount = reinterpret_cast<int32_t*>(at); at += bcount_bytes(r.W, r.H) * (size_t)r.n;
    d.stats = reinterpret_cast<int32_t*>(at); at += pass_stats_bytes();
    d.rects = reinterpret_cast<int32_t*>(at); at += pass_rects_bytes();
    d.kbcount = reinterpret_cast<int32_t*>(at);
    d.count = reinterpret_cast<int32_t*>(r.small);
    d.kept = reinterpret_cast<int32_t*>(r.small + small_part(r.n));
    d.off = reinterpret_cast<int32_t*>(r.small + 2 * small_part(r.n));
    return d;
}

unsigned blocks_of(size_t items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

size_t cc_work_per_page(int W, int H) { return plane_bytes(W, H) + bcount_bytes(W, H); }
size_t cc_work_bytes(int n, int W, int H) { return cc_work_per_page(W, H) * (size_t)n + pass_stats_bytes() + pass_rects_bytes() + pass_kb_bytes(); }
size_t cc_small_bytes(int n) { return 3 * small_part(n); }
size_t cc_pinned_bytes(int n) { return 3 * small_part(n); }
int cc_pass_components() { return env_knobs().cc_pass; }
int32_t* cc_pass_rects(const CcRun& r) { return cc_dev(r).rects; }

int cc_label(const CcRun& r)
{
    const CcDev d = cc_dev(r);
    const hipStream_t hs = r.stream;
    const size_t wh = (size_t)r.W * r.H;
    const dim3 tiles(blocks_of((size_t)r.W, kT), blocks_of((size_t)r.H, kT), (unsigned)r.n);
    hipLaunchKernelGGL(k_cc_tile, tiles, dim3(256), 0, hs, d);
    hipLaunchKernelGGL(k_cc_seam, tiles, dim3(128), 0, hs, d);
    hipLaunchKernelGGL(k_cc_flatten, dim3(blocks_of(wh, 256), (unsigned)r.n), dim3(256), 0, hs, d);
    if (r.external)
        hipLaunchKernelGGL(k_cc_outer, dim3(blocks_of(2 * ((size_t)r.W + r.H), 256), (unsigned)r.n), dim3(256), 0, hs, d);
    hipLaunchKernelGGL(k_cc_count<false>, dim3((unsigned)d.nb, (unsigned)r.n), dim3(256), 0, hs, d);
    hipLaunchKernelGGL(k_cc_scan, dim3((unsigned)r.n), dim3(256), 0, hs, d.bcount, d.nb_stride, d.nb, d.count);
    hipLaunchKernelGGL(k_cc_count<true>, dim3((unsigned)d.nb, (unsigned)r.n), dim3(256), 0, hs, d);
    PRL_HIP_CHECK(hipGetLastError());
    PRL_HIP_CHECK(hipMemsetAsync(d.kept, 0, (size_t)r.n * sizeof(int32_t), hs));
    PRL_HIP_CHECK(hipMemcpyAsync(r.pinned, d.count, (size_t)r.n * sizeof(int32_t), hipMemcpyDeviceToHost, hs));
    PRL_HIP_CHECK(hipStreamSynchronize(hs));
    int32_t* h_off = r.pinned + 2 * (small_part(r.n) / sizeof(int32_t));
    long long sum = 0;
    for (int i = 0; i < r.n; ++i) {
        h_off[i] = (int32_t)sum;
        sum += r.pinned[i];
    }
    if (sum > INT_MAX) {   // more components than a chunk's numbering holds (at least 2^32 pixels in one chunk): refused, whoever cut the chunk
        set_error_detail("components: too many components in a chunk");
        return PRL_ERR_BAD_ARG;
    }
    h_off[r.n] = (int32_t)sum;
    PRL_HIP_CHECK(hipMemcpyAsync(d.off, h_off, ((size_t)r.n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, hs));
    return PRL_OK;
}

int cc_stats_pass(const CcRun& r, int c0, int m, int32_t* d_stats)
{
    if (m <= 0) return PRL_OK;
    const CcDev d = cc_dev(r);
    const hipStream_t hs = r.stream;
    const unsigned cb = blocks_of((size_t)m, 256);
    hipLaunchKernelGGL(k_cc_stats_init, dim3(cb), dim3(256), 0, hs, d.stats, m);
    hipLaunchKernelGGL(k_cc_stats, dim3(blocks_of((size_t)r.W * r.H, 256), (unsigned)r.n), dim3(256), 0, hs, d, c0, m);
    if (d_stats) {
        hipLaunchKernelGGL(k_cc_stats_out, dim3(cb), dim3(256), 0, hs, d.stats, m, d_stats);
    } else {
        hipLaunchKernelGGL(k_cc_kept<false>, dim3(cb), dim3(256), 0, hs, d, c0, m);
        hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(256), 0, hs, d.kbcount, 0, (int)cb, d.kbcount + cb);
        hipLaunchKernelGGL(k_cc_kept<true>, dim3(cb), dim3(256), 0, hs, d, c0, m);
    }
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

int cc_read_kept(const CcRun& r)
{
    const CcDev d = cc_dev(r);
    PRL_HIP_CHECK(hipMemcpyAsync(r.pinned + r.n, d.kept, (size_t)r.n * sizeof(int32_t), hipMemcpyDeviceToHost, r.stream));
    PRL_HIP_CHECK(hipStreamSynchronize(r.stream));
    return PRL_OK;
}

int cc_write_labels(const CcRun& r, int32_t* d_labels, size_t page_stride, size_t step)
{
    const CcDev d = cc_dev(r);
    hipLaunchKernelGGL(k_cc_labels, dim3(blocks_of((size_t)r.W, 256), (unsigned)r.H, (unsigned)r.n), dim3(256), 0, r.stream, d,
                       reinterpret_cast<uint8_t*>(d_labels), page_stride, step);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

}  // namespace prl_hip

using namespace prl_hip;

namespace {

int cc_map_checks(const PageArgs& a)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if ((st = pages_rows_ok(a, 1, 0, true)) != PRL_OK) return st;
    return pages_sides_ok(a);   // (32768 x 32768 = 2^30 pixels: an index fits the label word's 30 bits)
}
static_assert((long long)kStageMaxSide * kStageMaxSide - 1 <= kCcIndex, "a page's last index must fit the label word");

// the chunk of pages [first, first + cnt) on w's blocks
CcRun cc_run_of(const PageArgs& a, int first, int cnt, int connectivity, bool external, const WorkScope& w)
{
    CcRun r;
    r.maps = src_pages(a, first);
    r.n = cnt; r.W = a.width; r.H = a.height;
    r.connectivity = connectivity;
    r.external = external;
    r.work = w.scratch();
    r.small = w.small();
    r.pinned = w.pinned<int32_t>();
    r.stream = w.stream;
    return r;
}

// pages per chunk by the workspace budget (a grid's page dimension holds any chunk: stage_chunk caps it at 65535)
int cc_chunk(const PageArgs& a) { return stage_chunk(a.n_pages, cc_work_per_page(a.width, a.height)); }

}  // namespace

extern "C" {

int prl_hip_connected_components_batch_device(int n_pages, int connectivity, const uint8_t* d_map, size_t map_page_stride, size_t map_step,
                                              int width, int height, int32_t* d_labels, size_t labels_page_stride, size_t labels_step,
                                              int32_t* n_components, int32_t* d_stats, int max_components, void* stream)
{
    const PageArgs a{n_pages, d_map, map_page_stride, map_step, width, height, nullptr, 0, 0};
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if (connectivity != 4 && connectivity != 8) return PRL_ERR_BAD_ARG;
    if ((st = cc_map_checks(a)) != PRL_OK) return st;
    if (!n_components || max_components < 0 || (max_components > 0 && !d_stats)) return PRL_ERR_BAD_ARG;
    if (d_labels && (labels_step < (size_t)width * sizeof(int32_t) || ((size_t)d_labels | labels_step | labels_page_stride) % sizeof(int32_t)))
        return PRL_ERR_BAD_ARG;
    if (n_pages == 0) return PRL_OK;
    const int chunk = cc_chunk(a), pass = cc_pass_components();
    WorkScope w;
    if ((st = w.open(stream, cc_work_bytes(chunk, width, height), cc_small_bytes(chunk), cc_pinned_bytes(chunk))) != PRL_OK) return st;
    DrainOnExit drain{w.stream};   // the counts are host values, and the pinned block is free when the call returns
    long long total = 0;   // components of the pages so far
    for (int first = 0; first < n_pages; first += chunk) {
        const int cnt = std::min(chunk, n_pages - first);
        const CcRun r = cc_run_of(a, first, cnt, connectivity, false, w);
        if ((st = cc_label(r)) != PRL_OK) return st;
        int in_chunk = 0;
        for (int i = 0; i < cnt; ++i) in_chunk += (n_components[first + i] = r.pinned[i]);
        if (d_labels && (st = cc_write_labels(r, reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(d_labels) + labels_page_stride * (size_t)first),
                                              labels_page_stride, labels_step)) != PRL_OK)
            return st;
        if (d_stats && total + in_chunk <= max_components)
            for (int c0 = 0; c0 < in_chunk; c0 += pass)
                if ((st = cc_stats_pass(r, c0, std::min(pass, in_chunk - c0), d_stats + 5 * (size_t)(total + c0))) != PRL_OK) return st;
        total += in_chunk;
        PRL_HIP_CHECK(hipStreamSynchronize(w.stream));   // (the next chunk reuses the planes and the pinned counts)
    }
    return PRL_OK;
}

int prl_hip_external_rects_batch_device(int n_pages, const uint8_t* d_map, size_t map_page_stride, size_t map_step, int width, int height,
                                        int32_t* d_rects, int max_rects, int32_t* rect_offsets, int32_t* n_found, int32_t* n_kept,
                                        void* stream)
{
    const PageArgs a{n_pages, d_map, map_page_stride, map_step, width, height, nullptr, 0, 0};
    int st = cc_map_checks(a);
    if (st != PRL_OK) return st;
    if (!rect_offsets || !n_found || !n_kept || max_rects < 0 || (max_rects > 0 && !d_rects)) return PRL_ERR_BAD_ARG;
    rect_offsets[0] = 0;
    if (n_pages == 0) return PRL_OK;
    const int chunk = cc_chunk(a), pass = cc_pass_components();
    WorkScope w;
    if ((st = w.open(stream, cc_work_bytes(chunk, width, height), cc_small_bytes(chunk), cc_pinned_bytes(chunk))) != PRL_OK) return st;
    DrainOnExit drain{w.stream};   // the counts are host values, and the pinned block is free when the call returns
    // One sweep over the chunks and their passes; `write`: a pass's rectangles go to d_rects behind those of the passes before.
    // Returns how many statistics passes it ran.
    int passes = 0;
    std::vector<int32_t> seen;   // the kept counts of the chunk's pages at the previous read
    auto sweep = [&](bool write) -> int {
        long long base = 0;
        passes = 0;
        for (int first = 0; first < n_pages; first += chunk) {
            const int cnt = std::min(chunk, n_pages - first);
            const CcRun r = cc_run_of(a, first, cnt, 8, true, w);
            int s = cc_label(r);
            if (s != PRL_OK) return s;
            int in_chunk = 0;
            for (int i = 0; i < cnt; ++i) in_chunk += (n_found[first + i] = r.pinned[i]);
            seen.assign((size_t)cnt, 0);
            for (int i = 0; i < cnt; ++i) n_kept[first + i] = 0;
            for (int c0 = 0; c0 < in_chunk; c0 += pass, ++passes) {
                if ((s = cc_stats_pass(r, c0, std::min(pass, in_chunk - c0), nullptr)) != PRL_OK) return s;
                if ((s = cc_read_kept(r)) != PRL_OK) return s;
                int kept_pass = 0;
                for (int i = 0; i < cnt; ++i) {
                    kept_pass += r.pinned[cnt + i] - seen[(size_t)i];
                    n_kept[first + i] = seen[(size_t)i] = r.pinned[cnt + i];
                }
                if (write && kept_pass) {
                    // (in stream order before the next pass overwrites the pass's block)
                    PRL_HIP_CHECK(hipMemcpyAsync(d_rects + 4 * base, cc_pass_rects(r), (size_t)kept_pass * 16, hipMemcpyDeviceToDevice, w.stream));
                }
                base += kept_pass;
            }
        }
        return PRL_OK;
    };
    // With one pass in all, its rectangles are still in the workspace when the counts are known; otherwise the sweep runs twice.
    const bool one = n_pages <= chunk;
    if ((st = sweep(false)) != PRL_OK) return st;
    long long sum = 0;
    for (int i = 0; i < n_pages; ++i) {
        sum += n_kept[i];
        if (sum > INT_MAX) return PRL_ERR_BAD_ARG;
        rect_offsets[i + 1] = (int32_t)sum;
    }
    if (sum == 0 || sum > max_rects) return PRL_OK;   // the counts alone: call again with room
    if (one && passes == 1) {
        const CcRun r = cc_run_of(a, 0, n_pages, 8, true, w);
        PRL_HIP_CHECK(hipMemcpyAsync(d_rects, cc_pass_rects(r), (size_t)sum * 16, hipMemcpyDeviceToDevice, w.stream));
        return PRL_OK;
    }
    return sweep(true);
}

}  // extern "C"
