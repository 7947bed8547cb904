// ppht.hip — cv::HoughLinesP on pages resident in device memory, and prl::findAngle on top of it.
//
// Reference: src/deskew/deskew.cpp:139-205 (findAngle = bitwise_not, cv::HoughLinesP(1, CV_PI/180, 100, width/8.f, 20), angle
// vote), :224 (the Otsu threshold prl::deskew applies first).  OpenCV's arithmetic [upstream] is restated with citations in the
// test oracle (oracle/, deskew file); the kernels below reproduce it bit for bit:
//
//   k_hist / k_otsu      256-bin histogram (LDS-privatised) and getThreshVal_Otsu_8u's float64 scan, one thread per page
//   k_dark_mask          mask = (p <= thr) (the bitwise_not of the thresholded page, as 0/1 bytes = HoughLinesP's own
//                        `mask` matrix) + the number of set pixels per row
//   k_row_offsets        exclusive scan of the row counts (one workgroup per page) -> where each row's points start
//   k_collect            HoughLinesP stage 1: the non-zero points in raster order, packed x | y << 16
//   k_ppht               HoughLinesP stage 2, ONE WAVEFRONT PER PAGE.  The progressive probabilistic Hough transform is
//                        sequential by construction (every random point votes into the accumulator the previous points
//                        left, and a detected line erases points and takes their votes back), so a page cannot be split;
//                        the batch dimension supplies the parallelism (1024 pages = one wavefront per SIMD).  Inside a
//                        page the 180 angles of a vote are spread over the lanes (3 per lane, `global_atomic_add` with
//                        return, owner-lane rows), the maximum is a wavefront reduction, and the two line walks test 64
//                        steps per memory round trip (ballot + scalar run-length scan) instead of one.  cv::RNG's
//                        multiply-with-carry sequence is reproduced exactly, so the segments - and therefore the angle -
//                        are those OpenCV finds.  Latency-bound by design: ~3 dependent L2/HBM round trips per point.
//   k_ppht_mw            the same with three wavefronts per page (below)
//   host                 atan2 + first-fit clustering of deskew.cpp:158-201 (host libm, as in the reference)
// The pages that qualify go to the group kernel of ppht_group.hip (accumulator in LDS); k_ppht_mw / k_ppht take the rest.  The
// driver (ppht_pages) is a sequence of five phases over one description of the pass (Search); its sizes come from ppht_plan.h.
#include <algorithm>
#include <climits>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ppht_plan.h"
#include "prl_device_math.h"
#include "prl_internal.h"

namespace prl_hip {
namespace {

// ---- Otsu --------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_hist(PageSet src, int width, int height, unsigned* __restrict__ hist)
{
    __shared__ unsigned h[256];
    const int page = blockIdx.z, t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const uint8_t* base = src.page(page);
    for (int y = blockIdx.y; y < height; y += gridDim.y) {
        const uint8_t* row = base + (size_t)y * src.step;
        for (int x = (blockIdx.x * 256 + t) * 4; x < width; x += gridDim.x * 1024) {
            const int n = min(4, width - x);
            for (int i = 0; i < n; ++i) atomicAdd(&h[row[x + i]], 1u);
        }
    }
    __syncthreads();
    if (h[t]) atomicAdd(&hist[(size_t)page * 256 + t], h[t]);
}

// getThreshVal_Otsu_8u [upstream]: the float64 scan over the 256 bins, one thread per page.
__global__ void k_otsu(const unsigned* __restrict__ hist, int width, int height, int n_pages, int* __restrict__ thr)
{
    const int page = blockIdx.x * blockDim.x + threadIdx.x;
    if (page >= n_pages) return;
    thr[page] = otsu_scan(hist + (size_t)page * 256, 1. / ((double)width * height));   // (prl_device_math.h)
}

// ---- HoughLinesP stage 1 -------------------------------------------------------------------------------------------

// one wavefront per row: mask byte = (p <= thr), row_count = number of set pixels
__global__ void __launch_bounds__(64) k_dark_mask(PageSet src, int width, int height, const int* __restrict__ thr,
                                                  uint8_t* __restrict__ mask, size_t mask_page, unsigned* __restrict__ row_count)
{
    const int page = blockIdx.y, y = blockIdx.x, lane = threadIdx.x;
    const uint8_t* row = src.page(page) + (size_t)y * src.step;
    uint8_t* m = mask + (size_t)page * mask_page + (size_t)y * width;
    const int t = thr[page];
    unsigned cnt = 0;
    for (int x = lane; x < width; x += 64) {
        const uint8_t v = row[x] <= t;
        m[x] = v;
        cnt += v;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) row_count[(size_t)page * height + y] = cnt;
}

// one workgroup per page: row_off[y] = sum of row_count[0..y), count[page] = total
__global__ void __launch_bounds__(256) k_row_offsets(int height, const unsigned* __restrict__ row_count,
                                                     unsigned* __restrict__ row_off, unsigned* __restrict__ count)
{
    __shared__ unsigned part[256];
    const int page = blockIdx.x, t = threadIdx.x;
    const unsigned* rc = row_count + (size_t)page * height;
    unsigned* ro = row_off + (size_t)page * height;
    const int per = (height + 255) / 256, y0 = t * per, y1 = min(height, y0 + per);
    unsigned s = 0;
    for (int y = y0; y < y1; ++y) s += rc[y];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        unsigned run = 0;
        for (int i = 0; i < 256; ++i) {
            const unsigned v = part[i];
            part[i] = run;
            run += v;
        }
        count[page] = run;
    }
    __syncthreads();
    unsigned run = part[t];
    for (int y = y0; y < y1; ++y) {
        ro[y] = run;
        run += rc[y];
    }
}

// one wavefront per row: the row's set pixels, in x order, to nz[nz_off[page] + row_off[y] ...]
__global__ void __launch_bounds__(64) k_collect(int width, int height, const uint8_t* __restrict__ mask, size_t mask_page,
                                                const unsigned* __restrict__ row_off, const unsigned long long* __restrict__ nz_off,
                                                unsigned* __restrict__ nz)
{
    const int page = blockIdx.y, y = blockIdx.x, lane = threadIdx.x;
    const uint8_t* m = mask + (size_t)page * mask_page + (size_t)y * width;
    unsigned* out = nz + nz_off[page] + row_off[(size_t)page * height + y];
    unsigned base = 0;
    for (int x0 = 0; x0 < width; x0 += 64) {
        const int x = x0 + lane;
        const bool set = x < width && m[x] != 0;
        const unsigned long long b = __ballot(set);
        if (set) out[base + __popcll(b & ((1ull << lane) - 1))] = (unsigned)x | ((unsigned)y << 16);
        base += __popcll(b);
    }
}

// ---- HoughLinesP stage 2 -------------------------------------------------------------------------------------------

struct PphtArgs {
    int width, height, numrho, threshold, line_length, line_gap;
    uint8_t* mask; size_t mask_page;
    unsigned* nz; const unsigned long long* nz_off; const unsigned* count;
    int* accum;                 // per page kNumAngle * numrho, zeroed
    const float* ttab;          // kNumAngle x {cos, sin}
    int* lines; const unsigned long long* lines_off; const unsigned* lines_cap; unsigned* n_lines;
    int prio;                   // raise the wavefront priority (PRL_HIP_PPHT_PRIO)
    const int* page_list;       // workgroup b takes page page_list[b], its accumulator is the b-th (null: page b)
    unsigned long long* prof;   // hooks build, PRL_HIP_PPHT_PROF=1: 16 counters per page (cycles per phase, event counts); else null
};

// Phase accounting of k_ppht_mw (hooks build only: the product kernel carries none of it).  Wavefront 0 / lane 0 adds the
// shader-clock cycles since the previous mark to the phase that just ended.
#ifdef PRL_TEST_HOOKS
#define PPHT_MARK(slot)                                                                  \
    do {                                                                                 \
        if (a.prof && wv == 0) {                                                         \
            const unsigned long long now_ = __builtin_readcyclecounter();                \
            if (lane == 0) a.prof[(size_t)page * 16 + (slot)] += now_ - prof_t;          \
            prof_t = now_;                                                               \
        }                                                                                \
    } while (0)
#define PPHT_COUNT(slot, n)                                                              \
    do {                                                                                 \
        if (a.prof && wv == 0 && lane == 0) a.prof[(size_t)page * 16 + (slot)] += (n);   \
    } while (0)
#else
#define PPHT_MARK(slot) do { } while (0)
#define PPHT_COUNT(slot, n) do { } while (0)
#endif

__device__ __forceinline__ int cv_round_f(float v) { return __float2int_rn(v); }

__device__ __forceinline__ unsigned uni(unsigned v) { return __builtin_amdgcn_readfirstlane(v); }

// Steps [0, ...) of a walk x += dx, y += dy from (x0, y0): pixel of step s.
__device__ __forceinline__ void step_pixel(int xflag, unsigned x0, unsigned y0, int dx, int dy, unsigned s, int* j1, int* i1)
{
    const int x = (int)(x0 + s * (unsigned)dx), y = (int)(y0 + s * (unsigned)dy);  // wraps like the reference's repeated adds
    if (xflag) { *j1 = x; *i1 = y >> 16; }
    else { *j1 = x >> 16; *i1 = y; }
}

// max over the 64 lanes of a signed value (DPP row shifts + row broadcasts; the result is uniform)
__device__ __forceinline__ int wave_max_i32(int x)
{
    x = max(x, __builtin_amdgcn_update_dpp(INT_MIN, x, 0x111, 0xf, 0xf, false));  // row_shr:1
    x = max(x, __builtin_amdgcn_update_dpp(INT_MIN, x, 0x112, 0xf, 0xf, false));  // row_shr:2
    x = max(x, __builtin_amdgcn_update_dpp(INT_MIN, x, 0x114, 0xf, 0xf, false));  // row_shr:4
    x = max(x, __builtin_amdgcn_update_dpp(INT_MIN, x, 0x118, 0xf, 0xf, false));  // row_shr:8
    x = max(x, __builtin_amdgcn_update_dpp(INT_MIN, x, 0x142, 0xa, 0xf, false));  // row_bcast:15 -> rows 1, 3
    x = max(x, __builtin_amdgcn_update_dpp(INT_MIN, x, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> rows 2, 3
    return __builtin_amdgcn_readlane(x, 63);
}

#ifndef PRL_PPHT_BLK
#define PRL_PPHT_BLK 32
#endif
// Points per block of k_ppht.  32: 96 returned counts in registers (136 VGPRs); 64 (234 VGPRs) measured 3 % slower on 256+
// pages - the batch keeps the memory system busy either way - and 24 / 16 the same as 32 (profiles/r02/chain_overlap.txt).
constexpr int kBlk = PRL_PPHT_BLK;

// A vote.  A lane is the only one that ever touches its cells, but a narrower scope buys nothing: wavefront, workgroup and agent
// scope compile to the same `global_atomic_add ... sc0`; where it executes is decided by the memory type (hipMalloc: behind the
// L2s, profiles/r02/pmc_ppht.txt).
__device__ __forceinline__ int vote(int* cell, int d) { return __hip_atomic_fetch_add(cell, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Cells hold count + 2^31 (the accumulator is filled with 0x80000000): a vote's returned value gives the count by flipping the top
// bit, and the un-votes of a good line can be taken from TWO adjacent cells with one 64-bit subtraction - the low half never
// borrows from the high one, because a biased cell is never smaller than what is subtracted from it.
constexpr unsigned kAccBias = 0x80000000u;
static_assert(kNumAngle % 2 == 0, "a page's accumulator must be a whole number of 8-byte cell pairs (Unvotes)");
__device__ __forceinline__ int count_of(int stored) { return (int)((unsigned)stored ^ kAccBias); }

// The un-votes of one lane's angle along a line walk.  For a fixed angle the cell index r = round(x cos + y sin) is monotone
// along the walk and moves by at most sqrt(2) per step, so consecutive erased pixels hit the same cell or its neighbour: the
// decrements are collected per aligned PAIR of cells and leave as one global_atomic_sub_x2 when the walk moves on - about a
// third of the atomics of one decrement per pixel and angle (the transform is bound by the rate of memory-side atomics:
// 2.1e10 per second for the whole chip), with identical cell values at every later vote.
struct Unvotes {
    int pair = -1;
    unsigned lo = 0, hi = 0;
    __device__ __forceinline__ void flush(unsigned long long* acc64)
    {
        if (pair >= 0)
            (void)__hip_atomic_fetch_sub(acc64 + pair, (unsigned long long)lo | ((unsigned long long)hi << 32), __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
        pair = -1;
        lo = hi = 0;
    }
    __device__ __forceinline__ void add(unsigned long long* acc64, int idx)   // idx: cell index from the page's accumulator base
    {
        const int p = idx >> 1;
        if (p != pair) {
            flush(acc64);
            pair = p;
        }
        if (idx & 1) ++hi;
        else ++lo;
    }
};

// HoughLinesP stage 2, one wavefront per page, BLOCKS OF kBlk POINTS (round 2, second version).  The first version walked the
// points one by one: list fetch -> mask byte -> 180 voting atomics -> decision, three dependent memory round trips per
// point (1.9 us).  Two facts allow overlapping them without changing a single result:
//  * the visiting order does not depend on the data (cv::RNG draws idx_t = next() % (N - t) and the list swap
//    nz[idx_t] = nz[N - t - 1] happens whatever the point does), so kBlk steps of it are taken at once: lane L fetches the list
//    entries of step t0 + L, and the swaps of the earlier steps of the same block are applied to its values in registers
//    (a kBlk-step loop of readlane / compare / select), duplicates resolved so that memory ends in the sequential state;
//  * a vote only matters when its cell reaches the threshold, which a fraction of a percent of the points do: the votes of
//    all points of the block are ISSUED back to back (atomics with return into 3 kBlk registers; a lane owns its angles' rows, so
//    successive points hitting one cell arrive in order) and then RETIRED in order; the first point that triggers a line has
//    the votes of the younger points taken back, its line is walked exactly as before, and the rest of the block starts
//    over (masks re-read: the walk may have erased some of them).
// Up to 63 vector memory instructions are in flight per wavefront (the vmcnt counter), i.e. about 21 points.
__global__ void __launch_bounds__(64) k_ppht(PphtArgs a)
{
    // One latency-bound wavefront per page that issues little: in the chain it shares its SIMD with the NL-means wavefronts of
    // the previous pass (glue.hip), which saturate the vector ALU - let the arbiter pick this one first.
    if (a.prio) __builtin_amdgcn_s_setprio(3);
    const int page = a.page_list ? a.page_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    const int W = a.width, H = a.height, numrho = a.numrho;
    volatile uint8_t* mask = a.mask + (size_t)page * a.mask_page;
    volatile unsigned* nz = a.nz + a.nz_off[page];
    int* accum = a.accum + (size_t)blockIdx.x * kNumAngle * numrho;
    int* lines = a.lines + a.lines_off[page] * 4;
    const unsigned cap = a.lines_cap[page];
    float tc[3], ts[3];
    int* arow[3];
    int row0[3];   // index of cell r = 0 of the lane's three angle rows
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int n = min(lane + 64 * q, kNumAngle - 1);
        tc[q] = a.ttab[2 * n];
        ts[q] = a.ttab[2 * n + 1];
        arow[q] = accum + (size_t)n * numrho + (numrho - 1) / 2;
        row0[q] = n * numrho + (numrho - 1) / 2;
    }
    unsigned long long* acc64 = reinterpret_cast<unsigned long long*>(accum);
    const bool has2 = lane + 128 < kNumAngle;
    unsigned long long rng = ~0ull;
    unsigned n_lines = 0;
    const unsigned N = a.count[page];

    // One detected line: walk both ways from (j, i) along angle max_n, clear the mask, take votes back (as the first version).
    auto process_line = [&](int j, int i, int max_n) {
        const float fa = -a.ttab[2 * max_n + 1], fb = a.ttab[2 * max_n];
        unsigned x0 = (unsigned)j, y0 = (unsigned)i;
        int dx0, dy0, xflag;
        if (fabs((double)fa) > fabs((double)fb)) {
            xflag = 1;
            dx0 = fa > 0 ? 1 : -1;
            dy0 = __double2int_rn((double)(fb * 65536.f) / fabs((double)fa));
            y0 = (y0 << 16) + (1u << 15);
        } else {
            xflag = 0;
            dy0 = fb > 0 ? 1 : -1;
            dx0 = __double2int_rn((double)(fa * 65536.f) / fabs((double)fb));
            x0 = (x0 << 16) + (1u << 15);
        }
        // first walk, both directions: the step of the last set pixel before the border or a gap above line_gap
        unsigned end_step[2];
        for (int k = 0; k < 2; ++k) {
            const int dx = k ? -dx0 : dx0, dy = k ? -dy0 : dy0;
            unsigned endk = 0;
            int gap = 0;  // consecutive cleared pixels so far
            bool stop = false;
            for (unsigned base = 0; !stop; base += 64) {
                int j1, i1;
                step_pixel(xflag, x0, y0, dx, dy, base + lane, &j1, &i1);
                const bool inb = j1 >= 0 && j1 < W && i1 >= 0 && i1 < H;
                const bool set = inb && mask[(size_t)i1 * W + j1] != 0;
                const unsigned long long oob = __ballot(!inb);
                unsigned long long nzb = __ballot(set);
                const int limit = oob ? __ffsll((long long)oob) - 1 : 64;  // steps [0, limit) are inside the image
                int prev = -1 - gap;                                        // position of the last set pixel (virtual)
                while (nzb) {
                    const int q = __ffsll((long long)nzb) - 1;
                    nzb &= nzb - 1;
                    if (q >= limit || q - prev - 1 > a.line_gap) { stop = true; break; }
                    endk = base + (unsigned)q;
                    prev = q;
                }
                if (!stop) {
                    if (limit - 1 - prev > a.line_gap || limit < 64) stop = true;
                    else gap = 63 - prev;
                }
            }
            end_step[k] = endk;
        }
        int ex[2], ey[2];
        step_pixel(xflag, x0, y0, dx0, dy0, end_step[0], &ex[0], &ey[0]);
        step_pixel(xflag, x0, y0, -dx0, -dy0, end_step[1], &ex[1], &ey[1]);
        const bool good_line = abs(ex[1] - ex[0]) >= a.line_length || abs(ey[1] - ey[0]) >= a.line_length;
        // second walk: clear the set pixels up to the line ends; a good line takes their votes back
        Unvotes uv[3];
        for (int k = 0; k < 2; ++k) {
            const int dx = k ? -dx0 : dx0, dy = k ? -dy0 : dy0;
            for (unsigned base = (unsigned)k; base <= end_step[k]; base += 64) {  // (step 0 was cleared by k = 0)
                const unsigned st = base + lane;
                int j1, i1;
                step_pixel(xflag, x0, y0, dx, dy, st, &j1, &i1);
                bool set = false;
                if (st <= end_step[k]) {
                    set = mask[(size_t)i1 * W + j1] != 0;
                    if (set) mask[(size_t)i1 * W + j1] = 0;
                }
                unsigned long long nzb = __ballot(set);
                if (good_line) {
                    while (nzb) {
                        const int q = __ffsll((long long)nzb) - 1;
                        nzb &= nzb - 1;
                        int jq, iq;
                        step_pixel(xflag, x0, y0, dx, dy, base + (unsigned)q, &jq, &iq);
#pragma unroll
                        for (int qq = 0; qq < 3; ++qq)
                            if (qq < 2 || has2) uv[qq].add(acc64, row0[qq] + cv_round_f((float)jq * tc[qq] + (float)iq * ts[qq]));
                    }
                }
            }
        }
#pragma unroll
        for (int qq = 0; qq < 3; ++qq) uv[qq].flush(acc64);   // before any later vote reads these cells
        if (good_line) {
            if (lane == 0 && n_lines < cap) {
                lines[4 * n_lines] = ex[0];
                lines[4 * n_lines + 1] = ey[0];
                lines[4 * n_lines + 2] = ex[1];
                lines[4 * n_lines + 3] = ey[1];
            }
            ++n_lines;
        }
    };

    for (unsigned t0 = 0; t0 < N; t0 += kBlk) {
        const unsigned nb = min((unsigned)kBlk, N - t0), c0 = N - t0;
        // the next nb outputs of cv::RNG, one per lane
        unsigned rv = 0;
        for (unsigned L = 0; L < nb; ++L) {
            rng = (unsigned long long)(unsigned)rng * 4164903690ull + (rng >> 32);
            if ((unsigned)lane == L) rv = (unsigned)rng;
        }
        const bool act = (unsigned)lane < nb;
        const unsigned cnt_l = act ? c0 - (unsigned)lane : 1u;  // list length at this lane's step
        const unsigned idx = rv % cnt_l, lastpos = cnt_l - 1u;
        unsigned rp = 0, rl = 0;
        if (act) {
            rp = nz[idx];
            rl = nz[lastpos];
        }
        // swaps of the earlier steps of this block, applied in registers; `skip`: steps whose slot a later step writes again
        unsigned long long skip = 0;
        for (unsigned st = 0; st + 1 < nb; ++st) {
            const unsigned is = (unsigned)__builtin_amdgcn_readlane((int)idx, (int)st);
            const unsigned ls = (unsigned)__builtin_amdgcn_readlane((int)rl, (int)st);
            const bool later = act && (unsigned)lane > st;
            const bool c1 = later && idx == is, c2 = later && lastpos == is;
            if (c1) rp = ls;
            if (c2) rl = ls;
            if (__ballot(c1)) skip |= 1ull << st;
        }
        if (act && !((skip >> lane) & 1ull)) nz[idx] = rl;   // memory ends in the sequential state
        const unsigned pt = rp;                               // this lane's point: x | y << 16

        unsigned start = 0;
        while (start < nb) {
            // mask bytes of the points not yet retired (a line walked meanwhile may have erased some)
            unsigned m = 0;
            if (act && (unsigned)lane >= start) m = mask[(size_t)(pt >> 16) * W + (pt & 0xffffu)];
            const unsigned long long vm = __ballot(m != 0);
            if (!vm) break;
            // issue: every point's votes, back to back; v[p][q] = the count before this vote
            int v[kBlk][3];
#pragma unroll
            for (int p = 0; p < kBlk; ++p) {
                if ((vm >> p) & 1ull) {
                    const unsigned q = (unsigned)__builtin_amdgcn_readlane((int)pt, p);
                    const float fj = (float)(q & 0xffffu), fi = (float)(q >> 16);
#pragma unroll
                    for (int qq = 0; qq < 3; ++qq)
                        if (qq < 2 || has2) v[p][qq] = vote(arow[qq] + cv_round_f(fj * tc[qq] + fi * ts[qq]), 1);
                }
            }
            // retire in order: key = count * 256 + (255 - angle), signed (counts go negative: a good line takes back the votes
            // of points that have not voted yet, as in the reference): the largest count, the first angle among equals
            int trig = -1, trig_n = 0;
#pragma unroll
            for (int p = 0; p < kBlk; ++p) {
                if (((vm >> p) & 1ull) && trig < 0) {
                    int key = INT_MIN;
#pragma unroll
                    for (int qq = 0; qq < 3; ++qq)
                        if (qq < 2 || has2) key = max(key, (count_of(v[p][qq]) + 1) * 256 + (255 - (lane + 64 * qq)));
                    key = wave_max_i32(key);
                    if ((key >> 8) >= a.threshold) {
                        trig = p;
                        trig_n = 255 - (key & 255);
                    }
                }
            }
            if (trig < 0) break;  // every vote of the block stands
            // the younger points voted on speculation: take their votes back, walk the line, start over behind it
            for (unsigned p = (unsigned)trig + 1; p < nb; ++p) {
                if ((vm >> p) & 1ull) {
                    const unsigned q = (unsigned)__builtin_amdgcn_readlane((int)pt, (int)p);
                    const float fj = (float)(q & 0xffffu), fi = (float)(q >> 16);
#pragma unroll
                    for (int qq = 0; qq < 3; ++qq)
                        if (qq < 2 || has2) vote(arow[qq] + cv_round_f(fj * tc[qq] + fi * ts[qq]), -1);
                }
            }
            const unsigned tq = (unsigned)__builtin_amdgcn_readlane((int)pt, trig);
            process_line((int)(tq & 0xffffu), (int)(tq >> 16), trig_n);
            start = (unsigned)trig + 1;
        }
    }
    if (lane == 0) a.n_lines[page] = n_lines;
}

// The same transform with THREE wavefronts per page (small batches: a single wavefront per page is bound by its own memory
// round trips - 0.7 s for an A4 page whatever the batch size up to ~64 pages - while the chip idles).  Wavefront v, lane l
// owns angle 64 v + l: a point's 180 votes are one instruction per wavefront, a block's votes are all in flight at once, and
// un-votes and roll-backs split three ways.  Everything that decides the visiting order (cv::RNG, the list swaps, the masks)
// is computed by all three wavefronts identically; what WRITES shared state is done by wavefront 0 alone (list stores, mask
// clearing, the segment list) and handed on through LDS / a barrier: the per-point maxima (keys, double-buffered), the set
// pixels of the clearing walk (one ballot per 64 steps).  Results are identical to k_ppht's by construction and by
// tests/test_deskew_gpu.py, which runs its cases through both kernels (PRL_HIP_PPHT_MW=0 in a child process).
constexpr int kMwWaves = 3;
#ifndef PRL_PPHT_BLK_MW
#define PRL_PPHT_BLK_MW 32
#endif
constexpr int kBlkMw = PRL_PPHT_BLK_MW;
constexpr int kPphtMwMaxPages = 1 << 30;   // never slower than one wavefront per page (1 .. 512 pages measured: DESIGN.md 4.10)
constexpr int kMwMaxGroups = 2 * (32768 / 64 + 2);
__global__ void __launch_bounds__(64 * kMwWaves) k_ppht_mw(PphtArgs a)
{
    __shared__ int s_keys[2][kMwWaves][kBlkMw];
    __shared__ unsigned long long s_ballot[kMwMaxGroups];
    if (a.prio) __builtin_amdgcn_s_setprio(3);
    const int page = a.page_list ? a.page_list[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int W = a.width, H = a.height, numrho = a.numrho;
    volatile uint8_t* mask = a.mask + (size_t)page * a.mask_page;
    volatile unsigned* nz = a.nz + a.nz_off[page];
    int* accum = a.accum + (size_t)blockIdx.x * kNumAngle * numrho;
    int* lines = a.lines + a.lines_off[page] * 4;
    const unsigned cap = a.lines_cap[page];
    const int ang = wv * 64 + lane;
    const bool has = ang < kNumAngle;
    const int angc = min(ang, kNumAngle - 1);
    const float tc = a.ttab[2 * angc], ts = a.ttab[2 * angc + 1];
    int* arow = accum + (size_t)angc * numrho + (numrho - 1) / 2;
    const int row0 = angc * numrho + (numrho - 1) / 2;   // index of this lane's cell r = 0
    unsigned long long* acc64 = reinterpret_cast<unsigned long long*>(accum);
    unsigned long long rng = ~0ull;
    unsigned n_lines = 0;
    const unsigned N = a.count[page];
    int kbuf = 0;
#ifdef PRL_TEST_HOOKS
    unsigned long long prof_t = __builtin_readcyclecounter();
#endif

    auto process_line = [&](int j, int i, int max_n) {
        const float fa = -a.ttab[2 * max_n + 1], fb = a.ttab[2 * max_n];
        unsigned x0 = (unsigned)j, y0 = (unsigned)i;
        int dx0, dy0, xflag;
        if (fabs((double)fa) > fabs((double)fb)) {
            xflag = 1;
            dx0 = fa > 0 ? 1 : -1;
            dy0 = __double2int_rn((double)(fb * 65536.f) / fabs((double)fa));
            y0 = (y0 << 16) + (1u << 15);
        } else {
            xflag = 0;
            dy0 = fb > 0 ? 1 : -1;
            dx0 = __double2int_rn((double)(fa * 65536.f) / fabs((double)fb));
            x0 = (x0 << 16) + (1u << 15);
        }
        // first walk (read only): every wavefront for itself, the results are identical
        unsigned end_step[2];
        for (int k = 0; k < 2; ++k) {
            const int dx = k ? -dx0 : dx0, dy = k ? -dy0 : dy0;
            unsigned endk = 0;
            int gap = 0;
            bool stop = false;
            for (unsigned base = 0; !stop; base += 64) {
                int j1, i1;
                step_pixel(xflag, x0, y0, dx, dy, base + lane, &j1, &i1);
                const bool inb = j1 >= 0 && j1 < W && i1 >= 0 && i1 < H;
                const bool set = inb && mask[(size_t)i1 * W + j1] != 0;
                const unsigned long long oob = __ballot(!inb);
                unsigned long long nzb = __ballot(set);
                const int limit = oob ? __ffsll((long long)oob) - 1 : 64;
                int prev = -1 - gap;
                while (nzb) {
                    const int q = __ffsll((long long)nzb) - 1;
                    nzb &= nzb - 1;
                    if (q >= limit || q - prev - 1 > a.line_gap) { stop = true; break; }
                    endk = base + (unsigned)q;
                    prev = q;
                }
                if (!stop) {
                    if (limit - 1 - prev > a.line_gap || limit < 64) stop = true;
                    else gap = 63 - prev;
                }
            }
            end_step[k] = endk;
        }
        int ex[2], ey[2];
        step_pixel(xflag, x0, y0, dx0, dy0, end_step[0], &ex[0], &ey[0]);
        step_pixel(xflag, x0, y0, -dx0, -dy0, end_step[1], &ex[1], &ey[1]);
        const bool good_line = abs(ex[1] - ex[0]) >= a.line_length || abs(ey[1] - ey[0]) >= a.line_length;
        PPHT_MARK(3);   // read-only walk
        PPHT_COUNT(9, (end_step[0] + end_step[1]) / 64 + 2);
        __syncthreads();  // nobody clears a pixel before everybody has finished the read-only walk
        // second walk: wavefront 0 clears the set pixels and publishes which ones they were
        if (wv == 0) {
            int gidx = 0;
            for (int k = 0; k < 2; ++k) {
                const int dx = k ? -dx0 : dx0, dy = k ? -dy0 : dy0;
                for (unsigned base = (unsigned)k; base <= end_step[k]; base += 64, ++gidx) {  // (step 0 was cleared by k = 0)
                    const unsigned st = base + lane;
                    int j1, i1;
                    step_pixel(xflag, x0, y0, dx, dy, st, &j1, &i1);
                    bool set = false;
                    if (st <= end_step[k]) {
                        set = mask[(size_t)i1 * W + j1] != 0;
                        if (set) mask[(size_t)i1 * W + j1] = 0;
                    }
                    const unsigned long long nzb = __ballot(set);
                    if (lane == 0) s_ballot[gidx] = nzb;
                }
            }
        }
        __syncthreads();
        PPHT_MARK(4);   // clearing walk
        if (good_line) {  // a good line takes the votes of its pixels back: every wavefront its own angles
            Unvotes uv;
            int gidx = 0;
            for (int k = 0; k < 2; ++k) {
                const int dx = k ? -dx0 : dx0, dy = k ? -dy0 : dy0;
                for (unsigned base = (unsigned)k; base <= end_step[k]; base += 64, ++gidx) {
                    unsigned long long nzb = s_ballot[gidx];
                    PPHT_COUNT(10, __popcll(nzb));
                    while (nzb) {
                        const int q = __ffsll((long long)nzb) - 1;
                        nzb &= nzb - 1;
                        int jq, iq;
                        step_pixel(xflag, x0, y0, dx, dy, base + (unsigned)q, &jq, &iq);
                        if (has) uv.add(acc64, row0 + cv_round_f((float)jq * tc + (float)iq * ts));
                    }
                }
            }
            uv.flush(acc64);   // before any later vote reads these cells
            if (wv == 0 && lane == 0 && n_lines < cap) {
                lines[4 * n_lines] = ex[0];
                lines[4 * n_lines + 1] = ey[0];
                lines[4 * n_lines + 2] = ex[1];
                lines[4 * n_lines + 3] = ey[1];
            }
            ++n_lines;
        }
        __syncthreads();  // s_ballot is free again; the cleared pixels are visible to everybody's next mask reads
        PPHT_MARK(5);   // un-votes (+ the segment store)
        PPHT_COUNT(8, good_line ? 1 : 0);
    };

    for (unsigned t0 = 0; t0 < N; t0 += kBlkMw) {
        const unsigned nb = min((unsigned)kBlkMw, N - t0), c0 = N - t0;
        unsigned rv = 0;
        for (unsigned L = 0; L < nb; ++L) {
            rng = (unsigned long long)(unsigned)rng * 4164903690ull + (rng >> 32);
            if ((unsigned)lane == L) rv = (unsigned)rng;
        }
        const bool act = (unsigned)lane < nb;
        const unsigned cnt_l = act ? c0 - (unsigned)lane : 1u;
        const unsigned idx = rv % cnt_l, lastpos = cnt_l - 1u;
        unsigned rp = 0, rl = 0;
        if (act) {
            rp = nz[idx];
            rl = nz[lastpos];
        }
        unsigned long long skip = 0;
        for (unsigned st = 0; st + 1 < nb; ++st) {
            const unsigned is = (unsigned)__builtin_amdgcn_readlane((int)idx, (int)st);
            const unsigned ls = (unsigned)__builtin_amdgcn_readlane((int)rl, (int)st);
            const bool later = act && (unsigned)lane > st;
            const bool c1 = later && idx == is, c2 = later && lastpos == is;
            if (c1) rp = ls;
            if (c2) rl = ls;
            if (__ballot(c1)) skip |= 1ull << st;
        }
        __syncthreads();  // every wavefront has read this block's list entries before the list moves on.  All three store the
        // same values: a wavefront's own store then orders its own reads of the next block (a block without a live point has
        // no further barrier)
        if (act && !((skip >> lane) & 1ull)) nz[idx] = rl;
        const unsigned pt = rp;
        PPHT_MARK(0);   // block prologue: RNG, list fetch, swaps
        PPHT_COUNT(6, 1);

        unsigned start = 0;
        while (start < nb) {
            unsigned m = 0;
            if (act && (unsigned)lane >= start) m = mask[(size_t)(pt >> 16) * W + (pt & 0xffffu)];
            const unsigned long long vm = __ballot(m != 0);
            if (!vm) { PPHT_MARK(1); break; }
            PPHT_COUNT(11, __popcll(vm));
            int v[kBlkMw];
#pragma unroll
            for (int p = 0; p < kBlkMw; ++p) {
                if ((vm >> p) & 1ull) {
                    const unsigned q = (unsigned)__builtin_amdgcn_readlane((int)pt, p);
                    const float fj = (float)(q & 0xffffu), fi = (float)(q >> 16);
                    if (has) v[p] = vote(arow + cv_round_f(fj * tc + fi * ts), 1);
                }
            }
            // this wavefront's maximum per point into lane p, then the three of them through LDS
            int mine = INT_MIN;
#pragma unroll
            for (int p = 0; p < kBlkMw; ++p) {
                if ((vm >> p) & 1ull) {
                    const int key = wave_max_i32(has ? (count_of(v[p]) + 1) * 256 + (255 - ang) : INT_MIN);
                    if (lane == p) mine = key;
                }
            }
            if (lane < kBlkMw) s_keys[kbuf][wv][lane] = mine;
            __syncthreads();
            int kk = INT_MIN;
            if (lane < kBlkMw) {
#pragma unroll
                for (int u = 0; u < kMwWaves; ++u) kk = max(kk, s_keys[kbuf][u][lane]);
            }
            kbuf ^= 1;
            const unsigned long long tb = __ballot(lane < kBlkMw && ((vm >> lane) & 1ull) && (kk >> 8) >= a.threshold);
            PPHT_MARK(1);   // mask bytes, votes issued and retired
            if (!tb) break;  // every vote of the block stands
            PPHT_COUNT(7, 1);
            const int trig = __ffsll((long long)tb) - 1;
            const int trig_n = 255 - (__builtin_amdgcn_readlane(kk, trig) & 255);
            for (unsigned p = (unsigned)trig + 1; p < nb; ++p) {
                if ((vm >> p) & 1ull) {
                    const unsigned q = (unsigned)__builtin_amdgcn_readlane((int)pt, (int)p);
                    const float fj = (float)(q & 0xffffu), fi = (float)(q >> 16);
                    if (has) vote(arow + cv_round_f(fj * tc + fi * ts), -1);
                }
            }
            const unsigned tq = (unsigned)__builtin_amdgcn_readlane((int)pt, trig);
            PPHT_MARK(2);   // roll-back of the younger points' votes
            process_line((int)(tq & 0xffffu), (int)(tq >> 16), trig_n);
            start = (unsigned)trig + 1;
        }
    }
    if (wv == 0 && lane == 0) a.n_lines[page] = n_lines;
}

// ---- the driver ------------------------------------------------------------------------------------------------------

// One call of ppht_pages: the pass's shape and parameters, its workspace, and what the phases hand to each other.  The host
// arrays that asynchronous copies read or write live here, that is until the call returns.
struct Search {
    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    SearchStart* start = nullptr;
    int n_pages = 0, width = 0, height = 0, numrho = 0, threshold = 0, line_length = 0, line_gap = 0;
    PphtFixed fixed{};                  // the fixed workspace, ctx->ppht_buf[0]; the lists are ctx->ppht_buf[1]
    uint8_t* ws = nullptr;
    template <typename T> T* block(size_t offset) const { return reinterpret_cast<T*>(ws + offset); }
    std::vector<unsigned> h_count;      // points per page
    PphtLists lists;
    float h_ttab[kNumAngle * 2];
    PphtPass pass;
    PphtGroupIn gin;                    // the group attempt: its arguments, the status it reports per page
    std::vector<unsigned> h_status;
    std::vector<unsigned long long> h_gprof;
    std::vector<unsigned> h_nl;         // segments found per page
    unsigned long long* d_prof = nullptr;   // hooks build, PRL_HIP_PPHT_PROF=1: the phase counters of k_ppht_mw
    ~Search() { if (d_prof) (void)hipFree(d_prof); }
};

// Phase 1, thresholds and point counts: Otsu's threshold or the fixed one per page, the dark mask with its row counts, their
// scan.  Leaves masks, row offsets and counts in the fixed workspace and the counts in s.h_count.  Synchronises.
int search_points(Search& s, const PageSet& gray, bool otsu, int fixed_thr)
{
    const int n = s.n_pages, W = s.width, H = s.height;
    int st = ensure_buffer(&s.ctx->ppht_buf[0], &s.ctx->ppht_bytes[0], s.fixed.total);
    if (st != PRL_OK) return st;
    s.ws = static_cast<uint8_t*>(s.ctx->ppht_buf[0]);
    const PphtFixed& f = s.fixed;
    PphtPass& p = s.pass;
    p.d_mask = s.block<uint8_t>(f.mask); p.mask_page = f.mask_page;
    p.d_count = s.block<unsigned>(f.count); p.d_nlines = s.block<unsigned>(f.n_lines); p.d_cap = s.block<unsigned>(f.cap);
    p.d_nzoff = s.block<unsigned long long>(f.nz_off); p.d_lnoff = s.block<unsigned long long>(f.lines_off);
    p.d_ttab = s.block<float>(f.ttab);
    int* d_thr = s.block<int>(f.thr);
    unsigned *d_rowcnt = s.block<unsigned>(f.row_count), *d_rowoff = s.block<unsigned>(f.row_off);
    const std::vector<int> h_thr((size_t)n, fixed_thr);
    if (otsu) {
        if ((st = otsu_thresholds(gray, W, H, n, s.block<unsigned>(f.hist), d_thr, s.stream)) != PRL_OK) return st;
    } else {
        PRL_HIP_CHECK(hipMemcpyAsync(d_thr, h_thr.data(), (size_t)n * 4, hipMemcpyHostToDevice, s.stream));
    }
    hipLaunchKernelGGL(k_dark_mask, dim3((unsigned)H, (unsigned)n), dim3(64), 0, s.stream, gray, W, H, d_thr, p.d_mask, p.mask_page, d_rowcnt);
    hipLaunchKernelGGL(k_row_offsets, dim3((unsigned)n), dim3(256), 0, s.stream, H, d_rowcnt, d_rowoff, p.d_count);
    PRL_HIP_CHECK(hipGetLastError());
    s.h_count.resize((size_t)n);
    PRL_HIP_CHECK(hipMemcpyAsync(s.h_count.data(), p.d_count, (size_t)n * 4, hipMemcpyDeviceToHost, s.stream));
    PRL_HIP_CHECK(hipStreamSynchronize(s.stream));
    return PRL_OK;
}

// Phase 2, lists: point and segment lists sized from the counts, their offsets, capacities and the trig table uploaded, the
// points collected, the segment counts zeroed; SearchStart's event ends this streaming prelude.  Enqueues only (growing the
// list buffer drains the device).
int search_lists(Search& s)
{
    const int n = s.n_pages;
    s.lists = ppht_lists(s.h_count.data(), n, s.line_length, s.line_gap);
    const PphtLists& l = s.lists;
    // (growing synchronises the device, which would stall a chain that overlaps this search with its other stages:
    // keep a quarter of headroom, the lists of the following passes differ by the ink on their pages)
    if (s.ctx->ppht_bytes[1] < l.nz_bytes + l.lines_bytes) {
        const int st = ensure_buffer(&s.ctx->ppht_buf[1], &s.ctx->ppht_bytes[1], (l.nz_bytes + l.lines_bytes) / 4 * 5);
        if (st != PRL_OK) return st;
    }
    PphtPass& p = s.pass;
    p.d_nz = static_cast<unsigned*>(s.ctx->ppht_buf[1]);
    p.d_lines = reinterpret_cast<int*>(static_cast<uint8_t*>(s.ctx->ppht_buf[1]) + l.nz_bytes);
    p.h_count = s.h_count.data(); p.h_nzoff = l.nz_off.data(); p.h_lnoff = l.lines_off.data(); p.h_cap = l.cap.data();
    p.h_ttab = s.h_ttab;
    PRL_HIP_CHECK(hipMemcpyAsync(p.d_nzoff, p.h_nzoff, (size_t)n * 8, hipMemcpyHostToDevice, s.stream));
    PRL_HIP_CHECK(hipMemcpyAsync(p.d_lnoff, p.h_lnoff, (size_t)n * 8, hipMemcpyHostToDevice, s.stream));
    PRL_HIP_CHECK(hipMemcpyAsync(p.d_cap, p.h_cap, (size_t)n * 4, hipMemcpyHostToDevice, s.stream));
    // the trig table of HoughLinesProbabilistic: (float)(cos((double)n * theta) * irho), host libm as in the reference
    const float theta = (float)(3.1415926535897932384626433832795 / 180), irho = 1.f;
    for (int a = 0; a < kNumAngle; ++a) {
        s.h_ttab[2 * a] = (float)(std::cos((double)a * theta) * irho);
        s.h_ttab[2 * a + 1] = (float)(std::sin((double)a * theta) * irho);
    }
    PRL_HIP_CHECK(hipMemcpyAsync(p.d_ttab, s.h_ttab, sizeof(s.h_ttab), hipMemcpyHostToDevice, s.stream));
    hipLaunchKernelGGL(k_collect, dim3((unsigned)s.height, (unsigned)n), dim3(64), 0, s.stream, s.width, s.height, p.d_mask, p.mask_page,
                       s.block<unsigned>(s.fixed.row_off), p.d_nzoff, p.d_nz);
    PRL_HIP_CHECK(hipGetLastError());
    PRL_HIP_CHECK(hipMemsetAsync(p.d_nlines, 0, (size_t)n * 4, s.stream));
    if (s.start && s.start->ev) PRL_HIP_CHECK(hipEventRecord(s.start->ev, s.stream));   // the streaming prelude ends here
    return PRL_OK;
}

#ifdef PRL_TEST_HOOKS
// PRL_HIP_PPHT_PROF=1, one JSON line on stderr per group attempt: the four pages that took longest, then every page
void print_group_profile(const Search& s)
{
    const int n_pages = s.n_pages;
    const PphtGroupIn& gin = s.gin;
    const std::vector<unsigned long long>& h_gprof = s.h_gprof;
    std::fprintf(stderr, "{\"ppht_group_prof\": {\"pages\": %d, \"width\": %d, \"height\": %d, \"members\": %d, \"groups\": %d, \"per_page\": [", n_pages, s.width,
                 s.height, gin.geometry_out[0], gin.geometry_out[1]);
    std::vector<int> by_time(gin.page_list);
    auto cyc = [&](int pg) { unsigned long long t = 0; for (int k = 5; k < 12; ++k) t += h_gprof[(size_t)pg * 16 + k]; return t; };
    std::sort(by_time.begin(), by_time.end(), [&](int x, int y) { return cyc(x) > cyc(y); });
    for (int i = 0; i < std::min(n_pages, 4); ++i) {
        const int pg = by_time[(size_t)i];
        const unsigned long long* q = h_gprof.data() + (size_t)pg * 16;
        std::fprintf(stderr, "%s{\"page\": %d, \"points\": %u, \"exchanges\": %llu, \"blocks\": %llu, \"triggers\": %llu, \"good_lines\": %llu, \"walk_rounds\": %llu, \"cyc\": {\"fetch\": %llu, \"vote\": %llu, \"collect\": %llu, \"post\": %llu, \"walk\": %llu, \"erase\": %llu, \"strike\": %llu}, \"polls\": %llu, \"prefetched_polls\": %llu, \"collect_poll_cyc\": %llu, \"collect_barrier_cyc\": %llu}",
                     i ? ", " : "", pg, s.h_count[(size_t)pg], q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10], q[11], q[12], q[13], q[14], q[15]);
    }
    std::fprintf(stderr, "], \"all_pages_points_triggers_mcycles\": [");
    for (int i = 0; i < n_pages; ++i) {
        const int pg = by_time[(size_t)i];
        std::fprintf(stderr, "%s[%u, %llu, %llu]", i ? ", " : "", s.h_count[(size_t)pg], h_gprof[(size_t)pg * 16 + 2], cyc(pg) / 1000000ull);
    }
    std::fprintf(stderr, "]}}\n");
}

// PRL_HIP_PPHT_PROF=1, one JSON line on stderr per call that ran k_ppht_mw: the three heaviest pages, cycles per phase and
// event counts
void print_mw_profile(const Search& s)
{
    const int n_pages = s.n_pages;
    std::vector<unsigned long long> hp((size_t)n_pages * 16);
    if (hipMemcpy(hp.data(), s.d_prof, hp.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) std::fill(hp.begin(), hp.end(), 0ull);
    std::vector<int> order((size_t)n_pages);
    for (int i = 0; i < n_pages; ++i) order[(size_t)i] = i;
    auto total = [&](int i) { unsigned long long t = 0; for (int k = 0; k < 6; ++k) t += hp[(size_t)i * 16 + k]; return t; };
    std::sort(order.begin(), order.end(), [&](int x, int y) { return total(x) > total(y); });
    static const char* names[12] = {"prologue_cyc", "vote_cyc", "rollback_cyc", "walk1_cyc", "walk2_cyc", "unvote_cyc", "blocks", "triggers",
                                    "good_lines", "walk_chunks", "unvoted_px", "voted_points"};
    std::fprintf(stderr, "{\"ppht_prof\": {\"pages\": %d, \"width\": %d, \"height\": %d, \"heaviest\": [", n_pages, s.width, s.height);
    for (int r = 0; r < std::min(3, n_pages); ++r) {
        const int i = order[(size_t)r];
        std::fprintf(stderr, "%s{\"page\": %d, \"points\": %u, \"segments\": %u", r ? ", " : "", i, s.h_count[(size_t)i], s.h_nl[(size_t)i]);
        for (int k = 0; k < 12; ++k) std::fprintf(stderr, ", \"%s\": %llu", names[k], hp[(size_t)i * 16 + k]);
        std::fprintf(stderr, "}");
    }
    std::fprintf(stderr, "]}}\n");
}
#endif

// The group kernel (accumulator in LDS, ppht_group.hip) over every page, heaviest first, where the pages qualify and no knob
// or caller prefers the device-memory kernels.  *ran: it was launched and will report a status per page.  A failure of the
// attempt other than PRL_ERR_NOMEM is not one of the search.  Enqueues only (PRL_HIP_DEBUG: waits, and prints the two times).
int group_attempt(Search& s, bool* ran)
{
    *ran = false;
    const int n = s.n_pages, grp_env = env_knobs().ppht_group;
    if (grp_env == 0 || (s.start && s.start->prefer_mw && grp_env < 0) || !ppht_group_eligible(s.width, s.height, s.threshold)) return PRL_OK;
    PphtGroupIn& gin = s.gin;
    gin.n_pages = n; gin.width = s.width; gin.height = s.height;
    gin.threshold = s.threshold; gin.line_length = s.line_length; gin.line_gap = s.line_gap;
    gin.pass = s.pass;
    gin.page_list.resize((size_t)n);
    for (int i = 0; i < n; ++i) gin.page_list[(size_t)i] = i;
    std::stable_sort(gin.page_list.begin(), gin.page_list.end(), [&](int x, int y) { return s.h_count[(size_t)x] > s.h_count[(size_t)y]; });
    s.h_status.assign((size_t)n, 0u);
    gin.status_out = s.h_status.data();
#ifdef PRL_TEST_HOOKS
    if (std::getenv("PRL_HIP_PPHT_PROF")) { s.h_gprof.assign((size_t)n * 16, 0ull); gin.prof_out = s.h_gprof.data(); }
#endif
    hipEvent_t dbg_ev[3] = {nullptr, nullptr, nullptr};
    struct EvFree { hipEvent_t* e; ~EvFree() { for (int i = 0; i < 3; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } ev_free{dbg_ev};
    if (env_knobs().debug) {
        for (hipEvent_t& e : dbg_ev) PRL_HIP_CHECK(hipEventCreate(&e));
        PRL_HIP_CHECK(hipEventRecord(dbg_ev[2], s.stream));
        gin.ev[0] = dbg_ev[0]; gin.ev[1] = dbg_ev[1];
    }
    const int gst = ppht_group_run(s.ctx, gin, s.stream);
    if (gst == PRL_ERR_NOMEM) return gst;
    if (gst == PRL_OK && env_knobs().debug) {
        PRL_HIP_CHECK(hipStreamSynchronize(s.stream));
        float ms_pre = 0, ms_k = 0;
        (void)hipEventElapsedTime(&ms_pre, dbg_ev[2], dbg_ev[0]);
        (void)hipEventElapsedTime(&ms_k, dbg_ev[0], dbg_ev[1]);
        std::fprintf(stderr, "[prl ppht] visiting order + bit masks %.2f ms, group kernel %.2f ms\n", ms_pre, ms_k);
    }
    *ran = gst == PRL_OK;
    return PRL_OK;
}

// Phase 3, the group attempt.  *redo: the pages it did not finish - too large for int16 cells, a group that gave up waiting,
// or all of them when it did not run - for phase 4, in this call.  SearchStart hears that the transform has been launched.
// Synchronises when the group kernel ran.
int search_group(Search& s, std::vector<int>* redo)
{
    bool group_ran = false;
    const int st = group_attempt(s, &group_ran);
    if (st != PRL_OK) return st;
    if (s.start) s.start->launched();
    if (!group_ran) {
        for (int i = 0; i < s.n_pages; ++i) redo->push_back(i);
        return PRL_OK;
    }
    PRL_HIP_CHECK(hipStreamSynchronize(s.stream));
    for (int i = 0; i < s.n_pages; ++i)
        if (s.h_status[(size_t)i] != 1u) redo->push_back(i);
    const int* geo = s.gin.geometry_out;
    if (env_knobs().debug)
        std::fprintf(stderr, "[prl ppht] group kernel: %d pages, %d members per group, %d groups, %d workgroups, %d bytes of LDS; %zu pages left to k_ppht_mw\n",
                     s.n_pages, geo[0], geo[1], geo[2], geo[3], redo->size());
#ifdef PRL_TEST_HOOKS
    if (s.gin.prof_out) print_group_profile(s);
#endif
    return PRL_OK;
}

// the kernel argument of k_ppht / k_ppht_mw from the pass: workgroup b takes page d_plist[b] with the b-th accumulator
PphtArgs device_memory_args(const Search& s, int* d_accum, const int* d_plist)
{
    const PphtPass& p = s.pass;
    PphtArgs a{};
    a.width = s.width; a.height = s.height; a.numrho = s.numrho; a.threshold = s.threshold; a.line_length = s.line_length; a.line_gap = s.line_gap;
    a.mask = p.d_mask; a.mask_page = p.mask_page; a.nz = p.d_nz; a.nz_off = p.d_nzoff; a.count = p.d_count; a.accum = d_accum; a.ttab = p.d_ttab;
    a.lines = p.d_lines; a.lines_off = p.d_lnoff; a.lines_cap = p.d_cap; a.n_lines = p.d_nlines;
    a.prio = env_knobs().ppht_prio; a.page_list = d_plist; a.prof = s.d_prof;
    return a;
}

// Phase 4, the device-memory kernels over the pages of `redo` (which must outlive the stream's work): one biased accumulator
// per such page in ctx->ppht_buf[4], then k_ppht_mw or k_ppht.  Enqueues only.
int search_device_memory(Search& s, const std::vector<int>& redo)
{
    if (redo.empty()) return PRL_OK;
    const int n_redo = (int)redo.size();
    const size_t cells = (size_t)n_redo * kNumAngle * s.numrho;
    const int st = ensure_buffer(&s.ctx->ppht_buf[4], &s.ctx->ppht_bytes[4], r256(cells * 4));
    if (st != PRL_OK) return st;
    int* d_accum = static_cast<int*>(s.ctx->ppht_buf[4]);
    // (the paired un-votes address the cells as 64-bit words: every page's accumulator starts on an 8-byte boundary - hipMalloc
    // gives 256, a page is kNumAngle x numrho x 4 bytes with kNumAngle even - and a biased cell never borrows:
    // count > -2^31 + W H)
    if (reinterpret_cast<uintptr_t>(d_accum) % 8 != 0) return PRL_ERR_BAD_ARG;
    int* d_plist = s.block<int>(s.fixed.page_list);
    PRL_HIP_CHECK(hipMemcpyAsync(d_plist, redo.data(), (size_t)n_redo * 4, hipMemcpyHostToDevice, s.stream));
    PRL_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_accum), (int)kAccBias, cells, s.stream));   // count 0 = bias
#ifdef PRL_TEST_HOOKS
    if (std::getenv("PRL_HIP_PPHT_PROF")) {
        PRL_HIP_CHECK(hipMalloc(&s.d_prof, (size_t)s.n_pages * 16 * 8));
        PRL_HIP_CHECK(hipMemsetAsync(s.d_prof, 0, (size_t)s.n_pages * 16 * 8, s.stream));
    }
#endif
    const PphtArgs a = device_memory_args(s, d_accum, d_plist);
    // three wavefronts per page (shorter critical path per page; equal to one per page once the memory system is the limit)
    const int mw_env = env_knobs().ppht_mw;
    if (mw_env == 1 || (mw_env < 0 && n_redo <= kPphtMwMaxPages)) hipLaunchKernelGGL(k_ppht_mw, dim3((unsigned)n_redo), dim3(64 * kMwWaves), 0, s.stream, a);
    else hipLaunchKernelGGL(k_ppht, dim3((unsigned)n_redo), dim3(64), 0, s.stream, a);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// Totals of the Hough searches since the last prl_hip_reset_deskew_stats (process-wide: the chain searches on a helper thread).
std::mutex g_deskew_stats_mu;
prl_deskew_stats g_deskew_stats{};

// diagnostics of the search (prl_hip_last_deskew_stats): what the lists held against what they had room for
void add_search_stats(const Search& s)
{
    std::lock_guard<std::mutex> lk(g_deskew_stats_mu);
    prl_deskew_stats& ds = g_deskew_stats;
    for (size_t i = 0; i < (size_t)s.n_pages; ++i) {
        const long long room = (long long)s.lists.cap[i] - (long long)s.h_nl[i];
        if (ds.pages == 0 || room < ds.min_page_headroom) ds.min_page_headroom = room;
        ds.pages += 1;
        ds.points += s.h_count[i];
        ds.segments += s.h_nl[i];
        ds.segment_capacity += s.lists.cap[i];
        ds.max_page_segments = std::max<uint64_t>(ds.max_page_segments, s.h_nl[i]);
        ds.max_page_points = std::max<uint64_t>(ds.max_page_points, s.h_count[i]);
    }
}

// Phase 5, fetch: first how many segments each page has, then those and no more (the lists' capacity is a loose bound - a
// segment per line_length / (line_gap + 1) points: 0.9 GB for 256 of the reference's scans, of which 7 MB hold segments);
// then the statistics, then the overflow check.  Synchronises twice.
int search_fetch(Search& s, std::vector<std::vector<int>>* lines_out)
{
    const size_t n = (size_t)s.n_pages;
    const PphtPass& p = s.pass;
    s.h_nl.resize(n);
    PRL_HIP_CHECK(hipMemcpyAsync(s.h_nl.data(), p.d_nlines, n * 4, hipMemcpyDeviceToHost, s.stream));
    PRL_HIP_CHECK(hipStreamSynchronize(s.stream));
    lines_out->assign(n, {});
    for (size_t i = 0; i < n; ++i) {
        const size_t have = std::min<size_t>(s.h_nl[i], p.h_cap[i]);
        (*lines_out)[i].resize(have * 4);
        if (have) PRL_HIP_CHECK(hipMemcpyAsync((*lines_out)[i].data(), p.d_lines + p.h_lnoff[i] * 4, have * 16, hipMemcpyDeviceToHost, s.stream));
    }
    PRL_HIP_CHECK(hipStreamSynchronize(s.stream));
#ifdef PRL_TEST_HOOKS
    if (s.d_prof) print_mw_profile(s);
#endif
    add_search_stats(s);
    for (size_t i = 0; i < n; ++i) {
        if (s.h_nl[i] > p.h_cap[i]) {
            set_error_detail("HoughLinesP: segment list overflow");
            return PRL_ERR_NOMEM;
        }
    }
    return PRL_OK;
}

// Segments of cv::HoughLinesP(~binarized, 1, CV_PI/180, threshold, line_length, line_gap) for `n_pages` 1-channel pages
// whose dark mask (p <= thr[page]; Otsu's threshold or `fixed_thr`) is the non-zero image.  `gray` pages are device resident.
// Returns the segments per page in `lines_out` (host).  Synchronises the stream.  The caller holds ctx->ppht_mu (the workspace
// is ctx->ppht_buf).  Pages that qualify go to the group kernel; what it does not finish is done by k_ppht_mw, in this call.
int ppht_pages(DeviceCtx* ctx, int n_pages, const PageSet& gray, int width, int height, int threshold, int line_length, int line_gap,
               bool otsu, int fixed_thr, std::vector<std::vector<int>>* lines_out, hipStream_t stream, SearchStart* start = nullptr)
{
    Search s;
    s.ctx = ctx; s.stream = stream; s.start = start;
    s.n_pages = n_pages; s.width = width; s.height = height;
    s.threshold = threshold; s.line_length = line_length; s.line_gap = line_gap;
    s.numrho = (int)std::lrint((double)(float)((width + height) * 2 + 1));
    s.fixed = ppht_fixed(n_pages, width, height);
    std::vector<int> redo;
    int st;
    if ((st = search_points(s, gray, otsu, fixed_thr)) != PRL_OK) return st;
    if ((st = search_lists(s)) != PRL_OK) return st;
    if ((st = search_group(s, &redo)) != PRL_OK) return st;
    if ((st = search_device_memory(s, redo)) != PRL_OK) return st;
    return search_fetch(s, lines_out);
}

}  // namespace

int otsu_thresholds(const PageSet& gray, int width, int height, int n_pages, unsigned* d_hist, int* d_thr, hipStream_t stream)
{
    PRL_HIP_CHECK(hipMemsetAsync(d_hist, 0, (size_t)n_pages * 256 * 4, stream));
    const dim3 hg((unsigned)std::min(4, (width + 1023) / 1024), (unsigned)std::min(height, 64), (unsigned)n_pages);
    hipLaunchKernelGGL(k_hist, hg, dim3(256), 0, stream, gray, width, height, d_hist);
    hipLaunchKernelGGL(k_otsu, dim3((unsigned)((n_pages + 63) / 64)), dim3(64), 0, stream, d_hist, width, height, n_pages, d_thr);
    PRL_HIP_CHECK(hipGetLastError());
    return PRL_OK;
}

// The angle vote of findAngle (deskew.cpp:158-201) over the segments of one page: every segment's atan2 joins the FIRST cluster
// whose representative (the angle that opened it) lies within 0.01 rad, else opens a new one; a cluster's tally counts the joiners
// only (it starts at 0, as the reference's does), the first cluster with the largest tally wins and its representative is
// returned in degrees.
double vote_angle(const int* segments, int n_segments)
{
    if (n_segments <= 0) return 0.0;
    constexpr double kClusterWidth = 0.01;
    std::vector<double> representative;   // cluster -> the angle that opened it
    std::vector<int> joiners;             // cluster -> segments that joined it afterwards
    for (int i = 0; i < n_segments; ++i) {
        const int* seg = segments + 4 * i;   // x0, y0, x1, y1
        const double theta = std::atan2((double)seg[3] - seg[1], (double)seg[2] - seg[0]);
        size_t c = 0;
        while (c < representative.size() && !(std::fabs(theta - representative[c]) <= kClusterWidth)) ++c;
        if (c == representative.size()) {
            representative.push_back(theta);
            joiners.push_back(0);
        } else {
            ++joiners[c];
        }
    }
    size_t winner = 0;   // (std::max_element keeps the first of equal maxima)
    for (size_t c = 1; c < joiners.size(); ++c)
        if (joiners[c] > joiners[winner]) winner = c;
    return representative[winner] * 180 / 3.14159265358979323846;
}

int find_angle_segments(DeviceCtx* ctx, int cnt, const PageSet& gray, int width, int height, bool otsu,
                        std::vector<std::vector<int>>* lines, hipStream_t hs, SearchStart* start)
{
    return ppht_pages(ctx, cnt, gray, width, height, 100, (int)std::lrint((double)(width / 8.f)), (int)std::lrint(20.0), otsu, 254, lines,
                      hs, start);
}

}  // namespace prl_hip

using namespace prl_hip;

namespace {
// The checks of the entries below on their one-channel pages without a destination, in the order tests/test_capi_cpu.py pins:
// empty; then null source, negative page count, short rows, the entry's own result pointers (`results_ok`), sides above 32767
// (a point is packed as x | y << 16).
int point_pages_checks(const PageArgs& a, bool results_ok)
{
    int st = pages_nonempty(a);
    if (st != PRL_OK) return st;
    if ((st = pages_rows_ok(a, 1, 0, true)) != PRL_OK || !results_ok) return PRL_ERR_BAD_ARG;
    return pages_sides_ok(a, 32767);
}
}  // namespace

extern "C" {

// cv::HoughLinesP(image, lines, 1, CV_PI/180, threshold, line_length, line_gap) on ONE 1-channel device page whose
// non-zero pixels are the points (test / building-block entry).  lines: host buffer of 4*cap ints; *n_lines = segments found.
int prl_hip_houghp_device(const uint8_t* d_image, size_t step, int width, int height, int threshold, int line_length, int line_gap,
                          int32_t* lines, int cap, int* n_lines, void* stream)
{
    int st = point_pages_checks(PageArgs{1, d_image, 0, step, width, height, nullptr, 0, 0}, n_lines && !(cap > 0 && !lines));
    if (st != PRL_OK) return st;
    DeviceCtx* ctx;
    if ((st = current_ctx(&ctx)) != PRL_OK) return st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    std::lock_guard<std::mutex> slk(ctx->stage_mu);  // lock order: stage_mu, then mu
    // HoughLinesP's points are the NON-ZERO pixels; the point stage selects "p <= thr", so it runs on the complement:
    // p != 0  <=>  (255 - p) <= 254
    const size_t bytes = (size_t)width * height;
    st = ensure_stage(ctx, bytes);
    if (st != PRL_OK) return st;
    st = stage_acquire(ctx, hs);
    if (st != PRL_OK) return st;
    StageRelease release{ctx, hs};
    st = prl_hip_invert_batch_device(1, d_image, 0, step, width, height, static_cast<uint8_t*>(ctx->stage), bytes, (size_t)width, stream);
    if (st != PRL_OK) return st;
    const PageSet g = page_set(static_cast<uint8_t*>(ctx->stage), 0, (size_t)width);
    std::vector<std::vector<int>> out;
    {
        std::lock_guard<std::mutex> lk(ctx->ppht_mu);
        st = ppht_pages(ctx, 1, g, width, height, threshold, line_length, line_gap, false, 254, &out, hs);
    }
    if (st != PRL_OK) return st;
    *n_lines = (int)(out[0].size() / 4);
    for (int i = 0; i < std::min(cap, *n_lines) * 4; ++i) lines[i] = out[0][(size_t)i];
    return PRL_OK;
}

int prl_hip_last_deskew_stats(prl_deskew_stats* out)
{
    if (!out) return PRL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lk(g_deskew_stats_mu);
    *out = g_deskew_stats;
    return PRL_OK;
}

int prl_hip_reset_deskew_stats(void)
{
    std::lock_guard<std::mutex> lk(g_deskew_stats_mu);
    g_deskew_stats = prl_deskew_stats{};
    return PRL_OK;
}

/*
 * prl::findAngle (src/deskew/deskew.cpp:139-205) on n_pages 1-channel device pages: bitwise_not (:146), cv::HoughLinesP(input,
 * lines, 1, CV_PI/180, 100, width/8.f, 20) (:148), atan2 per segment and the first-fit vote (:158-201).  HoughLinesP's points
 * are the non-zero pixels of the complement, i.e. the pixels p != 255: the point stage runs on the page as it is with the
 * fixed threshold 254 (no inverted copy).  angles / n_segments: host arrays, one entry per page.  Synchronises.
 */
int prl_hip_find_angle_batch_device(int n_pages, const uint8_t* d_image, size_t page_stride, size_t step, int width, int height,
                                    double* angles, int32_t* n_segments, void* stream)
{
    int st = point_pages_checks(PageArgs{n_pages, d_image, page_stride, step, width, height, nullptr, 0, 0}, angles != nullptr);
    if (st != PRL_OK) return st;
    if (n_pages == 0) return PRL_OK;
    DeviceCtx* ctx;
    if ((st = current_ctx(&ctx)) != PRL_OK) return st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const int chunk = deskew_pages_per_pass(n_pages, width, height);
    for (int first = 0; first < n_pages; first += chunk) {
        const int cnt = std::min(chunk, n_pages - first);
        const PageSet g = pages_from(page_set(d_image, page_stride, step), first);
        std::vector<std::vector<int>> lines;
        {
            std::lock_guard<std::mutex> lk(ctx->ppht_mu);
            st = find_angle_segments(ctx, cnt, g, width, height, false, &lines, hs, nullptr);
        }
        if (st != PRL_OK) return st;
        for (int i = 0; i < cnt; ++i) {
            const int n = (int)(lines[(size_t)i].size() / 4);
            angles[first + i] = vote_angle(lines[(size_t)i].data(), n);
            if (n_segments) n_segments[first + i] = n;
        }
    }
    return PRL_OK;
}

/* prl::findAngle on one host image (what the cv::Mat wrapper calls): the batch entry's checks, a null source being an empty image. */
int prl_hip_find_angle_host(const uint8_t* src, size_t src_step, int width, int height, double* angle, int32_t* n_segments)
{
    const PageArgs h{1, src, 0, src_step, width, height, nullptr, 0, 0};
    if (pages_nonempty(h) != PRL_OK || !src) return PRL_ERR_EMPTY;
    const int st = point_pages_checks(h, angle != nullptr);
    if (st != PRL_OK) return st;
    return host_roundtrip(h, 1, 0, 0, nullptr, nullptr, [&](const PageArgs& p, hipStream_t s) {
        return prl_hip_find_angle_batch_device(1, p.src, p.src_page_stride, p.src_step, width, height, angle, n_segments, s);
    });
}

}  // extern "C"
