// CPU test of prlib_amd/csrc/ppht_plan.h (the geometry of the HoughLinesP group kernel): for every page size below and every
// requested group size 1..32
//   range      every cvRound(x cos + y sin) of the page - two float32 products, one float32 sum, round half to even, as the kernel
//              and the oracle compute it - indexes a cell inside the row the plan gives that angle (all pixels of a page of up to
//              4 10^5, the four border lines of a larger one: the products are monotone in x and y);
//   ownership  member g owns the angles n = g (mod G), each once, in rising order; its rows follow each other without gap or
//              overlap; tab_dwords is ceil(cells / 2); lds_bytes is the largest member's size and within the budget;
//   group size the G returned is the smallest >= min_g whose largest member fits the budget - recomputed here from corner
//              projections in long double, not from the plan's own rows - and the values of five page sizes worked out beforehand;
//   refusals   no plan for a side of 8001 or a threshold of 0.
// And the workspace of a pass of the search, from figures worked out by hand: the fixed blocks (aligned, in order, without gap
// or overlap, the total), the two lists from given counts, the pages a pass takes under a budget.
// Built by tests/cpp/Makefile (g++), no device.
#include <cfenv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../prlib_amd/csrc/ppht_plan.h"

using namespace prl_hip;

static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { if (bad < 40) std::printf("line %d: %s\n", __LINE__, #cond); ++bad; } } while (0)

static const size_t kBudget = 155 * 1024;   // what a 160 KB CU leaves for the cells

static float ttab[2 * kNumAngle];

static int cv_round_f(float v) { return (int)std::lrintf(v); }   // round half to even (default rounding mode)

// the largest member's bytes for a group of G, from the exact extent of the projections (independent of plan_group's rows: a row
// must hold every integer from floor(min) - 1 to ceil(max) + 1, the page's corners being the extremes)
static size_t worst_bytes(int W, int H, int G)
{
    size_t worst = 0;
    for (int g = 0; g < G; ++g) {
        size_t cells = 0;
        for (int n = g; n < kNumAngle; n += G) {
            const long double c = ttab[2 * n], s = ttab[2 * n + 1];
            long double lo = 0, hi = 0;   // (corner (0, 0))
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) {
                    const long double p = (a ? W - 1 : 0) * c + (b ? H - 1 : 0) * s;
                    lo = std::min(lo, p);
                    hi = std::max(hi, p);
                }
            cells += (size_t)((long long)std::ceil(hi) + 1 - ((long long)std::floor(lo) - 1) + 1);
        }
        worst = std::max(worst, (cells + 1) / 2 * 4);
    }
    return worst;
}

// the smallest and the largest r = cvRound(x cos + y sin) a pixel of the page gives for each angle
static int r_lo[kNumAngle], r_hi[kNumAngle];

static void scan_pixel(int x, int y)
{
    const float fx = (float)x, fy = (float)y;
    for (int n = 0; n < kNumAngle; ++n) {
        const float px = fx * ttab[2 * n], py = fy * ttab[2 * n + 1];   // (-ffp-contract=off: one rounding each)
        const float fr = px + py;
        const int r = cv_round_f(fr);
        r_lo[n] = std::min(r_lo[n], r);
        r_hi[n] = std::max(r_hi[n], r);
    }
}

static void scan_page(int W, int H)
{
    for (int n = 0; n < kNumAngle; ++n) r_lo[n] = r_hi[n] = 0;   // (pixel (0, 0))
    if ((long long)W * H <= 400000) {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) scan_pixel(x, y);
    } else {
        for (int x = 0; x < W; ++x) { scan_pixel(x, 0); scan_pixel(x, H - 1); }
        for (int y = 0; y < H; ++y) { scan_pixel(0, y); scan_pixel(W - 1, y); }
    }
}

static void check_size(int W, int H)
{
    scan_page(W, H);
    int last_g = 0;
    for (int min_g = 1; min_g <= kMaxG; ++min_g) {
        const GroupPlan gp = plan_group(W, H, 100, ttab, kBudget, min_g);
        // group size: the smallest that fits
        int want_g = 0;
        for (int G = min_g; G <= kMaxG && !want_g; ++G)
            if (worst_bytes(W, H, G) <= kBudget) want_g = G;
        CHECK(gp.G == want_g);
        if (gp.G == 0) continue;
        if (gp.G == last_g) continue;   // (the same plan as for the min_g before: checked)
        last_g = gp.G;
        const int G = gp.G;
        CHECK(gp.tab.size() == (size_t)G * kMaxA && gp.tab_n.size() == (size_t)G && gp.tab_dwords.size() == (size_t)G);
        if (bad) return;
        // ownership
        int seen[kNumAngle] = {0};
        std::vector<int> start((size_t)G * kMaxA, 0), len((size_t)G * kMaxA, 0);
        size_t worst = 0;
        for (int g = 0; g < G; ++g) {
            const int A = gp.tab_n[(size_t)g];
            CHECK(A == (kNumAngle - g + G - 1) / G && A >= 1 && A <= kMaxA);
            int cells = 0;
            for (int k = 0; k < A; ++k) {
                const GrpAngle& t = gp.tab[(size_t)g * kMaxA + k];
                CHECK(t.n == g + k * G && t.n < kNumAngle);
                if (t.n < 0 || t.n >= kNumAngle) return;
                ++seen[t.n];
                CHECK(t.c == ttab[2 * t.n] && t.s == ttab[2 * t.n + 1]);
                // the row of this angle: from the smallest to the largest r over the page's corners (exact), one spare cell at
                // either end at the most beyond floor / ceil
                const long double c = t.c, s = t.s;
                long double lo = 0, hi = 0;
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b) {
                        const long double p = (a ? W - 1 : 0) * c + (b ? H - 1 : 0) * s;
                        lo = std::min(lo, p);
                        hi = std::max(hi, p);
                    }
                const int rmin = (int)std::floor(lo) - 1, rmax = (int)std::ceil(hi) + 1;
                // rows follow each other: this one starts where the one before ended
                start[(size_t)g * kMaxA + k] = cells;
                len[(size_t)g * kMaxA + k] = rmax - rmin + 1;
                CHECK(t.base + rmin == cells);
                cells += rmax - rmin + 1;
            }
            CHECK(gp.tab_dwords[(size_t)g] == (cells + 1) / 2);
            worst = std::max(worst, (size_t)((cells + 1) / 2) * 4);
        }
        for (int n = 0; n < kNumAngle; ++n) CHECK(seen[n] == 1);
        CHECK(gp.lds_bytes == worst && gp.lds_bytes <= kBudget);
        if (bad) return;
        // range: the cell index base + r is monotone in r, so the extremes of r decide for every pixel
        for (int g = 0; g < G; ++g)
            for (int k = 0; k < gp.tab_n[(size_t)g]; ++k) {
                const GrpAngle& t = gp.tab[(size_t)g * kMaxA + k];
                const int st = start[(size_t)g * kMaxA + k], en = st + len[(size_t)g * kMaxA + k];
                if (t.base + r_lo[t.n] < st || t.base + r_hi[t.n] >= en) {
                    if (bad < 40) std::printf("G %d, angle %d: r in [%d, %d] gives cells [%d, %d], the row is [%d, %d)\n", G, t.n, r_lo[t.n], r_hi[t.n],
                                              t.base + r_lo[t.n], t.base + r_hi[t.n], st, en);
                    ++bad;
                }
            }
    }
}

static int plan_g(int W, int H, int thr = 100, int min_g = 1) { return plan_group(W, H, thr, ttab, kBudget, min_g).G; }

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// The fixed workspace of a pass: the blocks in the driver's order, 256-aligned, each with room for what it holds and ending
// where the next one starts; the total is the sum the driver formed before the layout existed: hist + thr + 2 rows +
// 4 per-page words + 2 per-page offsets + trig table + masks, each rounded to 256.
static void check_fixed(int n, int W, int H, size_t want_total)
{
    const PphtFixed f = ppht_fixed(n, W, H);
    const size_t N = (size_t)n, mask_page = up256((size_t)W * H);
    const size_t off[13] = {f.hist, f.thr, f.row_count, f.row_off, f.count, f.n_lines, f.cap, f.nz_off, f.lines_off, f.ttab,
                            f.page_list, f.mask, f.total};
    const size_t need[12] = {N * 1024, N * 4, N * H * 4, N * H * 4, N * 4, N * 4, N * 4, N * 8, N * 8, 1440, N * 4, N * mask_page};
    CHECK(f.hist == 0 && f.mask_page == mask_page);
    for (int b = 0; b < 12; ++b) CHECK(off[b] % 256 == 0 && off[b + 1] == off[b] + up256(need[b]));
    const size_t total = up256(N * 1024) + up256(N * 4) + 2 * up256(N * H * 4) + 4 * up256(N * 4) + 2 * up256(N * 8) + up256(1440) + N * mask_page;
    CHECK(f.total == total && f.total == want_total);
}

static void check_layout()
{
    check_fixed(3, 300, 390, 367872);   // 3072 + 256 + 2 * 4864 + 4 * 256 + 2 * 256 + 1536 + 3 * 117248
    check_fixed(1, 1, 1, 5120);         // 1024 + 256 + 2 * 256 + 4 * 256 + 2 * 256 + 1536 + 256: no block below 256 bytes
    check_fixed(5, 203, 97, 111104);    // rows of 5 * 97 * 4 = 1940 -> 2048 bytes, masks of 19691 -> 19712: 5120 + 256 + 2 * 2048 + 4 * 256 + 2 * 256 + 1536 + 5 * 19712
    {   // the lists of five pages at findAngle's parameters for a page 896 wide: a segment per 112 / 21 = 5 points
        const unsigned count[5] = {0, 1, 64, 65, 1000};
        const PphtLists l = ppht_lists(count, 5, 112, 20);
        const unsigned long long nz_off[5] = {0, 0, 64, 128, 256}, ln_off[5] = {0, 16, 32, 60, 89};
        const unsigned cap[5] = {16, 16, 28, 29, 216};
        for (int i = 0; i < 5; ++i) CHECK(l.nz_off[(size_t)i] == nz_off[i] && l.cap[(size_t)i] == cap[i] && l.lines_off[(size_t)i] == ln_off[i]);
        CHECK(l.nz_total == 1280 && l.lines_total == 305);
        CHECK(l.nz_bytes == 5376 && l.lines_bytes == 5376);   // r256(4 * 1280 + 256), r256(16 * 305 + 256)
        // a line no longer than the gap + 1 may end after every point: line_length 37 / (line_gap 37 + 1) = 0 -> 1
        const PphtLists m = ppht_lists(count, 5, 37, 37), g0 = ppht_lists(count, 5, 37, 20);
        for (int i = 0; i < 5; ++i) CHECK(m.cap[(size_t)i] == count[i] + 16 && g0.cap[(size_t)i] == count[i] + 16);
        CHECK(ppht_lists(count, 0, 112, 20).nz_bytes == 256 && ppht_lists(count, 0, 112, 20).lines_bytes == 256);
    }
    // pages per pass: max(1, min(n, 16384, budget / per_page)) with the per-page cost written out
    CHECK(ppht_bytes_per_page(300, 390) == 1292484);   // 2 * 117248 + 180 * 1381 * 4 + 390 * 8 + 2048 + 58500
    static const int ns[] = {0, 1, 2, 3, 255, 16384, 16385, 100000};
    static const int wh[][2] = {{1, 1}, {300, 390}, {203, 97}, {2480, 3508}, {32767, 16}};
    static const size_t budgets[] = {0, 1, (size_t)1 << 20, 1292483, 1292484, 2 * 1292484 - 1, (size_t)1 << 30, (size_t)24576 << 20, (size_t)1 << 46};
    for (int n : ns)
        for (const auto& s : wh)
            for (size_t budget : budgets) {
                const size_t W = (size_t)s[0], H = (size_t)s[1];
                const size_t per = 2 * up256(W * H) + 180 * ((W + H) * 2 + 1) * 4 + H * 8 + 2048 + W * H / 2;
                const size_t want = std::max<size_t>(1, std::min<size_t>({(size_t)n, (size_t)16384, budget / per}));
                CHECK((size_t)ppht_pages_per_pass(n, s[0], s[1], budget) == want);
            }
    CHECK(ppht_pages_per_pass(3, 300, 390, (size_t)1 << 20) == 1 && ppht_pages_per_pass(100000, 1, 1, (size_t)1 << 46) == 16384);
}

int main()
{
    CHECK(std::fegetround() == FE_TONEAREST);
    // the trig table as the host code builds it (HoughLinesProbabilistic: (float)cos((double)n * theta), theta a float)
    const float theta = (float)(3.1415926535897932384626433832795 / 180);
    for (int n = 0; n < kNumAngle; ++n) {
        ttab[2 * n] = (float)std::cos((double)n * theta);
        ttab[2 * n + 1] = (float)std::sin((double)n * theta);
    }
    static const int sizes[][2] = {{1, 1}, {2, 3}, {50, 40}, {203, 97}, {97, 203}, {420, 300}, {4400, 24}, {8000, 16}, {16, 8000},
                                   {2480, 3508}, {8000, 8000}};
    for (const auto& s : sizes) {
        const int before = bad;
        check_size(s[0], s[1]);
        if (bad != before) std::printf("  (page %d x %d)\n", s[0], s[1]);
    }
    uint64_t rng = 0x9e3779b97f4a7c15ull;   // 40 seeded sizes below 600 (xorshift64)
    for (int i = 0; i < 40; ++i) {
        int wh[2];
        for (int& v : wh) {
            rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
            v = 1 + (int)(rng % 599);
        }
        const int before = bad;
        check_size(wh[0], wh[1]);
        if (bad != before) std::printf("  (page %d x %d)\n", wh[0], wh[1]);
    }
    // group sizes worked out beforehand (W x H)
    CHECK(plan_g(420, 300) == 2);
    CHECK(plan_g(4400, 24) == 7);
    CHECK(plan_g(2480, 3508) == 9);
    CHECK(plan_g(8000, 16) == 12);
    CHECK(plan_g(8000, 8000) == 26);
    CHECK(plan_g(50, 40) == 1);
    CHECK(plan_g(50, 40, 100, 32) == 32);
    CHECK(plan_g(50, 40, 100, 33) == 0);     // no group of more than kMaxG members
    CHECK(plan_g(50, 40, 100, 0) == 1 && plan_g(50, 40, 100, -3) == 1);
    // refusals
    CHECK(plan_g(8001, 16) == 0 && plan_g(16, 8001) == 0 && plan_g(8000, 16) != 0);
    CHECK(plan_g(420, 300, 0) == 0 && plan_g(420, 300, -1) == 0 && plan_g(420, 300, 1) == 2);
    CHECK(plan_g(8000, 8000, 100, 27) == 27);
    {   // a budget nothing fits
        CHECK(plan_group(8000, 8000, 100, ttab, 16 * 1024, 1).G == 0);
    }
    check_layout();
    if (bad) { std::printf("ppht_plan: %d FAILED\n", bad); return 1; }
    std::printf("ppht_plan: OK\n");
    return 0;
}
