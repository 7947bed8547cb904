// chain_schedule.h — how many pages each pass of the config-5 chain takes and which kernel searches its angles: the policy
// of prl_hip_chain_pages_device (glue.hip) as arithmetic on integers and seconds.  Plain C++17: no HIP header, no
// environment, no I/O - glue.hip fills the knobs from env_knobs(), tests/cpp/test_chain_schedule.cpp drives it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace prl_hip {

// Measured costs (A4 colour scans on one MI355X).  The search of a pass takes max(its heaviest page's own time, the pass's
// share of the chip's atomic rate): kTailS seconds per point for one page (one CU's path for scattered returning atomics),
// kRateS per point for the chip (profiles/r05: 7.4e6 points 4.4 s alone, 256 pages of 0.84e6 points 1.18 s).
constexpr double kTailS = 0.6e-6, kRateS = 5.5e-9;
constexpr double kNlmPageS = 4.35e-3;   // NL-means per 3508 x 3508 x 3 page (profiles/r06/chain_1024_schedules.txt)
constexpr double kSlack = 0.03;         // NL-means may run this fraction of a search's time past it before passes shrink

// Pass schedule (with deskew).  Passes must be large enough for the angle search to run near its full rate (>= ~128 pages) and,
// when NL-means runs beside the next pass's search, small enough for it to finish inside that search: the search's time per
// page grows as passes shrink (it is latency-bound per page), NL-means' does not.  The sizes below are STARTING values (A4
// colour scans with ~9 % ink: 192 pages per pass hide NL-means completely, 256 leave it 0.3 s past every search); with the
// head / body / tail split every pass measures how long its NL-means kernels ran past the search beside them and the
// following searches are sized from that (shrink in proportion; creep up while there is slack), so other page sizes and ink
// densities find their own balance.  chain_pass fixes the size (no adaptation).  Without denoise: 256, fixed.
struct ChainSchedule {
    int n_pages, chunk;   // chunk: pages the workspaces of a pass hold (chain_pass_layout)
    bool deskew, denoise;
    int overlap;          // PRL_HIP_CHAIN_OVERLAP
    int chain_pass;       // PRL_HIP_CHAIN_PASS
    int first_sz, main_sz;
    bool adaptive = false;
    int max_cnt = 1;      // the largest pass the workspace is sized for (an adaptive schedule may grow by a third)

    ChainSchedule(int n_pages_, int chunk_, bool deskew_, bool denoise_, int chain_overlap, int chain_pass_, int chain_first_pass)
        : n_pages(n_pages_), chunk(chunk_), deskew(deskew_), denoise(denoise_), overlap(chain_overlap), chain_pass(chain_pass_),
          first_sz(chunk_), main_sz(chunk_)
    {
        if (deskew && overlap) {
            const int want_main = chain_pass > 0 ? chain_pass : (denoise ? 192 : 256);
            main_sz = std::min(chunk, want_main);
            const int want_first = chain_first_pass > 0 ? chain_first_pass : main_sz;
            first_sz = n_pages >= 3 * want_first ? std::min(main_sz, want_first) : main_sz;
            adaptive = denoise && overlap == 2 && chain_pass == 0;
        }
        fix_max_cnt();
    }

    bool wants_census() const { return deskew && overlap && chain_pass == 0 && n_pages > main_sz; }

    // Tail-aware passes (round 5).  On text scans the chip's rate rules a search and passes of ~192 pages pipeline well; on
    // photographs with dark tables in them (the reference's own test images: up to 89 % of a page dark after Otsu) every pass
    // pays its heaviest page - 4.4 s - and two passes cost twice what one would.  A pass is therefore extended for as long as
    // the pages added to it hide behind its heaviest page (ink: the census of the dark pixels per page).  The NL-means balance
    // controller stays off for such a batch.  Returns the heaviest page's points.
    unsigned extend_for_tail(const std::vector<unsigned>& ink)
    {
        unsigned heaviest = 0;
        double sum = 0.0;
        int fit = 0;   // pages of the first pass that hide behind the heaviest of them
        for (int i = 0; i < std::min(n_pages, chunk); ++i) {
            heaviest = std::max(heaviest, ink[(size_t)i]);
            sum += ink[(size_t)i];
            if (sum * kRateS <= heaviest * kTailS) fit = i + 1;
        }
        if (fit > main_sz * 5 / 4) {
            main_sz = first_sz = std::min(chunk, fit);
            adaptive = false;
            fix_max_cnt();
        }
        return heaviest;
    }

    // pages of the pass that starts at page `first`
    int next_count(int first) const
    {
        int cnt = std::min({first == 0 ? first_sz : main_sz, n_pages - first, max_cnt});
        if (n_pages - first - cnt > 0 && n_pages - first - cnt < main_sz / 8 && n_pages - first <= max_cnt) cnt = n_pages - first;  // no tiny last pass
        return cnt;
    }

    // The controller step after a body that ran beside the search of the next pass (ncnt pages, search_seconds long):
    // past_seconds is how long NL-means ran past that search, early: it was through before.  Sizes the searches that are
    // still to start; returns main_sz before and after.
    std::pair<int, int> observe(double search_seconds, double past_seconds, bool early, int ncnt)
    {
        const int before = main_sz;
        if (adaptive && search_seconds > 0.0 && ncnt >= main_sz) {   // (a short last search says nothing about the balance)
            if (past_seconds > kSlack * search_seconds) main_sz = (int)(main_sz * search_seconds / (search_seconds + past_seconds)) / 16 * 16;
            else if (early) main_sz += 16;
            main_sz = std::max(std::min(64, max_cnt), std::min(main_sz, max_cnt));
        }
        return {before, main_sz};
    }

    // Which kernel searches a pass (round 6).  The group kernel (accumulator in LDS) is 3 to 5 times faster than k_ppht_mw but fills the
    // LDS of every CU it runs on: beside this chain's NL-means it does not hide, it takes turns with it.  k_ppht_mw lives on memory-side
    // atomics and does hide behind NL-means - when it is clearly shorter than the body it runs beside.  Measured on 1024 synthetic A4
    // text scans (profiles/r06/chain_1024_schedules.txt): group kernel for every pass, the pass size following the controller down
    // to 64 pages (the tails of search and body interleave) 6.14 s; group kernel, passes of 192-208 pages 6.40 s; k_ppht_mw for the
    // passes whose estimate fits the body (alternating with the group kernel) 6.54 s - its 192-page search takes 1.3 s beside NL-means,
    // not the 0.9 s it takes alone; round 5 (k_ppht_mw throughout) 6.16 s.  So k_ppht_mw is preferred only where its estimate is
    // HALF the body's (pages with few points): costs as measured, k_ppht_mw max(kRateS per point of the pass, kTailS per point of its
    // heaviest page), NL-means kNlmPageS per 3508 x 3508 x 3 page.  beside_cnt: pages of the body the search runs beside (0: none);
    // len: side of a deskewed page.
    bool prefers_mw(const std::vector<unsigned>& ink, int first, int cnt, int beside_cnt, int len) const
    {
        if (!denoise || overlap != 2 || beside_cnt <= 0 || ink.empty()) return false;
        double sum = 0.0, heaviest = 0.0;
        for (int i = first; i < first + cnt; ++i) {
            sum += ink[(size_t)i];
            heaviest = std::max(heaviest, (double)ink[(size_t)i]);
        }
        const double est_mw = std::max(sum * kRateS, heaviest * kTailS);
        const double est_nlm = kNlmPageS * beside_cnt * ((double)len * len) / (3508.0 * 3508.0);
        return est_mw <= 0.5 * est_nlm;
    }

private:
    void fix_max_cnt()
    {
        const int largest = std::max(main_sz, first_sz);
        max_cnt = std::max(1, std::min({chunk, n_pages, adaptive ? largest * 4 / 3 : largest}));
    }
};

}  // namespace prl_hip
