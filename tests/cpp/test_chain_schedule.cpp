// CPU test of prlib_amd/csrc/chain_schedule.h (the pass-size policy of the config-5 chain, glue.hip): the expected sizes are
// worked out by hand from the rules - the starting sizes 192 / 256, the 5/4 rule of tail-bound batches, the no-tiny-last-pass
// rule, the controller's proportional shrink in steps of 16 between 64 and max_cnt - not taken from the code under test.
// Built by tests/cpp/Makefile (g++).
#include <cstdio>
#include <vector>

#include "../../prlib_amd/csrc/chain_schedule.h"

using prl_hip::ChainSchedule;

static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++bad; } } while (0)

// the passes of a whole batch with no controller movement
static std::vector<int> passes(const ChainSchedule& s)
{
    std::vector<int> out;
    for (int first = 0; first < s.n_pages && out.size() < 100000;) {
        const int cnt = s.next_count(first);
        out.push_back(cnt);
        if (cnt <= 0) break;
        first += cnt;
    }
    return out;
}

// n_pages, chunk, deskew, denoise, overlap, chain_pass, chain_first_pass; the census is taken where the schedule wants one
static ChainSchedule make(int n, int chunk, bool denoise, int overlap, int pass, int first_pass, const std::vector<unsigned>& ink)
{
    ChainSchedule s(n, chunk, true, denoise, overlap, pass, first_pass);
    if (s.wants_census()) s.extend_for_tail(ink);
    return s;
}

int main()
{
    using V = std::vector<int>;
    const std::vector<unsigned> text1024(1024, 840000u);
    {   // 109 pages of 840000 points hide behind one of them (109 * 840000 * 5.5 ns <= 840000 * 0.6 us): not above 192 * 5 / 4
        ChainSchedule s = make(1024, 1024, true, 2, 0, 0, text1024);
        CHECK(s.wants_census());
        CHECK(s.main_sz == 192 && s.first_sz == 192 && s.adaptive && s.max_cnt == 256);
        CHECK(passes(s) == (V{192, 192, 192, 192, 192, 64}));
    }
    {
        ChainSchedule s = make(1024, 1024, false, 2, 0, 0, text1024);
        CHECK(s.main_sz == 256 && !s.adaptive && s.max_cnt == 256);
        CHECK(passes(s) == (V{256, 256, 256, 256}));
    }
    {   // the remainder of 8 pages is below 192 / 8 and 200 pages fit the workspace: absorbed
        ChainSchedule s = make(200, 200, true, 2, 0, 0, std::vector<unsigned>(200, 840000u));
        CHECK(s.max_cnt == 200);
        CHECK(passes(s) == (V{200}));
    }
    std::vector<unsigned> photo(260, 100000u);
    photo[0] = 7400000u;   // 4.44 s alone: 8000 pages of 100000 points would hide behind it
    {
        ChainSchedule s(260, 260, true, true, 2, 0, 0);
        CHECK(s.wants_census() && s.main_sz == 192);
        CHECK(s.extend_for_tail(photo) == 7400000u);
        CHECK(s.main_sz == 260 && s.first_sz == 260 && !s.adaptive && s.max_cnt == 260);
        CHECK(passes(s) == (V{260}));
    }
    {   // the workspace holds 250 pages: the last 10 cannot be absorbed
        ChainSchedule s = make(260, 250, true, 2, 0, 0, photo);
        CHECK(s.main_sz == 250 && s.first_sz == 250 && !s.adaptive && s.max_cnt == 250);
        CHECK(passes(s) == (V{250, 10}));
    }
    {
        ChainSchedule s(300, 300, true, true, 2, 64, 0);
        CHECK(!s.wants_census() && !s.adaptive && s.max_cnt == 64);
        CHECK(passes(s) == (V{64, 64, 64, 64, 44}));
    }
    {
        ChainSchedule s = make(1024, 1024, true, 2, 0, 64, text1024);
        CHECK(s.first_sz == 64 && s.main_sz == 192 && s.max_cnt == 256);
        CHECK(passes(s) == (V{64, 192, 192, 192, 192, 192}));
    }
    {
        ChainSchedule s(1024, 700, true, true, 0, 0, 0);
        CHECK(s.first_sz == 700 && s.main_sz == 700 && !s.wants_census() && !s.adaptive);
        CHECK(passes(s) == (V{700, 324}));
        ChainSchedule plain(1024, 700, false, true, 2, 0, 0);   // without deskew nothing is searched: whole chunks
        CHECK(plain.first_sz == 700 && plain.main_sz == 700 && !plain.wants_census() && !plain.adaptive);
    }

    // the controller, on the 1024-page denoise schedule (main 192, max_cnt 256)
    const ChainSchedule base = make(1024, 1024, true, 2, 0, 0, text1024);
    {
        ChainSchedule s = base;
        auto r = s.observe(1.0, 1.0, false, 192);   // the body took twice the search: half the pages
        CHECK(r.first == 192 && r.second == 96 && s.main_sz == 96);
        r = s.observe(1.0, 0.0, true, 96);          // slack: one step up
        CHECK(r.first == 96 && r.second == 112 && s.main_sz == 112);
        CHECK(passes(s)[0] == 192 && s.next_count(192) == 112);   // the first pass keeps its size
    }
    {
        ChainSchedule s = base;
        s.main_sz = 256;
        s.observe(1.0, 0.0, true, 256);
        CHECK(s.main_sz == 256);   // cap: max_cnt
    }
    {
        ChainSchedule s = base;
        s.observe(1.0, 9.0, false, 192);   // 19 pages by proportion
        CHECK(s.main_sz == 64);    // floor
    }
    {
        ChainSchedule s = base;
        s.observe(1.0, 0.02, false, 192);   // inside the slack, but not early
        CHECK(s.main_sz == 192);
        s.observe(1.0, 1.0, false, 191);    // a short last search
        CHECK(s.main_sz == 192);
        s.observe(0.0, 1.0, false, 192);    // no search time
        CHECK(s.main_sz == 192);
        s.adaptive = false;
        auto r = s.observe(1.0, 1.0, false, 192);
        CHECK(s.main_sz == 192 && r.first == 192 && r.second == 192);
    }

    // which kernel searches: len 3508, 192 pages beside a 192-page body (NL-means 0.8352 s)
    {
        const std::vector<unsigned> light(1024, 100000u);   // 192 * 100000 * 5.5 ns = 0.1056 s <= 0.4176 s
        CHECK(base.prefers_mw(light, 192, 192, 192, 3508));
        CHECK(!base.prefers_mw(text1024, 192, 192, 192, 3508));   // 0.887 s
        std::vector<unsigned> one_heavy = light;
        one_heavy[200] = 700000u;   // 0.42 s alone
        CHECK(!base.prefers_mw(one_heavy, 192, 192, 192, 3508));
        CHECK(base.prefers_mw(one_heavy, 0, 192, 192, 3508));
        CHECK(!base.prefers_mw(std::vector<unsigned>(), 192, 192, 192, 3508));
        CHECK(!base.prefers_mw(light, 192, 192, 0, 3508));
        CHECK(!ChainSchedule(1024, 1024, true, false, 2, 0, 0).prefers_mw(light, 192, 192, 192, 3508));
        CHECK(!ChainSchedule(1024, 1024, true, true, 1, 0, 0).prefers_mw(light, 192, 192, 192, 3508));
    }
    std::printf("chain_schedule: %s\n", bad == 0 ? "OK" : "FAILED");
    return bad == 0 ? 0 : 1;
}
