// The planner's wave packing (csrc/seg_pack.hpp pack_segment) on its own, built
// with -fsanitize=address,undefined by tests/test_seg_pack_host.py: seeded
// lists of (BC, nb, R) records sorted as the planner sorts them, each packed
// and checked. Exit status 0 and "ok" on stdout when every list passes.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

#include "../../gatk-haplotypecaller-cpp17_amd/csrc/seg_pack.hpp"

namespace {

struct Wave {   // the six fields pack_segment fills (LaneWave has more)
    int slot0, rmax, rmin, ncols, npairs, nsteps;
};

struct Entry {
    int bc, nb, R, id;
    int steps() const { return R + nb - 1; }
};

#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::fprintf(stderr, "list %d (%zu entries): %s failed\n", list, v.size(), #cond); \
            return false;                                                                   \
        }                                                                                   \
    } while (0)

// kind 0: nb 1 .. 64 mixed; 1: every nb 64; 2: every nb 1.
bool run_list(int list, size_t n, int kind, std::mt19937& rng)
{
    auto draw = [&](int lo, int hi) { return int(lo + rng() % unsigned(hi - lo + 1)); };
    const int nwidths = draw(2, 3);
    int widths[3];
    for (int& w : widths) w = 2 * draw(4, 32);
    const int nb_hi = draw(0, 3) ? draw(2, 12) : 64;   // mostly the planner's few lanes per pair, sometimes any
    std::vector<Entry> v(n);
    for (size_t k = 0; k < n; ++k)
        v[k] = Entry{widths[draw(0, nwidths - 1)], kind == 1 ? 64 : kind == 2 ? 1 : draw(1, nb_hi), draw(1, 300), 0};
    std::stable_sort(v.begin(), v.end(), [](const Entry& a, const Entry& b) {
        return a.bc != b.bc ? a.bc > b.bc : a.steps() > b.steps();
    });
    // pair ids: a permutation, so a lost or doubled entry shows
    std::vector<int> ids(n);
    std::iota(ids.begin(), ids.end(), 0);
    std::shuffle(ids.begin(), ids.end(), rng);
    std::vector<uint32_t> rec(n);
    std::vector<uint8_t> minnb(65, 64), used(n, 0);
    for (size_t k = 0; k < n; ++k) {
        v[k].id = ids[k];
        rec[k] = uint32_t(v[k].bc) | uint32_t(v[k].nb) << 8 | uint32_t(v[k].R) << 16;
        minnb[size_t(v[k].bc)] = std::min<uint8_t>(minnb[size_t(v[k].bc)], uint8_t(v[k].nb));
    }
    // as a task's segment in the planner: the order array is the part's, its slots start at `base`
    const int64_t base = draw(0, 5);
    std::vector<int> ordo(size_t(base) + n, -7);
    std::vector<Wave> W;
    hcphmm::eng::pack_segment(rec.data(), ids.data(), int64_t(n), minnb.data(), used.data(), ordo.data(), base, W);

    std::vector<const Entry*> by_id(n);
    for (const Entry& e : v) by_id[size_t(e.id)] = &e;
    std::vector<int> seen(n, 0);
    for (int64_t k = 0; k < base; ++k) CHECK(ordo[size_t(k)] == -7);
    for (size_t k = 0; k < n; ++k) {
        CHECK(used[k] == 1);
        const int id = ordo[size_t(base) + k];
        CHECK(id >= 0 && size_t(id) < n);
        ++seen[size_t(id)];
    }
    for (size_t k = 0; k < n; ++k) CHECK(seen[k] == 1);   // every entry placed exactly once
    int64_t slot = base;
    for (const Wave& w : W) {
        CHECK(w.slot0 == slot && w.npairs >= 1);
        CHECK(slot + w.npairs <= base + int64_t(n));
        int lanes = 0, rmax = 0, rmin = INT32_MAX;
        for (int k = 0; k < w.npairs; ++k) {
            const Entry& e = *by_id[size_t(ordo[size_t(slot + k)])];
            CHECK(e.bc == w.ncols);   // one width per wave
            lanes += e.nb;
            rmax = std::max(rmax, e.R);
            rmin = std::min(rmin, e.R);
            CHECK(e.steps() <= w.nsteps);
        }
        CHECK(lanes <= 64);
        CHECK(w.nsteps == by_id[size_t(ordo[size_t(slot)])]->steps());   // the first pair's
        CHECK(w.rmax == rmax && w.rmin == rmin);
        slot += w.npairs;
    }
    CHECK(slot == base + int64_t(n));
    return true;
}

}  // namespace

int main()
{
    std::mt19937 rng(20240611);
    for (int list = 0; list < 200; ++list) {
        // lists 0-2 of one entry, 3-5 every nb 64, 6-8 every nb 1, then mixed
        const int kind = list >= 3 && list < 6 ? 1 : list >= 6 && list < 9 ? 2 : 0;
        const size_t n = list < 3 ? 1 : list % 10 == 9 ? 3000 : size_t(1 + rng() % 3000);
        if (!run_list(list, n, kind, rng)) return 1;
    }
    std::puts("ok");
    return 0;
}
