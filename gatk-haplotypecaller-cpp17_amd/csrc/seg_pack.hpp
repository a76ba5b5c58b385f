// Wave packing of one task's segment of the sorted segmented pairs (planner.cpp
// pack_seg_waves). Plain C++ with no engine header, so tests/cpp/seg_pack_main.cpp
// builds it alone under the sanitizers.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

namespace hcphmm {
namespace eng {

// Packs entries [0, m) of a list sorted by (BC, steps = R + nb - 1) descending
// into waves of one width on at most 64 lanes. rec[k] = BC | nb << 8 | R << 16,
// in[k] the entry's pair id, minnb[bc] the smallest nb of width bc in the whole
// part, used[k] zero on entry. Pair ids go to ordo[slot_n ...] in slot order,
// the waves (slot0, ncols, npairs, rmax, rmin, nsteps) to the end of W.
template <typename Wave>
void pack_segment(const uint32_t* __restrict rec, const int* __restrict in, int64_t m, const uint8_t* minnb,
                  uint8_t* __restrict used, int* __restrict ordo, int64_t slot_n, std::vector<Wave>& W)
{
    constexpr int64_t kLook = 64;
    // Knapsack over the free lanes: best[kLook + c] is the largest
    // sum of nb * steps of the items seen so far on at most c lanes
    // (entries below kLook stand for c < 0), take[k][c] whether
    // item k raised it. Fixed trip counts, so the loops vectorise.
    constexpr int32_t kNever = -(1 << 30);
    int32_t bufa[2 * kLook], bufb[2 * kLook];
    std::fill(bufa, bufa + kLook, kNever);
    std::fill(bufb, bufb + kLook, kNever);
    uint8_t take[kLook][kLook];
    int item_j[kLook], item_nb[kLook];
    for (int64_t i = 0; i < m; ++i) {
        if (used[i]) continue;
        const int bc = int(rec[i] & 0xff);
        Wave w{};
        w.slot0 = int(slot_n);
        w.ncols = bc;
        int rmin = INT32_MAX, rmax = 0, nst = 0, np = 0;
        auto put = [&](int64_t j) {
            const uint32_t r = rec[j];
            const int nb = int((r >> 8) & 0xff), R = int(r >> 16);
            used[j] = 1;
            ordo[slot_n++] = in[j];
            ++np;
            rmax = R > rmax ? R : rmax;
            rmin = R < rmin ? R : rmin;
            nst = R + nb - 1 > nst ? R + nb - 1 : nst;
        };
        // The first unused pair opens the wave: no later entry of
        // the sorted list runs more steps, so none lengthens it.
        put(i);
        const int cap = 64 - int((rec[i] >> 8) & 0xff);
        if (cap >= minnb[size_t(bc)]) {
            // Of the unused pairs of this width in the window, the
            // subset on at most cap lanes with the largest sum of
            // nb * steps: in effect full lanes first, then the longest pairs.
            // Only the first cap / nb pairs of one nb can matter.
            uint8_t seen[kLook + 1] = {};
            int32_t* cur = bufa + kLook;
            int32_t* nxt = bufb + kLook;
            std::fill(cur, cur + kLook, 0);
            int n = 0;
            const int64_t jend = std::min(m, i + kLook);
            for (int64_t j = i + 1; j < jend; ++j) {
                if (used[j]) continue;
                const uint32_t r = rec[j];
                if (int(r & 0xff) != bc) break;
                const int nb = int((r >> 8) & 0xff);
                if (nb > cap || (seen[nb] + 1) * nb > cap) continue;
                ++seen[nb];
                const int32_t v = int32_t(nb) * (int32_t(r >> 16) + nb - 1);
                const int32_t* __restrict from = cur - nb;
                const int32_t* __restrict keep = cur;
                int32_t* __restrict to = nxt;
                uint8_t* __restrict tk = take[n];
                for (int c = 0; c < int(kLook); ++c) {
                    const int32_t with = from[c] + v;
                    const bool t = with > keep[c];   // ties stay with the earlier pairs
                    tk[c] = t;
                    to[c] = t ? with : keep[c];
                }
                std::swap(cur, nxt);
                item_j[n] = int(j - i);
                item_nb[n] = nb;
                ++n;
                // No later pair runs more steps than this one, so
                // they add at most `steps` per lane still free:
                // once no fill can pass best[cap] that way, the
                // rest of the window changes nothing.
                if (n % 4 == 0) {
                    const int32_t steps = int32_t(r >> 16) + nb - 1;
                    const int32_t* __restrict at = cur;
                    int32_t bound = 0;
                    for (int c = 0; c <= cap; ++c) {
                        const int32_t x = at[c] + (cap - c) * steps;
                        bound = x > bound ? x : bound;
                    }
                    if (bound <= cur[cap]) break;
                }
            }
            int c = cap, nsel = 0, sel[kLook];
            for (int k = n - 1; k >= 0; --k)
                if (take[k][c]) {
                    sel[nsel++] = item_j[k];
                    c -= item_nb[k];
                }
            for (int k = nsel - 1; k >= 0; --k) put(i + sel[k]);
        }
        w.npairs = np;
        w.rmax = rmax;
        w.rmin = rmin;
        w.nsteps = nst;
        W.push_back(w);
    }
}

}  // namespace eng
}  // namespace hcphmm
