// What the sorted buckets of the genome caller (include/hc_genome.h,
// HC_GENOME_SORTED_BUCKETS) decide per element, written once for the device and
// the host: the digit of a pass, the number of passes, where an element of a
// tile goes (its rank among the tile's earlier elements with the same digit),
// the head of a run of equal keys, a position with too many reads and the lower
// bound over the run table. genome_sort_kernels.hip makes the eight bit masks of
// a wave's digits by __ballot; with SAMX_HOST_ONLY (no HIP header)
// tests/cpp/genome_sort_host_main.cpp makes them with a loop over 64 elements
// and runs the same functions under the host sanitizers.
//
// The sort. Least significant digit first, 8 bits per pass, stable. A tile is
// kSortTile consecutive elements, taken in kSortRounds rounds of kSortBlock
// (kSortWaves waves of 64 lanes). Per pass the histogram holds, digit-major,
// hist[digit * n_tiles + tile] = the tile's elements with that digit; its
// exclusive scan is where the tile's first element with that digit goes. Inside
// the tile an element follows the earlier rounds' (a running count per digit),
// the earlier waves' of its round (a count per wave and digit) and the lower
// lanes' of its wave (the popcount of the match mask below its lane). Nothing
// depends on the order in which waves or workgroups run.
//
// The keys. A placed read's is off[contig] + POS - 1, an unplaced one's is
// total_len, which sorts behind every position; both are below 2^63.
#pragma once
#include "sam_body.hpp"

namespace hcgenome {

constexpr int kSortDigits = 256, kSortWaves = 4, kSortBlock = 64 * kSortWaves, kSortRounds = 8;
constexpr int kSortTile = kSortBlock * kSortRounds;

SAMX_FN inline int64_t sort_tiles(int64_t n) { return (n + kSortTile - 1) / kSortTile; }

SAMX_FN inline uint32_t sort_digit(int64_t key, int pass) { return uint32_t(uint64_t(key) >> (8 * pass)) & 255u; }

// Passes that cover every bit of the value total_len itself (the key of an unplaced read), at least one.
SAMX_FN inline int sort_passes(int64_t total_len)
{
    int bits = 1;
    while (bits < 63 && (uint64_t(total_len) >> bits) != 0) ++bits;
    return (bits + 7) / 8;
}

SAMX_FN inline int sort_popc(uint64_t m) { return __builtin_popcountll(m); }

// The lanes of a wave whose digit equals `digit`: bit[b] is the mask of the
// lanes whose digit has bit b set, `valid` the mask of the lanes that hold an element.
SAMX_FN inline uint64_t sort_match(const uint64_t* bit, uint32_t digit, uint64_t valid)
{
    uint64_t m = valid;
    for (int b = 0; b < 8; ++b) m &= ((digit >> b) & 1u) ? bit[b] : ~bit[b];
    return m;
}

// The rank of lane `lane`'s element among its tile's earlier elements with the
// same digit: `running` counts the earlier rounds', wave_count[k * kSortDigits +
// digit] wave k's of this round, `match` is sort_match of the lane's own wave.
SAMX_FN inline int32_t sort_rank(int32_t running, const int32_t* wave_count, int wave, uint32_t digit, uint64_t match, int lane)
{
    int32_t r = running;
    for (int k = 0; k < wave; ++k) r += wave_count[k * kSortDigits + int(digit)];
    return r + sort_popc(match & ((uint64_t(1) << lane) - 1u));
}

// Element i of the sorted keys begins a run: a placed read whose key differs from the one before.
SAMX_FN inline bool sort_head(const int64_t* key, int64_t i, int64_t total_len)
{
    return key[i] < total_len && (i == 0 || key[i] != key[i - 1]);
}

// Element i is read number max_reads + 1 or later of its position.
SAMX_FN inline bool sort_too_deep(const int64_t* key, int64_t i, int64_t total_len, int64_t max_reads)
{
    return key[i] < total_len && i >= max_reads && key[i - max_reads] == key[i];
}

// Element i is the last placed read.
SAMX_FN inline bool sort_last_placed(const int64_t* key, int64_t i, int64_t n, int64_t total_len)
{
    return key[i] < total_len && (i == n - 1 || key[i + 1] >= total_len);
}

// The first run at or behind `key`: the least r in [0, n] with r == n or run_pos[r] >= key.
SAMX_FN inline int64_t sort_lower_bound(const int64_t* run_pos, int64_t n, int64_t key)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (run_pos[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace hcgenome
