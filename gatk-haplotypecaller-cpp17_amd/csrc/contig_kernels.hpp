// Device side of the contig caller (include/hc_contig.h): the launch record
// shared by contig_kernels.hip and contig_engine.cpp, and the pick function.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/hc_contig.h"

namespace hccontig {

constexpr int kWavesPerBlock = 4;   // one wave per window

// The error word is min over offending reads of (1-based line) * 16 + code.
// kErrDepth is keyed by the 1-based position in the place of the line.
enum ContigError : int32_t { kErrNone = 0, kErrUnplaced = 1, kErrDefect = 2, kErrDepth = 3 };
constexpr unsigned long long kNoError = ~0ull;

struct ContigArgs {
    const hc_sam_record* records;
    const int32_t* line_no;
    int32_t n_records;
    int64_t ref_len;
    int32_t skip_unplaced;
    int32_t* count;            // per position: the reads that begin there (zeroed before the call)
    const int64_t* first;      // its exclusive scan
    int32_t* cursor;           // per position, zeroed: the scatter's arrival counter
    int32_t* bucket;           // per placed read: record indices, position-major, file order after the sort
    int32_t n_windows;
    int64_t region, padding;
    uint64_t seed;
    int32_t pick_mode;
    int32_t* n_picked;         // per window
    const int64_t* win_first;  // its exclusive scan
    int32_t* picked;           // per pick: record indices, window-major, ascending position
    unsigned long long* err;
};

// include/hc_contig.h, "The pick".
__host__ __device__ inline uint32_t pick_index(uint64_t seed, uint64_t window, uint64_t begin, uint32_t count, int32_t mode)
{
    if (mode == HC_CONTIG_PICK_FIRST) return 0u;
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((window << 32) + begin + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return uint32_t(((z >> 32) * uint64_t(count)) >> 32);
}

hipError_t launch_place(const ContigArgs& a, hipStream_t st);
hipError_t launch_scatter(const ContigArgs& a, hipStream_t st);
hipError_t launch_sort(const ContigArgs& a, hipStream_t st);
hipError_t launch_pick_count(const ContigArgs& a, hipStream_t st);
hipError_t launch_pick_write(const ContigArgs& a, hipStream_t st);

}  // namespace hccontig
