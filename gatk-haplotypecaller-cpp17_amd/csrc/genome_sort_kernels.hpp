// Device side of the genome caller's sorted buckets (include/hc_genome.h,
// HC_GENOME_SORTED_BUCKETS): the launch record shared by genome_sort_kernels.hip
// and genome_engine.cpp. Nothing here is sized by the contigs' bases.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "genome_kernels.hpp"
#include "genome_sort_body.hpp"

namespace hcgenome {

// `g` is the dense path's record with count, first, cursor and bucket unused.
// n elements are sorted: every record (scoped null, n = g.n_records), or the
// records of an interval call's scoped list, which ascends, so that the reads of
// a position stay in file order. tiles = sort_tiles(n). key[0] is the buffer the keys are made
// in; the sort leaves its result in key[passes & 1] / index[passes & 1], and the
// other pair is free from then on: its keys hold run_of, its indices the head flags.
struct GenomeSortArgs {
    GenomeArgs g;
    int32_t n;               // the elements
    const int32_t* scoped;   // n record indices, ascending, or null
    int64_t* key[2];      // n + 1 each
    int32_t* index[2];    // n each
    int32_t* hist;        // kSortDigits * tiles, digit-major
    int64_t* hist_first;  // its exclusive scan, kSortDigits * tiles + 1
    int64_t* scan_work;   // hcsam::scan_work_bytes of the longest scan
    int64_t* run_pos;     // per run: its key, ascending
    int64_t* run_first;   // per run: its first element in the sorted order; n_runs + 1
    int32_t passes;       // sort_passes(g.total_len)
    // set by launch_sorted_buckets
    const int64_t* keys;      // sorted
    const int32_t* sorted;    // record indices in key order, file order within a key
    const int64_t* run_of;    // n + 1: the exclusive scan of the head flags; run_of[n] = the number of runs
};

// Keys, the passes of the sort and the run table. Fills keys, sorted and run_of.
hipError_t launch_sorted_buckets(GenomeSortArgs& a, hipStream_t st);
hipError_t launch_sorted_pick_count(const GenomeSortArgs& a, hipStream_t st);
hipError_t launch_sorted_pick_write(const GenomeSortArgs& a, hipStream_t st);

}  // namespace hcgenome
