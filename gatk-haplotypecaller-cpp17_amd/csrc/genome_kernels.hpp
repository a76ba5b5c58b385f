// Device side of the genome caller (include/hc_genome.h): the launch record
// shared by genome_kernels.hip and genome_engine.cpp. The pick function and the
// error word are the contig caller's (contig_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "contig_kernels.hpp"
#include "genome_body.hpp"

namespace hcgenome {

using hccontig::kErrDefect;
using hccontig::kErrDepth;
using hccontig::kErrUnplaced;
using hccontig::kNoError;
using hccontig::kWavesPerBlock;

// As hccontig::ContigArgs, over the concatenated position space: position p of
// contig c is off[c] + p, and kErrDepth is keyed by that position plus one.
struct GenomeArgs {
    const hc_sam_record* records;
    const int32_t* line_no;
    int32_t n_records;
    const uint8_t* text;       // the SAM text on the device
    int64_t text_len;
    GenomeTable table;
    int32_t n_contigs;
    const int64_t* ref_len;    // per contig
    const int64_t* off;        // n_contigs + 1: the exclusive sum of ref_len
    const int64_t* win_off;    // n_contigs + 1: the exclusive sum of the window counts
    int32_t* contig_of;        // per record: its RNAME's index in the table, or -1
    int32_t skip_unplaced;
    int64_t total_len;         // off[n_contigs]
    int32_t* count;            // per position: the reads that begin there (zeroed before the call)
    const int64_t* first;      // its exclusive scan
    int32_t* cursor;           // per position, zeroed: the scatter's arrival counter
    int32_t* bucket;           // per placed read: record indices, position-major, file order after the sort
    int32_t n_windows;         // win_off[n_contigs]
    int64_t region, padding;
    uint64_t seed;
    int32_t pick_mode;
    int32_t* n_picked;         // per window
    const int64_t* win_first;  // its exclusive scan
    int32_t* picked;           // per pick: record indices, window-major, ascending position
    unsigned long long* err;
    // Of an interval call (interval_kernels.hpp); null in a plain call.
    const int32_t* scope;      // per record: 0 keeps it out of the buckets and raises no error. Null: every record.
    const int32_t* asked_list; // the windows that pick, ascending; the others' n_picked is zeroed beforehand. Null: every window.
    int32_t n_asked;           // their number; n_windows without a list
};

// The window of pick wave i (0 <= i < n_asked).
__host__ __device__ inline int64_t genome_pick_window(const GenomeArgs& a, int64_t i) { return a.asked_list ? a.asked_list[i] : i; }

hipError_t launch_resolve(const GenomeArgs& a, hipStream_t st);
hipError_t launch_place(const GenomeArgs& a, hipStream_t st);
hipError_t launch_scatter(const GenomeArgs& a, hipStream_t st);
hipError_t launch_sort(const GenomeArgs& a, hipStream_t st);
hipError_t launch_pick_count(const GenomeArgs& a, hipStream_t st);
hipError_t launch_pick_write(const GenomeArgs& a, hipStream_t st);

}  // namespace hcgenome
