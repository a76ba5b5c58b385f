// Device side of the interval calls (include/hc_intervals.h): the launch record
// shared by interval_kernels.hip and genome_engine.cpp. The decisions are
// interval_body.hpp's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "genome_kernels.hpp"
#include "interval_body.hpp"

namespace hcgenome {

// `g` is the genome caller's record: the table, the records and contig_of.
struct IntervalArgs {
    GenomeArgs g;
    IntervalSet set;           // the merged intervals on the device
    int32_t* asked;            // per genome-wide window: 1 when asked
    int64_t* asked_first;      // its exclusive scan, n_windows + 1
    int32_t* asked_list;       // the asked windows, ascending; asked_first[n_windows] of them
    int32_t* scope;            // per record: 1 when in scope
    int64_t* scope_first;      // its exclusive scan, n_records + 1
    int32_t* scoped_list;      // the records in scope, ascending; scope_first[n_records] of them
    int64_t* scan_work;        // hcsam::scan_work_bytes of the longer scan
};

// asked, asked_first and asked_list.
hipError_t launch_interval_ask(const IntervalArgs& a, hipStream_t st);
// scope, scope_first and scoped_list (behind the resolve).
hipError_t launch_interval_scope(const IntervalArgs& a, hipStream_t st);

}  // namespace hcgenome
