// Device hand-offs of the region caller (region_kernels.hip / region_engine.cpp):
// the aligner's CIGAR elements become the genotyper's runs, and the PairHMM's
// log10 matrices are normalised, filtered and compacted, without a host step.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gt_plan_kernels.hpp"
#include "sw_kernels.hpp"

namespace hcregion {

constexpr int kMaxRuns = 2048;   // a haplotype has fewer runs (ev / span hold run ids as int16)

// Bits of the device error word (RunsArgs::err).
enum : uint32_t {
    kErrOp = 1u,       // an element with an operator other than M I D S
    kErrHapLen = 2u,   // the runs do not consume the haplotype exactly
    kErrRefEnd = 4u,   // the runs start outside or run past the window
    kErrCount = 8u,    // no run at all, or kMaxRuns and more
};

struct RunsArgs {
    const hcsw::SwPair* pairs;
    const int32_t* pair_hap;      // pair p aligns haplotype pair_hap[p] of the call
    const hcsw::SwResult* res;
    const uint32_t* elems;        // the aligner's scratch: (len << 4) | op, CIGAR end first
    const uint16_t* slots;        // what the trace kernel leaves for a shortcut pair
    const int32_t* n_elems;
    const int32_t* offsets;
    int n;
    hcgt::PlanRun* runs;          // haplotype p's runs start at pairs[p].el_off
    hcgt::PlanHap* haps;          // run_off / n_runs are written here
    uint32_t* err;
};

struct FinishArgs {
    hcgt::PlanRegion* regions;    // n_reads becomes the kept count
    int n_regions;
    int n_reads;                  // of all regions
    const int32_t* read_len;
    double* L;                    // log10 matrices; capped in place
    const int64_t* read_begin;
    const int64_t* read_end;
    double* L_out;                // kept rows, compact, at the region's L_off
    int64_t* begin_out;           // kept reads' intervals, compact, at the region's read_off
    int64_t* end_out;
    uint8_t* keep;                // per read
    int32_t* dest;                // per read: row among the region's kept reads, or -1
    int32_t* n_kept;              // per region
};

hipError_t launch_runs(const RunsArgs& a, hipStream_t s);
hipError_t launch_finish(const FinishArgs& a, hipStream_t s);

}  // namespace hcregion
