// What gt_engine.cpp shares with region_engine.cpp: the genotyper's stage (stream
// and lock), the frame of a region (its checks, its PlanRegion, the running totals
// and their INT32 bound), the haplotype checks and the CIGAR parser, PlanArgs
// and GtArgs from offsets, the arithmetic launch and the materialisation of
// hc_gt_call_site records. One definition each, in gt_engine.cpp;
// hc_gt_call_regions and hc_region_call both go through them. The per-haplotype
// loop and the workspace layouts stay with the callers, where they differ. The
// plumbing under both (buffers, carver, HIP_TRY) is stage_host.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/hc_gt.h"
#include "gt_kernels.hpp"
#include "gt_plan_kernels.hpp"
#include "stage_host.hpp"

namespace hcgt_host {

// The genotyper's stage: its lock serialises every genotyper and region caller entry
// point, and ensure_init() leaves stream and Jacobian table ready.
stage_host::Stage& stage();
hipError_t launch_arithmetic(hcgt::GtArgs& a);

// What a region caller's input says about one region, whatever its record type.
struct RegionFrame {
    bool null_pointer;   // any of the pointers the entry point requires
    int32_t ref_len, n_haps, n_reads;
    int64_t padded_begin, origin_begin, origin_end;
};

// Running totals over the regions of a call; they size workspace 1 and bound workspace 2.
struct FrameTotals {
    int64_t ref = 0, reads = 0, L = 0, tab = 0;
    int64_t keep_bound = 0, map_bound = 0, site_bound = 0;
};

// Region r of a call, in the order errors are reported: checks the frame
// (HC_PHMM_EINVAL with its message), fills d from the totals so far, runs the
// caller's haplotype part, advances the totals and checks that every offset of
// the call still fits INT32. haps(at) appends the region's PlanHap records to ph
// (haplotype h has tab_off = t.tab + h * ref_len), its bases to hap_pool and its
// host-parsed runs to runs, and returns its own error or 0.
int add_region(int32_t r, const RegionFrame& f, FrameTotals& t, hcgt::PlanRegion& d,
               const std::function<int(const std::string& at)>& haps, const std::vector<hcgt::PlanHap>& ph,
               const std::string& hap_pool, const std::vector<hcgt::PlanRun>& runs);

// The HC_PHMM_EINVAL cases of a haplotype, with their messages.
int check_hap_frame(const std::string& hat, bool null_pointer, int32_t length, int32_t alignment_begin, int32_t ref_len);
// Parses and checks one haplotype's CIGAR text (appends to runs); 0 or HC_PHMM_EINVAL with the message set.
int parse_hap_cigar(const std::string& hat, const char* cigar, int32_t alignment_begin, int32_t length, int32_t ref_len,
                    std::vector<hcgt::PlanRun>& runs);

// Offsets of the plan kernels' arrays in workspace 1, as the callers carve them.
struct PlanOffsets {
    size_t reg, hap, runs, ref, pool, read_begin, read_end, bitmap, base, totals, ev, span;
};
// PlanArgs of the events and scan kernels (site_out, gt_sites, keep and amap come with workspace 2).
hcgt::PlanArgs plan_args(char* base, const PlanOffsets& o, int32_t n_regions, size_t n_haps);
// GtArgs of the sites a plan wrote: sites, keep and amap are the plan's.
hcgt::GtArgs gt_args(const hcgt::PlanArgs& p, int64_t n_sites, const double* L, double* al, double* gl, int32_t* gi,
                     int32_t* gq);

// The records of a call and what they point into.
struct Calls {
    std::vector<hc_gt_call_site> sites;
    std::vector<char> text;          // allele strings, NUL-terminated
    std::vector<const char*> ptrs;   // per site, n_alleles pointers into text
    std::vector<int32_t> ints;       // the downloaded keep and hap_allele blocks
    std::vector<double> gl;
};

struct RegionView {
    const uint8_t* ref;
    int64_t padded_begin;
    int32_t n_haps;
};

// Builds out.sites from the downloaded blocks. keep == nullptr: the records get
// keep = NULL and n_keep = 0 (the lists were not read back).
void materialise(const RegionView* regions, const char* hap_pool, const hcgt::SiteOut* so, int64_t ns, const double* gl,
                 const int32_t* gi, const int32_t* gq, const int32_t* keep, int64_t keep_cap, const int32_t* amap,
                 int64_t map_cap, Calls& out);

}  // namespace hcgt_host
