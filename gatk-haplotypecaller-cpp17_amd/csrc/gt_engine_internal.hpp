// What gt_engine.cpp shares with region_engine.cpp: the genotyper's stream and
// lock, its argument checks, the CIGAR parser, the arithmetic launch and the
// materialisation of hc_gt_call_site records. One definition each, in
// gt_engine.cpp; hc_gt_call_regions and hc_region_call both go through them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_gt.h"
#include "gt_kernels.hpp"
#include "gt_plan_kernels.hpp"

namespace hcgt_host {

// Serialises every genotyper entry point; held for the whole of a call.
std::mutex& mutex();
// With the lock held: engine initialised, primary device current, stream and Jacobian table ready.
int ensure_init();
hipStream_t stream();
hipError_t launch_arithmetic(hcgt::GtArgs& a);

// The HC_PHMM_EINVAL cases of a region and of a haplotype, with their messages.
int check_region_frame(const std::string& at, bool null_pointer, int32_t ref_len, int32_t n_haps, int32_t n_reads,
                       int64_t padded_begin, int64_t origin_begin, int64_t origin_end);
int check_hap_frame(const std::string& hat, bool null_pointer, int32_t length, int32_t alignment_begin, int32_t ref_len);
// Parses and checks one haplotype's CIGAR text (appends to runs); 0 or HC_PHMM_EINVAL with the message set.
int parse_hap_cigar(const std::string& hat, const char* cigar, int32_t alignment_begin, int32_t length, int32_t ref_len,
                    std::vector<hcgt::PlanRun>& runs);

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
