// Genotyper event bookkeeping on the device (gt_plan_kernels.hip / gt_engine.cpp):
// events per haplotype, sites per region, then alleles, haplotype -> allele maps
// and kept reads per site, written as the GtSite records gt_sites_kernel reads.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "gt_kernels.hpp"

namespace hcgt {

constexpr int kMaxRefLen = 1023;     // HC_GT_MAX_REF_LEN
constexpr int kMaxHaps = 128;        // HC_GT_MAX_HAPS
constexpr int kBitmapWords = 32;     // one bit per window position
constexpr int kMaxGenotypes = 28;    // out_off stride of a site

enum : int32_t { kOpM = 0, kOpI = 1, kOpD = 2, kOpS = 3 };
// Alt kinds; kAltStar is a spanning deletion (or an ALT that is the text "*").
enum : int32_t { kAltNone = 0, kAltSnp = 1, kAltIns = 2, kAltDel = 3, kAltStar = 4 };

struct PlanRun {          // one CIGAR run with its start positions (host prefix sums)
    int32_t len, op;
    int32_t ref_pos;      // window coordinate
    int32_t hap_pos;
};

struct PlanHap {
    int32_t region;
    int32_t base_off;     // first base in the haplotype pool
    int32_t run_off, n_runs;
    int32_t tab_off;      // first entry of this haplotype's position tables
};

struct PlanRegion {
    int64_t padded_begin, origin_begin, origin_end;
    int64_t L_off;        // first double of the region's matrix
    int32_t ref_off, ref_len;
    int32_t hap0, n_haps;
    int32_t read_off, n_reads;
};

struct PlanBase {         // per region, written by the scan
    int32_t site_base, n_sites;
    int32_t map_base;
    int32_t pad;
    int64_t keep_base;
};

struct PlanTotals {
    int64_t n_sites, keep_cap, map_cap;
};

struct AltDesc {          // an alt allele as kind + own bytes; the tail is reference text
    int32_t kind, len, hap_off;
};

struct SiteOut {
    int32_t region, pos;
    int32_t ref_len;      // length of the reference allele; loc_end = begin + ref_len
    int32_t n_alleles;    // kMaxAlleles + 1: skipped
    int32_t n_keep, keep_off, map_off, pad;
    AltDesc alt[kMaxAlleles - 1];
};

struct PlanArgs {
    const PlanRegion* regions;
    int n_regions;
    const PlanHap* haps;
    int n_haps;
    const PlanRun* runs;
    const uint8_t* ref;        // reference pool
    const uint8_t* hap;        // haplotype pool
    const int64_t* read_begin;
    const int64_t* read_end;
    int16_t* ev;               // per haplotype x position: run owning the event that begins there, or -1
    int16_t* span;             // per haplotype x position: deletion run covering it from an earlier begin, or -1
    uint32_t* bitmap;          // n_regions x kBitmapWords, zeroed before the events kernel
    PlanBase* base;
    PlanTotals* totals;
    // sized by the counted readback of totals:
    SiteOut* site_out;
    GtSite* gt_sites;
    int32_t* keep;
    int32_t* amap;
};

hipError_t launch_plan_events(const PlanArgs& a, hipStream_t s);   // events, scan (through totals)
hipError_t launch_plan_sites(const PlanArgs& a, int64_t n_sites, hipStream_t s);

}  // namespace hcgt
