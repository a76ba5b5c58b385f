/*
 * hc_region.h — C ABI of the MI355X region caller (in libhcpairhmm.so).
 *
 * One call for the compute of HaplotypeCaller::call_region
 * (src/haplotypecaller/haplotypecaller.hpp:83-107) behind the assembler, for
 * many regions at once:
 *
 *   haplotypes vs the region's window   the aligner of hc_sw.h (graph_wrapper.hpp:232-240),
 *                                       NEW_SW_PARAMETERS, soft-clipped overhangs, all-match
 *                                       shortcut: what hc::MI355XSWAligner::align_haplotypes does
 *   reads x haplotypes                  the PairHMM of hc_pairhmm.h, then
 *                                       normalize_likelihoods_and_filter_poorly_modeled_reads
 *                                       (pairhmm/intel_pairhmm.hpp:24-46)
 *   assign_genotype_likelihoods         the genotyper of hc_gt.h on the kept reads
 *
 * The results are those of hc_sw_align_flat, hc_phmm_compute_likelihoods per
 * region and hc_gt_call_regions on the kept reads, bit for bit. The two
 * hand-offs stay on the device: the aligner's CIGAR elements become the
 * genotyper's runs without passing through text, and the matrices are capped,
 * filtered and compacted where the genotyper reads them. The aligner, the event
 * bookkeeping and the site count run while the PairHMM pass is in flight.
 *
 * Status codes are the HC_PHMM_* codes of hc_pairhmm.h; message via
 * hc_phmm_last_error(). Invalid input is HC_PHMM_EINVAL with the messages of the
 * three separate calls. No CPU fallback. Thread safety and device are those of
 * hc_gt_call_regions (calls are serialised; the engine's primary device); the
 * PairHMM pass shards over the configured device slots by its own rules.
 */
#ifndef HC_REGION_H
#define HC_REGION_H

#include <stdint.h>

#include "hc_gt.h"
#include "hc_pairhmm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hc_region_hap {
    const uint8_t* bases;
    int32_t length;            /* 1 .. HC_GT_MAX_HAP_LEN */
    int32_t alignment_begin;   /* used only when cigar != NULL */
    const char* cigar;         /* NULL: align on the device against the region's window */
} hc_region_hap;

typedef struct hc_region_in {
    const uint8_t* ref;        /* limits of hc_gt_region */
    int32_t ref_len;
    int64_t padded_begin, origin_begin, origin_end;
    const hc_region_hap* haps; /* a region's cigars are all NULL or none is: mixed is HC_PHMM_EINVAL */
    int32_t n_haps;            /* 1 .. HC_GT_MAX_HAPS */
    const hc_phmm_read* reads; /* as hc_phmm_compute_likelihoods takes them */
    const int64_t* read_begin; /* read intervals [begin, end), contig coordinates */
    const int64_t* read_end;
    int32_t n_reads;           /* >= 0 */
} hc_region_in;

/* flags of hc_region_call. Bit 0 is HC_PHMM_FLAG_F64 itself, passed to the PairHMM. */
#define HC_REGION_F64 1u              /* = HC_PHMM_FLAG_F64: this call's PairHMM computes in fp64 only */
#define HC_REGION_DEFAULT_MODE 2u     /* take the PairHMM mode from the process default (hc_phmm_init) instead */
#define HC_REGION_WANT_L 16u          /* return the normalised matrices of the kept reads */
#define HC_REGION_WANT_SITE_READS 32u /* fill hc_gt_call_site.keep / n_keep; otherwise NULL / 0 */
#define HC_REGION_WANT_CIGARS 64u     /* return alignment_begin + CIGAR text of device-aligned haplotypes */

typedef struct hc_region_calls hc_region_calls;

/* One synchronous call. On success *out holds the results of every region;
 * release it with hc_region_calls_free. All pointers the accessors return are
 * owned by the handle. */
int hc_region_call(const hc_region_in* regions, int32_t n_regions, uint32_t flags, hc_region_calls** out);
/* Every in-origin site, in region order then ascending begin (hc_gt_calls_sites).
 * keep indexes the region's kept reads, in their order. */
int hc_region_calls_sites(const hc_region_calls* calls, const hc_gt_call_site** sites, int64_t* n);
/* keep[r] = 1 for the reads of `region` that survive the filter (the caller erases the others). */
int hc_region_calls_reads(const hc_region_calls* calls, int32_t region, const uint8_t** keep, int32_t* n_reads,
                          int32_t* n_kept);
/* HC_REGION_WANT_L: n_kept x n_haps, read-major, capped. HC_PHMM_EINVAL without the flag. */
int hc_region_calls_matrix(const hc_region_calls* calls, int32_t region, const double** L, int32_t* n_kept,
                           int32_t* n_haps);
/* HC_REGION_WANT_CIGARS: the alignment of a haplotype that arrived without a CIGAR.
 * HC_PHMM_EINVAL without the flag or for a haplotype that brought its own. */
int hc_region_calls_alignment(const hc_region_calls* calls, int32_t region, int32_t hap, int32_t* begin,
                              const char** cigar);
int hc_region_calls_free(hc_region_calls* calls);

#ifdef __cplusplus
}
#endif
#endif /* HC_REGION_H */
