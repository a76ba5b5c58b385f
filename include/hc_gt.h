/*
 * hc_gt.h — C ABI of the MI355X genotyper numeric core (in libhcpairhmm.so).
 *
 * Drop-in for the per-site likelihood arithmetic of
 * avis9ditiu/gatk-haplotypecaller-cpp17's Genetyper::assign_genotype_likelihoods
 * (src/haplotypecaller/genotyper/genotyper.hpp:369-399), for many sites at once:
 *
 *   marginalize / marginal_likelihoods            :245-274  allele likelihood of a read =
 *                                                            max over the haplotypes of the allele
 *   calculate_genotype_likelihoods                :276-328  per genotype (a1 <= a2), sum over reads
 *                                                            of log10(2)+L[a] or
 *                                                            MathUtils::approximate_log10_sum_log10
 *                                                            (utils/math_utils.hpp:11-33), minus
 *                                                            n_reads * log10(2)
 *   get_genotype_quality_and_max_genotype_index   :330-365  best genotype and its quality (<= 99)
 *
 * The caller keeps the event bookkeeping (set_events_for_haplotypes,
 * get_compatible_alleles, get_allele_mapper, get_read_indices_to_keep) and
 * passes, per site, the region's read-major likelihood matrix (the return value
 * of compute_likelihoods), the kept read indices, the haplotype -> allele map
 * (haplotype_mapper) and the allele count. Sites that share a matrix (one
 * region) share its upload. Results are bit-identical to the reference
 * arithmetic (sequential sums in read order, the Jacobian table as g++ folds it).
 *
 * Status codes are the HC_PHMM_* codes of hc_pairhmm.h; message via
 * hc_phmm_last_error(). No CPU fallback: without a gfx950 device the call fails.
 */
#ifndef HC_GT_H
#define HC_GT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HC_GT_MAX_ALLELES 7   /* Genetyper::MAX_ALLELE_COUNT (genotyper.hpp:19) */
#define HC_GT_MAX_GENOTYPES 28

typedef struct hc_gt_site {
    const double* L;              /* n_reads x n_haps, read-major (row r at L + r*n_haps) */
    int32_t n_reads;
    int32_t n_haps;
    const int32_t* keep;          /* n_keep read indices (< n_reads), in the reference's order */
    int32_t n_keep;
    const int32_t* hap_allele;    /* n_haps allele indices (< n_alleles) */
    int32_t n_alleles;            /* 2 .. HC_GT_MAX_ALLELES */
    double* genotype_likelihoods; /* out: n_alleles*(n_alleles+1)/2, genotype order a1 <= a2, a1-major */
    int32_t* genotype_index;      /* out: argmax (ties: the later index, :344-349) */
    int32_t* genotype_quality;    /* out: round(-10*(second - best)), capped at 99 */
} hc_gt_site;

int hc_gt_genotype_sites(const hc_gt_site* sites, int32_t n_sites);

/*
 * Whole drop-in for Genetyper::assign_genotype_likelihoods (:369-399): regions
 * in, called variants out. The event bookkeeping runs on the device in the same
 * pass as the arithmetic above:
 *
 *   process_cigar_for_initial_events  :35-111   SNP / insertion / deletion events of each
 *                                               haplotype's CIGAR; the first event in CIGAR
 *                                               order at a position wins (map emplace)
 *   set_events_for_haplotypes         :113-127  sites = ascending event begins in the origin
 *   get_events_from_haplotypes, replace_span_dels, get_compatible_alleles   :129-193
 *   get_allele_mapper, get_haplotype_mapper, get_read_indices_to_keep       :195-243
 *
 * The host only parses and validates the CIGAR text. Where the reference reads
 * out of bounds (a CIGAR that does not fit its haplotype or the window, an
 * origin outside the window) the call returns HC_PHMM_EINVAL instead; an
 * operator other than M I D S (the reference throws) is HC_PHMM_EINVAL too.
 */
#define HC_GT_MAX_REF_LEN 1023   /* = HC_SW_MAX_LEN1: the aligner's window limit */
#define HC_GT_MAX_HAP_LEN 1024   /* = HC_SW_MAX_LEN2 */
#define HC_GT_MAX_HAPS 128       /* per region; the reference's DEFAULT_NUM_PATHS */

/* hc_gt_call_site.status */
#define HC_GT_SITE_EMITTED 0           /* a variant of the reference's return value */
#define HC_GT_SITE_HOM_REF 1           /* best genotype is 0/0 (:392) */
#define HC_GT_SITE_LOW_QUALITY_HET 2   /* a1 == 0 and quality < 50 (:394) */
#define HC_GT_SITE_TOO_MANY_ALLELES 3  /* more than HC_GT_MAX_ALLELES alleles (:386) */

typedef struct hc_gt_hap_aln {
    const uint8_t* bases;
    int32_t length;           /* 1 .. HC_GT_MAX_HAP_LEN */
    int32_t alignment_begin;  /* alignment_begin_wrt_ref, in window coordinates */
    const char* cigar;        /* NUL-terminated "%d%c" runs of M I D S, as hc_sw writes them */
} hc_gt_hap_aln;

typedef struct hc_gt_region {
    const uint8_t* ref;       /* the padded region's reference window */
    int32_t ref_len;          /* 1 .. HC_GT_MAX_REF_LEN */
    int64_t padded_begin;     /* contig coordinate of ref[0], >= 0 */
    int64_t origin_begin;     /* padded_begin <= origin_begin <= origin_end <= padded_begin + ref_len */
    int64_t origin_end;
    const hc_gt_hap_aln* haps;
    int32_t n_haps;           /* 1 .. HC_GT_MAX_HAPS; the index is the haplotype's rank */
    const int64_t* read_begin; /* read intervals [begin, end), contig coordinates, >= 0 */
    const int64_t* read_end;
    int32_t n_reads;          /* >= 0 */
    const double* L;          /* n_reads x n_haps, read-major (compute_likelihoods' return value) */
} hc_gt_region;

/* One record per event begin inside a region's origin, skipped sites included.
 * For HC_GT_SITE_TOO_MANY_ALLELES the site is dropped before any map or
 * arithmetic exists: n_alleles is HC_GT_MAX_ALLELES + 1 (counting stops there),
 * alleles / hap_allele / keep / genotype_likelihoods are NULL with zero counts
 * and genotype_index, a1, a2 and genotype_quality are -1. begin and loc_end are
 * always valid. All pointers are owned by the hc_gt_calls handle. */
typedef struct hc_gt_call_site {
    int32_t region;
    int32_t status;
    int64_t begin;            /* alleles_loc.begin = the event begin (contig coordinate) */
    int64_t loc_end;          /* alleles_loc.end = the largest event end at the site */
    int32_t n_alleles;
    int32_t n_haps;           /* length of hap_allele (0 when NULL) */
    const char* const* alleles; /* n_alleles strings: the reference allele, then the alts sorted bytewise */
    const int32_t* hap_allele;
    const int32_t* keep;      /* ascending read indices overlapping [max(begin, 2) - 2, loc_end + 2): the
                               * window is cut at the contig's first base, where the reference throws */
    int32_t n_keep;
    int32_t n_genotypes;      /* n_alleles * (n_alleles + 1) / 2 */
    const double* genotype_likelihoods;
    int32_t genotype_index;
    int32_t a1, a2;           /* the genotype of genotype_index, a1 <= a2 */
    int32_t genotype_quality;
} hc_gt_call_site;

typedef struct hc_gt_calls hc_gt_calls;

/* One synchronous call on the engine's primary device. On success *out holds
 * the sites of every region; release it with hc_gt_calls_free. */
int hc_gt_call_regions(const hc_gt_region* regions, int32_t n_regions, hc_gt_calls** out);
/* Every in-origin site, in region order then ascending begin. */
int hc_gt_calls_sites(const hc_gt_calls* calls, const hc_gt_call_site** sites, int64_t* n);
int hc_gt_calls_free(hc_gt_calls* calls);

#ifdef __cplusplus
}
#endif
#endif /* HC_GT_H */
