/*
 * hc_call.h — C ABI of the MI355X window caller (in libhcpairhmm.so).
 *
 * HaplotypeCaller::call_region (src/haplotypecaller/haplotypecaller.hpp:83-107)
 * as one call, for any number of windows: aligned reads and the padded window
 * in, called variants out.
 *
 *   :93-94   filter_reads, hard_clip_reads      hc_prep_reads (hc_prep.h)
 *   :96      no read left                       the window ends HC_CALL_NO_READS
 *   :100     assembler.assemble                 hc_asm_assemble (hc_asm.h), one pass over the other windows;
 *                                               the reads are views into the caller's bases and qualities
 *   :101     at most one haplotype              the window ends HC_CALL_NO_VARIATION
 *   :103-104 compute_likelihoods and            hc_region_call (hc_region.h), one pass over the remaining
 *            assign_genotype_likelihoods        windows; the haplotypes are aligned there, once
 *
 * Each stage computes what its own header says, bit for bit; this call adds the
 * read views and the two early endings. The insertion, deletion and
 * continuation qualities are the reference's constants 'I', 'I', '+'
 * (sam/sam.hpp:30-32). No byte of bases or qualities is copied on the host
 * between the stages.
 *
 * Status codes are the HC_PHMM_* codes of hc_pairhmm.h; message via
 * hc_phmm_last_error(). Invalid input is HC_PHMM_EINVAL: null pointers,
 * negative counts, unknown flags, ref_len outside 1 .. HC_GT_MAX_REF_LEN, a
 * window whose kept reads sum to more than HC_ASM_MAX_REGION_READ_BASES, and
 * whatever the three stage calls refuse, with their messages. No CPU fallback.
 * Calls are serialised under the window caller's own lock.
 */
#ifndef HC_CALL_H
#define HC_CALL_H

#include <stdint.h>

#include "hc_asm.h"
#include "hc_gt.h"
#include "hc_pairhmm.h"
#include "hc_prep.h"
#include "hc_region.h"

#ifdef __cplusplus
extern "C" {
#endif

/* window status */
#define HC_CALL_CALLED 0        /* reached the genotyper; its sites are in hc_call_result_sites */
#define HC_CALL_NO_READS 1      /* no read survives the preparation (:96) */
#define HC_CALL_NO_VARIATION 2  /* the assembly gives at most one haplotype (:101) */

typedef struct hc_call_window {
    const uint8_t* ref;           /* the padded window's bases */
    int32_t ref_len;              /* 1 .. HC_GT_MAX_REF_LEN */
    int64_t padded_begin, padded_end, origin_begin, origin_end;
    const hc_prep_read* reads;    /* as hc_prep_reads takes them */
    const uint8_t* const* bases;  /* per read: seq_len bytes of SEQ */
    const uint8_t* const* quals;  /* per read: seq_len bytes of QUAL (ASCII, phred + 33) */
    int32_t n_reads;              /* >= 0 */
} hc_call_window;

/* flags of hc_call_windows; they map onto hc_region_call's */
#define HC_CALL_F64 1u              /* = HC_REGION_F64 */
#define HC_CALL_DEFAULT_MODE 2u     /* = HC_REGION_DEFAULT_MODE */
#define HC_CALL_WANT_L 16u          /* = HC_REGION_WANT_L */
#define HC_CALL_WANT_SITE_READS 32u /* = HC_REGION_WANT_SITE_READS */
#define HC_CALL_WANT_CIGARS 64u     /* = HC_REGION_WANT_CIGARS */

typedef struct hc_call_result hc_call_result;

/* One synchronous call. On success *out holds the results of every window;
 * release it with hc_call_result_free. All pointers the accessors return are
 * owned by the handle. Any out pointer of an accessor may be NULL. */
int hc_call_windows(const hc_call_window* windows, int32_t n_windows, uint32_t flags, hc_call_result** out);
/* status; the assembler's own status (HC_ASM_*), accepted k and haplotype count
 * (HC_ASM_NO_HAPLOTYPES, 0, 0 for a window that ended HC_CALL_NO_READS). */
int hc_call_result_window(const hc_call_result* res, int32_t window, int32_t* status, int32_t* asm_status,
                          int32_t* kmer_size, int32_t* n_haps);
/* The preparation's records, as hc_prep_result_window. */
int hc_call_result_prep(const hc_call_result* res, int32_t window, const hc_prep_record** records, int32_t* n_reads,
                        const int32_t** kept, int32_t* n_kept, int64_t* kept_bases);
/* Haplotype `hap` of `window` in the assembler's final order; bases are not
 * NUL-terminated. begin / cigar: its alignment against the window, with
 * HC_CALL_WANT_CIGARS (HC_PHMM_EINVAL when asked for without the flag); -1 and
 * NULL for a window that did not reach the region caller. */
int hc_call_result_hap(const hc_call_result* res, int32_t window, int32_t hap, const uint8_t** bases, int32_t* length,
                       double* score, int32_t* begin, const char** cigar);
/* Every in-origin site of the HC_CALL_CALLED windows, in window order then
 * ascending begin; `region` is the caller's window index. keep indexes the
 * window's surviving reads (hc_call_result_reads), in their order. */
int hc_call_result_sites(const hc_call_result* res, const hc_gt_call_site** sites, int64_t* n);
/* The reads that survive the preparation and, in a HC_CALL_CALLED window, the
 * PairHMM's filter as well: indices into the caller's reads, ascending. */
int hc_call_result_reads(const hc_call_result* res, int32_t window, const int32_t** reads, int32_t* n);
/* HC_CALL_WANT_L: surviving reads x haplotypes, read-major, capped. HC_PHMM_EINVAL
 * without the flag; 0 x n_haps for a window that did not reach the region caller. */
int hc_call_result_matrix(const hc_call_result* res, int32_t window, const double** L, int32_t* n_reads,
                          int32_t* n_haps);
int hc_call_result_free(hc_call_result* res);

#ifdef __cplusplus
}
#endif
#endif /* HC_CALL_H */
