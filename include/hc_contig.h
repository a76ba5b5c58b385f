/*
 * hc_contig.h — C ABI of the MI355X contig caller (in libhcpairhmm.so).
 *
 * HaplotypeCaller::do_work (src/haplotypecaller/haplotypecaller.hpp:24-50,
 * 112-154) as one call: the text of a SAM file and one contig's reference in,
 * the VCF text out.
 *
 *   :24-42    load_all_reads          hc_sam_parse (hc_sam.h), then on the device the reads
 *                                     per begin position (alignment_begin = POS - 1, whatever
 *                                     the RNAME), each position's reads in file order
 *   :125-151  the window loop         n_windows = ceil(ref_len / region_size); window i has the
 *                                     origin [i * region, (i + 1) * region) and the padded
 *                                     interval [origin.begin - padding, origin.end + padding),
 *                                     [0, region + padding) for i = 0; its reference is
 *                                     ref[padded.begin, padded.end) cut at the contig's end
 *   :141-143  select_one_read         per window and per position of its padded interval that
 *                                     holds reads, one of them (below); positions >= ref_len
 *                                     hold none. On the device, one wave per window.
 *   :145      "Ignore"                a window without reads is not sent: HC_CALL_NO_READS
 *   :146      call_region             hc_call_windows (hc_call.h), in batches of at most
 *                                     HC_CONTIG_BATCH_WINDOWS windows (environment, default 512)
 *   :132-135, Variant::print          the four header lines and one line per HC_GT_SITE_EMITTED
 *                                     site, in window order and site order
 *
 * The pick. The reference seeds mt19937 from random_device for every pick, so
 * it has no reproducible picks; the library defines its own. Of `count` reads
 * at position `begin`, window `window` takes index 0 with HC_CONTIG_PICK_FIRST,
 * and with HC_CONTIG_PICK_SEEDED (all arithmetic mod 2^64)
 *     z = seed + 0x9E3779B97F4A7C15 * (window * 2^32 + begin + 1)
 *     z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9
 *     z = (z ^ z >> 27) * 0x94D049BB133111EB
 *     z ^= z >> 31
 *     index = ((z >> 32) * count) >> 32.
 * Overlapping windows pick independently, as the reference does.
 *
 * Placement. A read with POS == 0 or alignment_begin >= ref_len is unplaced
 * (the reference writes outside reads_map there): HC_PHMM_EINVAL naming its
 * line, or with HC_CONTIG_SKIP_UNPLACED the read is left out. A placed read
 * that passes the four flag filters of hc_prep.h and has a non-zero defect
 * (hc_sam.h) is HC_PHMM_EINVAL as well, whether or not it is picked. The lowest
 * line wins.
 *
 * The chain is given the origin cut at the contig's end (no event lies past
 * it), the padded interval as the reference has it.
 *
 * Status codes are the HC_PHMM_* codes of hc_pairhmm.h; message via
 * hc_phmm_last_error(). HC_PHMM_EINVAL before any device work: null pointers,
 * unknown flags or pick mode, ref_len < 1, region_size < 1, padding_size < 0 or
 * > region_size (the reference's size_t wrap), region_size + 2 * padding_size >
 * HC_GT_MAX_REF_LEN; from the device, more than HC_CONTIG_MAX_READS_PER_POSITION
 * reads beginning at one position. The device workspace is 24 bytes per contig
 * base, 4 per record and 4 per picked read (a 250 Mbase contig: 6 GB); there is
 * no other bound on ref_len. `ref` is used as it is: upper-case it first, as do_work
 * does. No CPU fallback. Calls are serialised under the contig caller's own lock.
 */
#ifndef HC_CONTIG_H
#define HC_CONTIG_H

#include <stdint.h>

#include "hc_call.h"
#include "hc_sam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags; the first three are hc_call_windows' */
#define HC_CONTIG_F64 1u               /* = HC_CALL_F64 */
#define HC_CONTIG_DEFAULT_MODE 2u      /* = HC_CALL_DEFAULT_MODE */
#define HC_CONTIG_WANT_SITE_READS 32u  /* = HC_CALL_WANT_SITE_READS */
#define HC_CONTIG_SKIP_UNPLACED 256u

#define HC_CONTIG_PICK_SEEDED 0
#define HC_CONTIG_PICK_FIRST 1

/* More reads than this beginning at one position are HC_PHMM_EINVAL: a
 * position's reads are put in file order by one lane (deep amplicon pile-ups
 * are outside what the window caller downstream is built for as well). */
#define HC_CONTIG_MAX_READS_PER_POSITION 4096

#define HC_CONTIG_DEFAULT_REGION 245
#define HC_CONTIG_DEFAULT_PADDING 85

typedef struct hc_contig_result hc_contig_result;

/* One synchronous call. `contig` is the CHROM text (NUL-terminated). `sam` must
 * stay as it is until the result is freed: the result's records are views into
 * it. Release the result with hc_contig_result_free. All pointers the accessors
 * return are owned by the handle; any out pointer of an accessor may be NULL. */
int hc_contig_call(const uint8_t* sam, int64_t sam_len, const char* contig, const uint8_t* ref, int64_t ref_len,
                   int32_t region_size, int32_t padding_size, uint64_t seed, int32_t pick_mode, uint32_t flags,
                   hc_contig_result** out);
/* The VCF text (not NUL-counted in `length`) and the number of windows. */
int hc_contig_result_vcf(const hc_contig_result* res, const char** text, int64_t* length, int32_t* n_windows);
/* The parsed records, as hc_sam_result_records. */
int hc_contig_result_sam(const hc_contig_result* res, const hc_sam_record** records, const int32_t** line_no,
                         int32_t* n_records, const uint32_t** cigar_pool, int32_t* n_words);
/* The window's bounds as the reference has them, the length of its reference
 * slice, the picked reads as record indices in ascending position, and status,
 * assembler status, k and haplotype count as hc_call_result_window gives them
 * (HC_CALL_NO_READS, HC_ASM_NO_HAPLOTYPES, 0, 0 for a window without reads). */
int hc_contig_result_window(const hc_contig_result* res, int32_t window, int64_t* padded_begin, int64_t* padded_end,
                            int64_t* origin_begin, int64_t* origin_end, int32_t* ref_len, const int32_t** picked,
                            int32_t* n_picked, int32_t* status, int32_t* asm_status, int32_t* kmer_size,
                            int32_t* n_haps);
/* Every in-origin site of the HC_CALL_CALLED windows, in window order then
 * ascending begin; `region` is the contig-wide window index. keep indexes the
 * window's surviving reads (hc_contig_result_reads), in their order. */
int hc_contig_result_sites(const hc_contig_result* res, const hc_gt_call_site** sites, int64_t* n);
/* The picked reads of `window` that survive the preparation and, in a
 * HC_CALL_CALLED window, the PairHMM's filter: record indices. */
int hc_contig_result_reads(const hc_contig_result* res, int32_t window, const int32_t** reads, int32_t* n);
int hc_contig_result_free(hc_contig_result* res);

#ifdef __cplusplus
}
#endif
#endif /* HC_CONTIG_H */
