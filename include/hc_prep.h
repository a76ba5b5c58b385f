/*
 * hc_prep.h — C ABI of the MI355X read preparation (in libhcpairhmm.so).
 *
 * filter_reads and hard_clip_reads of HaplotypeCaller::call_region
 * (src/haplotypecaller/haplotypecaller.hpp:93-94) for many windows at once:
 * the four flag filters (utils/read_filter.hpp), ReadClipper::
 * revert_soft_clipped_bases and hard_clip_to_interval (utils/read_clipper.hpp:
 * 32-91) and the minimum-length filter. Bases and qualities are not inputs:
 * every clip of the reference is a substr, so a prepared read is a view
 * (offset, length) into the caller's own SEQ / QUAL.
 *
 * Per read, as the reference does it:
 *   filters   removed when MAPQ < 20, FLAG & 0x400, FLAG & 0x100 or the mate is
 *             on another contig (RNEXT != "="); drop_reason is the first that hits.
 *   revert    reverse strand (FLAG & 0x10): a front S removes its bases from the
 *             front of the sequence and leaves the CIGAR alone; a back S becomes M.
 *             Forward strand: a front S with alignment_begin >= its length becomes
 *             M and POS moves left by that length, otherwise nothing changes; a
 *             back S removes its bases from the end and leaves the CIGAR alone.
 *             back() is read after front() was rewritten, and a one-element CIGAR
 *             is both.
 *   hard clip alignment_begin = POS - 1 after the revert, alignment_end = that
 *             plus the reference length (M D N = X) of the rewritten CIGAR. Before
 *             the window: min(begin - alignment_begin, size) bases leave the front.
 *             Past its end: clip = alignment_end - end bases leave the back, except
 *             that clip > size keeps the read whole (the reference's size_t wrap in
 *             substr). POS and the CIGAR are not touched by the hard clip.
 *   length    fewer than 10 bases left removes the read (HC_PREP_DROP_MIN_LENGTH).
 *
 * Status codes are the HC_PHMM_* codes of hc_pairhmm.h; message via
 * hc_phmm_last_error(). HC_PHMM_EINVAL before any device work: null pointers,
 * negative counts, padded_begin < 0, padded_end < padded_begin, seq_len outside
 * 0 .. HC_PHMM_MAX_READ_LEN. HC_PHMM_EINVAL from
 * the device, naming the lowest (window, read), for a read that passes the four
 * flag filters with pos == 0, n_cigar == 0, an op code above 8 or a CIGAR whose
 * read length (M I S = X) differs from seq_len; the reads the flag filters
 * remove are never looked at, as in the reference. No CPU fallback. Calls are
 * serialised under the preparation's own lock and run on the engine's primary
 * device; a failed call leaves every engine usable.
 */
#ifndef HC_PREP_H
#define HC_PREP_H

#include <stdint.h>

#include "hc_pairhmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hc_prep_record.drop_reason, in the reference's order */
#define HC_PREP_KEPT 0
#define HC_PREP_DROP_MAPQ 1
#define HC_PREP_DROP_DUPLICATE 2
#define HC_PREP_DROP_SECONDARY 3
#define HC_PREP_DROP_MATE_CONTIG 4
#define HC_PREP_DROP_MIN_LENGTH 5

#define HC_PREP_MIN_MAPQ 20
#define HC_PREP_MIN_LENGTH 10

/* CIGAR words are BAM's: length << 4 | op, op indexing "MIDNSHP=X". */
#define HC_PREP_CIGAR_WORD(length, op) (((uint32_t)(length) << 4) | (uint32_t)(op))

typedef struct hc_prep_read {
    const uint32_t* cigar;    /* n_cigar words; may be NULL when n_cigar == 0 */
    int32_t n_cigar;          /* >= 0; 0 is SAM's "*" */
    uint32_t pos;             /* POS, 1-based */
    int32_t seq_len;          /* 0 .. HC_PHMM_MAX_READ_LEN */
    uint16_t flag;            /* FLAG */
    uint16_t mapq;            /* MAPQ */
    uint8_t mate_same_contig; /* RNEXT == "=" */
    uint8_t reserved[3];
} hc_prep_read;

typedef struct hc_prep_window {
    int64_t padded_begin, padded_end; /* contig coordinates, 0 <= begin <= end */
    const hc_prep_read* reads;
    int32_t n_reads;                  /* >= 0 */
} hc_prep_window;

/* One per read. A read the flag filters remove keeps offset 0, length seq_len,
 * new_pos = pos and begin = end = 0: its CIGAR is never read. */
typedef struct hc_prep_record {
    int64_t begin, end;  /* get_interval() after the revert: [new_pos - 1, + reference length) */
    uint32_t new_pos;    /* POS after the revert */
    int32_t offset;      /* the surviving view into SEQ / QUAL */
    int32_t length;
    uint8_t keep;
    uint8_t drop_reason; /* HC_PREP_KEPT or the first filter that removes the read */
    uint8_t front_to_M;  /* the revert rewrote CIGAR.front() from S to M */
    uint8_t back_to_M;   /* the revert rewrote CIGAR.back() from S to M */
} hc_prep_record;

typedef struct hc_prep_result hc_prep_result;

/* One synchronous call. On success *out holds every window's records; release it
 * with hc_prep_result_free. All pointers the accessors return are owned by the handle. */
int hc_prep_reads(const hc_prep_window* windows, int32_t n_windows, hc_prep_result** out);
/* The records of `window` in input order, the indices of the kept reads in input
 * order, their count and the sum of their lengths (what the assembler's
 * HC_ASM_MAX_REGION_READ_BASES bounds). Any out pointer may be NULL. */
int hc_prep_result_window(const hc_prep_result* res, int32_t window, const hc_prep_record** records, int32_t* n_reads,
                          const int32_t** kept, int32_t* n_kept, int64_t* kept_bases);
int hc_prep_result_free(hc_prep_result* res);

#ifdef __cplusplus
}
#endif
#endif /* HC_PREP_H */
