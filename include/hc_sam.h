/*
 * hc_sam.h — C ABI of the MI355X SAM text parser (in libhcpairhmm.so).
 *
 * load_all_reads' per-line `iss >> record` (src/haplotypecaller/
 * haplotypecaller.hpp:24-42, sam/sam.hpp:100-114, sam/cigar.hpp:57-68) for a
 * whole SAM file at once: a block of text in, one record per alignment line and
 * a pool of BAM-packed CIGAR words (hc_prep.h) out. SEQ and QUAL are not
 * copied: a record holds their offsets from the line's first byte.
 *
 *   lines     end at '\n'; a last line without one is a line, a text ending in
 *             '\n' has no extra empty line. No NUL terminator is assumed.
 *   header    the leading run of lines whose first byte is '@'. From the first
 *             line that does not begin with '@' every line is an alignment line,
 *             a later one that starts with '@' included.
 *   fields    maximal runs of non-whitespace; whitespace is ' ', \t, \v, \f, \r.
 *             The first eleven are QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT
 *             TLEN SEQ QUAL; what follows is ignored. A line without any field
 *             is skipped (it has no record); a line with 1 to 10 is an error.
 *   integers  decimal digits only (TLEN: an optional leading '-'), value in the
 *             range of the field: FLAG, MAPQ uint16; POS, PNEXT uint32; TLEN int32.
 *             Leading zeros are allowed. Everything else is an error.
 *   CIGAR     "*" alone is n_cigar = 0; otherwise one or more elements of digits
 *             followed by one of MIDNSHP=X, each length at most 2^28 - 1.
 *   defect    does not fail the parse: the first of HC_SAM_DEFECT_* that applies.
 *
 * Status codes are the HC_PHMM_* codes of hc_pairhmm.h; message via
 * hc_phmm_last_error(). A syntax error is HC_PHMM_EINVAL; the message names the
 * 1-based line of the text and the field, and the lowest offending line wins
 * (within a line: too few fields, then the fields in their order). The parse
 * runs on the engine's primary device; the text goes up through a pinned
 * staging block of HC_SAM_STAGE_BYTES (default 4 MiB), piece after piece. No
 * CPU fallback. Calls are serialised under the parser's own lock; a failed call
 * leaves every engine usable. Records and pool are the same bytes on every run.
 */
#ifndef HC_SAM_H
#define HC_SAM_H

#include <stdint.h>

#include "hc_pairhmm.h"
#include "hc_prep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hc_sam_record.defect: the first that applies */
#define HC_SAM_DEFECT_NONE 0
#define HC_SAM_DEFECT_POS_ZERO 1     /* pos == 0 */
#define HC_SAM_DEFECT_NO_CIGAR 2     /* n_cigar == 0 */
#define HC_SAM_DEFECT_CIGAR_LENGTH 3 /* the CIGAR's read length (M I S = X) differs from seq_len */
#define HC_SAM_DEFECT_QUAL_LENGTH 4  /* qual_len != seq_len */
#define HC_SAM_DEFECT_TOO_LONG 5     /* seq_len > HC_PHMM_MAX_READ_LEN */

#define HC_SAM_MAX_CIGAR_LENGTH ((1u << 28) - 1u)

typedef struct hc_sam_record {
    int64_t line;              /* byte offset of the line in the text */
    uint32_t seq_off, qual_off; /* SEQ and QUAL, from `line` */
    int32_t seq_len, qual_len;
    uint32_t pos;              /* POS, 1-based */
    int32_t cigar;             /* first word in the pool */
    int32_t n_cigar;           /* 0 is "*" */
    uint16_t flag, mapq;
    uint8_t mate_same_contig;  /* RNEXT == "=" */
    uint8_t defect;            /* HC_SAM_DEFECT_* */
    uint8_t reserved[6];       /* 0; the record is 48 bytes without hidden padding */
} hc_sam_record;

typedef struct hc_sam_result hc_sam_result;

/* One synchronous call. `text` may be NULL when text_len == 0. On success *out
 * holds the records; release it with hc_sam_result_free. All pointers the
 * accessor returns are owned by the handle. */
int hc_sam_parse(const uint8_t* text, int64_t text_len, hc_sam_result** out);
/* The records in file order, each record's 1-based line number in the text, the
 * CIGAR pool (record k's words precede record k + 1's) and the number of header
 * lines. Any out pointer may be NULL. */
int hc_sam_result_records(const hc_sam_result* res, const hc_sam_record** records, const int32_t** line_no,
                          int32_t* n_records, const uint32_t** cigar_pool, int32_t* n_words, int32_t* n_header_lines);
int hc_sam_result_free(hc_sam_result* res);

#ifdef __cplusplus
}
#endif
#endif /* HC_SAM_H */
