/*
 * hc_bam.h — C ABI of the MI355X BAM front (in libhcpairhmm.so): BGZF inflate
 * and BAM record decode on the device, and the genome caller on a BAM file.
 *
 *   hc_bgzf_inflate      any BGZF file (BAM or not) to its inflated bytes.
 *   hc_bam_parse         a BAM file to hc_sam_record records (hc_sam.h), a CIGAR
 *                        pool, the header's reference table and a bases buffer.
 *   hc_bam_genome_call   hc_genome_call (hc_genome.h) with a BAM file in the
 *                        place of the SAM text.
 *
 * The container. A BGZF file is a run of gzip members of at most 64 KiB each,
 * one DEFLATE stream apiece, with the member's size (BSIZE) in a `BC` extra
 * subfield and the CRC32 and the byte count (ISIZE) of its inflated bytes in
 * the trailer. The host walks the members once (header and trailer only); the
 * file goes up through the SAM parser's pinned staging block; one wave inflates
 * one member (stored, fixed and dynamic blocks, any number per member) and
 * checks its CRC32. The empty last member that marks the end of the file is
 * not required. A raw BAM stream that is not BGZF is refused.
 *
 * The records. The alignment records are framed on the host from the inflated
 * stream (the block_size chain) and decoded by one wave per record. A record's
 * SEQ, expanded to ASCII (=ACMGRSVTWYHKDBN), followed by its QUAL with 33 added,
 * goes to the bases buffer, 2 * l_seq bytes per record in file order. The
 * records are views into that buffer as SAM records are views into the text:
 * `line` is the record's offset in the bases buffer, seq_off is 0, qual_off is
 * seq_len. line_no is the 1-based ordinal of the alignment record. The CIGAR
 * pool follows the rule of hc_sam.h: record k's words precede record k + 1's;
 * the words are copied, not re-encoded.
 *
 * The stand-in rule. hc_bam_genome_call(file, table, ...) gives the result of
 * hc_genome_call(T, table, ...), T being the SAM text `samtools view -h` prints
 * for the file: every field, site and VCF byte. The exceptions are `line`,
 * seq_off, qual_off, line_no (an ordinal in the place of a text line) and the
 * wording of error messages ("record N" for "line N"). T is the header text,
 * then one line per record with RNAME from the header's reference table ("*"
 * for refID -1), POS = pos + 1, RNEXT "=" when next_refID == refID and
 * refID >= 0, else the name or "*". In record terms:
 *   pos               BAM's pos + 1; BAM's -1 gives 0, HC_SAM_DEFECT_POS_ZERO
 *   mate_same_contig  next_refID == refID && refID >= 0
 *   flag, mapq        as they are
 *
 * Contig resolution. Each name of the BAM header's reference table is looked up
 * in the caller's contig table byte for byte (the hash table of hc_genome.h);
 * contig_of per record comes from refID through that map, on the device. A
 * reference that is not in the table makes its reads unplaced, and so does
 * refID -1; unplaced reads are handled as in hc_genome.h (HC_PHMM_EINVAL, or
 * left out under HC_CONTIG_SKIP_UNPLACED). The header's l_ref values are not
 * compared with ref_len: placement uses the table's length.
 *
 * What has no SAM twin.
 *   l_seq == 0        seq_len 0 (T prints "*", which the SAM parser counts as one byte).
 *   QUAL 0xFF...      a QUAL whose first byte is 0xFF has qual_len 0; with
 *                     l_seq > 0 that is HC_SAM_DEFECT_QUAL_LENGTH.
 *   a quality > 93    cannot be written as text: HC_SAM_DEFECT_QUAL_RANGE, the
 *                     last defect in the order of hc_sam.h, from this path only.
 *   CG:B,I            the long-CIGAR convention is not followed: reads are at
 *                     most HC_PHMM_MAX_READ_LEN long, and a placeholder kSmN
 *                     CIGAR is taken as written.
 *   Auxiliary tags and QNAME are not read.
 *
 * Errors. All HC_PHMM_EINVAL, message via hc_phmm_last_error(); the lowest
 * member wins, then the lowest record.
 *   container ("member M at offset O", M 0-based, O its compressed offset): not
 *   a BGZF member (magic, the FEXTRA flag, the BC subfield); BSIZE past the end
 *   of the file; ISIZE above 65536; a DEFLATE stream that is malformed, ends
 *   early or produces another byte count than ISIZE; a back-reference before
 *   the member's first byte; a CRC32 mismatch.
 *   BAM ("record N", 1-based; the header is "BAM header"): missing BAM\1 magic;
 *   a header or a record cut short by the end of the stream; block_size smaller
 *   than the record's own fields need; a CIGAR op above 8; refID or next_refID
 *   outside [-1, n_ref); l_read_name 0.
 *
 * Status codes are the HC_PHMM_* codes. No CPU fallback. Calls are serialised
 * under the SAM parser's lock (BAM and SAM share the parser's stream and
 * workspaces); a failed call leaves every engine usable; the same input gives
 * the same bytes on every run. HC_GENOME_TRACE=1 prints front=bam and the
 * phases upload=, inflate=, crc=, frame=, decode= and readback= in the
 * [hc_genome] line of a BAM call; HC_BAM_TRACE=1 prints them for
 * hc_bgzf_inflate and hc_bam_parse as "[hc_bam] ...".
 */
#ifndef HC_BAM_H
#define HC_BAM_H

#include <stdint.h>

#include "hc_genome.h"
#include "hc_sam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hc_sam_record.defect, beside those of hc_sam.h: a quality above 93 (BAM only) */
#define HC_SAM_DEFECT_QUAL_RANGE 6

#define HC_BGZF_MAX_ISIZE 65536

typedef struct hc_bgzf_result hc_bgzf_result;
typedef struct hc_bam_result hc_bam_result;

/* One synchronous call. `file` may be NULL when file_len == 0 (no member, no
 * byte). Release the result with hc_bgzf_result_free. All pointers the accessors
 * return are owned by the handle; any out pointer may be NULL. */
int hc_bgzf_inflate(const uint8_t* file, int64_t file_len, hc_bgzf_result** out);
/* The inflated bytes, on the host. */
int hc_bgzf_result_bytes(const hc_bgzf_result* res, const uint8_t** bytes, int64_t* length);
/* Per member, in file order: its offset in the file, the offset of its bytes in the inflated bytes, its ISIZE. */
int hc_bgzf_result_members(const hc_bgzf_result* res, const int64_t** compressed_offset, const int64_t** inflated_offset,
                           const int32_t** isize, int32_t* n_members);
int hc_bgzf_result_free(hc_bgzf_result* res);

/* One synchronous call; `file` may be released when it returns. Release the result with hc_bam_result_free. */
int hc_bam_parse(const uint8_t* file, int64_t file_len, hc_bam_result** out);
/* As hc_sam_result_records, with ref_id[k] = record k's refID in the place of the header's line count. */
int hc_bam_result_records(const hc_bam_result* res, const hc_sam_record** records, const int32_t** line_no,
                          int32_t* n_records, const uint32_t** cigar_pool, int32_t* n_words, const int32_t** ref_id);
/* The header text (l_text bytes, as stored) and the number of references. */
int hc_bam_result_header(const hc_bam_result* res, const char** text, int64_t* text_len, int32_t* n_ref);
/* Reference `ref` of the header's table: its name (NUL-terminated; name_len without the NUL) and l_ref. */
int hc_bam_result_reference(const hc_bam_result* res, int32_t ref, const char** name, int32_t* name_len, int64_t* length);
/* The bases buffer the records' `line` offsets point into. */
int hc_bam_result_bases(const hc_bam_result* res, const uint8_t** bases, int64_t* length);
int hc_bam_result_free(hc_bam_result* res);

/* hc_genome_call on a BAM file. Every accessor of hc_genome.h works on the
 * result, hc_genome_result_sam gives the records described above, and
 * hc_genome_result_free releases it. The result owns the bases buffer: `file`
 * may be released when the call returns. flags and HC_GENOME_BUCKETS as in
 * hc_genome.h. */
int hc_bam_genome_call(const uint8_t* file, int64_t file_len, const hc_genome_contig* contigs, int32_t n_contigs,
                       int32_t region_size, int32_t padding_size, uint64_t seed, int32_t pick_mode, uint32_t flags,
                       hc_genome_result** out);
/* The bases buffer of a result of hc_bam_genome_call (NULL and 0 for one of hc_genome_call). */
int hc_bam_genome_result_bases(const hc_genome_result* res, const uint8_t** bases, int64_t* length);

#ifdef __cplusplus
}
#endif
#endif /* HC_BAM_H */
