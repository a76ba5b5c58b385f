/*
 * hc_intervals.h — C ABI of the interval calls of the MI355X genome caller (in
 * libhcpairhmm.so): hc_genome_call (hc_genome.h) and hc_bam_genome_call
 * (hc_bam.h) on the windows that a list of intervals asks for, and on nothing
 * else. An exome, a panel, one gene or one chromosome on a whole-genome table.
 *
 * Intervals. { contig, begin, end }: an index into the table and a 0-based,
 * half-open range of that contig's bases. Their order is free; overlapping,
 * abutting and duplicate intervals are merged on the host. HC_PHMM_EINVAL
 * before any device work, the message naming "interval K" (0-based, in the
 * caller's order): null intervals or n_intervals < 1 (no K), a contig index
 * outside the table, begin < 0, end <= begin, end > ref_len.
 *
 * Asked windows. Windows are the fixed tiling of hc_contig.h and keep their
 * genome-wide numbers and bounds, so the pick function is unchanged. Window w
 * of contig c is asked when its own bases [origin_begin, min(origin_end,
 * ref_len)) meet a merged interval of c. A window that is not asked has status
 * HC_CALL_NOT_ASKED, asm status HC_ASM_NO_HAPLOTYPES, k 0, 0 haplotypes, no
 * picks and no reads. An asked window without reads is HC_CALL_NO_READS.
 *
 * Scope. A record is in scope when it is placed (hc_genome.h) and POS - 1 lies
 * in the padded interval of an asked window of its contig; at most three
 * windows hold a position, since padding <= region, and window 0's padded
 * interval is [0, region + padding). Only records in scope are bucketed: a
 * record out of scope raises none of the three record errors of hc_genome.h
 * (unplaced, a defect behind the flag filters, more than
 * HC_CONTIG_MAX_READS_PER_POSITION reads at its position), because its position
 * has no bucket. HC_CONTIG_SKIP_UNPLACED is accepted and changes nothing. The
 * records out of scope stay in the result's records with their true contig_of.
 *
 * Sites and VCF. hc_genome_result_sites gives every site of the asked windows.
 * The VCF is the four header lines, then one line per HC_GT_SITE_EMITTED site
 * whose `begin` lies inside a merged interval of its contig: a site in an asked
 * window but outside every interval is in the sites and not in the text.
 *
 * The stand-in rule. Let P be the plain call (hc_genome_call or
 * hc_bam_genome_call) on the same input with HC_CONTIG_SKIP_UNPLACED. Where P
 * succeeds, the interval call has P's window count and bounds; for every asked
 * window P's picked reads, statuses, k, haplotype count and surviving reads;
 * its sites are P's sites of asked windows, in P's order, every field and
 * likelihood bit; its VCF follows the rule above. Dense and sorted buckets
 * (HC_GENOME_SORTED_BUCKETS, HC_GENOME_BUCKETS) give the same bytes. One
 * interval per contig that covers the whole contig gives P's result in every
 * field and byte.
 *
 * The device work. One thread per genome-wide window decides `asked` by a
 * binary search in its contig's merged intervals, a scan and a compaction give
 * the ascending list; one thread per record decides the scope; the bucket
 * kernels pass over the records out of scope (with sorted buckets the keys and
 * the sort are sized by the records in scope), and the pick kernels run one
 * wave per asked window. Beside the workspace of hc_genome.h: 16 bytes per
 * window, 16 per record, 16 per merged interval and 4 per contig.
 *
 * With an index. hc_bam_genome_call_intervals takes the bytes of the file's
 * .bai (SAM specification 5.2); NULL, 0 stands for no index: the call then
 * inflates and decodes the whole file as hc_bam_genome_call does and scopes the
 * records. With an index the file must be coordinate-sorted and the index its
 * own. The members from offset 0 are inflated until the BAM header is whole;
 * the header's references map to the table as in hc_bam.h. The query ranges are
 * the runs of consecutive asked windows of a contig, [first.padded_begin,
 * min(last.padded_end, ref_len)), through the header's refID for that contig
 * (a range that ends past 2^29, the index's reach, is HC_PHMM_EINVAL: call
 * such a contig without the index). Per range the chunks of the candidate bins
 * (reg2bins) are taken, but those that end at or in front of the linear
 * index's offset for the range's first 16 KiB window; all chunks are sorted by
 * their begin and merged where they overlap or share a member. BSIZE is
 * followed from each chunk's first member to the member its end lands in (the
 * whole file is not walked), only those members' bytes are uploaded, packed,
 * inflated and CRC-checked, and the records are framed chunk by chunk from the
 * chunk's in-member offset to its end.
 *   The records of the result are those framed, in file order; line_no is the
 * 1-based ordinal among them, and error messages say "record N (virtual offset
 * V)". Against the call without an index on the same file, every window field,
 * every site field and bit and the VCF bytes are identical; `picked` and
 * `reads` name records of the call's own list that are equal in pos, flag,
 * mapq, mate_same_contig, CIGAR words, SEQ and QUAL. Container and record
 * errors come only from members that are read.
 *   A stale or foreign index may give another result, or HC_PHMM_EINVAL when a
 * chunk's end is at no member, an in-member offset lies past its member's
 * bytes, or a chunk does not begin at a record. It never causes a read or
 * write out of bounds: every offset taken from the index is checked against
 * file_len and against the member it lands in before anything goes to the
 * device. BAI errors are HC_PHMM_EINVAL with messages beginning "BAI: ": a
 * missing BAI\1 magic, a file cut short, n_ref other than the BAM header's, a
 * negative count, a chunk with beg > end, a compressed offset at or past
 * file_len. Bin 37450 (the metadata pseudo-bin) is passed over; the trailing
 * n_no_coor is optional.
 *
 * Flags, pick modes and HC_GENOME_BUCKETS are hc_genome.h's. Calls are
 * serialised as the plain calls are. No CPU fallback. The same input gives the
 * same bytes on every run. HC_GENOME_TRACE=1 gains the phase scope= behind
 * resolve= and intervals=N (merged) asked=N (windows) scoped=N (records); an
 * indexed call also the phases header= and index= (the choice of the chunks
 * and the member walk) and chunks=N members=N bytes_up=B.
 */
#ifndef HC_INTERVALS_H
#define HC_INTERVALS_H

#include <stdint.h>

#include "hc_bam.h"
#include "hc_genome.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hc_interval {
    int32_t contig;      /* index into the table */
    int64_t begin, end;  /* 0-based, half-open */
} hc_interval;

#define HC_CALL_NOT_ASKED 3 /* a genome-wide window's status, beside hc_call.h's */

/* hc_genome_call on the asked windows. Every accessor of hc_genome.h works on the result. */
int hc_genome_call_intervals(const uint8_t* sam, int64_t sam_len, const hc_genome_contig* contigs, int32_t n_contigs,
                             const hc_interval* intervals, int32_t n_intervals, int32_t region_size, int32_t padding_size,
                             uint64_t seed, int32_t pick_mode, uint32_t flags, hc_genome_result** out);
/* hc_bam_genome_call on the asked windows; `bai`, `bai_len` are the index's bytes, or NULL, 0 (see "With an index").
 * hc_bam_genome_result_bases works on the result. */
int hc_bam_genome_call_intervals(const uint8_t* file, int64_t file_len, const uint8_t* bai, int64_t bai_len,
                                 const hc_genome_contig* contigs, int32_t n_contigs, const hc_interval* intervals,
                                 int32_t n_intervals, int32_t region_size, int32_t padding_size, uint64_t seed,
                                 int32_t pick_mode, uint32_t flags, hc_genome_result** out);
/* The merged intervals (sorted by contig, then begin) and the asked windows, ascending. Of a plain call's result: none. */
int hc_genome_result_intervals(const hc_genome_result* res, const hc_interval** merged, int32_t* n_merged,
                               const int32_t** asked, int32_t* n_asked);

/* Of an indexed call: the chunks after merging, the members uploaded and inflated (the header's included), the
 * compressed bytes uploaded and the records framed; all 0 for other results. */
int hc_bam_genome_result_index(const hc_genome_result* res, int32_t* n_chunks, int32_t* n_members, int64_t* bytes_up,
                               int64_t* n_records);

#ifdef __cplusplus
}
#endif
#endif /* HC_INTERVALS_H */
