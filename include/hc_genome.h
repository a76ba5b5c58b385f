/*
 * hc_genome.h — C ABI of the MI355X genome caller (in libhcpairhmm.so).
 *
 * The layer above HaplotypeCaller::do_work that the reference does not have:
 * the text of a SAM file and a table of contigs in, one VCF text out. The text
 * is parsed once (hc_sam.h), every record's RNAME is resolved against the table
 * on the device, the reads per begin position and the picks run over all
 * contigs in one pass, and hc_call_windows (hc_call.h) is given batches of
 * HC_CONTIG_BATCH_WINDOWS windows with reads (environment, default 512) that
 * are filled across contig borders: a batch is the next so many sent windows,
 * whatever contigs they belong to.
 *
 * Semantics. Contig c's windows, picks, statuses, sites and surviving reads
 * are those of
 *     hc_contig_call(the header lines + the alignment lines whose RNAME equals
 *                    contigs[c].name, in file order, contigs[c].name,
 *                    contigs[c].ref, contigs[c].ref_len, and the same
 *                    region_size, padding_size, seed, pick_mode and flags)
 * (hc_contig.h), with record indices translated to the whole text's. The pick
 * function of hc_contig.h takes the contig's own window index and the position
 * inside the contig; every contig uses the same `seed`. Windows are numbered
 * genome-wide: contig c's windows follow contig c - 1's, in table order. A
 * window's bounds are positions inside its contig. The VCF is the four header
 * lines once, then each contig's site lines in table order, CHROM = the
 * table's name. Header lines of the text (@SQ and the rest) are not read.
 *
 * Names are compared byte for byte with the RNAME token (the third
 * white-space separated token of the line, as the parser splits it).
 *
 * Placement. A read is unplaced when its RNAME is not in the table ("*"
 * included), when POS == 0, or when POS - 1 >= its own contig's ref_len (it
 * never spills into the next contig's positions): HC_PHMM_EINVAL naming the
 * 1-based line of the whole text, for an unknown name with the RNAME cut at 64
 * bytes; with HC_CONTIG_SKIP_UNPLACED the read is left out. A placed read that
 * passes the four flag filters and has a non-zero defect is HC_PHMM_EINVAL, as
 * in hc_contig.h. The lowest line wins, across both kinds and across contigs.
 * More than HC_CONTIG_MAX_READS_PER_POSITION reads beginning at one position
 * are HC_PHMM_EINVAL naming the contig and its 1-based position.
 *
 * HC_PHMM_EINVAL before any device work: the argument errors of hc_contig_call
 * for every contig, n_contigs < 1 or > HC_GENOME_MAX_CONTIGS, a name that is
 * null, empty, longer than HC_GENOME_MAX_NAME_LEN, equal to "*" or holds white
 * space, two equal names (the message names both indices), more than 2^31 - 1
 * windows in total.
 *
 * The device workspace. Besides the SAM text (which has to fit the device), the
 * table itself, 4 bytes per record, 4 per picked read and 12 per window (a
 * human genome at region 245 has 12.6 M windows), the buckets take
 *   dense (the default): that of hc_contig.h with the sum of all ref_len in the
 *     place of ref_len, 16 bytes per base of the table (two counters and an
 *     offset): about 50 GB for a human genome of 3.1 Gbases, with the memsets
 *     and a scan over every base;
 *   sorted (HC_GENOME_SORTED_BUCKETS): nothing per base. A stable radix sort of
 *     (off[contig] + POS - 1, record index), 8 bits per pass,
 *     ceil(bits(sum of ref_len) / 8) passes, and a table of the runs of equal
 *     keys: at most 42 bytes per record, a few hundred MB for an exome, a panel
 *     or a low-coverage sample on the full GRCh38 table. The sum of all ref_len
 *     is bounded by 2^63 only; the record count stays the parser's int32.
 * Both give the same result in every field and byte, errors and their messages
 * included; within a position the reads are in file order either way. Dense
 * stays the default: the choice is the caller's, through the flag, or through
 * the environment for a caller that cannot pass one: HC_GENOME_BUCKETS=sorted
 * acts as the flag, =dense or unset changes nothing (the flag wins over dense),
 * any other value is HC_PHMM_EINVAL naming the variable. It is read per call.
 * hc_contig_call (hc_contig.h) keeps its dense buckets and refuses the flag.
 * Where the dense workspace does not fit and the sorted one is not wanted: call
 * chromosome by chromosome, or with the contigs that have reads.
 *
 * `ref` is used as it is: upper-case it first; a contig no window of which has
 * reads is never read. FASTA reading stays on the host. No CPU fallback. Calls
 * are serialised under the genome caller's own lock; a failed call leaves every
 * engine usable. HC_GENOME_TRACE=1 prints one line "[hc_genome] key=value ..."
 * per call on stderr: the host wall clock of the phases, the counts, and
 * sorted=0|1, sort_passes=N, tile_bytes=B (the device bytes this call asked of
 * the record, position or sort, and window workspaces together; the grow-only
 * buffers may hold more).
 */
#ifndef HC_GENOME_H
#define HC_GENOME_H

#include <stdint.h>

#include "hc_contig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HC_GENOME_MAX_NAME_LEN 255
#define HC_GENOME_MAX_CONTIGS 4194304 /* the name pool and the table are indexed with 32 bits */

/* A flag of hc_genome_call beside the HC_CONTIG_* ones: buckets by a sort sized
 * by the records ("The device workspace" above). Not a flag of hc_contig_call. */
#define HC_GENOME_SORTED_BUCKETS 512u

typedef struct hc_genome_contig {
    const char* name;    /* the CHROM text and the RNAME it answers to (NUL-terminated) */
    const uint8_t* ref;
    int64_t ref_len;
} hc_genome_contig;

typedef struct hc_genome_result hc_genome_result;

/* One synchronous call. flags are HC_CONTIG_* and HC_GENOME_SORTED_BUCKETS, pick_mode HC_CONTIG_PICK_*.
 * `sam` must stay as it is until the result is freed: the result's records
 * are views into it. The table and what it points to are read during the call
 * only. Release the result with hc_genome_result_free. All pointers the
 * accessors return are owned by the handle; any out pointer may be NULL. */
int hc_genome_call(const uint8_t* sam, int64_t sam_len, const hc_genome_contig* contigs, int32_t n_contigs,
                   int32_t region_size, int32_t padding_size, uint64_t seed, int32_t pick_mode, uint32_t flags,
                   hc_genome_result** out);
/* The VCF text (not NUL-counted in `length`), the number of windows of all contigs and of contigs. */
int hc_genome_result_vcf(const hc_genome_result* res, const char** text, int64_t* length, int32_t* n_windows,
                         int32_t* n_contigs);
/* Contig `contig` of the table: its first genome-wide window, its window count
 * and the number of records whose RNAME resolved to it (placed or not). */
int hc_genome_result_contig(const hc_genome_result* res, int32_t contig, int32_t* first_window, int32_t* n_windows,
                            int32_t* n_records);
/* The parsed records, as hc_sam_result_records; contig_of[k] is the table index of record k's RNAME, or -1. */
int hc_genome_result_sam(const hc_genome_result* res, const hc_sam_record** records, const int32_t** line_no,
                         int32_t* n_records, const uint32_t** cigar_pool, int32_t* n_words, const int32_t** contig_of);
/* Genome-wide window `window`: its contig, then as hc_contig_result_window, the bounds inside the contig. */
int hc_genome_result_window(const hc_genome_result* res, int32_t window, int32_t* contig, int64_t* padded_begin,
                            int64_t* padded_end, int64_t* origin_begin, int64_t* origin_end, int32_t* ref_len,
                            const int32_t** picked, int32_t* n_picked, int32_t* status, int32_t* asm_status,
                            int32_t* kmer_size, int32_t* n_haps);
/* As hc_contig_result_sites; `region` is the genome-wide window index, `begin` a position inside the contig. */
int hc_genome_result_sites(const hc_genome_result* res, const hc_gt_call_site** sites, int64_t* n);
/* As hc_contig_result_reads, of a genome-wide window. */
int hc_genome_result_reads(const hc_genome_result* res, int32_t window, const int32_t** reads, int32_t* n);
int hc_genome_result_free(hc_genome_result* res);

#ifdef __cplusplus
}
#endif
#endif /* HC_GENOME_H */
