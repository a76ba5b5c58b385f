/*
 * hc_asm.h — C ABI of the MI355X assembler (in libhcpairhmm.so).
 *
 * Assembler::assemble (src/haplotypecaller/assembler/assembler.hpp:56-68) over
 * GraphWrapper (assembler/graph_wrapper.hpp) for many regions at once: reads and
 * the padded reference window in, candidate haplotypes out. Passed to
 * hc_region_call (hc_region.h) with cigar == NULL they complete the chain of
 * HaplotypeCaller::call_region.
 *
 * Per region, as the reference does it:
 *   attempts     k = 25, 35, .., 105; the first attempt that is accepted wins.
 *                An attempt is refused when ref_len < k (SHORT_REF), when it sees
 *                more than 2000 unique k-mers (TOO_MANY_KMERS) or when the
 *                filtered graph has a cycle (CYCLE).
 *   segments     maximal runs of bases with base != 'N' and (signed char)qual >= 43,
 *                kept for attempt k when at least k long; bytes are compared raw.
 *   graph        duplicate k-mers (twice within one sequence), threading of the
 *                window then the segments in order, edge filter
 *                is_ref || count >= 2 || out_degree(source) == 1.
 *   haplotypes   every source -> sink path depth first in out-edge order, scored
 *                by sum of log10(count / sum of on-path sibling counts), sorted
 *                by score descending with std::sort and the reference's comparator
 *                over the paths in discovery order, the first HC_ASM_MAX_HAPS
 *                kept. Among equal scores that is the reference's order (and its
 *                choice at the cut) wherever both are built with the same C++
 *                library: discovery order for up to 16 paths with libstdc++,
 *                introsort's permutation beyond.
 *
 * The graph is built on the device (one workgroup per region), the paths are
 * enumerated and scored on the host (glibc log10). Deviation from the reference:
 * an attempt with more than HC_ASM_MAX_PATHS paths ends the region as
 * HC_ASM_TOO_COMPLEX with no haplotypes; the reference enumerates without bound.
 *
 * Status codes of the calls are the HC_PHMM_* codes of hc_pairhmm.h; message via
 * hc_phmm_last_error(). Invalid input (null pointers, ref_len outside
 * 1 .. HC_GT_MAX_REF_LEN, negative lengths, quals == NULL with length > 0, a read
 * longer than HC_PHMM_MAX_READ_LEN, more than HC_ASM_MAX_REGION_READ_BASES read
 * bases in a region) is HC_PHMM_EINVAL before any device work. An internal bound
 * hit on the device (a graph of more than HC_ASM_MAX_GRAPH_EDGES on-path edges
 * among them) fails the call with HC_PHMM_EHIP; a graph is never silently wrong.
 * No CPU fallback. Calls are serialised under the assembler's own lock and run
 * on the engine's primary device.
 */
#ifndef HC_ASM_H
#define HC_ASM_H

#include <stdint.h>

#include "hc_gt.h"
#include "hc_pairhmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* region status */
#define HC_ASM_OK 0
#define HC_ASM_NO_HAPLOTYPES 1   /* all nine attempts refused */
#define HC_ASM_TOO_COMPLEX 2     /* more than HC_ASM_MAX_PATHS paths in the accepted attempt */

/* attempt outcome codes */
#define HC_ASM_NOT_TRIED 0
#define HC_ASM_SHORT_REF 1
#define HC_ASM_TOO_MANY_KMERS 2
#define HC_ASM_CYCLE 3
#define HC_ASM_ACCEPTED 4

#define HC_ASM_MAX_ATTEMPTS 9
#define HC_ASM_MAX_HAPS 128
#define HC_ASM_MAX_PATHS 65536
#define HC_ASM_MAX_REGION_READ_BASES 131072   /* sum of a region's read lengths */
#define HC_ASM_MAX_GRAPH_EDGES 16384          /* on-path edges of an accepted attempt */

typedef struct hc_asm_read {
    const uint8_t* bases;
    const uint8_t* quals;   /* ASCII, phred + 33 */
    int32_t length;         /* 0 .. HC_PHMM_MAX_READ_LEN */
} hc_asm_read;

typedef struct hc_asm_region {
    const uint8_t* ref;
    int32_t ref_len;          /* 1 .. HC_GT_MAX_REF_LEN */
    const hc_asm_read* reads;
    int32_t n_reads;          /* >= 0 */
} hc_asm_region;

/* One on-path edge of the accepted attempt's graph. Edges come in creation
 * order, which is also the out-edge order of every vertex; vertex numbers are
 * the device's and carry no meaning. The k-mer of `to` is the k-mer of `from`
 * without its first byte, plus `base`. */
typedef struct hc_asm_edge {
    int32_t from, to;
    int32_t count;
    int32_t seq;      /* creation sequence number among all edges of the attempt */
    uint8_t base;     /* last byte of the target's k-mer */
    uint8_t is_ref;
    uint16_t reserved;
} hc_asm_edge;

#define HC_ASM_WANT_GRAPH 1u /* keep the reduced graphs for hc_asm_result_graph (tests, debugging) */

typedef struct hc_asm_result hc_asm_result;

/* One synchronous call. On success *out holds every region's result; release it
 * with hc_asm_result_free. All pointers the accessors return are owned by the handle. */
int hc_asm_assemble(const hc_asm_region* regions, int32_t n_regions, uint32_t flags, hc_asm_result** out);
/* status, the accepted k (0 when none), the nine attempt codes, the number of
 * haplotypes kept and of paths found (HC_ASM_MAX_PATHS + 1 when TOO_COMPLEX).
 * Any out pointer may be NULL. */
int hc_asm_result_region(const hc_asm_result* res, int32_t region, int32_t* status, int32_t* kmer_size,
                         const uint8_t** attempts, int32_t* n_haps, int64_t* n_paths);
/* Haplotype `hap` of `region` in final order; bases are not NUL-terminated. */
int hc_asm_result_hap(const hc_asm_result* res, int32_t region, int32_t hap, const uint8_t** bases, int32_t* length,
                      double* score);
/* HC_ASM_WANT_GRAPH: the on-path edges of the accepted attempt, the source and
 * the sink vertex (the source's k-mer is the window's first kmer_size bytes).
 * HC_PHMM_EINVAL without the flag; n_edges = 0, source = sink = -1 without an accepted attempt. */
int hc_asm_result_graph(const hc_asm_result* res, int32_t region, const hc_asm_edge** edges, int32_t* n_edges,
                        int32_t* source, int32_t* sink);
int hc_asm_result_free(hc_asm_result* res);

#ifdef __cplusplus
}
#endif
#endif /* HC_ASM_H */
