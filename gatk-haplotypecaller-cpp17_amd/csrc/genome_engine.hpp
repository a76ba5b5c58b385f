// What the genome caller (genome_engine.cpp) shares with the fronts that feed
// it: hc_genome_call's SAM text (in genome_engine.cpp) and hc_bam_genome_call's
// BAM file (bam_engine.cpp). A front parses its input into records that stay on
// the device under the parser's lock, resolves every record's contig on the
// device, and names the host bytes the records' `line` offsets point into.
// Everything behind that (argument checks, the table, buckets, picks, the chain
// and the VCF) is genome_call's, once.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_genome.h"
#include "../../include/hc_intervals.h"
#include "genome_kernels.hpp"
#include "interval_host.hpp"
#include "sam_engine.hpp"
#include "stage_host.hpp"

struct hc_genome_result {
    hc_sam_result* sam = nullptr;
    std::vector<hc_call_result*> batches;
    int64_t region = 0, padding = 0;
    std::vector<std::string> names;          // per contig
    std::vector<int64_t> ref_len, win_off;   // per contig; n_contigs + 1: a contig's first window
    std::vector<int32_t> n_records;          // per contig: the records resolved to it
    std::vector<int32_t> contig_of;          // per record
    std::vector<int32_t> win_contig;         // per window
    std::vector<int64_t> win_first;          // n_windows + 1: a window's first pick
    std::vector<int32_t> picked;             // record indices
    std::vector<int32_t> status, asm_status, kmer_size, n_haps;   // per window
    std::vector<hc_gt_call_site> sites;      // `region` renumbered to the genome-wide window
    std::vector<std::vector<int32_t>> reads; // per window: the surviving reads, record indices
    std::string vcf;
    std::vector<uint8_t> bases;              // of a BAM call: what the records' `line` offsets point into
    bool with_intervals = false;             // of an interval call (hc_intervals.h)
    hcgenome::Merged merged;                 //   its merged intervals
    std::vector<int32_t> asked;              //   the asked windows, ascending
    int32_t idx_chunks = 0, idx_members = 0; //   of an indexed BAM call: chunks after merging, members read,
    int64_t idx_bytes_up = 0, idx_records = 0;   // compressed bytes uploaded, records framed
    ~hc_genome_result();
};

namespace hcgenome {

// The contig table as the device reads it, in one block: [ref_len | off | win_off | name_off | slots | pool].
struct Table {
    std::vector<char> blob;
    size_t o_len = 0, o_off = 0, o_win = 0, o_name = 0, o_slots = 0, o_pool = 0;
    uint32_t n_slots = 0;
    std::vector<int64_t> off;   // n_contigs + 1
    // The hash table over the host's copy.
    GenomeTable view() const
    {
        return GenomeTable{reinterpret_cast<const int32_t*>(blob.data() + o_slots), n_slots - 1u,
                           reinterpret_cast<const int32_t*>(blob.data() + o_name),
                           reinterpret_cast<const uint8_t*>(blob.data() + o_pool)};
    }
};

struct Front {
    virtual ~Front() = default;
    // Before anything else: the front's own argument errors.
    virtual int check() const = 0;
    // The parse. On success res.sam holds the records, `lk` owns the parser's
    // lock and `dev` names the records on the device until `lk` is released.
    virtual int open(hc_genome_result& res, const Table& t, stage_host::Trace& tr, std::unique_lock<std::mutex>& lk,
                     hcsam::Resident& dev) = 0;
    // a.contig_of[k] for every record, on `st`.
    virtual hipError_t resolve(const GenomeArgs& a, hipStream_t st) = 0;
    // The host bytes the records view (after open).
    virtual const uint8_t* text() const = 0;
    // Of an error message: "line 12: " (line_no as the records carry it).
    virtual std::string where(int64_t line_no) const = 0;
    // Of an unplaced record k whose reference is not in the table: its name, cut at 64 bytes.
    virtual std::string rname(const hc_sam_record& r, size_t k) const = 0;
};

// The intervals of an interval call, as the caller gave them (checked by genome_call).
struct Asking {
    const hc_interval* intervals;
    int32_t n;
};

// `ask` null: the plain call, every window of every contig.
int genome_call(Front& front, const hc_genome_contig* contigs, int32_t n_contigs, int32_t region_size, int32_t padding_size,
                uint64_t seed, int32_t pick_mode, uint32_t flags, hc_genome_result** out, const Asking* ask = nullptr);

}  // namespace hcgenome
