// Host engine + C ABI of the genome caller (include/hc_genome.h): every contig
// of a SAM text in one call.
//
//   the contig table: names into a pool and an open-addressing hash table
//             (genome_body.hpp), the exclusive sums of the lengths and of the
//             window counts; one upload
//   hc_sam_parse (kept on the device with the text, the parser's lock held
//             until the picks are back)
//   resolve:  contig_of per record, read back for the result
//   scope:    (an interval call, include/hc_intervals.h) the list checked and merged on the
//             host before any device work; asked per window and scope per record on the
//             device (interval_kernels.hip), their counts back. The buckets then pass over
//             the records out of scope and the picks run over the asked windows only
//   buckets:  place, scan, scatter, sort over the concatenated positions (dense),
//             or keys, a stable radix sort of (key, record) and the run table,
//             sized by the records (HC_GENOME_SORTED_BUCKETS, genome_sort_kernels.hip)
//   picks:    one wave per genome-wide window: count, scan, a small readback of
//             the offsets and the error word, then write and the readback of the picks
//   hc_call_window structs on the worker pool, `ref` aimed into the window's own contig
//   hc_call_windows, under its own lock, in batches of HC_CONTIG_BATCH_WINDOWS
//             sent windows whatever their contigs
//   the VCF text
//
// The engine owns the table and the tiling workspace: grow-only buffers of the
// shared host layer (stage_host.hpp), released by hc_phmm_shutdown. Its kernels
// run on the parser's stream. HC_GENOME_TRACE=1 prints the host wall clock of
// the phases on stderr.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_bam.h"
#include "../../include/hc_genome.h"
#include "genome_engine.hpp"
#include "genome_kernels.hpp"
#include "genome_sort_kernels.hpp"
#include "interval_kernels.hpp"
#include "pool.hpp"
#include "sam_engine.hpp"
#include "sam_kernels.hpp"
#include "stage_host.hpp"

using namespace hcgenome;
using namespace stage_host;

hc_genome_result::~hc_genome_result()
{
    for (hc_call_result* b : batches) (void)hc_call_result_free(b);
    (void)hc_sam_result_free(sam);
}

namespace {

// No stream of its own: the kernels run on the parser's, under the parser's lock.
Buf g_tab, g_pos, g_sort, g_win, g_picks, g_rec, g_htab{nullptr, 0, true}, g_hback{nullptr, 0, true}, g_hpicks{nullptr, 0, true},
    g_hrec{nullptr, 0, true};
Buf g_iv, g_hiv{nullptr, 0, true};   // of an interval call: the merged intervals, asked and scope
Stage g_st({&g_tab, &g_pos, &g_sort, &g_win, &g_picks, &g_rec, &g_htab, &g_hback, &g_hpicks, &g_hrec, &g_iv, &g_hiv}, false);

constexpr uint32_t kKnownFlags = HC_CONTIG_F64 | HC_CONTIG_DEFAULT_MODE | HC_CONTIG_WANT_SITE_READS | HC_CONTIG_SKIP_UNPLACED |
                                 HC_GENOME_SORTED_BUCKETS;

// HC_GENOME_BUCKETS, read per call: "sorted" sets HC_GENOME_SORTED_BUCKETS, "dense" or unset changes nothing.
int buckets_from_env(uint32_t& flags)
{
    const char* e = std::getenv("HC_GENOME_BUCKETS");
    if (!e || std::strcmp(e, "dense") == 0) return HC_PHMM_OK;
    if (std::strcmp(e, "sorted") != 0) return fail(HC_PHMM_EINVAL, "HC_GENOME_BUCKETS is neither sorted nor dense");
    flags |= HC_GENOME_SORTED_BUCKETS;
    return HC_PHMM_OK;
}

int32_t batch_windows()
{
    const char* e = std::getenv("HC_CONTIG_BATCH_WINDOWS");
    const long v = e ? std::atol(e) : 0;
    return v >= 1 && v <= (1 << 20) ? int32_t(v) : 512;
}

const char* defect_text(int d)
{
    switch (d) {
        case HC_SAM_DEFECT_POS_ZERO: return "pos == 0";
        case HC_SAM_DEFECT_NO_CIGAR: return "n_cigar == 0";
        case HC_SAM_DEFECT_CIGAR_LENGTH: return "the CIGAR's read length differs from seq_len";
        case HC_SAM_DEFECT_QUAL_LENGTH: return "qual_len differs from seq_len";
        case HC_SAM_DEFECT_TOO_LONG: return "seq_len above HC_PHMM_MAX_READ_LEN";
        case HC_SAM_DEFECT_QUAL_RANGE: return "a quality above 93";
        default: return "an unknown defect";
    }
}

struct Bounds {
    int64_t padded_begin, padded_end, origin_begin, origin_end;
    int32_t ref_len;
};

// Of genome-wide window w, inside its contig.
Bounds bounds_of(const hc_genome_result& r, int64_t w)
{
    const size_t c = size_t(r.win_contig[size_t(w)]);
    const int64_t lw = w - r.win_off[c];
    Bounds b;
    b.origin_begin = lw * r.region;
    b.origin_end = b.origin_begin + r.region;
    b.padded_begin = lw == 0 ? 0 : b.origin_begin - r.padding;
    b.padded_end = b.origin_end + r.padding;
    b.ref_len = int32_t(std::min(b.padded_end, r.ref_len[c]) - b.padded_begin);   // substr cuts at the contig's end
    return b;
}

// Names into the pool and the hash table; two equal names are an error.
int build_table(const hc_genome_contig* contigs, int32_t n, const hc_genome_result& res, Table& t)
{
    t.n_slots = genome_table_slots(n);
    size_t pool_bytes = 0;
    for (const std::string& s : res.names) pool_bytes += s.size();
    Carver c;
    t.o_len = c.take(sizeof(int64_t) * size_t(n));
    t.o_off = c.take(sizeof(int64_t) * (size_t(n) + 1));
    t.o_win = c.take(sizeof(int64_t) * (size_t(n) + 1));
    t.o_name = c.take(sizeof(int32_t) * (size_t(n) + 1));
    t.o_slots = c.take(sizeof(int32_t) * t.n_slots);
    t.o_pool = c.take(pool_bytes);
    t.blob.assign(c.off, 0);
    int64_t* len = reinterpret_cast<int64_t*>(t.blob.data() + t.o_len);
    int64_t* off = reinterpret_cast<int64_t*>(t.blob.data() + t.o_off);
    int64_t* win = reinterpret_cast<int64_t*>(t.blob.data() + t.o_win);
    int32_t* name_off = reinterpret_cast<int32_t*>(t.blob.data() + t.o_name);
    int32_t* slots = reinterpret_cast<int32_t*>(t.blob.data() + t.o_slots);
    uint8_t* pool = reinterpret_cast<uint8_t*>(t.blob.data() + t.o_pool);
    std::fill(slots, slots + t.n_slots, -1);
    GenomeTable view{slots, t.n_slots - 1u, name_off, pool};
    off[0] = 0;
    name_off[0] = 0;
    for (int32_t k = 0; k < n; ++k) {
        const std::string& s = res.names[size_t(k)];
        len[k] = contigs[k].ref_len;
        off[k + 1] = off[k] + len[k];
        win[k] = res.win_off[size_t(k)];
        // the lookup reads the names of the contigs before k only: theirs are the slots that are set
        uint32_t slot = 0;
        const int32_t same = genome_lookup(view, reinterpret_cast<const uint8_t*>(s.data()), int64_t(s.size()), slot);
        if (same >= 0)
            return fail(HC_PHMM_EINVAL, "contigs " + std::to_string(same) + " and " + std::to_string(k) + " have the same name");
        std::memcpy(pool + name_off[k], s.data(), s.size());
        name_off[k + 1] = name_off[k] + int32_t(s.size());
        slots[slot] = k;
    }
    win[n] = res.win_off[size_t(n)];
    t.off.assign(off, off + n + 1);
    return HC_PHMM_OK;
}

// The RNAME of the record at `line`, as the parser splits it, cut at 64 bytes.
std::string rname_of(const uint8_t* sam, int64_t sam_len, int64_t line)
{
    int64_t i = line;
    std::string out;
    for (int tok = 0; tok < 3; ++tok) {
        while (i < sam_len && hcsam::sam_space(sam[i])) ++i;
        const int64_t b = i;
        while (i < sam_len && !hcsam::sam_space(sam[i])) ++i;
        if (tok == 2) out.assign(reinterpret_cast<const char*>(sam) + b, size_t(std::min<int64_t>(i - b, 64)));
    }
    return out;
}

// Table upload, resolve, buckets and picks on the device; fills res.contig_of, res.win_first and res.picked.
int tile(Front& front, const hcsam::Resident& dev, const hc_sam_record* records, const int32_t* line_no, const Table& t, int32_t n_contigs, uint64_t seed, int32_t pick_mode, uint32_t flags, hc_genome_result& res, Trace& tr)
{
    hipStream_t st = dev.stream;
    const int64_t total_len = t.off[size_t(n_contigs)];
    const int32_t n_windows = int32_t(res.win_off[size_t(n_contigs)]);
    GenomeArgs a{};
    a.records = dev.records;
    a.line_no = dev.line_no;
    a.n_records = dev.n_records;
    a.text = dev.text;
    a.text_len = dev.text_len;
    a.n_contigs = n_contigs;
    a.total_len = total_len;
    a.skip_unplaced = (flags & HC_CONTIG_SKIP_UNPLACED) ? 1 : 0;
    a.n_windows = n_windows;
    a.region = res.region;
    a.padding = res.padding;
    a.seed = seed;
    a.pick_mode = pick_mode;
    a.n_asked = n_windows;   // scope and asked_list stay null: every record, every window

    // ---- an interval call's own workspace: [begin | end | first] go up, the rest is made on the device
    const Merged* iv = res.with_intervals ? &res.merged : nullptr;
    const size_t n_iv = iv ? iv->iv.size() : 0;
    Carver ic, ihc;
    size_t o_ib = 0, o_if = 0, iv_up = 0, o_asked = 0, o_afirst = 0, o_alist = 0, o_scope = 0, o_sfirst = 0, o_slist = 0, o_iscan = 0;
    size_t h_ib = 0, h_counts = 0, h_alist = 0;
    if (iv) {
        o_ib = ic.take(sizeof(int64_t) * 2 * n_iv);
        o_if = ic.take(sizeof(int32_t) * (size_t(n_contigs) + 1));
        iv_up = ic.off;
        o_asked = ic.take(sizeof(int32_t) * size_t(n_windows));
        o_afirst = ic.take(sizeof(int64_t) * (size_t(n_windows) + 1));
        o_alist = ic.take(sizeof(int32_t) * size_t(n_windows));
        o_scope = ic.take(sizeof(int32_t) * size_t(std::max(dev.n_records, 1)));
        o_sfirst = ic.take(sizeof(int64_t) * (size_t(std::max(dev.n_records, 1)) + 1));
        o_slist = ic.take(sizeof(int32_t) * size_t(std::max(dev.n_records, 1)));
        o_iscan = ic.take(std::max(hcsam::scan_work_bytes(n_windows), hcsam::scan_work_bytes(dev.n_records)));
        h_ib = ihc.take(iv_up);
        h_counts = ihc.take(sizeof(int64_t) * 2);
        h_alist = ihc.take(sizeof(int32_t) * size_t(n_windows));
        if (int rc = reserve(g_iv, ic.off, "interval call workspace")) return rc;
        if (int rc = reserve(g_hiv, ihc.off, "interval call staging")) return rc;
    }

    int rc = reserve(g_tab, t.blob.size(), "genome caller contig table");
    if (rc) return rc;
    rc = reserve(g_htab, t.blob.size(), "genome caller contig table staging");
    if (rc) return rc;
    const size_t rec_bytes = sizeof(int32_t) * size_t(std::max(dev.n_records, 1));
    rc = reserve(g_rec, rec_bytes, "genome caller record workspace");
    if (rc) return rc;
    rc = reserve(g_hrec, rec_bytes, "genome caller record readback");
    if (rc) return rc;
    // Dense: arrays over the concatenated positions. Sorted: nothing is sized by total_len.
    const bool sorted = (flags & HC_GENOME_SORTED_BUCKETS) != 0;
    const size_t n_rec = size_t(std::max(dev.n_records, 1));
    Carver pc;
    const size_t o_err = pc.take(sizeof(unsigned long long));
    size_t o_count = 0, o_cursor = 0, zero_bytes = 0, o_first = 0, o_bucket = 0, o_scan = 0;
    size_t o_key[2] = {0, 0}, o_index[2] = {0, 0}, o_hist = 0, o_hfirst = 0, o_rpos = 0, o_rfirst = 0;
    const int64_t n_hist = int64_t(kSortDigits) * sort_tiles(dev.n_records);
    if (!sorted) {
        o_count = pc.take(sizeof(int32_t) * size_t(total_len));
        o_cursor = pc.take(sizeof(int32_t) * size_t(total_len));
        zero_bytes = pc.off;   // [err | count | cursor] are set in front of every call
        o_first = pc.take(sizeof(int64_t) * (size_t(total_len) + 1));
        o_bucket = pc.take(sizeof(int32_t) * n_rec);
        o_scan = pc.take(std::max(hcsam::scan_work_bytes(total_len), hcsam::scan_work_bytes(n_windows)));
        rc = reserve(g_pos, pc.off, "genome caller position workspace");
    } else {
        for (int k = 0; k < 2; ++k) {
            o_key[k] = pc.take(sizeof(int64_t) * (n_rec + 1));
            o_index[k] = pc.take(sizeof(int32_t) * n_rec);
        }
        o_rpos = pc.take(sizeof(int64_t) * n_rec);
        o_rfirst = pc.take(sizeof(int64_t) * (n_rec + 1));
        o_hist = pc.take(sizeof(int32_t) * size_t(n_hist));
        o_hfirst = pc.take(sizeof(int64_t) * (size_t(n_hist) + 1));
        o_scan = pc.take(std::max({hcsam::scan_work_bytes(n_hist), hcsam::scan_work_bytes(dev.n_records),
                                   hcsam::scan_work_bytes(n_windows)}));
        rc = reserve(g_sort, pc.off, "genome caller sort workspace");
    }
    if (rc) return rc;
    Carver wc;
    const size_t o_np = wc.take(sizeof(int32_t) * size_t(n_windows));
    const size_t o_wf = wc.take(sizeof(int64_t) * (size_t(n_windows) + 1));
    rc = reserve(g_win, wc.off, "genome caller window workspace");
    if (rc) return rc;
    Carver hc;
    const size_t h_err = hc.take(sizeof(unsigned long long));
    const size_t h_wf = hc.take(sizeof(int64_t) * (size_t(n_windows) + 1));
    rc = reserve(g_hback, hc.off, "genome caller readback");
    if (rc) return rc;

    std::memcpy(g_htab.p, t.blob.data(), t.blob.size());
    HIP_TRY(st, hipMemcpyAsync(g_tab.p, g_htab.p, t.blob.size(), hipMemcpyHostToDevice, st));
    a.ref_len = reinterpret_cast<const int64_t*>(g_tab.p + t.o_len);
    a.off = reinterpret_cast<const int64_t*>(g_tab.p + t.o_off);
    a.win_off = reinterpret_cast<const int64_t*>(g_tab.p + t.o_win);
    a.table = GenomeTable{reinterpret_cast<const int32_t*>(g_tab.p + t.o_slots), t.n_slots - 1u,
                          reinterpret_cast<const int32_t*>(g_tab.p + t.o_name),
                          reinterpret_cast<const uint8_t*>(g_tab.p + t.o_pool)};
    a.contig_of = reinterpret_cast<int32_t*>(g_rec.p);
    char* work = sorted ? g_sort.p : g_pos.p;
    a.err = reinterpret_cast<unsigned long long*>(work + o_err);
    int64_t* first = nullptr;
    if (!sorted) {
        a.count = reinterpret_cast<int32_t*>(g_pos.p + o_count);
        a.cursor = reinterpret_cast<int32_t*>(g_pos.p + o_cursor);
        first = reinterpret_cast<int64_t*>(g_pos.p + o_first);
        a.first = first;
        a.bucket = reinterpret_cast<int32_t*>(g_pos.p + o_bucket);
    }
    int64_t* scan_work = reinterpret_cast<int64_t*>(work + o_scan);
    a.n_picked = reinterpret_cast<int32_t*>(g_win.p + o_np);
    int64_t* win_first = reinterpret_cast<int64_t*>(g_win.p + o_wf);
    a.win_first = win_first;

    HIP_TRY(st, front.resolve(a, st));
    if (dev.n_records)
        HIP_TRY(st, hipMemcpyAsync(g_hrec.p, g_rec.p, sizeof(int32_t) * size_t(dev.n_records), hipMemcpyDeviceToHost, st));
    if (tr.on) {
        HIP_TRY(st, hipStreamSynchronize(st));
        tr.mark("resolve");
    }
    // ---- an interval call: the asked windows and the records in scope, their counts back
    int32_t n_scoped = dev.n_records;
    const int32_t* scoped_list = nullptr;
    if (iv) {
        char* up_at = g_hiv.p + h_ib;
        if (n_iv) {
            std::memcpy(up_at + o_ib, iv->begin.data(), sizeof(int64_t) * n_iv);
            std::memcpy(up_at + o_ib + sizeof(int64_t) * n_iv, iv->end.data(), sizeof(int64_t) * n_iv);
        }
        std::memcpy(up_at + o_if, iv->first.data(), sizeof(int32_t) * (size_t(n_contigs) + 1));
        HIP_TRY(st, hipMemcpyAsync(g_iv.p, up_at, iv_up, hipMemcpyHostToDevice, st));
        IntervalArgs ia{};
        ia.g = a;
        ia.set = IntervalSet{reinterpret_cast<const int64_t*>(g_iv.p + o_ib), reinterpret_cast<const int64_t*>(g_iv.p + o_ib) + n_iv,
                             reinterpret_cast<const int32_t*>(g_iv.p + o_if)};
        ia.asked = reinterpret_cast<int32_t*>(g_iv.p + o_asked);
        ia.asked_first = reinterpret_cast<int64_t*>(g_iv.p + o_afirst);
        ia.asked_list = reinterpret_cast<int32_t*>(g_iv.p + o_alist);
        ia.scope = reinterpret_cast<int32_t*>(g_iv.p + o_scope);
        ia.scope_first = reinterpret_cast<int64_t*>(g_iv.p + o_sfirst);
        ia.scoped_list = reinterpret_cast<int32_t*>(g_iv.p + o_slist);
        ia.scan_work = reinterpret_cast<int64_t*>(g_iv.p + o_iscan);
        HIP_TRY(st, launch_interval_ask(ia, st));
        HIP_TRY(st, launch_interval_scope(ia, st));
        HIP_TRY(st, hipMemcpyAsync(g_hiv.p + h_counts, ia.asked_first + n_windows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(st, hipMemcpyAsync(g_hiv.p + h_counts + sizeof(int64_t), ia.scope_first + dev.n_records, sizeof(int64_t),
                                   hipMemcpyDeviceToHost, st));
        HIP_TRY(st, hipStreamSynchronize(st));
        int64_t counts[2];
        std::memcpy(counts, g_hiv.p + h_counts, sizeof(counts));
        if (counts[0] < 0 || counts[0] > n_windows || counts[1] < 0 || counts[1] > dev.n_records)
            return fail(HC_PHMM_EHIP, "interval call: asked or scoped count out of its bound");
        a.n_asked = int32_t(counts[0]);
        a.asked_list = ia.asked_list;
        a.scope = ia.scope;
        n_scoped = int32_t(counts[1]);
        scoped_list = ia.scoped_list;
        if (a.n_asked)   // complete at the sync behind the pick counts
            HIP_TRY(st, hipMemcpyAsync(g_hiv.p + h_alist, ia.asked_list, sizeof(int32_t) * size_t(a.n_asked), hipMemcpyDeviceToHost, st));
        tr.mark("scope");
    }
    GenomeSortArgs s{};
    if (!sorted) {
        HIP_TRY(st, hipMemsetAsync(g_pos.p, 0, zero_bytes, st));
        HIP_TRY(st, hipMemsetAsync(a.err, 0xFF, sizeof(unsigned long long), st));
        HIP_TRY(st, launch_place(a, st));
        HIP_TRY(st, hcsam::launch_scan(a.count, total_len, first, scan_work, st));
        HIP_TRY(st, launch_scatter(a, st));
        HIP_TRY(st, launch_sort(a, st));
    } else {
        s.g = a;
        s.n = n_scoped;   // a plain call: every record
        s.scoped = scoped_list;
        for (int k = 0; k < 2; ++k) {
            s.key[k] = reinterpret_cast<int64_t*>(g_sort.p + o_key[k]);
            s.index[k] = reinterpret_cast<int32_t*>(g_sort.p + o_index[k]);
        }
        s.hist = reinterpret_cast<int32_t*>(g_sort.p + o_hist);
        s.hist_first = reinterpret_cast<int64_t*>(g_sort.p + o_hfirst);
        s.scan_work = scan_work;
        s.run_pos = reinterpret_cast<int64_t*>(g_sort.p + o_rpos);
        s.run_first = reinterpret_cast<int64_t*>(g_sort.p + o_rfirst);
        s.passes = sort_passes(total_len);
        HIP_TRY(st, hipMemsetAsync(a.err, 0xFF, sizeof(unsigned long long), st));
        HIP_TRY(st, launch_sorted_buckets(s, st));
    }
    if (tr.on) {
        HIP_TRY(st, hipStreamSynchronize(st));
        tr.mark("buckets");
    }
    // ---- the picks: their counts first, so that the lists take what they need and no more
    if (iv) HIP_TRY(st, hipMemsetAsync(a.n_picked, 0, sizeof(int32_t) * size_t(n_windows), st));   // a window not asked picks nothing
    HIP_TRY(st, sorted ? launch_sorted_pick_count(s, st) : launch_pick_count(a, st));
    HIP_TRY(st, hcsam::launch_scan(a.n_picked, n_windows, win_first, scan_work, st));
    HIP_TRY(st, hipMemcpyAsync(g_hback.p + h_err, a.err, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(st, hipMemcpyAsync(g_hback.p + h_wf, win_first, sizeof(int64_t) * (size_t(n_windows) + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(st, hipStreamSynchronize(st));

    const int32_t* hc_of = reinterpret_cast<const int32_t*>(g_hrec.p);
    res.contig_of.assign(hc_of, hc_of + dev.n_records);
    res.n_records.assign(size_t(n_contigs), 0);
    for (int32_t c : res.contig_of) {
        if (c < -1 || c >= n_contigs) return fail(HC_PHMM_EHIP, "genome caller: a record's contig is out of its bound");
        if (c >= 0) ++res.n_records[size_t(c)];
    }
    if (iv) {
        const int32_t* ha = reinterpret_cast<const int32_t*>(g_hiv.p + h_alist);
        res.asked.assign(ha, ha + a.n_asked);
        for (size_t k = 0; k < res.asked.size(); ++k)
            if (res.asked[k] < 0 || res.asked[k] >= n_windows || (k && res.asked[k] <= res.asked[k - 1]))
                return fail(HC_PHMM_EHIP, "interval call: the asked windows do not ascend inside their bound");
    }
    unsigned long long err = 0;
    std::memcpy(&err, g_hback.p + h_err, sizeof(err));
    if (err != kNoError) {
        const int64_t key = int64_t(err >> 4);
        if ((err & 15ull) == kErrDepth) {
            const size_t c = size_t(std::upper_bound(t.off.begin(), t.off.end(), key - 1) - t.off.begin()) - 1;
            if (key < 1 || key > total_len) return fail(HC_PHMM_EHIP, "genome caller: error word names no position");
            return fail(HC_PHMM_EINVAL, "more than " + std::to_string(HC_CONTIG_MAX_READS_PER_POSITION) +
                                            " reads begin at position " + std::to_string(key - t.off[c]) +
                                            " (1-based) of contig " + res.names[c]);
        }
        const int32_t* at = std::lower_bound(line_no, line_no + dev.n_records, int32_t(key));
        if (at == line_no + dev.n_records || *at != key) return fail(HC_PHMM_EHIP, "genome caller: error word names no record");
        const size_t k = size_t(at - line_no);
        const hc_sam_record& r = records[k];
        const std::string where = front.where(key);
        if ((err & 15ull) == kErrUnplaced) {
            const int32_t c = res.contig_of[k];
            if (c < 0)
                return fail(HC_PHMM_EINVAL, where + "unplaced read, RNAME " + front.rname(r, k) +
                                                " is not in the contig table");
            return fail(HC_PHMM_EINVAL, where + "unplaced read, POS " + std::to_string(r.pos) + " is 0 or past the " +
                                            std::to_string(res.ref_len[size_t(c)]) + " bases of contig " + res.names[size_t(c)]);
        }
        return fail(HC_PHMM_EINVAL, where + "a read that passes the flag filters has " + defect_text(r.defect));
    }
    const int64_t* hf = reinterpret_cast<const int64_t*>(g_hback.p + h_wf);
    res.win_first.assign(hf, hf + n_windows + 1);
    const int64_t total = res.win_first[size_t(n_windows)];
    const int64_t span = res.region + 2 * res.padding;   // a window picks at most one read per position of its padded interval
    for (int32_t w = 0; w < n_windows; ++w) {
        const int64_t n = res.win_first[size_t(w) + 1] - res.win_first[size_t(w)];
        if (res.win_first[0] != 0 || n < 0 || n > span) return fail(HC_PHMM_EHIP, "genome caller: pick counts out of their bound");
    }
    const size_t pick_bytes = sizeof(int32_t) * size_t(total);
    rc = reserve(g_picks, pick_bytes, "genome caller picks");
    if (rc) return rc;
    rc = reserve(g_hpicks, pick_bytes, "genome caller picks readback");
    if (rc) return rc;
    a.picked = reinterpret_cast<int32_t*>(g_picks.p);
    s.g.picked = a.picked;
    if (total) {
        HIP_TRY(st, sorted ? launch_sorted_pick_write(s, st) : launch_pick_write(a, st));
        HIP_TRY(st, hipMemcpyAsync(g_hpicks.p, g_picks.p, pick_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(st, hipStreamSynchronize(st));
    }
    tr.mark("picks");
    tr.count("sorted", sorted ? 1 : 0);
    tr.count("sort_passes", sorted ? s.passes : 0);
    tr.count("tile_bytes", int64_t(rec_bytes + pc.off + wc.off));   // asked of the record, position / sort and window workspaces
    if (iv) {
        tr.count("intervals", int64_t(n_iv));
        tr.count("asked", a.n_asked);
        tr.count("scoped", n_scoped);
    }
    const int32_t* hp = reinterpret_cast<const int32_t*>(g_hpicks.p);
    res.picked.assign(hp, hp + total);
    for (int32_t k : res.picked)
        if (k < 0 || k >= dev.n_records) return fail(HC_PHMM_EHIP, "genome caller: a pick is out of its bound");
    return HC_PHMM_OK;
}

void print_site(std::string& out, const std::string& contig, const hc_gt_call_site& s)
{
    out += contig;
    out += '\t';
    out += std::to_string(s.begin + 1);
    out += "\t.\t";
    out += s.alleles[0];
    out += '\t';
    for (int32_t i = 1; i < s.n_alleles; ++i) {
        out += s.alleles[i];
        out += i == s.n_alleles - 1 ? '\t' : ',';
    }
    out += ".\t.\t.\tGT:GQ\t";
    out += std::to_string(s.a1) + '/' + std::to_string(s.a2) + ':' + std::to_string(s.genotype_quality) + '\n';
}

int run(Front& front, const hc_genome_contig* contigs, int32_t n_contigs, const Table& t, uint64_t seed,
        int32_t pick_mode, uint32_t flags, hc_genome_result& res)
{
    Trace tr("HC_GENOME_TRACE", "[hc_genome]");
    const int32_t n_windows = int32_t(res.win_off[size_t(n_contigs)]);
    res.win_contig.resize(size_t(n_windows));
    for (int32_t c = 0; c < n_contigs; ++c)
        std::fill(res.win_contig.begin() + res.win_off[size_t(c)], res.win_contig.begin() + res.win_off[size_t(c) + 1], c);
    const hc_sam_record* records = nullptr;
    const int32_t* line_no = nullptr;
    const uint32_t* pool = nullptr;
    int32_t n_records = 0;
    {
        std::unique_lock<std::mutex> parser;   // held while the records and the text on the device are in use
        hcsam::Resident dev;
        int rc = front.open(res, t, tr, parser, dev);
        if (rc) return rc;
        rc = hc_sam_result_records(res.sam, &records, &line_no, &n_records, &pool, nullptr, nullptr);
        if (rc) return rc;
        HIP_TRY(dev.stream, hipSetDevice(hcphmm::primary_device()));
        rc = tile(front, dev, records, line_no, t, n_contigs, seed, pick_mode, flags, res, tr);
        if (rc) return rc;
    }

    // ---- the chain's structs: views into the front's text and the parser's pool
    const uint8_t* sam = front.text();
    const int64_t total = res.win_first[size_t(n_windows)];
    std::vector<hc_prep_read> reads(static_cast<size_t>(total));
    std::vector<const uint8_t*> bases(static_cast<size_t>(total)), quals(static_cast<size_t>(total));
    hcphmm::parallel_for(total, [&](int64_t lo, int64_t hi) {
        for (int64_t k = lo; k < hi; ++k) {
            const hc_sam_record& r = records[res.picked[size_t(k)]];
            hc_prep_read& d = reads[size_t(k)];
            d = hc_prep_read{};
            d.cigar = r.n_cigar ? pool + r.cigar : nullptr;
            d.n_cigar = r.n_cigar;
            d.pos = r.pos;
            // a read too long for the chain got here behind a flag filter: its bases are never looked at
            d.seq_len = r.seq_len > HC_PHMM_MAX_READ_LEN ? 0 : r.seq_len;
            d.flag = r.flag;
            d.mapq = r.mapq;
            d.mate_same_contig = r.mate_same_contig;
            bases[size_t(k)] = sam + r.line + r.seq_off;
            quals[size_t(k)] = sam + r.line + r.qual_off;
        }
    });
    std::vector<int32_t> sent;   // the windows with reads, of all contigs
    for (int32_t w = 0; w < n_windows; ++w)
        if (res.win_first[size_t(w) + 1] > res.win_first[size_t(w)]) sent.push_back(w);
    res.status.assign(size_t(n_windows), res.with_intervals ? HC_CALL_NOT_ASKED : HC_CALL_NO_READS);
    for (int32_t w : res.asked) res.status[size_t(w)] = HC_CALL_NO_READS;
    res.asm_status.assign(size_t(n_windows), HC_ASM_NO_HAPLOTYPES);
    res.kmer_size.assign(size_t(n_windows), 0);
    res.n_haps.assign(size_t(n_windows), 0);
    res.reads.resize(size_t(n_windows));
    tr.mark("structs");

    // ---- the chain, batch by batch: a batch does not end where a contig does
    const uint32_t call_flags = flags & (HC_CONTIG_F64 | HC_CONTIG_DEFAULT_MODE | HC_CONTIG_WANT_SITE_READS);
    const size_t per = size_t(batch_windows());
    std::vector<hc_call_window> cw;
    int64_t n_calls = 0;
    for (size_t b0 = 0; b0 < sent.size(); b0 += per) {
        const size_t nb = std::min(per, sent.size() - b0);
        cw.assign(nb, hc_call_window{});
        for (size_t k = 0; k < nb; ++k) {
            const int32_t w = sent[b0 + k];
            const size_t c = size_t(res.win_contig[size_t(w)]);
            const Bounds b = bounds_of(res, w);
            const int64_t at = res.win_first[size_t(w)];
            hc_call_window& g = cw[k];
            g.ref = contigs[c].ref + b.padded_begin;
            g.ref_len = b.ref_len;
            g.padded_begin = b.padded_begin;
            g.padded_end = b.padded_end;
            g.origin_begin = b.origin_begin;
            g.origin_end = std::min(b.origin_end, res.ref_len[c]);
            g.reads = reads.data() + at;
            g.bases = bases.data() + at;
            g.quals = quals.data() + at;
            g.n_reads = int32_t(res.win_first[size_t(w) + 1] - at);
        }
        hc_call_result* h = nullptr;
        int rc = hc_call_windows(cw.data(), int32_t(nb), call_flags, &h);
        if (rc) return rc;
        ++n_calls;
        res.batches.push_back(h);
        for (size_t k = 0; k < nb; ++k) {
            const int32_t w = sent[b0 + k];
            rc = hc_call_result_window(h, int32_t(k), &res.status[size_t(w)], &res.asm_status[size_t(w)],
                                       &res.kmer_size[size_t(w)], &res.n_haps[size_t(w)]);
            if (rc) return rc;
            const int32_t* idx = nullptr;
            int32_t n = 0;
            rc = hc_call_result_reads(h, int32_t(k), &idx, &n);
            if (rc) return rc;
            std::vector<int32_t>& v = res.reads[size_t(w)];
            v.resize(size_t(n));
            for (int32_t j = 0; j < n; ++j) v[size_t(j)] = res.picked[size_t(res.win_first[size_t(w)] + idx[j])];
        }
        const hc_gt_call_site* sites = nullptr;
        int64_t n_sites = 0;
        rc = hc_call_result_sites(h, &sites, &n_sites);
        if (rc) return rc;
        for (int64_t s = 0; s < n_sites; ++s) {
            hc_gt_call_site c = sites[s];
            c.region = sent[b0 + size_t(c.region)];
            res.sites.push_back(c);
        }
        tr.mark("chain");
    }

    // ---- the header once, then every contig's lines: the sites are in window order, which is table order
    res.vcf = "##fileformat=VCFv4.2\n"
              "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype Quality\">\n"
              "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tNA12878\n";
    // of an interval call: the sites that begin inside a merged interval of their contig
    if (!res.with_intervals) {
        for (const hc_gt_call_site& s : res.sites)
            if (s.status == HC_GT_SITE_EMITTED) print_site(res.vcf, res.names[size_t(res.win_contig[size_t(s.region)])], s);
    } else {
        const IntervalSet set{res.merged.begin.data(), res.merged.end.data(), res.merged.first.data()};
        for (const hc_gt_call_site& s : res.sites) {
            const int32_t c = res.win_contig[size_t(s.region)];
            if (s.status == HC_GT_SITE_EMITTED && interval_meets(set, c, s.begin, s.begin + 1)) print_site(res.vcf, res.names[size_t(c)], s);
        }
    }
    tr.mark("vcf");
    tr.value("contigs", double(n_contigs));
    tr.value("windows", double(n_windows));
    tr.value("sent", double(sent.size()));
    tr.value("chain_calls", double(n_calls));
    tr.value("picked_reads", double(total));
    return HC_PHMM_OK;
}

int check_name(const char* name, int32_t k)
{
    const std::string at = "contig " + std::to_string(k) + ": ";
    if (!name) return fail(HC_PHMM_EINVAL, at + "null name");
    const size_t n = strnlen(name, size_t(HC_GENOME_MAX_NAME_LEN) + 1);
    if (n == 0) return fail(HC_PHMM_EINVAL, at + "empty name");
    if (n > HC_GENOME_MAX_NAME_LEN) return fail(HC_PHMM_EINVAL, at + "name longer than " + std::to_string(HC_GENOME_MAX_NAME_LEN) + " bytes");
    if (n == 1 && name[0] == '*') return fail(HC_PHMM_EINVAL, at + "the name * stands for no contig");
    for (size_t i = 0; i < n; ++i)
        if (hcsam::sam_space(uint8_t(name[i]))) return fail(HC_PHMM_EINVAL, at + "white space in the name");
    return HC_PHMM_OK;
}

// hc_genome_call's front: the SAM text, parsed by hc_sam_parse and left on the device.
struct SamFront final : Front {
    const uint8_t* sam;
    int64_t sam_len;
    SamFront(const uint8_t* s, int64_t n) : sam(s), sam_len(n) {}
    int check() const override
    {
        return sam_len < 0 || (sam_len && !sam) ? fail(HC_PHMM_EINVAL, "null sam / negative length") : HC_PHMM_OK;
    }
    int open(hc_genome_result& res, const Table&, Trace& tr, std::unique_lock<std::mutex>& lk, hcsam::Resident& dev) override
    {
        const int rc = hcsam::parse_resident(sam, sam_len, &res.sam, lk, dev);
        if (!rc) tr.mark("parse");
        return rc;
    }
    hipError_t resolve(const GenomeArgs& a, hipStream_t st) override { return launch_resolve(a, st); }
    const uint8_t* text() const override { return sam; }
    std::string where(int64_t line_no) const override { return "line " + std::to_string(line_no) + ": "; }
    std::string rname(const hc_sam_record& r, size_t) const override { return rname_of(sam, sam_len, r.line); }
};

}  // namespace

int hcgenome::genome_call(Front& front, const hc_genome_contig* contigs, int32_t n_contigs, int32_t region_size,
                          int32_t padding_size, uint64_t seed, int32_t pick_mode, uint32_t flags_in, hc_genome_result** out,
                          const Asking* ask)
{
    std::lock_guard<std::mutex> lk(g_st.mu);
    return call_frame(out, nullptr, [&](hc_genome_result& res) -> int {
        uint32_t flags = flags_in;
        if (int rc = front.check()) return rc;
        if (!contigs) return fail(HC_PHMM_EINVAL, "null contigs");
        if (n_contigs < 1) return fail(HC_PHMM_EINVAL, "n_contigs below 1");
        if (n_contigs > HC_GENOME_MAX_CONTIGS) return fail(HC_PHMM_EINVAL, "more than " + std::to_string(HC_GENOME_MAX_CONTIGS) + " contigs");
        if (flags & ~kKnownFlags) return fail(HC_PHMM_EINVAL, "unknown flags");
        if (int rc = buckets_from_env(flags)) return rc;
        if (pick_mode != HC_CONTIG_PICK_SEEDED && pick_mode != HC_CONTIG_PICK_FIRST) return fail(HC_PHMM_EINVAL, "unknown pick mode");
        if (region_size < 1) return fail(HC_PHMM_EINVAL, "region_size below 1");
        if (padding_size < 0 || padding_size > region_size) return fail(HC_PHMM_EINVAL, "padding_size outside 0 .. region_size");
        if (int64_t(region_size) + 2 * int64_t(padding_size) > HC_GT_MAX_REF_LEN)
            return fail(HC_PHMM_EINVAL, "region_size + 2 * padding_size above " + std::to_string(HC_GT_MAX_REF_LEN));
        res.region = region_size;
        res.padding = padding_size;
        res.win_off.assign(1, 0);
        for (int32_t k = 0; k < n_contigs; ++k) {
            if (int rc = check_name(contigs[k].name, k)) return rc;
            if (!contigs[k].ref) return fail(HC_PHMM_EINVAL, "contig " + std::to_string(k) + ": null ref");
            if (contigs[k].ref_len < 1) return fail(HC_PHMM_EINVAL, "contig " + std::to_string(k) + ": ref_len below 1");
            res.names.emplace_back(contigs[k].name);
            res.ref_len.push_back(contigs[k].ref_len);
            res.win_off.push_back(res.win_off.back() + (contigs[k].ref_len + region_size - 1) / region_size);
            if (res.win_off.back() > 0x7fffffffLL) return fail(HC_PHMM_EINVAL, "more than 2147483647 windows");
        }
        if (ask) {
            if (!ask->intervals) return fail(HC_PHMM_EINVAL, "null intervals");
            if (ask->n < 1) return fail(HC_PHMM_EINVAL, "n_intervals below 1");
            std::string why;
            const int64_t bad = interval_check(ask->intervals, ask->n, res.ref_len.data(), n_contigs, why);
            if (bad >= 0) return fail(HC_PHMM_EINVAL, "interval " + std::to_string(bad) + ": " + why);
            interval_merge(ask->intervals, ask->n, n_contigs, res.merged);
            res.with_intervals = true;
        }
        Table t;
        if (int rc = build_table(contigs, n_contigs, res, t)) return rc;
        return run(front, contigs, n_contigs, t, seed, pick_mode, flags, res);
    });
}

extern "C" int hc_genome_call(const uint8_t* sam, int64_t sam_len, const hc_genome_contig* contigs, int32_t n_contigs,
                              int32_t region_size, int32_t padding_size, uint64_t seed, int32_t pick_mode, uint32_t flags,
                              hc_genome_result** out)
{
    SamFront front(sam, sam_len);
    return genome_call(front, contigs, n_contigs, region_size, padding_size, seed, pick_mode, flags, out);
}

extern "C" int hc_genome_call_intervals(const uint8_t* sam, int64_t sam_len, const hc_genome_contig* contigs, int32_t n_contigs,
                                        const hc_interval* intervals, int32_t n_intervals, int32_t region_size,
                                        int32_t padding_size, uint64_t seed, int32_t pick_mode, uint32_t flags,
                                        hc_genome_result** out)
{
    SamFront front(sam, sam_len);
    const Asking ask{intervals, n_intervals};
    return genome_call(front, contigs, n_contigs, region_size, padding_size, seed, pick_mode, flags, out, &ask);
}

extern "C" int hc_genome_result_intervals(const hc_genome_result* res, const hc_interval** merged, int32_t* n_merged,
                                          const int32_t** asked, int32_t* n_asked)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (merged) *merged = res->merged.iv.data();
    if (n_merged) *n_merged = int32_t(res->merged.iv.size());
    if (asked) *asked = res->asked.data();
    if (n_asked) *n_asked = int32_t(res->asked.size());
    return HC_PHMM_OK;
}

extern "C" int hc_genome_result_vcf(const hc_genome_result* res, const char** text, int64_t* length, int32_t* n_windows,
                                    int32_t* n_contigs)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (text) *text = res->vcf.c_str();
    if (length) *length = int64_t(res->vcf.size());
    if (n_windows) *n_windows = int32_t(res->status.size());
    if (n_contigs) *n_contigs = int32_t(res->names.size());
    return HC_PHMM_OK;
}

extern "C" int hc_genome_result_contig(const hc_genome_result* res, int32_t contig, int32_t* first_window, int32_t* n_windows,
                                       int32_t* n_records)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (contig < 0 || size_t(contig) >= res->names.size()) return fail(HC_PHMM_EINVAL, "contig index out of range");
    const size_t c = size_t(contig);
    if (first_window) *first_window = int32_t(res->win_off[c]);
    if (n_windows) *n_windows = int32_t(res->win_off[c + 1] - res->win_off[c]);
    if (n_records) *n_records = res->n_records[c];
    return HC_PHMM_OK;
}

extern "C" int hc_genome_result_sam(const hc_genome_result* res, const hc_sam_record** records, const int32_t** line_no,
                                    int32_t* n_records, const uint32_t** cigar_pool, int32_t* n_words, const int32_t** contig_of)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (contig_of) *contig_of = res->contig_of.data();
    return hc_sam_result_records(res->sam, records, line_no, n_records, cigar_pool, n_words, nullptr);
}

extern "C" int hc_genome_result_window(const hc_genome_result* res, int32_t window, int32_t* contig, int64_t* padded_begin,
                                       int64_t* padded_end, int64_t* origin_begin, int64_t* origin_end, int32_t* ref_len,
                                       const int32_t** picked, int32_t* n_picked, int32_t* status, int32_t* asm_status,
                                       int32_t* kmer_size, int32_t* n_haps)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (window < 0 || size_t(window) >= res->status.size()) return fail(HC_PHMM_EINVAL, "window index out of range");
    const size_t w = size_t(window);
    const Bounds b = bounds_of(*res, window);
    if (contig) *contig = res->win_contig[w];
    if (padded_begin) *padded_begin = b.padded_begin;
    if (padded_end) *padded_end = b.padded_end;
    if (origin_begin) *origin_begin = b.origin_begin;
    if (origin_end) *origin_end = b.origin_end;
    if (ref_len) *ref_len = b.ref_len;
    if (picked) *picked = res->picked.data() + res->win_first[w];
    if (n_picked) *n_picked = int32_t(res->win_first[w + 1] - res->win_first[w]);
    if (status) *status = res->status[w];
    if (asm_status) *asm_status = res->asm_status[w];
    if (kmer_size) *kmer_size = res->kmer_size[w];
    if (n_haps) *n_haps = res->n_haps[w];
    return HC_PHMM_OK;
}

extern "C" int hc_genome_result_sites(const hc_genome_result* res, const hc_gt_call_site** sites, int64_t* n)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (sites) *sites = res->sites.data();
    if (n) *n = int64_t(res->sites.size());
    return HC_PHMM_OK;
}

extern "C" int hc_genome_result_reads(const hc_genome_result* res, int32_t window, const int32_t** reads, int32_t* n)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (window < 0 || size_t(window) >= res->reads.size()) return fail(HC_PHMM_EINVAL, "window index out of range");
    if (reads) *reads = res->reads[size_t(window)].data();
    if (n) *n = int32_t(res->reads[size_t(window)].size());
    return HC_PHMM_OK;
}

extern "C" int hc_genome_result_free(hc_genome_result* res)
{
    delete res;
    return HC_PHMM_OK;
}
