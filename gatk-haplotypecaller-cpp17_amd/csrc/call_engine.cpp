// Host engine + C ABI of the window caller (include/hc_call.h): call_region as
// one call. It chains the three public stage calls, each under its own lock:
//
//   hc_prep_reads      every window
//   hc_asm_assemble    the windows with a kept read; reads are views
//                      (bases + offset, quals + offset, length) into the caller's buffers
//   hc_region_call     the windows with more than one haplotype; cigar == NULL,
//                      read intervals from the preparation's records
//
// The engine owns no device memory: what it adds on the host is the views, the
// two early endings and the index maps of the result. HC_CALL_TRACE=1 prints
// the host wall clock of the phases and the three stage calls' durations on stderr.
#include <chrono>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_call.h"
#include "stage_host.hpp"

using namespace stage_host;

struct hc_call_result {
    uint32_t flags = 0;
    hc_prep_result* prep = nullptr;
    hc_asm_result* assembled = nullptr;
    hc_region_calls* calls = nullptr;
    std::vector<int32_t> status;       // per window
    std::vector<int32_t> asm_index;    // per window: its region in `assembled`, -1: none
    std::vector<int32_t> call_index;   // per window: its region in `calls`, -1: none
    std::vector<hc_gt_call_site> sites;   // `region` renumbered to the window
    std::vector<std::vector<int32_t>> reads;   // per window: the surviving reads, caller's indices
    ~hc_call_result()
    {
        (void)hc_region_calls_free(calls);
        (void)hc_asm_result_free(assembled);
        (void)hc_prep_result_free(prep);
    }
};

namespace {

std::mutex g_mu;

// sam/sam.hpp:30-32 (GOP, GCP): one constant buffer each, every view points at them.
const std::string& gap_open()
{
    static const std::string s(HC_PHMM_MAX_READ_LEN, 'I');
    return s;
}
const std::string& gap_continue()
{
    static const std::string s(HC_PHMM_MAX_READ_LEN, '+');
    return s;
}

constexpr uint32_t kKnownFlags =
    HC_CALL_F64 | HC_CALL_DEFAULT_MODE | HC_CALL_WANT_L | HC_CALL_WANT_SITE_READS | HC_CALL_WANT_CIGARS;

int validate(const hc_call_window* windows, int32_t n)
{
    for (int32_t w = 0; w < n; ++w) {
        const hc_call_window& g = windows[w];
        auto at = [&] { return "window " + std::to_string(w); };
        if (!g.ref) return fail(HC_PHMM_EINVAL, at() + ": null ref");
        if (g.ref_len < 1 || g.ref_len > HC_GT_MAX_REF_LEN)
            return fail(HC_PHMM_EINVAL, at() + ": ref_len outside 1 .. " + std::to_string(HC_GT_MAX_REF_LEN));
        if (g.n_reads < 0) return fail(HC_PHMM_EINVAL, at() + ": negative read count");
        if (g.n_reads && (!g.reads || !g.bases || !g.quals)) return fail(HC_PHMM_EINVAL, at() + ": null reads / bases / quals");
        for (int32_t j = 0; j < g.n_reads; ++j)
            if (g.reads[j].seq_len > 0 && (!g.bases[j] || !g.quals[j]))
                return fail(HC_PHMM_EINVAL, at() + " read " + std::to_string(j) + ": null bases / quals");
    }
    return HC_PHMM_OK;
}

int run(const hc_call_window* windows, int32_t n, uint32_t flags, hc_call_result& res)
{
    Trace tr("HC_CALL_TRACE", "[hc_call]");
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };

    // ---- :93-94
    std::vector<hc_prep_window> pw(static_cast<size_t>(n));
    for (int32_t w = 0; w < n; ++w)
        pw[size_t(w)] = hc_prep_window{windows[w].padded_begin, windows[w].padded_end, windows[w].reads, windows[w].n_reads};
    auto t = clock::now();
    int rc = hc_prep_reads(pw.data(), n, &res.prep);
    if (rc) return rc;
    tr.value("prep_call", ms_since(t));

    res.status.assign(size_t(n), HC_CALL_NO_READS);
    res.asm_index.assign(size_t(n), -1);
    res.call_index.assign(size_t(n), -1);
    res.reads.resize(size_t(n));

    // ---- :96, and the views of the other windows
    std::vector<hc_asm_region> ar;
    std::vector<std::vector<hc_asm_read>> views(static_cast<size_t>(n));
    std::vector<int32_t> asm_window;
    int64_t view_bytes = 0;
    for (int32_t w = 0; w < n; ++w) {
        const hc_prep_record* rec = nullptr;
        const int32_t* kept = nullptr;
        int32_t n_kept = 0;
        int64_t kept_bases = 0;
        rc = hc_prep_result_window(res.prep, w, &rec, nullptr, &kept, &n_kept, &kept_bases);
        if (rc) return rc;
        if (n_kept == 0) continue;
        if (kept_bases > HC_ASM_MAX_REGION_READ_BASES)
            return fail(HC_PHMM_EINVAL, "window " + std::to_string(w) + ": more than " +
                                            std::to_string(HC_ASM_MAX_REGION_READ_BASES) + " read bases after the preparation");
        std::vector<hc_asm_read>& v = views[size_t(w)];
        v.resize(size_t(n_kept));
        for (int32_t k = 0; k < n_kept; ++k) {
            const int32_t j = kept[k];
            v[size_t(k)] = hc_asm_read{windows[w].bases[j] + rec[j].offset, windows[w].quals[j] + rec[j].offset, rec[j].length};
        }
        view_bytes += kept_bases;
        res.reads[size_t(w)].assign(kept, kept + n_kept);
        res.asm_index[size_t(w)] = int32_t(ar.size());
        asm_window.push_back(w);
        ar.push_back(hc_asm_region{windows[w].ref, windows[w].ref_len, v.data(), n_kept});
    }
    tr.mark("views");

    // ---- :100
    t = clock::now();
    rc = hc_asm_assemble(ar.data(), int32_t(ar.size()), 0, &res.assembled);
    if (rc) return rc;
    tr.value("asm_call", ms_since(t));

    // ---- :101, and the region caller's input
    std::vector<hc_region_in> rin;
    std::vector<std::vector<hc_region_hap>> haps;
    std::vector<std::vector<hc_phmm_read>> reads;
    std::vector<std::vector<int64_t>> rb, re;
    std::vector<int32_t> call_window;
    const char* gop = gap_open().data();
    const char* gcp = gap_continue().data();
    for (size_t a = 0; a < ar.size(); ++a) {
        const int32_t w = asm_window[a];
        int32_t n_haps = 0;
        rc = hc_asm_result_region(res.assembled, int32_t(a), nullptr, nullptr, nullptr, &n_haps, nullptr);
        if (rc) return rc;
        if (n_haps <= 1) {
            res.status[size_t(w)] = HC_CALL_NO_VARIATION;
            continue;
        }
        res.status[size_t(w)] = HC_CALL_CALLED;
        res.call_index[size_t(w)] = int32_t(rin.size());
        call_window.push_back(w);
        haps.emplace_back(size_t(n_haps));
        for (int32_t h = 0; h < n_haps; ++h) {
            hc_region_hap& d = haps.back()[size_t(h)];
            d.alignment_begin = 0;
            d.cigar = nullptr;
            rc = hc_asm_result_hap(res.assembled, int32_t(a), h, &d.bases, &d.length, nullptr);
            if (rc) return rc;
        }
        const hc_prep_record* rec = nullptr;
        rc = hc_prep_result_window(res.prep, w, &rec, nullptr, nullptr, nullptr, nullptr);
        if (rc) return rc;
        const std::vector<hc_asm_read>& v = views[size_t(w)];
        const std::vector<int32_t>& kept = res.reads[size_t(w)];
        reads.emplace_back(v.size());
        rb.emplace_back(v.size());
        re.emplace_back(v.size());
        for (size_t k = 0; k < v.size(); ++k) {
            reads.back()[k] = hc_phmm_read{v[k].length, reinterpret_cast<const char*>(v[k].bases),
                                           reinterpret_cast<const char*>(v[k].quals), gop, gop, gcp};
            rb.back()[k] = rec[kept[k]].begin;
            re.back()[k] = rec[kept[k]].end;
        }
        hc_region_in g{};
        g.ref = windows[w].ref;
        g.ref_len = windows[w].ref_len;
        g.padded_begin = windows[w].padded_begin;
        g.origin_begin = windows[w].origin_begin;
        g.origin_end = windows[w].origin_end;
        g.haps = haps.back().data();
        g.n_haps = n_haps;
        g.reads = reads.back().data();
        g.read_begin = rb.back().data();
        g.read_end = re.back().data();
        g.n_reads = int32_t(v.size());
        rin.push_back(g);
    }
    tr.mark("region_input");

    // ---- :103-104
    if (rin.empty()) return HC_PHMM_OK;   // nothing reaches the region caller: no sites
    t = clock::now();
    rc = hc_region_call(rin.data(), int32_t(rin.size()), flags, &res.calls);
    if (rc) return rc;
    tr.value("region_call", ms_since(t));

    // ---- the result's maps
    const hc_gt_call_site* sites = nullptr;
    int64_t n_sites = 0;
    rc = hc_region_calls_sites(res.calls, &sites, &n_sites);
    if (rc) return rc;
    res.sites.assign(sites, sites + n_sites);
    for (hc_gt_call_site& s : res.sites) s.region = call_window[size_t(s.region)];
    for (size_t c = 0; c < rin.size(); ++c) {
        const uint8_t* keep = nullptr;
        int32_t nr = 0, nk = 0;
        rc = hc_region_calls_reads(res.calls, int32_t(c), &keep, &nr, &nk);
        if (rc) return rc;
        std::vector<int32_t>& v = res.reads[size_t(call_window[c])];
        size_t m = 0;
        for (int32_t k = 0; k < nr; ++k)
            if (keep[k]) v[m++] = v[size_t(k)];
        v.resize(m);
    }
    tr.mark("result");
    tr.value("windows", double(n));
    tr.value("assembled", double(ar.size()));
    tr.value("called", double(rin.size()));
    tr.value("view_bytes", double(view_bytes));
    return HC_PHMM_OK;
}

int window_of(const hc_call_result* res, int32_t window)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (window < 0 || size_t(window) >= res->status.size()) return fail(HC_PHMM_EINVAL, "window index out of range");
    return HC_PHMM_OK;
}

}  // namespace

extern "C" int hc_call_windows(const hc_call_window* windows, int32_t n_windows, uint32_t flags, hc_call_result** out)
{
    std::lock_guard<std::mutex> lk(g_mu);
    return call_frame(out, nullptr, [&](hc_call_result& res) -> int {
        if (n_windows < 0 || (n_windows && !windows)) return fail(HC_PHMM_EINVAL, "null windows / negative count");
        if (flags & ~kKnownFlags) return fail(HC_PHMM_EINVAL, "unknown hc_call_windows flags");
        if (int rc = validate(windows, n_windows)) return rc;
        res.flags = flags;
        return run(windows, n_windows, flags, res);
    });
}

extern "C" int hc_call_result_window(const hc_call_result* res, int32_t window, int32_t* status, int32_t* asm_status,
                                     int32_t* kmer_size, int32_t* n_haps)
{
    int rc = window_of(res, window);
    if (rc) return rc;
    if (status) *status = res->status[size_t(window)];
    const int32_t a = res->asm_index[size_t(window)];
    if (a < 0) {
        if (asm_status) *asm_status = HC_ASM_NO_HAPLOTYPES;
        if (kmer_size) *kmer_size = 0;
        if (n_haps) *n_haps = 0;
        return HC_PHMM_OK;
    }
    return hc_asm_result_region(res->assembled, a, asm_status, kmer_size, nullptr, n_haps, nullptr);
}

extern "C" int hc_call_result_prep(const hc_call_result* res, int32_t window, const hc_prep_record** records,
                                   int32_t* n_reads, const int32_t** kept, int32_t* n_kept, int64_t* kept_bases)
{
    const int rc = window_of(res, window);
    if (rc) return rc;
    return hc_prep_result_window(res->prep, window, records, n_reads, kept, n_kept, kept_bases);
}

extern "C" int hc_call_result_hap(const hc_call_result* res, int32_t window, int32_t hap, const uint8_t** bases,
                                  int32_t* length, double* score, int32_t* begin, const char** cigar)
{
    int rc = window_of(res, window);
    if (rc) return rc;
    if ((begin || cigar) && !(res->flags & HC_CALL_WANT_CIGARS))
        return fail(HC_PHMM_EINVAL, "hc_call_windows ran without HC_CALL_WANT_CIGARS");
    const int32_t a = res->asm_index[size_t(window)];
    if (a < 0) return fail(HC_PHMM_EINVAL, "haplotype index out of range");
    rc = hc_asm_result_hap(res->assembled, a, hap, bases, length, score);
    if (rc) return rc;
    if (begin) *begin = -1;
    if (cigar) *cigar = nullptr;
    const int32_t c = res->call_index[size_t(window)];
    if ((begin || cigar) && c >= 0) {
        int32_t b = -1;
        const char* text = nullptr;
        rc = hc_region_calls_alignment(res->calls, c, hap, &b, &text);
        if (rc) return rc;
        if (begin) *begin = b;
        if (cigar) *cigar = text;
    }
    return HC_PHMM_OK;
}

extern "C" int hc_call_result_sites(const hc_call_result* res, const hc_gt_call_site** sites, int64_t* n)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (sites) *sites = res->sites.data();
    if (n) *n = int64_t(res->sites.size());
    return HC_PHMM_OK;
}

extern "C" int hc_call_result_reads(const hc_call_result* res, int32_t window, const int32_t** reads, int32_t* n)
{
    const int rc = window_of(res, window);
    if (rc) return rc;
    if (reads) *reads = res->reads[size_t(window)].data();
    if (n) *n = int32_t(res->reads[size_t(window)].size());
    return HC_PHMM_OK;
}

extern "C" int hc_call_result_matrix(const hc_call_result* res, int32_t window, const double** L, int32_t* n_reads,
                                     int32_t* n_haps)
{
    int rc = window_of(res, window);
    if (rc) return rc;
    if (!(res->flags & HC_CALL_WANT_L)) return fail(HC_PHMM_EINVAL, "hc_call_windows ran without HC_CALL_WANT_L");
    const int32_t c = res->call_index[size_t(window)];
    if (c >= 0) {
        const double* p = nullptr;
        int32_t nr = 0, nh = 0;
        rc = hc_region_calls_matrix(res->calls, c, &p, &nr, &nh);
        if (rc) return rc;
        if (L) *L = p;
        if (n_reads) *n_reads = nr;
        if (n_haps) *n_haps = nh;
        return HC_PHMM_OK;
    }
    if (L) *L = nullptr;
    if (n_reads) *n_reads = 0;
    return hc_call_result_window(res, window, nullptr, nullptr, nullptr, n_haps);
}

extern "C" int hc_call_result_free(hc_call_result* res)
{
    delete res;
    return HC_PHMM_OK;
}
