// Host engine + C ABI of the read preparation (include/hc_prep.h).
//
// One call = filter_reads and hard_clip_reads for any number of windows:
//
//   validate, lay out (the caller's records packed on the worker pool)
//   one upload of [window records | read records | CIGAR words]
//   prep_kernel (one wave per window) on the preparation's stream
//   one readback of [error word | per-window totals | records | kept indices]
//
// The workspace is the engine's own: four grow-only buffers of the shared host
// layer (stage_host.hpp), released by hc_phmm_shutdown. A HIP error drains the
// stream before it returns. Calls serialise under the preparation's own lock
// and use the engine's primary device. HC_PREP_TRACE=1 prints the host wall
// clock of the phases and the bytes moved on stderr.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_prep.h"
#include "pool.hpp"
#include "prep_kernels.hpp"
#include "stage_host.hpp"

using namespace hcprep;
using namespace stage_host;

struct hc_prep_result {
    std::vector<int64_t> first;   // n_windows + 1: a window's first read in the pools below
    std::vector<hc_prep_record> records;
    std::vector<int32_t> kept;    // per window at first[w]: n_kept[w] indices, the rest 0
    std::vector<int32_t> n_kept;
    std::vector<int64_t> kept_bases;
};

namespace {

Buf g_in, g_out, g_hin{nullptr, 0, true}, g_hback{nullptr, 0, true};
Stage g_st({&g_in, &g_out, &g_hin, &g_hback});

// The HC_PHMM_EINVAL cases, before any device work. Totals the reads, and the
// CIGAR words in front of every window (word_first, n + 1 entries).
int validate(const hc_prep_window* windows, int32_t n, int64_t& n_reads, std::vector<int64_t>& word_first)
{
    n_reads = 0;
    int64_t n_words = 0;
    word_first.assign(size_t(n) + 1, 0);
    for (int32_t w = 0; w < n; ++w) {
        const hc_prep_window& g = windows[w];
        auto at = [&] { return "window " + std::to_string(w); };
        if (g.padded_begin < 0) return fail(HC_PHMM_EINVAL, at() + ": negative padded_begin");
        if (g.padded_end < g.padded_begin) return fail(HC_PHMM_EINVAL, at() + ": padded_end before padded_begin");
        if (g.n_reads < 0) return fail(HC_PHMM_EINVAL, at() + ": negative read count");
        if (g.n_reads && !g.reads) return fail(HC_PHMM_EINVAL, at() + ": null reads");
        for (int32_t j = 0; j < g.n_reads; ++j) {
            const hc_prep_read& rd = g.reads[j];
            auto rat = [&] { return at() + " read " + std::to_string(j); };
            if (rd.seq_len < 0 || rd.seq_len > HC_PHMM_MAX_READ_LEN)
                return fail(HC_PHMM_EINVAL, rat() + ": seq_len outside 0 .. " + std::to_string(HC_PHMM_MAX_READ_LEN));
            if (rd.n_cigar < 0) return fail(HC_PHMM_EINVAL, rat() + ": negative n_cigar");
            if (rd.n_cigar && !rd.cigar) return fail(HC_PHMM_EINVAL, rat() + ": null cigar");
            n_words += rd.n_cigar;
        }
        n_reads += g.n_reads;
        word_first[size_t(w) + 1] = n_words;
    }
    return HC_PHMM_OK;
}

const char* error_text(int64_t code)
{
    switch (code) {
        case kErrPosZero: return "pos == 0";
        case kErrNoCigar: return "n_cigar == 0";
        case kErrOp: return "a CIGAR op code above 8";
        case kErrLength: return "the CIGAR's read length differs from seq_len";
        default: return "unknown device error";
    }
}

int run(const hc_prep_window* windows, int32_t n, int64_t n_reads, const std::vector<int64_t>& word_first,
        hc_prep_result& res)
{
    const int64_t n_words = word_first[size_t(n)];
    Trace tr("HC_PREP_TRACE", "[hc_prep]");
    // ---- layout
    res.first.assign(size_t(n) + 1, 0);
    for (int32_t w = 0; w < n; ++w) res.first[size_t(w) + 1] = res.first[size_t(w)] + windows[w].n_reads;

    Carver in;
    const size_t o_win = in.take(sizeof(PrepWindow) * size_t(n));
    const size_t o_rd = in.take(sizeof(PrepRead) * size_t(n_reads));
    const size_t o_words = in.take(sizeof(uint32_t) * size_t(n_words));
    const size_t in_bytes = in.off;
    Carver oc;
    const size_t o_err = oc.take(sizeof(unsigned long long));
    const size_t o_nk = oc.take(sizeof(int32_t) * size_t(n));
    const size_t o_kb = oc.take(sizeof(int64_t) * size_t(n));
    const size_t o_rec = oc.take(sizeof(hc_prep_record) * size_t(n_reads));
    const size_t o_kept = oc.take(sizeof(int32_t) * size_t(n_reads));
    const size_t out_bytes = oc.off;
    int rc = reserve(g_hin, in_bytes, "read preparation staging");
    if (rc) return rc;
    rc = reserve(g_in, in_bytes, "read preparation input");
    if (rc) return rc;
    rc = reserve(g_out, out_bytes, "read preparation output");
    if (rc) return rc;
    rc = reserve(g_hback, out_bytes, "read preparation readback");
    if (rc) return rc;

    char* h = g_hin.p;
    PrepWindow* hw = reinterpret_cast<PrepWindow*>(h + o_win);
    PrepRead* hr = reinterpret_cast<PrepRead*>(h + o_rd);
    uint32_t* hc = reinterpret_cast<uint32_t*>(h + o_words);
    hcphmm::parallel_for(
        n,
        [&](int64_t lo, int64_t hi) {
            for (int64_t w = lo; w < hi; ++w) {
                const hc_prep_window& g = windows[w];
                hw[w] = PrepWindow{g.padded_begin, g.padded_end, res.first[size_t(w)], g.n_reads, 0};
                PrepRead* d = hr + res.first[size_t(w)];
                int64_t word = word_first[size_t(w)];
                for (int32_t j = 0; j < g.n_reads; ++j) {
                    const hc_prep_read& rd = g.reads[j];
                    d[j] = PrepRead{word, rd.pos, rd.seq_len, rd.n_cigar, rd.flag, rd.mapq, rd.mate_same_contig ? 1u : 0u, 0u};
                    if (rd.n_cigar) std::memcpy(hc + word, rd.cigar, sizeof(uint32_t) * size_t(rd.n_cigar));
                    word += rd.n_cigar;
                }
            }
        },
        8);
    tr.mark("layout");

    PrepArgs a{};
    a.windows = reinterpret_cast<const PrepWindow*>(g_in.p + o_win);
    a.n_windows = n;
    a.reads = reinterpret_cast<const PrepRead*>(g_in.p + o_rd);
    a.words = reinterpret_cast<const uint32_t*>(g_in.p + o_words);
    a.err = reinterpret_cast<unsigned long long*>(g_out.p + o_err);
    a.n_kept = reinterpret_cast<int32_t*>(g_out.p + o_nk);
    a.kept_bases = reinterpret_cast<int64_t*>(g_out.p + o_kb);
    a.records = reinterpret_cast<hc_prep_record*>(g_out.p + o_rec);
    a.kept = reinterpret_cast<int32_t*>(g_out.p + o_kept);

    HIP_TRY(g_st.stream, hipMemcpyAsync(g_in.p, h, in_bytes, hipMemcpyHostToDevice, g_st.stream));
    HIP_TRY(g_st.stream, hipMemsetAsync(g_out.p + o_err, 0xFF, sizeof(unsigned long long), g_st.stream));
    if (tr.on) {
        HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
        tr.mark("upload");
    }
    HIP_TRY(g_st.stream, launch_prep(a, g_st.stream));
    if (tr.on) {
        HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
        tr.mark("kernel");
    }
    char* hb = g_hback.p;
    HIP_TRY(g_st.stream, hipMemcpyAsync(hb, g_out.p, out_bytes, hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
    tr.mark("readback");

    unsigned long long err = 0;
    std::memcpy(&err, hb + o_err, sizeof(err));
    if (err != kNoError) {
        const int64_t g = int64_t(err >> 3);
        if (g >= n_reads) return fail(HC_PHMM_EHIP, "read preparation: error word out of its bound");
        const int64_t w = (std::upper_bound(res.first.begin(), res.first.end(), g) - res.first.begin()) - 1;
        return fail(HC_PHMM_EINVAL, "window " + std::to_string(w) + " read " + std::to_string(g - res.first[size_t(w)]) +
                                        ": " + error_text(int64_t(err & 7ull)));
    }
    res.n_kept.resize(size_t(n));
    res.kept_bases.resize(size_t(n));
    res.records.resize(size_t(n_reads));
    res.kept.assign(size_t(n_reads), 0);
    if (n) std::memcpy(res.n_kept.data(), hb + o_nk, sizeof(int32_t) * size_t(n));
    if (n) std::memcpy(res.kept_bases.data(), hb + o_kb, sizeof(int64_t) * size_t(n));
    if (n_reads) std::memcpy(res.records.data(), hb + o_rec, sizeof(hc_prep_record) * size_t(n_reads));
    const int32_t* hk = reinterpret_cast<const int32_t*>(hb + o_kept);
    for (int32_t w = 0; w < n; ++w) {
        const int32_t nk = res.n_kept[size_t(w)];
        if (nk < 0 || nk > windows[w].n_reads) return fail(HC_PHMM_EHIP, "read preparation: a window's kept count is out of its bound");
        if (nk) std::memcpy(res.kept.data() + res.first[size_t(w)], hk + res.first[size_t(w)], sizeof(int32_t) * size_t(nk));
    }
    tr.mark("records");
    tr.value("upload_bytes", double(in_bytes));
    tr.value("readback_bytes", double(out_bytes));
    return HC_PHMM_OK;
}

}  // namespace

extern "C" int hc_prep_reads(const hc_prep_window* windows, int32_t n_windows, hc_prep_result** out)
{
    std::lock_guard<std::mutex> lk(g_st.mu);
    return call_frame(out, &g_st.stream, [&](hc_prep_result& res) -> int {
        if (n_windows < 0 || (n_windows && !windows)) return fail(HC_PHMM_EINVAL, "null windows / negative count");
        int64_t n_reads = 0;
        std::vector<int64_t> word_first;
        if (int rc = validate(windows, n_windows, n_reads, word_first)) return rc;
        res.first.assign(1, 0);
        if (!n_windows) return HC_PHMM_OK;
        if (int rc = g_st.ensure_init()) return rc;
        return run(windows, n_windows, n_reads, word_first, res);
    });
}

extern "C" int hc_prep_result_window(const hc_prep_result* res, int32_t window, const hc_prep_record** records,
                                     int32_t* n_reads, const int32_t** kept, int32_t* n_kept, int64_t* kept_bases)
{
    if (!res) return fail(HC_PHMM_EINVAL, "null result");
    if (window < 0 || size_t(window) + 1 >= res->first.size()) return fail(HC_PHMM_EINVAL, "window index out of range");
    const size_t w = size_t(window);
    const int64_t at = res->first[w];
    if (records) *records = res->records.data() + at;
    if (n_reads) *n_reads = int32_t(res->first[w + 1] - at);
    if (kept) *kept = res->kept.data() + at;
    if (n_kept) *n_kept = res->n_kept[w];
    if (kept_bases) *kept_bases = res->kept_bases[w];
    return HC_PHMM_OK;
}

extern "C" int hc_prep_result_free(hc_prep_result* res)
{
    delete res;
    return HC_PHMM_OK;
}
