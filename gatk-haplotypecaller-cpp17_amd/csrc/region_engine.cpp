// Host engine + C ABI of the region caller (include/hc_region.h).
//
// One call = align, PairHMM, filter and genotype of any number of regions:
//
//   validate, lay out, reserve
//   on the genotyper's stream: one upload of windows, haplotype bases and
//     descriptors; sw_dp_kernel + sw_trace_kernel on those buffers;
//     region_runs_kernel (or the host-parsed runs of haplotypes that brought a
//     CIGAR); gt_plan_events_kernel + scan; the counted readback of the totals
//   submit the PairHMM job while the device works through that; its out pointers
//     are the pinned block the matrices are uploaded from, so collect writes the
//     log10 values where the H2D reads
//   collect; upload matrices, read lengths and intervals; region_finish_*;
//     gt_plan_site_kernel; gt_sites_kernel
//   one readback: records, likelihoods, maps, keep bytes and counts, and only
//     on request the per-site read lists, the matrices and the CIGAR elements
//
// The workspace is the call's own: four grow-only buffers of the shared host
// layer (stage_host.hpp), registered with the genotyper's stage and released
// with it. Stream, lock and Jacobian table are the genotyper's, so the call serialises
// with hc_gt_* as those do among themselves; the frame of a region and the
// PlanArgs / GtArgs helpers are the genotyper's too (gt_engine_internal.hpp).
// Inside a call HIP_BAIL wraps the shared HIP error text: collect the PairHMM
// job, drain the stream, restore the message.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_region.h"
#include "gt_engine_internal.hpp"
#include "pool.hpp"
#include "region_kernels.hpp"
#include "stage_host.hpp"
#include "sw_engine_internal.hpp"

namespace hcphmm {
int submit_regions_with_mode(const hc_phmm_region* regions, int32_t n_regions, uint32_t mode, hc_phmm_job** job);
uint32_t default_mode();
}

using namespace hcgt;
using namespace hcregion;
using namespace stage_host;

namespace {

// Grow-only buffers, guarded by the genotyper's lock and dropped with its stage.
Buf g_dev1, g_dev2, g_hin{nullptr, 0, true}, g_hback{nullptr, 0, true};
Stage& g_st = hcgt_host::stage().with({&g_dev1, &g_dev2, &g_hin, &g_hback});

// The aligner as hc::MI355XSWAligner::align_haplotypes runs it.
constexpr hc_sw_params kSwParams{200, -150, -260, -11};   // NEW_SW_PARAMETERS
constexpr int kSwOverhang = HC_SW_SOFTCLIP;
constexpr int kSwShortcut = 1;

// Layout of the block regions_finish_* work on, used by the call and by hcx_region_finish.
struct FinishLayout {
    size_t o_len, o_rb, o_re, o_L, in_end;   // uploaded
    size_t o_Lout, o_rbo, o_reo, o_dest, end;
    FinishLayout(Carver& c, int64_t reads, int64_t L_total)
    {
        o_len = c.take(sizeof(int32_t) * size_t(reads));
        o_rb = c.take(sizeof(int64_t) * size_t(reads));
        o_re = c.take(sizeof(int64_t) * size_t(reads));
        o_L = c.take(sizeof(double) * size_t(L_total));
        in_end = c.off;
        o_Lout = c.take(sizeof(double) * size_t(L_total));
        o_rbo = c.take(sizeof(int64_t) * size_t(reads));
        o_reo = c.take(sizeof(int64_t) * size_t(reads));
        o_dest = c.take(sizeof(int32_t) * size_t(reads));
        end = c.off;
    }
};

}  // namespace

struct hc_region_calls {
    hcgt_host::Calls c;
    uint32_t flags = 0;
    int32_t n = 0;
    std::vector<int32_t> read_off, n_reads, n_kept, n_haps, hap0;
    std::vector<int64_t> L_off;
    std::vector<uint8_t> keep;         // per read of the call
    std::vector<double> L;             // kept rows, compact per region at L_off
    std::vector<uint8_t> aligned;      // per region: its haplotypes were aligned on the device
    std::vector<int32_t> begins;       // per haplotype of the call
    std::vector<std::string> cigars;
};

namespace {

int run(const hc_region_in* regions, int32_t n, uint32_t flags, hc_region_calls& out)
{
    const hipStream_t st = g_st.stream;
    Trace trace("HC_REGION_TRACE", "[hc_region]");
    // ---- validate and lay out
    std::vector<PlanRegion> pr(static_cast<size_t>(n));
    std::vector<PlanHap> ph;
    std::vector<PlanRun> host_runs;
    std::vector<hcsw::SwPair> pairs;
    std::vector<int32_t> pair_hap;
    std::vector<hc_phmm_hap> hh;
    std::vector<hc_phmm_region> hr(static_cast<size_t>(n));
    std::string hap_pool;
    out.aligned.assign(size_t(n), 0);
    hcgt_host::FrameTotals t;
    for (int32_t r = 0; r < n; ++r) {
        const hc_region_in& x = regions[r];
        const hcgt_host::RegionFrame f{!x.ref || !x.haps || (x.n_reads > 0 && (!x.read_begin || !x.read_end || !x.reads)),
                                       x.ref_len, x.n_haps, x.n_reads, x.padded_begin, x.origin_begin, x.origin_end};
        PlanRegion& d = pr[size_t(r)];
        auto haps = [&](const std::string& at) {
            int with = 0;
            for (int32_t h = 0; h < x.n_haps; ++h) with += x.haps[h].cigar != nullptr;
            if (with != 0 && with != x.n_haps)
                return fail(HC_PHMM_EINVAL, at + ": haplotypes with and without a CIGAR (all or none)");
            out.aligned[size_t(r)] = with == 0;
            for (int32_t h = 0; h < x.n_haps; ++h) {
                const hc_region_hap& y = x.haps[h];
                const std::string hat = at + " haplotype " + std::to_string(h);
                if (int rc = hcgt_host::check_hap_frame(hat, !y.bases, y.length, y.cigar ? y.alignment_begin : 0, x.ref_len))
                    return rc;
                PlanHap e;
                e.region = r;
                e.base_off = int32_t(hap_pool.size());
                e.tab_off = int32_t(t.tab + int64_t(h) * x.ref_len);
                e.run_off = 0;   // device-aligned: written by region_runs_kernel
                e.n_runs = 0;
                if (y.cigar) {
                    e.run_off = int32_t(host_runs.size());   // rebased behind the device runs below
                    if (int rc = hcgt_host::parse_hap_cigar(hat, y.cigar, y.alignment_begin, y.length, x.ref_len, host_runs))
                        return rc;
                    e.n_runs = int32_t(host_runs.size()) - e.run_off;
                } else {
                    hcsw::SwPair P{};
                    P.ref_off = d.ref_off;
                    P.alt_off = e.base_off;
                    P.n1 = x.ref_len;
                    P.n2 = y.length;
                    pairs.push_back(P);
                    pair_hap.push_back(int32_t(ph.size()));
                }
                hap_pool.append(reinterpret_cast<const char*>(y.bases), size_t(y.length));
                hh.push_back(hc_phmm_hap{y.length, reinterpret_cast<const char*>(y.bases)});
                ph.push_back(e);
            }
            return HC_PHMM_OK;
        };
        if (int rc = hcgt_host::add_region(r, f, t, d, haps, ph, hap_pool, host_runs)) return rc;
    }
    const int64_t read_total = t.reads, L_total = t.L;
    const size_t nh = ph.size(), np = pairs.size();
    const hcsw_host::PairLayout lay = hcsw_host::layout_pairs(pairs);
    // Run buffer: the aligner's own bound of n1 + n2 + 3 elements per pair, at the
    // pair's element offset, then the host-parsed runs. No readback sizes it.
    const int64_t run_total = lay.el_total + int64_t(host_runs.size());
    if (run_total > INT32_MAX) return fail(HC_PHMM_EINVAL, "too many regions for one call");
    for (PlanHap& e : ph)
        if (!out.aligned[size_t(e.region)]) e.run_off += int32_t(lay.el_total);

    // Workspace 1, part A (no likelihood needed):
    //   uploaded [regions | haps | pairs | order | pair_hap | ref | hap | host runs]
    //   device   [res | bt | elems | slots | n_elems | offsets | runs | bitmap | base | totals + err | ev | span]
    Carver cv;
    hcgt_host::PlanOffsets o{};
    o.reg = cv.take(sizeof(PlanRegion) * size_t(n));
    o.hap = cv.take(sizeof(PlanHap) * nh);
    const size_t o_pairs = cv.take(sizeof(hcsw::SwPair) * np);
    const size_t o_order = cv.take(sizeof(int32_t) * np);
    const size_t o_phap = cv.take(sizeof(int32_t) * np);
    o.ref = cv.take(size_t(t.ref));
    o.pool = cv.take(hap_pool.size());
    const size_t o_hruns = cv.take(sizeof(PlanRun) * host_runs.size());
    const size_t a_in = cv.off;
    const size_t o_res = cv.take(sizeof(hcsw::SwResult) * np);
    const size_t o_bt = cv.take(sizeof(uint32_t) * size_t(lay.bt_total));
    const size_t o_el = cv.take(sizeof(uint32_t) * size_t(lay.el_total));
    const size_t o_slots = cv.take(sizeof(uint16_t) * hcsw::kSlotElems * np);
    const size_t o_nel = cv.take(sizeof(int32_t) * np);
    const size_t o_offs = cv.take(sizeof(int32_t) * np);
    const size_t sw_tail = cv.off - o_slots;   // [slots | n_elems | offsets]
    o.runs = cv.take(sizeof(PlanRun) * size_t(run_total));
    o.bitmap = cv.take(sizeof(uint32_t) * kBitmapWords * size_t(n));
    o.base = cv.take(sizeof(PlanBase) * size_t(n));
    o.totals = cv.take(sizeof(PlanTotals) + sizeof(uint32_t));   // the error word sits behind the totals
    const size_t o_err = o.totals + sizeof(PlanTotals);
    o.ev = cv.take(sizeof(int16_t) * size_t(t.tab));
    o.span = cv.take(sizeof(int16_t) * size_t(t.tab));
    // part B (after the PairHMM): pinned image = device image shifted by b0
    const size_t b0 = cv.off;
    const FinishLayout fl(cv, read_total, L_total);
    o.read_begin = fl.o_rbo;   // the compacted intervals
    o.read_end = fl.o_reo;
    const size_t dev1_bytes = cv.off;
    const size_t b_in = fl.in_end - b0;
    // Pinned input block: [part A inputs | part B inputs | totals + err | aligner tail]
    const size_t h_b = a_in;
    const size_t h_tot = up(h_b + b_in);
    const size_t h_tail = up(h_tot + sizeof(PlanTotals) + sizeof(uint32_t));
    const bool want_cigars = (flags & HC_REGION_WANT_CIGARS) && np > 0;
    int rc = reserve(g_dev1, dev1_bytes, "region caller device workspace");
    if (rc) return rc;
    rc = reserve(g_hin, h_tail + (want_cigars ? sw_tail : 0), "region caller pinned workspace");
    if (rc) return rc;
    char* const h = g_hin.p;
    char* const dv = g_dev1.p;
    trace.mark("laid_out");

    // From here on every exit collects the job (once there is one) and drains the
    // stream, so the three engines and this workspace are reusable whatever happened.
    hc_phmm_job* job = nullptr;
    auto bail = [&](int code) {
        const std::string msg = hc_phmm_last_error();
        if (job) (void)hc_phmm_collect(job);
        job = nullptr;
        (void)hipStreamSynchronize(st);
        hcphmm::set_last_error(msg);
        return code;
    };
    // (hip_fail with no stream only sets the message: bail collects, then drains, then restores it)
#define HIP_BAIL(expr)                                                              \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess) return bail(hip_fail(nullptr, #expr, e_));            \
    } while (0)

    // ---- part A, enqueued ahead of the PairHMM job: the device works through it
    // while the host plans and packs that job (a quarter of the call), and the
    // PairHMM kernels then find the device free
    std::memcpy(h + o.reg, pr.data(), sizeof(PlanRegion) * size_t(n));
    std::memcpy(h + o.hap, ph.data(), sizeof(PlanHap) * nh);
    if (np) {
        std::memcpy(h + o_pairs, pairs.data(), sizeof(hcsw::SwPair) * np);
        std::memcpy(h + o_order, lay.order.data(), sizeof(int32_t) * np);
        std::memcpy(h + o_phap, pair_hap.data(), sizeof(int32_t) * np);
    }
    std::memcpy(h + o.pool, hap_pool.data(), hap_pool.size());
    if (!host_runs.empty()) std::memcpy(h + o_hruns, host_runs.data(), sizeof(PlanRun) * host_runs.size());
    for (int32_t r = 0; r < n; ++r)
        std::memcpy(h + o.ref + size_t(pr[size_t(r)].ref_off), regions[r].ref, size_t(regions[r].ref_len));
    HIP_BAIL(hipMemcpyAsync(dv, h, a_in, hipMemcpyHostToDevice, st));
    PlanRun* const d_runs = reinterpret_cast<PlanRun*>(dv + o.runs);
    if (!host_runs.empty())
        HIP_BAIL(hipMemcpyAsync(d_runs + lay.el_total, dv + o_hruns, sizeof(PlanRun) * host_runs.size(),
                                hipMemcpyDeviceToDevice, st));
    HIP_BAIL(hipMemsetAsync(dv + o_err, 0, sizeof(uint32_t), st));
    if (np) {
        hcsw_host::DeviceBatch b;
        b.n = int64_t(np);
        b.pairs = reinterpret_cast<const hcsw::SwPair*>(dv + o_pairs);
        b.order = reinterpret_cast<const int32_t*>(dv + o_order);
        b.refs = reinterpret_cast<const uint8_t*>(dv + o.ref);
        b.alts = reinterpret_cast<const uint8_t*>(dv + o.pool);
        b.res = reinterpret_cast<hcsw::SwResult*>(dv + o_res);
        b.bt = reinterpret_cast<uint32_t*>(dv + o_bt);
        b.elems = reinterpret_cast<uint32_t*>(dv + o_el);
        b.slots = reinterpret_cast<uint16_t*>(dv + o_slots);
        b.n_elems = reinterpret_cast<int32_t*>(dv + o_nel);
        b.offsets = reinterpret_cast<int32_t*>(dv + o_offs);
        b.params = kSwParams;
        b.overhang = kSwOverhang;
        b.shortcut = kSwShortcut;
        b.n1max = lay.n1max;
        b.n2max = lay.n2max;
        b.fast = hcsw_host::dp_variant(kSwParams, kSwOverhang, lay.n1max, lay.n2max);
        HIP_BAIL(hcsw_host::launch_batch(b, st, nullptr));
        RunsArgs ra{};
        ra.pairs = b.pairs;
        ra.pair_hap = reinterpret_cast<const int32_t*>(dv + o_phap);
        ra.res = b.res;
        ra.elems = b.elems;
        ra.slots = b.slots;
        ra.n_elems = b.n_elems;
        ra.offsets = b.offsets;
        ra.n = int(np);
        ra.runs = d_runs;
        ra.haps = reinterpret_cast<PlanHap*>(dv + o.hap);
        ra.err = reinterpret_cast<uint32_t*>(dv + o_err);
        HIP_BAIL(launch_runs(ra, st));
    }
    PlanArgs p = hcgt_host::plan_args(dv, o, n, nh);
    HIP_BAIL(launch_plan_events(p, st));
    HIP_BAIL(hipMemcpyAsync(h + h_tot, dv + o.totals, sizeof(PlanTotals) + sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (want_cigars) HIP_BAIL(hipMemcpyAsync(h + h_tail, dv + o_slots, sw_tail, hipMemcpyDeviceToHost, st));
    // A query makes the runtime hand the queued work to the device now, not at the next wait.
    (void)hipStreamQuery(st);
    trace.mark("part_a_enqueued");

    // ---- the PairHMM job, written straight into the matrix upload
    double* const hL = reinterpret_cast<double*>(h + h_b + (fl.o_L - b0));
    for (int32_t r = 0; r < n; ++r) {
        const hc_region_in& x = regions[r];
        hr[size_t(r)] = hc_phmm_region{x.reads, x.n_reads, hh.data() + pr[size_t(r)].hap0, x.n_haps,
                                       hL + pr[size_t(r)].L_off};
    }
    const uint32_t mode = (flags & HC_REGION_DEFAULT_MODE) ? hcphmm::default_mode() : (flags & HC_REGION_F64);
    rc = hcphmm::submit_regions_with_mode(hr.data(), n, mode, &job);
    if (rc) return bail(rc);
    trace.mark("submitted");
    if (trace.on) trace.mark(hipStreamQuery(st) == hipSuccess ? "part_a_done_by_then" : "part_a_still_running");
    // Read lengths and intervals are staged while that runs.
    int32_t* const hlen = reinterpret_cast<int32_t*>(h + h_b + (fl.o_len - b0));
    int64_t* const hrb = reinterpret_cast<int64_t*>(h + h_b + (fl.o_rb - b0));
    int64_t* const hre = reinterpret_cast<int64_t*>(h + h_b + (fl.o_re - b0));
    for (int32_t r = 0; r < n; ++r) {
        const hc_region_in& x = regions[r];
        const size_t at = size_t(pr[size_t(r)].read_off);
        for (int32_t i = 0; i < x.n_reads; ++i) hlen[at + size_t(i)] = x.reads[i].length;
        if (x.n_reads) {
            std::memcpy(hrb + at, x.read_begin, sizeof(int64_t) * size_t(x.n_reads));
            std::memcpy(hre + at, x.read_end, sizeof(int64_t) * size_t(x.n_reads));
        }
    }
    // The one counted readback: the site count sizes everything that follows.
    HIP_BAIL(hipStreamSynchronize(st));
    trace.mark("totals");
    PlanTotals tot;
    uint32_t err = 0;
    std::memcpy(&tot, h + h_tot, sizeof(tot));
    std::memcpy(&err, h + h_tot + sizeof(PlanTotals), sizeof(err));
    if (err)
        return bail(fail(HC_PHMM_EHIP, "region caller: the aligner's CIGAR elements do not form valid runs (error word " +
                                           std::to_string(err) + ")"));
    const int64_t ns = tot.n_sites;
    if (ns < 0 || ns > t.site_bound || tot.keep_cap > t.keep_bound || tot.map_cap > t.map_bound)
        return bail(fail(HC_PHMM_EHIP, "genotyper site count out of its bound"));
    // CIGAR text of the device-aligned haplotypes, "%d%c" as hc_sw_align_flat prints it.
    if (flags & HC_REGION_WANT_CIGARS) {
        out.begins.assign(nh, 0);
        out.cigars.assign(nh, std::string());
        const uint16_t* slotv = reinterpret_cast<const uint16_t*>(h + h_tail);
        const int32_t* cntv = reinterpret_cast<const int32_t*>(h + h_tail + (o_nel - o_slots));
        const int32_t* offv = reinterpret_cast<const int32_t*>(h + h_tail + (o_offs - o_slots));
        std::vector<uint32_t> big;
        for (size_t k = 0; k < np; ++k) {
            const int cnt = cntv[k];
            const bool in_slots = cnt <= hcsw::kSlotElems;
            if (!in_slots) {   // rare: the pair's whole scratch
                big.resize(size_t(cnt));
                HIP_BAIL(hipMemcpy(big.data(), reinterpret_cast<const uint32_t*>(dv + o_el) + pairs[k].el_off,
                                   sizeof(uint32_t) * size_t(cnt), hipMemcpyDeviceToHost));
            }
            std::string& text = out.cigars[size_t(pair_hap[k])];
            char tmp[24];
            for (int e = cnt - 1; e >= 0; --e) {
                const uint32_t v = in_slots ? uint32_t(slotv[k * hcsw::kSlotElems + size_t(e)]) : big[size_t(e)];
                const int op = int(v & 15);
                const char ch = op == hcsw::kOpM ? 'M' : op == hcsw::kOpI ? 'I' : op == hcsw::kOpD ? 'D'
                                : op == hcsw::kOpS ? 'S' : 'R';
                std::snprintf(tmp, sizeof(tmp), "%u%c", v >> 4, ch);
                text += tmp;
            }
            out.begins[size_t(pair_hap[k])] = offv[k];
        }
    }

    // ---- collect: the log10 values are now in the pinned block
    rc = hc_phmm_collect(job);
    job = nullptr;
    if (rc) return bail(rc);
    trace.mark("collected");

    // ---- part B
    // Workspace 2: [site_out | gl | gi | gq | amap | keep bytes | kept counts | site read lists] read back
    // (the lists only on request), then [gt_sites | al] scratch.
    const bool want_lists = (flags & HC_REGION_WANT_SITE_READS) != 0;
    Carver c2;
    const size_t o_so = c2.take(sizeof(SiteOut) * size_t(ns));
    const size_t o_gl = c2.take(sizeof(double) * kMaxGenotypes * size_t(ns));
    const size_t o_gi = c2.take(sizeof(int32_t) * size_t(ns));
    const size_t o_gq = c2.take(sizeof(int32_t) * size_t(ns));
    const size_t o_map = c2.take(sizeof(int32_t) * size_t(tot.map_cap));
    const size_t o_keepb = c2.take(size_t(read_total));
    const size_t o_nk = c2.take(sizeof(int32_t) * size_t(n));
    const size_t back_short = c2.off;
    const size_t o_keep = c2.take(sizeof(int32_t) * size_t(tot.keep_cap));
    const size_t back = want_lists ? c2.off : back_short;
    const size_t o_gs = c2.take(sizeof(GtSite) * size_t(ns));
    const size_t o_al = c2.take(sizeof(double) * kMaxAlleles * size_t(std::max<int64_t>(tot.keep_cap, 1)));
    const bool want_L = (flags & HC_REGION_WANT_L) != 0;
    const size_t h_L = up(back);
    rc = reserve(g_dev2, c2.off, "region caller site workspace");
    if (rc) return bail(rc);
    rc = reserve(g_hback, h_L + (want_L ? sizeof(double) * size_t(L_total) : 0), "region caller pinned readback");
    if (rc) return bail(rc);
    char* const d2 = g_dev2.p;
    char* const hb = g_hback.p;
    if (b_in) HIP_BAIL(hipMemcpyAsync(dv + b0, h + h_b, b_in, hipMemcpyHostToDevice, st));
    FinishArgs fa{};
    fa.regions = reinterpret_cast<PlanRegion*>(dv + o.reg);
    fa.n_regions = n;
    fa.n_reads = int(read_total);
    fa.read_len = reinterpret_cast<const int32_t*>(dv + fl.o_len);
    fa.L = reinterpret_cast<double*>(dv + fl.o_L);
    fa.read_begin = reinterpret_cast<const int64_t*>(dv + fl.o_rb);
    fa.read_end = reinterpret_cast<const int64_t*>(dv + fl.o_re);
    fa.L_out = reinterpret_cast<double*>(dv + fl.o_Lout);
    fa.begin_out = reinterpret_cast<int64_t*>(dv + fl.o_rbo);
    fa.end_out = reinterpret_cast<int64_t*>(dv + fl.o_reo);
    fa.keep = reinterpret_cast<uint8_t*>(d2 + o_keepb);
    fa.dest = reinterpret_cast<int32_t*>(dv + fl.o_dest);
    fa.n_kept = reinterpret_cast<int32_t*>(d2 + o_nk);
    HIP_BAIL(launch_finish(fa, st));
    if (ns > 0) {
        p.site_out = reinterpret_cast<SiteOut*>(d2 + o_so);
        p.gt_sites = reinterpret_cast<GtSite*>(d2 + o_gs);
        p.keep = reinterpret_cast<int32_t*>(d2 + o_keep);
        p.amap = reinterpret_cast<int32_t*>(d2 + o_map);
        HIP_BAIL(launch_plan_sites(p, ns, st));
        GtArgs a = hcgt_host::gt_args(p, ns, fa.L_out, reinterpret_cast<double*>(d2 + o_al),
                                      reinterpret_cast<double*>(d2 + o_gl), reinterpret_cast<int32_t*>(d2 + o_gi),
                                      reinterpret_cast<int32_t*>(d2 + o_gq));
        HIP_BAIL(hcgt_host::launch_arithmetic(a));
    }
    // ---- the one readback
    HIP_BAIL(hipMemcpyAsync(hb, d2, back, hipMemcpyDeviceToHost, st));
    if (want_L && L_total)
        HIP_BAIL(hipMemcpyAsync(hb + h_L, dv + fl.o_Lout, sizeof(double) * size_t(L_total), hipMemcpyDeviceToHost, st));
    HIP_BAIL(hipStreamSynchronize(st));
    trace.mark("read_back");
#undef HIP_BAIL

    out.flags = flags;
    out.n = n;
    out.read_off.resize(size_t(n));
    out.n_reads.resize(size_t(n));
    out.n_haps.resize(size_t(n));
    out.hap0.resize(size_t(n));
    out.L_off.resize(size_t(n));
    std::vector<hcgt_host::RegionView> views(static_cast<size_t>(n));
    for (int32_t r = 0; r < n; ++r) {
        out.read_off[size_t(r)] = pr[size_t(r)].read_off;
        out.n_reads[size_t(r)] = pr[size_t(r)].n_reads;
        out.n_haps[size_t(r)] = pr[size_t(r)].n_haps;
        out.hap0[size_t(r)] = pr[size_t(r)].hap0;
        out.L_off[size_t(r)] = pr[size_t(r)].L_off;
        views[size_t(r)] = hcgt_host::RegionView{regions[r].ref, regions[r].padded_begin, regions[r].n_haps};
    }
    out.keep.assign(reinterpret_cast<const uint8_t*>(hb + o_keepb), reinterpret_cast<const uint8_t*>(hb + o_keepb) + read_total);
    out.n_kept.assign(reinterpret_cast<const int32_t*>(hb + o_nk), reinterpret_cast<const int32_t*>(hb + o_nk) + n);
    if (want_L)
        out.L.assign(reinterpret_cast<const double*>(hb + h_L), reinterpret_cast<const double*>(hb + h_L) + L_total);
    if (ns > 0)
        hcgt_host::materialise(views.data(), hap_pool.data(), reinterpret_cast<const SiteOut*>(hb + o_so), ns,
                               reinterpret_cast<const double*>(hb + o_gl), reinterpret_cast<const int32_t*>(hb + o_gi),
                               reinterpret_cast<const int32_t*>(hb + o_gq),
                               want_lists ? reinterpret_cast<const int32_t*>(hb + o_keep) : nullptr, tot.keep_cap,
                               reinterpret_cast<const int32_t*>(hb + o_map), tot.map_cap, out.c);
    trace.mark("records");
    return HC_PHMM_OK;
}

bool region_ok(const hc_region_calls* c, int32_t region) { return c && region >= 0 && region < c->n; }

}  // namespace

extern "C" int hc_region_call(const hc_region_in* regions, int32_t n_regions, uint32_t flags, hc_region_calls** out)
{
    std::lock_guard<std::mutex> lk(g_st.mu);
    return call_frame(out, &g_st.stream, [&](hc_region_calls& calls) -> int {
        if (n_regions < 0 || (n_regions && !regions)) return fail(HC_PHMM_EINVAL, "null regions / negative count");
        constexpr uint32_t known = HC_REGION_F64 | HC_REGION_DEFAULT_MODE | HC_REGION_WANT_L | HC_REGION_WANT_SITE_READS |
                                   HC_REGION_WANT_CIGARS;
        if (flags & ~known) return fail(HC_PHMM_EINVAL, "unknown hc_region_call flags");
        if (int rc = g_st.ensure_init()) return rc;
        calls.flags = flags;
        return n_regions ? run(regions, n_regions, flags, calls) : HC_PHMM_OK;
    });
}

extern "C" int hc_region_calls_sites(const hc_region_calls* calls, const hc_gt_call_site** sites, int64_t* n)
{
    if (!calls || !sites || !n) return fail(HC_PHMM_EINVAL, "null argument");
    *sites = calls->c.sites.data();
    *n = int64_t(calls->c.sites.size());
    return HC_PHMM_OK;
}

extern "C" int hc_region_calls_reads(const hc_region_calls* calls, int32_t region, const uint8_t** keep,
                                     int32_t* n_reads, int32_t* n_kept)
{
    if (!region_ok(calls, region) || !keep || !n_reads || !n_kept) return fail(HC_PHMM_EINVAL, "bad argument");
    *keep = calls->keep.data() + calls->read_off[size_t(region)];
    *n_reads = calls->n_reads[size_t(region)];
    *n_kept = calls->n_kept[size_t(region)];
    return HC_PHMM_OK;
}

extern "C" int hc_region_calls_matrix(const hc_region_calls* calls, int32_t region, const double** L, int32_t* n_kept,
                                      int32_t* n_haps)
{
    if (!region_ok(calls, region) || !L || !n_kept || !n_haps) return fail(HC_PHMM_EINVAL, "bad argument");
    if (!(calls->flags & HC_REGION_WANT_L)) return fail(HC_PHMM_EINVAL, "the call did not ask for HC_REGION_WANT_L");
    *L = calls->L.data() + calls->L_off[size_t(region)];
    *n_kept = calls->n_kept[size_t(region)];
    *n_haps = calls->n_haps[size_t(region)];
    return HC_PHMM_OK;
}

extern "C" int hc_region_calls_alignment(const hc_region_calls* calls, int32_t region, int32_t hap, int32_t* begin,
                                         const char** cigar)
{
    if (!region_ok(calls, region) || !begin || !cigar || hap < 0 || hap >= calls->n_haps[size_t(region)])
        return fail(HC_PHMM_EINVAL, "bad argument");
    if (!(calls->flags & HC_REGION_WANT_CIGARS))
        return fail(HC_PHMM_EINVAL, "the call did not ask for HC_REGION_WANT_CIGARS");
    if (!calls->aligned[size_t(region)]) return fail(HC_PHMM_EINVAL, "the region's haplotypes brought their own CIGARs");
    const size_t k = size_t(calls->hap0[size_t(region)] + hap);
    *begin = calls->begins[k];
    *cigar = calls->cigars[k].c_str();
    return HC_PHMM_OK;
}

extern "C" int hc_region_calls_free(hc_region_calls* calls)
{
    delete calls;
    return HC_PHMM_OK;
}

// Test hook (tests only): region_finish_* alone on a caller's matrices. Region r
// has n_reads[r] x n_haps[r] values in L (regions back to back, read-major).
// L_out gets the capped kept rows, compact per region at the region's offset;
// keep the per-read flags; n_kept the per-region counts; order_out, per region
// at its read offset, the indices of the kept reads as the compacted intervals
// carry them.
extern "C" int hcx_region_finish(const double* L, int32_t n_regions, const int32_t* n_reads, const int32_t* n_haps,
                                 const int32_t* read_len, double* L_out, uint8_t* keep, int32_t* n_kept,
                                 int64_t* order_out)
{
    std::lock_guard<std::mutex> lk(g_st.mu);
    if (n_regions < 0 || (n_regions && (!n_reads || !n_haps || !n_kept)))
        return fail(HC_PHMM_EINVAL, "hcx_region_finish: bad argument");
    int rc = g_st.ensure_init();
    if (rc) return rc;
    if (n_regions == 0) return HC_PHMM_OK;
    const hipStream_t st = g_st.stream;
    std::vector<PlanRegion> pr(static_cast<size_t>(n_regions));
    int64_t reads = 0, L_total = 0;
    for (int32_t r = 0; r < n_regions; ++r) {
        if (n_reads[r] < 0 || n_haps[r] < 1 || n_haps[r] > HC_GT_MAX_HAPS)
            return fail(HC_PHMM_EINVAL, "hcx_region_finish: shape out of range");
        PlanRegion d{};
        d.L_off = L_total;
        d.n_haps = n_haps[r];
        d.read_off = int32_t(reads);
        d.n_reads = n_reads[r];
        pr[size_t(r)] = d;
        reads += n_reads[r];
        L_total += int64_t(n_reads[r]) * n_haps[r];
        if (reads > INT32_MAX) return fail(HC_PHMM_EINVAL, "hcx_region_finish: too many reads");
    }
    if (reads && (!L || !read_len || !L_out || !keep || !order_out))
        return fail(HC_PHMM_EINVAL, "hcx_region_finish: null array");
    Carver cv;
    const size_t o_reg = cv.take(sizeof(PlanRegion) * size_t(n_regions));
    const FinishLayout fl(cv, reads, L_total);
    const size_t o_keepb = cv.take(size_t(reads));
    const size_t o_nk = cv.take(sizeof(int32_t) * size_t(n_regions));
    rc = reserve(g_dev1, cv.off, "region caller device workspace");
    if (rc) return rc;
    rc = reserve(g_hin, fl.in_end, "region caller pinned workspace");
    if (rc) return rc;
    char* const h = g_hin.p;
    char* const dv = g_dev1.p;
    std::memcpy(h + o_reg, pr.data(), sizeof(PlanRegion) * size_t(n_regions));
    if (reads) {
        std::memcpy(h + fl.o_len, read_len, sizeof(int32_t) * size_t(reads));
        std::memcpy(h + fl.o_L, L, sizeof(double) * size_t(L_total));
        int64_t* rb = reinterpret_cast<int64_t*>(h + fl.o_rb);
        int64_t* re = reinterpret_cast<int64_t*>(h + fl.o_re);
        for (int32_t r = 0; r < n_regions; ++r)
            for (int32_t i = 0; i < n_reads[r]; ++i) {
                rb[pr[size_t(r)].read_off + i] = i;
                re[pr[size_t(r)].read_off + i] = int64_t(i) + 1000;
            }
    }
    HIP_TRY(st, hipMemcpyAsync(dv, h, fl.in_end, hipMemcpyHostToDevice, st));
    FinishArgs fa{};
    fa.regions = reinterpret_cast<PlanRegion*>(dv + o_reg);
    fa.n_regions = n_regions;
    fa.n_reads = int(reads);
    fa.read_len = reinterpret_cast<const int32_t*>(dv + fl.o_len);
    fa.L = reinterpret_cast<double*>(dv + fl.o_L);
    fa.read_begin = reinterpret_cast<const int64_t*>(dv + fl.o_rb);
    fa.read_end = reinterpret_cast<const int64_t*>(dv + fl.o_re);
    fa.L_out = reinterpret_cast<double*>(dv + fl.o_Lout);
    fa.begin_out = reinterpret_cast<int64_t*>(dv + fl.o_rbo);
    fa.end_out = reinterpret_cast<int64_t*>(dv + fl.o_reo);
    fa.keep = reinterpret_cast<uint8_t*>(dv + o_keepb);
    fa.dest = reinterpret_cast<int32_t*>(dv + fl.o_dest);
    fa.n_kept = reinterpret_cast<int32_t*>(dv + o_nk);
    // The out-of-place matrix starts as zeros here, so the rows behind the kept ones are defined.
    HIP_TRY(st, hipMemsetAsync(dv + fl.o_Lout, 0, sizeof(double) * size_t(std::max<int64_t>(L_total, 1)), st));
    HIP_TRY(st, hipMemsetAsync(dv + fl.o_rbo, 0xff, sizeof(int64_t) * size_t(std::max<int64_t>(reads, 1)), st));
    HIP_TRY(st, launch_finish(fa, st));
    HIP_TRY(st, hipStreamSynchronize(st));
    if (reads) {
        HIP_TRY(st, hipMemcpy(L_out, dv + fl.o_Lout, sizeof(double) * size_t(L_total), hipMemcpyDeviceToHost));
        HIP_TRY(st, hipMemcpy(keep, dv + o_keepb, size_t(reads), hipMemcpyDeviceToHost));
        HIP_TRY(st, hipMemcpy(order_out, dv + fl.o_rbo, sizeof(int64_t) * size_t(reads), hipMemcpyDeviceToHost));
    }
    HIP_TRY(st, hipMemcpy(n_kept, dv + o_nk, sizeof(int32_t) * size_t(n_regions), hipMemcpyDeviceToHost));
    return HC_PHMM_OK;
}
