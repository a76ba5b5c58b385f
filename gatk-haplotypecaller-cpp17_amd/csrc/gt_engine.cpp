// Host engine + C ABI of the genotyper numeric core (include/hc_gt.h).
//
// One call = every variant site of any number of regions: the regions'
// likelihood matrices are uploaded once each (sites of a region share it),
// with the kept-read lists and haplotype -> allele maps, in one H2D from a
// pinned staging block; one launch of gt_sites_kernel; one D2H of the genotype
// likelihoods, indices and qualities. hc_gt_call_regions plans the sites on the
// device first (events, scan, the counted readback, then the site kernel).
//
// Three grow-only buffers of the shared host layer (stage_host.hpp): device,
// site (sized by the counted readback) and pinned; every layout is written with
// its Carver, and a HIP error drains the genotyper's stream before it returns.
// What hc_region_call shares with this file is in gt_engine_internal.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/hc_gt.h"
#include "../../include/hc_pairhmm.h"
#include "gt_engine_internal.hpp"
#include "gt_kernels.hpp"
#include "gt_plan_kernels.hpp"
#include "pool.hpp"
#include "stage_host.hpp"

// MathUtils Jacobian table as g++ folds it at compile time (tools/gen_jacobian.py).
#include "math_jacobian.inc"

using namespace hcgt;
using namespace stage_host;

namespace {

double* g_jac = nullptr;
// Grow-only workspaces: sized by the input, by the site count, and the pinned image of either.
Buf g_dev, g_dev2, g_host{nullptr, 0, true};

// Once per stream: the Jacobian table on the device.
int upload_jacobian(hipStream_t st)
{
    HIP_TRY(st, hipMalloc(&g_jac, sizeof(double) * kJacobianLen));
    static_assert(sizeof(kMathJacobianBits) == sizeof(double) * kJacobianLen, "table length");
    HIP_TRY(st, hipMemcpy(g_jac, kMathJacobianBits, sizeof(double) * kJacobianLen, hipMemcpyHostToDevice));
    return HC_PHMM_OK;
}

void free_jacobian()
{
    if (g_jac) (void)hipFree(g_jac);
    g_jac = nullptr;
}

Stage& g_st = hcgt_host::stage();

// The one launch of the arithmetic, shared by hc_gt_genotype_sites (records,
// keep lists and maps uploaded) and hc_gt_call_regions (written on the device).
hipError_t launch_arithmetic(GtArgs& a)
{
    a.jac = g_jac;
    const double table_step = 0.0001;   // JacobianLogTable::TABLE_STEP (math_utils.hpp:24)
    a.inv_step = 1.0 / table_step;      // INV_STEP (:25)
    a.log10_2 = std::log10(2.0);        // std::log10(2) (genotyper.hpp:280,321)
    return launch_sites(a, g_st.stream);
}

int run(const hc_gt_site* sites, int32_t n)
{
    // Validate; one upload per distinct matrix.
    std::unordered_map<const double*, int32_t> mat_at;   // matrix -> index in mats
    std::vector<const hc_gt_site*> mats;                  // first site naming each matrix
    std::vector<int64_t> mat_off;                         // its offset in the L image
    std::vector<GtSite> ds(static_cast<size_t>(n));
    int64_t L_total = 0, keep_total = 0, map_total = 0, al_total = 0, out_total = 0;
    for (int32_t s = 0; s < n; ++s) {
        const hc_gt_site& x = sites[s];
        if (!x.L || x.n_reads < 0 || x.n_haps < 1 || x.n_keep < 0 || (x.n_keep && !x.keep) || !x.hap_allele ||
            x.n_alleles < 2 || x.n_alleles > HC_GT_MAX_ALLELES || !x.genotype_likelihoods || !x.genotype_index ||
            !x.genotype_quality)
            return fail(HC_PHMM_EINVAL, "site " + std::to_string(s) + ": bad argument");
        for (int32_t k = 0; k < x.n_keep; ++k)
            if (x.keep[k] < 0 || x.keep[k] >= x.n_reads)
                return fail(HC_PHMM_EINVAL, "site " + std::to_string(s) + ": kept read index out of range");
        for (int32_t h = 0; h < x.n_haps; ++h)
            if (x.hap_allele[h] < 0 || x.hap_allele[h] >= x.n_alleles)
                return fail(HC_PHMM_EINVAL, "site " + std::to_string(s) + ": haplotype allele out of range");
        auto it = mat_at.find(x.L);
        if (it == mat_at.end()) {
            it = mat_at.emplace(x.L, int32_t(mats.size())).first;
            mats.push_back(&x);
            mat_off.push_back(L_total);
            L_total += int64_t(x.n_reads) * x.n_haps;
        } else if (mats[size_t(it->second)]->n_reads != x.n_reads || mats[size_t(it->second)]->n_haps != x.n_haps) {
            // A matrix pointer shared by sites must describe the same shape.
            return fail(HC_PHMM_EINVAL, "sites sharing a matrix disagree on its shape");
        }
        GtSite& d = ds[size_t(s)];
        d.L_off = mat_off[size_t(it->second)];
        d.al_off = al_total;
        d.n_haps = x.n_haps;
        d.keep_off = int32_t(keep_total);
        d.n_keep = x.n_keep;
        d.map_off = int32_t(map_total);
        d.n_alleles = x.n_alleles;
        d.out_off = int32_t(out_total);
        keep_total += x.n_keep;
        map_total += x.n_haps;
        al_total += int64_t(x.n_keep) * x.n_alleles;
        out_total += x.n_alleles * (x.n_alleles + 1) / 2;
        if (keep_total > INT32_MAX || map_total > INT32_MAX || out_total > INT32_MAX)
            return fail(HC_PHMM_EINVAL, "too many sites for one call");
    }
    // Layout: [sites | L | keep | amap] uploaded, then [gl | gi | gq] read back, then scratch.
    Carver cv;
    const size_t o_sites = cv.take(sizeof(GtSite) * size_t(n));
    const size_t o_L = cv.take(sizeof(double) * size_t(L_total));
    const size_t o_keep = cv.take(sizeof(int32_t) * size_t(keep_total));
    const size_t o_map = cv.take(sizeof(int32_t) * size_t(map_total));
    const size_t in_bytes = cv.off;
    const size_t o_gl = cv.take(sizeof(double) * size_t(out_total));
    const size_t o_gi = cv.take(sizeof(int32_t) * size_t(n));
    const size_t o_gq = cv.take(sizeof(int32_t) * size_t(n));
    const size_t tail = cv.off - o_gl;
    const size_t o_al = cv.take(sizeof(double) * size_t(al_total));
    int rc = reserve(g_dev, cv.off, "genotyper device workspace");
    if (rc) return rc;
    rc = reserve(g_host, std::max(in_bytes, tail), "genotyper pinned workspace");
    if (rc) return rc;
    char* const h = g_host.p;
    char* const dv = g_dev.p;
    std::memcpy(h + o_sites, ds.data(), sizeof(GtSite) * size_t(n));
    // The likelihood matrices dominate the upload (512 regions of 415 x 32:
    // 54 MB): staged by the engine's worker pool, in slices so each slice's
    // H2D starts while the next is being copied.
    const int64_t nm = int64_t(mats.size());
    const int64_t slices = std::min<int64_t>(nm, 8);
    size_t sent = 0;
    for (int64_t sl = 0; sl < slices; ++sl) {
        const int64_t m0 = nm * sl / slices, m1 = nm * (sl + 1) / slices;
        hcphmm::parallel_for(m1 - m0, [&](int64_t lo, int64_t hi) {
            for (int64_t k = m0 + lo; k < m0 + hi; ++k) {
                const hc_gt_site* m = mats[size_t(k)];
                std::memcpy(h + o_L + sizeof(double) * size_t(mat_off[size_t(k)]), m->L,
                            sizeof(double) * size_t(m->n_reads) * size_t(m->n_haps));
            }
        }, 1);
        const size_t end = m1 < nm ? o_L + sizeof(double) * size_t(mat_off[size_t(m1)]) : o_keep;
        HIP_TRY(g_st.stream, hipMemcpyAsync(dv + sent, h + sent, end - sent, hipMemcpyHostToDevice, g_st.stream));
        sent = end;
    }
    for (int32_t s = 0; s < n; ++s) {
        const hc_gt_site& x = sites[s];
        if (x.n_keep) std::memcpy(h + o_keep + sizeof(int32_t) * size_t(ds[size_t(s)].keep_off), x.keep, sizeof(int32_t) * size_t(x.n_keep));
        std::memcpy(h + o_map + sizeof(int32_t) * size_t(ds[size_t(s)].map_off), x.hap_allele, sizeof(int32_t) * size_t(x.n_haps));
    }
    HIP_TRY(g_st.stream, hipMemcpyAsync(dv + sent, h + sent, in_bytes - sent, hipMemcpyHostToDevice, g_st.stream));
    GtArgs a{};
    a.sites = reinterpret_cast<const GtSite*>(dv + o_sites);
    a.n = n;
    a.L = reinterpret_cast<const double*>(dv + o_L);
    a.keep = reinterpret_cast<const int32_t*>(dv + o_keep);
    a.amap = reinterpret_cast<const int32_t*>(dv + o_map);
    a.al = reinterpret_cast<double*>(dv + o_al);
    a.gl = reinterpret_cast<double*>(dv + o_gl);
    a.gi = reinterpret_cast<int32_t*>(dv + o_gi);
    a.gq = reinterpret_cast<int32_t*>(dv + o_gq);
    HIP_TRY(g_st.stream, launch_arithmetic(a));
    HIP_TRY(g_st.stream, hipMemcpyAsync(h, dv + o_gl, tail, hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
    const double* gl = reinterpret_cast<const double*>(h);
    const int32_t* gi = reinterpret_cast<const int32_t*>(h + (o_gi - o_gl));
    const int32_t* gq = reinterpret_cast<const int32_t*>(h + (o_gq - o_gl));
    for (int32_t s = 0; s < n; ++s) {
        const hc_gt_site& x = sites[s];
        std::memcpy(x.genotype_likelihoods, gl + ds[size_t(s)].out_off,
                    sizeof(double) * size_t(x.n_alleles * (x.n_alleles + 1) / 2));
        *x.genotype_index = gi[s];
        *x.genotype_quality = gq[s];
    }
    return HC_PHMM_OK;
}


// ---- hc_gt_call_regions: events, sites, alleles, maps and kept reads on the device ----

using hcgt_host::Calls;
using hcgt_host::RegionView;

// "%d%c" runs of M I D S, each with the window and haplotype position it starts at.
bool parse_cigar(const char* t, int32_t begin, std::vector<PlanRun>& runs, int32_t& ref_pos, int32_t& hap_pos)
{
    ref_pos = begin;
    hap_pos = 0;
    if (!*t) return false;
    while (*t) {
        if (*t < '0' || *t > '9') return false;
        int64_t len = 0;
        while (*t >= '0' && *t <= '9') {
            len = len * 10 + (*t++ - '0');
            if (len > HC_GT_MAX_REF_LEN + HC_GT_MAX_HAP_LEN) return false;
        }
        if (len < 1) return false;
        PlanRun r{int32_t(len), 0, ref_pos, hap_pos};
        switch (*t++) {
        case 'M': r.op = kOpM; ref_pos += r.len; hap_pos += r.len; break;
        case 'I': r.op = kOpI; hap_pos += r.len; break;
        case 'D': r.op = kOpD; ref_pos += r.len; break;
        case 'S': r.op = kOpS; hap_pos += r.len; break;
        default: return false;   // the reference throws on any other operator
        }
        if (ref_pos > HC_GT_MAX_REF_LEN || hap_pos > HC_GT_MAX_HAP_LEN) return false;
        runs.push_back(r);
    }
    return true;
}

int run_regions(const hc_gt_region* regions, int32_t n, Calls& out)
{
    std::vector<PlanRegion> pr(static_cast<size_t>(n));
    std::vector<PlanHap> ph;
    std::vector<PlanRun> runs;
    std::string hap_pool;
    hcgt_host::FrameTotals t;
    for (int32_t r = 0; r < n; ++r) {
        const hc_gt_region& x = regions[r];
        const hcgt_host::RegionFrame f{!x.ref || !x.haps || (x.n_reads > 0 && (!x.read_begin || !x.read_end || !x.L)),
                                       x.ref_len, x.n_haps, x.n_reads, x.padded_begin, x.origin_begin, x.origin_end};
        auto haps = [&](const std::string& at) {
            for (int32_t h = 0; h < x.n_haps; ++h) {
                const hc_gt_hap_aln& y = x.haps[h];
                const std::string hat = at + " haplotype " + std::to_string(h);
                if (int rc = hcgt_host::check_hap_frame(hat, !y.bases || !y.cigar, y.length, y.alignment_begin, x.ref_len))
                    return rc;
                PlanHap e;
                e.region = r;
                e.base_off = int32_t(hap_pool.size());
                e.run_off = int32_t(runs.size());
                e.tab_off = int32_t(t.tab + int64_t(h) * x.ref_len);
                if (int rc = hcgt_host::parse_hap_cigar(hat, y.cigar, y.alignment_begin, y.length, x.ref_len, runs)) return rc;
                e.n_runs = int32_t(runs.size()) - e.run_off;
                hap_pool.append(reinterpret_cast<const char*>(y.bases), size_t(y.length));
                ph.push_back(e);
            }
            return HC_PHMM_OK;
        };
        if (int rc = hcgt_host::add_region(r, f, t, pr[size_t(r)], haps, ph, hap_pool, runs)) return rc;
    }
    // Workspace 1: [regions | haps | runs | ref | hap | read_begin | read_end | L] uploaded, then
    // [bitmap | base | totals | ev | span] written by the events and scan kernels.
    const size_t nh = ph.size();
    Carver cv;
    hcgt_host::PlanOffsets o{};
    o.reg = cv.take(sizeof(PlanRegion) * size_t(n));
    o.hap = cv.take(sizeof(PlanHap) * nh);
    o.runs = cv.take(sizeof(PlanRun) * runs.size());
    o.ref = cv.take(size_t(t.ref));
    o.pool = cv.take(hap_pool.size());
    o.read_begin = cv.take(sizeof(int64_t) * size_t(t.reads));
    o.read_end = cv.take(sizeof(int64_t) * size_t(t.reads));
    const size_t o_L = cv.take(sizeof(double) * size_t(t.L));
    const size_t in_bytes = cv.off;
    o.bitmap = cv.take(sizeof(uint32_t) * kBitmapWords * size_t(n));
    o.base = cv.take(sizeof(PlanBase) * size_t(n));
    o.totals = cv.take(sizeof(PlanTotals));
    o.ev = cv.take(sizeof(int16_t) * size_t(t.tab));
    o.span = cv.take(sizeof(int16_t) * size_t(t.tab));
    const size_t h_tot = in_bytes;   // the totals land behind the staged input
    int rc = reserve(g_dev, cv.off, "genotyper device workspace");
    if (rc) return rc;
    rc = reserve(g_host, in_bytes + 256, "genotyper pinned workspace");
    if (rc) return rc;
    char* h = g_host.p;
    char* const dv = g_dev.p;
    std::memcpy(h + o.reg, pr.data(), sizeof(PlanRegion) * size_t(n));
    std::memcpy(h + o.hap, ph.data(), sizeof(PlanHap) * nh);
    std::memcpy(h + o.runs, runs.data(), sizeof(PlanRun) * runs.size());
    std::memcpy(h + o.pool, hap_pool.data(), hap_pool.size());
    for (int32_t r = 0; r < n; ++r) {
        const hc_gt_region& x = regions[r];
        std::memcpy(h + o.ref + size_t(pr[size_t(r)].ref_off), x.ref, size_t(x.ref_len));
        if (x.n_reads) {
            std::memcpy(h + o.read_begin + sizeof(int64_t) * size_t(pr[size_t(r)].read_off), x.read_begin, sizeof(int64_t) * size_t(x.n_reads));
            std::memcpy(h + o.read_end + sizeof(int64_t) * size_t(pr[size_t(r)].read_off), x.read_end, sizeof(int64_t) * size_t(x.n_reads));
        }
    }
    HIP_TRY(g_st.stream, hipMemcpyAsync(dv, h, o_L, hipMemcpyHostToDevice, g_st.stream));
    PlanArgs p = hcgt_host::plan_args(dv, o, n, nh);
    HIP_TRY(g_st.stream, launch_plan_events(p, g_st.stream));
    HIP_TRY(g_st.stream, hipMemcpyAsync(h + h_tot, dv + o.totals, sizeof(PlanTotals), hipMemcpyDeviceToHost, g_st.stream));
    // The matrices are staged while the events and scan kernels run.
    hcphmm::parallel_for(n, [&](int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; ++r) {
            const hc_gt_region& x = regions[r];
            if (x.n_reads)
                std::memcpy(h + o_L + sizeof(double) * size_t(pr[size_t(r)].L_off), x.L,
                            sizeof(double) * size_t(x.n_reads) * size_t(x.n_haps));
        }
    }, 1);
    if (t.L) HIP_TRY(g_st.stream, hipMemcpyAsync(dv + o_L, h + o_L, in_bytes - o_L, hipMemcpyHostToDevice, g_st.stream));
    // The one counted readback: the site count sizes everything that follows.
    HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
    PlanTotals tot;
    std::memcpy(&tot, h + h_tot, sizeof(tot));
    const int64_t ns = tot.n_sites;
    if (ns < 0 || ns > t.site_bound || tot.keep_cap > t.keep_bound || tot.map_cap > t.map_bound)
        return fail(HC_PHMM_EHIP, "genotyper site count out of its bound");
    if (ns == 0) return HC_PHMM_OK;
    // Workspace 2: [site_out | gl | gi | gq | keep, amap] read back, then [gt_sites | al] scratch.
    // keep and amap are one piece, the map directly behind the keep list: materialise gets them as one block.
    Carver c2;
    const size_t o_so = c2.take(sizeof(SiteOut) * size_t(ns));
    const size_t o_gl = c2.take(sizeof(double) * kMaxGenotypes * size_t(ns));
    const size_t o_gi = c2.take(sizeof(int32_t) * size_t(ns));
    const size_t o_gq = c2.take(sizeof(int32_t) * size_t(ns));
    const size_t o_keep = c2.take(sizeof(int32_t) * size_t(tot.keep_cap + tot.map_cap));
    const size_t o_map = o_keep + sizeof(int32_t) * size_t(tot.keep_cap);
    const size_t back = c2.off;
    const size_t o_gs = c2.take(sizeof(GtSite) * size_t(ns));
    const size_t o_al = c2.take(sizeof(double) * kMaxAlleles * size_t(tot.keep_cap));
    rc = reserve(g_dev2, c2.off, "genotyper site workspace");
    if (rc) return rc;
    rc = reserve(g_host, back, "genotyper pinned workspace");
    if (rc) return rc;
    h = g_host.p;
    char* const d2 = g_dev2.p;
    p.site_out = reinterpret_cast<SiteOut*>(d2 + o_so);
    p.gt_sites = reinterpret_cast<GtSite*>(d2 + o_gs);
    p.keep = reinterpret_cast<int32_t*>(d2 + o_keep);
    p.amap = reinterpret_cast<int32_t*>(d2 + o_map);
    HIP_TRY(g_st.stream, launch_plan_sites(p, ns, g_st.stream));
    GtArgs a = hcgt_host::gt_args(p, ns, reinterpret_cast<const double*>(dv + o_L), reinterpret_cast<double*>(d2 + o_al),
                                  reinterpret_cast<double*>(d2 + o_gl), reinterpret_cast<int32_t*>(d2 + o_gi),
                                  reinterpret_cast<int32_t*>(d2 + o_gq));
    HIP_TRY(g_st.stream, launch_arithmetic(a));
    HIP_TRY(g_st.stream, hipMemcpyAsync(h, d2, back, hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
    std::vector<RegionView> views(static_cast<size_t>(n));
    for (int32_t r = 0; r < n; ++r) views[size_t(r)] = RegionView{regions[r].ref, regions[r].padded_begin, regions[r].n_haps};
    hcgt_host::materialise(views.data(), hap_pool.data(), reinterpret_cast<const SiteOut*>(h + o_so), ns,
                           reinterpret_cast<const double*>(h + o_gl), reinterpret_cast<const int32_t*>(h + o_gi),
                           reinterpret_cast<const int32_t*>(h + o_gq), reinterpret_cast<const int32_t*>(h + o_keep),
                           tot.keep_cap, reinterpret_cast<const int32_t*>(h + o_map), tot.map_cap, out);
    return HC_PHMM_OK;
}

}  // namespace

namespace hcgt_host {

Stage& stage()
{
    static Stage st({&g_dev, &g_dev2, &g_host}, true, upload_jacobian, free_jacobian);
    return st;
}
hipError_t launch_arithmetic(hcgt::GtArgs& a) { return ::launch_arithmetic(a); }

int add_region(int32_t r, const RegionFrame& f, FrameTotals& t, PlanRegion& d,
               const std::function<int(const std::string& at)>& haps, const std::vector<PlanHap>& ph,
               const std::string& hap_pool, const std::vector<PlanRun>& runs)
{
    const std::string at = "region " + std::to_string(r);
    if (f.null_pointer) return fail(HC_PHMM_EINVAL, at + ": null pointer");
    if (f.ref_len < 1 || f.ref_len > HC_GT_MAX_REF_LEN || f.n_haps < 1 || f.n_haps > HC_GT_MAX_HAPS || f.n_reads < 0)
        return fail(HC_PHMM_EINVAL, at + ": ref_len, n_haps or n_reads out of range");
    if (f.padded_begin < 0 || f.origin_begin < f.padded_begin || f.origin_end < f.origin_begin ||
        f.origin_end > f.padded_begin + f.ref_len)
        return fail(HC_PHMM_EINVAL, at + ": origin outside the padded window");
    d.padded_begin = f.padded_begin;
    d.origin_begin = f.origin_begin;
    d.origin_end = f.origin_end;
    d.L_off = t.L;
    d.ref_off = int32_t(t.ref);
    d.ref_len = f.ref_len;
    d.hap0 = int32_t(ph.size());
    d.n_haps = f.n_haps;
    d.read_off = int32_t(t.reads);
    d.n_reads = f.n_reads;
    if (int rc = haps(at)) return rc;
    const int64_t width = std::min<int64_t>(f.origin_end - f.origin_begin, f.ref_len);
    t.ref += f.ref_len;
    t.reads += f.n_reads;
    t.L += int64_t(f.n_reads) * f.n_haps;
    t.tab += int64_t(f.n_haps) * f.ref_len;
    t.site_bound += width;
    t.keep_bound += width * f.n_reads;   // by the unfiltered count: a scan may run before a filter
    t.map_bound += width * f.n_haps;
    if (t.tab > INT32_MAX || hap_pool.size() > size_t(INT32_MAX) || runs.size() > size_t(INT32_MAX) ||
        t.reads > INT32_MAX || t.site_bound * kMaxGenotypes > INT32_MAX || t.keep_bound > INT32_MAX ||
        t.map_bound > INT32_MAX)
        return fail(HC_PHMM_EINVAL, "too many regions for one call");
    return HC_PHMM_OK;
}

PlanArgs plan_args(char* base, const PlanOffsets& o, int32_t n_regions, size_t n_haps)
{
    PlanArgs p{};
    p.regions = reinterpret_cast<const PlanRegion*>(base + o.reg);
    p.n_regions = n_regions;
    p.haps = reinterpret_cast<const PlanHap*>(base + o.hap);
    p.n_haps = int(n_haps);
    p.runs = reinterpret_cast<const PlanRun*>(base + o.runs);
    p.ref = reinterpret_cast<const uint8_t*>(base + o.ref);
    p.hap = reinterpret_cast<const uint8_t*>(base + o.pool);
    p.read_begin = reinterpret_cast<const int64_t*>(base + o.read_begin);
    p.read_end = reinterpret_cast<const int64_t*>(base + o.read_end);
    p.ev = reinterpret_cast<int16_t*>(base + o.ev);
    p.span = reinterpret_cast<int16_t*>(base + o.span);
    p.bitmap = reinterpret_cast<uint32_t*>(base + o.bitmap);
    p.base = reinterpret_cast<PlanBase*>(base + o.base);
    p.totals = reinterpret_cast<PlanTotals*>(base + o.totals);
    return p;
}

GtArgs gt_args(const PlanArgs& p, int64_t n_sites, const double* L, double* al, double* gl, int32_t* gi, int32_t* gq)
{
    GtArgs a{};
    a.sites = p.gt_sites;
    a.n = int(n_sites);
    a.L = L;
    a.keep = p.keep;
    a.amap = p.amap;
    a.al = al;
    a.gl = gl;
    a.gi = gi;
    a.gq = gq;
    return a;
}

int check_hap_frame(const std::string& hat, bool null_pointer, int32_t length, int32_t alignment_begin, int32_t ref_len)
{
    if (null_pointer) return fail(HC_PHMM_EINVAL, hat + ": null pointer");
    if (length < 1 || length > HC_GT_MAX_HAP_LEN || alignment_begin < 0 || alignment_begin > ref_len)
        return fail(HC_PHMM_EINVAL, hat + ": length or alignment_begin out of range");
    return HC_PHMM_OK;
}

int parse_hap_cigar(const std::string& hat, const char* cigar, int32_t alignment_begin, int32_t length, int32_t ref_len,
                    std::vector<hcgt::PlanRun>& runs)
{
    int32_t ref_end = 0, hap_end = 0;
    if (!parse_cigar(cigar, alignment_begin, runs, ref_end, hap_end))
        return fail(HC_PHMM_EINVAL, hat + ": bad CIGAR '" + std::string(cigar).substr(0, 64) + "'");
    if (hap_end != length)
        return fail(HC_PHMM_EINVAL, hat + ": CIGAR consumes " + std::to_string(hap_end) + " bases of " +
                                        std::to_string(length));
    if (ref_end > ref_len) return fail(HC_PHMM_EINVAL, hat + ": CIGAR runs past the reference window");
    return HC_PHMM_OK;
}

// Strings from the alt descriptors, pointers into the copied blocks.
void materialise(const RegionView* regions, const char* hap_pool, const hcgt::SiteOut* so, int64_t ns, const double* gl,
                 const int32_t* gi, const int32_t* gq, const int32_t* keep_in, int64_t keep_cap, const int32_t* amap_in,
                 int64_t map_cap, Calls& out)
{
    const size_t nk = keep_in ? size_t(keep_cap) : 0;
    out.ints.resize(nk + size_t(map_cap));
    if (nk) std::memcpy(out.ints.data(), keep_in, sizeof(int32_t) * nk);
    if (map_cap) std::memcpy(out.ints.data() + nk, amap_in, sizeof(int32_t) * size_t(map_cap));
    const int32_t* keep = keep_in ? out.ints.data() : nullptr;
    const int32_t* amap = out.ints.data() + nk;
    out.sites.resize(size_t(ns));
    size_t n_ptrs = 0, n_gl = 0;
    std::vector<size_t> text_at;
    for (int64_t s = 0; s < ns; ++s) {
        const SiteOut& o = so[s];
        if (o.n_alleles > HC_GT_MAX_ALLELES) continue;
        const RegionView& x = regions[o.region];
        const char* ref = reinterpret_cast<const char*>(x.ref);
        const size_t R = size_t(o.ref_len);
        text_at.push_back(out.text.size());
        out.text.insert(out.text.end(), ref + o.pos, ref + o.pos + R);
        out.text.push_back('\0');
        for (int32_t k = 0; k + 1 < o.n_alleles; ++k) {
            const AltDesc& d = o.alt[k];
            const char* own = hap_pool + d.hap_off;
            text_at.push_back(out.text.size());
            if (d.kind == kAltStar) {
                out.text.push_back('*');
            } else if (d.kind == kAltSnp) {
                out.text.push_back(*own);
                out.text.insert(out.text.end(), ref + o.pos + 1, ref + o.pos + R);
            } else if (d.kind == kAltIns) {
                out.text.push_back(ref[o.pos]);
                out.text.insert(out.text.end(), own, own + d.len);
                out.text.insert(out.text.end(), ref + o.pos + 1, ref + o.pos + R);
            } else {
                out.text.push_back(ref[o.pos]);
                out.text.insert(out.text.end(), ref + o.pos + d.len + 1, ref + o.pos + R);
            }
            out.text.push_back('\0');
        }
        n_ptrs += size_t(o.n_alleles);
        n_gl += size_t(o.n_alleles * (o.n_alleles + 1) / 2);
    }
    out.ptrs.resize(n_ptrs);
    out.gl.resize(n_gl);
    for (size_t k = 0; k < n_ptrs; ++k) out.ptrs[k] = out.text.data() + text_at[k];
    n_ptrs = n_gl = 0;
    for (int64_t s = 0; s < ns; ++s) {
        const SiteOut& o = so[s];
        hc_gt_call_site& c = out.sites[size_t(s)];
        c = hc_gt_call_site{};
        c.region = o.region;
        c.begin = regions[o.region].padded_begin + o.pos;
        c.loc_end = c.begin + o.ref_len;
        c.n_alleles = o.n_alleles;
        c.genotype_index = c.a1 = c.a2 = c.genotype_quality = -1;
        if (o.n_alleles > HC_GT_MAX_ALLELES) {
            c.status = HC_GT_SITE_TOO_MANY_ALLELES;
            continue;
        }
        const int32_t A = o.n_alleles, G = A * (A + 1) / 2;
        c.n_haps = regions[o.region].n_haps;
        c.alleles = out.ptrs.data() + n_ptrs;
        c.hap_allele = amap + o.map_off;
        c.keep = keep ? keep + o.keep_off : nullptr;
        c.n_keep = keep ? o.n_keep : 0;
        c.n_genotypes = G;
        std::memcpy(out.gl.data() + n_gl, gl + s * kMaxGenotypes, sizeof(double) * size_t(G));
        c.genotype_likelihoods = out.gl.data() + n_gl;
        n_ptrs += size_t(A);
        n_gl += size_t(G);
        c.genotype_index = gi[s];
        c.genotype_quality = gq[s];
        int32_t a1 = 0, rem = gi[s];   // allele_index_cache: a1-major, a1 <= a2
        while (rem >= A - a1) {
            rem -= A - a1;
            ++a1;
        }
        c.a1 = a1;
        c.a2 = a1 + rem;
        c.status = gi[s] == 0 ? HC_GT_SITE_HOM_REF
                   : (a1 == 0 && gq[s] < 50) ? HC_GT_SITE_LOW_QUALITY_HET   // MIN_HETEROZYGOSITY_QUALITY
                                             : HC_GT_SITE_EMITTED;
    }
}

}  // namespace hcgt_host

struct hc_gt_calls {
    Calls c;
};

extern "C" int hc_gt_genotype_sites(const hc_gt_site* sites, int32_t n_sites)
{
    std::lock_guard<std::mutex> lk(g_st.mu);
    if (n_sites < 0 || (n_sites && !sites)) return fail(HC_PHMM_EINVAL, "null sites / negative count");
    if (int rc = g_st.ensure_init()) return rc;
    if (n_sites == 0) return HC_PHMM_OK;
    return run(sites, n_sites);
}

extern "C" int hc_gt_call_regions(const hc_gt_region* regions, int32_t n_regions, hc_gt_calls** out)
{
    std::lock_guard<std::mutex> lk(g_st.mu);
    return call_frame(out, &g_st.stream, [&](hc_gt_calls& calls) -> int {
        if (n_regions < 0 || (n_regions && !regions)) return fail(HC_PHMM_EINVAL, "null regions / negative count");
        if (int rc = g_st.ensure_init()) return rc;
        return n_regions ? run_regions(regions, n_regions, calls.c) : HC_PHMM_OK;
    });
}

extern "C" int hc_gt_calls_sites(const hc_gt_calls* calls, const hc_gt_call_site** sites, int64_t* n)
{
    if (!calls || !sites || !n) return fail(HC_PHMM_EINVAL, "null argument");
    *sites = calls->c.sites.data();
    *n = int64_t(calls->c.sites.size());
    return HC_PHMM_OK;
}

extern "C" int hc_gt_calls_free(hc_gt_calls* calls)
{
    delete calls;
    return HC_PHMM_OK;
}
