// Flat calls (hc_phmm_pairs_flat / hc_phmm_submit_pairs: independent pairs in
// the caller's host pools) planned on the device. The host does only what
// needs the caller's memory, in two parallel passes over the pairs
// (flat_records.hpp):
//   pass 1  validate, lengths and record sizes per mini-task, a sample of
//           haplotype lengths for the width-cap model (lengths only: 8 bytes
//           per pair);
//   pass 2  write each pair's record — base qualities, read and hap base codes
//           as nibbles (1.5 bytes per read base, 0.5 per hap base instead of
//           2 + 1), gap planes only when they vary — and descriptor into the
//           device's pinned staging ring, chunk by chunk, each chunk's H2D
//           overlapping the fill of the next. The gap qualities' constancy
//           (the reference's constant 'I'/'+' strings, sam.hpp:30-32, travel
//           as three bytes per read) is checked while filling; a part that
//           turns out to hold a read with varying gap qualities is planned
//           again with the check in pass 1, so its records carry the planes;
//           one whose reads or haps do not fit the compact fields (an 'N') is
//           planned again with the nibble fields (pass 1 still lengths only).
// The device then packs rows and hap tables, chooses each pair's
// column-segmented shape by the planner's cost model (plan_model.hpp), sorts
// the pairs by (block width, lanes, R) and cuts the sorted runs into waves
// (pack_kernels.hip flat_*), and runs the pass. No per-call pinned allocation.
//
// One attempt (plan_flat_try) is a driver over the stages below, in this
// order: flat_scan, flat_model, flat_chunks, flat_layout, flat_memory,
// fill_tables, bind_flat_part, upload_chunks, record_stage_rate,
// enqueue_flat_plan, flat_run.
#include <algorithm>
#include <chrono>
#include <atomic>
#include <cstring>

#include "engine_core.hpp"
#include "flat_records.hpp"
#include "part_setup.hpp"
#include "plan_model.hpp"
#include "pool.hpp"

namespace hcphmm {
namespace eng {
namespace {

constexpr int kMaxGroups = 1024;        // flat_scan_kernel: one group per thread
constexpr int kMaxBins = 1 << 20;

using clk = std::chrono::steady_clock;

struct FlatScratch {
    std::vector<int32_t> gapw;
    std::vector<uint8_t> fmtw;   // scanning pass 1: each pair's record format (kFmt* bits)
    std::vector<Mini> mini;
    std::vector<int32_t> hsamp;
};
thread_local FlatScratch t_fs;

bool default_policies()
{
    for (const char* e : {"HC_PHMM_KERNEL", "HC_PHMM_LANE_SEG"}) {
        const char* v = std::getenv(e);
        if (v && *v && std::strcmp(v, "auto") != 0) return false;
    }
    return env_i64("HC_PHMM_SEG_CAP", 0) <= 0 && env_i64("HC_PHMM_SEG_Q", -1) < 0 &&
           env_i64("HC_PHMM_FLAT_PLAN", 1) != 0;
}

// plan_flat_try's HC_PHMM_* settings, read once at its top.
struct FlatSettings {
    int64_t tail_rounds = std::max<int64_t>(0, env_i64("HC_PHMM_TAIL_ROUNDS", 2));
    int prep_blocks = int(env_i64("HC_PHMM_PREP_BLOCKS", 0));
};

// ---- the stages of one attempt

// Pass 1 over the part's pairs [lo, lo + n), folded: the mini-tasks' offsets
// (this thread's scratch) and the part's bounds and totals.
struct FlatScan {
    int64_t lo = 0, n = 0, nmini = 0;
    int64_t stride = 1, nsamp = 0;   // cap-model sample of hap lengths: every stride-th pair
    const Mini* mini = nullptr;
    const int32_t* gapw = nullptr;
    const uint8_t* fmtw = nullptr;
    const int32_t* hsamp = nullptr;
    FlatTotals t;
    clk::time_point scanned;   // pass 1 done (the staging clock runs to here, not over the fold)
};

FlatScan flat_scan(const Src& src, const PartSpec& spec, bool scan_gaps, int fmt0)
{
    FlatScratch& S = t_fs;
    FlatScan sc;
    sc.lo = spec.lo;
    sc.n = spec.hi - spec.lo;
    grow(S.gapw, size_t(sc.n));
    grow(S.fmtw, size_t(sc.n));
    sc.nmini = (sc.n + kMini - 1) / kMini;
    S.mini.assign(size_t(sc.nmini), Mini{});
    sc.stride = std::max<int64_t>(1, sc.n / 8192);
    sc.nsamp = (sc.n + sc.stride - 1) / sc.stride;
    grow(S.hsamp, size_t(sc.nsamp));
    scan_pass(src, sc.lo, sc.n, scan_gaps, fmt0, S.mini.data(), S.gapw.data(), S.fmtw.data(), S.hsamp.data(), sc.stride);
    sc.scanned = clk::now();
    sc.t = fold_minis(S.mini.data(), sc.nmini);
    sc.mini = S.mini.data();
    sc.gapw = S.gapw.data();
    sc.fmtw = S.fmtw.data();
    sc.hsamp = S.hsamp.data();
    return sc;
}

// Width cap and the per-length candidates; groups = distinct (BC, nb), widest
// block first; the counting-sort bins and the bound on the waves.
struct FlatModel {
    const float* waste = nullptr;
    std::vector<Cand> cand;       // per hap length in [hmin, hmax]
    std::vector<uint16_t> keys;   // group g: bc << 8 | nb
    std::vector<int> gid;         // key -> group
    int ngroups = 0;
    int rshift = 0, rspan = 0, nbins = 0;
    int64_t max_waves = 0;
};

// false: more groups or waves than the device passes take (the host planner's).
bool flat_model(const Src& src, const FlatScan& sc, int n_cu, FlatModel& M)
{
    const FlatTotals& t = sc.t;
    const double ravg = double(t.rows) / double(sc.n);
    int64_t lanes_at[kNCaps] = {};
    double work_at[kNCaps] = {};
    {   // the model over the sample's distinct lengths, weighted by their counts
        std::vector<int32_t> hist(size_t(std::min(t.hmax, 64 * kSegMaxBC)) + 1, 0);
        for (int64_t s = 0; s < sc.nsamp; ++s) ++hist[size_t(std::min(sc.hsamp[s], 64 * kSegMaxBC))];
        for (int H = 1; H < int(hist.size()); ++H)
            if (hist[size_t(H)]) cap_sample(H, ravg, sc.stride * hist[size_t(H)], lanes_at, work_at);
    }
    const CapChoice cc = choose_cap(lanes_at, work_at, n_cu);
    M.waste = cc.few_waves ? waste_per_lane() : waste_full();
    M.cand.assign(size_t(t.hmax) + 1, Cand{});
    for (int H = t.hmin; H <= t.hmax; ++H) {
        M.cand[size_t(H)] = cand_of(H, cc.cap);
        for (int q = 0; q < 2; ++q) M.keys.push_back(uint16_t(M.cand[size_t(H)].bc[q] << 8 | M.cand[size_t(H)].nb[q]));
    }
    std::sort(M.keys.begin(), M.keys.end(), std::greater<uint16_t>());
    M.keys.erase(std::unique(M.keys.begin(), M.keys.end()), M.keys.end());
    M.ngroups = int(M.keys.size());
    if (M.ngroups > kMaxGroups) return false;
    M.gid.assign(1 << 16, -1);
    for (int g = 0; g < M.ngroups; ++g) M.gid[M.keys[size_t(g)]] = g;
    // Counting-sort bins: (group, R descending), R coarsened if the span is wide.
    while (int64_t(M.ngroups) * (((t.rmax - t.rmin) >> M.rshift) + 1) > kMaxBins) ++M.rshift;
    M.rspan = ((t.rmax - t.rmin) >> M.rshift) + 1;
    M.nbins = M.ngroups * M.rspan;
    // Waves the launch must cover: at most ceil(pairs / per) per group, per =
    // floor(64 / nb) with nb the larger of a length's two candidates.
    std::vector<float> inv_per(size_t(t.hmax) + 1, 0.f);
    for (int H = t.hmin; H <= t.hmax; ++H)
        inv_per[size_t(H)] = 1.f / float(64 / std::max(M.cand[size_t(H)].nb[0], M.cand[size_t(H)].nb[1]));
    std::atomic<int64_t> wsum{0};
    const int32_t* Hs = src.H + sc.lo;
    parallel_for(sc.n, [&](int64_t a, int64_t e) {
        double s = 0;
        for (int64_t k = a; k < e; ++k) s += inv_per[size_t(Hs[k])];
        wsum += int64_t(s) + 2;
    }, 16384);
    M.max_waves = wsum.load() + M.ngroups + 1;
    return M.max_waves <= INT32_MAX / 4;
}

// Upload chunks: runs of mini-tasks whose records + descriptors fit a ring
// chunk; the boundaries (mini-task indices, first 0, last nmini). false: one
// mini-task larger than a chunk (the host planner's).
bool flat_chunks(const FlatScan& sc, std::vector<int64_t>& chunk_m)
{
    chunk_m.assign(1, 0);
    int64_t m = 0;
    while (m < sc.nmini) {
        int64_t e = m;
        auto bytes = [&](int64_t m1) {
            const int64_t r1 = m1 < sc.nmini ? sc.mini[m1].rec : sc.t.rec;
            const int64_t pairs = std::min(sc.n, m1 * kMini) - m * kMini;
            return ((r1 - sc.mini[m].rec + 255) & ~int64_t(255)) + int64_t(sizeof(FlatDesc)) * pairs;
        };
        while (e < sc.nmini && bytes(e + 1) <= int64_t(kRingChunk)) ++e;
        if (e == m) return false;
        chunk_m.push_back(e);
        m = e;
    }
    return true;
}

// Device layout: the upload image, descriptors and tables, then what the
// device builds, the outputs and the rescue scratch; and the host side's
// tables with (slots) the results image behind them.
struct FlatLayout {
    size_t o_img, o_desc, o_tab, o_rows, o_hapw, o_pairs, o_binof, o_hist, o_gtab, o_order, o_waves, o_wtmp, o_wcost,
        o_nw, o_slotof;
    RescueLayout RS;
    size_t tab_bytes, total, host_res_off;
    int tail;
};

int flat_layout(const FlatScan& sc, const FlatModel& M, const FlatSettings& cfg, int n_cu, FlatLayout& F)
{
    const FlatTotals& t = sc.t;
    const size_t n1 = size_t(sc.n);
    Layout L;
    F.o_img = L.take(size_t(t.rec) + 16);
    F.o_desc = L.take(sizeof(FlatDesc) * n1);
    F.tab_bytes = sizeof(int2) * (size_t(t.hmax) + 1) + sizeof(float) * 65 + sizeof(int2) * size_t(M.ngroups);
    F.o_tab = L.take(F.tab_bytes);
    const size_t row_pad = row_pad_words(t.rmax);
    if (const int bad = check_pool_words(t.rows, row_pad, t.hapw)) return bad;
    F.o_rows = L.take(sizeof(uint32_t) * (size_t(t.rows) + row_pad));
    F.o_hapw = L.take(sizeof(uint32_t) * (size_t(t.hapw) + 16));
    F.o_pairs = L.take(sizeof(PairDesc) * n1);
    F.o_binof = L.take(sizeof(int) * n1);
    F.o_hist = L.take(sizeof(int) * size_t(M.nbins));
    F.o_gtab = L.take(sizeof(int) * 3 * size_t(M.ngroups));
    F.o_order = L.take(sizeof(int) * n1);
    F.o_waves = L.take(sizeof(LaneWave) * size_t(M.max_waves));
    // The last two rounds of wave slots (3 per SIMD) dispatched longest first
    // (planner.cpp reorder_tail: 125k-pair shard 1.39 -> 1.25 ms with it on the host plan).
    F.tail = int(cfg.tail_rounds) * 4 * n_cu * 3;
    F.o_wtmp = L.take(F.tail > 0 ? sizeof(LaneWave) * size_t(M.max_waves) : 0);
    F.o_wcost = L.take(F.tail > 0 ? sizeof(int) * size_t(M.max_waves) : 0);
    F.o_nw = L.take(2 * sizeof(int));   // wave count, then the largest modelled wave cost
    F.RS = take_rescue(L, n1, n1);      // every pair is a seg pair: n1 slots
    F.o_slotof = L.take(sizeof(int) * n1);
    F.total = L.off;
    F.host_res_off = (F.tab_bytes + 255) & ~size_t(255);
    return HC_PHMM_OK;
}

// Jobs borrow their slot's workspace; batches (slot == nullptr) own their
// device memory, and their tables go up from plain host memory.
struct FlatMemory {
    char* dev = nullptr;
    char* host = nullptr;        // the tables (the slot's pinned area; its results image follows)
    std::vector<char> own_tab;   // a batch's
};

int flat_memory(Slot* slot, const FlatLayout& F, FlatMemory& mem)
{
    if (slot) {
        if (const int rc = slot_reserve(*slot, F.total, F.host_res_off + F.RS.RL.bytes)) return rc;
        mem.dev = slot->dev;
        mem.host = slot->host;
        return HC_PHMM_OK;
    }
    mem.own_tab.resize(F.tab_bytes);
    mem.host = mem.own_tab.data();
    if (hipMalloc(&mem.dev, F.total) != hipSuccess)
        return fail(HC_PHMM_ENOMEM, "device allocation failed (" + std::to_string(F.total >> 20) + " MiB)");
    return HC_PHMM_OK;
}

// The host tables: per hap length its two candidates with their groups, the
// lane-waste table, the groups.
void fill_tables(char* host, const FlatScan& sc, const FlatModel& M)
{
    const int hmin = sc.t.hmin, hmax = sc.t.hmax;
    int2* ct = reinterpret_cast<int2*>(host);
    for (int H = 0; H <= hmax; ++H) {
        if (H < hmin) {
            ct[H] = make_int2(0, 0);
            continue;
        }
        const Cand c = M.cand[size_t(H)];
        ct[H] = make_int2(c.bc[0] | c.nb[0] << 8 | M.gid[size_t(c.bc[0] << 8 | c.nb[0])] << 16,
                          c.bc[1] | c.nb[1] << 8 | M.gid[size_t(c.bc[1] << 8 | c.nb[1])] << 16);
    }
    float* wt = reinterpret_cast<float*>(ct + hmax + 1);
    std::memcpy(wt, M.waste, sizeof(float) * 65);
    int2* gt = reinterpret_cast<int2*>(wt + 65);
    for (int g = 0; g < M.ngroups; ++g) gt[g] = make_int2(M.keys[size_t(g)] >> 8, M.keys[size_t(g)] & 0xff);
}

// A new part that holds `dev` from the start: a batch's own allocation (freed
// with the part, or here if the part cannot be made), or the slot's.
Part* new_part_holding(Device& dv, Slot* slot, char* dev)
{
    Part* b = nullptr;
    try {
        b = new_part(&dv);
    } catch (...) {
        if (!slot) (void)hipFree(dev);
        throw;
    }
    b->slot = slot;
    b->dev_base = dev;
    return b;
}

void bind_flat_part(Part& b, Device& dv, const PartSpec& spec, Slot* slot, const FlatScan& sc, const FlatModel& M,
                    const FlatLayout& F, const FlatMemory& mem)
{
    char* dev = mem.dev;
    const size_t n1 = size_t(sc.n);
    b.spec = spec;
    b.n = sc.n;
    b.Hmax = sc.t.hmax;
    b.n_lane = int(sc.n);
    b.n_seg_waves = int(M.max_waves);
    b.lane_waves = int(M.max_waves);
    b.d_nwaves = reinterpret_cast<int*>(dev + F.o_nw);
    b.d_pairs = reinterpret_cast<PairDesc*>(dev + F.o_pairs);
    b.d_rows = reinterpret_cast<uint32_t*>(dev + F.o_rows) + kRowPadBefore;
    b.d_hapw = reinterpret_cast<uint32_t*>(dev + F.o_hapw);
    b.d_lane_order = reinterpret_cast<int*>(dev + F.o_order);
    b.d_lane_waves = reinterpret_cast<LaneWave*>(dev + F.o_waves);
    bind_rescue(b, dev, F.RS, n1);
    b.d_slot_of = reinterpret_cast<int*>(dev + F.o_slotof);
    b.n_wide = sc.t.nwide;
    if (slot) b.host_res = mem.host + F.host_res_off;
    bind_streams(b, dv, slot);
    b.upload_bytes = size_t(sc.t.rec) + sizeof(FlatDesc) * n1 + F.tab_bytes;
}

// Pass 2: chunks through the ring, each H2D'd as soon as it is filled.
// The staging rate counts the fills only: not the wait for the ring's
// lock (another part's fill) nor for a chunk's previous H2D (device
// backpressure), which are not host staging (advisor round 5).
struct Uploaded {
    clk::duration fill{};   // the fills' host time
    int refused = 0;        // kGapsVary | kNotCompact: stopped at the first refused chunk
};

int upload_chunks(Device& dv, const Src& src, const FlatScan& sc, bool scan_gaps, int fmt0,
                  const std::vector<int64_t>& chunk_m, char* d_img, char* d_desc, hipStream_t ps, Uploaded& up)
{
    std::atomic<int> retry{0};
    std::lock_guard<std::mutex> lk(dv.ring.mu);
    for (size_t c = 0; c + 1 < chunk_m.size(); ++c) {
        const int64_t m0 = chunk_m[c], m1 = chunk_m[c + 1];
        const int64_t p0 = m0 * kMini, p1 = std::min(sc.n, m1 * kMini);
        const int64_t r0 = sc.mini[m0].rec, r1 = m1 < sc.nmini ? sc.mini[m1].rec : sc.t.rec;
        const int ri = dv.ring.next;
        dv.ring.next = (ri + 1) % kRingN;
        if (dv.ring.used[ri]) HIP_TRY(hipEventSynchronize(dv.ring.ev[ri]));
        char* buf = dv.ring.buf[ri];
        const size_t dbase = (size_t(r1 - r0) + 255) & ~size_t(255);
        FlatDesc* dd = reinterpret_cast<FlatDesc*>(buf + dbase);
        const clk::time_point t_fill = clk::now();
        fill_chunk(src, sc.lo, sc.n, m0, m1, sc.mini, sc.gapw, sc.fmtw, scan_gaps, fmt0, buf, r0, dd, p0, retry);
        up.fill += clk::now() - t_fill;
        if ((up.refused = retry.load()) != 0) return HC_PHMM_OK;
        HIP_TRY(hipMemcpyAsync(d_img + r0, buf, size_t(r1 - r0), hipMemcpyHostToDevice, ps));
        HIP_TRY(hipMemcpyAsync(d_desc + sizeof(FlatDesc) * size_t(p0), dd, sizeof(FlatDesc) * size_t(p1 - p0),
                               hipMemcpyHostToDevice, ps));
        HIP_TRY(hipEventRecord(dv.ring.ev[ri], ps));
        dv.ring.used[ri] = true;
    }
    return HC_PHMM_OK;
}

// Running mean over calls (weight 1/2 to the newest part), of parts
// large enough to be pipeline parts (a small call's rate is its fixed
// costs': hc_phmm_init's warm-up call would read as slow staging).
void record_stage_rate(Device& dv, double cells, clk::duration t_stage)
{
    if (cells < 5e8) return;
    const double ps = std::chrono::duration<double, std::pico>(t_stage).count() / cells;
    double old_ps = dv.stage_ps_per_cell.load(std::memory_order_relaxed);
    while (!dv.stage_ps_per_cell.compare_exchange_weak(old_ps, old_ps > 0 ? 0.5 * (old_ps + ps) : ps,
                                                       std::memory_order_relaxed)) {
    }
}

// The tables' H2D and the device planning launch, between the pack events.
int enqueue_flat_plan(Part* b, const FlatScan& sc, const FlatModel& M, const FlatLayout& F, const FlatMemory& mem,
                      const FlatSettings& cfg, hipStream_t ps)
{
    char* dev = mem.dev;
    const size_t hmax1 = size_t(sc.t.hmax) + 1;
    if (const int rc = b->evs.make_pack()) return rc;
    HIP_TRY(hipMemcpyAsync(dev + F.o_tab, mem.host, F.tab_bytes, hipMemcpyHostToDevice, ps));
    HIP_TRY(hipEventRecord(b->evs.pack_begin(), ps));
    FlatPlanArgs a{};
    a.img = reinterpret_cast<const uint8_t*>(dev + F.o_img);
    a.desc = reinterpret_cast<const FlatDesc*>(dev + F.o_desc);
    a.n = int(sc.n);
    a.rows = b->d_rows;
    a.hapw = b->d_hapw;
    a.pairs = b->d_pairs;
    a.ctab = reinterpret_cast<const int2*>(dev + F.o_tab);
    a.waste = reinterpret_cast<const float*>(dev + F.o_tab + sizeof(int2) * hmax1);
    a.groups = reinterpret_cast<const int2*>(dev + F.o_tab + sizeof(int2) * hmax1 + sizeof(float) * 65);
    a.rmax = sc.t.rmax;
    a.rshift = M.rshift;
    a.rspan = M.rspan;
    a.bin_of = reinterpret_cast<int*>(dev + F.o_binof);
    a.hist = reinterpret_cast<int*>(dev + F.o_hist);
    a.nbins = M.nbins;
    a.ngroups = M.ngroups;
    a.gtab = reinterpret_cast<int*>(dev + F.o_gtab);
    a.order = b->d_lane_order;
    a.slot_of = b->d_slot_of;
    a.sdesc = b->d_sdesc;
    a.waves = b->d_lane_waves;
    a.waves_tmp = reinterpret_cast<LaneWave*>(dev + F.o_wtmp);
    a.wcost = reinterpret_cast<int*>(dev + F.o_wcost);
    a.tail = F.tail;
    a.max_waves = int(M.max_waves);
    a.nwaves = reinterpret_cast<int*>(dev + F.o_nw);
    a.counters = b->d_count;
    a.prep_blocks = cfg.prep_blocks;
    HIP_TRY(launch_flat_plan(a, ps));
    HIP_TRY(hipEventRecord(b->evs.pack_end(), ps));
    return HC_PHMM_OK;
}

// Jobs: the device pass and the return of its results. Batches run later; one
// that owns its memory waits here for its uploads.
int flat_run(Part* b, bool with_run, hipStream_t s)
{
    if (with_run) {
        if (const int r = run_part(b, s)) return r;
        return enqueue_results(b, s);
    }
    if (!b->slot) HIP_TRY(hipStreamSynchronize(s));   // the tables' host memory goes with this call
    return HC_PHMM_OK;
}

// ---- the driver

// What an attempt came to: an error (rc), else `what`, with the part if Planned.
struct FlatTry {
    int rc = HC_PHMM_OK;
    FlatOutcome what = FlatOutcome::HostPlanner;
    Part* part = nullptr;
};
FlatTry flat_error(int rc) { return FlatTry{rc, FlatOutcome::HostPlanner, nullptr}; }
FlatTry flat_is(FlatOutcome what, Part* p = nullptr) { return FlatTry{HC_PHMM_OK, what, p}; }

// One attempt: scan_gaps = false assumes constant gap qualities and format
// fmt0 everywhere (checked in pass 2; RetryPlanes / RetryNibbles if not), true
// finds each pair's in pass 1. record_rate: this attempt's host staging time
// updates the device's measured rate (not after a refused attempt, whose
// wasted work would read as slow staging).
FlatTry plan_flat_try(Device& dv, const Src& src, const PartSpec& spec, Slot* slot, bool with_run, bool scan_gaps,
                      int fmt0, bool record_rate)
{
    PhaseTimer tm;
    const FlatSettings cfg;
    const clk::time_point t_begin = clk::now();
    const int64_t n = spec.hi - spec.lo;
    if (n <= 0 || n > (int64_t(1) << 31) - 1) return flat_is(FlatOutcome::HostPlanner);

    const FlatScan sc = flat_scan(src, spec, scan_gaps, fmt0);
    clk::duration t_stage = sc.scanned - t_begin;   // scan + fill: the host staging rate (Device::stage_ps_per_cell)
    tm.mark("flat: scan");
    if (sc.t.bad)
        return flat_error(fail(HC_PHMM_EINVAL, "pair with invalid read length (1.." +
                                                   std::to_string(HC_PHMM_MAX_READ_LEN) + ") or hap length (1.." +
                                                   std::to_string(HC_PHMM_MAX_HAP_LEN) + ")"));
    // Every pair must fit the column-segmented kernel (64 lanes of 64 columns);
    // the host planner takes the others. So must the row and table pools.
    if (sc.t.hmax > 64 * kSegMaxBC || sc.t.rows > INT32_MAX - 4096 || sc.t.hapw > INT32_MAX)
        return flat_is(FlatOutcome::HostPlanner);
    FlatModel M;
    if (!flat_model(src, sc, dv.n_cu, M)) return flat_is(FlatOutcome::HostPlanner);
    tm.mark("flat: model");
    std::vector<int64_t> chunk_m;
    if (!flat_chunks(sc, chunk_m)) return flat_is(FlatOutcome::HostPlanner);
    FlatLayout F;
    if (const int rc = flat_layout(sc, M, cfg, dv.n_cu, F)) return flat_error(rc);
    if (slot) tm.mark("flat: layout (sizes)");
    FlatMemory mem;
    if (const int rc = flat_memory(slot, F, mem)) return flat_error(rc);
    tm.mark("flat: layout");
    fill_tables(mem.host, sc, M);

    Part* b = new_part_holding(dv, slot, mem.dev);
    PartGuard guard(b);   // error returns, refusals and exceptions discard it (and a batch's own allocation)
    bind_flat_part(*b, dv, spec, slot, sc, M, F, mem);
    // Uploads and preparation on the part's own stream (a greatest-priority
    // stream for them gained ~0.2 ms with four equal parts and lost with the
    // growing parts, profiles/r05_e2e_parts_ab.txt; removed).
    const hipStream_t s = b->stream;
    FlatTry r = flat_is(FlatOutcome::Planned, b);
    Uploaded up;
    int rc = upload_chunks(dv, src, sc, scan_gaps, fmt0, chunk_m, mem.dev + F.o_img, mem.dev + F.o_desc, s, up);
    t_stage += up.fill;
    if (!rc && up.refused) {
        r = flat_is((up.refused & kGapsVary) ? FlatOutcome::RetryPlanes : FlatOutcome::RetryNibbles);
    } else if (!rc) {
        tm.mark("flat: fill + H2D");
        if (record_rate) record_stage_rate(dv, spec.cells, t_stage);
        rc = enqueue_flat_plan(b, sc, M, F, mem, cfg, s);
        if (!rc) rc = flat_run(b, with_run, s);
    }
    tm.mark("flat: enqueue");
    // Anything but Planned: the guard drains the stream and discards the part (the caller returns the slot).
    if (rc) return flat_error(rc);
    if (r.what == FlatOutcome::Planned) guard.release();
    return r;
}

}  // namespace

int plan_flat_device(Device& dv, const Src& src, const PartSpec& spec, Slot* slot, bool with_run, Part** out,
                     FlatOutcome* what)
{
    *out = nullptr;
    *what = FlatOutcome::HostPlanner;
    if (!spec.flat || !src.R || !default_policies() || (!slot && with_run)) return HC_PHMM_OK;   // (the host planner's)
    // Compact fields unless a sample of the part shows a pair that does not
    // fit them; refused in pass 2: the nibble fields (pass 1 still lengths
    // only), and varying gap qualities: pass 1 scanning every read.
    // After a refusal the device's next kNibbleParts parts skip the compact
    // attempt (rare 'N's the sample misses: 1 read in 10 000 made every S2
    // part refuse in pass 2, 25.7 vs 12.6 ms a call).
    const int64_t n = spec.hi - spec.lo;
    const bool skip_compact = dv.nibble_parts.load(std::memory_order_relaxed) > 0 &&
                              dv.nibble_parts.fetch_sub(1, std::memory_order_relaxed) > 0;
    int fmt0 = !skip_compact && n > 0 && sample_fits_compact(src, spec.lo, n) ? compact_fmt() : 0;
    FlatTry t = plan_flat_try(dv, src, spec, slot, with_run, false, fmt0, true);
    if (!t.rc && t.what == FlatOutcome::RetryNibbles) {
        dv.nibble_parts.store(kNibbleParts, std::memory_order_relaxed);
        t = plan_flat_try(dv, src, spec, slot, with_run, false, 0, false);
    }
    if (!t.rc && t.what == FlatOutcome::RetryPlanes) t = plan_flat_try(dv, src, spec, slot, with_run, true, 0, false);
    if (t.rc) return t.rc;
    switch (t.what) {
    case FlatOutcome::Planned:
        *out = t.part;
        break;
    case FlatOutcome::HostPlanner:
        break;
    case FlatOutcome::RetryNibbles:   // (neither is refused with the nibble fields and scanned gaps)
    case FlatOutcome::RetryPlanes:
        return fail(HC_PHMM_EHIP, "flat planner: pass 2 refused a part planned with nibble fields and gap planes");
    }
    *what = t.what;
    return HC_PHMM_OK;
}

}  // namespace eng
}  // namespace hcphmm

// Host-logic test hook (not part of the ABI): the record's nibble packing.
extern "C" void hcx_pack_nibbles(const uint8_t* s, int n, uint8_t* d) { hcphmm::eng::pack_nibbles(s, n, d); }
// Host-logic test hooks (not part of the ABI): the compact record fields.
// Returns 1 if the read fits one byte per base (d holds it), else 0.
extern "C" int hcx_pack_read_1b(const uint8_t* q, const uint8_t* b, int n, uint8_t* d)
{
    return hcphmm::eng::read_1b(q, b, n, d) ? 1 : 0;
}
// Returns 1 if the hap has no 'N' (d holds its 2-bit codes), else 0.
extern "C" int hcx_pack_hap_2b(const uint8_t* s, int n, uint8_t* d) { return hcphmm::eng::pack_hap_2b(s, n, d) ? 1 : 0; }

// Host-pass timing without a GPU (not part of the ABI: tools/flat_host_bench.py):
// pass 1 and pass 2 of a flat call over pairs [0, n) into host memory, `reps`
// times; ms[0] = pass 1, ms[1] = pass 2 (mean per call).
extern "C" void hcx_flat_host_passes(int64_t n, const int64_t* read_off, const int32_t* R, const int64_t* hap_off,
                                     const int32_t* H, const uint8_t* rs, const uint8_t* q, const uint8_t* ins,
                                     const uint8_t* del, const uint8_t* gcp, const uint8_t* hap, int reps, double* ms)
{
    using namespace hcphmm;
    using namespace hcphmm::eng;
    const Src src = flat_src(read_off, R, hap_off, H, rs, q, ins, del, gcp, hap);
    const int64_t nmini = (n + kMini - 1) / kMini;
    std::vector<Mini> mini;
    std::vector<int32_t> gapw(static_cast<size_t>(n)), hsamp(static_cast<size_t>(n));
    std::vector<uint8_t> fmtw(static_cast<size_t>(n));
    std::vector<char> buf;
    std::vector<FlatDesc> dd(static_cast<size_t>(n));
    ms[0] = ms[1] = 0;
    for (int r = 0; r <= reps; ++r) {   // rep 0 sizes the buffers (untimed)
        auto t0 = std::chrono::steady_clock::now();
        mini.assign(size_t(nmini), Mini{});
        const int fmt0 = sample_fits_compact(src, 0, n) ? compact_fmt() : 0;
        scan_pass(src, 0, n, false, fmt0, mini.data(), gapw.data(), fmtw.data(), hsamp.data(),
                  std::max<int64_t>(1, n / 8192));
        const int64_t rec = fold_minis(mini.data(), nmini).rec;
        if (buf.size() < size_t(rec)) buf.resize(size_t(rec));
        auto t1 = std::chrono::steady_clock::now();
        std::atomic<int> retry{0};
        fill_chunk(src, 0, n, 0, nmini, mini.data(), gapw.data(), fmtw.data(), false, fmt0, buf.data(), 0, dd.data(),
                   0, retry);
        auto t2 = std::chrono::steady_clock::now();
        if (r == 0) continue;
        ms[0] += std::chrono::duration<double, std::milli>(t1 - t0).count() / reps;
        ms[1] += std::chrono::duration<double, std::milli>(t2 - t1).count() / reps;
    }
}
