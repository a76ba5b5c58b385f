// Internal interface of the PairHMM host engine (libhcpairhmm.so), shared by
//   device.cpp   device slots: init / shutdown, per-slot streams + workspaces
//   planner.cpp  host planning of a part: length binning, wave packing, staging
//   flat_plan.cpp  flat batches planned on the device (the real call path):
//                  plan_flat_try drives named stages; flat_records.hpp holds
//                  its host record passes (host-only: src_view.hpp, kernels.hpp)
//   run.cpp      the device pass of a part and the host log10 finish
//   api.cpp      splitting calls into parts, submit / collect, the C ABI
//
// The reference's computeLikelihoodsNative (intel_pairhmm.hpp:115-152) split
// into plan / execute / finish over one or more device slots:
//   plan     (host) length-bin the pairs and pack them into waves, or (flat
//            calls) only stage the raw inputs and let the device plan them
//   execute  (device) H2D, pack rows + hap match tables, fp32 kernels ->
//            raw f32 + rescue list, fp64 rescue over the list, D2H of results
//   finish   (host) glibc log10f / log10 exactly as intel_pairhmm.hpp:137-143,
//            scattered into the caller's outputs
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_pairhmm.h"
#include "kernels.hpp"
#include "src_view.hpp"

namespace stage_host {
void release_all();   // stage_host.cpp: every stage engine's stream and workspace
}

namespace hcphmm {

// Shared with the stage engines (stage_host.hpp).
void set_last_error(const std::string& msg);
int primary_device();   // HIP ordinal of the first device slot, -1 if not initialised

namespace eng {

int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return ::hcphmm::eng::fail(HC_PHMM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

int64_t env_i64(const char* name, int64_t dflt);
// Test hook (hcx_test_plan_timeout, api.cpp): the fp64 launch's non-planner
// workgroups give up waiting for the plan at once. Off unless a test sets it;
// no environment variable reaches it.
bool test_plan_timeout();

// HC_PHMM_TRACE=1: per-phase host timings on stderr.
struct PhaseTimer {
    bool on;
    std::chrono::steady_clock::time_point t0;
    PhaseTimer() : on(std::getenv("HC_PHMM_TRACE") != nullptr), t0(std::chrono::steady_clock::now()) {}
    void mark(const char* what)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[hc_phmm] %-22s %8.3f ms\n", what,
                     std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// ---------------------------------------------------------------------------
// Device slots (device.cpp).

// Grow-only workspace of one part in flight: device memory (upload image,
// packed rows and tables, outputs, scratch) and pinned host memory (upload
// image, then the D2H'd results).
struct Slot {
    char* dev = nullptr;
    size_t dev_cap = 0;
    char* host = nullptr;
    size_t host_cap = 0;
    bool busy = false;
    // Streams of the part in this slot: parts in different slots of one device
    // run concurrently (a call cut into parts overlaps the planning of part
    // k + 1 and the kernels of part k, and its kernels fill the chip together).
    hipStream_t stream = nullptr, side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;   // side-stream fork / join (timing disabled)
    hipEvent_t ev[7] = {};   // pack [2], fp32 / fp64 pass [3], done, early results: reused by every part in the slot (bind_streams)
    hipEvent_t up_ev[2] = {};   // staging halves: H2D of a half done (timing disabled)
};

// Pinned staging ring of a device: the flat call path streams its upload
// through these chunks (fill chunk k on the host while chunk k-1 is copied),
// so no call allocates pinned memory; allocated once at init.
constexpr int kRingN = 4;
constexpr size_t kRingChunk = size_t(32) << 20;
struct Ring {
    std::mutex mu;   // held by one part's fill at a time
    char* buf[kRingN] = {};
    hipEvent_t ev[kRingN] = {};   // the last H2D out of each chunk
    bool used[kRingN] = {};
    int next = 0;
};

struct Device {
    int ordinal = 0;
    int n_cu = 256;   // compute units (4 SIMDs each): sizes the latency models
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;                  // segmented waves beside one-lane waves
    hipStream_t aux = nullptr;                   // speculative fp64 beside the fp32 pass
    hipEvent_t fork = nullptr, join = nullptr;   // side-stream fork / join (timing disabled)
    float* lut_f = nullptr;
    double* lut_d = nullptr;
    std::vector<Slot*> slots;
    double outstanding = 0;   // cells submitted and not yet collected
    Ring ring;
    // Host staging time of flat parts (scan + fill), ps per cell, a running
    // mean over the calls so far (0: none yet): sizes a call's parts
    // (api.cpp submit_flat, HC_PHMM_PART_GROWTH_PCT).
    std::atomic<double> stage_ps_per_cell{0.0};
    // Flat parts left to start with the nibble records without trying the
    // compact ones: set when a part's compact attempt is refused in pass 2 (a
    // rare 'N' its sample missed), so data that carries them pays one refusal
    // per kNibbleParts parts, not one per part (flat_plan.cpp plan_flat_device).
    std::atomic<int> nibble_parts{0};
};
constexpr int kNibbleParts = 64;

// Engine state, guarded by g_mu: the device list, the slot pools, the
// outstanding counters, and the number of parts alive and calls running (a
// shutdown while either is non-zero is refused: parts hold Device / Slot
// pointers).
extern std::mutex g_mu;
extern std::vector<Device*> g_devs;
extern int64_t g_live_parts;
extern int64_t g_active_calls;
// hc_phmm_init flags of the most recent successful init (HC_PHMM_FLAG_*): the
// default mode of later calls and batches (HC_PHMM_FLAG_F64 = initNative(
// use_double = true)), captured into each PartSpec when the call is made.
extern std::atomic<uint32_t> g_flags;

int init_devices_locked(const int32_t* devices, int32_t n, bool any_ok);
// Slots made at hc_phmm_init per device (a flat call of S2's size runs 8
// parts; more are made on demand).
constexpr int kInitSlots = 8;
Slot* make_slot();   // a new idle slot of the current device (streams, events)
Slot* take_slot(Device& d);
void give_slot(Slot* s);
int slot_reserve(Slot& s, size_t dev_bytes, size_t host_bytes);
void release_device(Device* d);

// A call in progress: initialises the engine on first use and snapshots the
// device list; shutdown is refused while any call holds one.
class CallGuard {
public:
    CallGuard();
    ~CallGuard();
    CallGuard(const CallGuard&) = delete;
    CallGuard& operator=(const CallGuard&) = delete;
    int rc = HC_PHMM_OK;
    std::vector<Device*> devs;
};

// ---------------------------------------------------------------------------
// Inputs.

// ReadView / HapView / Src, flat_src: src_view.hpp.

// Cross-product block: reads [r0, r0+nr) x haps [h0, h0+nh) of the Src, results
// to out[r * ostride + h] (read-major, as hc_phmm_cross / a region).
struct Block {
    int64_t r0;
    int32_t nr;
    int64_t h0;
    int32_t nh;
    double* out;
    int64_t ostride;
};

// Caller outputs of flat (pair) calls; any may be null.
struct Outputs {
    double* loglik = nullptr;
    float* raw32 = nullptr;
    double* raw64 = nullptr;
    uint8_t* resc = nullptr;
};

// What one part computes: flat pairs [lo, hi) (read p x hap p), or blocks.
struct PartSpec {
    bool flat = true;
    int64_t lo = 0, hi = 0;
    std::vector<Block> blocks;
    // hc_phmm_init flags of the call (HC_PHMM_FLAG_F64 = initNative's
    // use_double), fixed when the call is made: the reference's g_use_double
    // is per IntelPairHMM instance (intel_pairhmm.hpp:58,81), so a later init
    // from another thread must not switch the mode of work already submitted.
    uint32_t flags = 0;
    // Parts below this many pairs write results in place instead of per-slot
    // records (run.cpp); -1: HC_PHMM_REC_MIN_PAIRS (200 000). A part of a
    // pipelined call takes 40 000: its gather's latency is hidden behind the
    // next part's staging.
    int64_t rec_min = -1;
    double cells = 0;   // R x H summed over the part's pairs (flat parts)
};

// Planning modes: a real part (device calls), or a dry run that plans on the
// host only and keeps the plan for the host-logic tests (hcx_* hooks).
enum class PlanMode { Real, Dry };

// A part's results block, one contiguous device range returned to the host by
// one store (enqueue_results): [raw32 | raw64 | flag | run counters]. The run
// counters (kNumCounters ints, kernels.hpp) ride along so the host sees the
// device error word (kErrWord) with the results, at no extra transfer.
// (part_setup.hpp res_layout lays it out.)
struct ResLayout {
    size_t o64 = 0, ofl = 0, ocnt = 0, bytes = 0;
};
// The block's typed pointers at `base`: the device block, the pinned host
// image, or a host copy.
struct ResView {
    float* raw32;
    double* raw64;
    uint8_t* flag;
    int* counters;
};
inline ResView res_view(char* base, const ResLayout& r)
{
    return {reinterpret_cast<float*>(base), reinterpret_cast<double*>(base + r.o64),
            reinterpret_cast<uint8_t*>(base + r.ofl), reinterpret_cast<int*>(base + r.ocnt)};
}

// ---------------------------------------------------------------------------
// A part's events, each with its owner: a job part borrows its slot's (pack
// pair, first run triple, done, early; Slot::ev), a batch part makes its own as
// they are needed; a further run of either makes a triple the part owns. The
// destructor destroys exactly the owned ones (the part's device current).
// A batch's run triples accumulate until hc_phmm_batch_stats reads them
// (reset_runs); they are reused after that, never shrunk.
class RunEvents {
public:
    // start, end of the fp32 pass, end of the fp64 pass (not recorded when the
    // run was solo: no fp64 launch, ev[1] ends the run).
    struct Run {
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        bool own = false, solo = false;
    };
    RunEvents() = default;
    RunEvents(const RunEvents&) = delete;
    RunEvents& operator=(const RunEvents&) = delete;
    ~RunEvents()
    {
        for (Run& r : runs_)
            for (hipEvent_t e : r.ev)
                if (r.own && e) (void)hipEventDestroy(e);
        for (hipEvent_t e : pack_)
            if (own_pack_ && e) (void)hipEventDestroy(e);
        if (own_done_ && done_) (void)hipEventDestroy(done_);
    }
    // The slot's seven (pack 0-1, the first run 2-4, done 5, early results 6).
    void borrow(hipEvent_t const (&ev)[7])
    {
        pack_[0] = ev[0];
        pack_[1] = ev[1];
        Run r;
        for (int k = 0; k < 3; ++k) r.ev[k] = ev[2 + k];
        runs_.push_back(r);
        done_ = ev[5];
        early_ = ev[6];
    }
    // The pack pair, around the part's device preparation (made unless borrowed).
    int make_pack()
    {
        if (pack_[0] && pack_[1]) return HC_PHMM_OK;
        own_pack_ = true;
        for (auto& e : pack_)
            if (!e) HIP_TRY(hipEventCreate(&e));
        return HC_PHMM_OK;
    }
    hipEvent_t pack_begin() const { return pack_[0]; }   // null: none made yet
    hipEvent_t pack_end() const { return pack_[1]; }
    // The next run's triple (a new one the part owns when all are in use).
    int begin_run(Run** run)
    {
        if (used_ == runs_.size()) {
            Run r;
            r.own = true;
            for (auto& e : r.ev)
                if (hipEventCreate(&e) != hipSuccess) {
                    for (hipEvent_t x : r.ev)
                        if (x) (void)hipEventDestroy(x);
                    return fail(HC_PHMM_EHIP, "hipEventCreate");
                }
            runs_.push_back(r);
        }
        *run = &runs_[used_++];
        (*run)->solo = false;
        return HC_PHMM_OK;
    }
    size_t n_runs() const { return used_; }   // since the last reset_runs
    void reset_runs() { used_ = 0; }
    // The event that ends run k.
    hipEvent_t end_of(size_t k) const { return runs_[k].ev[runs_[k].solo ? 1 : 2]; }
    // Device time of run k's passes once it has ended (waits for it); a solo
    // run's fp64 time is 0.
    hipError_t run_ms(size_t k, float* f32, float* f64) const
    {
        const Run& r = runs_[k];
        *f32 = *f64 = 0;
        hipError_t e = hipEventSynchronize(end_of(k));
        if (e == hipSuccess) e = hipEventElapsedTime(f32, r.ev[0], r.ev[1]);
        if (e == hipSuccess && !r.solo) e = hipEventElapsedTime(f64, r.ev[1], r.ev[2]);
        return e;
    }
    // Jobs: the D2H of the results complete (made on first use unless borrowed).
    int make_done()
    {
        if (done_) return HC_PHMM_OK;
        own_done_ = true;
        HIP_TRY(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
        return HC_PHMM_OK;
    }
    hipEvent_t done() const { return done_; }
    // Jobs: the fp32 pass's raw sums and flags on the host while the fp64
    // launch runs (run_part), so collect() finishes the unflagged pairs early.
    hipEvent_t early() const { return early_; }   // the slot's; null: never
    bool early_used = false;                      // the last run stored them early

private:
    hipEvent_t pack_[2] = {nullptr, nullptr};
    hipEvent_t done_ = nullptr, early_ = nullptr;
    bool own_pack_ = false, own_done_ = false;
    std::vector<Run> runs_;
    size_t used_ = 0;
};

// ---------------------------------------------------------------------------
// A part prepared on one device: every device array lives in one allocation,
// filled by H2D copies from one pinned staging image.
struct Part {
    Device* dev = nullptr;
    PartSpec spec;
    int64_t n = 0;          // pairs
    int64_t cells = 0;
    int Hmax = 0;
    struct Cls {
        int W = 16;
        int n = 0;
        int ring_len = 0;
        int* d_order = nullptr;
    } cls[2];
    int n_lane = 0;
    int n_seg_waves = 0;
    int lane_waves = 0;
    int lane_variant = 0;
    const int* d_nwaves = nullptr;   // device-planned parts: the wave count lives on the device
    int max_seg_waves = 0;           //   and this bounds it (the launch grid)
    int* d_lane_order = nullptr;
    LaneWave* d_lane_waves = nullptr;
    float2* d_carry = nullptr;
    void* d_ring = nullptr;        // anti-diagonal rings beyond the LDS (planner.cpp)
    PairDesc* d_pairs = nullptr;
    uint32_t* d_rows = nullptr;
    uint32_t* d_hapw = nullptr;
    float* d_raw32 = nullptr;     // current output targets (own or bound)
    double* d_raw64 = nullptr;
    uint8_t* d_flag = nullptr;
    float* own_raw32 = nullptr;   // outputs in the part's allocation: [raw32 | raw64 | flag]
    double* own_raw64 = nullptr;
    uint8_t* own_flag = nullptr;
    ResLayout res;                // that contiguous output block (res_view)
    uint4* d_rec = nullptr;       // seg slot result records (LaneArgs::rec), gathered by the fp64 launch
    int* d_slot_of = nullptr;     // pair -> seg slot (-1: one-lane / anti-diagonal pair)
    PairDesc* d_sdesc = nullptr;  // seg slot -> pair descriptor (pairs[order[slot]])
    int* d_list = nullptr;
    int* d_sorted = nullptr;
    int* d_worder = nullptr;      // fp64 pass: dispatch position -> wave
    int* d_big = nullptr;
    int* d_big_count = nullptr;
    Seg64Plan* d_plan = nullptr;
    int64_t n_wide = 0;
    int wide_ring_blocks = 0;     // fp64 wide pass: workgroups its global ring has room for (0: ring in LDS)
    int* d_count = nullptr;
    int inker_limit = 0;   // in-wave rescues allowed in the last run
    int parity = 0;
    char* dev_base = nullptr;
    Slot* slot = nullptr;         // borrowed workspace (jobs), else dev_base is owned
    char* host_res = nullptr;     // pinned results image (slot) after the D2H
    size_t upload_bytes = 0;
    RunEvents evs;                // pack, run, done and early events, the slot's or its own
    hipStream_t stream = nullptr;             // the part's stream: its slot's, else its device's
    hipStream_t side = nullptr;               // segmented waves beside one-lane waves
    hipEvent_t fork = nullptr, join = nullptr;
    hipStream_t last_stream = nullptr;
    int64_t launch_waves = 0;
    bool ran = false;
    unsigned long long* timeline = nullptr;   // HC_PHMM_TIMELINE=1: this part's wave records
    int timeline_n = 0;                       //   (allocated), of which the fp32 seg waves' first,
    int timeline_n32 = 0;                     //   then the fp64 waves' (Seg64Args::timeline)
};

Part* new_part(Device* d);   // counted in g_live_parts
void free_part(Part* p);
void discard_part(Part* p);  // failed before hand-out: the slot and its memory stay with the caller

// A part under construction: discarded (after its stream drains) when the
// planner leaves by an error return or an exception, unless handed out.
class PartGuard {
public:
    explicit PartGuard(Part* p) : p_(p) {}
    ~PartGuard()
    {
        if (!p_) return;
        if (p_->stream) (void)hipStreamSynchronize(p_->stream);
        discard_part(p_);
    }
    PartGuard(const PartGuard&) = delete;
    PartGuard& operator=(const PartGuard&) = delete;
    Part* release()
    {
        Part* q = p_;
        p_ = nullptr;
        return q;
    }

private:
    Part* p_;
};

// planner.cpp: plan one part on device d. A driver over named stages:
// scan_inputs, upload_layout + staging_memory, classify_haps, then
// choose_grid_policy + plan_grid (cross products) or plan_general
// (classify_pairs, sort_seg_pairs, pack_seg_waves), reorder_tail,
// bin_lane_and_diag, fill_staging; dry runs stop there (keep_dry_dump,
// *out = nullptr); then device_layout, bind_part and enqueue_upload (the H2D,
// device packing and, with_run, the device pass and the D2H of the results,
// all on the part's stream). slot == nullptr: the part owns its memory
// (batches). part_setup.hpp holds what it shares with plan_flat_device.
int plan_part(Device& d, const Src& src, const PartSpec& spec, Slot* slot, bool with_run, PlanMode mode,
              Part** out);
// flat_plan.cpp: a flat part whose pairs are planned on the device. What came
// of it, beside the HC_PHMM_* return code (which is an error's alone): the part
// is planned (*out), the host planner must take it, or (one attempt,
// plan_flat_try) pass 2 refused it and it is planned again with the nibble
// fields or with the gap planes.
enum class FlatOutcome { Planned, HostPlanner, RetryNibbles, RetryPlanes };
int plan_flat_device(Device& d, const Src& src, const PartSpec& spec, Slot* slot, bool with_run, Part** out,
                     FlatOutcome* what);
// run.cpp
int run_part(Part* b, hipStream_t s);
// which: every pair; the unflagged ones only (their raw f64 is 0: d unread);
// the flagged ones only.
enum class Finish { All, Plain, Rescued };
void finish_part(const Part& P, const float* f, const double* d, const uint8_t* fl, const Outputs& o,
                 Finish which = Finish::All);
// Enqueue the results' return to the pinned host image and the part's done
// event (with_run parts). A kernel stores them into the mapped host memory
// rather than a DMA copy: DMA copies run in enqueue order, so a D2H enqueued
// behind its part's kernels held the next part's uploads until those kernels
// finished (the parts of a call ran one after another: S2 end to end 22 ms).
int enqueue_results(Part* b, hipStream_t s);
int check_device_error(const int* counters);   // run.cpp: counters = a host copy of a part's run counters

// The last dry-run plan (hcx_dump_sizes / hcx_dump_plan).
struct DryDump {
    std::mutex mu;
    std::vector<int4> pairs;
    std::vector<int> order;
    std::vector<LaneWave> waves;
    int n_seg_slots = 0;
    bool grid = false;
};
extern DryDump g_dump;

// HC_PHMM_TIMELINE=1 diagnostics: the last traced part's records.
struct TimelineRef {
    std::mutex mu;
    const Part* part = nullptr;
    unsigned long long* buf = nullptr;
    int n = 0;
    hipStream_t stream = nullptr;
    int ordinal = 0;
};
extern TimelineRef g_tl;

}  // namespace eng
}  // namespace hcphmm

struct hc_phmm_batch {
    std::vector<hcphmm::eng::Part*> parts;   // one per device slot
    int64_t n = 0;
};

struct hc_phmm_job {
    std::vector<hcphmm::eng::Part*> parts;
    hcphmm::eng::Outputs out;
    std::vector<double> cells_per_part;
};
