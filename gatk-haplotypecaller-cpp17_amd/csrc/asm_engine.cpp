// Host engine + C ABI of the assembler (include/hc_asm.h).
//
// One call = the candidate haplotypes of any number of regions:
//
//   validate, lay out
//   one upload of [regions | sequences | base pool | quality pool]
//   asm_segments_kernel (one wave per window or read), asm_graph_kernel (one
//     workgroup per region, all attempts), both on the assembler's stream
//   one readback of the per-region records, the error word and the edge count,
//     then the on-path edges that were written
//   per region on the worker pool: paths, scores, sort and bytes (asm_paths.cpp)
//
// The workspace is the engine's own: six grow-only buffers of the shared host
// layer (stage_host.hpp, with the carver, the trace and HIP_TRY), released by
// hc_phmm_shutdown. A HIP error drains the assembler's stream before it returns.
// Calls serialise under the assembler's own lock and use the engine's primary
// device. HC_ASM_TRACE=1 prints the host wall clock of the phases on stderr, and
// from the device's own clock the share of the single-thread threading.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hc_asm.h"
#include "asm_kernels.hpp"
#include "asm_paths.hpp"
#include "pool.hpp"
#include "stage_host.hpp"

using namespace hcasm;
using namespace stage_host;

namespace {

int g_cus = 0;
int g_clock_khz = 0;   // of wall_clock64(), for the trace

Buf g_in, g_seg, g_work, g_out, g_hin{nullptr, 0, true}, g_hback{nullptr, 0, true};

// Once per stream: what the launch sizes and the trace need to know of the device.
Stage g_st({&g_in, &g_seg, &g_work, &g_out, &g_hin, &g_hback}, true, [](hipStream_t st) -> int {
    HIP_TRY(st, hipDeviceGetAttribute(&g_cus, hipDeviceAttributeMultiprocessorCount, hcphmm::primary_device()));
    if (hipDeviceGetAttribute(&g_clock_khz, hipDeviceAttributeWallClockRate, hcphmm::primary_device()) != hipSuccess)
        g_clock_khz = 0;
    return HC_PHMM_OK;
});

// The HC_PHMM_EINVAL cases, before any device work.
int validate(const hc_asm_region* regions, int32_t n)
{
    for (int32_t r = 0; r < n; ++r) {
        const hc_asm_region& g = regions[r];
        // (the texts are built only for the case that fails: a call has hundreds of thousands of reads)
        auto at = [&] { return "region " + std::to_string(r); };
        if (!g.ref) return fail(HC_PHMM_EINVAL, at() + ": null ref");
        if (g.ref_len < 1 || g.ref_len > HC_GT_MAX_REF_LEN)
            return fail(HC_PHMM_EINVAL, at() + ": ref_len outside 1 .. " + std::to_string(HC_GT_MAX_REF_LEN));
        if (g.n_reads < 0) return fail(HC_PHMM_EINVAL, at() + ": negative read count");
        if (g.n_reads && !g.reads) return fail(HC_PHMM_EINVAL, at() + ": null reads");
        int64_t sum = 0;
        for (int32_t j = 0; j < g.n_reads; ++j) {
            const hc_asm_read& rd = g.reads[j];
            auto rat = [&] { return at() + " read " + std::to_string(j); };
            if (rd.length < 0) return fail(HC_PHMM_EINVAL, rat() + ": negative length");
            if (rd.length > HC_PHMM_MAX_READ_LEN)
                return fail(HC_PHMM_EINVAL, rat() + ": longer than " + std::to_string(HC_PHMM_MAX_READ_LEN));
            if (rd.length && !rd.bases) return fail(HC_PHMM_EINVAL, rat() + ": null bases");
            if (rd.length && !rd.quals) return fail(HC_PHMM_EINVAL, rat() + ": null quals");
            sum += rd.length;
        }
        if (sum > HC_ASM_MAX_REGION_READ_BASES)
            return fail(HC_PHMM_EINVAL, at() + ": more than " + std::to_string(HC_ASM_MAX_REGION_READ_BASES) + " read bases");
    }
    return HC_PHMM_OK;
}

int run(const hc_asm_region* regions, int32_t n, uint32_t flags, hc_asm_result& res)
{
    Trace tr("HC_ASM_TRACE", "[hc_asm]");
    // ---- layout
    int64_t n_seqs = 0, pool = 0;
    int32_t max_bases = 1, max_hash = 64, max_cap = 1;
    int64_t edge_cap = 0;
    std::vector<AsmRegion> regs(static_cast<size_t>(n));
    for (int32_t r = 0; r < n; ++r) {
        const hc_asm_region& g = regions[r];
        AsmRegion& d = regs[size_t(r)];
        d.off = pool;
        d.ref_len = g.ref_len;
        int64_t bases = g.ref_len, cap = std::max(0, g.ref_len - (kFirstK - 1));
        for (int32_t j = 0; j < g.n_reads; ++j) {
            bases += g.reads[j].length;
            cap += std::max(0, g.reads[j].length - (kFirstK - 1));
        }
        d.n_bases = int32_t(bases);
        d.cap = int32_t(std::max<int64_t>(cap, 1));
        int32_t hs = 64;
        while (hs < 2 * d.cap) hs *= 2;
        d.hash_size = hs;
        pool += bases;
        n_seqs += 1 + g.n_reads;
        max_bases = std::max(max_bases, d.n_bases);
        max_hash = std::max(max_hash, d.hash_size);
        max_cap = std::max(max_cap, d.cap);
        edge_cap += std::min<int64_t>(d.cap, HC_ASM_MAX_GRAPH_EDGES);
    }
    if (n_seqs > INT32_MAX) return fail(HC_PHMM_EINVAL, "too many reads in one call");

    Carver in;
    const size_t o_reg = in.take(sizeof(AsmRegion) * size_t(n));
    const size_t o_seq = in.take(sizeof(AsmSeq) * size_t(n_seqs));
    const size_t o_bases = in.take(size_t(pool));
    const size_t o_quals = in.take(size_t(pool));
    const size_t in_bytes = in.off;
    int rc = reserve(g_hin, in_bytes, "assembler staging");
    if (rc) return rc;
    rc = reserve(g_in, in_bytes, "assembler input");
    if (rc) return rc;
    char* h = g_hin.p;
    std::memcpy(h + o_reg, regs.data(), sizeof(AsmRegion) * size_t(n));
    {
        // sequence records: their first index per region, then filled in parallel
        std::vector<int64_t> first(size_t(n) + 1, 0);
        for (int32_t r = 0; r < n; ++r) first[size_t(r) + 1] = first[size_t(r)] + 1 + regions[r].n_reads;
        AsmSeq* seqs = reinterpret_cast<AsmSeq*>(h + o_seq);
        uint8_t* hb = reinterpret_cast<uint8_t*>(h + o_bases);
        uint8_t* hq = reinterpret_cast<uint8_t*>(h + o_quals);
        hcphmm::parallel_for(
            n,
            [&](int64_t lo, int64_t hi) {
                for (int64_t r = lo; r < hi; ++r) {
                    const hc_asm_region& g = regions[r];
                    AsmSeq* s = seqs + first[size_t(r)];
                    int64_t at = regs[size_t(r)].off;
                    int32_t rel = 0;
                    *s++ = AsmSeq{at, g.ref_len, rel, 1, 0};
                    std::memcpy(hb + at, g.ref, size_t(g.ref_len));
                    std::memset(hq + at, 0, size_t(g.ref_len));
                    at += g.ref_len;
                    rel += g.ref_len;
                    for (int32_t j = 0; j < g.n_reads; ++j) {
                        const hc_asm_read& rd = g.reads[j];
                        *s++ = AsmSeq{at, rd.length, rel, 0, 0};
                        if (rd.length) {
                            std::memcpy(hb + at, rd.bases, size_t(rd.length));
                            std::memcpy(hq + at, rd.quals, size_t(rd.length));
                        }
                        at += rd.length;
                        rel += rd.length;
                    }
                }
            },
            8);
    }
    tr.mark("layout");

    // ---- device buffers
    const int n_slots = std::max(1, std::min<int>(n, 2 * std::max(g_cus, 1)));
    const size_t slot_bytes = asm_slot_bytes(max_bases, max_hash, max_cap);
    rc = reserve(g_seg, 2 * up(sizeof(int32_t) * size_t(pool)), "assembler segments");
    if (rc) return rc;
    rc = reserve(g_work, slot_bytes * size_t(n_slots), "assembler workspace");
    if (rc) return rc;
    Carver oc;   // the tail that is read back first, then the edges
    const size_t o_out = oc.take(sizeof(AsmOut) * size_t(n));
    const size_t o_used = oc.take(sizeof(unsigned long long));
    const size_t o_err = oc.take(sizeof(int32_t) * 2);
    const size_t head_bytes = oc.off;
    const size_t o_edges = oc.take(sizeof(hc_asm_edge) * size_t(edge_cap));
    rc = reserve(g_out, oc.off, "assembler output");
    if (rc) return rc;
    rc = reserve(g_hback, oc.off, "assembler readback");
    if (rc) return rc;

    AsmArgs a{};
    a.regions = reinterpret_cast<const AsmRegion*>(g_in.p + o_reg);
    a.n_regions = n;
    a.seqs = reinterpret_cast<const AsmSeq*>(g_in.p + o_seq);
    a.n_seqs = int32_t(n_seqs);
    a.bases = reinterpret_cast<const uint8_t*>(g_in.p + o_bases);
    a.quals = reinterpret_cast<const uint8_t*>(g_in.p + o_quals);
    a.rem = reinterpret_cast<int32_t*>(g_seg.p);
    a.seg_start = reinterpret_cast<int32_t*>(g_seg.p + up(sizeof(int32_t) * size_t(pool)));
    a.work = g_work.p;
    a.slot_bytes = slot_bytes;
    a.max_bases = max_bases;
    a.max_hash = max_hash;
    a.max_cap = max_cap;
    a.out = reinterpret_cast<AsmOut*>(g_out.p + o_out);
    a.edge_pool = reinterpret_cast<hc_asm_edge*>(g_out.p + o_edges);
    a.edge_pool_cap = edge_cap;
    a.edge_pool_used = reinterpret_cast<unsigned long long*>(g_out.p + o_used);
    a.err = reinterpret_cast<int32_t*>(g_out.p + o_err);

    HIP_TRY(g_st.stream, hipMemcpyAsync(g_in.p, h, in_bytes, hipMemcpyHostToDevice, g_st.stream));
    HIP_TRY(g_st.stream, hipMemsetAsync(g_out.p + o_used, 0, head_bytes - o_used, g_st.stream));
    if (tr.on) {
        HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
        tr.mark("upload");
    }
    HIP_TRY(g_st.stream, launch_asm_segments(a, g_st.stream));
    HIP_TRY(g_st.stream, launch_asm_graph(a, n_slots, g_st.stream));
    if (tr.on) {
        HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
        tr.mark("graph");
    }
    char* hb = g_hback.p;
    HIP_TRY(g_st.stream, hipMemcpyAsync(hb, g_out.p, head_bytes, hipMemcpyDeviceToHost, g_st.stream));
    HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
    int32_t err[2];
    std::memcpy(err, hb + o_err, sizeof(err));
    if (err[0] != kErrNone)
        return fail(HC_PHMM_EHIP, "assembler: an internal bound did not hold on the device (error word " +
                                      std::to_string(err[0]) + ", region " + std::to_string(err[1]) + ")");
    unsigned long long used = 0;
    std::memcpy(&used, hb + o_used, sizeof(used));
    if (used > static_cast<unsigned long long>(edge_cap)) return fail(HC_PHMM_EHIP, "assembler: edge count out of its bound");
    if (used) {
        HIP_TRY(g_st.stream, hipMemcpyAsync(hb + o_edges, g_out.p + o_edges, sizeof(hc_asm_edge) * size_t(used), hipMemcpyDeviceToHost,
                               g_st.stream));
        HIP_TRY(g_st.stream, hipStreamSynchronize(g_st.stream));
    }
    tr.mark("readback");

    // ---- host: paths, scores, order, bytes
    const AsmOut* outs = reinterpret_cast<const AsmOut*>(hb + o_out);
    const hc_asm_edge* pool_edges = reinterpret_cast<const hc_asm_edge*>(hb + o_edges);
    for (int32_t r = 0; r < n; ++r) {
        const AsmOut& o = outs[r];
        if (o.n_edges < 0 || o.edge_off < 0 || static_cast<unsigned long long>(o.edge_off) + size_t(o.n_edges) > used)
            return fail(HC_PHMM_EHIP, "assembler: a region's edge range is outside the pool");
    }
    if (tr.on && g_clock_khz > 0) {
        // the device's own clock: how much of the regions' time is the single-thread threading
        long long total = 0, walk = 0, slowest = 0, slowest_walk = 0;
        for (int32_t r = 0; r < n; ++r) {
            total += outs[r].t_total;
            walk += outs[r].t_walk;
            if (outs[r].t_total > slowest) {
                slowest = outs[r].t_total;
                slowest_walk = outs[r].t_walk;
            }
        }
        tr.value("walk_share", total ? double(walk) / double(total) : 0.0);
        tr.value("slowest_region_ms", double(slowest) / g_clock_khz);
        tr.value("its_walk_ms", double(slowest_walk) / g_clock_khz);
    }
    res.regions.resize(size_t(n));
    hcphmm::parallel_for(
        n,
        [&](int64_t lo, int64_t hi) {
            for (int64_t r = lo; r < hi; ++r) {
                const AsmOut& o = outs[r];
                RegionResult& rr = res.regions[size_t(r)];
                std::memcpy(rr.attempts, o.attempts, sizeof(rr.attempts));
                if (o.kmer_size == 0) {
                    rr.status = HC_ASM_NO_HAPLOTYPES;
                    continue;
                }
                rr.kmer_size = o.kmer_size;
                rr.source = o.source;
                rr.sink = o.sink;
                const hc_asm_edge* e = pool_edges + o.edge_off;
                paths_from_graph(regions[r].ref + o.source_pos, o.kmer_size, e, o.n_edges, o.source, o.sink, rr);
                if (flags & HC_ASM_WANT_GRAPH) rr.edges.assign(e, e + o.n_edges);
            }
        },
        1);
    tr.mark("paths");
    return HC_PHMM_OK;
}

}  // namespace

extern "C" int hc_asm_assemble(const hc_asm_region* regions, int32_t n_regions, uint32_t flags, hc_asm_result** out)
{
    std::lock_guard<std::mutex> lk(g_st.mu);
    return call_frame(out, &g_st.stream, [&](hc_asm_result& res) -> int {
        if (n_regions < 0 || (n_regions && !regions)) return fail(HC_PHMM_EINVAL, "null regions / negative count");
        if (flags & ~uint32_t(HC_ASM_WANT_GRAPH)) return fail(HC_PHMM_EINVAL, "unknown hc_asm_assemble flags");
        if (int rc = validate(regions, n_regions)) return rc;
        res.flags = flags;
        if (!n_regions) return HC_PHMM_OK;
        if (int rc = g_st.ensure_init()) return rc;
        return run(regions, n_regions, flags, res);
    });
}
