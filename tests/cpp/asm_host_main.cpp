// Stand-alone host program over the assembler's host code, built with
// -fsanitize=address,undefined by tests/test_asm_host.py. No GPU, no Python.
//
//   graph  <in> <out>   a reduced graph through hcx_asm_paths_from_graph (asm_paths.cpp)
//   bubbles <n>         a chain of n two-way bubbles through the same hook: 2^n paths
//   emul   <in> <out>   whole regions: the text of the device's graph phases
//                       (csrc/asm_graph_body.hpp) compiled for one host thread, with the
//                       ballot arithmetic of asm_segments_kernel emulated lane by lane,
//                       then the paths. What the device computes, bounds checked.
//   emulslot <in> <out> the same with one workspace slice for all the regions, in order
//
// Files are text, bytes in hex:
//   graph in:  k source_kmer source sink n_edges, then n_edges x "from to count seq base is_ref"
//   emul in:   n_regions, then per region "ref n_reads" and n_reads x "bases quals" ("-" = empty)
//   out:       per region "R status k attempts n_haps n_paths source sink n_edges",
//              n_edges x "E from to count seq base is_ref", n_haps x "H score_bits bases"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#define ASMX_HOST_ONLY
#define ASMX_FN
#define ASMX_TID 0
#define ASMX_NT 1
#define ASMX_SYNC() ((void)0)
template <class T>
static T asmx_cas(T* p, T c, T v)
{
    const T old = *p;
    if (old == c) *p = v;
    return old;
}
template <class T>
static T asmx_add(T* p, T v)
{
    const T old = *p;
    *p = T(old + v);
    return old;
}
#define ASMX_CAS(p, c, v) asmx_cas((p), (c), (v))
#define ASMX_MIN(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define ASMX_ADD(p, v) asmx_add((p), (v))
#define ASMX_OR(p, v) (*(p) |= (v))
#define ASMX_LOAD(p) (*(p))
#define ASMX_CLOCK() 0LL
#include "../../gatk-haplotypecaller-cpp17_amd/csrc/asm_graph_body.hpp"
#include "../../gatk-haplotypecaller-cpp17_amd/csrc/asm_paths.hpp"

namespace hcphmm {
void set_last_error(const std::string& msg) { std::fprintf(stderr, "error: %s\n", msg.c_str()); }
}
extern "C" int hcx_asm_paths_from_graph(const uint8_t*, int32_t, const hc_asm_edge*, int32_t, int32_t, int32_t,
                                        hc_asm_result**);

using namespace hcasm;

static std::vector<uint8_t> unhex(const std::string& s)
{
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(uint8_t(std::stoi(s.substr(i, 2), nullptr, 16)));
    return out;
}

static void put_hex(FILE* f, const uint8_t* p, size_t n)
{
    for (size_t i = 0; i < n; ++i) std::fprintf(f, "%02x", p[i]);
}

static void print_region(FILE* f, const RegionResult& r)
{
    std::fprintf(f, "R %d %d ", r.status, r.kmer_size);
    for (int t = 0; t < HC_ASM_MAX_ATTEMPTS; ++t) std::fprintf(f, "%d", r.attempts[t]);
    std::fprintf(f, " %zu %" PRId64 " %d %d %zu\n", r.haps.size(), r.n_paths, r.source, r.sink, r.edges.size());
    for (const hc_asm_edge& e : r.edges)
        std::fprintf(f, "E %d %d %d %d %d %d\n", e.from, e.to, e.count, e.seq, e.base, e.is_ref);
    for (const Hap& h : r.haps) {
        uint64_t bits;
        std::memcpy(&bits, &h.score, 8);
        std::fprintf(f, "H %016" PRIx64 " ", bits);
        put_hex(f, reinterpret_cast<const uint8_t*>(h.bases.data()), h.bases.size());
        std::fprintf(f, "\n");
    }
}

static int run_hook(const std::vector<uint8_t>& kmer, const std::vector<hc_asm_edge>& edges, int source, int sink,
                    FILE* f)
{
    hc_asm_result* res = nullptr;
    const int rc = hcx_asm_paths_from_graph(kmer.data(), int32_t(kmer.size()), edges.data(), int32_t(edges.size()),
                                            source, sink, &res);
    if (rc) return 2;
    print_region(f, res->regions[0]);
    hc_asm_result_free(res);
    return 0;
}

static int mode_graph(const char* in, const char* outp)
{
    std::ifstream is(in);
    int k, source, sink, n;
    std::string kmer;
    is >> k >> kmer >> source >> sink >> n;
    std::vector<hc_asm_edge> edges(static_cast<size_t>(n));
    for (auto& e : edges) {
        int base, is_ref;
        is >> e.from >> e.to >> e.count >> e.seq >> base >> is_ref;
        e.base = uint8_t(base);
        e.is_ref = uint8_t(is_ref);
        e.reserved = 0;
    }
    if (!is) return 3;
    FILE* f = std::fopen(outp, "w");
    const int rc = run_hook(unhex(kmer), edges, source, sink, f);
    std::fclose(f);
    return rc;
}

static int mode_bubbles(int n)
{
    // vertex 3b is the b-th joint; two branches 3b+1, 3b+2 lead to joint 3(b+1)
    std::vector<hc_asm_edge> edges;
    for (int b = 0; b < n; ++b)
        for (int br = 0; br < 2; ++br) {
            const int mid = 3 * b + 1 + br;
            edges.push_back(hc_asm_edge{3 * b, mid, 2 + br, int32_t(edges.size()), uint8_t("AC"[br]), 0, 0});
            edges.push_back(hc_asm_edge{mid, 3 * b + 3, 2 + br, int32_t(edges.size()), uint8_t('G'), 0, 0});
        }
    return run_hook(std::vector<uint8_t>(25, uint8_t('T')), edges, 0, 3 * n, stdout);
}

// asm_segments_kernel, lane by lane.
static void segments(const AsmSeq& s, const uint8_t* bases, const uint8_t* quals, int32_t* rem_pool, int32_t* seg_pool)
{
    int32_t* rem = rem_pool + s.off;
    int32_t* seg = seg_pool + s.off;
    if (s.is_ref) {
        for (int32_t i = 0; i < s.len; ++i) {
            rem[i] = s.len - i;
            seg[i] = s.rel;
        }
        return;
    }
    const uint8_t* b = bases + s.off;
    const uint8_t* q = quals + s.off;
    const int32_t n_chunks = (s.len + 63) / 64;
    auto ballot = [&](int32_t c) {
        unsigned long long m = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int32_t i = c * 64 + lane;
            if (i < s.len && asm_usable(b[i], q[i])) m |= 1ull << lane;
        }
        return m;
    };
    int32_t carry = 0;
    for (int32_t c = n_chunks - 1; c >= 0; --c) {
        const unsigned long long m = ballot(c);
        int32_t lane0 = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int32_t i = c * 64 + lane;
            const int32_t r = ((m >> lane) & 1) ? asm_run_right(m, lane, carry) : 0;
            if (i < s.len) rem[i] = r;
            if (lane == 0) lane0 = r;
        }
        carry = lane0;
    }
    carry = 0;
    for (int32_t c = 0; c < n_chunks; ++c) {
        const unsigned long long m = ballot(c);
        int32_t lane63 = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int32_t i = c * 64 + lane;
            const bool u = (m >> lane) & 1;
            const int32_t d = u ? asm_run_left(m, lane, carry) : 0;
            if (i < s.len) seg[i] = s.rel + i - (u ? d - 1 : 0);
            if (lane == 63) lane63 = d;
        }
        carry = lane63;
    }
}

// One region's input as the device sees it: the window then the reads in one pool.
struct EmulRegion {
    std::vector<uint8_t> bases, quals;
    std::vector<AsmSeq> seqs;
    AsmRegion rg{};
};

// A workgroup's slice of the workspace (AsmSlot), sized for a region.
struct EmulSlot {
    std::vector<uint32_t> id, h_rep, h_min;
    std::vector<int32_t> vert_of;
    std::vector<uint8_t> dup;
    std::vector<AsmVertex> vs;
    std::vector<AsmEdge> es;
    void grow(const AsmRegion& rg)
    {
        const size_t n = size_t(rg.n_bases), h = size_t(rg.hash_size), c = size_t(rg.cap);
        if (id.size() < n) id.resize(n), vert_of.resize(n), dup.resize(n);
        if (h_rep.size() < h) h_rep.resize(h), h_min.resize(h);
        if (vs.size() < c) vs.resize(c), es.resize(c);
    }
    AsmSlot slot() { return AsmSlot{id.data(), vert_of.data(), dup.data(), h_rep.data(), h_min.data(), vs.data(), es.data()}; }
};

static bool read_region(std::istream& is, EmulRegion& x)
{
    std::string ref_hex;
    int n_reads;
    is >> ref_hex >> n_reads;
    x.bases = unhex(ref_hex);
    const int32_t ref_len = int32_t(x.bases.size());
    x.quals.assign(x.bases.size(), 0);
    x.seqs.assign(1, AsmSeq{0, ref_len, 0, 1, 0});
    int64_t cap = std::max(0, ref_len - (kFirstK - 1));
    for (int j = 0; j < n_reads; ++j) {
        std::string bh, qh;
        is >> bh >> qh;
        const std::vector<uint8_t> b = unhex(bh), q = unhex(qh);
        if (b.size() != q.size()) return false;
        x.seqs.push_back(AsmSeq{int64_t(x.bases.size()), int32_t(b.size()), int32_t(x.bases.size()), 0, 0});
        x.bases.insert(x.bases.end(), b.begin(), b.end());
        x.quals.insert(x.quals.end(), q.begin(), q.end());
        cap += std::max<int64_t>(0, int64_t(b.size()) - (kFirstK - 1));
    }
    if (!is) return false;
    x.rg = AsmRegion{0, ref_len, int32_t(x.bases.size()), int32_t(std::max<int64_t>(cap, 1)), 64};
    while (x.rg.hash_size < 2 * x.rg.cap) x.rg.hash_size *= 2;
    return true;
}

static int run_region(int r, const EmulRegion& x, EmulSlot& ws, FILE* f)
{
    const AsmRegion& rg = x.rg;
    std::vector<int32_t> rem(x.bases.size()), seg(x.bases.size());
    for (const AsmSeq& s : x.seqs) segments(s, x.bases.data(), x.quals.data(), rem.data(), seg.data());
    const AsmSlot w = ws.slot();
    const int64_t pool_cap = std::min<int64_t>(rg.cap, HC_ASM_MAX_GRAPH_EDGES);
    std::vector<hc_asm_edge> pool(static_cast<size_t>(pool_cap));
    AsmOut o{};
    unsigned long long used = 0;
    int32_t err[2] = {0, 0};
    AsmArgs a{};
    a.regions = &rg;
    a.n_regions = 1;
    a.seqs = x.seqs.data();
    a.n_seqs = int32_t(x.seqs.size());
    a.bases = x.bases.data();
    a.quals = x.quals.data();
    a.rem = rem.data();
    a.seg_start = seg.data();
    a.out = &o;
    a.edge_pool = pool.data();
    a.edge_pool_cap = pool_cap;
    a.edge_pool_used = &used;
    a.err = err;
    AsmShared sh{};
    asm_region_graph(a, 0, w, &sh);
    if (err[0]) {
        std::fprintf(stderr, "region %d: device error word %d\n", r, err[0]);
        return 4;
    }
    RegionResult rr;
    std::memcpy(rr.attempts, o.attempts, sizeof(rr.attempts));
    if (o.kmer_size) {
        rr.kmer_size = o.kmer_size;
        rr.source = o.source;
        rr.sink = o.sink;
        const hc_asm_edge* e = pool.data() + o.edge_off;
        rr.edges.assign(e, e + o.n_edges);
        paths_from_graph(x.bases.data() + o.source_pos, o.kmer_size, rr.edges.data(), o.n_edges, o.source, o.sink, rr);
    }
    print_region(f, rr);
    return 0;
}

// one_slot: every region runs in the same slice, sized by the largest and never
// cleared in between, as a workgroup of asm_graph_kernel that handles several
// regions uses its slice. Otherwise every region gets exactly sized heap
// blocks of its own, so that the sanitizer sees every overrun.
static int mode_emul(const char* in, const char* outp, bool one_slot)
{
    std::ifstream is(in);
    int n;
    is >> n;
    std::vector<EmulRegion> regions(static_cast<size_t>(n));
    for (EmulRegion& x : regions)
        if (!read_region(is, x)) return 3;
    FILE* f = std::fopen(outp, "w");
    EmulSlot shared;
    if (one_slot)
        for (const EmulRegion& x : regions) shared.grow(x.rg);
    int rc = 0;
    for (int r = 0; r < n && rc == 0; ++r) {
        EmulSlot own;
        if (!one_slot) own.grow(regions[size_t(r)].rg);
        rc = run_region(r, regions[size_t(r)], one_slot ? shared : own, f);
    }
    std::fclose(f);
    return rc;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "graph" && argc == 4) return mode_graph(argv[2], argv[3]);
    if (mode == "bubbles" && argc == 3) return mode_bubbles(std::atoi(argv[2]));
    if (mode == "emul" && argc == 4) return mode_emul(argv[2], argv[3], false);
    if (mode == "emulslot" && argc == 4) return mode_emul(argv[2], argv[3], true);
    std::fprintf(stderr, "usage: asm_host_main graph|emul|emulslot <in> <out> | bubbles <n>\n");
    return 1;
}
