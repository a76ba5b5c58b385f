// Device side of the assembler (include/hc_asm.h): records shared by
// asm_kernels.hip, asm_graph_body.hpp and asm_engine.cpp.
//
// ASMX_HOST_ONLY: no HIP header and no launchers, for the single-threaded host
// build of asm_graph_body.hpp (tests/cpp/asm_host_main.cpp).
#pragma once
#ifdef ASMX_HOST_ONLY
#define ASMX_HD
#else
#include <hip/hip_runtime.h>
#define ASMX_HD __host__ __device__
#endif

#include <cstddef>
#include <cstdint>

#include "../../include/hc_asm.h"

namespace hcasm {

constexpr int kAsmThreads = 256;       // one workgroup per region
constexpr int kFirstK = 25, kStepK = 10;
constexpr int kMaxUnique = 2000;       // MAX_UNIQUE_KMERS_COUNT_TO_DISCARD
constexpr int kMinQual = 43;           // MIN_BASE_QUALITY_TO_USE, as a signed char
constexpr uint32_t kEmpty = 0xFFFFFFFFu;

// device error word: {code, region}
enum AsmError : int32_t {
    kErrNone = 0,
    kErrTableFull = 1,     // k-mer table: no free slot within its size
    kErrVertices = 2,      // more vertices than k-mer positions
    kErrEdges = 3,         // more edges than k-mer positions
    kErrOutEdges = 4,      // more than HC_ASM_MAX_GRAPH_EDGES on-path edges
    kErrPool = 5,          // the output pool's bound does not hold
};

// One sequence of the pool: a region's window (is_ref) or one read. `off` is
// the first byte in the base and quality pools, `rel` the same position
// relative to its region's first byte.
struct AsmSeq {
    int64_t off;
    int32_t len;
    int32_t rel;
    int32_t is_ref;
    int32_t pad;
};

// A region's bytes are contiguous in the pool: window, then the reads in order.
struct AsmRegion {
    int64_t off;        // first byte in the pools
    int32_t ref_len;
    int32_t n_bases;    // window + reads
    int32_t cap;        // bound on k-mer positions at k = 25: vertices and edges fit in it
    int32_t hash_size;  // power of two >= 2 * cap
};

struct AsmVertex {
    int32_t first, last;   // out-edge list in creation order (-1: none)
    int32_t indeg, pred;   // in-degree and the first in-edge (the only one while indeg == 1)
    int32_t outdeg;
    int32_t deg_f;         // in-degree over filtered edges, counted down by the peel
    uint32_t flags;        // kVRemoved | kVFwd | kVBwd
    int32_t pad;
};
constexpr uint32_t kVRemoved = 1u, kVFwd = 2u, kVBwd = 4u;

struct AsmEdge {   // index = creation sequence number
    int32_t from, to, count, next;
    uint8_t base, is_ref, pass, pad;
};

// What a region hands to the host.
struct AsmOut {
    int64_t edge_off;     // first record in the edge pool
    int32_t n_edges;      // on-path edges
    int32_t kmer_size;    // 0: no attempt accepted
    int32_t source, sink;
    int32_t source_pos;   // position of the source's k-mer in the window
    int32_t n_vertices, n_all_edges, n_unique;   // of the last attempt tried (statistics)
    uint8_t attempts[HC_ASM_MAX_ATTEMPTS];
    uint8_t pad[3];
    long long t_total, t_walk;   // wall clock ticks of the region and of its single-thread threading (HC_ASM_TRACE)
};

// One workgroup's tables (a slice of the global workspace, sized by the host
// from the largest region of the call).
struct AsmSlot {
    uint32_t* id;        // [n_bases] canonical position of the k-mer that starts here
    int32_t* vert_of;    // [n_bases] vertex of a non-duplicate k-mer, by canonical position
    uint8_t* dup;        // [n_bases] duplicate flag, by canonical position
    uint32_t* h_rep;     // [hash_size] a position holding the slot's k-mer
    uint32_t* h_min;     // [hash_size] the smallest such position
    AsmVertex* v;        // [cap]
    AsmEdge* e;          // [cap]
};

struct AsmArgs {
    const AsmRegion* regions;
    int32_t n_regions;
    const AsmSeq* seqs;
    int32_t n_seqs;
    const uint8_t* bases;
    const uint8_t* quals;
    int32_t* rem;        // per pool byte: usable bases from here to the end of the run (0: unusable)
    int32_t* seg_start;  // per pool byte: region-relative start of its run
    char* work;          // n_slots * slot_bytes
    size_t slot_bytes;
    int32_t max_bases, max_hash, max_cap;   // the slice layout
    AsmOut* out;
    hc_asm_edge* edge_pool;
    int64_t edge_pool_cap;
    unsigned long long* edge_pool_used;
    int32_t* err;        // {code, region}
};

// The slice layout, the same on both sides.
inline ASMX_HD size_t asm_up(size_t x) { return (x + 255) & ~size_t(255); }
inline ASMX_HD size_t asm_slot_bytes(int32_t max_bases, int32_t max_hash, int32_t max_cap)
{
    return asm_up(sizeof(uint32_t) * size_t(max_bases)) + asm_up(sizeof(int32_t) * size_t(max_bases)) +
           asm_up(size_t(max_bases)) + 2 * asm_up(sizeof(uint32_t) * size_t(max_hash)) +
           asm_up(sizeof(AsmVertex) * size_t(max_cap)) + asm_up(sizeof(AsmEdge) * size_t(max_cap));
}
inline ASMX_HD AsmSlot asm_carve(char* p, int32_t max_bases, int32_t max_hash, int32_t max_cap)
{
    AsmSlot s;
    s.id = reinterpret_cast<uint32_t*>(p);
    p += asm_up(sizeof(uint32_t) * size_t(max_bases));
    s.vert_of = reinterpret_cast<int32_t*>(p);
    p += asm_up(sizeof(int32_t) * size_t(max_bases));
    s.dup = reinterpret_cast<uint8_t*>(p);
    p += asm_up(size_t(max_bases));
    s.h_rep = reinterpret_cast<uint32_t*>(p);
    p += asm_up(sizeof(uint32_t) * size_t(max_hash));
    s.h_min = reinterpret_cast<uint32_t*>(p);
    p += asm_up(sizeof(uint32_t) * size_t(max_hash));
    s.v = reinterpret_cast<AsmVertex*>(p);
    p += asm_up(sizeof(AsmVertex) * size_t(max_cap));
    s.e = reinterpret_cast<AsmEdge*>(p);
    return s;
}

#ifndef ASMX_HOST_ONLY
hipError_t launch_asm_segments(const AsmArgs& a, hipStream_t st);
hipError_t launch_asm_graph(const AsmArgs& a, int n_slots, hipStream_t st);
#endif

}  // namespace hcasm
