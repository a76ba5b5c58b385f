// The assembler's graph for one region, all attempts: k-mer identity, duplicate
// marking, threading, filter, cycle test and on-path marking
// (graph_wrapper.hpp build / has_cycles / the reachability that equals
// mark_edges_on_paths on an acyclic graph).
//
// Written once against a small set of macros so that the same text is the body
// of asm_graph_kernel (one workgroup per region) and of a single-threaded host
// build that tests/cpp/asm_host_main.cpp checks under the host sanitizers:
//
//   ASMX_FN              function qualifier            (__device__ / nothing)
//   ASMX_TID, ASMX_NT    thread index and count        (threadIdx.x, blockDim.x / 0, 1)
//   ASMX_SYNC()          workgroup barrier             (__syncthreads() / nothing)
//   ASMX_CAS(p, c, v) ASMX_MIN(p, v) ASMX_ADD(p, v) ASMX_OR(p, v) ASMX_LOAD(p)
//   ASMX_CLOCK()         wall clock ticks              (wall_clock64() / 0)
//
// Every loop is bounded by the region's n_bases, cap or hash_size, all known
// to the host; a bound that does not hold goes to the error word.
#pragma once
#include "asm_kernels.hpp"

namespace hcasm {

// Block-shared scalars (LDS on the device).
struct AsmShared {
    int32_t unique, n_v, n_e, source, sink, removed, changed, err, total;
    long long out_base;
    int32_t scan[kAsmThreads];
};

// The per-lane arithmetic of asm_segments_kernel over one 64-base chunk: `m` has
// a bit per usable base of the chunk, the lane's own bit is set.
// Usable bases from the lane to the end of its run; `carry` is the value of the
// next chunk's first base, taken when the run reaches the chunk's end.
ASMX_FN inline int32_t asm_run_right(unsigned long long m, int lane, int32_t carry)
{
    const unsigned long long t = ~(m >> lane);
    const int32_t n = t ? int32_t(__builtin_ctzll(t)) : 64;
    return n + (lane + n == 64 ? carry : 0);
}
// Usable bases from the start of the run to the lane, itself included; `carry`
// is the value of the previous chunk's last base.
ASMX_FN inline int32_t asm_run_left(unsigned long long m, int lane, int32_t carry)
{
    const unsigned long long t = ~(m << (63 - lane));
    const int32_t n = t ? int32_t(__builtin_clzll(t)) : 64;
    return n + (n == lane + 1 ? carry : 0);
}

ASMX_FN inline bool asm_usable(uint8_t base, uint8_t qual)
{
    return base != uint8_t('N') && int(static_cast<signed char>(qual)) >= kMinQual;
}

ASMX_FN inline uint64_t asm_hash(const uint8_t* s, int k)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (int j = 0; j < k; ++j) h = (h ^ s[j]) * 0x100000001b3ull;
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 29;
    return h;
}

ASMX_FN inline bool asm_same(const uint8_t* a, const uint8_t* b, int k)
{
    for (int j = 0; j < k; ++j)
        if (a[j] != b[j]) return false;
    return true;
}

// get_vertex / create_vertex. Returns -1 when the vertex bound does not hold.
ASMX_FN inline int32_t asm_get_vertex(const AsmSlot& w, uint32_t canon, int32_t cap, int32_t& n_v)
{
    const bool is_dup = w.dup[canon] != 0;
    if (!is_dup && w.vert_of[canon] >= 0) return w.vert_of[canon];
    if (n_v >= cap) return -1;
    const int32_t v = n_v++;
    AsmVertex nv;
    nv.first = nv.last = nv.pred = -1;
    nv.indeg = nv.outdeg = nv.deg_f = 0;
    nv.flags = 0;
    nv.pad = 0;
    w.v[v] = nv;
    if (!is_dup) w.vert_of[canon] = v;
    return v;
}

// add_seq over every sequence of the region, by one thread. The precomputed
// ids make a step one list walk: no k-mer bytes are read here except the last.
ASMX_FN inline int32_t asm_thread_sequences(const AsmSlot& w, const AsmRegion& rg, const uint8_t* S, const int32_t* rem,
                                            const int32_t* seg_start, int k, AsmShared* sh)
{
    int32_t n_v = 0, n_e = 0, v = -1;
    const int32_t cap = rg.cap;
    for (int32_t i = 0; i < rg.n_bases; ++i) {
        if (rem[i] < k) continue;
        const bool is_ref = i < rg.ref_len;
        const uint32_t canon = w.id[i];
        if (seg_start[i] == i) {
            v = asm_get_vertex(w, canon, cap, n_v);
            if (v < 0) return kErrVertices;
            // increase_counts_backwards: while in_degree == 1, at most k - 1 steps. Its
            // byte check always holds: the predecessor's k-mer overlaps this one.
            int32_t u = v;
            for (int step = 0; step < k - 1 && w.v[u].indeg == 1; ++step) {
                AsmEdge& e = w.e[w.v[u].pred];
                ++e.count;
                u = e.from;
            }
            if (is_ref) sh->source = v;
        } else {
            // extend_chain
            const uint8_t b = S[i + k - 1];
            int32_t e = w.v[v].first, hit = -1;
            for (int32_t guard = 0; e >= 0 && guard <= n_e; ++guard) {
                if (w.e[e].base == b) {
                    hit = e;
                    break;
                }
                e = w.e[e].next;
            }
            if (hit >= 0) {
                ++w.e[hit].count;
                v = w.e[hit].to;
            } else {
                const int32_t t = asm_get_vertex(w, canon, cap, n_v);
                if (t < 0) return kErrVertices;
                if (n_e >= cap) return kErrEdges;
                const int32_t ne = n_e++;
                AsmEdge ed;
                ed.from = v;
                ed.to = t;
                ed.count = 1;
                ed.next = -1;
                ed.base = b;
                ed.is_ref = is_ref ? 1 : 0;
                ed.pass = 0;
                ed.pad = 0;
                w.e[ne] = ed;
                if (w.v[v].last >= 0)
                    w.e[w.v[v].last].next = ne;
                else
                    w.v[v].first = ne;
                w.v[v].last = ne;
                ++w.v[v].outdeg;
                if (w.v[t].indeg++ == 0) w.v[t].pred = ne;
                v = t;
            }
        }
        if (is_ref && i == rg.ref_len - k) sh->sink = v;
    }
    sh->n_v = n_v;
    sh->n_e = n_e;
    return kErrNone;
}

// One region. `S`, `rem`, `seg_start` point at the region's first pool byte.
ASMX_FN inline void asm_region_graph(const AsmArgs& a, int32_t region, const AsmSlot& w, AsmShared* sh)
{
    const AsmRegion rg = a.regions[region];
    const uint8_t* S = a.bases + rg.off;
    const int32_t* rem = a.rem + rg.off;
    const int32_t* seg_start = a.seg_start + rg.off;
    const int tid = ASMX_TID, nt = ASMX_NT;
    const int32_t L = rg.n_bases;
    const uint32_t hmask = uint32_t(rg.hash_size) - 1u;
    AsmOut* out = a.out + region;
    long long t_begin = 0, t_walk = 0;   // thread 0 only

    if (tid == 0) {
        t_begin = ASMX_CLOCK();
        AsmOut o;
        o.t_total = o.t_walk = 0;
        o.edge_off = 0;
        o.n_edges = 0;
        o.kmer_size = 0;
        o.source = o.sink = -1;
        o.source_pos = 0;
        o.n_vertices = o.n_all_edges = o.n_unique = 0;
        for (int t = 0; t < HC_ASM_MAX_ATTEMPTS; ++t) o.attempts[t] = HC_ASM_NOT_TRIED;
        o.pad[0] = o.pad[1] = o.pad[2] = 0;
        *out = o;
        sh->err = kErrNone;
    }
    ASMX_SYNC();

    for (int attempt = 0; attempt < HC_ASM_MAX_ATTEMPTS; ++attempt) {
        const int k = kFirstK + kStepK * attempt;
        if (rg.ref_len < k) {
            if (tid == 0) out->attempts[attempt] = HC_ASM_SHORT_REF;
            continue;
        }
        // ---- reset
        for (int32_t i = tid; i < L; i += nt) {
            w.dup[i] = 0;
            w.vert_of[i] = -1;
        }
        for (int32_t h = tid; h < rg.hash_size; h += nt) {
            w.h_rep[h] = kEmpty;
            w.h_min[h] = kEmpty;
        }
        if (tid == 0) {
            sh->unique = 0;
            sh->removed = 0;
            sh->n_v = sh->n_e = 0;
            sh->source = sh->sink = -1;
        }
        ASMX_SYNC();

        // ---- k-mer identity: the slot of each position's k-mer, bytes always compared
        for (int32_t i = tid; i < L; i += nt) {
            if (rem[i] < k) continue;
            uint32_t h = uint32_t(asm_hash(S + i, k)) & hmask;
            bool placed = false;
            for (int32_t probe = 0; probe < rg.hash_size; ++probe) {
                const uint32_t cur = ASMX_CAS(&w.h_rep[h], kEmpty, uint32_t(i));
                if (cur == kEmpty || cur == uint32_t(i) || asm_same(S + cur, S + i, k)) {
                    placed = true;
                    break;
                }
                h = (h + 1u) & hmask;
            }
            if (!placed) {
                sh->err = kErrTableFull;
                continue;
            }
            w.id[i] = h;
            ASMX_MIN(&w.h_min[h], uint32_t(i));
        }
        ASMX_SYNC();
        if (sh->err != kErrNone) break;
        // the canonical id: the smallest position that holds the k-mer
        for (int32_t i = tid; i < L; i += nt)
            if (rem[i] >= k) w.id[i] = w.h_min[w.id[i]];
        ASMX_SYNC();

        // ---- duplicates: the same id twice within one sequence
        for (int32_t i = tid; i < L; i += nt) {
            if (rem[i] < k) continue;
            const uint32_t c = w.id[i];
            for (int32_t j = seg_start[i]; j < i; ++j)
                if (w.id[j] == c) {
                    w.dup[c] = 1;
                    break;
                }
        }
        ASMX_SYNC();
        // unique_kmers.size(): the distinct non-duplicate k-mers
        {
            int32_t mine = 0;
            for (int32_t i = tid; i < L; i += nt)
                if (rem[i] >= k && w.id[i] == uint32_t(i) && !w.dup[i]) ++mine;
            if (mine) ASMX_ADD(&sh->unique, mine);
        }
        ASMX_SYNC();
        if (sh->unique > kMaxUnique) {
            if (tid == 0) {
                out->attempts[attempt] = HC_ASM_TOO_MANY_KMERS;
                out->n_unique = sh->unique;
            }
            ASMX_SYNC();
            continue;
        }

        // ---- threading: order dependent, one thread
        if (tid == 0) {
            const long long t0 = ASMX_CLOCK();
            const int32_t rc = asm_thread_sequences(w, rg, S, rem, seg_start, k, sh);
            if (rc != kErrNone) sh->err = rc;
            t_walk += ASMX_CLOCK() - t0;
        }
        ASMX_SYNC();
        if (sh->err != kErrNone) break;
        const int32_t n_v = sh->n_v, n_e = sh->n_e;

        // ---- edge filter, then the peel of zero in-degree vertices (Kahn)
        for (int32_t e = tid; e < n_e; e += nt) {
            AsmEdge& ed = w.e[e];
            const bool pass = ed.is_ref || ed.count >= 2 || w.v[ed.from].outdeg == 1;
            ed.pass = pass ? 1 : 0;
            if (pass) ASMX_ADD(&w.v[ed.to].deg_f, 1);
        }
        ASMX_SYNC();
        for (int32_t round = 0; round <= n_v; ++round) {
            if (tid == 0) sh->changed = 0;
            ASMX_SYNC();
            int32_t mine = 0;
            for (int32_t v = tid; v < n_v; v += nt) {
                AsmVertex& vx = w.v[v];
                if ((vx.flags & kVRemoved) || ASMX_LOAD(&vx.deg_f) != 0) continue;
                vx.flags |= kVRemoved;
                ++mine;
                int32_t e = vx.first;
                for (int32_t guard = 0; e >= 0 && guard <= n_e; ++guard) {
                    if (w.e[e].pass) ASMX_ADD(&w.v[w.e[e].to].deg_f, -1);
                    e = w.e[e].next;
                }
            }
            if (mine) {
                ASMX_ADD(&sh->removed, mine);
                sh->changed = 1;
            }
            ASMX_SYNC();
            if (!sh->changed) break;
            ASMX_SYNC();
        }
        if (sh->removed < n_v) {   // vertices remain: a cycle among filtered edges
            if (tid == 0) {
                out->attempts[attempt] = HC_ASM_CYCLE;
                out->n_vertices = n_v;
                out->n_all_edges = n_e;
                out->n_unique = sh->unique;
            }
            ASMX_SYNC();
            continue;
        }

        // ---- accepted. On-path edges: reachable from the source and reaching the sink.
        if (tid == 0) {
            w.v[sh->source].flags |= kVFwd;
            w.v[sh->sink].flags |= kVBwd;
        }
        ASMX_SYNC();
        for (int32_t round = 0; round <= n_v; ++round) {
            if (tid == 0) sh->changed = 0;
            ASMX_SYNC();
            bool any = false;
            for (int32_t e = tid; e < n_e; e += nt) {
                const AsmEdge ed = w.e[e];
                if (!ed.pass) continue;
                const uint32_t ff = ASMX_LOAD(&w.v[ed.from].flags), ft = ASMX_LOAD(&w.v[ed.to].flags);
                if ((ff & kVFwd) && !(ft & kVFwd)) {
                    ASMX_OR(&w.v[ed.to].flags, kVFwd);
                    any = true;
                }
                if ((ft & kVBwd) && !(ff & kVBwd)) {
                    ASMX_OR(&w.v[ed.from].flags, kVBwd);
                    any = true;
                }
            }
            if (any) sh->changed = 1;
            ASMX_SYNC();
            if (!sh->changed) break;
            ASMX_SYNC();
        }

        // ---- output: the on-path edges in creation order
        const int32_t chunk = (n_e + nt - 1) / nt;
        const int32_t lo = tid * chunk < n_e ? tid * chunk : n_e;
        const int32_t hi = lo + chunk < n_e ? lo + chunk : n_e;
        int32_t mine = 0;
        for (int32_t e = lo; e < hi; ++e) {
            const AsmEdge& ed = w.e[e];
            if (ed.pass && (w.v[ed.from].flags & kVFwd) && (w.v[ed.to].flags & kVBwd)) ++mine;
        }
        sh->scan[tid] = mine;
        ASMX_SYNC();
        if (tid == 0) {
            int32_t run = 0;
            for (int t = 0; t < nt; ++t) {
                const int32_t c = sh->scan[t];
                sh->scan[t] = run;
                run += c;
            }
            sh->total = run;
            sh->out_base = 0;
            if (run > HC_ASM_MAX_GRAPH_EDGES) {
                sh->err = kErrOutEdges;
            } else {
                const unsigned long long at = ASMX_ADD(a.edge_pool_used, (unsigned long long)run);
                if ((long long)(at + (unsigned long long)run) > a.edge_pool_cap)
                    sh->err = kErrPool;
                else
                    sh->out_base = (long long)at;
            }
        }
        ASMX_SYNC();
        if (sh->err != kErrNone) break;
        {
            hc_asm_edge* dst = a.edge_pool + sh->out_base + sh->scan[tid];
            for (int32_t e = lo; e < hi; ++e) {
                const AsmEdge& ed = w.e[e];
                if (!(ed.pass && (w.v[ed.from].flags & kVFwd) && (w.v[ed.to].flags & kVBwd))) continue;
                hc_asm_edge o;
                o.from = ed.from;
                o.to = ed.to;
                o.count = ed.count;
                o.seq = e;
                o.base = ed.base;
                o.is_ref = ed.is_ref;
                o.reserved = 0;
                *dst++ = o;
            }
        }
        if (tid == 0) {
            out->attempts[attempt] = HC_ASM_ACCEPTED;
            out->kmer_size = k;
            out->edge_off = sh->out_base;
            out->n_edges = sh->total;
            out->source = sh->source;
            out->sink = sh->sink;
            out->source_pos = 0;
            out->n_vertices = n_v;
            out->n_all_edges = n_e;
            out->n_unique = sh->unique;
        }
        break;
    }
    ASMX_SYNC();
    if (tid == 0) {
        out->t_walk = t_walk;
        out->t_total = ASMX_CLOCK() - t_begin;
        if (sh->err != kErrNone && ASMX_CAS(&a.err[0], int32_t(kErrNone), sh->err) == kErrNone) a.err[1] = region;
    }
    ASMX_SYNC();
}

}  // namespace hcasm
