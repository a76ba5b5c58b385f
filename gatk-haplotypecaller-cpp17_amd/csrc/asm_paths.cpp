// Paths, scores and haplotype bytes of the assembler, on the host
// (graph_wrapper.hpp:142-230), and the accessors of hc_asm_result.
//
// The device hands over the on-path edges of the accepted attempt in creation
// order. log10 is glibc's here for the reason hc_phmm_collect keeps it on the
// host: nothing on the device reproduces its bits.
#include "asm_paths.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <numeric>

namespace hcphmm {
void set_last_error(const std::string& msg);
}

namespace hcasm {
namespace {

struct Walker {
    // compact vertices, CSR out-edges in creation order
    std::vector<int32_t> ids, first, adj, to;
    int32_t src = 0, snk = 0;
    // the walk's state
    std::vector<int32_t> vstack, estack, cursor;
    std::vector<uint8_t> on_stack;

    int32_t vertex(int32_t id) const { return int32_t(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin()); }

    Walker(const hc_asm_edge* edges, int32_t n, int32_t source, int32_t sink)
    {
        ids.reserve(size_t(n) * 2 + 2);
        for (int32_t e = 0; e < n; ++e) {
            ids.push_back(edges[e].from);
            ids.push_back(edges[e].to);
        }
        ids.push_back(source);
        ids.push_back(sink);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        const size_t nv = ids.size();
        first.assign(nv + 1, 0);
        to.resize(size_t(n));
        std::vector<int32_t> from(static_cast<size_t>(n));
        for (int32_t e = 0; e < n; ++e) {
            from[size_t(e)] = vertex(edges[e].from);
            to[size_t(e)] = vertex(edges[e].to);
            ++first[size_t(from[size_t(e)]) + 1];
        }
        for (size_t v = 0; v < nv; ++v) first[v + 1] += first[v];
        adj.resize(size_t(n));
        std::vector<int32_t> fill(first.begin(), first.end() - 1);
        for (int32_t e = 0; e < n; ++e) adj[size_t(fill[size_t(from[size_t(e)])]++)] = e;
        src = vertex(source);
        snk = vertex(sink);
        on_stack.assign(nv, 0);
    }

    // path_finder: calls found() with estack = the path's edges at every arrival
    // at the sink, push(e) / pop() around every edge taken. found() returning
    // false ends the walk. Returns false when ended that way or when `budget`
    // steps were not enough.
    template <class Found, class Push, class Pop>
    bool walk(int64_t budget, Found&& found, Push&& push, Pop&& pop)
    {
        vstack.assign(1, src);
        estack.clear();
        cursor.assign(1, first[size_t(src)]);
        std::fill(on_stack.begin(), on_stack.end(), uint8_t(0));
        on_stack[size_t(src)] = 1;
        while (!vstack.empty()) {
            const int32_t v = vstack.back();
            bool descended = false;
            if (v == snk) {
                if (!found()) return false;   // a path ends at its first arrival
            } else {
                while (cursor.back() < first[size_t(v) + 1]) {
                    const int32_t e = adj[size_t(cursor.back()++)];
                    const int32_t w = to[size_t(e)];
                    if (on_stack[size_t(w)]) continue;   // std::find(path.begin(), path.end(), v)
                    if (--budget < 0) return false;
                    vstack.push_back(w);
                    estack.push_back(e);
                    cursor.push_back(first[size_t(w)]);
                    on_stack[size_t(w)] = 1;
                    push(e);
                    descended = true;
                    break;
                }
            }
            if (descended) continue;
            on_stack[size_t(v)] = 0;
            vstack.pop_back();
            cursor.pop_back();
            if (!estack.empty()) {
                estack.pop_back();
                pop();
            }
        }
        return true;
    }
};

}  // namespace

void paths_from_graph(const uint8_t* source_kmer, int32_t kmer_size, const hc_asm_edge* edges, int32_t n_edges,
                      int32_t source, int32_t sink, RegionResult& out)
{
    out.haps.clear();
    Walker w(edges, n_edges, source, sink);
    const size_t ne = size_t(n_edges);
    const int64_t budget = (int64_t(HC_ASM_MAX_PATHS) + 1) * int64_t(w.ids.size() + 1);

    // 1: count the paths, mark the edges some path uses (mark_edges_on_paths)
    std::vector<uint8_t> on_path(ne, 0);
    int64_t n_paths = 0;
    size_t marked = 0;   // estack[0 .. marked) is marked already
    const bool done = w.walk(
        budget,
        [&] {
            if (++n_paths > HC_ASM_MAX_PATHS) return false;
            for (size_t d = marked; d < w.estack.size(); ++d) on_path[size_t(w.estack[d])] = 1;
            marked = w.estack.size();
            return true;
        },
        [](int32_t) {}, [&] { marked = std::min(marked, w.estack.size()); });
    if (!done) {
        out.status = HC_ASM_TOO_COMPLEX;
        out.n_paths = int64_t(HC_ASM_MAX_PATHS) + 1;
        return;
    }
    out.n_paths = n_paths;
    if (n_paths == 0) {
        out.status = HC_ASM_NO_HAPLOTYPES;
        return;
    }

    // compute_edges_score: per vertex, over its on-path out-edges in order
    std::vector<double> score(ne, 0.0);
    for (size_t v = 0; v + 1 < w.first.size(); ++v) {
        double sum = 0;
        for (int32_t a = w.first[v]; a < w.first[v + 1]; ++a) {
            const int32_t e = w.adj[size_t(a)];
            if (on_path[size_t(e)]) sum += double(size_t(edges[e].count));
        }
        for (int32_t a = w.first[v]; a < w.first[v + 1]; ++a) {
            const int32_t e = w.adj[size_t(a)];
            if (on_path[size_t(e)]) score[size_t(e)] = std::log10(double(size_t(edges[e].count)) / sum);
        }
    }

    // 2: every path's score, summed in path order from 0.0
    std::vector<double> path_score;
    path_score.reserve(size_t(n_paths));
    std::vector<double> prefix(1, 0.0);
    w.walk(
        budget,
        [&] {
            path_score.push_back(prefix.back());
            return true;
        },
        [&](int32_t e) { prefix.push_back(prefix.back() + score[size_t(e)]); }, [&] { prefix.pop_back(); });

    // std::sort by score descending over the paths in discovery order, as
    // graph_wrapper.hpp:220 sorts its haplotypes; the first HC_ASM_MAX_HAPS stay.
    // Not a stable sort: where scores are equal, std::sort's permutation is a
    // function of the comparison results alone, so with the same C++ library it
    // is the reference's, element type regardless.
    std::vector<int32_t> order(path_score.size());
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(),
              [&](int32_t a, int32_t b) { return path_score[size_t(a)] > path_score[size_t(b)]; });
    if (order.size() > size_t(HC_ASM_MAX_HAPS)) order.resize(size_t(HC_ASM_MAX_HAPS));
    std::vector<int32_t> rank(path_score.size(), -1);
    for (size_t r = 0; r < order.size(); ++r) rank[size_t(order[r])] = int32_t(r);

    // 3: the bytes of the paths that stay
    out.haps.resize(order.size());
    std::string seq(reinterpret_cast<const char*>(source_kmer), size_t(kmer_size));
    int64_t at = 0;
    w.walk(
        budget,
        [&] {
            const int32_t r = rank[size_t(at)];
            if (r >= 0) {
                out.haps[size_t(r)].bases = seq;
                out.haps[size_t(r)].score = path_score[size_t(at)];
            }
            ++at;
            return true;
        },
        [&](int32_t e) { seq.push_back(char(edges[e].base)); }, [&] { seq.pop_back(); });
    out.status = HC_ASM_OK;
}

}  // namespace hcasm

namespace {

int fail(const std::string& msg)
{
    hcphmm::set_last_error(msg);
    return HC_PHMM_EINVAL;
}

bool region_ok(const hc_asm_result* r, int32_t region)
{
    return r && region >= 0 && size_t(region) < r->regions.size();
}

}  // namespace

extern "C" {

int hc_asm_result_region(const hc_asm_result* res, int32_t region, int32_t* status, int32_t* kmer_size,
                         const uint8_t** attempts, int32_t* n_haps, int64_t* n_paths)
{
    if (!region_ok(res, region)) return fail("hc_asm_result_region: null result or region out of range");
    const hcasm::RegionResult& r = res->regions[size_t(region)];
    if (status) *status = r.status;
    if (kmer_size) *kmer_size = r.kmer_size;
    if (attempts) *attempts = r.attempts;
    if (n_haps) *n_haps = int32_t(r.haps.size());
    if (n_paths) *n_paths = r.n_paths;
    return HC_PHMM_OK;
}

int hc_asm_result_hap(const hc_asm_result* res, int32_t region, int32_t hap, const uint8_t** bases, int32_t* length,
                      double* score)
{
    if (!region_ok(res, region)) return fail("hc_asm_result_hap: null result or region out of range");
    const hcasm::RegionResult& r = res->regions[size_t(region)];
    if (hap < 0 || size_t(hap) >= r.haps.size()) return fail("hc_asm_result_hap: haplotype out of range");
    const hcasm::Hap& h = r.haps[size_t(hap)];
    if (bases) *bases = reinterpret_cast<const uint8_t*>(h.bases.data());
    if (length) *length = int32_t(h.bases.size());
    if (score) *score = h.score;
    return HC_PHMM_OK;
}

int hc_asm_result_graph(const hc_asm_result* res, int32_t region, const hc_asm_edge** edges, int32_t* n_edges,
                        int32_t* source, int32_t* sink)
{
    if (!region_ok(res, region)) return fail("hc_asm_result_graph: null result or region out of range");
    if (!(res->flags & HC_ASM_WANT_GRAPH)) return fail("hc_asm_result_graph: the call did not ask for HC_ASM_WANT_GRAPH");
    const hcasm::RegionResult& r = res->regions[size_t(region)];
    if (edges) *edges = r.edges.data();
    if (n_edges) *n_edges = int32_t(r.edges.size());
    if (source) *source = r.source;
    if (sink) *sink = r.sink;
    return HC_PHMM_OK;
}

int hc_asm_result_free(hc_asm_result* res)
{
    delete res;
    return HC_PHMM_OK;
}

// Test hook: the host half alone. A reduced graph in, a one-region result out
// (accessors as after hc_asm_assemble; the graph is kept).
int hcx_asm_paths_from_graph(const uint8_t* source_kmer, int32_t kmer_size, const hc_asm_edge* edges, int32_t n_edges,
                             int32_t source, int32_t sink, hc_asm_result** out)
{
    if (!out) return fail("hcx_asm_paths_from_graph: null out");
    *out = nullptr;
    if (!source_kmer || kmer_size < 1 || n_edges < 0 || (n_edges && !edges))
        return fail("hcx_asm_paths_from_graph: null pointer, kmer_size < 1 or negative edge count");
    try {
        std::unique_ptr<hc_asm_result> res(new hc_asm_result());
        res->flags = HC_ASM_WANT_GRAPH;
        res->regions.resize(1);
        hcasm::RegionResult& r = res->regions[0];
        r.kmer_size = kmer_size;
        r.source = source;
        r.sink = sink;
        r.edges.assign(edges, edges + n_edges);
        hcasm::paths_from_graph(source_kmer, kmer_size, edges, n_edges, source, sink, r);
        *out = res.release();
    } catch (const std::bad_alloc&) {
        hcphmm::set_last_error("hcx_asm_paths_from_graph: host allocation failed");
        return HC_PHMM_ENOMEM;
    }
    return HC_PHMM_OK;
}

}  // extern "C"
