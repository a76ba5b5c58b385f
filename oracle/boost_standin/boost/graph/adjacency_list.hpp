// Stand-in for the Boost.Graph header of this name: TEST INFRASTRUCTURE ONLY,
// on the include path of oracle/ref_asm_driver.cpp (and of
// tests/cpp/graph_standin_main.cpp, which tests it). Our own text: a
// vector-backed adjacency list that answers what the reference's
// assembler/graph_wrapper.hpp asks of adjacency_list<vecS, vecS,
// bidirectionalS, VP, EP>, with the semantics that Boost's has and that the
// assembler's result depends on:
//   * vertex descriptors are indices, in the order of add_vertex;
//   * out_edges(u) and in_edges(v) are in the order of add_edge, parallel
//     edges allowed, add_edge always succeeds;
//   * edge(u, v, g) is the first out-edge of u whose target is v;
//   * edges(g) is in the order of add_edge.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace boost {

struct vecS {};
struct bidirectionalS {};

// An edge descriptor. In namespace boost itself, so that an unqualified
// target(e, g) finds boost::target by argument-dependent lookup.
struct edge_desc {
    std::size_t m_source = 0, m_target = 0, m_index = 0;
    bool operator==(const edge_desc& o) const { return m_index == o.m_index; }
    bool operator!=(const edge_desc& o) const { return m_index != o.m_index; }
};

template <class It>
struct iterator_range {
    It m_begin, m_end;
    It begin() const { return m_begin; }
    It end() const { return m_end; }
};
template <class It>
iterator_range<It> make_iterator_range(const std::pair<It, It>& p)
{
    return iterator_range<It>{p.first, p.second};
}

// vertices(g): the numbers 0 .. n - 1.
struct counting_iterator {
    std::size_t at;
    std::size_t operator*() const { return at; }
    counting_iterator& operator++()
    {
        ++at;
        return *this;
    }
    bool operator==(const counting_iterator& o) const { return at == o.at; }
    bool operator!=(const counting_iterator& o) const { return at != o.at; }
};

template <class OutEdgeList, class VertexList, class Directed, class VP, class EP>
class adjacency_list {
public:
    using vertex_descriptor = std::size_t;
    using edge_descriptor = edge_desc;
    using edge_iterator = std::vector<edge_desc>::const_iterator;
    using out_edge_iterator = edge_iterator;
    using in_edge_iterator = edge_iterator;
    using vertex_iterator = counting_iterator;

    VP& operator[](vertex_descriptor v) { return m_vp[v]; }
    const VP& operator[](vertex_descriptor v) const { return m_vp[v]; }
    EP& operator[](const edge_desc& e) { return m_ep[e.m_index]; }
    const EP& operator[](const edge_desc& e) const { return m_ep[e.m_index]; }

    std::vector<VP> m_vp;
    std::vector<EP> m_ep;
    std::vector<edge_desc> m_edges;
    std::vector<std::vector<edge_desc>> m_out, m_in;
};

template <class G>
struct graph_traits {
    using vertex_descriptor = typename G::vertex_descriptor;
    using edge_descriptor = typename G::edge_descriptor;
    using out_edge_iterator = typename G::out_edge_iterator;
    using in_edge_iterator = typename G::in_edge_iterator;
    using edge_iterator = typename G::edge_iterator;
    using vertex_iterator = typename G::vertex_iterator;
};

#define HC_STANDIN_GRAPH template <class O, class V, class D, class VP, class EP>
#define HC_STANDIN_LIST adjacency_list<O, V, D, VP, EP>

HC_STANDIN_GRAPH std::size_t add_vertex(HC_STANDIN_LIST& g)
{
    g.m_vp.emplace_back();
    g.m_out.emplace_back();
    g.m_in.emplace_back();
    return g.m_vp.size() - 1;
}

HC_STANDIN_GRAPH std::pair<edge_desc, bool> add_edge(std::size_t u, std::size_t v, HC_STANDIN_LIST& g)
{
    const edge_desc e{u, v, g.m_edges.size()};
    g.m_ep.emplace_back();
    g.m_edges.push_back(e);
    g.m_out[u].push_back(e);
    g.m_in[v].push_back(e);
    return {e, true};
}

HC_STANDIN_GRAPH std::size_t num_vertices(const HC_STANDIN_LIST& g) { return g.m_vp.size(); }
HC_STANDIN_GRAPH std::size_t out_degree(std::size_t v, const HC_STANDIN_LIST& g) { return g.m_out[v].size(); }
HC_STANDIN_GRAPH std::size_t in_degree(std::size_t v, const HC_STANDIN_LIST& g) { return g.m_in[v].size(); }

HC_STANDIN_GRAPH auto out_edges(std::size_t v, const HC_STANDIN_LIST& g)
{
    return std::make_pair(g.m_out[v].cbegin(), g.m_out[v].cend());
}
HC_STANDIN_GRAPH auto in_edges(std::size_t v, const HC_STANDIN_LIST& g)
{
    return std::make_pair(g.m_in[v].cbegin(), g.m_in[v].cend());
}
HC_STANDIN_GRAPH auto edges(const HC_STANDIN_LIST& g) { return std::make_pair(g.m_edges.cbegin(), g.m_edges.cend()); }
HC_STANDIN_GRAPH auto vertices(const HC_STANDIN_LIST& g)
{
    return std::make_pair(counting_iterator{0}, counting_iterator{g.m_vp.size()});
}

template <class G>
std::size_t source(const edge_desc& e, const G&)
{
    return e.m_source;
}
template <class G>
std::size_t target(const edge_desc& e, const G&)
{
    return e.m_target;
}

HC_STANDIN_GRAPH std::pair<edge_desc, bool> edge(std::size_t u, std::size_t v, const HC_STANDIN_LIST& g)
{
    for (const edge_desc& e : g.m_out[u])
        if (e.m_target == v) return {e, true};
    return {edge_desc{}, false};
}

#undef HC_STANDIN_GRAPH
#undef HC_STANDIN_LIST

}  // namespace boost
