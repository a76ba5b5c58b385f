// Stand-in for the Boost.Graph header of this name: TEST INFRASTRUCTURE ONLY
// (see adjacency_list.hpp beside it). Our own text: filtered_graph<G, F> is a
// view of a graph and an edge predicate; the predicate is a copy, the graph is
// not. Only depth_first_search (depth_first_search.hpp) walks it.
#pragma once
#include "adjacency_list.hpp"

namespace boost {

template <class G, class EdgePredicate>
struct filtered_graph {
    filtered_graph(const G& g, EdgePredicate p) : m_g(g), m_edge_pred(p) {}
    const G& m_g;
    EdgePredicate m_edge_pred;
};

}  // namespace boost
