// Stand-in for the Boost.Graph header of this name: TEST INFRASTRUCTURE ONLY
// (see adjacency_list.hpp beside it). Our own text: the coloured depth first
// search over a filtered_graph, iterative, with Boost's semantics as far as a
// visitor that overrides back_edge can tell:
//   * every white vertex is a root, in index order;
//   * out-edges are examined in list order, those the predicate refuses are
//     not seen at all;
//   * an edge to a white vertex is followed, an edge to a grey vertex (one on
//     the current stack, the vertex itself included) is a back edge, an edge
//     to a black vertex is neither.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

#include "adjacency_list.hpp"
#include "filtered_graph.hpp"

namespace boost {

struct null_visitor {};

template <class Visitors = null_visitor>
struct dfs_visitor {
    template <class E, class G>
    void back_edge(E, G&) {}
};

// visitor(vis): the named parameter depth_first_search takes.
template <class Vis>
struct dfs_params {
    Vis m_vis;
};
template <class Vis>
dfs_params<Vis> visitor(const Vis& vis)
{
    return dfs_params<Vis>{vis};
}

template <class G, class P, class Vis>
void depth_first_search(const filtered_graph<G, P>& fg, dfs_params<Vis> params)
{
    enum : unsigned char { white, grey, black };
    const G& g = fg.m_g;
    const std::size_t n = num_vertices(g);
    std::vector<unsigned char> colour(n, white);
    std::vector<std::pair<std::size_t, std::size_t>> stack;   // (vertex, next out-edge)
    for (std::size_t root = 0; root < n; ++root) {
        if (colour[root] != white) continue;
        colour[root] = grey;
        stack.emplace_back(root, 0);
        while (!stack.empty()) {
            const std::size_t u = stack.back().first;
            const auto& out = g.m_out[u];
            bool descended = false;
            while (stack.back().second < out.size()) {
                const edge_desc e = out[stack.back().second++];
                if (!fg.m_edge_pred(e)) continue;
                const std::size_t v = e.m_target;
                if (colour[v] == white) {
                    colour[v] = grey;
                    stack.emplace_back(v, 0);
                    descended = true;
                    break;
                }
                if (colour[v] == grey) params.m_vis.back_edge(e, fg);
            }
            if (descended) continue;
            colour[u] = black;
            stack.pop_back();
        }
    }
}

}  // namespace boost
