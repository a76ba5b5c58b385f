// Stand-alone test of oracle/boost_standin/boost/graph/: the container and the
// depth first search that stand in for Boost.Graph under the reference's
// assembler (oracle/ref_asm_driver.cpp). Built with
// -fsanitize=address,undefined by tests/test_asm_ref_pins.py. No GPU, no Python,
// nothing of the reference. Exit status 0 and "ok" when every check holds.
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include <boost/graph/adjacency_list.hpp>
#include <boost/graph/depth_first_search.hpp>
#include <boost/graph/filtered_graph.hpp>

struct VP {
    std::string name;
};
struct EP {
    int count = 0;
    bool keep = true;
};
using Graph = boost::adjacency_list<boost::vecS, boost::vecS, boost::bidirectionalS, VP, EP>;
using Vertex = boost::graph_traits<Graph>::vertex_descriptor;
using Edge = boost::graph_traits<Graph>::edge_descriptor;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);      \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct back_edges : public boost::dfs_visitor<> {
    explicit back_edges(std::vector<std::pair<Vertex, Vertex>>& seen) : seen(seen) {}
    template <class E, class G>
    void back_edge(E e, G& g)
    {
        (void)g;
        seen.emplace_back(e.m_source, e.m_target);
    }
    std::vector<std::pair<Vertex, Vertex>>& seen;
};

struct KeepFilter {
    bool operator()(Edge e) const { return (*g)[e].keep; }
    const Graph* g;
};

static std::vector<std::pair<Vertex, Vertex>> search(const Graph& g)
{
    std::vector<std::pair<Vertex, Vertex>> seen;
    back_edges vis(seen);
    boost::filtered_graph<Graph, KeepFilter> fg(g, KeepFilter{&g});
    boost::depth_first_search(fg, boost::visitor(vis));
    return seen;
}

static Graph with_vertices(int n)
{
    Graph g;
    for (int i = 0; i < n; ++i) {
        const Vertex v = boost::add_vertex(g);
        CHECK(v == Vertex(i));
        g[v].name = "v" + std::to_string(i);
    }
    return g;
}

static void lists_and_degrees()
{
    Graph g = with_vertices(4);
    const Vertex order[][2] = {{0, 2}, {0, 1}, {3, 1}, {0, 2}, {2, 1}, {1, 1}};
    int n = 0;
    for (const auto& uv : order) {
        auto [e, added] = boost::add_edge(uv[0], uv[1], g);
        CHECK(added);
        CHECK(boost::source(e, g) == uv[0] && target(e, g) == uv[1]);   // target by ADL, as the reference calls it
        g[e].count = ++n;
    }
    CHECK(g[Vertex(2)].name == "v2");
    CHECK(boost::out_degree(0, g) == 3 && boost::in_degree(0, g) == 0);
    CHECK(boost::out_degree(1, g) == 1 && boost::in_degree(1, g) == 4);   // the loop counts on both sides
    CHECK(boost::out_degree(3, g) == 1 && boost::in_degree(2, g) == 2);
    std::vector<int> out0, in1, all;
    for (auto e : boost::make_iterator_range(boost::out_edges(0, g))) out0.push_back(g[e].count);
    for (auto e : boost::make_iterator_range(boost::in_edges(1, g))) in1.push_back(g[e].count);
    for (auto e : boost::make_iterator_range(boost::edges(g))) all.push_back(g[e].count);
    CHECK((out0 == std::vector<int>{1, 2, 4}));       // insertion order, the parallel edge kept
    CHECK((in1 == std::vector<int>{2, 3, 5, 6}));
    CHECK((all == std::vector<int>{1, 2, 3, 4, 5, 6}));
    std::vector<Vertex> vs;
    for (auto v : boost::make_iterator_range(boost::vertices(g))) vs.push_back(v);
    CHECK((vs == std::vector<Vertex>{0, 1, 2, 3}));
    // edge(u, v): the first of the parallel edges, and "none" where there is none
    auto [first, found] = boost::edge(0, 2, g);
    CHECK(found && g[first].count == 1);
    CHECK(!boost::edge(2, 0, g).second && !boost::edge(3, 3, g).second);
    CHECK(boost::edge(1, 1, g).second);
    const Graph& cg = g;
    CHECK(cg[boost::edge(2, 1, cg).first].count == 5);
}

static void searches()
{
    {   // a DAG with a cross edge and a forward edge: no back edge
        Graph g = with_vertices(5);
        for (auto uv : {std::pair<int, int>{0, 1}, {0, 2}, {1, 3}, {2, 3}, {0, 3}, {4, 0}}) boost::add_edge(uv.first, uv.second, g);
        CHECK(search(g).empty());
    }
    {   // a cycle: exactly the edge to the grey vertex
        Graph g = with_vertices(4);
        for (auto uv : {std::pair<int, int>{0, 1}, {1, 2}, {2, 3}, {3, 1}}) boost::add_edge(uv.first, uv.second, g);
        const auto seen = search(g);
        CHECK(seen.size() == 1 && seen[0] == (std::pair<Vertex, Vertex>{3, 1}));
    }
    {   // a loop is a back edge
        Graph g = with_vertices(2);
        boost::add_edge(0, 1, g);
        boost::add_edge(1, 1, g);
        CHECK(search(g).size() == 1);
    }
    {   // a cycle in a component that vertex 0 does not reach: every white vertex is a root
        Graph g = with_vertices(6);
        for (auto uv : {std::pair<int, int>{0, 1}, {1, 2}, {3, 4}, {4, 5}, {5, 3}}) boost::add_edge(uv.first, uv.second, g);
        const auto seen = search(g);
        CHECK(seen.size() == 1 && seen[0] == (std::pair<Vertex, Vertex>{5, 3}));
    }
    {   // roots in index order: from 0 the edge 2 -> 0 is a back edge; were 2 the first root, 1 -> 2 would be
        Graph g = with_vertices(3);
        for (auto uv : {std::pair<int, int>{2, 0}, {0, 1}, {1, 2}}) boost::add_edge(uv.first, uv.second, g);
        const auto seen = search(g);
        CHECK(seen.size() == 1 && seen[0] == (std::pair<Vertex, Vertex>{2, 0}));
    }
    {   // a cycle closed only by an edge the filter refuses: none; with the edge let through: one
        Graph g = with_vertices(4);
        for (auto uv : {std::pair<int, int>{0, 1}, {1, 2}, {2, 3}}) boost::add_edge(uv.first, uv.second, g);
        const Edge closing = boost::add_edge(3, 0, g).first;
        g[closing].keep = false;
        CHECK(search(g).empty());
        g[closing].keep = true;
        CHECK(search(g).size() == 1);
        // a refused edge does not make its target visited either: 1 stays a root of its own
        g[boost::edge(0, 1, g).first].keep = false;
        g[closing].keep = true;
        CHECK(search(g).empty());
    }
    {   // deep: iterative, no recursion to overflow
        const int n = 200000;
        Graph g = with_vertices(n);
        for (int i = 0; i + 1 < n; ++i) boost::add_edge(Vertex(i), Vertex(i + 1), g);
        CHECK(search(g).empty());
        boost::add_edge(Vertex(n - 1), Vertex(n / 2), g);
        CHECK(search(g).size() == 1);
    }
}

int main()
{
    lists_and_degrees();
    searches();
    if (failures) {
        std::fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
