// Driver around the REFERENCE's assembler: TEST INFRASTRUCTURE ONLY.
//
// Compiled by oracle/Makefile (target `ref`) into oracle/_ref/libref_asm.so,
// directly against the reference headers where they lie: assembler/assembler.hpp
// and assembler/graph_wrapper.hpp. No reference source is copied into this
// repository. The Boost.Graph headers graph_wrapper.hpp includes are answered
// by oracle/boost_standin/boost/graph/ (a vector-backed adjacency list and a
// coloured depth first search of our own, tested by
// tests/cpp/graph_standin_main.cpp); everything the assembler decides - dup
// k-mers, add_seq, increase_counts_backwards, the edge filter, path_finder, the
// scores, std::sort and the cut at 128 - is the reference's text.
//
// The haplotypes come from Assembler::assemble itself. The per-k outcomes and
// the accepted graph cannot be read off that call (the GraphWrapper is a local
// of a private member), so they come from a second pass, marked "restated
// orchestration" below, that calls GraphWrapper's own members in the sequence
// of assembler.hpp:22-53. The two passes must agree on the accepted k (taken
// from the line the reference prints) and on the number of paths; the driver
// abort()s if they do not.
//
// Private members are reached by compiling this one file with
// -fno-access-control, as ref_chain_driver.cpp is.
//
// C ABI: hcr_asm writes a little-endian blob (int64 / double / length-prefixed
// bytes) into a caller buffer and returns the number of bytes, or HCR_SMALL
// (-2) when the buffer is too small. A std::exception out of the reference is
// the blob's first word, not a return code.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <iostream>
#include <istream>
#include <iterator>
#include <limits>
#include <map>
#include <memory>
#include <numeric>
#include <ostream>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <string_view>
#include <tuple>
#include <utility>
#include <vector>
#include <immintrin.h>
#include <x86intrin.h>
#include <xmmintrin.h>
#include <stdio.h>
#include <string.h>
#include <omp.h>

#include "assembler/assembler.hpp"

namespace {

constexpr long HCR_SMALL = -2;
// the attempt codes of include/hc_asm.h
enum Outcome { NOT_TRIED = 0, SHORT_REF = 1, TOO_MANY_KMERS = 2, CYCLE = 3, ACCEPTED = 4 };

class Out {
public:
    Out(uint8_t* p, long cap) : p_(p), cap_(cap) {}
    void i64(int64_t v) { put(&v, 8); }
    void f64(double v) { put(&v, 8); }
    void str(std::string_view s) { i64(int64_t(s.size())); put(s.data(), long(s.size())); }
    long done() const { return n_ > cap_ ? HCR_SMALL : n_; }
private:
    void put(const void* src, long n)
    {
        if (n_ + n <= cap_) std::memcpy(p_ + n_, src, size_t(n));
        n_ += n;
    }
    uint8_t* p_;
    long cap_, n_ = 0;
};

// The reference prints its decisions to std::cout; they are kept here instead.
struct CoutCapture {
    std::ostringstream text;
    std::streambuf* old = std::cout.rdbuf(text.rdbuf());
    ~CoutCapture() { std::cout.rdbuf(old); }
};

[[noreturn]] void disagree(const char* what, long a, long b)
{
    std::fprintf(stderr, "ref_asm_driver: Assembler::assemble and the restated orchestration disagree on %s: %ld, %ld\n",
                 what, a, b);
    std::abort();
}

// The k of the last "Using kmer size of <k> in assembler" line, 0 when there is none.
long accepted_k_printed(const std::string& text)
{
    static const std::string key = "Using kmer size of ";
    const std::size_t at = text.rfind(key);
    return at == std::string::npos ? 0 : std::atol(text.c_str() + at + key.size());
}

}  // namespace

extern "C" {

// Assembler::assemble(reads, ref). Reads are bytes: read j is
// bases/quals[read_off[j] .. read_off[j] + read_len[j]). Blob:
//   threw (0/1); if it did, nothing more.
//   n haplotypes, then per haplotype in the reference's order: bases, score.
//   9 x (outcome, unique k-mer count (0 for SHORT_REF / NOT_TRIED)).
//   accepted k (0 when none), number of paths, source, sink, n edges, then per
//   edge in the order of boost::edges: from, to, the target k-mer's last byte,
//   count, is_ref, is_on_path, index in that order.
long hcr_asm(const char* ref, long ref_len, long n_reads, const int64_t* read_off, const int32_t* read_len,
             const uint8_t* bases, const uint8_t* quals, uint8_t* out, long cap)
{
    Out o(out, cap);
    CoutCapture printed;
    try {
        const std::string window(ref, size_t(ref_len));
        std::vector<hc::SAMRecord> reads(static_cast<size_t>(n_reads));
        for (long j = 0; j < n_reads; ++j) {
            reads[size_t(j)].SEQ.assign(reinterpret_cast<const char*>(bases) + read_off[j], size_t(read_len[j]));
            reads[size_t(j)].QUAL.assign(reinterpret_cast<const char*>(quals) + read_off[j], size_t(read_len[j]));
        }

        long n_haps = 0;
        {
            hc::Assembler assembler;
            const std::vector<hc::Haplotype> haps = assembler.assemble(reads, window);
            o.i64(0);
            o.i64(int64_t(haps.size()));
            for (const hc::Haplotype& h : haps) {
                o.str(h.bases);
                o.f64(h.score);
            }
            n_haps = long(haps.size());
        }
        const long k_printed = accepted_k_printed(printed.text.str());

        // RESTATED ORCHESTRATION of assembler.hpp:22-53 and :56-68: the loop over k,
        // the two refusals and their order. Every statement that builds or judges
        // the graph is a GraphWrapper member. find_paths (:52) is replaced by its
        // first two steps, which is all the graph's is_on_path needs.
        int64_t outcome[hc::Assembler::MAX_KMER_ITERATIONS_TO_ATTEMPT] = {}, count[hc::Assembler::MAX_KMER_ITERATIONS_TO_ATTEMPT] = {};
        std::size_t k = hc::Assembler::INITIAL_KMER_SIZE;
        std::unique_ptr<hc::GraphWrapper> accepted;
        for (std::size_t it = 0; it < hc::Assembler::MAX_KMER_ITERATIONS_TO_ATTEMPT && !accepted;
             ++it, k += hc::Assembler::KMER_SIZE_ITERATION_INCREASE) {
            if (window.size() < k) {
                outcome[it] = SHORT_REF;
                continue;
            }
            auto graph = std::make_unique<hc::GraphWrapper>(k);
            graph->set_ref(window);
            for (const auto& read : reads) graph->set_read(read);
            graph->build();
            count[it] = int64_t(graph->unique_kmers_count());
            if (graph->unique_kmers_count() > hc::Assembler::MAX_UNIQUE_KMERS_COUNT_TO_DISCARD) {
                outcome[it] = TOO_MANY_KMERS;
                continue;
            }
            if (graph->has_cycles()) {
                outcome[it] = CYCLE;
                continue;
            }
            outcome[it] = ACCEPTED;
            graph->find_all_paths();
            graph->mark_edges_on_paths();
            if (!graph->paths.empty()) accepted = std::move(graph);   // no path: no haplotype, the loop goes on
        }
        for (std::size_t it = 0; it < hc::Assembler::MAX_KMER_ITERATIONS_TO_ATTEMPT; ++it) {
            o.i64(outcome[it]);
            o.i64(count[it]);
        }
        const long k_here = accepted ? long(accepted->kmer_size) : 0;
        if (k_here != k_printed) disagree("the accepted k", k_printed, k_here);
        if (!accepted) {
            if (n_haps) disagree("the number of haplotypes", n_haps, 0);
            for (int z = 0; z < 5; ++z) o.i64(z == 2 || z == 3 ? -1 : 0);
            return o.done();
        }
        const long kept = long(std::min<std::size_t>(accepted->paths.size(), hc::GraphWrapper::DEFAULT_NUM_PATHS));
        if (kept != n_haps) disagree("the number of haplotypes", n_haps, kept);
        const auto& g = accepted->g;
        o.i64(k_here);
        o.i64(int64_t(accepted->paths.size()));
        o.i64(int64_t(accepted->source));
        o.i64(int64_t(accepted->sink));
        int64_t n_edges = 0;
        for (auto e : boost::make_iterator_range(boost::edges(g))) { (void)e; ++n_edges; }
        o.i64(n_edges);
        int64_t index = 0;
        for (auto e : boost::make_iterator_range(boost::edges(g))) {
            o.i64(int64_t(boost::source(e, g)));
            o.i64(int64_t(boost::target(e, g)));
            o.i64(int64_t(uint8_t(g[boost::target(e, g)].kmer.back())));
            o.i64(int64_t(g[e].count));
            o.i64(g[e].is_ref ? 1 : 0);
            o.i64(g[e].is_on_path ? 1 : 0);
            o.i64(index++);
        }
        return o.done();
    } catch (const std::exception&) {
        Out t(out, cap);
        t.i64(1);
        return t.done();
    }
}

}  // extern "C"
