// The host half of the assembler (include/hc_asm.h): what a call returns, and
// the path enumeration over a reduced graph. No HIP in here: asm_paths.cpp
// compiles and runs without a device (tests/cpp/asm_paths_main.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/hc_asm.h"

namespace hcasm {

struct Hap {
    std::string bases;
    double score = 0.0;
};

struct RegionResult {
    int32_t status = HC_ASM_NO_HAPLOTYPES;
    int32_t kmer_size = 0;
    uint8_t attempts[HC_ASM_MAX_ATTEMPTS] = {};
    int64_t n_paths = 0;
    std::vector<Hap> haps;
    std::vector<hc_asm_edge> edges;   // kept with HC_ASM_WANT_GRAPH
    int32_t source = -1, sink = -1;
};

// path_finder .. get_haplotypes of graph_wrapper.hpp over `edges` (creation
// order = out-edge order): every source -> sink path depth first, the scores,
// the stable sort and the cut at HC_ASM_MAX_HAPS. Sets status, n_paths and
// haps of `out`; more than HC_ASM_MAX_PATHS paths: HC_ASM_TOO_COMPLEX, no haplotypes.
void paths_from_graph(const uint8_t* source_kmer, int32_t kmer_size, const hc_asm_edge* edges, int32_t n_edges,
                      int32_t source, int32_t sink, RegionResult& out);

}  // namespace hcasm

struct hc_asm_result {
    uint32_t flags = 0;
    std::vector<hcasm::RegionResult> regions;
};
