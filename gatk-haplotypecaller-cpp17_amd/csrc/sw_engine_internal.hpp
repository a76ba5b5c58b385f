// What sw_engine.cpp shares with region_engine.cpp: the aligner's pair setup
// (scratch layout, launch order, kernel variant) and the launch of its two
// kernels on buffers the caller owns. One definition each, in sw_engine.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/hc_sw.h"
#include "sw_kernels.hpp"

namespace hcsw_host {

struct PairLayout {
    std::vector<int32_t> order;   // wave -> pair, longest first
    int64_t bt_total = 0;         // backtrack words
    int64_t el_total = 0;         // CIGAR element scratch: n1 + n2 + 3 per pair
    int n1max = 0, n2max = 0;
    int64_t cells = 0;
};

// pairs arrive with ref_off, alt_off, n1 and n2 set; el_off and bt_off are assigned here.
PairLayout layout_pairs(std::vector<hcsw::SwPair>& pairs);

// The kernel variant of a batch: 1 when the fast DP is proven exact for it.
int dp_variant(const hc_sw_params& params, int overhang, int n1max, int n2max);

struct DeviceBatch {
    int64_t n = 0;
    const hcsw::SwPair* pairs = nullptr;
    const int32_t* order = nullptr;
    const uint8_t* refs = nullptr;
    const uint8_t* alts = nullptr;
    hcsw::SwResult* res = nullptr;
    uint32_t* bt = nullptr;
    uint32_t* elems = nullptr;
    uint16_t* slots = nullptr;
    int32_t* n_elems = nullptr;
    int32_t* offsets = nullptr;
    hc_sw_params params{};
    int overhang = 0, shortcut = 1, fast = 0;
    int n1max = 0, n2max = 0;
};

// sw_dp_kernel then sw_trace_kernel on s. ev: nullptr, or three events recorded
// before, between and after the two launches.
hipError_t launch_batch(const DeviceBatch& b, hipStream_t s, hipEvent_t* ev);

}  // namespace hcsw_host
