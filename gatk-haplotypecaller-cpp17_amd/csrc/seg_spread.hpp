// The spread form of a lane's match window (seg_common.hpp fill_window, quad
// waves): one byte per group of four columns, holding the group's four match
// bits at bits 7:4, the bits a quad table address takes them at. Plain C++ with
// no engine header, so tests/cpp/seg_spread_main.cpp builds it alone.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HC_SPREAD_FN __host__ __device__ inline
#else
#define HC_SPREAD_FN inline
#endif

namespace hcphmm {
namespace seg {

// Bytes of a lane's spread window per read code: 64 columns, four per byte.
constexpr int kSpreadGroups = 16;

// h: 16 window columns, MSB first (bit 15 the first column): four groups of
// four. Byte j of the result (bits 8j+7 .. 8j) is group j's pattern << 4, so
// stored little-endian the groups' bytes follow each other in column order.
HC_SPREAD_FN uint32_t spread_nibbles(uint32_t h)
{
    return ((h >> 8) & 0xf0u) | ((h << 4) & 0xf000u) | ((h << 16) & 0xf00000u) | (h << 28);
}

// Byte offset of group g of a (read code, lane) in a wave's spread window,
// laid out [code][g / 4][lane][g % 4]: the 64 lanes of a byte read of one
// group sit in 64 different dwords of one 256-byte line, whatever their codes,
// so the read has no bank conflict, and the group is an offset known at
// compile time from the lane's slot (code, lane).
HC_SPREAD_FN constexpr uint32_t spread_group_off(int g) { return uint32_t(g >> 2) * 256u + uint32_t(g & 3); }
HC_SPREAD_FN constexpr uint32_t spread_slot_off(int code, int lane) { return uint32_t(code) * 1024u + uint32_t(lane) * 4u; }
constexpr int kSpreadWaveBytes = 5 * 64 * kSpreadGroups;   // 5 120

}  // namespace seg
}  // namespace hcphmm
