// The nibble spread of a lane's match window (csrc/seg_spread.hpp) on its own,
// built with -fsanitize=address,undefined by tests/test_seg_spread_host.py.
// Reads 16-bit window chunks in hex from stdin, one per line, and prints each
// one's spread word; then one line per group with its byte offset in a wave's
// window and the slot offset of (code 4, lane 63), the last of the window.
#include <cstdint>
#include <cstdio>

#include "../../gatk-haplotypecaller-cpp17_amd/csrc/seg_spread.hpp"

int main()
{
    using namespace hcphmm::seg;
    unsigned h;
    while (std::scanf("%x", &h) == 1) std::printf("%08x\n", unsigned(spread_nibbles(uint32_t(h))));
    for (int g = 0; g < kSpreadGroups; ++g) std::printf("group %d %u\n", g, unsigned(spread_group_off(g)));
    std::printf("last %u of %d\n", unsigned(spread_slot_off(4, 63) + spread_group_off(kSpreadGroups - 1)), kSpreadWaveBytes);
    return 0;
}
