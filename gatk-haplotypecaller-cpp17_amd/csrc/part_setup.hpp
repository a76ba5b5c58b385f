// What the host planner (planner.cpp) and the flat planner (flat_plan.cpp) set
// up alike for a part: the bump allocator of its one device allocation, the
// packed-row pad and pool limits, the results block with the rescue pass's
// scratch, and the streams and events it runs on. What differs between the two
// (when slot memory is reserved, d_slot_of, the flat device passes' buffers)
// stays with each.
#pragma once
#include <algorithm>

#include "engine_core.hpp"

namespace hcphmm {
namespace eng {

// Bump allocator over one region: 256-B aligned segments.
struct Layout {
    size_t off = 0;
    size_t take(size_t bytes)
    {
        const size_t o = off;
        off += (bytes + 255) & ~size_t(255);
        return o;
    }
};

// The results block of n1 = max(pairs, 1) pairs (engine_core.hpp ResLayout):
// [raw32 | raw64 | flag | run counters], each from a 256-B boundary.
inline ResLayout res_layout(size_t n1)
{
    Layout L;
    ResLayout r;
    L.take(sizeof(float) * n1);
    r.o64 = L.take(sizeof(double) * n1);
    r.ofl = L.take(n1);
    r.ocnt = L.off;
    r.bytes = (r.ocnt + kNumCounters * sizeof(int) + 15) & ~size_t(15);   // whole 16-byte stores (launch_store_to_host)
    return r;
}

template <typename T>
void grow(std::vector<T>& v, size_t n)
{
    if (v.size() < n) v.resize(n);
}

// Packed rows with slack on both sides: the segmented kernels prefetch
// read words PD steps ahead without clamping to the read (run_seg), so a
// lane in pipeline fill reads up to 64 words before its read and a pair
// shorter than its wave's longest read up to that length + 64 past it;
// those words only feed rows that are never used.
inline size_t row_pad_words(int rmax) { return kRowPadBefore + size_t(rmax) + 256; }

// The packed rows (with their pad) and the hap match tables of one part must
// stay below the kernels' 2^30-word addressing.
inline int check_pool_words(int64_t rows, size_t row_pad, int64_t hap_words)
{
    if (rows + int64_t(row_pad) > kMaxRowWords)
        return fail(HC_PHMM_EINVAL, "batch too large (read bases of one part exceed 2^30)");
    if (hap_words + 16 > kMaxHapWords)
        return fail(HC_PHMM_EINVAL, "batch too large (hap match tables of one part exceed 2^30 words)");
    return HC_PHMM_OK;
}

// Offsets of a part's results block and of the scratch of the rescue (fp64)
// pass in its device allocation.
struct RescueLayout {
    ResLayout RL;
    size_t o_res, o_list, o_rec, o_sdesc, o_sorted, o_worder, o_big, o_bigc, o_plan;
};

// n1 = max(pairs, 1); n_slots = segmented slots (their records and descriptors).
inline RescueLayout take_rescue(Layout& L, size_t n1, size_t n_slots)
{
    RescueLayout o;
    o.RL = res_layout(n1);
    const size_t ns1 = std::max<size_t>(n_slots, 1);
    o.o_res = L.take(o.RL.bytes);
    o.o_rec = L.take(sizeof(uint4) * ns1);       // seg slot records
    o.o_sdesc = L.take(sizeof(PairDesc) * ns1);   // slot -> descriptor
    o.o_list = L.take(2 * sizeof(int) * n1);      // pair ids, then pack_rh (Seg64Args::list_rh)
    o.o_sorted = L.take(sizeof(int) * n1);
    o.o_worder = L.take(sizeof(int) * n1);
    o.o_big = L.take(sizeof(int) * n1);
    o.o_bigc = L.take(sizeof(int));
    o.o_plan = L.take(sizeof(Seg64Plan));
    return o;
}

inline void bind_rescue(Part& b, char* dev, const RescueLayout& o, size_t n_slots)
{
    b.res = o.RL;
    const ResView v = res_view(dev + o.o_res, o.RL);
    b.own_raw32 = b.d_raw32 = v.raw32;
    b.own_raw64 = b.d_raw64 = v.raw64;
    b.own_flag = b.d_flag = v.flag;
    b.d_count = v.counters;   // run counters (kNumCounters): the results block's tail
    b.d_list = reinterpret_cast<int*>(dev + o.o_list);
    b.d_sorted = reinterpret_cast<int*>(dev + o.o_sorted);
    b.d_worder = reinterpret_cast<int*>(dev + o.o_worder);
    b.d_big = reinterpret_cast<int*>(dev + o.o_big);
    b.d_big_count = reinterpret_cast<int*>(dev + o.o_bigc);
    b.d_plan = reinterpret_cast<Seg64Plan*>(dev + o.o_plan);
    b.d_rec = n_slots > 0 ? reinterpret_cast<uint4*>(dev + o.o_rec) : nullptr;
    b.d_sdesc = reinterpret_cast<PairDesc*>(dev + o.o_sdesc);
}

// The part's streams and events: its slot's (Slot::ev, engine_core.hpp: pack
// 0-1, the fp32 / fp64 passes 2-4, done 5, early results 6), else its device's
// streams, with events of its own made as they are needed (RunEvents).
inline void bind_streams(Part& b, Device& dv, Slot* slot)
{
    if (slot) {
        b.stream = slot->stream;
        b.side = slot->side;
        b.fork = slot->fork;
        b.join = slot->join;
        b.evs.borrow(slot->ev);
    } else {
        b.stream = dv.stream;
        b.side = dv.side;
        b.fork = dv.fork;
        b.join = dv.join;
    }
}

}  // namespace eng
}  // namespace hcphmm
