// What an interval call (include/hc_intervals.h) decides per window and per
// record, written once for the device and the host: whether a half-open range
// of a contig meets one of the contig's merged intervals (a binary search in the
// contig's slice), whether a window is asked, the up to three windows whose
// padded interval holds a position, and whether a record is in scope.
// interval_kernels.hip runs them one thread per window and per record; with
// SAMX_HOST_ONLY (no HIP header) tests/cpp/intervals_host_main.cpp runs the same
// functions under the host sanitizers, and genome_engine.cpp uses
// interval_meets for the lines of the VCF.
//
// The merged intervals. Sorted by contig, then begin; inside a contig disjoint
// and not abutting, so begin and end both ascend. Contig c's are the entries
// [first[c], first[c + 1]). No entry outside that slice is read.
//
// The windows. Window lw of a contig covers [lw * region, (lw + 1) * region),
// its padded interval is that widened by `padding` on both sides and begun at 0
// for window 0 (hc_contig.h). With padding <= region a position lies in the
// padded interval of its own window and of at most one neighbour on each side.
#pragma once
#include "genome_body.hpp"

namespace hcgenome {

struct IntervalSet {
    const int64_t* begin;   // per merged interval, 0-based
    const int64_t* end;     // half-open
    const int32_t* first;   // n_contigs + 1
};

// [b, e) (b < e) meets one of contig c's intervals: the first of them that ends
// behind b, if there is one, begins in front of e.
SAMX_FN inline bool interval_meets(const IntervalSet& s, int32_t c, int64_t b, int64_t e)
{
    int32_t lo = s.first[c];
    const int32_t top = s.first[c + 1];
    int32_t hi = top;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (s.end[mid] <= b)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < top && s.begin[lo] < e;
}

// Window lw of contig c (0 <= lw < the contig's window count) is asked: its own
// bases [origin_begin, min(origin_end, ref_len)) meet an interval.
SAMX_FN inline bool interval_window_asked(const IntervalSet& s, int32_t c, int64_t lw, int64_t region, int64_t ref_len)
{
    const int64_t b = lw * region;
    const int64_t e = b + region < ref_len ? b + region : ref_len;
    return interval_meets(s, c, b, e);
}

// The windows of a contig with n_win windows whose padded interval holds
// position p (0 <= p < ref_len), ascending in out[0 .. the return value).
SAMX_FN inline int interval_windows_of(int64_t p, int64_t region, int64_t padding, int64_t n_win, int64_t* out)
{
    const int64_t own = p / region;
    const int64_t in = p - own * region;
    int n = 0;
    if (own >= 1 && in < padding) out[n++] = own - 1;          // behind the neighbour's end by less than the padding
    out[n++] = own;
    if (own + 1 < n_win && in >= region - padding) out[n++] = own + 1;
    return n;
}

// A record of contig c (-1: none) with 1-based POS is in scope: it is placed and
// one of the windows that hold POS - 1 is asked. `asked` is per genome-wide window.
SAMX_FN inline bool interval_in_scope(int32_t c, uint32_t pos, const int64_t* ref_len, const int64_t* win_off, int64_t region,
                                      int64_t padding, const int32_t* asked)
{
    if (!genome_placed(c, pos, ref_len)) return false;
    int64_t w[3];
    const int n = interval_windows_of(int64_t(pos - 1u), region, padding, win_off[c + 1] - win_off[c], w);
    for (int k = 0; k < n; ++k)
        if (asked[win_off[c] + w[k]]) return true;
    return false;
}

}  // namespace hcgenome
