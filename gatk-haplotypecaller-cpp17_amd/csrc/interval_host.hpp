// Host side of an interval list (include/hc_intervals.h): the argument check
// and the merge. Host only and free of HIP, so that
// tests/cpp/intervals_host_main.cpp runs it under the host sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/hc_intervals.h"

namespace hcgenome {

// The merged intervals as interval_body.hpp's IntervalSet reads them.
struct Merged {
    std::vector<hc_interval> iv;   // sorted by contig, then begin; disjoint and not abutting inside a contig
    std::vector<int64_t> begin, end;
    std::vector<int32_t> first;    // n_contigs + 1
};

// The first interval that is no range of its contig, with the reason, or -1.
inline int64_t interval_check(const hc_interval* iv, int32_t n, const int64_t* ref_len, int32_t n_contigs, std::string& why)
{
    for (int32_t k = 0; k < n; ++k) {
        const hc_interval& x = iv[k];
        if (x.contig < 0 || x.contig >= n_contigs)
            why = "contig index outside the table";
        else if (x.begin < 0)
            why = "begin below 0";
        else if (x.end <= x.begin)
            why = "end not above begin";
        else if (x.end > ref_len[x.contig])
            why = "end above the contig's ref_len";
        else
            continue;
        return k;
    }
    return -1;
}

// Of checked intervals. An interval that begins at or in front of the end of the one before joins it.
inline void interval_merge(const hc_interval* iv, int32_t n, int32_t n_contigs, Merged& m)
{
    std::vector<hc_interval> v(iv, iv + n);
    std::sort(v.begin(), v.end(), [](const hc_interval& a, const hc_interval& b) {
        return a.contig != b.contig ? a.contig < b.contig : a.begin != b.begin ? a.begin < b.begin : a.end < b.end;
    });
    m.iv.clear();
    for (const hc_interval& x : v) {
        if (!m.iv.empty() && m.iv.back().contig == x.contig && x.begin <= m.iv.back().end)
            m.iv.back().end = std::max(m.iv.back().end, x.end);
        else
            m.iv.push_back(x);
    }
    m.begin.clear();
    m.end.clear();
    m.first.assign(size_t(n_contigs) + 1, 0);
    for (const hc_interval& x : m.iv) {
        m.begin.push_back(x.begin);
        m.end.push_back(x.end);
        ++m.first[size_t(x.contig) + 1];
    }
    for (int32_t c = 0; c < n_contigs; ++c) m.first[size_t(c) + 1] += m.first[size_t(c)];
}

}  // namespace hcgenome
