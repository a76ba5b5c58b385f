// The BAM index (.bai, SAM specification §5.2) as the indexed front of
// bam_engine.cpp reads it: the parse with its checks, reg2bins over the six
// levels up to 2^29, the query of one range and the merge of the chosen chunks.
// Host only and free of HIP, so that tests/cpp/intervals_host_main.cpp runs it
// under the host sanitizers. No byte at or past the index's length is read.
//
// A virtual offset is (the member's offset in the file << 16) | the offset in
// the member's inflated bytes. A chunk [beg, end) holds records of one bin. The
// linear index gives, per 16 KiB window of a reference, the least virtual
// offset of a record that overlaps the window.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace hcbai {

constexpr int64_t kMaxPos = int64_t(1) << 29;
constexpr uint32_t kMetaBin = 37450;   // the metadata pseudo-bin: passed over
constexpr int kMaxBins = 37449;        // ((1 << 18) - 1) / 7

struct Chunk {
    uint64_t beg, end;
};

struct Bin {
    uint32_t bin;
    int32_t first, n;   // its chunks in Ref::chunks
};

struct Ref {
    std::vector<Bin> bins;
    std::vector<Chunk> chunks;
    std::vector<uint64_t> linear;
};

struct Index {
    std::vector<Ref> refs;
};

inline uint64_t bai_coff(uint64_t v) { return v >> 16; }

struct Reader {
    const uint8_t* p;
    int64_t len, at = 0;
    bool cut = false;
    uint64_t take(int n)
    {
        if (cut || at + n > len) {
            cut = true;
            return 0;
        }
        uint64_t v = 0;
        for (int k = 0; k < n; ++k) v |= uint64_t(p[at + k]) << (8 * k);
        at += n;
        return v;
    }
    int32_t i32() { return int32_t(uint32_t(take(4))); }
};

// "" or the error, beginning "BAI: ". n_ref is the BAM header's, file_len the BAM file's.
inline std::string bai_parse(const uint8_t* p, int64_t len, int64_t n_ref, int64_t file_len, Index& out)
{
    const std::string cut = "BAI: cut short";
    out.refs.clear();
    if (!p || len < 0) return "BAI: null index / negative length";
    if (len < 4) return cut;
    if (p[0] != 'B' || p[1] != 'A' || p[2] != 'I' || p[3] != 1) return "BAI: missing BAI\\1 magic";
    Reader r{p, len, 4};
    const int32_t n = r.i32();
    if (r.cut) return cut;
    if (n != n_ref) return "BAI: n_ref is " + std::to_string(n) + ", the BAM header has " + std::to_string(n_ref) + " references";
    const auto past = [&](uint64_t v) { return int64_t(bai_coff(v)) >= file_len; };
    for (int32_t k = 0; k < n; ++k) {
        out.refs.emplace_back();
        Ref& ref = out.refs.back();
        const int32_t n_bin = r.i32();
        if (r.cut) return cut;
        if (n_bin < 0) return "BAI: a negative count";
        for (int32_t b = 0; b < n_bin; ++b) {
            const uint32_t bin = uint32_t(r.take(4));
            const int32_t n_chunk = r.i32();
            if (r.cut) return cut;
            if (n_chunk < 0) return "BAI: a negative count";
            if (int64_t(n_chunk) * 16 > len - r.at) return cut;   // before anything is reserved for them
            Bin entry{bin, int32_t(ref.chunks.size()), 0};
            for (int32_t c = 0; c < n_chunk; ++c) {
                const Chunk ch{r.take(8), r.take(8)};
                if (bin == kMetaBin) continue;
                if (ch.beg > ch.end) return "BAI: a chunk with beg above end";
                if (past(ch.beg) || past(ch.end)) return "BAI: a compressed offset at or past the file's length";
                ref.chunks.push_back(ch);
                ++entry.n;
            }
            if (bin != kMetaBin) ref.bins.push_back(entry);
        }
        const int32_t n_intv = r.i32();
        if (r.cut) return cut;
        if (n_intv < 0) return "BAI: a negative count";
        if (int64_t(n_intv) * 8 > len - r.at) return cut;
        for (int32_t i = 0; i < n_intv; ++i) {
            const uint64_t v = r.take(8);
            if (past(v)) return "BAI: a compressed offset at or past the file's length";
            ref.linear.push_back(v);
        }
    }
    return "";   // the trailing n_no_coor is optional and not read
}

// The bins that may hold a record overlapping [beg, end), 0 <= beg < end <= 2^29; at most kMaxBins.
inline int reg2bins(int64_t beg, int64_t end, uint16_t* list)
{
    int n = 0;
    --end;
    list[n++] = 0;
    for (int64_t k = 1 + (beg >> 26); k <= 1 + (end >> 26); ++k) list[n++] = uint16_t(k);
    for (int64_t k = 9 + (beg >> 23); k <= 9 + (end >> 23); ++k) list[n++] = uint16_t(k);
    for (int64_t k = 73 + (beg >> 20); k <= 73 + (end >> 20); ++k) list[n++] = uint16_t(k);
    for (int64_t k = 585 + (beg >> 17); k <= 585 + (end >> 17); ++k) list[n++] = uint16_t(k);
    for (int64_t k = 4681 + (beg >> 14); k <= 4681 + (end >> 14); ++k) list[n++] = uint16_t(k);
    return n;
}

// Appends the chunks of the candidate bins of reference `ref` for [beg, end),
// but those that end at or in front of the linear index's offset for the
// 16 KiB window of `beg` (beyond the linear index: its last entry).
inline void bai_query(const Index& idx, int32_t ref, int64_t beg, int64_t end, std::vector<Chunk>& out)
{
    if (ref < 0 || size_t(ref) >= idx.refs.size() || beg < 0 || beg >= end || end > kMaxPos) return;
    const Ref& r = idx.refs[size_t(ref)];
    uint64_t min_off = 0;
    if (!r.linear.empty()) min_off = r.linear[std::min(size_t(beg >> 14), r.linear.size() - 1)];
    std::vector<uint16_t> bins(static_cast<size_t>(kMaxBins), 0);
    const int n = reg2bins(beg, end, bins.data());
    std::vector<bool> wanted(static_cast<size_t>(kMaxBins), false);
    for (int k = 0; k < n; ++k) wanted[bins[size_t(k)]] = true;
    for (const Bin& b : r.bins) {
        if (b.bin >= uint32_t(kMaxBins) || !wanted[b.bin]) continue;
        for (int32_t c = 0; c < b.n; ++c) {
            const Chunk& ch = r.chunks[size_t(b.first + c)];
            if (ch.end > min_off) out.push_back(ch);
        }
    }
}

// Sorted by beg; a chunk that begins inside the one before, or in the member the one before ends in, joins it.
inline void bai_merge(std::vector<Chunk>& v)
{
    std::sort(v.begin(), v.end(), [](const Chunk& a, const Chunk& b) { return a.beg != b.beg ? a.beg < b.beg : a.end < b.end; });
    size_t n = 0;
    for (const Chunk& ch : v) {
        if (n && (ch.beg <= v[n - 1].end || bai_coff(ch.beg) <= bai_coff(v[n - 1].end)))
            v[n - 1].end = std::max(v[n - 1].end, ch.end);
        else
            v[n++] = ch;
    }
    v.resize(n);
}

}  // namespace hcbai
