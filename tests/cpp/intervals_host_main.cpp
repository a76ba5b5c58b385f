// Host program for tests/test_intervals_host.py: csrc/interval_body.hpp and
// csrc/interval_host.hpp compiled for the host (SAMX_HOST_ONLY) and run on one
// thread under -fsanitize=address,undefined. It does what genome_engine.cpp and
// interval_kernels.hip do with an interval list: the check, the merge, then one
// step per genome-wide window (interval_ask_kernel) and one per record
// (interval_scope_kernel). The contig lengths, the window sums, the merged
// begins, ends and slices, the asked flags and the records live in heap blocks
// of exactly their sizes, so a read past them is an error, not a silent success.
//
//   intervals_host_main IN OUT
//
// IN:  any number of cases, each "region padding n_contigs n_intervals n_records",
//      n_contigs lengths, n_intervals lines "contig begin end", n_records lines
//      "contig pos" (contig -1: none; pos 1-based).
// OUT: per case "E k" (interval k fails the check) or
//      "M n", n lines "contig begin end"; "A n", n asked windows; "S" and one
//      0/1 per record; "W" and per placed record its windows "n w ...".
//
//   intervals_host_main bai INDEX N_REF FILE_LEN QUERIES OUT
//
// csrc/bai.hpp on the bytes of INDEX, held in a heap block of exactly their
// number. QUERIES: lines "ref beg end". OUT: "E message" and nothing else when
// the parse fails, else "OK" and per query "B n" with the n bins of reg2bins,
// "Q n" with n lines "beg end" (the chosen chunks) and "G n" with their merge.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <fstream>
#include <memory>
#include <string>

#include "../../gatk-haplotypecaller-cpp17_amd/csrc/bai.hpp"
#include "../../gatk-haplotypecaller-cpp17_amd/csrc/interval_body.hpp"
#include "../../gatk-haplotypecaller-cpp17_amd/csrc/interval_host.hpp"

using namespace hcgenome;

template <class T>
static std::unique_ptr<T[]> exact(const T* from, size_t n)
{
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; ++i) p[i] = from[i];
    return p;
}

static int bai_main(char** argv)
{
    std::ifstream file(argv[2], std::ios::binary);
    if (!file) return 2;
    const std::string bytes((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
    const auto block = exact(reinterpret_cast<const uint8_t*>(bytes.data()), bytes.size());
    std::FILE* out = std::fopen(argv[6], "w");
    if (!out) return 2;
    hcbai::Index idx;
    const std::string bad = hcbai::bai_parse(block.get(), int64_t(bytes.size()), std::atoll(argv[3]), std::atoll(argv[4]), idx);
    if (!bad.empty()) {
        std::fprintf(out, "E %s\n", bad.c_str());
        std::fclose(out);
        return 0;
    }
    std::fprintf(out, "OK\n");
    std::ifstream queries(argv[5]);
    int32_t ref = 0;
    int64_t beg = 0, end = 0;
    while (queries >> ref >> beg >> end) {
        std::unique_ptr<uint16_t[]> bins(new uint16_t[size_t(hcbai::kMaxBins)]);
        const int n = beg >= 0 && beg < end && end <= hcbai::kMaxPos ? hcbai::reg2bins(beg, end, bins.get()) : 0;
        std::fprintf(out, "B %d\n", n);
        for (int k = 0; k < n; ++k) std::fprintf(out, "%d\n", int(bins[size_t(k)]));
        std::vector<hcbai::Chunk> chunks;
        hcbai::bai_query(idx, ref, beg, end, chunks);
        std::fprintf(out, "Q %zu\n", chunks.size());
        for (const hcbai::Chunk& c : chunks)
            std::fprintf(out, "%llu %llu\n", static_cast<unsigned long long>(c.beg), static_cast<unsigned long long>(c.end));
        hcbai::bai_merge(chunks);
        std::fprintf(out, "G %zu\n", chunks.size());
        for (const hcbai::Chunk& c : chunks)
            std::fprintf(out, "%llu %llu\n", static_cast<unsigned long long>(c.beg), static_cast<unsigned long long>(c.end));
    }
    std::fclose(out);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 7 && std::string(argv[1]) == "bai") return bai_main(argv);
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    std::FILE* out = std::fopen(argv[2], "w");
    if (!out) return 2;
    int64_t region = 0, padding = 0;
    int32_t n_contigs = 0, n_iv = 0, n_rec = 0;
    while (in >> region >> padding >> n_contigs >> n_iv >> n_rec) {
        if (region < 1 || padding < 0 || padding > region || n_contigs < 1 || n_iv < 0 || n_rec < 0) return 2;
        std::unique_ptr<int64_t[]> ref_len(new int64_t[size_t(n_contigs)]);
        std::unique_ptr<int64_t[]> win_off(new int64_t[size_t(n_contigs) + 1]);
        win_off[0] = 0;
        for (int32_t c = 0; c < n_contigs; ++c) {
            if (!(in >> ref_len[size_t(c)]) || ref_len[size_t(c)] < 1) return 2;
            win_off[size_t(c) + 1] = win_off[size_t(c)] + (ref_len[size_t(c)] + region - 1) / region;
        }
        std::unique_ptr<hc_interval[]> iv(new hc_interval[size_t(n_iv)]);
        for (int32_t k = 0; k < n_iv; ++k)
            if (!(in >> iv[size_t(k)].contig >> iv[size_t(k)].begin >> iv[size_t(k)].end)) return 2;
        std::unique_ptr<int32_t[]> rec_contig(new int32_t[size_t(n_rec)]);
        std::unique_ptr<uint32_t[]> rec_pos(new uint32_t[size_t(n_rec)]);
        for (int32_t k = 0; k < n_rec; ++k)
            if (!(in >> rec_contig[size_t(k)] >> rec_pos[size_t(k)])) return 2;

        std::string why;
        const int64_t bad = interval_check(iv.get(), n_iv, ref_len.get(), n_contigs, why);
        if (bad >= 0) {
            if (why.empty()) return 3;
            std::fprintf(out, "E %lld\n", static_cast<long long>(bad));
            continue;
        }
        Merged m;
        interval_merge(iv.get(), n_iv, n_contigs, m);
        std::fprintf(out, "M %zu\n", m.iv.size());
        for (const hc_interval& x : m.iv)
            std::fprintf(out, "%d %lld %lld\n", x.contig, static_cast<long long>(x.begin), static_cast<long long>(x.end));
        const auto begin = exact(m.begin.data(), m.begin.size()), end = exact(m.end.data(), m.end.size());
        const auto first = exact(m.first.data(), m.first.size());
        const IntervalSet set{begin.get(), end.get(), first.get()};

        const int64_t n_windows = win_off[size_t(n_contigs)];
        std::unique_ptr<int32_t[]> asked(new int32_t[size_t(n_windows)]);
        int64_t n_asked = 0;
        for (int64_t w = 0; w < n_windows; ++w) {   // interval_ask_kernel
            const int32_t c = genome_contig_of_window(win_off.get(), n_contigs, w);
            asked[size_t(w)] = interval_window_asked(set, c, w - win_off[size_t(c)], region, ref_len[size_t(c)]) ? 1 : 0;
            n_asked += asked[size_t(w)];
        }
        std::fprintf(out, "A %lld\n", static_cast<long long>(n_asked));
        for (int64_t w = 0; w < n_windows; ++w)
            if (asked[size_t(w)]) std::fprintf(out, "%lld\n", static_cast<long long>(w));
        std::fprintf(out, "S\n");
        for (int32_t k = 0; k < n_rec; ++k)         // interval_scope_kernel
            std::fprintf(out, "%d\n", interval_in_scope(rec_contig[size_t(k)], rec_pos[size_t(k)], ref_len.get(), win_off.get(),
                                                        region, padding, asked.get())
                                          ? 1
                                          : 0);
        std::fprintf(out, "W\n");
        for (int32_t k = 0; k < n_rec; ++k) {
            const int32_t c = rec_contig[size_t(k)];
            if (!genome_placed(c, rec_pos[size_t(k)], ref_len.get())) continue;
            int64_t w[3];
            const int n = interval_windows_of(int64_t(rec_pos[size_t(k)] - 1u), region, padding,
                                              win_off[size_t(c) + 1] - win_off[size_t(c)], w);
            std::fprintf(out, "%d", n);
            for (int j = 0; j < n; ++j) std::fprintf(out, " %lld", static_cast<long long>(w[j]));
            std::fprintf(out, "\n");
        }
    }
    std::fclose(out);
    return 0;
}
