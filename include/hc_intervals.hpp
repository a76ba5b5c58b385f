// hc_intervals.hpp — hc::MI355XBamGenomeCaller (hc_bam.hpp) on the windows that
// a list of intervals asks for.
//
//     hc::MI355XIntervalCaller caller;
//     caller.in_path = "reads.bam"; caller.ref_path = "ref.fa"; caller.out_path = "out.vcf";
//     caller.bed_path = "panel.bed";
//     caller.intervals.push_back({"chr7", 55019016, 55211628});
//     caller.do_work();
//
// The members are hc::MI355XBamGenomeCaller's, plus index_path (empty: no index),
// bed_path (empty: none) and `intervals`, which are used together: the call
// asks for the BED file's intervals and for the vector's. in_path is taken as a
// BAM file when it begins with the bytes 1f 8b, else as SAM text. do_work reads
// the FASTA file as that class does and makes one call of libhcpairhmm.so
// (hc_genome_call_intervals or hc_bam_genome_call_intervals, hc_intervals.h)
// with the FASTA records as the contig table; out_path gets the VCF text.
//
// BED. The first three white-space separated columns are read: a FASTA record's
// name, begin and end, 0-based and half-open. Empty lines and lines that begin
// with '#', "track" or "browser" are skipped. A name that is no FASTA record, a
// line with fewer than three columns or a begin or end that is no number throws
// std::invalid_argument naming the 1-based line; so does a Region whose name is
// no FASTA record.
//
// Header-only and free of reference headers. Invalid input throws
// std::invalid_argument, everything else std::runtime_error, with the
// library's message. index_path names the .bai of a coordinate-sorted BAM file:
// with it only the members that hold the asked ranges are read (hc_intervals.h,
// "With an index"); it is not used for SAM text.
#pragma once

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <fstream>
#include <iterator>
#include <sstream>
#include <stdexcept>
#include <string>
#include <string_view>
#include <unordered_map>
#include <utility>
#include <vector>

#include "hc_intervals.h"

namespace hc {

class MI355XIntervalCaller {
public:
    struct Region {
        std::string name;
        std::int64_t begin, end;
    };

    std::string in_path, out_path, ref_path, index_path, bed_path;
    std::vector<Region> intervals;
    std::uint64_t seed = 0;
    int pick_mode = HC_CONTIG_PICK_SEEDED;
    bool skip_unplaced = false;
    bool sorted_buckets = false;

    explicit MI355XIntervalCaller(int device = -1, bool use_double = false) : device_(device), use_double_(use_double) {}

    void do_work(std::size_t region_size = HC_CONTIG_DEFAULT_REGION, std::size_t padding_size = HC_CONTIG_DEFAULT_PADDING)
    {
        const std::vector<std::pair<std::string, std::string>> fasta = read_fasta();
        std::vector<hc_genome_contig> table;
        std::unordered_map<std::string, int32_t> where;
        for (const auto& r : fasta) {
            where.emplace(r.first, static_cast<int32_t>(table.size()));
            table.push_back(hc_genome_contig{r.first.c_str(), reinterpret_cast<const uint8_t*>(r.second.data()),
                                             static_cast<int64_t>(r.second.size())});
        }
        std::vector<hc_interval> asked = read_bed(where);
        for (const Region& r : intervals) {
            const auto at = where.find(r.name);
            if (at == where.end()) throw std::invalid_argument("hc_intervals: interval contig " + r.name + " is no FASTA record");
            asked.push_back(hc_interval{at->second, r.begin, r.end});
        }

        const std::string in = slurp(in_path), index = index_path.empty() ? std::string() : slurp(index_path);
        if (region_size > 0x7fffffffu || padding_size > 0x7fffffffu)
            throw std::invalid_argument("hc_intervals: region_size / padding_size out of range");
        if (table.size() > 0x7fffffffu) throw std::invalid_argument("hc_intervals: too many FASTA records");
        if (asked.size() > 0x7fffffffu) throw std::invalid_argument("hc_intervals: too many intervals");
        check(hc_phmm_init(HC_PHMM_FLAG_KEEP_MODE, device_));   // device only: the mode goes with the call
        hc_genome_result* res = nullptr;
        const uint32_t flags = (use_double_ ? HC_CONTIG_F64 : 0u) | (skip_unplaced ? HC_CONTIG_SKIP_UNPLACED : 0u) |
                               (sorted_buckets ? HC_GENOME_SORTED_BUCKETS : 0u);
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(in.data());
        const bool bam = in.size() >= 2 && bytes[0] == 0x1f && bytes[1] == 0x8b;
        if (bam)
            check(hc_bam_genome_call_intervals(bytes, static_cast<int64_t>(in.size()),
                                               index_path.empty() ? nullptr : reinterpret_cast<const uint8_t*>(index.data()),
                                               static_cast<int64_t>(index.size()), table.data(), static_cast<int32_t>(table.size()),
                                               asked.data(), static_cast<int32_t>(asked.size()), static_cast<int32_t>(region_size),
                                               static_cast<int32_t>(padding_size), seed, pick_mode, flags, &res));
        else
            check(hc_genome_call_intervals(bytes, static_cast<int64_t>(in.size()), table.data(), static_cast<int32_t>(table.size()),
                                           asked.data(), static_cast<int32_t>(asked.size()), static_cast<int32_t>(region_size),
                                           static_cast<int32_t>(padding_size), seed, pick_mode, flags, &res));
        Holder hold{res};
        const char* text = nullptr;
        int64_t length = 0;
        check(hc_genome_result_vcf(res, &text, &length, &n_windows_, &n_contigs_));
        check(hc_genome_result_intervals(res, nullptr, nullptr, nullptr, &n_asked_));
        std::ofstream ofs(out_path, std::ios::binary);
        if (!ofs) throw std::runtime_error("hc_intervals: cannot open " + out_path);
        ofs.write(text, static_cast<std::streamsize>(length));
        if (!ofs) throw std::runtime_error("hc_intervals: cannot write " + out_path);
    }

    // Of the last do_work.
    int n_windows() const { return n_windows_; }
    int n_contigs() const { return n_contigs_; }
    int n_asked() const { return n_asked_; }

private:
    struct Holder {
        hc_genome_result* p;
        ~Holder() { hc_genome_result_free(p); }
    };

    static void check(int rc)
    {
        if (rc == HC_PHMM_EINVAL) throw std::invalid_argument(std::string("hc_intervals: ") + hc_phmm_last_error());
        if (rc != HC_PHMM_OK) throw std::runtime_error(std::string("hc_intervals: ") + hc_phmm_last_error());
    }

    static std::string slurp(const std::string& path)
    {
        std::ifstream file(path, std::ios::binary);
        if (!file) throw std::runtime_error("hc_intervals: cannot open " + path);
        return std::string((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
    }

    std::vector<hc_interval> read_bed(const std::unordered_map<std::string, int32_t>& where) const
    {
        std::vector<hc_interval> out;
        if (bed_path.empty()) return out;
        std::ifstream ifs(bed_path);
        if (!ifs) throw std::runtime_error("hc_intervals: cannot open " + bed_path);
        std::string line;
        for (std::size_t no = 1; std::getline(ifs, line); ++no) {
            const std::string at = "hc_intervals: BED line " + std::to_string(no) + ": ";
            std::istringstream cols(line);
            std::string name, begin, end;
            if (!(cols >> name)) continue;   // empty
            if (line.front() == '#' || line.rfind("track", 0) == 0 || line.rfind("browser", 0) == 0) continue;
            if (!(cols >> begin >> end)) throw std::invalid_argument(at + "fewer than three columns");
            const auto c = where.find(name);
            if (c == where.end()) throw std::invalid_argument(at + name + " is no FASTA record");
            hc_interval iv{c->second, 0, 0};
            if (!number(begin, iv.begin) || !number(end, iv.end)) throw std::invalid_argument(at + "begin or end is not a number");
            out.push_back(iv);
        }
        return out;
    }

    static bool number(const std::string& s, std::int64_t& v)
    {
        if (s.empty() || s.size() > 18) return false;
        v = 0;
        for (const char c : s) {
            if (c < '0' || c > '9') return false;
            v = v * 10 + (c - '0');
        }
        return true;
    }

    // fasta/fasta.hpp:23-46, applied until the file ends, as hc::MI355XGenomeCaller reads it.
    std::vector<std::pair<std::string, std::string>> read_fasta() const
    {
        std::ifstream ifs(ref_path);
        if (!ifs) throw std::runtime_error("hc_intervals: cannot open " + ref_path);
        std::vector<std::pair<std::string, std::string>> out;
        std::string line;
        while (std::getline(ifs, line)) {
            if (line.empty() || line.front() != '>') throw std::runtime_error("error: expected '>'");
            const std::string_view header = std::string_view(line).substr(1);
            std::string name(header.substr(0, header.find_first_of(" \t\v\f\r")));
            if (ifs.peek() == '>' || ifs.peek() == std::ifstream::traits_type::eof())
                throw std::invalid_argument("hc_intervals: FASTA record " + name + " has no sequence line");
            std::string seq;
            while (std::getline(ifs, line)) {
                seq.append(line);
                if (ifs.peek() == '>') break;
            }
            std::transform(seq.begin(), seq.end(), seq.begin(), [](unsigned char c) { return char(std::toupper(c)); });
            out.emplace_back(std::move(name), std::move(seq));
        }
        return out;
    }

    int device_;
    bool use_double_;
    int32_t n_windows_ = 0, n_contigs_ = 0, n_asked_ = 0;
};

}  // namespace hc
