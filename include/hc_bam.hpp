// hc_bam.hpp — hc::MI355XGenomeCaller (hc_genome.hpp) for a BAM file.
//
//     hc::MI355XBamGenomeCaller caller;
//     caller.in_path = "reads.bam"; caller.ref_path = "ref.fa"; caller.out_path = "out.vcf";
//     caller.do_work();
//
// The members are hc::MI355XGenomeCaller's; in_path names a BGZF-compressed BAM
// file. do_work reads every record of the FASTA file as that class does (the
// same text, restated here: its reader is private), reads the BAM file into one
// block and makes one call of libhcpairhmm.so (hc_bam_genome_call, hc_bam.h)
// with the FASTA records as the contig table; out_path gets the VCF text, the
// bytes hc::MI355XGenomeCaller writes for the SAM text `samtools view -h`
// prints for the file.
//
// Header-only and free of reference headers. Invalid input throws
// std::invalid_argument, everything else std::runtime_error, with the
// library's message.
#pragma once

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "hc_bam.h"

namespace hc {

class MI355XBamGenomeCaller {
public:
    std::string in_path, out_path, ref_path;
    std::uint64_t seed = 0;
    int pick_mode = HC_CONTIG_PICK_SEEDED;
    bool skip_unplaced = false;
    bool sorted_buckets = false;

    explicit MI355XBamGenomeCaller(int device = -1, bool use_double = false) : device_(device), use_double_(use_double) {}

    void do_work(std::size_t region_size = HC_CONTIG_DEFAULT_REGION, std::size_t padding_size = HC_CONTIG_DEFAULT_PADDING)
    {
        const std::vector<std::pair<std::string, std::string>> fasta = read_fasta();
        std::vector<hc_genome_contig> table;
        for (const auto& r : fasta)
            table.push_back(hc_genome_contig{r.first.c_str(), reinterpret_cast<const uint8_t*>(r.second.data()),
                                             static_cast<int64_t>(r.second.size())});

        std::ifstream bam_file(in_path, std::ios::binary);
        if (!bam_file) throw std::runtime_error("hc_bam: cannot open " + in_path);
        const std::string bam((std::istreambuf_iterator<char>(bam_file)), std::istreambuf_iterator<char>());

        if (region_size > 0x7fffffffu || padding_size > 0x7fffffffu)
            throw std::invalid_argument("hc_bam: region_size / padding_size out of range");
        if (table.size() > 0x7fffffffu) throw std::invalid_argument("hc_bam: too many FASTA records");
        check(hc_phmm_init(HC_PHMM_FLAG_KEEP_MODE, device_));   // device only: the mode goes with the call
        hc_genome_result* res = nullptr;
        const uint32_t flags = (use_double_ ? HC_CONTIG_F64 : 0u) | (skip_unplaced ? HC_CONTIG_SKIP_UNPLACED : 0u) |
                               (sorted_buckets ? HC_GENOME_SORTED_BUCKETS : 0u);
        check(hc_bam_genome_call(reinterpret_cast<const uint8_t*>(bam.data()), static_cast<int64_t>(bam.size()), table.data(),
                                 static_cast<int32_t>(table.size()), static_cast<int32_t>(region_size),
                                 static_cast<int32_t>(padding_size), seed, pick_mode, flags, &res));
        Holder hold{res};
        const char* text = nullptr;
        int64_t length = 0;
        check(hc_genome_result_vcf(res, &text, &length, &n_windows_, &n_contigs_));
        std::ofstream ofs(out_path, std::ios::binary);
        if (!ofs) throw std::runtime_error("hc_bam: cannot open " + out_path);
        ofs.write(text, static_cast<std::streamsize>(length));
        if (!ofs) throw std::runtime_error("hc_bam: cannot write " + out_path);
    }

    // Of the last do_work.
    int n_windows() const { return n_windows_; }
    int n_contigs() const { return n_contigs_; }

private:
    struct Holder {
        hc_genome_result* p;
        ~Holder() { hc_genome_result_free(p); }
    };

    static void check(int rc)
    {
        if (rc == HC_PHMM_EINVAL) throw std::invalid_argument(std::string("hc_bam: ") + hc_phmm_last_error());
        if (rc != HC_PHMM_OK) throw std::runtime_error(std::string("hc_bam: ") + hc_phmm_last_error());
    }

    // fasta/fasta.hpp:23-46, applied until the file ends, as hc::MI355XGenomeCaller reads it.
    std::vector<std::pair<std::string, std::string>> read_fasta() const
    {
        std::ifstream ifs(ref_path);
        if (!ifs) throw std::runtime_error("hc_bam: cannot open " + ref_path);
        std::vector<std::pair<std::string, std::string>> out;
        std::string line;
        while (std::getline(ifs, line)) {
            if (line.empty() || line.front() != '>') throw std::runtime_error("error: expected '>'");
            const std::string_view header = std::string_view(line).substr(1);
            std::string name(header.substr(0, header.find_first_of(" \t\v\f\r")));
            if (ifs.peek() == '>' || ifs.peek() == std::ifstream::traits_type::eof())
                throw std::invalid_argument("hc_bam: FASTA record " + name + " has no sequence line");
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
    int32_t n_windows_ = 0, n_contigs_ = 0;
};

}  // namespace hc
