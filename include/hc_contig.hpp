// hc_contig.hpp — C++ drop-in for HaplotypeCaller itself.
//
// The reference's driver object (src/haplotypecaller/haplotypecaller.hpp:109-154)
// carries in_path, out_path and ref_path and does everything in do_work. With
//
//     hc::MI355XHaplotypeCaller caller;
//     caller.in_path = "reads.sam"; caller.ref_path = "ref.fa"; caller.out_path = "out.vcf";
//     caller.do_work();
//
// do_work reads the FASTA file's first record as fasta/fasta.hpp:23-46 does
// (the name up to the first of " \t\v\f\r", the lines appended as they are),
// upper-cases the sequence, reads the SAM file into one block and makes one
// call of libhcpairhmm.so (hc_contig_call, hc_contig.h); out_path gets the VCF
// text. The progress lines on std::cout are not written.
//
// The reference draws every pick from a fresh random_device; here the picks are
// a function of `seed` (hc_contig.h), or the first read of every position with
// pick_mode = HC_CONTIG_PICK_FIRST. skip_unplaced leaves out the reads with POS 0
// or past the contig's end, where the reference writes outside reads_map.
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

#include "hc_contig.h"

namespace hc {

class MI355XHaplotypeCaller {
public:
    std::string in_path, out_path, ref_path;
    std::uint64_t seed = 0;
    int pick_mode = HC_CONTIG_PICK_SEEDED;
    bool skip_unplaced = false;

    // use_double: the PairHMM's per-instance mode, as hc::MI355XWindowCaller's.
    explicit MI355XHaplotypeCaller(int device = -1, bool use_double = false) : device_(device), use_double_(use_double) {}

    void do_work(std::size_t region_size = HC_CONTIG_DEFAULT_REGION, std::size_t padding_size = HC_CONTIG_DEFAULT_PADDING)
    {
        std::string name, seq;
        read_fasta(name, seq);
        std::transform(seq.begin(), seq.end(), seq.begin(), [](unsigned char c) { return char(std::toupper(c)); });

        std::ifstream sam_file(in_path, std::ios::binary);
        if (!sam_file) throw std::runtime_error("hc_contig: cannot open " + in_path);
        const std::string sam((std::istreambuf_iterator<char>(sam_file)), std::istreambuf_iterator<char>());

        if (region_size > 0x7fffffffu || padding_size > 0x7fffffffu)
            throw std::invalid_argument("hc_contig: region_size / padding_size out of range");
        check(hc_phmm_init(HC_PHMM_FLAG_KEEP_MODE, device_));   // device only: the mode goes with the call
        hc_contig_result* res = nullptr;
        const uint32_t flags = (use_double_ ? HC_CONTIG_F64 : 0u) | (skip_unplaced ? HC_CONTIG_SKIP_UNPLACED : 0u);
        check(hc_contig_call(reinterpret_cast<const uint8_t*>(sam.data()), static_cast<int64_t>(sam.size()), name.c_str(),
                             reinterpret_cast<const uint8_t*>(seq.data()), static_cast<int64_t>(seq.size()),
                             static_cast<int32_t>(region_size), static_cast<int32_t>(padding_size), seed, pick_mode, flags,
                             &res));
        Holder hold{res};
        const char* text = nullptr;
        int64_t length = 0;
        check(hc_contig_result_vcf(res, &text, &length, &n_windows_));
        std::ofstream ofs(out_path, std::ios::binary);
        if (!ofs) throw std::runtime_error("hc_contig: cannot open " + out_path);
        ofs.write(text, static_cast<std::streamsize>(length));
        if (!ofs) throw std::runtime_error("hc_contig: cannot write " + out_path);
    }

    // Of the last do_work.
    int n_windows() const { return n_windows_; }

private:
    struct Holder {
        hc_contig_result* p;
        ~Holder() { hc_contig_result_free(p); }
    };

    static void check(int rc)
    {
        if (rc == HC_PHMM_EINVAL) throw std::invalid_argument(std::string("hc_contig: ") + hc_phmm_last_error());
        if (rc != HC_PHMM_OK) throw std::runtime_error(std::string("hc_contig: ") + hc_phmm_last_error());
    }

    // fasta/fasta.hpp:23-46, the first record.
    void read_fasta(std::string& name, std::string& seq) const
    {
        std::ifstream ifs(ref_path);
        if (!ifs) throw std::runtime_error("hc_contig: cannot open " + ref_path);
        std::string line;
        std::getline(ifs, line);
        if (line.empty() || line.front() != '>') throw std::runtime_error("error: expected '>'");
        const std::string_view header = std::string_view(line).substr(1);
        name = std::string(header.substr(0, header.find_first_of(" \t\v\f\r")));
        while (std::getline(ifs, line)) {
            seq.append(line);
            if (ifs.peek() == '>') break;
        }
    }

    int device_;
    bool use_double_;
    int32_t n_windows_ = 0;
};

}  // namespace hc
