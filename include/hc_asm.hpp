// hc_asm.hpp — C++ drop-in for the reference's Assembler.
//
// HaplotypeCaller::call_region (src/haplotypecaller/haplotypecaller.hpp:83-107)
// begins with
//
//     auto haplotypes = assembler.assemble(reads, ref);
//
// With `hc::MI355XAssembler<Haplotype> assembler;` that line compiles unchanged:
// assemble() has the signature of assembler/assembler.hpp:56 and returns the
// haplotypes with bases, score, alignment_begin_wrt_ref and cigar set, the last
// two through hc::MI355XSWAligner::align_haplotypes exactly as
// graph_wrapper.hpp:232-240 does. assemble_regions() does many regions in one
// device pass (and one aligner pass per region).
//
// Header-only over the C ABI of hc_asm.h and hc_sw.h; templated on the caller's
// types (ReadT: .SEQ and .QUAL strings; HaplotypeT: constructible from
// (std::string, double), with .bases, .alignment_begin_wrt_ref and a .cigar
// assignable from the CIGAR text), so it needs no reference header.
//
// A region that ends HC_ASM_NO_HAPLOTYPES or HC_ASM_TOO_COMPLEX gives an empty
// vector, as the reference's nine failed attempts do; region_status() tells the
// two apart after the call.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "hc_asm.h"
#include "hc_sw.hpp"

namespace hc {

template <class HaplotypeT>
class MI355XAssembler {
public:
    // assembler/assembler.hpp:15-18
    static constexpr std::size_t INITIAL_KMER_SIZE = 25;
    static constexpr std::size_t KMER_SIZE_ITERATION_INCREASE = 10;
    static constexpr std::size_t MAX_KMER_ITERATIONS_TO_ATTEMPT = HC_ASM_MAX_ATTEMPTS;
    static constexpr std::size_t MAX_UNIQUE_KMERS_COUNT_TO_DISCARD = 2000;

    template <class ReadT>
    struct Region {
        const std::vector<ReadT>* reads;
        std::string_view ref;
    };

    explicit MI355XAssembler(int device = -1) : aligner_(device) {}

    // Assembler::assemble.
    template <class ReadT>
    std::vector<HaplotypeT> assemble(const std::vector<ReadT>& reads, std::string_view ref)
    {
        std::vector<Region<ReadT>> one{Region<ReadT>{&reads, ref}};
        return std::move(assemble_regions(one)[0]);
    }

    // Every region in one device pass; the haplotypes of region r in out[r].
    template <class ReadT>
    std::vector<std::vector<HaplotypeT>> assemble_regions(const std::vector<Region<ReadT>>& regions)
    {
        std::vector<std::vector<hc_asm_read>> reads(regions.size());
        std::vector<hc_asm_region> in(regions.size());
        for (size_t r = 0; r < regions.size(); ++r) {
            const auto& src = *regions[r].reads;
            reads[r].reserve(src.size());
            for (const auto& rd : src) {
                if (rd.QUAL.size() < rd.SEQ.size()) throw std::invalid_argument("hc_asm: a read with fewer qualities than bases");
                reads[r].push_back(hc_asm_read{reinterpret_cast<const uint8_t*>(rd.SEQ.data()),
                                               reinterpret_cast<const uint8_t*>(rd.QUAL.data()),
                                               static_cast<int32_t>(rd.SEQ.size())});
            }
            in[r] = hc_asm_region{reinterpret_cast<const uint8_t*>(regions[r].ref.data()),
                                  static_cast<int32_t>(regions[r].ref.size()), reads[r].data(),
                                  static_cast<int32_t>(reads[r].size())};
        }
        hc_asm_result* res = nullptr;
        check(hc_asm_assemble(in.data(), static_cast<int32_t>(in.size()), 0, &res));
        Holder hold{res};
        std::vector<std::vector<HaplotypeT>> out(regions.size());
        status_.assign(regions.size(), HC_ASM_NO_HAPLOTYPES);
        kmer_size_.assign(regions.size(), 0);
        for (size_t r = 0; r < regions.size(); ++r) {
            int32_t n_haps = 0;
            check(hc_asm_result_region(res, static_cast<int32_t>(r), &status_[r], &kmer_size_[r], nullptr, &n_haps, nullptr));
            out[r].reserve(static_cast<size_t>(n_haps));
            for (int32_t h = 0; h < n_haps; ++h) {
                const uint8_t* bases = nullptr;
                int32_t length = 0;
                double score = 0;
                check(hc_asm_result_hap(res, static_cast<int32_t>(r), h, &bases, &length, &score));
                out[r].emplace_back(std::string(reinterpret_cast<const char*>(bases), static_cast<size_t>(length)), score);
            }
            if (!out[r].empty()) aligner_.align_haplotypes(regions[r].ref, out[r]);   // graph_wrapper.hpp:232-240
        }
        return out;
    }

    // Of the last call: HC_ASM_OK, HC_ASM_NO_HAPLOTYPES or HC_ASM_TOO_COMPLEX, and the accepted k (0: none).
    int region_status(std::size_t region = 0) const { return status_.at(region); }
    std::size_t kmer_size(std::size_t region = 0) const { return static_cast<std::size_t>(kmer_size_.at(region)); }

private:
    struct Holder {
        hc_asm_result* p;
        ~Holder() { hc_asm_result_free(p); }
    };
    static void check(int rc)
    {
        if (rc != HC_PHMM_OK) throw std::runtime_error(std::string("hc_asm: ") + hc_phmm_last_error());
    }
    MI355XSWAligner aligner_;
    std::vector<int32_t> status_, kmer_size_;
};

}  // namespace hc
