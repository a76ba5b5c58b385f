// hc_region.hpp — C++ drop-in for the compute of HaplotypeCaller::call_region.
//
// The driver (src/haplotypecaller/haplotypecaller.hpp:83-107) runs, behind the
// assembler,
//
//     auto likelihoods = pairhmm.compute_likelihoods(haplotypes, reads);                    // :103
//     auto variants = genotyper.assign_genotype_likelihoods(reads, haplotypes, likelihoods,
//                                                           ref, padded_region, origin_region);   // :104
//
// Replacing both lines with
//
//     hc::MI355XRegionCaller<Variant> caller;
//     auto variants = caller.call(reads, haplotypes, ref, padded_region, origin_region);
//
// gives the same variants and leaves `reads` as compute_likelihoods does: the
// poorly modelled reads are erased. Haplotypes that arrive with an empty CIGAR
// are aligned against `ref` on the device first, as hc::MI355XSWAligner::
// align_haplotypes would (NEW_SW_PARAMETERS, soft-clipped overhangs), and get
// their alignment_begin_wrt_ref and cigar filled: the assembler's alignment loop
// (assembler/graph_wrapper.hpp:232-240) may then be dropped as well. One call of
// libhcpairhmm.so (hc_region_call, hc_region.h) does all of it; call_many takes
// any number of regions in one device pass.
//
// Header-only; templated on the caller's types so it needs no reference header:
//   Haplotype  .bases, .alignment_begin_wrt_ref, .cigar (assignable from
//              std::string; convertible to std::string, or with .to_string())
//   SAMRecord  .SEQ, .QUAL, .insertionGOP(), .deletionGOP(), .overallGCP(),
//              .get_interval() with .begin and .end
//   Interval   {contig, begin, end}
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <type_traits>
#include <utility>
#include <vector>

#include "hc_region.h"

namespace hc {

template <class VariantT>
class MI355XRegionCaller {
public:
    // use_double: the PairHMM's per-instance mode, as hc::MI355XPairHMM's.
    explicit MI355XRegionCaller(int device = -1, bool use_double = false) : device_(device), use_double_(use_double) {}

    // One region of a batch for call_many(): reads and haplotypes are updated in place.
    template <class SAMRecordT, class HaplotypeT, class IntervalT>
    struct Region {
        std::vector<SAMRecordT>* reads;
        std::vector<HaplotypeT>* haplotypes;
        std::string_view ref;
        IntervalT padded_region, origin_region;
    };

    template <class SAMRecordT, class HaplotypeT, class IntervalT>
    std::vector<VariantT> call(std::vector<SAMRecordT>& reads, std::vector<HaplotypeT>& haplotypes, std::string_view ref,
                               const IntervalT& padded_region, const IntervalT& origin_region)
    {
        std::vector<Region<SAMRecordT, HaplotypeT, IntervalT>> one{{&reads, &haplotypes, ref, padded_region, origin_region}};
        return std::move(call_many(one)[0]);
    }

    template <class SAMRecordT, class HaplotypeT, class IntervalT>
    std::vector<std::vector<VariantT>> call_many(const std::vector<Region<SAMRecordT, HaplotypeT, IntervalT>>& regions)
    {
        const size_t n = regions.size();
        std::vector<hc_region_in> rv(n);
        std::vector<std::vector<hc_region_hap>> haps(n);
        std::vector<std::vector<std::string>> cigars(n);
        std::vector<std::vector<hc_phmm_read>> reads(n);
        std::vector<std::vector<int64_t>> rb(n), re(n);
        std::vector<std::string> gaps;   // owned i/d/c strings where a record's are short
        size_t total_reads = 0;
        for (const auto& x : regions) total_reads += x.reads->size();
        gaps.reserve(3 * total_reads);
        bool want_cigars = false;
        for (size_t k = 0; k < n; ++k) {
            const auto& x = regions[k];
            const size_t nh = x.haplotypes->size(), nr = x.reads->size();
            cigars[k].reserve(nh);
            haps[k].resize(nh);
            for (size_t h = 0; h < nh; ++h) {
                const auto& hap = (*x.haplotypes)[h];
                cigars[k].push_back(cigar_text(hap.cigar));
                haps[k][h].bases = reinterpret_cast<const uint8_t*>(hap.bases.data());
                haps[k][h].length = static_cast<int32_t>(hap.bases.size());
                haps[k][h].alignment_begin = static_cast<int32_t>(hap.alignment_begin_wrt_ref);
                haps[k][h].cigar = cigars[k][h].empty() ? nullptr : cigars[k][h].c_str();
                want_cigars |= cigars[k][h].empty();
            }
            reads[k].resize(nr);
            rb[k].resize(nr);
            re[k].resize(nr);
            for (size_t r = 0; r < nr; ++r) {
                const auto& rec = (*x.reads)[r];
                const size_t len = rec.SEQ.size();
                auto pick = [&](auto view, char fill) -> const char* {
                    if (view.size() >= len) return view.data();
                    gaps.emplace_back(len, fill);
                    return gaps.back().data();
                };
                reads[k][r].length = static_cast<int32_t>(len);
                reads[k][r].bases = rec.SEQ.data();
                reads[k][r].q = rec.QUAL.data();
                reads[k][r].i = pick(rec.insertionGOP(), 'I');
                reads[k][r].d = pick(rec.deletionGOP(), 'I');
                reads[k][r].c = pick(rec.overallGCP(), '+');
                const auto iv = rec.get_interval();
                rb[k][r] = static_cast<int64_t>(iv.begin);
                re[k][r] = static_cast<int64_t>(iv.end);
            }
            hc_region_in& g = rv[k];
            g.ref = reinterpret_cast<const uint8_t*>(x.ref.data());
            g.ref_len = static_cast<int32_t>(x.ref.size());
            g.padded_begin = static_cast<int64_t>(x.padded_region.begin);
            g.origin_begin = static_cast<int64_t>(x.origin_region.begin);
            g.origin_end = static_cast<int64_t>(x.origin_region.end);
            g.haps = haps[k].data();
            g.n_haps = static_cast<int32_t>(nh);
            g.reads = reads[k].data();
            g.read_begin = rb[k].data();
            g.read_end = re[k].data();
            g.n_reads = static_cast<int32_t>(nr);
        }
        check(hc_phmm_init(HC_PHMM_FLAG_KEEP_MODE, device_));   // device only: the mode goes with the call
        hc_region_calls* calls = nullptr;
        const uint32_t flags = (use_double_ ? HC_REGION_F64 : 0u) | (want_cigars ? HC_REGION_WANT_CIGARS : 0u);
        check(hc_region_call(rv.data(), static_cast<int32_t>(n), flags, &calls));
        const hc_gt_call_site* sites = nullptr;
        int64_t ns = 0;
        hc_region_calls_sites(calls, &sites, &ns);
        std::vector<std::vector<VariantT>> out(n);
        for (int64_t s = 0; s < ns; ++s) {
            const hc_gt_call_site& c = sites[s];
            if (c.status != HC_GT_SITE_EMITTED) continue;
            const auto& x = regions[static_cast<size_t>(c.region)];
            std::vector<std::string> alleles(c.alleles, c.alleles + c.n_alleles);
            IntervalT loc{x.padded_region.contig, static_cast<std::size_t>(c.begin), static_cast<std::size_t>(c.loc_end)};
            out[static_cast<size_t>(c.region)].emplace_back(
                std::move(loc), std::move(alleles),
                std::pair<std::size_t, std::size_t>(static_cast<std::size_t>(c.a1), static_cast<std::size_t>(c.a2)),
                static_cast<std::size_t>(c.genotype_quality));
        }
        for (size_t k = 0; k < n; ++k) {
            const auto& x = regions[k];
            // Alignments of the haplotypes that came without one.
            if (!x.haplotypes->empty() && cigars[k][0].empty())
                for (size_t h = 0; h < x.haplotypes->size(); ++h) {
                    int32_t begin = 0;
                    const char* text = nullptr;
                    hc_region_calls_alignment(calls, static_cast<int32_t>(k), static_cast<int32_t>(h), &begin, &text);
                    (*x.haplotypes)[h].alignment_begin_wrt_ref = static_cast<std::size_t>(begin);
                    (*x.haplotypes)[h].cigar = std::string(text ? text : "");
                }
            // IntelPairHMM::compute_likelihoods erases the poorly modelled reads.
            const uint8_t* keep = nullptr;
            int32_t nr = 0, kept = 0;
            hc_region_calls_reads(calls, static_cast<int32_t>(k), &keep, &nr, &kept);
            std::vector<SAMRecordT> survivors;
            survivors.reserve(static_cast<size_t>(kept));
            for (int32_t r = 0; r < nr; ++r)
                if (keep[r]) survivors.push_back(std::move((*x.reads)[static_cast<size_t>(r)]));
            x.reads->swap(survivors);
        }
        hc_region_calls_free(calls);
        return out;
    }

private:
    template <class CigarT>
    static std::string cigar_text(const CigarT& c)
    {
        if constexpr (std::is_convertible_v<const CigarT&, std::string>) return c;
        else return c.to_string();
    }
    static void check(int rc)
    {
        if (rc == HC_PHMM_EINVAL) throw std::invalid_argument(std::string("hc_region: ") + hc_phmm_last_error());
        if (rc != HC_PHMM_OK) throw std::runtime_error(std::string("hc_region: ") + hc_phmm_last_error());
    }
    int device_;
    bool use_double_;
};

}  // namespace hc
