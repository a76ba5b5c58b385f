// hc_gt.hpp — C++ drop-in for the reference's Genetyper.
//
// The HaplotypeCaller driver calls (src/haplotypecaller/haplotypecaller.hpp)
//
//     Genetyper genotyper;
//     auto variants = genotyper.assign_genotype_likelihoods(reads, haplotypes, likelihoods,
//                                                           ref, padded_region, origin_region);
//
// Replacing `Genetyper` with `hc::MI355XGenotyper<Variant>` keeps that call as it
// is: the argument order of genotyper/genotyper.hpp:369-374 and the same result,
// a std::vector<Variant> built from (Interval alleles_loc, alleles, genotype pair,
// quality) for every emitted site in ascending begin. Events, sites, alleles,
// haplotype -> allele maps, kept reads and the likelihood arithmetic run in one
// device pass of libhcpairhmm.so (hc_gt_call_regions, hc_gt.h).
//
// Unlike the reference it does not fill Haplotype::event_map or
// Haplotype::rank: the haplotypes are read only. Input the reference would read
// out of bounds (a CIGAR that does not fit, an origin outside the padded
// region) and CIGAR operators it throws on raise std::invalid_argument.
//
// Header-only; templated on the caller's types so it needs no reference header:
//   Haplotype  .bases, .alignment_begin_wrt_ref, .cigar (convertible to
//              std::string, or with .to_string() as the reference's Cigar)
//   SAMRecord  .get_interval() with .begin and .end
//   Interval   {contig, begin, end}
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <type_traits>
#include <utility>
#include <vector>

#include "hc_gt.h"
#include "hc_pairhmm.h"

namespace hc {

template <class VariantT>
class MI355XGenotyper {
public:
    // One region of a batch for assign_many().
    template <class SAMRecordT, class HaplotypeT, class IntervalT>
    struct Region {
        const std::vector<SAMRecordT>* reads;
        const std::vector<HaplotypeT>* haplotypes;
        const std::vector<std::vector<double>>* likelihoods;
        std::string_view ref;
        IntervalT padded_region, origin_region;
    };

    template <class SAMRecordT, class HaplotypeT, class IntervalT>
    std::vector<VariantT> assign_genotype_likelihoods(const std::vector<SAMRecordT>& reads,
                                                      const std::vector<HaplotypeT>& haplotypes,
                                                      const std::vector<std::vector<double>>& haplotype_likelihoods,
                                                      std::string_view ref, const IntervalT& padded_region,
                                                      const IntervalT& origin_region)
    {
        std::vector<Region<SAMRecordT, HaplotypeT, IntervalT>> one{
            {&reads, &haplotypes, &haplotype_likelihoods, ref, padded_region, origin_region}};
        return std::move(assign_many(one)[0]);
    }

    // Any number of regions in one device pass; one variant list per region.
    template <class SAMRecordT, class HaplotypeT, class IntervalT>
    std::vector<std::vector<VariantT>> assign_many(const std::vector<Region<SAMRecordT, HaplotypeT, IntervalT>>& regions)
    {
        const size_t n = regions.size();
        std::vector<hc_gt_region> rv(n);
        std::vector<std::vector<hc_gt_hap_aln>> haps(n);
        std::vector<std::vector<std::string>> cigars(n);
        std::vector<std::vector<int64_t>> rb(n), re(n);
        std::vector<std::vector<double>> flat(n);
        for (size_t k = 0; k < n; ++k) {
            const auto& x = regions[k];
            const size_t nh = x.haplotypes->size(), nr = x.reads->size();
            if (x.likelihoods->size() != nr) throw std::invalid_argument("hc_gt: one likelihood row per read");
            cigars[k].reserve(nh);
            haps[k].resize(nh);
            for (size_t h = 0; h < nh; ++h) {
                const auto& hap = (*x.haplotypes)[h];
                cigars[k].push_back(cigar_text(hap.cigar));
                haps[k][h].bases = reinterpret_cast<const uint8_t*>(hap.bases.data());
                haps[k][h].length = static_cast<int32_t>(hap.bases.size());
                haps[k][h].alignment_begin = static_cast<int32_t>(hap.alignment_begin_wrt_ref);
                haps[k][h].cigar = cigars[k][h].c_str();
            }
            rb[k].resize(nr);
            re[k].resize(nr);
            flat[k].reserve(nr * nh);
            for (size_t r = 0; r < nr; ++r) {
                const auto iv = (*x.reads)[r].get_interval();
                rb[k][r] = static_cast<int64_t>(iv.begin);
                re[k][r] = static_cast<int64_t>(iv.end);
                const auto& row = (*x.likelihoods)[r];
                if (row.size() != nh) throw std::invalid_argument("hc_gt: one likelihood per haplotype in every row");
                flat[k].insert(flat[k].end(), row.begin(), row.end());
            }
            hc_gt_region& g = rv[k];
            g.ref = reinterpret_cast<const uint8_t*>(x.ref.data());
            g.ref_len = static_cast<int32_t>(x.ref.size());
            g.padded_begin = static_cast<int64_t>(x.padded_region.begin);
            g.origin_begin = static_cast<int64_t>(x.origin_region.begin);
            g.origin_end = static_cast<int64_t>(x.origin_region.end);
            g.haps = haps[k].data();
            g.n_haps = static_cast<int32_t>(nh);
            g.read_begin = rb[k].data();
            g.read_end = re[k].data();
            g.n_reads = static_cast<int32_t>(nr);
            g.L = flat[k].data();
        }
        hc_gt_calls* calls = nullptr;
        const int rc = hc_gt_call_regions(rv.data(), static_cast<int32_t>(n), &calls);
        if (rc == HC_PHMM_EINVAL) throw std::invalid_argument(std::string("hc_gt: ") + hc_phmm_last_error());
        if (rc != HC_PHMM_OK) throw std::runtime_error(std::string("hc_gt: ") + hc_phmm_last_error());
        const hc_gt_call_site* sites = nullptr;
        int64_t ns = 0;
        hc_gt_calls_sites(calls, &sites, &ns);
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
        hc_gt_calls_free(calls);
        return out;
    }

private:
    template <class CigarT>
    static std::string cigar_text(const CigarT& c)
    {
        if constexpr (std::is_convertible_v<const CigarT&, std::string>) return c;
        else return c.to_string();
    }
};

}  // namespace hc
