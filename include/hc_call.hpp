// hc_call.hpp — C++ drop-in for the whole of HaplotypeCaller::call_region.
//
// The driver's call_region (src/haplotypecaller/haplotypecaller.hpp:83-107)
// filters and clips the reads, assembles, computes the likelihoods, genotypes
// and prints the variants. With
//
//     hc::MI355XWindowCaller<Variant, Haplotype> caller;
//     for (const auto& variant : caller.call_region(reads, ref, padded_region, origin_region))
//         variant.print(os);
//
// its body is one call of libhcpairhmm.so (hc_call_windows, hc_call.h), with the
// same variants, and `reads` left as lines 93-103 leave it: filtered, clipped,
// and in a window that reaches the PairHMM without the poorly modelled reads. A
// window that ends early (no read left, at most one haplotype) gives no variant,
// as the two returns of the reference do. call_windows takes any number of
// windows in one pass; status() and haplotypes() describe the last call.
//
// Header-only; templated on the caller's types so it needs no reference header:
//   SAMRecord  as hc_prep.hpp needs it
//   Haplotype  constructible from (std::string, double), with
//              .alignment_begin_wrt_ref and a .cigar assignable from std::string
//   Variant    constructible from (Interval, std::vector<std::string>,
//              std::pair<std::size_t, std::size_t>, std::size_t)
//   Interval   {contig, begin, end}
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "hc_call.h"
#include "hc_prep.hpp"

namespace hc {

template <class VariantT, class HaplotypeT>
class MI355XWindowCaller {
public:
    // use_double: the PairHMM's per-instance mode, as hc::MI355XRegionCaller's.
    explicit MI355XWindowCaller(int device = -1, bool use_double = false) : device_(device), use_double_(use_double) {}

    // One window of a batch for call_windows(): reads are updated in place.
    template <class SAMRecordT, class IntervalT>
    struct Window {
        std::vector<SAMRecordT>* reads;
        std::string_view ref;
        IntervalT padded_region, origin_region;
    };

    template <class SAMRecordT, class IntervalT>
    std::vector<VariantT> call_region(std::vector<SAMRecordT>& reads, std::string_view ref, const IntervalT& padded_region,
                                      const IntervalT& origin_region)
    {
        std::vector<Window<SAMRecordT, IntervalT>> one{{&reads, ref, padded_region, origin_region}};
        return std::move(call_windows(one)[0]);
    }

    template <class SAMRecordT, class IntervalT>
    std::vector<std::vector<VariantT>> call_windows(const std::vector<Window<SAMRecordT, IntervalT>>& windows)
    {
        const size_t n = windows.size();
        std::vector<hc_call_window> wv(n);
        std::vector<std::vector<hc_prep_read>> reads(n);
        std::vector<std::vector<uint32_t>> words(n);
        std::vector<std::vector<const uint8_t*>> bases(n), quals(n);
        for (size_t k = 0; k < n; ++k) {
            const auto& x = windows[k];
            prep_detail::fill(*x.reads, reads[k], words[k]);
            bases[k].reserve(x.reads->size());
            quals[k].reserve(x.reads->size());
            for (const auto& rec : *x.reads) {
                bases[k].push_back(reinterpret_cast<const uint8_t*>(rec.SEQ.data()));
                quals[k].push_back(reinterpret_cast<const uint8_t*>(rec.QUAL.data()));
            }
            hc_call_window& g = wv[k];
            g.ref = reinterpret_cast<const uint8_t*>(x.ref.data());
            g.ref_len = static_cast<int32_t>(x.ref.size());
            g.padded_begin = static_cast<int64_t>(x.padded_region.begin);
            g.padded_end = static_cast<int64_t>(x.padded_region.end);
            g.origin_begin = static_cast<int64_t>(x.origin_region.begin);
            g.origin_end = static_cast<int64_t>(x.origin_region.end);
            g.reads = reads[k].data();
            g.bases = bases[k].data();
            g.quals = quals[k].data();
            g.n_reads = static_cast<int32_t>(reads[k].size());
        }
        prep_detail::check(hc_phmm_init(HC_PHMM_FLAG_KEEP_MODE, device_), "hc_call: ");   // device only: the mode goes with the call
        hc_call_result* res = nullptr;
        const uint32_t flags = (use_double_ ? HC_CALL_F64 : 0u) | HC_CALL_WANT_CIGARS;
        prep_detail::check(hc_call_windows(wv.data(), static_cast<int32_t>(n), flags, &res), "hc_call: ");
        Holder hold{res};

        std::vector<std::vector<VariantT>> out(n);
        const hc_gt_call_site* sites = nullptr;
        int64_t ns = 0;
        prep_detail::check(hc_call_result_sites(res, &sites, &ns), "hc_call: ");
        for (int64_t s = 0; s < ns; ++s) {
            const hc_gt_call_site& c = sites[s];
            if (c.status != HC_GT_SITE_EMITTED) continue;
            const auto& x = windows[static_cast<size_t>(c.region)];
            std::vector<std::string> alleles(c.alleles, c.alleles + c.n_alleles);
            IntervalT loc{x.padded_region.contig, static_cast<std::size_t>(c.begin), static_cast<std::size_t>(c.loc_end)};
            out[static_cast<size_t>(c.region)].emplace_back(
                std::move(loc), std::move(alleles),
                std::pair<std::size_t, std::size_t>(static_cast<std::size_t>(c.a1), static_cast<std::size_t>(c.a2)),
                static_cast<std::size_t>(c.genotype_quality));
        }
        status_.assign(n, HC_CALL_NO_READS);
        haplotypes_.assign(n, {});
        for (size_t k = 0; k < n; ++k) {
            const int32_t w = static_cast<int32_t>(k);
            int32_t n_haps = 0;
            prep_detail::check(hc_call_result_window(res, w, &status_[k], nullptr, nullptr, &n_haps), "hc_call: ");
            for (int32_t h = 0; h < n_haps; ++h) {
                const uint8_t* b = nullptr;
                const char* cigar = nullptr;
                int32_t length = 0, begin = 0;
                double score = 0;
                prep_detail::check(hc_call_result_hap(res, w, h, &b, &length, &score, &begin, &cigar), "hc_call: ");
                haplotypes_[k].emplace_back(std::string(reinterpret_cast<const char*>(b), static_cast<size_t>(length)), score);
                if (cigar) {
                    haplotypes_[k].back().alignment_begin_wrt_ref = static_cast<std::size_t>(begin);
                    haplotypes_[k].back().cigar = std::string(cigar);
                }
            }
            const hc_prep_record* rec = nullptr;
            const int32_t* left = nullptr;
            int32_t n_left = 0;
            prep_detail::check(hc_call_result_prep(res, w, &rec, nullptr, nullptr, nullptr, nullptr), "hc_call: ");
            prep_detail::check(hc_call_result_reads(res, w, &left, &n_left), "hc_call: ");
            prep_detail::keep_only(*windows[k].reads, rec, left, n_left);
        }
        return out;
    }

    // Of the last call: HC_CALL_CALLED, HC_CALL_NO_READS or HC_CALL_NO_VARIATION, and the assembled
    // haplotypes (aligned only in a HC_CALL_CALLED window, where the reference's caller would see them).
    int status(std::size_t window = 0) const { return status_.at(window); }
    const std::vector<HaplotypeT>& haplotypes(std::size_t window = 0) const { return haplotypes_.at(window); }

private:
    struct Holder {
        hc_call_result* p;
        ~Holder() { hc_call_result_free(p); }
    };
    int device_;
    bool use_double_;
    std::vector<int32_t> status_;
    std::vector<std::vector<HaplotypeT>> haplotypes_;
};

}  // namespace hc
