// hc_prep.hpp — C++ drop-in for the read preparation of HaplotypeCaller::call_region.
//
// The driver (src/haplotypecaller/haplotypecaller.hpp:83-107) begins with
//
//     filter_reads(reads);                        // :93
//     hard_clip_reads(reads, padded_region);      // :94
//
// Replacing both lines with
//
//     hc::MI355XReadPrep prep;
//     prep.prepare(reads, padded_region);
//
// leaves `reads` exactly as the reference would: the same survivors in the same
// order, SEQ and QUAL clipped, POS and the CIGAR's first or last element
// rewritten where revert_soft_clipped_bases did so (the hard clip moves neither).
// One call of libhcpairhmm.so (hc_prep_reads, hc_prep.h); prepare_many takes any
// number of windows in one device pass. No base or quality byte leaves the host.
//
// Header-only; templated on the caller's types so it needs no reference header:
//   SAMRecord  .FLAG .MAPQ .POS .RNEXT .SEQ .QUAL, and .CIGAR iterable as
//              {length, op} elements (op a char or an enum over 'M' 'I' 'D' ..)
//              with assignable front() / back()
//   Interval   .begin .end
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "hc_prep.h"

namespace hc {

namespace prep_detail {

inline uint32_t op_code(char c)
{
    switch (c) {
        case 'M': return 0;
        case 'I': return 1;
        case 'D': return 2;
        case 'N': return 3;
        case 'S': return 4;
        case 'H': return 5;
        case 'P': return 6;
        case '=': return 7;
        case 'X': return 8;
        default: return 15;   // refused on the device, as an operator the reference does not know
    }
}

// The hc_prep_read of every record of `reads`; the packed words go to `words`
// (reserved up front, so the pointers taken into it stay valid).
template <class SAMRecordT>
void fill(const std::vector<SAMRecordT>& reads, std::vector<hc_prep_read>& out, std::vector<uint32_t>& words)
{
    size_t n_words = 0;
    for (const auto& rec : reads)
        for (auto it = rec.CIGAR.begin(); it != rec.CIGAR.end(); ++it) ++n_words;
    words.clear();
    words.reserve(n_words);
    out.resize(reads.size());
    for (size_t r = 0; r < reads.size(); ++r) {
        const auto& rec = reads[r];
        if (rec.QUAL.size() != rec.SEQ.size()) throw std::invalid_argument("hc_prep: a read whose QUAL and SEQ differ in length");
        hc_prep_read& d = out[r];
        d = hc_prep_read{};
        d.cigar = words.data() + words.size();
        for (const auto& e : rec.CIGAR) {
            const auto& [length, op] = e;
            if (static_cast<uint64_t>(length) >= (1ull << 28)) throw std::invalid_argument("hc_prep: a CIGAR length above 2^28 - 1");
            words.push_back(HC_PREP_CIGAR_WORD(length, op_code(static_cast<char>(op))));
            ++d.n_cigar;
        }
        d.pos = static_cast<uint32_t>(rec.POS);
        d.seq_len = static_cast<int32_t>(rec.SEQ.size());
        d.flag = static_cast<uint16_t>(rec.FLAG);
        d.mapq = static_cast<uint16_t>(rec.MAPQ);
        d.mate_same_contig = rec.RNEXT == "=" ? 1 : 0;
    }
}

// What the reference's two functions leave of a surviving read.
template <class SAMRecordT>
void apply(const hc_prep_record& p, SAMRecordT& rec)
{
    using Elem = std::decay_t<decltype(rec.CIGAR.front())>;
    using Op = std::decay_t<decltype(std::declval<Elem>().op)>;
    rec.SEQ = rec.SEQ.substr(static_cast<size_t>(p.offset), static_cast<size_t>(p.length));
    rec.QUAL = rec.QUAL.substr(static_cast<size_t>(p.offset), static_cast<size_t>(p.length));
    rec.POS = p.new_pos;
    if (p.front_to_M) rec.CIGAR.front() = Elem{rec.CIGAR.front().length, static_cast<Op>('M')};
    if (p.back_to_M) rec.CIGAR.back() = Elem{rec.CIGAR.back().length, static_cast<Op>('M')};
}

// Erases all but `kept` (ascending indices), applying records[j] to the survivors.
template <class SAMRecordT>
void keep_only(std::vector<SAMRecordT>& reads, const hc_prep_record* records, const int32_t* kept, int32_t n_kept)
{
    std::vector<SAMRecordT> survivors;
    survivors.reserve(static_cast<size_t>(n_kept));
    for (int32_t k = 0; k < n_kept; ++k) {
        SAMRecordT& rec = reads[static_cast<size_t>(kept[k])];
        if (records) apply(records[kept[k]], rec);
        survivors.push_back(std::move(rec));
    }
    reads.swap(survivors);
}

inline void check(int rc, const char* who)
{
    if (rc == HC_PHMM_EINVAL) throw std::invalid_argument(std::string(who) + hc_phmm_last_error());
    if (rc != HC_PHMM_OK) throw std::runtime_error(std::string(who) + hc_phmm_last_error());
}

}  // namespace prep_detail

class MI355XReadPrep {
public:
    explicit MI355XReadPrep(int device = -1) : device_(device) {}

    // One window of a batch for prepare_many(): reads are updated in place.
    template <class SAMRecordT, class IntervalT>
    struct Window {
        std::vector<SAMRecordT>* reads;
        IntervalT padded_region;
    };

    // filter_reads + hard_clip_reads.
    template <class SAMRecordT, class IntervalT>
    void prepare(std::vector<SAMRecordT>& reads, const IntervalT& padded_region)
    {
        std::vector<Window<SAMRecordT, IntervalT>> one{{&reads, padded_region}};
        prepare_many(one);
    }

    template <class SAMRecordT, class IntervalT>
    void prepare_many(const std::vector<Window<SAMRecordT, IntervalT>>& windows)
    {
        const size_t n = windows.size();
        std::vector<hc_prep_window> wv(n);
        std::vector<std::vector<hc_prep_read>> reads(n);
        std::vector<std::vector<uint32_t>> words(n);
        for (size_t k = 0; k < n; ++k) {
            prep_detail::fill(*windows[k].reads, reads[k], words[k]);
            wv[k] = hc_prep_window{static_cast<int64_t>(windows[k].padded_region.begin),
                                   static_cast<int64_t>(windows[k].padded_region.end), reads[k].data(),
                                   static_cast<int32_t>(reads[k].size())};
        }
        prep_detail::check(hc_phmm_init(HC_PHMM_FLAG_KEEP_MODE, device_), "hc_prep: ");
        hc_prep_result* res = nullptr;
        prep_detail::check(hc_prep_reads(wv.data(), static_cast<int32_t>(n), &res), "hc_prep: ");
        Holder hold{res};
        for (size_t k = 0; k < n; ++k) {
            const hc_prep_record* rec = nullptr;
            const int32_t* kept = nullptr;
            int32_t n_kept = 0;
            prep_detail::check(hc_prep_result_window(res, static_cast<int32_t>(k), &rec, nullptr, &kept, &n_kept, nullptr),
                               "hc_prep: ");
            prep_detail::keep_only(*windows[k].reads, rec, kept, n_kept);
        }
    }

private:
    struct Holder {
        hc_prep_result* p;
        ~Holder() { hc_prep_result_free(p); }
    };
    int device_;
};

}  // namespace hc
