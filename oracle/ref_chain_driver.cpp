// Driver around the REFERENCE's region chain: TEST INFRASTRUCTURE ONLY.
//
// Compiled by oracle/Makefile (target `ref`) into oracle/_ref/libref_chain.so,
// directly against the reference headers where they lie: sam/sam.hpp,
// utils/read_filter.hpp, utils/read_clipper.hpp,
// smithwaterman/intel_smithwaterman.hpp, pairhmm/intel_pairhmm.hpp and
// genotyper/genotyper.hpp. No reference source is copied into this repository.
// The three Boost.Serialization headers those files include (and use nothing
// of) are answered by oracle/boost_standin/, which holds standard includes only.
// assembler/graph_wrapper.hpp needs Boost.Graph for real: the assembler is
// compiled by ref_asm_driver.cpp, over a stand-in container of its own, and
// haplotypecaller.hpp (which includes it) is not compiled at all.
//
// What this file restates, because it lies in haplotypecaller.hpp or inside one
// reference function and cannot be called: the ORCHESTRATION only, marked
// "restated orchestration" below. Every statement that computes something is
// the reference's own, called through its headers.
//
// Private members (Genetyper's per-site steps and constants, IntelPairHMM's
// computeLikelihoodsNative) are reached by compiling this one file with
// -fno-access-control: it changes no generated code, and it is the only way to
// the per-site intermediates of Genetyper.
//
// C ABI: every hcr_* entry writes a little-endian blob (int64 / double / length
// -prefixed bytes, see class Out) into a caller buffer and returns the number
// of bytes, HCR_THREW (-1) when the reference threw a std::exception,
// HCR_SMALL (-2) when the buffer is too small, HCR_BAD_INPUT (-3) for input the
// driver refuses because the reference would abort() or read outside its
// buffers on it (an RNAME other than the contig's trips an assert; a read
// longer than SAMRecord::MAX_READ_LENGTH reads past the static GOP string).
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <exception>
#include <functional>
#include <iostream>
#include <istream>
#include <iterator>
#include <limits>
#include <map>
#include <memory>
#include <numeric>
#include <ostream>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <string_view>
#include <tuple>
#include <utility>
#include <vector>
#include <immintrin.h>
#include <x86intrin.h>
#include <xmmintrin.h>
#include <stdio.h>
#include <string.h>
#include <omp.h>

#include "sam/sam.hpp"
#include "utils/read_filter.hpp"
#include "utils/read_clipper.hpp"
#include "smithwaterman/intel_smithwaterman.hpp"
#include "pairhmm/intel_pairhmm.hpp"
#include "genotyper/genotyper.hpp"

namespace {

constexpr long HCR_THREW = -1, HCR_SMALL = -2, HCR_BAD_INPUT = -3;
const char* const CONTIG = "c";

class Out {
public:
    Out(uint8_t* p, long cap) : p_(p), cap_(cap) {}
    void i64(int64_t v) { put(&v, 8); }
    void u64(uint64_t v) { put(&v, 8); }
    void f64(double v) { put(&v, 8); }
    void str(std::string_view s) { i64(int64_t(s.size())); put(s.data(), long(s.size())); }
    long mark() const { return n_; }
    void rewind(long m) { n_ = m; }
    long done() const { return n_ > cap_ ? HCR_SMALL : n_; }
private:
    void put(const void* src, long n)
    {
        if (n_ + n <= cap_) std::memcpy(p_ + n_, src, size_t(n));
        n_ += n;
    }
    uint8_t* p_;
    long cap_, n_ = 0;
};

// Reads arrive as SAM text, one line each, and go through the reference's own
// operator>>. QNAME is the read's index in the call, so that a read can be
// followed through the reference's erase-remove steps.
bool parse_reads(const char* sam, std::vector<hc::SAMRecord>& reads)
{
    std::istringstream all{std::string(sam)};
    std::string line;
    while (std::getline(all, line)) {
        std::istringstream iss(line);
        hc::SAMRecord r{};
        iss >> r;
        if (iss.fail() || r.RNAME != CONTIG || r.SEQ.size() > hc::SAMRecord::MAX_READ_LENGTH) return false;
        reads.push_back(std::move(r));
    }
    return true;
}

// Haplotypes arrive as lines "BASES BEGIN CIGAR" (CIGAR "-" : not aligned yet).
void parse_haps(const char* text, std::vector<hc::Haplotype>& haps)
{
    std::istringstream all{std::string(text)};
    std::string bases, cigar;
    std::size_t begin;
    while (all >> bases >> begin >> cigar) {
        hc::Haplotype h(bases, 0.0);
        h.alignment_begin_wrt_ref = begin;
        if (cigar != "-") h.cigar = cigar;
        haps.push_back(std::move(h));
    }
}

enum Reason { KEPT = 0, MAPQ = 1, DUPLICATE = 2, SECONDARY = 3, MATE_CONTIG = 4, MIN_LENGTH = 5 };

// RESTATED ORCHESTRATION of haplotypecaller.hpp:52-81 (filter_reads and
// hard_clip_reads are private members of a class that cannot be compiled
// here): the four remove_ifs, the two for_eachs and the last remove_if, in
// that order, over the reference's own predicates and ReadClipper.
template <class Pred>
void remove_reads(std::vector<hc::SAMRecord>& reads, std::vector<int>& reason, Reason why, Pred pred)
{
    for (const auto& r : reads)
        if (pred(r)) reason[std::stoul(r.QNAME)] = why;
    reads.erase(std::remove_if(reads.begin(), reads.end(), pred), reads.end());
}

void prepare(std::vector<hc::SAMRecord>& reads, const hc::Interval& padded, std::vector<int>& reason)
{
    reason.assign(reads.size(), KEPT);
    remove_reads(reads, reason, MAPQ, hc::MappingQualityReadFilter{});
    remove_reads(reads, reason, DUPLICATE, hc::DuplicateReadFilter{});
    remove_reads(reads, reason, SECONDARY, hc::SecondaryAlignmentReadFilter{});
    remove_reads(reads, reason, MATE_CONTIG, hc::MateOnSameContigReadFilter{});
    for (hc::SAMRecord& r : reads) hc::ReadClipper::revert_soft_clipped_bases(r);   // every read, then
    for (hc::SAMRecord& r : reads) hc::ReadClipper::hard_clip_to_interval(r, padded);   // every read again
    remove_reads(reads, reason, MIN_LENGTH, hc::MinimumLengthReadFilter{});
}

// graph_wrapper.hpp:232-240 (RESTATED ORCHESTRATION: the loop, not the aligner).
void align_haplotypes(std::vector<hc::Haplotype>& haps, std::string_view ref)
{
    hc::IntelSWAligner aligner;
    for (hc::Haplotype& h : haps) {
        std::pair<size_t, hc::Cigar> placed = aligner.align(ref, h.bases);
        h.alignment_begin_wrt_ref = placed.first;
        h.cigar = std::move(placed.second);
    }
}

// One thread: initNative() switches flush-to-zero on for the calling thread
// only, so with one thread every pair is computed under the mode it sets. The
// caller's MXCSR is put back afterwards.
struct OneThreadFtzGuard {
    unsigned csr = _mm_getcsr();
    int threads = omp_get_max_threads();
    OneThreadFtzGuard() { omp_set_num_threads(1); }
    ~OneThreadFtzGuard() { omp_set_num_threads(threads); _mm_setcsr(csr); }
};

void write_variants(Out& o, const std::vector<hc::Variant>& variants)
{
    o.i64(int64_t(variants.size()));
    for (const auto& v : variants) {
        o.u64(v.location.begin);
        o.u64(v.location.end);
        o.i64(int64_t(v.alleles.size()));
        for (const auto& a : v.alleles) o.str(a);
        o.i64(int64_t(v.GT.first));
        o.i64(int64_t(v.GT.second));
        o.i64(int64_t(v.GQ));
        std::ostringstream os;
        v.print(os);
        o.str(os.str());
    }
}

long guarded(Out& o, const std::function<long()>& body)
{
    try {
        const long rc = body();
        return rc < 0 ? rc : o.done();
    } catch (const std::exception&) {
        return HCR_THREW;
    }
}

}  // namespace

extern "C" {

// One SAM line through operator>>(istream&, SAMRecord&). Blob: fail bit, FLAG,
// POS, MAPQ, n CIGAR elements, (length, op) each, RNEXT, PNEXT, TLEN, SEQ, QUAL.
long hcr_parse(const char* line, long len, uint8_t* out, long cap)
{
    Out o(out, cap);
    return guarded(o, [&]() -> long {
        std::istringstream iss(std::string(line, size_t(len)));
        hc::SAMRecord r{};
        iss >> r;
        o.i64(iss.fail() ? 1 : 0);
        o.i64(r.FLAG);
        o.i64(r.POS);
        o.i64(r.MAPQ);
        o.i64(std::distance(r.CIGAR.begin(), r.CIGAR.end()));
        for (auto [length, op] : r.CIGAR) {
            o.u64(length);
            o.i64(int64_t(uint8_t(op)));
        }
        o.str(r.RNEXT);
        o.i64(r.PNEXT);
        o.i64(r.TLEN);
        o.str(r.SEQ);
        o.str(r.QUAL);
        return 0;
    });
}

// filter_reads + hard_clip_reads on one window's reads. Blob: n reads, then per
// input read: reason, POS, CIGAR text, SEQ, QUAL (as the read was when it left
// or, for a survivor, as it ended).
long hcr_prepare(const char* sam, uint64_t begin, uint64_t end, uint8_t* out, long cap)
{
    Out o(out, cap);
    return guarded(o, [&]() -> long {
        std::vector<hc::SAMRecord> reads;
        if (!parse_reads(sam, reads)) return HCR_BAD_INPUT;
        const std::vector<hc::SAMRecord> before = reads;
        std::vector<int> reason;
        prepare(reads, hc::Interval(CONTIG, begin, end), reason);
        std::map<std::size_t, const hc::SAMRecord*> left;
        for (const auto& r : reads) left[std::stoul(r.QNAME)] = &r;
        o.i64(int64_t(before.size()));
        for (std::size_t k = 0; k < before.size(); ++k) {
            o.i64(reason[k]);
            o.i64(left.count(k));
            if (!left.count(k)) continue;   // an erased read's last state is gone with it
            const hc::SAMRecord& r = *left[k];
            o.i64(r.POS);
            o.str(r.CIGAR.to_string());
            o.str(r.SEQ);
            o.str(r.QUAL);
        }
        return 0;
    });
}

// IntelSWAligner::align(ref, alt, params). Blob: offset, CIGAR text.
long hcr_align(const char* ref, long ref_len, const char* alt, long alt_len, int w_match, int w_mismatch,
               int w_open, int w_extend, uint8_t* out, long cap)
{
    Out o(out, cap);
    return guarded(o, [&]() -> long {
        hc::IntelSWAligner aligner;
        auto [offset, cigar] = aligner.align(std::string_view(ref, size_t(ref_len)), std::string_view(alt, size_t(alt_len)),
                                             hc::IntelSWAligner::SWParameters{w_match, w_mismatch, w_open, w_extend});
        o.u64(offset);
        o.str(cigar.to_string());
        return 0;
    });
}

// IntelPairHMM::compute_likelihoods(haplotypes, reads). Blob: n reads, n haps,
// the matrix before normalisation (computeLikelihoodsNative, read-major), then
// the number of surviving reads, their indices and the returned matrix.
long hcr_likelihoods(const char* sam, const char* haps_text, uint8_t* out, long cap)
{
    Out o(out, cap);
    return guarded(o, [&]() -> long {
        std::vector<hc::SAMRecord> reads;
        std::vector<hc::Haplotype> haps;
        if (!parse_reads(sam, reads)) return HCR_BAD_INPUT;
        parse_haps(haps_text, haps);
        if (reads.empty() || haps.empty()) return HCR_BAD_INPUT;   // testcases[0] / max_element of nothing
        OneThreadFtzGuard guard;
        o.i64(int64_t(reads.size()));
        o.i64(int64_t(haps.size()));
        {
            hc::IntelPairHMM raw;
            raw.initNative();
            std::vector<std::vector<double>> L(reads.size(), std::vector<double>(haps.size()));
            raw.computeLikelihoodsNative(reads, haps, L);
            for (const auto& row : L)
                for (double v : row) o.f64(v);
        }
        hc::IntelPairHMM pairhmm;
        auto L = pairhmm.compute_likelihoods(haps, reads);
        o.i64(int64_t(reads.size()));
        for (const auto& r : reads) o.i64(int64_t(std::stoul(r.QNAME)));
        for (const auto& row : L)
            for (double v : row) o.f64(v);
        return 0;
    });
}

// IntelPairHMM::normalize_likelihoods_and_filter_poorly_modeled_reads alone, on
// a matrix handed in (n reads x n_haps, read-major): thresholds and caps that no
// real read reaches bit for bit. Blob: number of surviving reads, their
// indices, the matrix left.
long hcr_normalize(const char* sam, long n_haps, const double* L, uint8_t* out, long cap)
{
    Out o(out, cap);
    return guarded(o, [&]() -> long {
        std::vector<hc::SAMRecord> reads;
        if (!parse_reads(sam, reads)) return HCR_BAD_INPUT;
        if (n_haps <= 0) return HCR_BAD_INPUT;   // max_element of an empty row
        std::vector<std::vector<double>> lik(reads.size(), std::vector<double>(size_t(n_haps)));
        for (std::size_t r = 0; r < reads.size(); ++r)
            for (long h = 0; h < n_haps; ++h) lik[r][size_t(h)] = L[r * size_t(n_haps) + size_t(h)];
        hc::IntelPairHMM pairhmm;
        pairhmm.normalize_likelihoods_and_filter_poorly_modeled_reads(reads, lik);
        o.i64(int64_t(reads.size()));
        for (const auto& r : reads) o.i64(int64_t(std::stoul(r.QNAME)));
        for (const auto& row : lik)
            for (double v : row) o.f64(v);
        return 0;
    });
}

// Genetyper::assign_genotype_likelihoods. Blob:
//   whole call: threw (0/1), then (if it did not) the Variants: begin, end,
//     alleles, GT, GQ and Variant::print's text;
//   per site of events_begins inside the origin (RESTATED ORCHESTRATION of
//     genotyper.hpp:379-394, every step the reference's own private member):
//     begin, threw (0/1), and if not: loc begin, loc end, n alleles, alleles,
//     then for <= MAX_ALLELE_COUNT alleles haplotype_mapper, read_indices_to_keep,
//     the genotype likelihoods, genotype index and quality.
long hcr_genotype(const char* sam, const char* haps_text, const double* L, const char* ref, long ref_len,
                  uint64_t padded_begin, uint64_t padded_end, uint64_t origin_begin, uint64_t origin_end,
                  uint8_t* out, long cap)
{
    Out o(out, cap);
    return guarded(o, [&]() -> long {
        std::vector<hc::SAMRecord> reads;
        std::vector<hc::Haplotype> haps0;
        if (!parse_reads(sam, reads)) return HCR_BAD_INPUT;
        parse_haps(haps_text, haps0);
        std::vector<std::vector<double>> lik(reads.size(), std::vector<double>(haps0.size()));
        for (std::size_t r = 0; r < reads.size(); ++r)
            for (std::size_t h = 0; h < haps0.size(); ++h) lik[r][h] = L[r * haps0.size() + h];
        const std::string_view window(ref, size_t(ref_len));
        const hc::Interval padded(CONTIG, padded_begin, padded_end), origin(CONTIG, origin_begin, origin_end);

        {
            auto haps = haps0;
            hc::Genetyper g;
            const long at = o.mark();
            try {
                o.i64(0);
                write_variants(o, g.assign_genotype_likelihoods(reads, haps, lik, window, padded, origin));
            } catch (const std::exception&) {
                o.rewind(at);
                o.i64(1);
            }
        }

        auto haps = haps0;
        hc::Genetyper g;
        const std::set<std::size_t> all_begins = g.set_events_for_haplotypes(haps, window, padded);
        std::vector<std::size_t> inside;   // :381, the origin's half-open range
        for (std::size_t b : all_begins)
            if (b >= origin_begin && b < origin_end) inside.push_back(b);
        o.i64(int64_t(inside.size()));
        for (auto begin : inside) {
            o.u64(begin);
            const long at = o.mark();
            try {
                o.i64(0);
                std::vector<hc::Variant> evs = g.get_events_from_haplotypes(begin, haps);
                g.replace_span_dels(evs, window[begin - padded.begin], begin);
                auto site = g.get_compatible_alleles(evs);   // (alleles, location)
                const std::vector<std::string>& names = site.first;
                hc::Interval& loc = site.second;
                o.u64(loc.begin);
                o.u64(loc.end);
                o.i64(int64_t(names.size()));
                for (const std::string& a : names) o.str(a);
                if (names.size() > hc::Genetyper::MAX_ALLELE_COUNT) continue;
                const auto by_allele = g.get_allele_mapper(names, begin, haps);
                const auto hap_to_allele = g.get_haplotype_mapper(by_allele, haps.size());
                const hc::Interval widened = loc.expand_within_contig(hc::Genetyper::ALLELE_EXTENSION);   // may throw
                const auto kept = g.get_read_indices_to_keep(reads, widened);
                const auto per_allele = g.marginalize(hap_to_allele, names.size(), reads, lik, widened);
                const std::vector<double> gl = g.calculate_genotype_likelihoods(per_allele, names.size());
                const auto best = g.get_genotype_quality_and_max_genotype_index(gl);   // (index, quality)
                for (std::size_t a : hap_to_allele) o.i64(int64_t(a));
                o.i64(int64_t(kept.size()));
                for (std::size_t k : kept) o.i64(int64_t(k));
                for (double v : gl) o.f64(v);
                o.i64(int64_t(best.first));
                o.i64(int64_t(best.second));
            } catch (const std::exception&) {
                o.rewind(at);
                o.i64(1);
            }
        }
        return 0;
    });
}

// One site's arithmetic on maps handed in: marginal_likelihoods,
// calculate_genotype_likelihoods and get_genotype_quality_and_max_genotype_index
// (genotyper.hpp:245-362). Blob: the genotype likelihoods, index, quality.
long hcr_gt_site(const double* L, long n_reads, long n_haps, const int32_t* keep, long n_keep, const int32_t* hap_allele,
                 long n_alleles, uint8_t* out, long cap)
{
    Out o(out, cap);
    return guarded(o, [&]() -> long {
        if (n_alleles < 2 || n_haps <= 0) return HCR_BAD_INPUT;   // genotypes[1] is read unconditionally
        const std::size_t nr = std::size_t(n_reads), nh = std::size_t(n_haps);
        std::vector<std::vector<double>> lik(nr, std::vector<double>(nh));
        for (long r = 0; r < n_reads; ++r)
            for (long h = 0; h < n_haps; ++h) lik[size_t(r)][size_t(h)] = L[r * n_haps + h];
        std::vector<std::size_t> mapper(hap_allele, hap_allele + n_haps), kept(keep, keep + n_keep);
        hc::Genetyper g;
        auto allele_likelihoods = g.marginal_likelihoods(size_t(n_alleles), mapper, kept, lik);
        auto genotype_likelihoods = g.calculate_genotype_likelihoods(allele_likelihoods, size_t(n_alleles));
        auto [genotype_index, genotype_quality] = g.get_genotype_quality_and_max_genotype_index(genotype_likelihoods);
        for (double v : genotype_likelihoods) o.f64(v);
        o.i64(int64_t(genotype_index));
        o.i64(int64_t(genotype_quality));
        return 0;
    });
}

// Lines 93-106 of HaplotypeCaller::call_region with the haplotype bases handed
// in where the assembler would make them (RESTATED ORCHESTRATION: the sequence
// of calls and the two early returns). Blob: outcome (0 called, 1 no reads
// left, 2 at most one haplotype), then for outcome 0 the number of reads the
// likelihood filter left, and the Variants as hcr_genotype writes them.
long hcr_chain(const char* sam, const char* haps_text, const char* ref, long ref_len, uint64_t padded_begin,
               uint64_t padded_end, uint64_t origin_begin, uint64_t origin_end, uint8_t* out, long cap)
{
    Out o(out, cap);
    return guarded(o, [&]() -> long {
        std::vector<hc::SAMRecord> reads;
        std::vector<hc::Haplotype> haps;
        if (!parse_reads(sam, reads)) return HCR_BAD_INPUT;
        parse_haps(haps_text, haps);
        const std::string_view window(ref, size_t(ref_len));
        const hc::Interval padded(CONTIG, padded_begin, padded_end), origin(CONTIG, origin_begin, origin_end);
        std::vector<int> reason;
        prepare(reads, padded, reason);
        if (reads.empty()) { o.i64(1); return 0; }
        align_haplotypes(haps, window);
        if (haps.size() <= 1) { o.i64(2); return 0; }
        OneThreadFtzGuard guard;
        hc::IntelPairHMM pairhmm;
        hc::Genetyper genetyper;
        const std::vector<std::vector<double>> lik = pairhmm.compute_likelihoods(haps, reads);
        const std::vector<hc::Variant> called = genetyper.assign_genotype_likelihoods(reads, haps, lik, window, padded, origin);
        o.i64(0);
        o.i64(int64_t(reads.size()));
        write_variants(o, called);
        return 0;
    });
}

}  // extern "C"
