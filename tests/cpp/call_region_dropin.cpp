// Program for tests/test_gpu_call_dropin.py (and compiled by test_call_capi.py):
// hc::MI355XReadPrep and hc::MI355XWindowCaller (include/hc_prep.hpp,
// include/hc_call.hpp) against stand-in types shaped like the reference's
// SAMRecord, Cigar, Haplotype, Interval and Variant.
//
//   call_region_dropin IN OUT
//
// IN:  n_windows, then per window "ref padded_begin padded_end origin_begin
//      origin_end n_reads" and per read "FLAG POS MAPQ CIGAR RNEXT SEQ QUAL".
// OUT, per window w:
//   "P w n"  then n lines "POS CIGAR SEQ QUAL"     reads after MI355XReadPrep::prepare
//   "C w status n_variants n_reads n_haps"         MI355XWindowCaller::call_region on a fresh copy
//   n_variants lines "V begin end gt1 gt2 gq allele..."
//   n_reads lines "POS CIGAR SEQ QUAL"
//   n_haps lines "H begin cigar bases"
// then "M w status n_variants n_reads" per window from one call_windows over all
// of them (the same again, in one pass).
#include <cctype>
#include <cstddef>
#include <fstream>
#include <iostream>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "hc_call.hpp"
#include "hc_prep.hpp"

enum class CigarOperator : char { M = 'M', I = 'I', D = 'D', N = 'N', S = 'S', H = 'H', P = 'P', EQ = '=', X = 'X' };
struct CigarElement {
    std::size_t length{};
    CigarOperator op{};
};
struct Cigar {
    std::vector<CigarElement> e;
    Cigar() = default;
    Cigar(const std::string& s)
    {
        for (std::size_t i = 0; i < s.size(); ++i) {
            std::size_t n = 0;
            for (; std::isdigit(static_cast<unsigned char>(s[i])); ++i) n = n * 10 + std::size_t(s[i] - '0');
            e.push_back({n, CigarOperator(s[i])});
        }
    }
    auto begin() const { return e.begin(); }
    auto end() const { return e.end(); }
    auto& front() { return e.front(); }
    auto& back() { return e.back(); }
    auto& front() const { return e.front(); }
    auto& back() const { return e.back(); }
    std::string to_string() const
    {
        std::string s;
        for (auto [n, op] : e) s += std::to_string(n) + char(op);
        return s;
    }
};
struct Interval {
    std::string contig;
    std::size_t begin = 0, end = 0;
};
struct SAMRecord {
    std::uint16_t FLAG = 0;
    std::uint32_t POS = 0;
    std::uint16_t MAPQ = 0;
    Cigar CIGAR;
    std::string RNEXT, SEQ, QUAL;
};
struct Haplotype {
    std::string bases;
    double score = 0;
    std::size_t alignment_begin_wrt_ref = 0;
    std::string cigar;
    Haplotype(std::string b, double s) : bases(std::move(b)), score(s) {}
};
struct Variant {
    Interval loc;
    std::vector<std::string> alleles;
    std::pair<std::size_t, std::size_t> gt;
    std::size_t gq;
    Variant(Interval l, std::vector<std::string> a, std::pair<std::size_t, std::size_t> g, std::size_t q)
        : loc(std::move(l)), alleles(std::move(a)), gt(g), gq(q) {}
};

struct Win {
    std::string ref;
    Interval padded, origin;
    std::vector<SAMRecord> reads;
};

static void print_reads(std::ostream& os, const std::vector<SAMRecord>& reads)
{
    for (const auto& r : reads) os << r.POS << ' ' << r.CIGAR.to_string() << ' ' << r.SEQ << ' ' << r.QUAL << '\n';
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    int n = 0;
    if (!(in >> n)) return 2;
    std::vector<Win> wins(static_cast<std::size_t>(n));
    for (auto& w : wins) {
        int nr = 0;
        w.padded.contig = w.origin.contig = "chr";
        if (!(in >> w.ref >> w.padded.begin >> w.padded.end >> w.origin.begin >> w.origin.end >> nr)) return 2;
        w.reads.resize(static_cast<std::size_t>(nr));
        for (auto& r : w.reads) {
            std::string cigar;
            if (!(in >> r.FLAG >> r.POS >> r.MAPQ >> cigar >> r.RNEXT >> r.SEQ >> r.QUAL)) return 2;
            r.CIGAR = Cigar(cigar);
        }
    }
    try {
        hc::MI355XReadPrep prep;
        hc::MI355XWindowCaller<Variant, Haplotype> caller;
        for (int w = 0; w < n; ++w) {
            auto reads = wins[std::size_t(w)].reads;
            prep.prepare(reads, wins[std::size_t(w)].padded);
            out << "P " << w << ' ' << reads.size() << '\n';
            print_reads(out, reads);
            reads = wins[std::size_t(w)].reads;
            const auto variants = caller.call_region(reads, std::string_view{wins[std::size_t(w)].ref},
                                                     wins[std::size_t(w)].padded, wins[std::size_t(w)].origin);
            out << "C " << w << ' ' << caller.status() << ' ' << variants.size() << ' ' << reads.size() << ' '
                << caller.haplotypes().size() << '\n';
            for (const auto& v : variants) {
                out << "V " << v.loc.begin << ' ' << v.loc.end << ' ' << v.gt.first << ' ' << v.gt.second << ' ' << v.gq;
                for (const auto& a : v.alleles) out << ' ' << a;
                out << '\n';
            }
            print_reads(out, reads);
            for (const auto& h : caller.haplotypes())
                out << "H " << h.alignment_begin_wrt_ref << ' ' << (h.cigar.empty() ? "*" : h.cigar) << ' ' << h.bases << '\n';
        }
        std::vector<hc::MI355XWindowCaller<Variant, Haplotype>::Window<SAMRecord, Interval>> many;
        for (auto& w : wins) many.push_back({&w.reads, std::string_view{w.ref}, w.padded, w.origin});
        const auto all = caller.call_windows(many);
        for (int w = 0; w < n; ++w)
            out << "M " << w << ' ' << caller.status(std::size_t(w)) << ' ' << all[std::size_t(w)].size() << ' '
                << wins[std::size_t(w)].reads.size() << '\n';
    } catch (const std::exception& e) {
        std::cerr << e.what() << '\n';
        return 1;
    }
    return 0;
}
