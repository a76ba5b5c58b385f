// C++ drop-in check for include/hc_region.hpp: seeded regions go through
// hc::MI355XRegionCaller<Variant>::call_many, and through the three separate
// drop-ins in call_region's order (hc::MI355XSWAligner::align_haplotypes,
// hc::MI355XPairHMM::compute_likelihoods, hc::MI355XGenotyper::
// assign_genotype_likelihoods). Everything both produce is compared: alignment
// begins and CIGAR text, the surviving reads, the variants (location, alleles,
// genotype, quality). The mismatch counts are written as JSON; all must be zero.
//
// usage: region_call <in> <out.json>
// Input (region_workloads.write_regions): n_regions, then per region ref,
// padded_begin, origin_begin, origin_end (int64), n_haps, the haplotypes' bases,
// n_reads, per read bases, qualities, begin, end (int64); strings are int32
// length-prefixed.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <string_view>
#include <vector>

#include "hc_gt.hpp"
#include "hc_pairhmm.hpp"
#include "hc_region.hpp"
#include "hc_sw.hpp"

struct Interval {
    std::string contig;
    std::size_t begin = 0, end = 0;
};
struct Cigar {   // stand-in: assigned from text, gives it back as the reference's to_string()
    std::string text;
    Cigar() = default;
    Cigar(std::string t) : text(std::move(t)) {}
    std::string to_string() const { return text; }
};
struct Haplotype {
    std::string bases;
    std::size_t alignment_begin_wrt_ref = 0;
    Cigar cigar;
};
struct SAMRecord {
    std::string SEQ, QUAL;
    Interval iv;
    int id = 0;
    static inline const std::string GOP = std::string(256, 'I');   // sam.hpp:30-32
    static inline const std::string GCP = std::string(256, '+');
    std::string_view insertionGOP() const { return std::string_view{GOP}.substr(0, SEQ.size()); }
    std::string_view deletionGOP() const { return std::string_view{GOP}.substr(0, SEQ.size()); }
    std::string_view overallGCP() const { return std::string_view{GCP}.substr(0, SEQ.size()); }
    Interval get_interval() const { return iv; }
};
struct Variant {
    Interval location;
    std::vector<std::string> alleles;
    std::pair<std::size_t, std::size_t> GT;
    std::size_t GQ = 0;
    Variant(Interval loc, std::vector<std::string> al, std::pair<std::size_t, std::size_t> gt, std::size_t gq)
        : location(std::move(loc)), alleles(std::move(al)), GT(gt), GQ(gq) {}
    bool same(const Variant& o) const
    {
        return location.begin == o.location.begin && location.end == o.location.end && alleles == o.alleles && GT == o.GT &&
               GQ == o.GQ;
    }
};

struct RegionIn {
    std::string ref;
    Interval padded, origin;
    std::vector<Haplotype> haplotypes;
    std::vector<SAMRecord> reads;
};

template <class T>
static T rd(std::ifstream& in)
{
    T v{};
    in.read(reinterpret_cast<char*>(&v), sizeof(T));
    return v;
}

static std::string rds(std::ifstream& in)
{
    std::string s(static_cast<size_t>(rd<int32_t>(in)), 0);
    in.read(s.data(), static_cast<std::streamsize>(s.size()));
    return s;
}

static std::vector<RegionIn> load(const char* path)
{
    std::ifstream in(path, std::ios::binary);
    std::vector<RegionIn> out(static_cast<size_t>(rd<int32_t>(in)));
    for (auto& r : out) {
        r.ref = rds(in);
        const auto pb = static_cast<std::size_t>(rd<int64_t>(in));
        const auto ob = static_cast<std::size_t>(rd<int64_t>(in));
        const auto oe = static_cast<std::size_t>(rd<int64_t>(in));
        r.padded = {"chr1", pb, pb + r.ref.size()};
        r.origin = {"chr1", ob, oe};
        r.haplotypes.resize(static_cast<size_t>(rd<int32_t>(in)));
        for (auto& h : r.haplotypes) h.bases = rds(in);
        r.reads.resize(static_cast<size_t>(rd<int32_t>(in)));
        int id = 0;
        for (auto& x : r.reads) {
            x.SEQ = rds(in);
            x.QUAL = rds(in);
            x.iv.begin = static_cast<std::size_t>(rd<int64_t>(in));
            x.iv.end = static_cast<std::size_t>(rd<int64_t>(in));
            x.id = id++;
        }
    }
    return out;
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::vector<RegionIn> input = load(argv[1]);
    long n_haps = 0, n_reads = 0, n_kept = 0, n_variants = 0;
    long bad_sw = 0, bad_keep = 0, bad_variants = 0, bad_passed_in = 0;

    // The three drop-ins, region by region, in call_region's order.
    std::vector<RegionIn> sep = input;
    std::vector<std::vector<Variant>> sep_variants;
    hc::MI355XSWAligner aligner(0);
    hc::MI355XPairHMM pairhmm(0);
    hc::MI355XGenotyper<Variant> genotyper;
    for (auto& r : sep) {
        aligner.align_haplotypes(r.ref, r.haplotypes);
        auto L = pairhmm.compute_likelihoods(r.haplotypes, r.reads);
        sep_variants.push_back(
            genotyper.assign_genotype_likelihoods(r.reads, r.haplotypes, L, std::string_view{r.ref}, r.padded, r.origin));
    }

    // The region caller, all regions in one call; then once more with the CIGARs passed in.
    using Caller = hc::MI355XRegionCaller<Variant>;
    Caller caller(0);
    auto run = [&](std::vector<RegionIn>& regs) {
        std::vector<Caller::Region<SAMRecord, Haplotype, Interval>> batch;
        for (auto& r : regs) batch.push_back({&r.reads, &r.haplotypes, std::string_view{r.ref}, r.padded, r.origin});
        return caller.call_many(batch);
    };
    std::vector<RegionIn> one = input;
    const auto one_variants = run(one);
    std::vector<RegionIn> two = input;
    for (size_t k = 0; k < two.size(); ++k) two[k].haplotypes = sep[k].haplotypes;
    const auto two_variants = run(two);

    auto same_variants = [](const std::vector<Variant>& a, const std::vector<Variant>& b) {
        if (a.size() != b.size()) return false;
        for (size_t v = 0; v < a.size(); ++v)
            if (!a[v].same(b[v])) return false;
        return true;
    };
    for (size_t k = 0; k < input.size(); ++k) {
        n_haps += long(input[k].haplotypes.size());
        n_reads += long(input[k].reads.size());
        n_kept += long(sep[k].reads.size());
        n_variants += long(sep_variants[k].size());
        for (size_t h = 0; h < input[k].haplotypes.size(); ++h)
            bad_sw += one[k].haplotypes[h].alignment_begin_wrt_ref != sep[k].haplotypes[h].alignment_begin_wrt_ref ||
                      one[k].haplotypes[h].cigar.text != sep[k].haplotypes[h].cigar.text ||
                      one[k].haplotypes[h].cigar.text.empty();
        bool same_keep = one[k].reads.size() == sep[k].reads.size() && two[k].reads.size() == sep[k].reads.size();
        for (size_t r = 0; same_keep && r < sep[k].reads.size(); ++r)
            same_keep = one[k].reads[r].id == sep[k].reads[r].id && two[k].reads[r].id == sep[k].reads[r].id;
        bad_keep += !same_keep;
        bad_variants += !same_variants(one_variants[k], sep_variants[k]);
        bad_passed_in += !same_variants(two_variants[k], sep_variants[k]);
    }
    FILE* f = std::fopen(argv[2], "w");
    if (!f) return 5;
    std::fprintf(f,
                 "{\"regions\": %zu, \"haplotypes\": %ld, \"reads\": %ld, \"reads_kept\": %ld, \"variants\": %ld, "
                 "\"sw_mismatch\": %ld, \"keep_mismatch\": %ld, \"variant_mismatch\": %ld, "
                 "\"passed_in_cigar_mismatch\": %ld}\n",
                 input.size(), n_haps, n_reads, n_kept, n_variants, bad_sw, bad_keep, bad_variants, bad_passed_in);
    std::fclose(f);
    return (bad_sw | bad_keep | bad_variants | bad_passed_in) ? 1 : 0;
}
