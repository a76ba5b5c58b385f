// C++ drop-in check for include/hc_gt.hpp: the call of haplotypecaller.hpp
// compiled against hc::MI355XGenotyper<Variant> with SAMRecord / Haplotype /
// Cigar / Interval / Variant stand-ins shaped like the reference's.
//
//   gt_dropin run <in> <out>     per region the reference's call, one line per
//                                variant: region begin end alleles a1/a2 quality
//   gt_dropin host <in> <reps>   the event bookkeeping the drop-in takes off the
//                                host (events, sites, alleles, maps, kept reads)
//                                restated with std::map / std::set on one core:
//                                prints "<ms per pass> <sites> <kept reads>
//                                <sum of hap_allele> <allele bytes>"
//
// Input: n_regions, then per region: ref, padded_begin, origin_begin,
// origin_end (int64), n_haps, per haplotype bases, begin (int32), cigar;
// n_reads, read_begin[], read_end[] (int64), L[n_reads x n_haps] (strings are
// int32 length-prefixed).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "hc_gt.hpp"

struct Interval {
    std::string contig;
    std::size_t begin = 0, end = 0;
};
struct Cigar {   // stand-in: holds the text, gives it back as the reference's to_string()
    std::string text;
    std::string to_string() const { return text; }
};
struct Haplotype {
    std::string bases;
    std::size_t alignment_begin_wrt_ref = 0;
    Cigar cigar;
};
struct SAMRecord {
    Interval iv;
    Interval get_interval() const { return iv; }
};
struct Variant {
    Interval location;
    std::vector<std::string> alleles;
    std::pair<std::size_t, std::size_t> GT;
    std::size_t GQ = 0;
    Variant(Interval loc, std::vector<std::string> al, std::pair<std::size_t, std::size_t> gt, std::size_t gq)
        : location(std::move(loc)), alleles(std::move(al)), GT(gt), GQ(gq) {}
};

struct RegionIn {
    std::string ref;
    Interval padded, origin;
    std::vector<Haplotype> haplotypes;
    std::vector<SAMRecord> reads;
    std::vector<std::vector<double>> likelihoods;
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
        for (auto& h : r.haplotypes) {
            h.bases = rds(in);
            h.alignment_begin_wrt_ref = static_cast<std::size_t>(rd<int32_t>(in));
            h.cigar.text = rds(in);
        }
        r.reads.resize(static_cast<size_t>(rd<int32_t>(in)));
        for (auto& x : r.reads) x.iv.begin = static_cast<std::size_t>(rd<int64_t>(in));
        for (auto& x : r.reads) x.iv.end = static_cast<std::size_t>(rd<int64_t>(in));
        r.likelihoods.assign(r.reads.size(), std::vector<double>(r.haplotypes.size()));
        for (auto& row : r.likelihoods)
            in.read(reinterpret_cast<char*>(row.data()), static_cast<std::streamsize>(sizeof(double) * row.size()));
    }
    return out;
}

// ---- host bookkeeping, restated (what a caller of hc_gt_genotype_sites has to do itself) ----

struct Event {
    std::size_t begin, end;
    std::string REF, ALT;
    bool operator<(const Event& o) const { return std::tie(begin, end, REF, ALT) < std::tie(o.begin, o.end, o.REF, o.ALT); }
};

struct HostSums {
    long sites = 0, kept = 0, map_sum = 0, allele_bytes = 0;
};

static void host_region(const RegionIn& r, HostSums& sums)
{
    const std::string& ref = r.ref;
    std::vector<std::map<std::size_t, Event>> maps(r.haplotypes.size());
    std::set<std::size_t> begins;
    for (size_t h = 0; h < maps.size(); ++h) {
        const Haplotype& hap = r.haplotypes[h];
        std::size_t rp = hap.alignment_begin_wrt_ref, hp = 0;
        const char* t = hap.cigar.text.c_str();
        while (*t) {
            char* e = nullptr;
            const std::size_t n = std::strtoul(t, &e, 10);
            const char op = *e;
            t = e + 1;
            if (op == 'M') {
                for (std::size_t o = 0; o < n; ++o)
                    if (ref[rp + o] != hap.bases[hp + o]) {
                        const std::size_t b = r.padded.begin + rp + o;
                        maps[h].emplace(b, Event{b, b + 1, ref.substr(rp + o, 1), hap.bases.substr(hp + o, 1)});
                    }
                rp += n;
                hp += n;
            } else if (op == 'I') {
                if (rp > 0) {
                    const std::size_t b = r.padded.begin + rp - 1;
                    maps[h].emplace(b, Event{b, b + 1, ref.substr(rp - 1, 1), ref.substr(rp - 1, 1) + hap.bases.substr(hp, n)});
                }
                hp += n;
            } else if (op == 'D') {
                if (rp > 0) {
                    const std::size_t b = r.padded.begin + rp - 1;
                    maps[h].emplace(b, Event{b, b + n + 1, ref.substr(rp - 1, n + 1), ref.substr(rp - 1, 1)});
                }
                rp += n;
            } else {
                hp += n;
            }
        }
        for (const auto& kv : maps[h]) begins.insert(kv.first);
    }
    for (const std::size_t begin : begins) {
        if (begin < r.origin.begin || begin >= r.origin.end) continue;
        std::vector<std::vector<Event>> over(maps.size());
        std::set<Event> events;
        for (size_t h = 0; h < maps.size(); ++h)
            for (auto it = maps[h].begin(); it != maps[h].end() && it->first <= begin; ++it)
                if (it->second.end > begin) {
                    over[h].push_back(it->second);
                    events.insert(it->second.begin == begin
                                      ? it->second
                                      : Event{begin, begin + 1, ref.substr(begin - r.padded.begin, 1), "*"});
                }
        std::string ref_allele;
        std::size_t loc_end = begin;
        for (const Event& e : events) {
            if (e.REF.size() > ref_allele.size()) ref_allele = e.REF;
            loc_end = std::max(loc_end, e.end);
        }
        auto compatible = [&](const Event& e) {
            return (e.REF == ref_allele || e.ALT == "*") ? e.ALT : e.ALT + ref_allele.substr(e.REF.size());
        };
        std::set<std::string> alts;
        for (const Event& e : events) alts.insert(compatible(e));
        sums.sites += 1;
        if (alts.size() + 1 > HC_GT_MAX_ALLELES) continue;
        std::vector<std::string> alleles{ref_allele};
        alleles.insert(alleles.end(), alts.begin(), alts.end());
        for (const auto& a : alleles) sums.allele_bytes += long(a.size());
        for (size_t h = 0; h < maps.size(); ++h) {
            long best = 0;
            for (const Event& e : over[h]) {
                const std::string want = e.begin == begin ? compatible(e) : std::string("*");
                best = std::max(best, long(std::find(alleles.begin(), alleles.end(), want) - alleles.begin()));
            }
            sums.map_sum += best;
        }
        const std::size_t lo = begin < 2 ? 0 : begin - 2, hi = loc_end + 2;   // cut at the contig's first base (hc_gt.h)
        for (const auto& rec : r.reads)
            if (rec.iv.begin < hi && lo < rec.iv.end) sums.kept += 1;
    }
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const std::string mode = argv[1];
    std::vector<RegionIn> regions = load(argv[2]);
    if (mode == "host") {
        const int reps = std::atoi(argv[3]);
        HostSums sums;
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < reps; ++k) {
            sums = HostSums{};
            for (const auto& r : regions) host_region(r, sums);
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("%.6f %ld %ld %ld %ld\n", ms / reps, sums.sites, sums.kept, sums.map_sum, sums.allele_bytes);
        return 0;
    }
    std::FILE* out = std::fopen(argv[3], "w");
    hc::MI355XGenotyper<Variant> genotyper;   // the reference: Genetyper genotyper;
    for (size_t k = 0; k < regions.size(); ++k) {
        auto& [ref, padded_region, origin_region, haplotypes, reads, likelihoods] = regions[k];
        auto variants = genotyper.assign_genotype_likelihoods(reads, haplotypes, likelihoods, ref, padded_region,
                                                              origin_region);
        for (const Variant& v : variants) {
            std::string al;
            for (const auto& a : v.alleles) al += (al.empty() ? "" : ",") + a;
            std::fprintf(out, "%zu %zu %zu %s %zu/%zu %zu\n", k, v.location.begin, v.location.end, al.c_str(),
                         v.GT.first, v.GT.second, v.GQ);
        }
    }
    std::fclose(out);
    return 0;
}
