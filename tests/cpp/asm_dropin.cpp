// C++ drop-in check for include/hc_asm.hpp: the first line of
// HaplotypeCaller::call_region (haplotypecaller.hpp:83-107),
//     auto haplotypes = assembler.assemble(reads, ref);
// compiled against hc::MI355XAssembler with SAMRecord / Haplotype / Cigar
// stand-ins, then the same regions through assemble_regions().
// Input (text, bytes in hex): n_regions, then per region "ref n_reads" and
// n_reads x "bases quals". Output per region, twice (per-region call, then the
// batched call): "R status k n_haps" and n_haps x "H score_bits bases begin cigar".
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "hc_asm.hpp"

struct Cigar {   // stand-in: only the assignment the aligner's loop uses
    std::string text;
    Cigar& operator=(const std::string& s) { text = s; return *this; }
};
struct Haplotype {   // haplotype/haplotype.hpp:17-26
    std::string bases;
    Cigar cigar;
    std::size_t alignment_begin_wrt_ref = 0;
    double score = 0;
    Haplotype() = default;
    Haplotype(std::string b, double s) : bases(std::move(b)), score(s) {}
};
struct SAMRecord {   // sam/sam.hpp:28-29
    std::string SEQ, QUAL;
};

static std::string unhex(const std::string& s)
{
    std::string out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back(char(std::stoi(s.substr(i, 2), nullptr, 16)));
    return out;
}

static void print(std::FILE* out, int status, std::size_t k, const std::vector<Haplotype>& haplotypes)
{
    std::fprintf(out, "R %d %zu %zu\n", status, k, haplotypes.size());
    for (const auto& h : haplotypes) {
        uint64_t bits;
        std::memcpy(&bits, &h.score, 8);
        std::fprintf(out, "H %016" PRIx64 " %s %zu %s\n", bits, h.bases.c_str(), h.alignment_begin_wrt_ref,
                     h.cigar.text.c_str());
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    std::FILE* out = std::fopen(argv[2], "w");
    int nreg = 0;
    in >> nreg;
    std::vector<std::string> refs(static_cast<size_t>(nreg));
    std::vector<std::vector<SAMRecord>> all_reads(static_cast<size_t>(nreg));
    for (int r = 0; r < nreg; ++r) {
        std::string ref_hex;
        int n_reads = 0;
        in >> ref_hex >> n_reads;
        refs[size_t(r)] = unhex(ref_hex);
        for (int j = 0; j < n_reads; ++j) {
            std::string b, q;
            in >> b >> q;
            all_reads[size_t(r)].push_back(SAMRecord{unhex(b), unhex(q)});
        }
    }
    if (!in) return 3;
    hc::MI355XAssembler<Haplotype> assembler;
    for (int r = 0; r < nreg; ++r) {
        const std::vector<SAMRecord>& reads = all_reads[size_t(r)];
        const std::string& ref = refs[size_t(r)];
        auto haplotypes = assembler.assemble(reads, ref);   // haplotypecaller.hpp, unchanged
        print(out, assembler.region_status(), assembler.kmer_size(), haplotypes);
    }
    std::vector<hc::MI355XAssembler<Haplotype>::Region<SAMRecord>> regions;
    for (int r = 0; r < nreg; ++r) regions.push_back({&all_reads[size_t(r)], refs[size_t(r)]});
    const auto many = assembler.assemble_regions(regions);
    for (int r = 0; r < nreg; ++r) print(out, assembler.region_status(size_t(r)), assembler.kmer_size(size_t(r)), many[size_t(r)]);
    std::fclose(out);
    return 0;
}
