// Host program for tests/test_prep_host.py: csrc/prep_body.hpp compiled for the
// host (PREPX_HOST_ONLY) and run under -fsanitize=address,undefined. Every
// read's CIGAR words and every window's outputs live in heap blocks of exactly
// their size, so a read or write past them is an error, not a silent success.
//
//   prep_host_main IN OUT
//
// IN:  n_windows, then per window "begin end n_reads" and per read
//      "flag mapq pos seq_len mate_same n_cigar word...".
// OUT: per window "W n_reads n_kept kept_bases kept..." and per read
//      "keep drop_reason offset length new_pos front_to_M back_to_M begin end".
// A read with an input error ends the program with status 3 after printing
// "E window read code" to OUT.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>

#include "../../gatk-haplotypecaller-cpp17_amd/csrc/prep_body.hpp"

using namespace hcprep;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::ifstream in(argv[1]);
    std::ofstream out(argv[2]);
    int n_windows = 0;
    if (!(in >> n_windows)) return 2;
    for (int w = 0; w < n_windows; ++w) {
        long long begin = 0, end = 0;
        int n_reads = 0;
        if (!(in >> begin >> end >> n_reads)) return 2;
        std::unique_ptr<hc_prep_record[]> recs(new hc_prep_record[size_t(n_reads)]);
        std::unique_ptr<int32_t[]> kept(new int32_t[size_t(n_reads)]);
        int32_t n_kept = 0;
        int64_t kept_bases = 0;
        for (int j = 0; j < n_reads; ++j) {
            unsigned flag = 0, mapq = 0, pos = 0, mate = 0;
            int seq_len = 0, n_cigar = 0;
            if (!(in >> flag >> mapq >> pos >> seq_len >> mate >> n_cigar)) return 2;
            std::unique_ptr<uint32_t[]> words(new uint32_t[size_t(n_cigar)]);
            for (int k = 0; k < n_cigar; ++k)
                if (!(in >> words[size_t(k)])) return 2;
            const PrepRead r{0, pos, seq_len, n_cigar, uint16_t(flag), uint16_t(mapq), mate, 0u};
            const int32_t e = prep_one(r, words.get(), uint64_t(begin), uint64_t(end), recs[size_t(j)]);
            if (e != kErrNone) {
                out << "E " << w << ' ' << j << ' ' << e << '\n';
                return 3;
            }
            if (recs[size_t(j)].keep) {
                kept[size_t(n_kept++)] = j;
                kept_bases += recs[size_t(j)].length;
            }
        }
        out << "W " << n_reads << ' ' << n_kept << ' ' << kept_bases;
        for (int32_t k = 0; k < n_kept; ++k) out << ' ' << kept[size_t(k)];
        out << '\n';
        for (int j = 0; j < n_reads; ++j) {
            const hc_prep_record& o = recs[size_t(j)];
            out << int(o.keep) << ' ' << int(o.drop_reason) << ' ' << o.offset << ' ' << o.length << ' ' << o.new_pos << ' '
                << int(o.front_to_M) << ' ' << int(o.back_to_M) << ' ' << o.begin << ' ' << o.end << '\n';
        }
    }
    return 0;
}
