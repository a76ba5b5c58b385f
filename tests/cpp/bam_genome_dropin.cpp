// The compiled example of include/hc_bam.hpp, and the program of
// tests/test_gpu_bam_genome.py: tests/cpp/genome_dropin.cpp with
// hc::MI355XBamGenomeCaller in the place of hc::MI355XGenomeCaller.
//
//   bam_genome_dropin IN.bam REF.fa OUT.vcf [seed [first|seeded [skip]]]
//
// Status 3 with the message on stderr for invalid input, 4 for any other error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "hc_bam.hpp"

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    hc::MI355XBamGenomeCaller caller;
    caller.in_path = argv[1];
    caller.ref_path = argv[2];
    caller.out_path = argv[3];
    if (argc > 4) caller.seed = std::strtoull(argv[4], nullptr, 10);
    if (argc > 5 && std::strcmp(argv[5], "first") == 0) caller.pick_mode = HC_CONTIG_PICK_FIRST;
    if (argc > 6 && std::strcmp(argv[6], "skip") == 0) caller.skip_unplaced = true;
    try {
        caller.do_work();
    } catch (const std::invalid_argument& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    std::printf("contigs %d windows %d\n", caller.n_contigs(), caller.n_windows());
    return 0;
}
