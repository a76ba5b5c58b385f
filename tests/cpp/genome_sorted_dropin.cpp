// The program of tests/test_gpu_genome_sorted.py's drop-in test:
// hc::MI355XGenomeCaller (include/hc_genome.hpp) with its sorted_buckets member
// set from the command line.
//
//   genome_sorted_dropin IN.sam REF.fa OUT.vcf SEED dense|sorted
//
// Status 3 with the message on stderr for invalid input, 4 for any other error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "hc_genome.hpp"

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    hc::MI355XGenomeCaller caller;
    caller.in_path = argv[1];
    caller.ref_path = argv[2];
    caller.out_path = argv[3];
    caller.seed = std::strtoull(argv[4], nullptr, 10);
    caller.sorted_buckets = std::strcmp(argv[5], "sorted") == 0;
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
