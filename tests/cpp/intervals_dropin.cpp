// The compiled example of include/hc_intervals.hpp, and the program of
// tests/test_gpu_intervals_dropin.py.
//
//   intervals_dropin IN.sam|IN.bam REF.fa OUT.vcf BED|- INDEX|- seed [NAME BEGIN END]...
//
// Status 3 with the message on stderr for invalid input, 4 for any other error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "hc_intervals.hpp"

int main(int argc, char** argv)
{
    if (argc < 7 || (argc - 7) % 3 != 0) return 2;
    hc::MI355XIntervalCaller caller;
    caller.in_path = argv[1];
    caller.ref_path = argv[2];
    caller.out_path = argv[3];
    if (std::strcmp(argv[4], "-") != 0) caller.bed_path = argv[4];
    if (std::strcmp(argv[5], "-") != 0) caller.index_path = argv[5];
    caller.seed = std::strtoull(argv[6], nullptr, 10);
    for (int k = 7; k < argc; k += 3)
        caller.intervals.push_back({argv[k], std::strtoll(argv[k + 1], nullptr, 10), std::strtoll(argv[k + 2], nullptr, 10)});
    try {
        caller.do_work();
    } catch (const std::invalid_argument& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    std::printf("contigs %d windows %d asked %d\n", caller.n_contigs(), caller.n_windows(), caller.n_asked());
    return 0;
}
