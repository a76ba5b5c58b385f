// Host program for tests/test_genome_sort_host.py: csrc/genome_sort_body.hpp
// compiled for the host (SAMX_HOST_ONLY) and run on one thread under
// -fsanitize=address,undefined. genome_sort_scatter_kernel makes the eight bit
// masks of a wave's digits by __ballot; here a loop over the wave's 64 elements
// makes them. Everything else is genome_sort_body.hpp's own text, run as the
// kernels of genome_sort_kernels.hip run it: pass by pass, the histogram
// digit-major per tile, its exclusive scan, the scatter tile by tile, round by
// round and wave by wave against the running and the per-wave counts; then the
// head flags, their scan, the run table with its closing entry, the depth test
// and the lower bounds. Keys, indices, histogram, flags and runs live in heap
// blocks of exactly their sizes (the two key buffers of n + 1, as the engine's),
// so a read or a store past them is an error, not a silent success.
//
//   genome_sort_host_main IN MAX_READS OUT
//
// IN:  "n total_len q", then n keys, then q keys to search for.
// OUT: "T tile passes", n lines "key index" in sorted order, "R n_runs", one
//      line "run_pos run_first" per run, "C closing", "D" and the least key + 1
//      with more than MAX_READS elements (0: none), "Q q" and q lower bounds.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <utility>

#include "../../gatk-haplotypecaller-cpp17_amd/csrc/genome_sort_body.hpp"

using namespace hcgenome;

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    std::ifstream in(argv[1]);
    const int64_t max_reads = std::atoll(argv[2]);
    int64_t n = 0, total_len = 0, q = 0;
    if (!(in >> n >> total_len >> q) || n < 0 || total_len < 1 || q < 0 || max_reads < 1) return 2;
    std::unique_ptr<int64_t[]> key[2] = {std::unique_ptr<int64_t[]>(new int64_t[size_t(n) + 1]),
                                         std::unique_ptr<int64_t[]>(new int64_t[size_t(n) + 1])};
    std::unique_ptr<int32_t[]> index[2] = {std::unique_ptr<int32_t[]>(new int32_t[size_t(n)]),
                                           std::unique_ptr<int32_t[]>(new int32_t[size_t(n)])};
    for (int64_t i = 0; i < n; ++i) {
        if (!(in >> key[0][size_t(i)]) || key[0][size_t(i)] < 0 || key[0][size_t(i)] > total_len) return 2;
        index[0][size_t(i)] = int32_t(i);
    }
    std::unique_ptr<int64_t[]> query(new int64_t[size_t(q)]);
    for (int64_t i = 0; i < q; ++i)
        if (!(in >> query[size_t(i)])) return 2;

    const int64_t n_tiles = sort_tiles(n);
    const int64_t n_hist = int64_t(kSortDigits) * n_tiles;
    const int passes = sort_passes(total_len);
    std::unique_ptr<int32_t[]> hist(new int32_t[size_t(n_hist)]);
    std::unique_ptr<int64_t[]> hist_first(new int64_t[size_t(n_hist) + 1]);
    for (int pass = 0; pass < passes; ++pass) {
        const int64_t* kin = key[pass & 1].get();
        const int32_t* iin = index[pass & 1].get();
        int64_t* kout = key[(pass & 1) ^ 1].get();
        int32_t* iout = index[(pass & 1) ^ 1].get();
        // genome_sort_hist_kernel
        for (int64_t i = 0; i < n_hist; ++i) hist[size_t(i)] = 0;
        for (int64_t i = 0; i < n; ++i) ++hist[size_t(int64_t(sort_digit(kin[i], pass)) * n_tiles + i / kSortTile)];
        // the scan
        hist_first[0] = 0;
        for (int64_t i = 0; i < n_hist; ++i) hist_first[size_t(i) + 1] = hist_first[size_t(i)] + hist[size_t(i)];
        // genome_sort_scatter_kernel, one tile after the other
        for (int64_t tile = 0; tile < n_tiles; ++tile) {
            int32_t running[kSortDigits] = {};
            for (int round = 0; round < kSortRounds && tile * kSortTile + round * kSortBlock < n; ++round) {
                const int64_t at = tile * kSortTile + round * kSortBlock;
                int32_t wave_count[kSortWaves * kSortDigits] = {};
                uint64_t match[kSortBlock] = {};
                for (int wave = 0; wave < kSortWaves; ++wave) {
                    uint64_t bit[8] = {}, valid = 0;
                    for (int lane = 0; lane < 64; ++lane) {   // the ballots
                        const int64_t i = at + wave * 64 + lane;
                        if (i >= n) continue;
                        valid |= uint64_t(1) << lane;
                        for (int b = 0; b < 8; ++b)
                            if ((sort_digit(kin[i], pass) >> b) & 1u) bit[b] |= uint64_t(1) << lane;
                    }
                    for (int lane = 0; lane < 64; ++lane) {
                        const int64_t i = at + wave * 64 + lane;
                        if (i >= n) continue;
                        const uint32_t d = sort_digit(kin[i], pass);
                        const uint64_t m = sort_match(bit, d, valid);
                        match[wave * 64 + lane] = m;
                        if ((m >> lane) == 1u) wave_count[wave * kSortDigits + int(d)] = sort_popc(m);
                    }
                }
                for (int t = 0; t < kSortBlock && at + t < n; ++t) {
                    const uint32_t d = sort_digit(kin[at + t], pass);
                    const int64_t to = hist_first[size_t(int64_t(d) * n_tiles + tile)] +
                                       sort_rank(running[d], wave_count, t >> 6, d, match[t], t & 63);
                    kout[to] = kin[at + t];   // no bound check here: a wrong rank must show
                    iout[to] = iin[at + t];
                }
                for (int d = 0; d < kSortDigits; ++d)
                    for (int wave = 0; wave < kSortWaves; ++wave) running[d] += wave_count[wave * kSortDigits + d];
            }
        }
    }
    const int last = passes & 1;
    const int64_t* keys = key[last].get();
    int32_t* head = index[last ^ 1].get();   // the free pair holds the flags and their scan, as the engine's
    int64_t* run_of = key[last ^ 1].get();
    int64_t deep = 0;
    for (int64_t i = 0; i < n; ++i) {        // genome_sort_heads_kernel
        head[i] = sort_head(keys, i, total_len) ? 1 : 0;
        if (sort_too_deep(keys, i, total_len, max_reads) && (deep == 0 || keys[i] + 1 < deep)) deep = keys[i] + 1;
    }
    run_of[0] = 0;
    for (int64_t i = 0; i < n; ++i) run_of[i + 1] = run_of[i] + head[i];
    const int64_t n_runs = run_of[n];
    std::unique_ptr<int64_t[]> run_pos(new int64_t[size_t(n_runs)]);
    std::unique_ptr<int64_t[]> run_first(new int64_t[size_t(n_runs) + 1]);
    if (n == 0) run_first[0] = 0;            // the pick kernel reads no run then; the program prints the entry
    for (int64_t i = 0; i < n; ++i) {        // genome_sort_runs_kernel
        if (head[i]) {
            run_pos[size_t(run_of[i])] = keys[i];
            run_first[size_t(run_of[i])] = i;
        }
        if (sort_last_placed(keys, i, n, total_len)) run_first[size_t(run_of[n])] = i + 1;
        if (i == 0 && keys[0] >= total_len) run_first[0] = 0;
    }

    std::FILE* out = std::fopen(argv[3], "w");
    if (!out) return 2;
    std::fprintf(out, "T %d %d\n", kSortTile, passes);
    for (int64_t i = 0; i < n; ++i) std::fprintf(out, "%lld %d\n", static_cast<long long>(keys[i]), index[last][size_t(i)]);
    std::fprintf(out, "R %lld\n", static_cast<long long>(n_runs));
    for (int64_t r = 0; r < n_runs; ++r)
        std::fprintf(out, "%lld %lld\n", static_cast<long long>(run_pos[size_t(r)]), static_cast<long long>(run_first[size_t(r)]));
    std::fprintf(out, "C %lld\nD %lld\nQ %lld\n", static_cast<long long>(run_first[size_t(n_runs)]), static_cast<long long>(deep),
                 static_cast<long long>(q));
    for (int64_t i = 0; i < q; ++i)
        std::fprintf(out, "%lld\n", static_cast<long long>(sort_lower_bound(run_pos.get(), n_runs, query[size_t(i)])));
    std::fclose(out);
    return 0;
}
