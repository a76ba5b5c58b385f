// Sorted buckets of the genome caller (include/hc_genome.h,
// HC_GENOME_SORTED_BUCKETS), gfx950. All integer, plain vector loads and
// stores; no global atomic decides where an element goes, so two runs give the
// same bytes. The rules are genome_sort_body.hpp's.
//
//   genome_sort_keys_kernel     one lane per record, or per record of an interval
//                               call's scoped list: genome_place_kernel's
//                               placement and defect tests and its two
//                               atomicMins; the key is off[contig] + POS - 1, or
//                               total_len for an unplaced read, the payload the
//                               record index.
//   genome_sort_hist_kernel     one workgroup per tile: the tile's elements per
//                               digit of this pass, counted in LDS, stored
//                               digit-major.
//   (scan of the histogram: sam_scan_kernel)
//   genome_sort_scatter_kernel  one workgroup per tile, round by round: the eight
//                               ballots of a wave's digits give each lane the
//                               mask of its wave's lanes with the same digit;
//                               the wave's count per digit goes to LDS, and an
//                               element is stored at the tile's offset for its
//                               digit + the earlier rounds' + the earlier waves'
//                               + the lower lanes' elements with that digit.
//   genome_sort_heads_kernel    one lane per sorted element: the head flag of a
//                               run, and kErrDepth for read number
//                               HC_CONTIG_MAX_READS_PER_POSITION + 1 of a position.
//   (scan of the flags: sam_scan_kernel)
//   genome_sort_runs_kernel     one lane per sorted element: a head stores its
//                               run's key and first element; the last placed
//                               read closes the table.
//   genome_sorted_pick_kernel   one wave per genome-wide window, or per asked window
//                               of an interval call's list, its contig and
//                               padded interval as genome_pick_kernel's; two
//                               wave-uniform lower bounds over the run keys give
//                               its runs (the second over no more runs than the
//                               interval has positions), lane j takes run
//                               r0 + j (+ 64, ...).
#include "genome_sort_kernels.hpp"

#include "../../include/hc_genome.h"
#include "sam_kernels.hpp"

namespace hcgenome {

__global__ __launch_bounds__(256) void genome_sort_keys_kernel(GenomeArgs a, const int32_t* scoped, int32_t n, int64_t* key,
                                                               int32_t* index)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t k = scoped ? scoped[i] : i;   // below n_records: the list holds record indices
    const hc_sam_record r = a.records[k];
    const int32_t c = a.contig_of[k];
    const unsigned long long line = static_cast<unsigned long long>(a.line_no[k]);
    int64_t at = a.total_len;
    if (!genome_placed(c, r.pos, a.ref_len)) {
        if (!a.skip_unplaced) atomicMin(a.err, line * 16ull + kErrUnplaced);
    } else {
        const bool filtered = r.mapq < HC_PREP_MIN_MAPQ || (r.flag & 0x500) || !r.mate_same_contig;
        if (!filtered && r.defect) atomicMin(a.err, line * 16ull + kErrDefect);
        at = a.off[c] + int64_t(r.pos - 1u);
    }
    key[i] = at;
    index[i] = int32_t(k);
}

__global__ __launch_bounds__(kSortBlock) void genome_sort_hist_kernel(const int64_t* key, int32_t n, int pass, int32_t* hist,
                                                                      int32_t n_tiles)
{
    __shared__ int32_t count[kSortDigits];
    const int tid = int(threadIdx.x);
    count[tid] = 0;
    __syncthreads();
    const int64_t begin = int64_t(blockIdx.x) * kSortTile;
    for (int round = 0; round < kSortRounds; ++round) {
        const int64_t i = begin + round * kSortBlock + tid;
        if (i < n) atomicAdd(&count[sort_digit(key[i], pass)], 1);   // a count only: no order comes from it
    }
    __syncthreads();
    hist[int64_t(tid) * n_tiles + blockIdx.x] = count[tid];
}

__global__ __launch_bounds__(kSortBlock) void genome_sort_scatter_kernel(const int64_t* key_in, const int32_t* index_in,
                                                                         int64_t* key_out, int32_t* index_out, int32_t n, int pass,
                                                                         const int64_t* hist_first, int32_t n_tiles)
{
    __shared__ int64_t base[kSortDigits];                      // where the tile's first element with the digit goes
    __shared__ int32_t running[kSortDigits];                   // the earlier rounds' elements with the digit
    __shared__ int32_t wave_count[kSortWaves * kSortDigits];   // this round's, per wave
    const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    base[tid] = hist_first[int64_t(tid) * n_tiles + blockIdx.x];
    running[tid] = 0;
    for (int k = 0; k < kSortWaves; ++k) wave_count[k * kSortDigits + tid] = 0;
    __syncthreads();
    const int64_t begin = int64_t(blockIdx.x) * kSortTile;
    for (int round = 0; round < kSortRounds && begin + round * kSortBlock < n; ++round) {   // uniform in the workgroup
        const int64_t i = begin + round * kSortBlock + tid;
        const bool valid = i < n;
        const int64_t key = valid ? key_in[i] : 0;
        const uint32_t digit = sort_digit(key, pass);
        uint64_t bit[8];
        for (int b = 0; b < 8; ++b) bit[b] = __ballot(valid && ((digit >> b) & 1u));
        const uint64_t match = sort_match(bit, digit, __ballot(valid));
        if (valid && (match >> lane) == 1ull) wave_count[wave * kSortDigits + int(digit)] = sort_popc(match);   // its highest lane
        __syncthreads();
        if (valid) {
            const int64_t to = base[digit] + sort_rank(running[digit], wave_count, wave, digit, match, lane);
            if (uint64_t(to) < uint64_t(n)) {   // holds by construction: the histogram counted these keys
                key_out[to] = key;
                index_out[to] = index_in[i];
            }
        }
        __syncthreads();
        int32_t add = 0;
        for (int k = 0; k < kSortWaves; ++k) {
            add += wave_count[k * kSortDigits + tid];
            wave_count[k * kSortDigits + tid] = 0;
        }
        running[tid] += add;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void genome_sort_heads_kernel(const int64_t* key, int32_t n, int64_t total_len, int32_t* head,
                                                                unsigned long long* err)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    head[i] = sort_head(key, i, total_len) ? 1 : 0;
    if (sort_too_deep(key, i, total_len, HC_CONTIG_MAX_READS_PER_POSITION))
        atomicMin(err, static_cast<unsigned long long>(key[i] + 1) * 16ull + kErrDepth);
}

__global__ __launch_bounds__(256) void genome_sort_runs_kernel(const int64_t* key, int32_t n, int64_t total_len, const int32_t* head,
                                                               const int64_t* run_of, int64_t* run_pos, int64_t* run_first)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    if (head[i]) {
        const int64_t r = run_of[i];
        run_pos[r] = key[i];
        run_first[r] = i;
    }
    if (sort_last_placed(key, i, n, total_len)) run_first[run_of[n]] = i + 1;   // the number of placed reads
    if (i == 0 && key[0] >= total_len) run_first[0] = 0;                        // no read is placed
}

template <bool kWrite>
__global__ __launch_bounds__(64 * kWavesPerBlock) void genome_sorted_pick_kernel(GenomeSortArgs s)
{
    const GenomeArgs& a = s.g;
    const int lane = int(threadIdx.x) & 63;
    const int64_t i = int64_t(blockIdx.x) * kWavesPerBlock + (int(threadIdx.x) >> 6);
    if (i >= a.n_asked) return;   // wave-uniform, as is everything below that is not indexed by `lane`
    const int64_t w = genome_pick_window(a, i);
    const int32_t c = genome_contig_of_window(a.win_off, a.n_contigs, w);
    const int64_t lw = w - a.win_off[c];   // the contig's own window index
    const int64_t len = a.ref_len[c];
    const int64_t origin = lw * a.region;
    const int64_t begin = lw == 0 ? 0 : origin - a.padding;
    int64_t end = origin + a.region + a.padding;
    if (end > len) end = len;   // positions at and past the contig's end are another contig's
    const int64_t off = a.off[c];
    const int64_t n_runs = s.run_of[s.n];
    const int64_t r0 = sort_lower_bound(s.run_pos, n_runs, off + begin);
    // the run keys are distinct and ascending, so run r0 + j lies at or behind begin + j: the second search is short
    const int64_t most = n_runs - r0 < end - begin ? n_runs - r0 : end - begin;
    const int64_t r1 = r0 + sort_lower_bound(s.run_pos + r0, most, off + end);
    if (!kWrite) {
        if (lane == 0) a.n_picked[w] = int32_t(r1 - r0);
        return;
    }
    int32_t* out = a.picked + a.win_first[w];
    for (int64_t r = r0 + lane; r < r1; r += 64) {
        const int64_t first = s.run_first[r];
        const uint32_t n = uint32_t(s.run_first[r + 1] - first);
        out[r - r0] = s.sorted[first + hccontig::pick_index(a.seed, uint64_t(lw), uint64_t(s.run_pos[r] - off), n, a.pick_mode)];
    }
}

static unsigned blocks_of(int64_t n, int per) { return unsigned((n + per - 1) / per); }

hipError_t launch_sorted_buckets(GenomeSortArgs& a, hipStream_t st)
{
    const int32_t n = a.n;
    const int32_t n_tiles = int32_t(sort_tiles(n));
    const int last = a.passes & 1;
    a.keys = a.key[last];
    a.sorted = a.index[last];
    int32_t* head = a.index[last ^ 1];
    int64_t* run_of = a.key[last ^ 1];
    a.run_of = run_of;
    if (n > 0) {
        hipLaunchKernelGGL(genome_sort_keys_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, a.g, a.scoped, n, a.key[0],
                           a.index[0]);
        for (int pass = 0; pass < a.passes; ++pass) {
            const int in = pass & 1;
            hipLaunchKernelGGL(genome_sort_hist_kernel, dim3(unsigned(n_tiles)), dim3(kSortBlock), 0, st, a.key[in], n, pass, a.hist,
                               n_tiles);
            if (hipError_t e = hcsam::launch_scan(a.hist, int64_t(kSortDigits) * n_tiles, a.hist_first, a.scan_work, st)) return e;
            hipLaunchKernelGGL(genome_sort_scatter_kernel, dim3(unsigned(n_tiles)), dim3(kSortBlock), 0, st, a.key[in], a.index[in],
                               a.key[in ^ 1], a.index[in ^ 1], n, pass, a.hist_first, n_tiles);
        }
        hipLaunchKernelGGL(genome_sort_heads_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, a.keys, n, a.g.total_len, head,
                           a.g.err);
    }
    if (hipError_t e = hcsam::launch_scan(head, n, run_of, a.scan_work, st)) return e;   // no record: run_of[0] = 0 runs
    if (n > 0)
        hipLaunchKernelGGL(genome_sort_runs_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, a.keys, n, a.g.total_len, head,
                           a.run_of, a.run_pos, a.run_first);
    return hipGetLastError();
}

hipError_t launch_sorted_pick_count(const GenomeSortArgs& a, hipStream_t st)
{
    if (a.g.n_asked <= 0) return hipSuccess;
    hipLaunchKernelGGL(genome_sorted_pick_kernel<false>, dim3(blocks_of(a.g.n_asked, kWavesPerBlock)), dim3(64 * kWavesPerBlock),
                       0, st, a);
    return hipGetLastError();
}

hipError_t launch_sorted_pick_write(const GenomeSortArgs& a, hipStream_t st)
{
    if (a.g.n_asked <= 0) return hipSuccess;
    hipLaunchKernelGGL(genome_sorted_pick_kernel<true>, dim3(blocks_of(a.g.n_asked, kWavesPerBlock)), dim3(64 * kWavesPerBlock),
                       0, st, a);
    return hipGetLastError();
}

}  // namespace hcgenome
