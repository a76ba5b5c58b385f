// Genome caller kernels (include/hc_genome.h), gfx950. All integer, plain vector stores.
//
//   genome_resolve_kernel  one wave per record: the line is read again in rows of
//                          64 bytes from its first byte, a ballot over "not
//                          whitespace" gives the masks of token starts and ends
//                          (sam_body.hpp), GenomeRname keeps the third token's.
//                          The token is looked up in the contig table
//                          (genome_body.hpp); lane 0 stores contig_of[k].
//   genome_place_kernel    one lane per record, as contig_place_kernel: a read
//                          without a contig, with POS 0 or past its own contig's
//                          end is unplaced; the placed ones count into
//                          off[contig] + POS - 1.
//   (scan of the counts: sam_scan_kernel)
//   genome_scatter_kernel, genome_sort_kernel
//                          as the contig caller's, over the concatenated positions.
//                          A record out of an interval call's scope (scope[k] == 0)
//                          is passed over by place and scatter: no count, no error.
//   genome_pick_kernel     one wave per genome-wide window, or per asked window of
//                          an interval call's list: its contig by binary
//                          search over the windows' exclusive sums (wave-uniform),
//                          its padded interval from the contig-local window index,
//                          begun at the contig's position 0 and cut at its end, so
//                          it never reaches a neighbour's positions. Compaction by
//                          ballot and carried base as contig_pick_kernel's; the pick
//                          function takes the contig-local window and position.
#include "genome_kernels.hpp"

#include "../../include/hc_genome.h"

namespace hcgenome {

__global__ __launch_bounds__(64 * kWavesPerBlock) void genome_resolve_kernel(GenomeArgs a)
{
    const int lane = int(threadIdx.x) & 63;
    const int64_t k = int64_t(blockIdx.x) * kWavesPerBlock + (int(threadIdx.x) >> 6);
    if (k >= a.n_records) return;   // wave-uniform, as is everything below that is not indexed by `lane`
    const int64_t begin = a.records[k].line;
    GenomeRname tk;
    for (int64_t off = 0; begin + off < a.text_len && !tk.done(); off += 64) {
        const int64_t i = begin + off + lane;
        tk.row(__ballot(i < a.text_len && !hcsam::sam_space(a.text[i])), off);
    }
    int32_t c = -1;
    if (tk.done() && tk.end - tk.begin <= HC_GENOME_MAX_NAME_LEN) {
        uint32_t slot;
        c = genome_lookup(a.table, a.text + begin + tk.begin, tk.end - tk.begin, slot);
    }
    if (lane == 0) a.contig_of[k] = c;
}

__global__ __launch_bounds__(256) void genome_place_kernel(GenomeArgs a)
{
    const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (k >= a.n_records || (a.scope && !a.scope[k])) return;
    const hc_sam_record r = a.records[k];
    const int32_t c = a.contig_of[k];
    const unsigned long long line = static_cast<unsigned long long>(a.line_no[k]);
    if (!genome_placed(c, r.pos, a.ref_len)) {
        if (!a.skip_unplaced) atomicMin(a.err, line * 16ull + kErrUnplaced);
        return;
    }
    const bool filtered = r.mapq < HC_PREP_MIN_MAPQ || (r.flag & 0x500) || !r.mate_same_contig;
    if (!filtered && r.defect) atomicMin(a.err, line * 16ull + kErrDefect);
    atomicAdd(a.count + (a.off[c] + int64_t(r.pos - 1u)), 1);
}

__global__ __launch_bounds__(256) void genome_scatter_kernel(GenomeArgs a)
{
    const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (k >= a.n_records || (a.scope && !a.scope[k])) return;
    const hc_sam_record r = a.records[k];
    const int32_t c = a.contig_of[k];
    if (!genome_placed(c, r.pos, a.ref_len)) return;
    const int64_t b = a.off[c] + int64_t(r.pos - 1u);
    a.bucket[a.first[b] + atomicAdd(a.cursor + b, 1)] = int32_t(k);
}

__global__ __launch_bounds__(256) void genome_sort_kernel(GenomeArgs a)
{
    const int64_t p = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (p >= a.total_len) return;
    const int32_t n = a.count[p];
    if (n > HC_CONTIG_MAX_READS_PER_POSITION) {   // the sort below is quadratic in the worst arrival order
        atomicMin(a.err, static_cast<unsigned long long>(p + 1) * 16ull + kErrDepth);
        return;
    }
    int32_t* v = a.bucket + a.first[p];
    for (int32_t i = 1; i < n; ++i) {
        const int32_t x = v[i];
        int32_t j = i;
        for (; j > 0 && v[j - 1] > x; --j) v[j] = v[j - 1];
        v[j] = x;
    }
}

template <bool kWrite>
__global__ __launch_bounds__(64 * kWavesPerBlock) void genome_pick_kernel(GenomeArgs a)
{
    const int lane = int(threadIdx.x) & 63;
    const int64_t i = int64_t(blockIdx.x) * kWavesPerBlock + (int(threadIdx.x) >> 6);
    if (i >= a.n_asked) return;   // wave-uniform
    const int64_t w = genome_pick_window(a, i);
    const int32_t c = genome_contig_of_window(a.win_off, a.n_contigs, w);
    const int64_t lw = w - a.win_off[c];   // the contig's own window index
    const int64_t len = a.ref_len[c];
    const int64_t origin = lw * a.region;
    const int64_t begin = lw == 0 ? 0 : origin - a.padding;
    int64_t end = origin + a.region + a.padding;
    if (end > len) end = len;   // positions at and past the contig's end are another contig's
    const int32_t* count = a.count + a.off[c];
    const int64_t* first = a.first + a.off[c];
    int32_t* out = kWrite ? a.picked + a.win_first[w] : nullptr;
    int32_t base = 0;
    for (int64_t p0 = begin; p0 < end; p0 += 64) {
        const int64_t p = p0 + lane;
        const int32_t n = p < end ? count[p] : 0;
        const unsigned long long m = __ballot(n > 0);
        if (kWrite && n > 0)
            out[base + __popcll(m & ((1ull << lane) - 1ull))] =
                a.bucket[first[p] + hccontig::pick_index(a.seed, uint64_t(lw), uint64_t(p), uint32_t(n), a.pick_mode)];
        base += __popcll(m);
    }
    if (!kWrite && lane == 0) a.n_picked[w] = base;
}

static unsigned blocks_of(int64_t n, int per) { return unsigned((n + per - 1) / per); }

hipError_t launch_resolve(const GenomeArgs& a, hipStream_t st)
{
    if (a.n_records <= 0) return hipSuccess;
    hipLaunchKernelGGL(genome_resolve_kernel, dim3(blocks_of(a.n_records, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_place(const GenomeArgs& a, hipStream_t st)
{
    if (a.n_records <= 0) return hipSuccess;
    hipLaunchKernelGGL(genome_place_kernel, dim3(blocks_of(a.n_records, 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_scatter(const GenomeArgs& a, hipStream_t st)
{
    if (a.n_records <= 0) return hipSuccess;
    hipLaunchKernelGGL(genome_scatter_kernel, dim3(blocks_of(a.n_records, 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_sort(const GenomeArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(genome_sort_kernel, dim3(blocks_of(a.total_len, 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pick_count(const GenomeArgs& a, hipStream_t st)
{
    if (a.n_asked <= 0) return hipSuccess;
    hipLaunchKernelGGL(genome_pick_kernel<false>, dim3(blocks_of(a.n_asked, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0,
                       st, a);
    return hipGetLastError();
}

hipError_t launch_pick_write(const GenomeArgs& a, hipStream_t st)
{
    if (a.n_asked <= 0) return hipSuccess;
    hipLaunchKernelGGL(genome_pick_kernel<true>, dim3(blocks_of(a.n_asked, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0,
                       st, a);
    return hipGetLastError();
}

}  // namespace hcgenome
