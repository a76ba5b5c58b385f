// Contig caller kernels (include/hc_contig.h), gfx950. All integer, plain vector stores.
//
//   contig_place_kernel    one lane per record: the unplaced and the defective
//                          reads lower the error word, the placed ones count
//                          into their begin position.
//   (scan of the counts: sam_scan_kernel)
//   contig_scatter_kernel  one lane per placed record: into its position's
//                          bucket, in the order of arrival.
//   contig_sort_kernel     one lane per position: its bucket by record index,
//                          which is file order, whatever the arrival was. An
//                          insertion sort: linear when the arrival was in order,
//                          quadratic at worst, so a bucket holds at most
//                          HC_CONTIG_MAX_READS_PER_POSITION reads (an error beyond).
//   contig_pick_kernel     one wave per window, 64 positions of the padded
//                          interval per round: a ballot over "holds reads", the
//                          popcount of the lower lanes and a base carried from
//                          round to round compact the picks in ascending
//                          position. <false> counts, <true> writes at the scanned base.
#include "contig_kernels.hpp"

namespace hccontig {

__device__ inline bool placed(const hc_sam_record& r, int64_t ref_len) { return r.pos != 0u && int64_t(r.pos - 1u) < ref_len; }

__global__ __launch_bounds__(256) void contig_place_kernel(ContigArgs a)
{
    const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (k >= a.n_records) return;
    const hc_sam_record r = a.records[k];
    const unsigned long long line = static_cast<unsigned long long>(a.line_no[k]);
    if (!placed(r, a.ref_len)) {
        if (!a.skip_unplaced) atomicMin(a.err, line * 16ull + kErrUnplaced);
        return;
    }
    const bool filtered = r.mapq < HC_PREP_MIN_MAPQ || (r.flag & 0x500) || !r.mate_same_contig;
    if (!filtered && r.defect) atomicMin(a.err, line * 16ull + kErrDefect);
    atomicAdd(a.count + (r.pos - 1u), 1);
}

__global__ __launch_bounds__(256) void contig_scatter_kernel(ContigArgs a)
{
    const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (k >= a.n_records) return;
    const hc_sam_record r = a.records[k];
    if (!placed(r, a.ref_len)) return;
    const int64_t b = int64_t(r.pos - 1u);
    a.bucket[a.first[b] + atomicAdd(a.cursor + b, 1)] = int32_t(k);
}

__global__ __launch_bounds__(256) void contig_sort_kernel(ContigArgs a)
{
    const int64_t p = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (p >= a.ref_len) return;
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
__global__ __launch_bounds__(64 * kWavesPerBlock) void contig_pick_kernel(ContigArgs a)
{
    const int lane = int(threadIdx.x) & 63;
    const int64_t w = int64_t(blockIdx.x) * kWavesPerBlock + (int(threadIdx.x) >> 6);
    if (w >= a.n_windows) return;   // wave-uniform
    const int64_t origin = w * a.region;
    const int64_t begin = w == 0 ? 0 : origin - a.padding;
    int64_t end = origin + a.region + a.padding;
    if (end > a.ref_len) end = a.ref_len;   // positions at and past the contig's end hold no reads
    int32_t* out = kWrite ? a.picked + a.win_first[w] : nullptr;
    int32_t base = 0;
    for (int64_t p0 = begin; p0 < end; p0 += 64) {
        const int64_t p = p0 + lane;
        const int32_t n = p < end ? a.count[p] : 0;
        const unsigned long long m = __ballot(n > 0);
        if (kWrite && n > 0)
            out[base + __popcll(m & ((1ull << lane) - 1ull))] =
                a.bucket[a.first[p] + pick_index(a.seed, uint64_t(w), uint64_t(p), uint32_t(n), a.pick_mode)];
        base += __popcll(m);
    }
    if (!kWrite && lane == 0) a.n_picked[w] = base;
}

static unsigned blocks_of(int64_t n, int per) { return unsigned((n + per - 1) / per); }

hipError_t launch_place(const ContigArgs& a, hipStream_t st)
{
    if (a.n_records <= 0) return hipSuccess;
    hipLaunchKernelGGL(contig_place_kernel, dim3(blocks_of(a.n_records, 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_scatter(const ContigArgs& a, hipStream_t st)
{
    if (a.n_records <= 0) return hipSuccess;
    hipLaunchKernelGGL(contig_scatter_kernel, dim3(blocks_of(a.n_records, 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_sort(const ContigArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(contig_sort_kernel, dim3(blocks_of(a.ref_len, 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pick_count(const ContigArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(contig_pick_kernel<false>, dim3(blocks_of(a.n_windows, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0,
                       st, a);
    return hipGetLastError();
}

hipError_t launch_pick_write(const ContigArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(contig_pick_kernel<true>, dim3(blocks_of(a.n_windows, kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0,
                       st, a);
    return hipGetLastError();
}

}  // namespace hccontig
