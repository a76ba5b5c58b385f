// Interval kernels (include/hc_intervals.h), gfx950. All integer, plain vector
// stores; every index is below the count its launch is sized by.
//
//   interval_ask_kernel      one thread per genome-wide window: its contig by the
//                            binary search of genome_pick_kernel, its own bases cut
//                            at the contig's end, asked[w] by a binary search in the
//                            contig's slice of the merged intervals.
//   interval_scope_kernel    one thread per record: placed, and one of the up to
//                            three windows that hold POS - 1 is asked.
//   (scans of the flags: sam_scan_kernel)
//   interval_compact_kernel  one thread per flag: element i with flag[i] set goes
//                            to list[first[i]], so the list ascends and two runs
//                            give the same bytes. first[i] < first[n] <= n.
#include "interval_kernels.hpp"

#include "sam_kernels.hpp"

namespace hcgenome {

__global__ __launch_bounds__(256) void interval_ask_kernel(IntervalArgs a)
{
    const int64_t w = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (w >= a.g.n_windows) return;
    const int32_t c = genome_contig_of_window(a.g.win_off, a.g.n_contigs, w);
    a.asked[w] = interval_window_asked(a.set, c, w - a.g.win_off[c], a.g.region, a.g.ref_len[c]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void interval_scope_kernel(IntervalArgs a)
{
    const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (k >= a.g.n_records) return;
    a.scope[k] = interval_in_scope(a.g.contig_of[k], a.g.records[k].pos, a.g.ref_len, a.g.win_off, a.g.region, a.g.padding,
                                   a.asked)
                     ? 1
                     : 0;
}

__global__ __launch_bounds__(256) void interval_compact_kernel(const int32_t* flag, const int64_t* first, int64_t n, int32_t* list)
{
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) list[first[i]] = int32_t(i);
}

static unsigned blocks_of(int64_t n, int per) { return unsigned((n + per - 1) / per); }

hipError_t launch_interval_ask(const IntervalArgs& a, hipStream_t st)
{
    const int64_t n = a.g.n_windows;   // at least one: every contig has a window
    hipLaunchKernelGGL(interval_ask_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, a);
    if (hipError_t e = hcsam::launch_scan(a.asked, n, a.asked_first, a.scan_work, st)) return e;
    hipLaunchKernelGGL(interval_compact_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, a.asked, a.asked_first, n, a.asked_list);
    return hipGetLastError();
}

hipError_t launch_interval_scope(const IntervalArgs& a, hipStream_t st)
{
    const int64_t n = a.g.n_records;
    if (n > 0) hipLaunchKernelGGL(interval_scope_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, a);
    if (hipError_t e = hcsam::launch_scan(a.scope, n, a.scope_first, a.scan_work, st)) return e;   // no record: scope_first[0] = 0
    if (n > 0)
        hipLaunchKernelGGL(interval_compact_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, st, a.scope, a.scope_first, n,
                           a.scoped_list);
    return hipGetLastError();
}

}  // namespace hcgenome
