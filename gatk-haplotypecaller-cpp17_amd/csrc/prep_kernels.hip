// Read preparation on the device (include/hc_prep.h).
//
// prep_kernel: one wave per window, four waves per workgroup, 64 reads per
// round. Each lane derives its read's record (prep_body.hpp) and stores it; the
// wave compacts the kept reads' indices in input order with a ballot, the
// popcount of the lower lanes and a base carried from round to round. n_kept is
// the last base, the kept-length sum a wave reduction per round. All integer;
// bounded by launch and copy latency, not by throughput.
#include "prep_kernels.hpp"

namespace hcprep {

__global__ __launch_bounds__(64 * kPrepWavesPerBlock) void prep_kernel(PrepArgs a)
{
    const int lane = int(threadIdx.x) & 63;
    const int w = int(blockIdx.x) * kPrepWavesPerBlock + (int(threadIdx.x) >> 6);
    if (w >= a.n_windows) return;   // wave-uniform
    const PrepWindow win = a.windows[w];
    int32_t base = 0;
    int64_t bases = 0;
    for (int32_t first = 0; first < win.n_reads; first += 64) {
        const int32_t j = first + lane;
        bool keep = false;
        int32_t len = 0;
        if (j < win.n_reads) {
            const int64_t g = win.first_read + j;
            const PrepRead r = a.reads[g];
            hc_prep_record o;
            const int32_t e = prep_one(r, a.words + r.cigar_off, uint64_t(win.padded_begin), uint64_t(win.padded_end), o);
            if (e != kErrNone) atomicMin(a.err, static_cast<unsigned long long>(g) * 8ull + static_cast<unsigned long long>(e));
            a.records[g] = o;
            keep = o.keep != 0;
            len = keep ? o.length : 0;
        }
        const unsigned long long m = __ballot(keep);
        if (keep) a.kept[win.first_read + base + __popcll(m & ((1ull << lane) - 1ull))] = j;
        base += __popcll(m);
        for (int d = 32; d >= 1; d >>= 1) len += __shfl_xor(len, d, 64);
        bases += len;
    }
    if (lane == 0) {
        a.n_kept[w] = base;
        a.kept_bases[w] = bases;
    }
}

hipError_t launch_prep(const PrepArgs& a, hipStream_t st)
{
    if (a.n_windows <= 0) return hipSuccess;
    const unsigned blocks = unsigned((a.n_windows + kPrepWavesPerBlock - 1) / kPrepWavesPerBlock);
    hipLaunchKernelGGL(prep_kernel, dim3(blocks), dim3(64 * kPrepWavesPerBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace hcprep
