// Region caller hand-offs on the device (gfx950, wave64).
//
// region_runs_kernel     the aligner's CIGAR elements (traceback order) -> the
//                        genotyper's PlanRun list with window / haplotype start
//                        positions (gt_engine.cpp's parse_cigar, without the text)
// region_finish_*        normalize_likelihoods_and_filter_poorly_modeled_reads
//                        (pairhmm/intel_pairhmm.hpp:24-46) per read row, then the
//                        kept rows and read intervals written compact and in order
//
// Built with -ffp-contract=off like the file's neighbours: the cap is one
// double add, the threshold one multiply, a ceil, a min and a second multiply,
// in the reference's order, so the bits are the host loop's.
#include "region_kernels.hpp"

#include <cmath>

namespace hcregion {
namespace {

constexpr int kWavesPerBlock = 4;

__device__ inline int wave_inclusive(int v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void region_runs_kernel(RunsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (p >= a.n) return;
    const hcsw::SwPair P = a.pairs[p];
    const int n = a.n_elems[p];
    // The all-match shortcut leaves one element in the pair's slot and nothing
    // in its scratch (sw_trace_kernel); everything else is read from the scratch,
    // which holds every element however many there are.
    const bool shortcut = a.res[p].shortcut != 0;
    const uint32_t* el = a.elems + P.el_off;
    hcgt::PlanRun* out = a.runs + P.el_off;
    uint32_t err = 0;
    if (n < 1 || n >= kMaxRuns || n > P.n1 + P.n2 + 3 || (shortcut && n != 1)) err |= kErrCount;
    int ref = a.offsets[p], hap = 0;
    if (ref < 0 || ref > P.n1) err |= kErrRefEnd;
    if (!err) {
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            int len = 0, op = -1, dr = 0, dh = 0;
            if (i < n) {
                const uint32_t v = shortcut ? uint32_t(a.slots[int64_t(p) * hcsw::kSlotElems]) : el[n - 1 - i];
                len = int(v >> 4);
                const int sop = int(v & 15u);
                op = sop == hcsw::kOpM ? hcgt::kOpM
                     : sop == hcsw::kOpI ? hcgt::kOpI
                     : sop == hcsw::kOpD ? hcgt::kOpD
                     : sop == hcsw::kOpS ? hcgt::kOpS
                                         : -1;
                if (op < 0 || len < 1) err |= kErrOp;
                dr = (op == hcgt::kOpM || op == hcgt::kOpD) ? len : 0;
                dh = (op == hcgt::kOpM || op == hcgt::kOpI || op == hcgt::kOpS) ? len : 0;
            }
            const int ir = wave_inclusive(dr, lane), ih = wave_inclusive(dh, lane);
            if (i < n) out[i] = hcgt::PlanRun{len, op < 0 ? 0 : op, ref + ir - dr, hap + ih - dh};
            ref += __shfl(ir, 63);
            hap += __shfl(ih, 63);
        }
        if (hap != P.n2) err |= kErrHapLen;
        if (ref > P.n1) err |= kErrRefEnd;
    }
    // Any lane's finding is the wave's.
    for (int d = 32; d >= 1; d >>= 1) err |= uint32_t(__shfl_xor(int(err), d));
    if (lane == 0) {
        // A haplotype in error gets no runs: the events kernel behind this one
        // then touches nothing of it, and the host fails the call.
        hcgt::PlanHap& H = a.haps[a.pair_hap[p]];
        H.run_off = int32_t(P.el_off);
        H.n_runs = err ? 0 : n;
        if (err) atomicOr(a.err, err);
    }
}

// Region of global read g: the last region whose read_off is <= g (regions
// without reads share their successor's offset, so the last one owns the read).
__device__ inline int region_of(const hcgt::PlanRegion* regions, int n_regions, int g)
{
    int lo = 0, hi = n_regions - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (regions[mid].read_off <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One wave per read row: best, cap, keep flag. n_haps <= 128: two values per lane.
__global__ __launch_bounds__(64 * kWavesPerBlock) void region_finish_rows_kernel(FinishArgs a)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= a.n_reads) return;
    const hcgt::PlanRegion R = a.regions[region_of(a.regions, a.n_regions, g)];
    const int nh = R.n_haps;
    double* row = a.L + R.L_off + int64_t(g - R.read_off) * nh;
    const double ninf = -INFINITY;
    double v0 = lane < nh ? row[lane] : ninf;
    double v1 = lane + 64 < nh ? row[lane + 64] : ninf;
    double best = v0 < v1 ? v1 : v0;
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(best, d);
        best = best < o ? o : best;
    }
    const double cap = best + -4.5;
    if (lane < nh && v0 < cap) row[lane] = cap;
    if (lane + 64 < nh && v1 < cap) row[lane + 64] = cap;
    if (lane == 0) {
        const double thr = fmin(2.0, ceil(double(a.read_len[g]) * 0.02)) * -4.0;
        a.keep[g] = !(best < thr);
    }
}

// One wave per region: keep flags -> ascending destinations, 64 reads per step;
// the kept reads' intervals move to their destinations, n_reads becomes the count.
__global__ __launch_bounds__(64) void region_finish_compact_kernel(FinishArgs a)
{
    const int lane = threadIdx.x;
    const int r = blockIdx.x;
    const hcgt::PlanRegion R = a.regions[r];
    int kept = 0;
    for (int r0 = 0; r0 < R.n_reads; r0 += 64) {
        const int i = r0 + lane;
        const bool on = i < R.n_reads && a.keep[R.read_off + i] != 0;
        const uint64_t m = __ballot(on);
        if (i < R.n_reads) {
            const int d = on ? kept + __popcll(m & ((1ull << lane) - 1ull)) : -1;
            a.dest[R.read_off + i] = d;
            if (on) {
                a.begin_out[R.read_off + d] = a.read_begin[R.read_off + i];
                a.end_out[R.read_off + d] = a.read_end[R.read_off + i];
            }
        }
        kept += __popcll(m);
    }
    if (lane == 0) {
        a.regions[r].n_reads = kept;
        a.n_kept[r] = kept;
    }
}

// One wave per read row: a kept row goes to its destination in the out-of-place matrix.
__global__ __launch_bounds__(64 * kWavesPerBlock) void region_finish_rows_out_kernel(FinishArgs a)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (g >= a.n_reads) return;
    const int d = a.dest[g];
    if (d < 0) return;
    // read_off, L_off and n_haps are unchanged by the compaction; n_reads is not read here.
    const hcgt::PlanRegion R = a.regions[region_of(a.regions, a.n_regions, g)];
    const int nh = R.n_haps;
    const double* row = a.L + R.L_off + int64_t(g - R.read_off) * nh;
    double* to = a.L_out + R.L_off + int64_t(d) * nh;
    for (int h = lane; h < nh; h += 64) to[h] = row[h];
}

}  // namespace

hipError_t launch_runs(const RunsArgs& a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    const unsigned blocks = unsigned((a.n + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(region_runs_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_finish(const FinishArgs& a, hipStream_t s)
{
    if (a.n_regions <= 0) return hipSuccess;
    const unsigned blocks = unsigned((a.n_reads + kWavesPerBlock - 1) / kWavesPerBlock);
    if (a.n_reads > 0) hipLaunchKernelGGL(region_finish_rows_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), 0, s, a);
    hipLaunchKernelGGL(region_finish_compact_kernel, dim3(unsigned(a.n_regions)), dim3(64), 0, s, a);
    if (a.n_reads > 0)
        hipLaunchKernelGGL(region_finish_rows_out_kernel, dim3(blocks), dim3(64 * kWavesPerBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace hcregion
