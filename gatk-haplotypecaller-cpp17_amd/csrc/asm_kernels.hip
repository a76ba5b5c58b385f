// Assembler kernels (include/hc_asm.h), gfx950.
//
//   asm_segments_kernel   one wave per sequence (a window or a read): a ballot
//                         over the usable flags gives, per base, the length of
//                         the usable run from there on and the run's start, so
//                         "position i starts a k-mer of attempt k" is rem[i] >= k
//                         and "i heads a segment" is seg_start[i] == i.
//   asm_graph_kernel      one workgroup per region, all attempts
//                         (asm_graph_body.hpp). Workgroups never wait on each other.
#include "asm_kernels.hpp"

#define ASMX_FN __device__
#define ASMX_TID int(threadIdx.x)
#define ASMX_NT int(blockDim.x)
#define ASMX_SYNC() __syncthreads()
#define ASMX_CAS(p, c, v) atomicCAS((p), (c), (v))
#define ASMX_MIN(p, v) atomicMin((p), (v))
#define ASMX_ADD(p, v) atomicAdd((p), (v))
#define ASMX_OR(p, v) atomicOr((p), (v))
#define ASMX_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define ASMX_CLOCK() wall_clock64()
#include "asm_graph_body.hpp"

namespace hcasm {

static_assert(sizeof(hc_asm_edge) == 20, "hc_asm_edge layout");

__global__ __launch_bounds__(256) void asm_segments_kernel(AsmArgs a)
{
    const int lane = int(threadIdx.x) & 63;
    const long long wave = (static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    if (wave >= a.n_seqs) return;   // uniform over the wave
    const AsmSeq s = a.seqs[wave];
    int32_t* rem = a.rem + s.off;
    int32_t* seg = a.seg_start + s.off;
    if (s.is_ref) {   // the window is one run whatever its bytes
        for (int32_t i = lane; i < s.len; i += 64) {
            rem[i] = s.len - i;
            seg[i] = s.rel;
        }
        return;
    }
    const uint8_t* b = a.bases + s.off;
    const uint8_t* q = a.quals + s.off;
    const int32_t n_chunks = (s.len + 63) / 64;
    // right to left: usable bases from here to the end of the run
    int32_t carry = 0;
    for (int32_t c = n_chunks - 1; c >= 0; --c) {
        const int32_t i = c * 64 + lane;
        const bool u = i < s.len && asm_usable(b[i], q[i]);
        const unsigned long long m = __ballot(u);
        const int32_t r = u ? asm_run_right(m, lane, carry) : 0;
        if (i < s.len) rem[i] = r;
        carry = __shfl(r, 0);
    }
    // left to right: usable bases from the start of the run to here
    carry = 0;
    for (int32_t c = 0; c < n_chunks; ++c) {
        const int32_t i = c * 64 + lane;
        const bool u = i < s.len && asm_usable(b[i], q[i]);
        const unsigned long long m = __ballot(u);
        const int32_t d = u ? asm_run_left(m, lane, carry) : 0;
        if (i < s.len) seg[i] = s.rel + i - (u ? d - 1 : 0);
        carry = __shfl(d, 63);
    }
}

__global__ __launch_bounds__(kAsmThreads) void asm_graph_kernel(AsmArgs a)
{
    __shared__ AsmShared sh;
    const AsmSlot w = asm_carve(a.work + size_t(blockIdx.x) * a.slot_bytes, a.max_bases, a.max_hash, a.max_cap);
    for (int32_t r = int32_t(blockIdx.x); r < a.n_regions; r += int32_t(gridDim.x)) asm_region_graph(a, r, w, &sh);
}

hipError_t launch_asm_segments(const AsmArgs& a, hipStream_t st)
{
    if (a.n_seqs == 0) return hipSuccess;
    const unsigned blocks = unsigned((a.n_seqs + 3) / 4);
    hipLaunchKernelGGL(asm_segments_kernel, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_asm_graph(const AsmArgs& a, int n_slots, hipStream_t st)
{
    if (a.n_regions == 0) return hipSuccess;
    hipLaunchKernelGGL(asm_graph_kernel, dim3(unsigned(n_slots)), dim3(kAsmThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace hcasm
