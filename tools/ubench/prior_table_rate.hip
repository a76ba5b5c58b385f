// Micro-benchmark: the fp32 EQ cell with its priors by the carry select
// (seg_common.hpp cell / prior_next) against the pair table (cell_tab / ptab),
// registers and LDS only, in workgroups of one wave (the seg kernel's until
// round 12; its workgroups of four waves are in the byte form's rows below); every
// lane sweeps `rows` rows of one block of BC columns with a random quality and
// random window words per lane and row, the next row's constants fetched from
// LDS one row ahead as the step loop does. Three waves per SIMD are what the
// registers allow (__launch_bounds__, 8 KB of LDS as the seg kernel's wave);
// for two, 20 KB of dynamic LDS a wave leave 8 waves on a CU's 160 KB.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize \
//         -fgpu-flush-denormals-to-zero prior_table_rate.hip -o prior_table_rate
//   ./prior_table_rate            one JSON line per (form, BC, waves per SIMD)
// Rows of the quad table in its byte form, as the kernel runs it (seg_common.hpp
// fill_shared_tabs, quad_base2, win_byte, quad_read, cell_tab): workgroups of
// four waves that share the table of 64 quality rows, each wave with a spread
// window of random columns per (read code, lane), a row drawing its read code
// and its quality from 31 consecutive values as S2's; beside it the pair table
// at those qualities in the same workgroups. (The word form of round 12, a
// shift and a v_and_or_b32 per group on a packed window, is recorded in
// profiles/quad128_ubench.jsonl, and round 11's two-read forms in
// profiles/quad_table_ubench.jsonl; the kernel no longer has them.)
// LDS bank conflicts: the same binary under a counters-only profiler run
// (SQ_INSTS_LDS, SQ_LDS_BANK_CONFLICT, SQ_LDS_IDX_ACTIVE per kernel name).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "../../gatk-haplotypecaller-cpp17_amd/csrc/seg_common.hpp"

namespace hcphmm {
namespace seg {

__device__ __forceinline__ uint32_t lcg(uint32_t r) { return r * 1664525u + 1013904223u; }
// Window words and quality of a row from its random word (the low LCG bits are poor).
__device__ __forceinline__ uint2 row_words(uint32_t r) { return make_uint2(r ^ (r >> 15), (r * 0x85ebca6bu) ^ (r >> 7)); }
__device__ __forceinline__ uint32_t row_qual(uint32_t r) { return (r >> 12) & 127u; }

enum Form { kPairWin = 0, kByte };
constexpr int kWinLo = 43, kWinSpan = 31;   // S2's qualities
constexpr int kWPB = 4;                     // waves per workgroup (lane_kernel.hip HC_SEG_WPB)
__device__ __forceinline__ uint32_t win_qual(uint32_t r) { return kWinLo + ((((r >> 12) & 1023u) * kWinSpan) >> 10); }
__device__ __forceinline__ uint32_t win_code(uint32_t r) { return ((r >> 22) * 5u) >> 10; }   // 0 .. 4

template <int BC, int FORM>
__global__ __launch_bounds__(64 * kWPB, 3) void quad_kernel(float* __restrict__ out, const float* __restrict__ lut,
                                                            int rows, uint32_t seed)
{
    __shared__ __attribute__((aligned(256))) float qtab[kQuadLen];
    __shared__ __attribute__((aligned(16))) float ptab[kPtabLen];
    __shared__ __attribute__((aligned(256))) uint2 mtab[kWPB][kWindowBytes / 8];
    const int lane = __lane_id();
    fill_shared_tabs(ptab, qtab, lut, int(threadIdx.x), 64 * kWPB);
    uint32_t r = lcg(seed ^ ((blockIdx.x * (64u * kWPB) + threadIdx.x) * 0x9e3779b9u));
    uint2* mt = mtab[threadIdx.x >> 6];
    constexpr bool Q = FORM == kByte;
    // The lane's window of every read code: random columns, in the form's layout.
    for (int c = 0; c < 5; ++c) {
        r = lcg(r);
        const uint2 m = row_words(r);
        if constexpr (Q) {
            uint32_t* d = reinterpret_cast<uint32_t*>(mt) + spread_slot_off(c, lane) / 4;
            d[spread_group_off(0) / 4] = spread_nibbles(m.x >> 16);
            d[spread_group_off(4) / 4] = spread_nibbles(m.x & 0xffffu);
            d[spread_group_off(8) / 4] = spread_nibbles(m.y >> 16);
            d[spread_group_off(12) / 4] = spread_nibbles(m.y & 0xffffu);
        } else {
            mt[c * 64 + lane] = m;
        }
    }
    __syncthreads();
    float Tt[BC], X[BC];
#pragma unroll
    for (int j = 0; j < BC; ++j) {
        Tt[j] = 1.f + float(lane + j) * 1e-3f;
        X[j] = 0.f;
    }
    RowConst<float> k;
    k.my = k.mx = lut[kOffPh2pr + 45];
    k.yy = k.xx = lut[kOffPh2pr + 10];
    k.mm = lut[kOffGapm + 42];
    k.g = lut[kOffGapm + 10];
    k.pm = k.px = 0.f;
    k.rc = 0;
    const uint32_t tab_lds = lds_addr(Q ? qtab : ptab), win_lds = lds_addr(mt);
    TabRow<Q> tr{};
    TabEnt<Q> pr0{};
    // The coming row's table base, window slot and first entry (the step's end in run_seg).
    auto next_row = [&](uint32_t rw) {
        tr.base = tab_row<Q>(tab_lds, win_qual(rw));
        if constexpr (Q) {
            tr.slot = win_lds + spread_slot_off(win_code(rw), lane);
            pr0 = quad_read(tr.base, win_byte<0>(tr.slot));
            tr.byte = win_byte<1>(tr.slot);
        } else {
            tr.m = mt[win_code(rw) * 64 + lane];
            pr0 = ptab_pair<0>(tr.base, tr.m);
        }
    };
    next_row(r);
    float sumM = 0.f, sumX = 0.f, y_in = 0.f, t_diag = 1.f;
    for (int i = 0; i < rows; ++i) {
        r = lcg(r);
        float Ml = 0.f, Yl = y_in;
        constexpr int D = kPtabAhead;
        TabEnt<Q> pr[D];
        pr[0] = pr0;
        if constexpr (Q) {
            pr[1] = quad_read(tr.base, tr.byte);
            tr.byte = win_byte<2>(tr.slot);
        } else {
            pr[1] = ptab_pair<1>(tr.base, tr.m);
        }
        cell_tab<BC, 0, false, D, Q>(Tt, X, t_diag * pr0.x, Ml, Yl, pr, tr, k, sumM, sumX);
        next_row(r);
        y_in = y_next<true>(Ml, Yl, k.my, k.yy);
        t_diag = Tt[BC - 1];
    }
    float acc = y_in;
#pragma unroll
    for (int j = 0; j < BC; ++j) acc += Tt[j] + X[j];
    out[blockIdx.x * (64 * kWPB) + threadIdx.x] = acc;
}

template <int BC, bool TAB>
__global__ __launch_bounds__(64, 3) void rate_kernel(float* __restrict__ out, const float* __restrict__ lut, int rows,
                                                     uint32_t seed)
{
    extern __shared__ __attribute__((aligned(32))) float lds[];   // ptab or slut; the rest sets the occupancy
    const int lane = threadIdx.x;
    if constexpr (TAB)
        fill_ptab(lds, lut, lane, 64);
    else
        for (int t = lane; t < kSlutLen; t += 64) lds[t] = lut[t];
    __builtin_amdgcn_wave_barrier();
    float Tt[BC], X[BC];
#pragma unroll
    for (int j = 0; j < BC; ++j) {
        Tt[j] = 1.f + float(lane + j) * 1e-3f;
        X[j] = 0.f;
    }
    RowConst<float> k;
    k.my = k.mx = lut[kOffPh2pr + 45];
    k.yy = k.xx = lut[kOffPh2pr + 10];
    k.mm = lut[kOffGapm + 42];
    k.g = lut[kOffGapm + 10];
    k.pm = k.px = 0.f;
    k.rc = 0;
    uint32_t r = lcg(seed ^ ((blockIdx.x * 64u + lane) * 0x9e3779b9u));
    uint2 mrow = row_words(r);
    const uint32_t ptab_lds = lds_addr(lds);
    TabRow<false> tr{ptab_row(ptab_lds, row_qual(r)), mrow};
    float2 pr0 = make_float2(0.f, 0.f);
    float pm = 0.f, px = 0.f;
    if constexpr (TAB) {
        pr0 = ptab_pair<0>(tr.base, tr.m);
    } else {
        pm = lds[kOffPm + row_qual(r)];
        px = lds[kOffPx + row_qual(r)];
    }
    float sumM = 0.f, sumX = 0.f, y_in = 0.f, t_diag = 1.f;
    for (int i = 0; i < rows; ++i) {
        r = lcg(r);
        const uint2 m_n = row_words(r);
        float pm_n = 0.f, px_n = 0.f;
        if constexpr (!TAB) {
            pm_n = lds[kOffPm + row_qual(r)];
            px_n = lds[kOffPx + row_qual(r)];
        }
        float Ml = 0.f, Yl = y_in;
        if constexpr (TAB) {
            constexpr int D = kPtabAhead, NP = BC / 2;
            float2 pr[D];
            pr[0] = pr0;
            static_assert(D == 2 && NP > D, "a ring of two pairs");
            pr[1] = ptab_pair<1>(tr.base, tr.m);
            const float M0 = t_diag * pr0.x;
            cell_tab<BC, 0, false, D, false>(Tt, X, M0, Ml, Yl, pr, tr, k, sumM, sumX);
            tr.m = m_n;
            tr.base = ptab_row(ptab_lds, row_qual(r));
            pr0 = ptab_pair<0>(tr.base, tr.m);
        } else {
            const float M0 = t_diag * prior_next(mrow.x, pm, px);
            cell<float, BC, 0, BC, false, true>(Tt, X, M0, Ml, Yl, mrow.x, mrow.y, pm, px, k, 0, sumM, sumX);
            pm = pm_n;
            px = px_n;
            mrow = m_n;
        }
        y_in = y_next<true>(Ml, Yl, k.my, k.yy);
        t_diag = Tt[BC - 1];
    }
    float acc = y_in;
#pragma unroll
    for (int j = 0; j < BC; ++j) acc += Tt[j] + X[j];
    out[blockIdx.x * 64 + lane] = acc;
}

template <int BC, bool TAB>
void run(float* out, const float* lut, int cus, int wps, int rows)
{
    const int grid = cus * 4 * wps;                       // one round: every wave resident from the start
    const size_t lds = wps == 3 ? 8 * 1024 : 20 * 1024;    // 12 (by registers) or 8 workgroups of one wave per CU
    hipEvent_t a, e;
    hipEventCreate(&a);
    hipEventCreate(&e);
    rate_kernel<BC, TAB><<<grid, 64, lds>>>(out, lut, rows, 1u);
    const int reps = 3;
    hipEventRecord(a);
    for (int rep = 0; rep < reps; ++rep) rate_kernel<BC, TAB><<<grid, 64, lds>>>(out, lut, rows, 7u + rep);
    hipEventRecord(e);
    hipEventSynchronize(e);
    float ms = 0.f;
    hipEventElapsedTime(&ms, a, e);
    const hipError_t err = hipGetLastError();
    const double cells = double(grid) * 64 * BC * rows * reps;
    printf("{\"form\": \"%s\", \"bc\": %d, \"waves_per_simd\": %d, \"rows\": %d, \"ms_per_launch\": %.4f, "
           "\"gcells_per_s\": %.1f, \"status\": \"%s\"}\n",
           TAB ? "table" : "select", BC, wps, rows, ms / reps, cells / (ms * 1e-3) / 1e9, hipGetErrorName(err));
    fflush(stdout);
    hipEventDestroy(a);
    hipEventDestroy(e);
}

// The byte form's workgroups of four waves: the seg kernel's LDS (three
// workgroups per CU, 12 waves) or 16 KB more (two workgroups, 8 waves).
template <int BC, int FORM>
void run_quad(float* out, const float* lut, int cus, int wps, int rows)
{
    const int grid = cus * wps;   // one round: every wave resident from the start
    const size_t lds = wps == 3 ? 0 : 16 * 1024;
    hipEvent_t a, e;
    hipEventCreate(&a);
    hipEventCreate(&e);
    quad_kernel<BC, FORM><<<grid, 64 * kWPB, lds>>>(out, lut, rows, 1u);
    const int reps = 3;
    hipEventRecord(a);
    for (int rep = 0; rep < reps; ++rep) quad_kernel<BC, FORM><<<grid, 64 * kWPB, lds>>>(out, lut, rows, 7u + rep);
    hipEventRecord(e);
    hipEventSynchronize(e);
    float ms = 0.f;
    hipEventElapsedTime(&ms, a, e);
    const hipError_t err = hipGetLastError();
    const double cells = double(grid) * kWPB * 64 * BC * rows * reps;
    static const char* names[] = {"pair table, 31 qualities, workgroups of 4 waves",
                                  "quad table, byte form (ds_read_u8 + v_xor_b32 + ds_read_b128)"};
    printf("{\"form\": \"%s\", \"bc\": %d, \"waves_per_simd\": %d, \"rows\": %d, \"ms_per_launch\": %.4f, "
           "\"gcells_per_s\": %.1f, \"status\": \"%s\"}\n",
           names[FORM], BC, wps, rows, ms / reps, cells / (ms * 1e-3) / 1e9, hipGetErrorName(err));
    fflush(stdout);
    hipEventDestroy(a);
    hipEventDestroy(e);
}

}  // namespace seg
}  // namespace hcphmm

int main()
{
    using namespace hcphmm;
    using namespace hcphmm::seg;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    const int cus = prop.multiProcessorCount;
    std::vector<float> h(kOffMM, 0.f);
    for (int q = 0; q < kQuals; ++q) {
        const float p = std::pow(10.f, -float(q) / 10.f);
        h[kOffPh2pr + q] = p;
        h[kOffPm + q] = 1.f - p;
        h[kOffPx + q] = p / 3.f;
        h[kOffGapm + q] = 1.f - p;
    }
    float *lut, *out;
    if (hipMalloc(&lut, h.size() * sizeof(float)) != hipSuccess) return 1;
    if (hipMalloc(&out, size_t(cus) * 4 * 3 * 64 * sizeof(float)) != hipSuccess) return 1;
    hipMemcpy(lut, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
    const int rows = 2048;
    {   // what the runtime gives the seg kernel's workgroup of four waves with its static LDS
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, quad_kernel<64, kByte>, 64 * kWPB, 0) != hipSuccess) return 1;
        printf("{\"what\": \"resident workgroups of %d waves per CU (quad_kernel<64, byte form>, %d B of static LDS)\", "
               "\"value\": %d, \"waves_per_cu\": %d}\n",
               kWPB, int((kQuadLen + kPtabLen) * 4 + kWPB * kWindowBytes), nb, nb * kWPB);
    }
    for (int wps : {3, 2}) {
        run<64, false>(out, lut, cus, wps, rows);
        run<64, true>(out, lut, cus, wps, rows);
        run<48, false>(out, lut, cus, wps, rows);
        run<48, true>(out, lut, cus, wps, rows);
        run<16, false>(out, lut, cus, wps, rows);
        run<16, true>(out, lut, cus, wps, rows);
    }
    for (int wps : {3, 2}) {
        run_quad<64, kPairWin>(out, lut, cus, wps, rows);
        run_quad<64, kByte>(out, lut, cus, wps, rows);
        run_quad<48, kPairWin>(out, lut, cus, wps, rows);
        run_quad<48, kByte>(out, lut, cus, wps, rows);
    }
    hipFree(lut);
    hipFree(out);
    return 0;
}
